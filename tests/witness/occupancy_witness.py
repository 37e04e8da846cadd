"""Witness of the occupancy grid and the saved map (rgrid_occupancy_grid / rgrid_batch_occupancy_* of include/rgrid.h,
GridFrontEnd.OccupancyGrid, ScanMatchFleet.occupancy_grids, MapBuilder.OccupancyGrid / SaveMap), pure numpy.

It restates what the reference's node does with a submap texture -- io::FillSubmapSlice + io::PaintSubmapSlices
(src/io/submap_painter.cc:44-164), Node::CreateOccupancyGridMsg, Node::WritePgm, Node::WriteYaml (src/ros_node.cc:865-945) -- as
the closed form that tests/test_occupancy_cpu.py pins against libcairo itself (tests/golden/occupancy_cairo.npz).  It is written
from those formulas, not from the product's host code.

A texture is ``(pairs uint8 (height, width, 2), box, slice_max)`` as ``GridFrontEnd.DrawTexture`` and ``oracle_draw_texture`` give
it.  ``paint`` gives the image as cairo leaves it: ARGB32 words, premultiplied, native endian.

    transform   submap.pose * submap.slice_pose is the translation t = (slice_max - o) + o per component, in double (o = the
                submap's origin); the cairo matrix (xx, yx, xy, yy, x0, y0) = (0, 1, -1, -0, t.x, -t.y) goes between
                cairo_scale(1 / r) and cairo_scale(r), each call replacing the CTM by (new matrix) * CTM.
    size        the four corners of the texture through the CTM, rounded to float32, their float32 min and max:
                size = ceil(float32(max - min)) + 10, origin = float32(-min + 5).  The rounding sometimes gives one pixel more
                than (height + 10, width + 10): the QUIRK.  The extra column or row is background.
    pixels      nearest neighbour: texture pixel (u, v) lands at image pixel (X, Y) = (height + 4 - v, u + 5), composited OVER
                the background 0xff800000 with pixman's 8-bit arithmetic; everything else is background.

Every DEFECT can be planted to show that a comparison notices it.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

BACKGROUND = 0xFF800000                 # cairo_set_source_rgba(0.5, 0, 0, 1): alpha 255, red 128
PADDING = 5                             # kPaddingPixel
DOMAIN_PIXELS = 16384.0                 # |t / r| below this: a float32 ulp of a corner coordinate is at most 1/1024 pixel
MAX_SIDE = 32767                        # cairo's largest image side

DEFECTS = ("transposed", "no_column_flip", "no_row_flip", "padding4", "no_quirk", "round", "plain_mul", "slice_max")
_f32 = np.float32


class OutOfDomain(ValueError):
    pass


def mul8(a, b):
    """pixman's MUL_UN8: a * b / 255 rounded, for 0 <= a, b <= 255 (ints or integer arrays)."""
    t = a * b + 128
    return (t + (t >> 8)) >> 8


def _mul(a, b, defect):
    return a * b // 255 if defect == "plain_mul" else mul8(a, b)


def texture_words(pairs):
    """io::DrawTexture (submap_painter.cc:135-164): one ARGB32 word per (value, alpha) pair -> uint32 (height, width)."""
    p = np.asarray(pairs, np.uint8).astype(np.uint32)
    value, alpha = p[..., 0], p[..., 1]
    observed = np.where((value == 0) & (alpha == 0), 0, 255).astype(np.uint32)
    return (alpha << 24) | (value << 16) | (observed << 8)


def over_background(words, defect=None):
    """cairo_paint of the words with operator OVER onto BACKGROUND: per channel min(255, src + mul8(255 - src alpha, dst))."""
    w = np.asarray(words, np.uint32).astype(np.int64)
    na = 255 - (w >> 24)
    out = np.zeros_like(w)
    for shift in (24, 16, 8, 0):
        src, dst = (w >> shift) & 255, (BACKGROUND >> shift) & 255
        out |= np.minimum(255, src + _mul(na, dst, defect)) << shift
    return out.astype(np.uint32)


def _multiply(a, b):
    """cairo_matrix_multiply: (xx, yx, xy, yy, x0, y0) of a applied first, then b."""
    return (a[0] * b[0] + a[1] * b[2], a[0] * b[1] + a[1] * b[3], a[2] * b[0] + a[3] * b[2], a[2] * b[1] + a[3] * b[3],
            a[4] * b[0] + a[5] * b[2] + b[4], a[4] * b[1] + a[5] * b[3] + b[5])


def translation(slice_max, submap_origin, defect=None):
    """(submap.pose * submap.slice_pose).translation(): slice_pose = slice_max - o, pose = o, both double."""
    if defect == "slice_max":
        return float(slice_max[0]), float(slice_max[1])
    return tuple((float(s) - float(o)) + float(o) for s, o in zip(slice_max, submap_origin))


def in_domain(width, height, slice_max, resolution, submap_origin):
    t = translation(slice_max, submap_origin)
    if not all(abs(c / float(resolution)) < DOMAIN_PIXELS for c in t):
        return False
    return max(size_and_origin(width, height, slice_max, resolution, submap_origin)[0]) <= MAX_SIDE


def size_and_origin(width, height, slice_max, resolution, submap_origin, defect=None):
    """PaintSubmapSlices' first pass -> ((size_x, size_y), (origin_x, origin_y) float32)."""
    r = float(resolution)
    t = translation(slice_max, submap_origin, defect)
    ctm = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)
    ctm = _multiply((1.0 / r, 0.0, 0.0, 1.0 / r, 0.0, 0.0), ctm)
    ctm = _multiply((0.0, 1.0, -1.0, -0.0, t[0], -t[1]), ctm)
    ctm = _multiply((r, 0.0, 0.0, r, 0.0, 0.0), ctm)
    xs, ys = [], []
    for x, y in ((0.0, 0.0), (float(width), 0.0), (0.0, float(height)), (float(width), float(height))):
        xs.append(_f32((ctm[0] * x + ctm[2] * y) + ctm[4]))
        ys.append(_f32((ctm[1] * x + ctm[3] * y) + ctm[5]))
    pad = 4 if defect == "padding4" else PADDING
    size, origin = [], []
    for lo, hi, plain in ((min(xs), max(xs), height), (min(ys), max(ys), width)):
        extent = _f32(hi - lo)
        size.append(plain + 2 * pad if defect == "no_quirk" else int(math.ceil(float(extent))) + 2 * pad)
        origin.append(_f32(_f32(-lo) + _f32(pad)))
    return tuple(size), tuple(origin)


@dataclass
class Painting:
    """What PaintSubmapSlices returns: ``argb`` uint32 (size_y, size_x), ``size`` (x, y), ``origin`` float32 (x, y); ``quirk`` says
    per axis whether the size is one more than the texture's side + 10."""
    argb: np.ndarray
    size: tuple
    origin: tuple
    quirk: tuple


def paint(texture, resolution, submap_origin, defect=None):
    assert defect is None or defect in DEFECTS
    pairs, _, slice_max = texture
    pairs = np.asarray(pairs, np.uint8)
    h, w = pairs.shape[:2]
    if not in_domain(w, h, slice_max, resolution, submap_origin):
        raise OutOfDomain("translation of 16384 pixels or more, or an image side above 32767")
    size, origin = size_and_origin(w, h, slice_max, resolution, submap_origin, defect)
    pad = 4 if defect == "padding4" else PADDING
    words = over_background(texture_words(pairs), defect)                       # (h, w): [v, u]
    if defect == "transposed":
        block = words.reshape(w, h)[:, ::-1]
    elif defect == "no_column_flip":
        block = words.T
    else:
        block = words.T[:, ::-1]                                                 # [u, h - 1 - v]
    argb = np.full((size[1], size[0]), BACKGROUND, np.uint32)
    argb[pad:pad + w, pad:pad + h] = block
    return Painting(argb, size, origin, (size[0] - h - 2 * pad, size[1] - w - 2 * pad))


def occupancy(painting, resolution, defect=None):
    """Node::CreateOccupancyGridMsg -> (data int8 (height, width), (origin_x, origin_y))."""
    red = ((painting.argb >> 16) & 255).astype(np.float64)
    observed = (painting.argb >> 8) & 255
    value = (1.0 - red / 255.0) * 100.0
    rounded = np.rint(value) if defect == "round" else np.floor(value + 0.5)    # lround: halves away from zero (value >= 0)
    data = np.where(observed == 0, -1, rounded).astype(np.int8)
    if defect != "no_row_flip":
        data = data[::-1]
    r = float(resolution)
    width, height = painting.size
    ox, oy = painting.origin
    return np.ascontiguousarray(data), (float(_f32(-ox)) * r, float(_f32(_f32(-height) + oy)) * r)


def image_red(painting):
    """The bytes WritePgm writes: the red channel, rows top to bottom -> uint8 (height, width)."""
    return ((painting.argb >> 16) & 255).astype(np.uint8)


def pgm_bytes(painting, resolution):
    """Node::WritePgm; std::to_string of a double is "%f"."""
    width, height = painting.size
    header = "P5\n# Cartographer map; " + "%f" % float(resolution) + " m/pixel\n" + str(width) + " " + str(height) + "\n255\n"
    return header.encode() + image_red(painting).tobytes()


def yaml_bytes(painting, resolution, pgm_filename):
    """Node::WriteYaml with HandleSaveMap's origin (-origin.x * r, (origin.y - height) * r)."""
    r = float(resolution)
    ox, oy = painting.origin
    x, y = float(_f32(-ox)) * r, float(_f32(oy - _f32(painting.size[1]))) * r
    return ("image: " + pgm_filename + "\nresolution: " + "%f" % r + "\norigin: [" + "%f" % x + ", " + "%f" % y +
            ", 0.0]\nnegate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n").encode()
