"""Regenerates tests/golden/occupancy_cairo.npz: what libcairo itself makes of a submap texture when it is driven with the call
sequence of the reference's io::PaintSubmapSlices (src/io/submap_painter.cc:13-91) -- the pin of tests/witness/occupancy_witness.py.

    python tests/golden/make_golden_occupancy.py

Needs libcairo.so.2 (through ctypes; nothing else).  ``cairo_paint_texture`` is also what tests/test_occupancy_cpu.py sweeps where
the library is present.  A case is (pairs uint8 (height, width, 2), slice_max (2), resolution, submap_origin (2)); recorded are
cairo's image (ARGB32 words), its size and the float32 origin.

The cases, 45 textures of at most 40 x 40 pixels:
    0       16 x 16: every (value, 0) and (0, alpha) for 0 .. 127 -- a superset of what the texture table emits
    1 - 12  four of each quirk form (size one more than side + 10 in x only, y only, both), found by a seeded search with cairo's own
            size computation
    13 - 20 corners near +-16000 pixels, every sign combination, two resolutions
    21 - 40 random sizes 1 .. 40 (1 x 1, 1 x N and N x 1 among them), resolutions 0.02 .. 0.1, corners up to +-400 m
    41 - 44 the translation (slice_max - origin) + origin is not slice_max AND cairo's float32 origin shows it (``replay_case``: a directed
            search that puts a corner next to the midpoint of two float32 values)
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "occupancy_cairo.npz")
_f32 = np.float32


class _Matrix(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("xx", "yx", "xy", "yy", "x0", "y0")]


_cairo = None


def cairo():
    """libcairo.so.2 with the argtypes of the calls used here; OSError where it is absent."""
    global _cairo
    if _cairo is None:
        L = C.CDLL("libcairo.so.2")
        vp, d = C.c_void_p, C.c_double
        L.cairo_image_surface_create.restype = vp
        L.cairo_image_surface_create.argtypes = [C.c_int, C.c_int, C.c_int]
        L.cairo_image_surface_create_for_data.restype = vp
        L.cairo_image_surface_create_for_data.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
        L.cairo_create.restype = vp
        L.cairo_create.argtypes = [vp]
        for name, args in (("cairo_scale", [vp, d, d]), ("cairo_translate", [vp, d, d]), ("cairo_save", [vp]), ("cairo_restore", [vp]),
                           ("cairo_transform", [vp, C.POINTER(_Matrix)]), ("cairo_matrix_init", [C.POINTER(_Matrix)] + [d] * 6),
                           ("cairo_user_to_device", [vp, C.POINTER(d), C.POINTER(d)]), ("cairo_set_source_rgba", [vp, d, d, d, d]),
                           ("cairo_paint", [vp]), ("cairo_set_source_surface", [vp, vp, d, d]), ("cairo_surface_flush", [vp]),
                           ("cairo_destroy", [vp]), ("cairo_surface_destroy", [vp])):
            getattr(L, name).restype = None
            getattr(L, name).argtypes = args
        L.cairo_image_surface_get_data.restype = vp
        L.cairo_image_surface_get_data.argtypes = [vp]
        for name in ("cairo_image_surface_get_width", "cairo_image_surface_get_height", "cairo_image_surface_get_stride", "cairo_status",
                     "cairo_surface_status"):
            getattr(L, name).restype = C.c_int
            getattr(L, name).argtypes = [vp]
        L.cairo_format_stride_for_width.restype = C.c_int
        L.cairo_format_stride_for_width.argtypes = [C.c_int, C.c_int]
        _cairo = L
    return _cairo


ARGB32 = 0


def _slice_transform(L, cr, scale, t, submap_resolution):
    """CairoPaintSubmapSlices up to the callback (the caller restores)."""
    L.cairo_scale(cr, scale, scale)
    L.cairo_save(cr)
    m = _Matrix()
    L.cairo_matrix_init(C.byref(m), 0.0, 1.0, -1.0, -0.0, t[0], -t[1])          # homo = Translation(t) * identity rotation
    L.cairo_transform(cr, C.byref(m))
    L.cairo_scale(cr, submap_resolution, submap_resolution)


def cairo_size_and_origin(width, height, slice_max, resolution, submap_origin):
    """PaintSubmapSlices' first pass: cairo's user_to_device of the four corners, Eigen's AlignedBox2f -> ((sx, sy), (ox, oy) float32)."""
    t = tuple((float(s) - float(o)) + float(o) for s, o in zip(slice_max, submap_origin))     # (pose * slice_pose).translation()
    return size_and_origin_at(width, height, t, resolution)


def size_and_origin_at(width, height, t, resolution):
    """... for the translation t."""
    L = cairo()
    r = float(resolution)
    surface = L.cairo_image_surface_create(ARGB32, 1, 1)
    cr = L.cairo_create(surface)
    _slice_transform(L, cr, 1.0 / r, t, r)
    xs, ys = [], []
    for x, y in ((0, 0), (width, 0), (0, height), (width, height)):
        dx, dy = C.c_double(x), C.c_double(y)
        L.cairo_user_to_device(cr, C.byref(dx), C.byref(dy))
        xs.append(_f32(dx.value))
        ys.append(_f32(dy.value))
    L.cairo_restore(cr)
    L.cairo_destroy(cr)
    L.cairo_surface_destroy(surface)
    size = (int(math.ceil(float(_f32(max(xs) - min(xs))))) + 10, int(math.ceil(float(_f32(max(ys) - min(ys))))) + 10)
    origin = (_f32(_f32(-min(xs)) + _f32(5)), _f32(_f32(-min(ys)) + _f32(5)))
    return size, origin


def cairo_paint_texture(pairs, slice_max, resolution, submap_origin):
    """FillSubmapSlice + PaintSubmapSlices -> (argb uint32 (size_y, size_x), (size_x, size_y), (origin_x, origin_y) float32)."""
    L = cairo()
    pairs = np.ascontiguousarray(pairs, np.uint8)
    height, width = pairs.shape[:2]
    r = float(resolution)
    t = tuple((float(s) - float(o)) + float(o) for s, o in zip(slice_max, submap_origin))
    size, origin = cairo_size_and_origin(width, height, slice_max, resolution, submap_origin)
    value, alpha = pairs[..., 0].astype(np.uint32), pairs[..., 1].astype(np.uint32)
    observed = np.where((value == 0) & (alpha == 0), 0, 255).astype(np.uint32)
    data = np.ascontiguousarray((alpha << 24) | (value << 16) | (observed << 8))                 # io::DrawTexture
    assert L.cairo_format_stride_for_width(ARGB32, width) == 4 * width
    tex = L.cairo_image_surface_create_for_data(data.ctypes.data, ARGB32, width, height, 4 * width)
    assert L.cairo_surface_status(tex) == 0
    surface = L.cairo_image_surface_create(ARGB32, size[0], size[1])
    assert L.cairo_surface_status(surface) == 0, size
    cr = L.cairo_create(surface)
    L.cairo_set_source_rgba(cr, 0.5, 0.0, 0.0, 1.0)
    L.cairo_paint(cr)
    L.cairo_translate(cr, float(origin[0]), float(origin[1]))
    _slice_transform(L, cr, 1.0 / r, t, r)
    L.cairo_set_source_surface(cr, tex, 0.0, 0.0)
    L.cairo_paint(cr)
    L.cairo_restore(cr)
    L.cairo_surface_flush(surface)
    assert L.cairo_status(cr) == 0
    sx, sy = L.cairo_image_surface_get_width(surface), L.cairo_image_surface_get_height(surface)
    stride = L.cairo_image_surface_get_stride(surface)
    assert (sx, sy) == size and stride == 4 * sx
    raw = C.string_at(L.cairo_image_surface_get_data(surface), stride * sy)
    argb = np.frombuffer(raw, np.uint32).reshape(sy, sx).copy()
    L.cairo_destroy(cr)
    L.cairo_surface_destroy(surface)
    L.cairo_surface_destroy(tex)
    return argb, size, origin


EMITTED = [(v, 0) for v in range(128)] + [(0, a) for a in range(128)]          # (value, alpha): the texture table's range and more


def random_pairs(rng, height, width):
    """A texture of pairs the table can emit, a third of it unknown."""
    pick = rng.integers(0, len(EMITTED), (height, width))
    pairs = np.array(EMITTED, np.uint8)[pick]
    pairs[rng.random((height, width)) < 0.33] = 0
    return pairs


def random_case(rng, max_side, reach_m=None, reach_px=None):
    """One case with corners up to +-reach_m metres or +-reach_px pixels."""
    height, width = int(rng.integers(1, max_side + 1)), int(rng.integers(1, max_side + 1))
    resolution = float(_f32(rng.choice([0.02, 0.025, 0.05, 0.1]))) if rng.random() < 0.5 else float(rng.uniform(0.02, 0.1))
    reach = reach_m if reach_px is None else reach_px * resolution
    origin = tuple(float(_f32(v)) for v in rng.uniform(-reach, reach, 2))      # the submap origin is a float cast to double
    far = min(reach, 0.97 * 16384 * resolution)
    slice_max = tuple(float(v) for v in rng.uniform(-far, far, 2))
    return random_pairs(rng, height, width), slice_max, resolution, origin


def quirk_of(case):
    pairs, slice_max, resolution, origin = case
    size, _ = cairo_size_and_origin(pairs.shape[1], pairs.shape[0], slice_max, resolution, origin)
    return size[0] - pairs.shape[0] - 10, size[1] - pairs.shape[1] - 10


def replay_case(rng):
    """A case in which the translation (slice_max - o) + o and slice_max itself give cairo different float32 corners: a directed
    search that puts the corner (0, height) within a few ulps of the midpoint between two float32 values and keeps the first
    slice_max.x for which cairo's own first pass answers differently for the two translations."""
    while True:
        height, width = int(rng.integers(2, 25)), int(rng.integers(2, 25))
        resolution = float(_f32(0.05)) if rng.random() < 0.5 else float(rng.uniform(0.02, 0.1))
        origin = tuple(float(_f32(v)) for v in rng.uniform(-5.0, 5.0, 2))
        corner = _f32(rng.uniform(100.0, 12000.0) * rng.choice([-1.0, 1.0]))      # where the corner (0, height) is to land, in pixels
        midpoint = 0.5 * (float(corner) + float(np.nextafter(corner, _f32(np.inf))))
        x = (midpoint + height) * resolution
        for k in range(-4, 5):
            sx = x
            for _ in range(abs(k)):
                sx = float(np.nextafter(sx, math.inf if k > 0 else -math.inf))
            slice_max = (sx, float(rng.uniform(-20.0, 20.0)))
            t = tuple((s - o) + o for s, o in zip(slice_max, origin))
            if t != slice_max and size_and_origin_at(width, height, t, resolution) != size_and_origin_at(width, height, slice_max, resolution):
                return random_pairs(rng, height, width), slice_max, resolution, origin


N_REPLAY = 4


def cases():
    return base_cases() + replay_cases()


def replay_cases():
    rng = np.random.default_rng(31337)
    return [replay_case(rng) for _ in range(N_REPLAY)]


def base_cases():
    rng = np.random.default_rng(20260417)
    out = [(np.array(EMITTED, np.uint8).reshape(16, 16, 2), (1.25, -0.75), float(_f32(0.05)), (float(_f32(0.3)), float(_f32(0.5))))]
    want = {(1, 0): 4, (0, 1): 4, (1, 1): 4}
    found = {k: [] for k in want}
    while any(len(found[k]) < n for k, n in want.items()):
        c = random_case(rng, 24, reach_m=400.0)
        q = quirk_of(c)
        if q in found and len(found[q]) < want[q]:
            found[q].append(c)
    for k in ((1, 0), (0, 1), (1, 1)):
        out += found[k]
    for resolution in (float(_f32(0.05)), 0.0371):
        for sx in (-1, 1):
            for sy in (-1, 1):
                h, w = int(rng.integers(2, 25)), int(rng.integers(2, 25))
                px = rng.uniform(15900, 16000, 2)
                slice_max = (sx * px[0] * resolution, sy * px[1] * resolution)
                origin = tuple(float(_f32(v)) for v in rng.uniform(-5, 5, 2))
                out.append((random_pairs(rng, h, w), slice_max, resolution, origin))
    shapes = [(1, 1), (1, 40), (40, 1), (40, 40), (39, 17)]
    for k in range(20):
        c = random_case(rng, 40, reach_m=400.0)
        if k < len(shapes):
            c = (random_pairs(rng, *shapes[k]),) + c[1:]
        out.append(c)
    return out


def pack(cs):
    """The cases and cairo's answers as flat arrays."""
    rec = {"shape": [], "slice_max": [], "resolution": [], "submap_origin": [], "size": [], "origin": [], "pairs": [], "argb": []}
    for pairs, slice_max, resolution, origin in cs:
        argb, size, org = cairo_paint_texture(pairs, slice_max, resolution, origin)
        rec["shape"].append(pairs.shape[:2]); rec["slice_max"].append(slice_max); rec["resolution"].append(resolution)
        rec["submap_origin"].append(origin); rec["size"].append(size); rec["origin"].append(org)
        rec["pairs"].append(pairs.reshape(-1)); rec["argb"].append(argb.reshape(-1))
    return {"shape": np.array(rec["shape"], np.int32), "slice_max": np.array(rec["slice_max"], np.float64),
            "resolution": np.array(rec["resolution"], np.float64), "submap_origin": np.array(rec["submap_origin"], np.float64),
            "size": np.array(rec["size"], np.int32), "origin": np.array(rec["origin"], np.float32),
            "pairs": np.concatenate(rec["pairs"]).astype(np.uint8), "argb": np.concatenate(rec["argb"]).astype(np.uint32)}


def load(path=OUT):
    """-> [(pairs, slice_max, resolution, submap_origin, argb, size, origin)] of the committed file."""
    z = np.load(path)
    out, at_p, at_a = [], 0, 0
    for k in range(z["shape"].shape[0]):
        h, w = (int(v) for v in z["shape"][k])
        sx, sy = (int(v) for v in z["size"][k])
        pairs = z["pairs"][at_p:at_p + 2 * h * w].reshape(h, w, 2)
        argb = z["argb"][at_a:at_a + sx * sy].reshape(sy, sx)
        at_p, at_a = at_p + 2 * h * w, at_a + sx * sy
        out.append((pairs, tuple(float(v) for v in z["slice_max"][k]), float(z["resolution"][k]),
                    tuple(float(v) for v in z["submap_origin"][k]), argb, (sx, sy), tuple(z["origin"][k])))
    return out


if __name__ == "__main__":
    np.savez_compressed(OUT, **pack(cases()))
    print(OUT, os.path.getsize(OUT), "bytes,", len(load()), "cases")
