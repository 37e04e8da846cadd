"""The occupancy grid's C ABI, Python layer and witness without a GPU (rgrid_occupancy_grid / rgrid_batch_occupancy_* of
include/rgrid.h, GridFrontEnd.OccupancyGrid, ScanMatchFleet.occupancy_grids, MapBuilder.OccupancyGrid / SaveMap): the header declares
what the library exports, a library without the calls is reported on their first use only; the witness
(tests/witness/occupancy_witness.py) equals what libcairo itself painted (tests/golden/occupancy_cairo.npz, and libcairo directly
where it loads); the library's HOST text (size / origin replay, byte tables, frame copy) equals the witness; and the conditions the
GPU cases of tests/occupancy_cases.py rely on hold."""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import fleet_texture_cases as TC
from tests import occupancy_cases as OC
from tests.golden import make_golden_occupancy as G
from tests.witness import occupancy_witness as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rgrid_occupancy_grid", "rgrid_batch_occupancy_submit", "rgrid_batch_occupancy_collect")


def _header():
    text = open(os.path.join(ROOT, "include", "rgrid.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_three_calls():
    h = _header()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", h), name
    args = lambda name: [re.sub(r"\s+", " ", a).strip() for a in re.search(name + r"\s*\((.*?)\)\s*;", h, flags=re.S).group(1).split(",")]
    assert args(NEW[0]) == ["rgrid_t *h", "int mode", "const double submap_origin[2]", "int8_t *out", "long cap", "int size[2]",
                            "double origin[2]", "int box[4]"]
    assert args(NEW[1]) == ["rgrid_batch_t *b", "int mode", "const int *grids", "const double *submap_origins", "int count"]
    assert args(NEW[2]) == ["rgrid_batch_t *b", "int *status", "int *sizes", "double *origins", "int *boxes", "long *offsets",
                            "int8_t *out", "long cap"]


def test_library_exports_them():
    from reflector_ekf_slam_amd import fleet_match as M
    from reflector_ekf_slam_amd import grid
    L = M._occupancy_lib()
    assert not [n for n in NEW if not hasattr(L, n)]
    assert L is M._batch_lib() and grid._occupancy_lib() is grid._lib_rgrid()


def test_abi_version_stays_4():
    from reflector_ekf_slam_amd import fleet_match, grid
    assert int(re.search(r"#define\s+RGRID_ABI_VERSION\s+(\d+)", _header()).group(1)) == 4 == grid.RGRID_ABI_VERSION
    assert fleet_match._occupancy_lib().rgrid_abi_version() == 4


def test_null_handles_are_refused_with_a_code():
    from reflector_ekf_slam_amd import fleet_match as M
    from reflector_ekf_slam_amd import grid
    L = M._occupancy_lib()
    grid._occupancy_lib()
    buf = (C.c_double * 8)()
    a = C.addressof(buf)
    assert L.rgrid_batch_occupancy_submit(None, 0, a, a, 1) == M.RGRID_ERR_INVALID
    assert L.rgrid_batch_occupancy_submit(None, 0, None, None, 0) == M.RGRID_ERR_INVALID
    assert L.rgrid_batch_occupancy_collect(None, a, a, a, a, a, a, 8) == M.RGRID_ERR_INVALID
    d2, i2, i4 = (C.c_double * 2)(), (C.c_int * 2)(), (C.c_int * 4)()
    assert L.rgrid_occupancy_grid(None, 0, d2, a, 8, i2, d2, i4) == M.RGRID_ERR_INVALID


class _Without:
    """The built library seen through a filter: without the names in `hidden`."""

    def __init__(self, real, hidden=()):
        self._real, self._hidden = real, set(hidden)

    def __getattr__(self, name):
        if name in self._hidden:
            raise AttributeError(name)
        return getattr(self._real, name)


def test_a_library_without_the_calls_is_reported_by_them_only(monkeypatch):
    from reflector_ekf_slam_amd import _lib, grid
    from reflector_ekf_slam_amd import fleet_match as M
    from reflector_ekf_slam_amd import map_builder as MB
    real_root, real, insert, texture = grid._lib_rgrid(), M._batch_lib(), M._insert_lib(), M._texture_lib()
    for hidden in (NEW[1:], NEW[2:]):
        old = _Without(real, hidden)
        monkeypatch.setattr(M._batch_lib, "ready", old)
        for feature in (M._insert_lib, M._texture_lib, M._occupancy_lib):
            monkeypatch.setattr(feature, "ready", None)
        m = object.__new__(M.ScanMatchFleet)                       # a handle as an older library would have made it
        m._L, m._h, m._pending, m.num_grids = old, None, None, 1
        for call in (lambda: m.submit_occupancy_code([], []), m.collect_occupancy_code, lambda: m.submit_occupancy([0], [(0, 0)]),
                     m.collect_occupancy, lambda: m.occupancy_grids([], [])):
            with pytest.raises(_lib.LibraryMissing) as e:
                call()
            assert hidden[0] in str(e.value)
        # the calls it has keep working, the texture's included
        assert M._batch_lib() is old and M._insert_lib() is old and M._texture_lib() is old
        assert m.submit_texture_code([]) == M.RGRID_ERR_INVALID    # (a null handle: refused by the library itself)
        assert m.submit_insert_code([]) == M.RGRID_ERR_INVALID
    monkeypatch.setattr(M._batch_lib, "ready", real)
    monkeypatch.setattr(M._insert_lib, "ready", insert)
    monkeypatch.setattr(M._texture_lib, "ready", texture)
    monkeypatch.setattr(M._occupancy_lib, "ready", None)
    assert M._occupancy_lib() is real
    # the single handle's call
    old = _Without(real_root, NEW[:1])
    monkeypatch.setattr(grid._lib_rgrid, "ready", old)
    monkeypatch.setattr(grid._occupancy_lib, "ready", None)
    fe = object.__new__(grid.GridFrontEnd)
    fe._L, fe._h, fe._grid_shape = old, None, (3, 3)
    builder = object.__new__(MB.MapBuilder)
    builder._fe, builder._have_submap, builder._submap_origin = fe, True, (0.0, 0.0)
    for call in (lambda: fe.OccupancyGrid((0.0, 0.0)), builder.OccupancyGrid, lambda: builder.SaveMap("never_written")):
        with pytest.raises(_lib.LibraryMissing) as e:
            call()
        assert NEW[0] in str(e.value)
    assert not os.path.exists("never_written.pgm")
    assert old.rgrid_draw_texture(None, None, 0, None, None) == M.RGRID_ERR_INVALID
    monkeypatch.setattr(grid._lib_rgrid, "ready", real_root)
    monkeypatch.setattr(grid._occupancy_lib, "ready", None)
    assert grid._occupancy_lib() is real_root


def test_package_exports_and_the_record():
    import reflector_ekf_slam_amd as R
    from reflector_ekf_slam_amd import fleet_match as M
    from reflector_ekf_slam_amd import grid
    from reflector_ekf_slam_amd import map_builder as MB
    assert R.OccupancyGrid is grid.OccupancyGrid and R.FleetOccupancyGrid is M.FleetOccupancyGrid
    for name in ("submit_occupancy_code", "submit_occupancy", "collect_occupancy_code", "collect_occupancy", "occupancy_grids"):
        assert callable(getattr(M.ScanMatchFleet, name)), name
    assert callable(grid.GridFrontEnd.OccupancyGrid) and callable(MB.MapBuilder.OccupancyGrid) and callable(MB.MapBuilder.SaveMap)
    g = grid.OccupancyGrid(np.zeros((3, 2), np.int8), 0.05, (1.0, 2.0), (0, 0, 1, 1))
    assert (g.width, g.height) == (2, 3)
    assert M.FleetOccupancyGrid(g.data, 0.05, g.origin, g.box).status == 0
    builder = object.__new__(MB.MapBuilder)
    builder._have_submap = False
    assert builder.OccupancyGrid() is None and builder.SaveMap("never_written") is None


# ---- the witness against cairo ----------------------------------------------------------------------------------------------------
def _same_painting(p, argb, size, origin):
    return p.size == tuple(size) and tuple(p.origin) == tuple(origin) and p.argb.shape == argb.shape and np.array_equal(p.argb, argb)


@pytest.fixture(scope="module")
def golden():
    return G.load()


def test_witness_equals_the_golden_file(golden):
    assert 36 <= len(golden) <= 48 and os.path.getsize(G.OUT) < 200 * 1024
    for k, (pairs, slice_max, r, origin, argb, size, org) in enumerate(golden):
        assert max(pairs.shape[:2]) <= 40
        assert _same_painting(W.paint((pairs, None, slice_max), r, origin), argb, size, org), k


def test_golden_file_holds_what_it_should(golden, oracle_lib):
    emitted = {tuple(p) for p in TC.byte_table().tolist()}
    have = {tuple(p) for c in golden for p in c[0].reshape(-1, 2).tolist()}
    assert emitted <= have and (0, 0) in emitted and len(emitted) == 255      # every pair the texture table emits
    quirks = [(c[5][0] - c[0].shape[0] - 10, c[5][1] - c[0].shape[1] - 10) for c in golden]
    assert set(quirks) == {(0, 0), (1, 0), (0, 1), (1, 1)}
    for form in OC.QUIRK_FORMS:
        assert quirks.count(form) >= 4, form
    far = [np.array(c[1]) / c[2] for c in golden]
    for sx in (-1, 1):                                                              # corners near +-16000 px, every sign combination
        for sy in (-1, 1):
            assert any(15900 <= sx * t[0] < 16384 and 15900 <= sy * t[1] < 16384 for t in far), (sx, sy)
    shapes = {c[0].shape[:2] for c in golden}
    assert {(1, 1), (1, 40), (40, 1), (40, 40)} <= shapes
    # cases in which replaying (slice_max - o) + o instead of taking slice_max changes the float32 origin cairo arrived at
    shows = [c for c in golden if W.size_and_origin(c[0].shape[1], c[0].shape[0], c[1], c[2], c[3], "slice_max") != (tuple(c[5]), tuple(c[6]))]
    assert len(shows) >= 4


def _cairo_or_skip():
    try:
        return G.cairo()
    except OSError:
        pytest.skip("libcairo.so.2 is not on this machine")


def test_witness_equals_cairo_on_the_golden_inputs(golden):
    _cairo_or_skip()
    for k, (pairs, slice_max, r, origin, argb, size, org) in enumerate(golden):
        got = G.cairo_paint_texture(pairs, slice_max, r, origin)
        assert np.array_equal(got[0], argb) and got[1] == tuple(size) and tuple(got[2]) == tuple(org), k   # the file is what cairo gives here


def test_witness_equals_cairo_on_a_seeded_sweep():
    _cairo_or_skip()
    rng = np.random.default_rng(61)
    quirks, far = 0, 0
    for k in range(320):
        c = G.random_case(rng, 72, reach_px=16383.0) if k % 2 else G.random_case(rng, 72, reach_m=400.0)
        argb, size, org = G.cairo_paint_texture(*c)
        p = W.paint((c[0], None, c[1]), c[2], c[3])
        assert _same_painting(p, argb, size, org), k
        quirks += p.quirk != (0, 0)
        far += max(abs(c[1][0]), abs(c[1][1])) / c[2] > 12000
    assert quirks >= 3 and far >= 60                                                # the sweep reaches the quirk and the domain's far end


@pytest.mark.parametrize("defect", W.DEFECTS)
def test_every_planted_defect_is_caught_by_a_golden_case(golden, defect):
    """`round` (half to even) in place of lround (half away from zero) is the one defect no image can show: (1 - red / 255) * 100
    is a multiple of 20 / 51 and never within 1 / 102 of a half, so both roundings agree for all 256 reds -- that is what is
    asserted for it, over every red and not only the golden ones."""
    if defect == "round":
        red = np.arange(256, dtype=np.float64)
        value = (1.0 - red / 255.0) * 100.0
        assert np.abs(value - np.floor(value) - 0.5).min() > 1.0 / 103 and np.array_equal(np.rint(value), np.floor(value + 0.5))
        return
    caught = 0
    for pairs, slice_max, r, origin, argb, size, org in golden:
        try:
            p = W.paint((pairs, None, slice_max), r, origin, defect)
        except ValueError:                                                          # a block that does not fit its image
            caught += 1
            continue
        good = W.paint((pairs, None, slice_max), r, origin)
        if not _same_painting(p, argb, size, org) or not np.array_equal(W.occupancy(p, r, defect)[0], W.occupancy(good, r)[0]):
            caught += 1
    assert caught, defect


def test_pgm_and_yaml_bytes_by_hand():
    pairs = np.array([[[0, 0], [0, 127], [127, 0]]], np.uint8)                     # one row: unknown, occupied, free -> a 1 x 3 texture
    p = W.paint((pairs, (0, 0, 3, 1), (0.5, 0.25)), 0.05, (0.0, 0.0))
    assert p.size == (11, 13) and p.quirk == (0, 0) and p.origin == (-4.0, 10.0)
    assert W.image_red(p)[5:8, 5].tolist() == [128, 64, 255] and np.count_nonzero(W.image_red(p) != 128) == 2
    assert W.pgm_bytes(p, 0.05) == b"P5\n# Cartographer map; 0.050000 m/pixel\n11 13\n255\n" + W.image_red(p).tobytes()
    assert W.yaml_bytes(p, 0.05, "/tmp/m.pgm") == (b"image: /tmp/m.pgm\nresolution: 0.050000\norigin: [0.200000, -0.150000, 0.0]\n"
                                                   b"negate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n")
    data, origin = W.occupancy(p, 0.05)
    assert data.shape == (13, 11) and data[12 - 5:12 - 8:-1, 5].tolist() == [-1, 75, 0] and origin == (4.0 * 0.05, -3.0 * 0.05)
    # the product's writers give the same bytes from the same fields
    from reflector_ekf_slam_amd import grid
    image = grid.OccupancyGrid(W.image_red(p), 0.05, origin, (0, 0, 3, 1))
    assert grid.pgm_bytes(image) == W.pgm_bytes(p, 0.05) and grid.yaml_bytes(image, "/tmp/m.pgm") == W.yaml_bytes(p, 0.05, "/tmp/m.pgm")


# ---- the library's host text against the witness ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/cpp/occupancy_host.cpp, built host-only: the text of csrc/rgrid_dev.h that runs on the host, without a GPU."""
    if shutil.which("hipcc") is None:
        pytest.skip("needs hipcc")
    exe = str(tmp_path_factory.mktemp("occupancy_host") / "occupancy_host")
    r = subprocess.run(["hipcc", "-x", "hip", "--offload-host-only", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "occupancy_host.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_host_tables_compose_the_texture_table_with_the_witness(host_program, tmp_path, oracle_lib):
    out = str(tmp_path / "tables.bin")
    subprocess.run([host_program, "tables", out], check=True)
    t = np.fromfile(out, np.uint8)
    pairs = TC.byte_table()                                                         # the oracle's (value, alpha) per cell value
    words = W.over_background(W.texture_words(pairs.reshape(1, -1, 2)))[0]
    red = ((words >> 16) & 255).astype(np.uint8)
    occupancy = np.where(((words >> 8) & 255) == 0, -1, np.floor((1.0 - red / 255.0) * 100.0 + 0.5)).astype(np.int8)
    assert np.array_equal(t[32768:], red) and np.array_equal(t[:32768].view(np.int8), occupancy)
    assert occupancy[0] == -1 and red[0] == 128 and set(occupancy[1:].tolist()) <= set(range(0, 101))


def test_host_replay_equals_the_witness(host_program, tmp_path, golden):
    rng = np.random.default_rng(97)
    cases = [(c[0].shape[1], c[0].shape[0], c[1], c[2], c[3]) for c in golden]
    for k in range(300):
        c = G.random_case(rng, 600, reach_px=16383.0) if k % 2 else G.random_case(rng, 600, reach_m=400.0)
        cases.append((c[0].shape[1], c[0].shape[0], c[1], c[2], c[3]))
    cases += [(9, 7, (18000 * 0.05, 1.0), 0.05, (0.5, -0.5)), (9, 7, (1.0, -16385 * 0.05), 0.05, (0.0, 0.0)), (32758, 2, (0.0, 0.0), 0.05, (0.0, 0.0))]
    path = str(tmp_path / "frames.txt")
    with open(path, "w") as f:
        for w, h, slice_max, r, o in cases:                                          # box at offset 0: limits.max = slice_max
            f.write("0 0 %d %d %s %s %s %s %s\n" % (w, h, float(r).hex(), float(slice_max[0]).hex(), float(slice_max[1]).hex(),
                                                     float(o[0]).hex(), float(o[1]).hex()))
    lines = subprocess.run([host_program, "frames", path], check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    assert len(lines) == len(cases)
    refused = 0
    for (w, h, slice_max, r, o), line in zip(cases, lines):
        rc, sx, sy, ox, oy = line.split()
        if not W.in_domain(w, h, slice_max, r, o):
            assert int(rc) == -4, line
            refused += 1
            continue
        size, origin = W.size_and_origin(w, h, slice_max, r, o)
        p = W.Painting(np.zeros((size[1], size[0]), np.uint32), size, origin, (0, 0))
        assert int(rc) == 0 and (int(sx), int(sy)) == size and (float.fromhex(ox), float.fromhex(oy)) == W.occupancy(p, r)[1], line
    assert refused == 3
    # the replay of (slice_max - o) + o is pinned: on the golden cases made for it, t = slice_max gives another message origin
    told = 0
    for (w, h, slice_max, r, o), line in zip(cases[:len(golden)], lines):
        size, origin = W.size_and_origin(w, h, slice_max, r, o, "slice_max")
        wrong = W.occupancy(W.Painting(np.zeros((size[1], size[0]), np.uint32), size, origin, (0, 0)), r)[1]
        told += wrong != tuple(float.fromhex(v) for v in line.split()[3:])
    assert told >= 4


@pytest.mark.parametrize("mode", [OC.OCCUPANCY, OC.IMAGE])
def test_host_frame_copy_equals_the_witness_layout(host_program, tmp_path, mode):
    for w, h, qx, qy in ((1, 1, 0, 0), (3, 17, 1, 0), (16, 5, 0, 1), (33, 31, 1, 1)):
        sx, sy = h + 10 + qx, w + 10 + qy
        out = str(tmp_path / "image.bin")
        subprocess.run([host_program, "paint", str(mode), str(w), str(h), str(sx), str(sy), out], check=True)
        got = np.fromfile(out, np.uint8).reshape(sy, sx)
        u, c = np.meshgrid(np.arange(w), np.arange(h), indexing="ij")
        want = np.full((sy, sx), 255 if mode == OC.OCCUPANCY else 128, np.uint8)
        want[5:5 + w, 5:5 + h] = (31 * u + 7 * c + 1) & 255
        assert np.array_equal(got, want[::-1] if mode == OC.OCCUPANCY else want), (w, h)


def test_cpp_adapter_occupancy_calls_compile():
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "occupancy_adapter_syntax.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


# ---- the case file -----------------------------------------------------------------------------------------------------------------
def test_cases_hold_their_conditions(oracle_lib):
    assert OC.T == 64 and OC.WG_THREADS == TC.WG_THREADS and OC.EDGE_MAX_CELLS % 2 == 1 and TC.SWEEP_MAX_CELLS % 2 == 1
    src = open(os.path.join(ROOT, "reflector_ekf_slam_amd", "csrc", "rgrid_dev.h")).read()
    assert re.search(r"#define\s+OCC_T\s+%d\b" % OC.T, src) and re.search(r"#define\s+KGT_THREADS\s+%d\b" % OC.WG_THREADS, src)
    sweep = OC.sweep_case()
    assert len(sweep) == 8 and all(a[0] is b for a, b in zip(sweep, TC.sweep_case())) and sweep[7][0][0].shape == (181, 183)
    edges = OC.edge_cases()
    boxes = [TC.oracle_texture(g)[1] for g, _ in edges]
    assert [(b[2], b[3]) for b in boxes] == OC.EDGE_BOXES + OC.STRIDE_BOXES + OC.LONG_BOXES
    assert len(OC.EDGE_BOXES) == 16 and all(b[0] > 0 and b[1] > 0 for b in boxes)
    assert all(b[0] + b[2] < g[0].shape[1] and b[1] + b[3] < g[0].shape[0] for b, (g, _) in zip(boxes, edges))      # strictly inside
    assert max(g[0].size for g, _ in edges) <= OC.EDGE_MAX_CELLS < max(g[0].size for g, _ in edges) + 2
    assert {h % OC.STRIDE_ALIGN for _, h in OC.STRIDE_BOXES} == {15, 0, 1} and OC.LONG_N > OC.WG_THREADS
    for case in sweep + edges:
        assert OC.expected(case, OC.OCCUPANCY) is not None
    # the quirk cases have the quirk, one form each, according to the witness
    for form, case in zip(OC.QUIRK_FORMS, OC.quirk_cases()):
        data, _, box = OC.expected(case, OC.IMAGE)
        assert (data.shape[1] - box[3] - 10, data.shape[0] - box[2] - 10) == form
        assert (data[:, box[3] + 10:] == 128).all() and (data[box[2] + 10:] == 128).all()       # the extra column / row is background
    # the replay case really needs the replay: with t = slice_max the witness gives another origin
    grid, origin = OC.replay_case()
    tex = TC.oracle_texture(grid)
    assert tex[1][:2] == (2, 1)
    good = W.paint(tex, grid[1], origin)
    bad = W.paint(tex, grid[1], origin, "slice_max")
    assert W.occupancy(good, grid[1])[1] != W.occupancy(bad, grid[1])[1] and W.translation(tex[2], origin) != tuple(tex[2])
    # the out-of-domain case is out of domain, and only just
    case = OC.out_of_domain_case()
    assert OC.expected(case, OC.OCCUPANCY) is None
    grid, origin = case
    near = ((grid[0], grid[1], (16000 * grid[1], grid[2][1])), origin)
    assert OC.expected(near, OC.OCCUPANCY) is not None
    # the two modes of a case are the same painting
    occ, o0, b0 = OC.expected(edges[3], OC.OCCUPANCY)
    img, o1, b1 = OC.expected(edges[3], OC.IMAGE)
    assert o0 == o1 and b0 == b1 and occ.dtype == np.int8 and img.dtype == np.uint8 and occ.shape == img.shape
    assert np.array_equal(occ[::-1] == -1, img == 128)                              # red 128 is the unknown cell and the background, nothing else
