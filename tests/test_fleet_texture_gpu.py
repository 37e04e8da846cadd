"""The fleet texture on the GPU (kgb_texture of csrc/rgrid_batch.hip behind ScanMatchFleet.draw_textures): every named slot's bytes,
box and slice corner exactly what a GridFrontEnd holding the same grid returns from DrawTexture (the specification) and what the CPU
oracle computes.  Every assertion is exact equality: the result is a function of the grid only."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests import fleet_insert_cases as IC
from tests import fleet_texture_cases as TC

pytestmark = pytest.mark.gpu

OK, INVALID, BUFFER = 0, -1, -5


def fleet(num_grids, max_cells, max_points=512, **kw):
    from reflector_ekf_slam_amd import fleet_match as M
    return M.ScanMatchFleet(max_scans=num_grids, max_points=max_points, num_grids=num_grids, max_cells=max_cells, max_rotations=1, **kw)


def front_end(max_cells, max_points=512):
    from reflector_ekf_slam_amd.grid import GridFrontEnd
    return GridFrontEnd(max_points=max_points, max_cells=max_cells, max_candidates=1 << 10)


def set_grids(m, grids):
    for slot, (cells, res, max_xy) in enumerate(grids):
        m.SetGrid(slot, cells, res, max_xy)


def handle_texture(gf, grid):
    gf.SetGrid(*grid)
    return gf.DrawTexture()


@pytest.fixture(scope="module")
def sweep(oracle_lib):
    """The sweep's grids resident in one handle, and what the oracle draws of them (computed once, never changed)."""
    grids = TC.sweep_case()
    m = fleet(8, TC.SWEEP_MAX_CELLS)
    set_grids(m, grids)
    want = [TC.oracle_texture(g) for g in grids]
    yield m, grids, want
    m.close()


def test_sweep_in_any_order_alone_and_repeated(sweep):
    m, grids, want = sweep
    assert m.set_slots() == list(range(8))
    got = m.draw_textures()                                                        # every slot that has been set
    assert len(got) == 8
    gf = front_end(TC.SWEEP_MAX_CELLS)
    for k, g in enumerate(grids):
        assert TC.same_texture(got[k], want[k]), (TC.SWEEP_NAMES[k], got[k].box, want[k][1], got[k].slice_max, want[k][2])
        assert TC.same_texture(got[k], handle_texture(gf, g)), TC.SWEEP_NAMES[k]
    gf.close()
    assert got[4].cells.tolist() == [[[0, 0]]] and got[4].box == (0, 0, 1, 1)
    back = m.draw_textures(range(7, -1, -1))                                       # the same call reversed
    assert all(TC.same_texture(back[7 - k], want[k]) for k in range(8))
    for k in range(8):                                                             # each slot alone
        assert TC.same_texture(m.draw_textures([k])[0], want[k]), TC.SWEEP_NAMES[k]
    some = m.draw_textures([6, 1, 7])
    assert [TC.same_texture(t, want[k]) for t, k in zip(some, (6, 1, 7))] == [True] * 3
    thrice = m.draw_textures([2, 0, 2, 2, 7, 0])                                   # a slot any number of times: the call only reads
    assert [TC.same_texture(t, want[k]) for t, k in zip(thrice, (2, 0, 2, 2, 7, 0))] == [True] * 6
    for k, g in enumerate(grids):                                                  # ... and it left the slots as they were
        assert np.array_equal(m.GetGrid(k), g[0])


def test_garbage_behind_the_slot_is_not_read(oracle_lib):
    garbage, grid = TC.multi_pass_case()
    m = fleet(2, TC.MULTI_MAX_CELLS)
    m.SetGrid(TC.MULTI_SLOT, *garbage)
    full = m.draw_textures([TC.MULTI_SLOT])[0]
    assert TC.same_texture(full, TC.oracle_texture(garbage)) and full.box == (0, 0, garbage[0].shape[1], garbage[0].shape[0])
    m.SetGrid(TC.MULTI_SLOT, *grid)                                                # the slot's last cells keep the larger grid's values
    got = m.draw_textures()[0]
    assert TC.same_texture(got, TC.oracle_texture(grid)), (got.box, got.slice_max)
    gf = front_end(TC.MULTI_MAX_CELLS)
    assert TC.same_texture(got, handle_texture(gf, grid))
    gf.close(); m.close()


def test_after_the_write_path_the_box_moves_with_the_growth(oracle_lib):
    from oracle.binding import oracle_grow
    case = IC.growth_case()
    m = fleet(2, IC.GROW_MAX_CELLS)
    grids = [grid for grid, _ in case]
    set_grids(m, grids)
    before = m.draw_textures()
    moved = 0
    for k in range(len(IC.GROW_FAR)):
        scans = [case[slot][1][k] for slot in range(2)]
        offs = [oracle_grow(*m_grid, scans[slot][1], scans[slot][2], scans[slot][3])[2] for slot, m_grid in enumerate(grids)]
        assert m.insert(scans) == [OK, OK]
        now = []
        for slot in range(2):
            lim = m.GetLimits(slot)
            now.append((m.GetGrid(slot), lim[2], (lim[3], lim[4])))
        after = m.draw_textures()
        for slot in range(2):
            assert TC.same_texture(after[slot], TC.oracle_texture(now[slot])), (k, slot, after[slot].box)
            # the old box, moved by the growth's offsets, lies inside the new one: the insertion only adds known cells
            (ox, oy, ow, oh), (nx, ny, nw, nh) = before[slot].box, after[slot].box
            sx, sy = ox + offs[slot][0], oy + offs[slot][1]
            assert nx <= sx and ny <= sy and sx + ow <= nx + nw and sy + oh <= ny + nh, (k, slot, before[slot].box, offs[slot], after[slot].box)
            moved += offs[slot] != (0, 0) and (nx, ny) != (ox, oy)
        grids, before = now, after
    assert moved >= 2 and all(g[0].shape[0] >= 8 * IC.GROW_SHAPES[slot][0] for slot, g in enumerate(grids))
    m.close()


def test_buffer_protocol_of_the_c_calls(sweep):
    from reflector_ekf_slam_amd import fleet_match as M
    m, grids, want = sweep
    L = M._texture_lib()
    ids = np.array([0, 7, 4, 2], np.int32)
    total = sum(want[k][0].size for k in ids)
    boxes, sm, offs = np.zeros((4, 4), np.int32), np.zeros((4, 2)), np.zeros(4, dtype=C.c_long)
    out = np.full(total, 0xAB, np.uint8)
    assert L.rgrid_batch_texture_submit(m._h, ids.ctypes.data, 4) == OK
    for cap, cells in ((total - 1, out.ctypes.data), (total, None)):               # a byte short; room but nowhere to put it
        boxes[:], sm[:], offs[:] = -7, -7.0, -7
        assert L.rgrid_batch_texture_collect(m._h, boxes.ctypes.data, sm.ctypes.data, offs.ctypes.data, cells, cap) == BUFFER
        assert [tuple(b) for b in boxes.tolist()] == [want[k][1] for k in ids]
        assert [tuple(s) for s in sm.tolist()] == [want[k][2] for k in ids]
        assert offs.tolist() == np.concatenate([[0], np.cumsum([want[k][0].size for k in ids])[:-1]]).tolist()
        assert (out == 0xAB).all()                                                 # nothing was copied
    assert L.rgrid_batch_texture_submit(m._h, ids.ctypes.data, 4) == INVALID       # it is still pending
    assert L.rgrid_batch_texture_collect(m._h, boxes.ctypes.data, sm.ctypes.data, offs.ctypes.data, out.ctypes.data, total) == OK
    for j, k in enumerate(ids):
        n = want[k][0].size
        assert np.array_equal(out[offs[j]:offs[j] + n].reshape(want[k][0].shape), want[k][0]), k
    assert L.rgrid_batch_texture_collect(m._h, boxes.ctypes.data, sm.ctypes.data, offs.ctypes.data, out.ctypes.data, total) == INVALID
    # the Python layer reports the same: too little room leaves the submit pending
    assert m.submit_texture_code([3, 5]) == OK
    rc, need = m.collect_texture_code(cap=3)
    assert rc == BUFFER and need == [(want[3][1], want[3][2], 0), (want[5][1], want[5][2], 2)]
    rc, got = m.collect_texture_code()
    assert rc == OK and TC.same_texture(got[0], want[3]) and TC.same_texture(got[1], want[5])


def test_refusals_launch_nothing_and_leave_the_handle_usable(oracle_lib):
    from reflector_ekf_slam_amd import fleet_match as M
    grids = TC.sweep_case()
    L = M._texture_lib()
    m = fleet(8, TC.SWEEP_MAX_CELLS)
    set_grids(m, grids[:4])                                                        # slots 4 .. 7 are not set
    want = [TC.oracle_texture(g) for g in grids[:4]]
    good = lambda: all(TC.same_texture(t, w) for t, w in zip(m.draw_textures(), want)) and len(m.draw_textures([2, 0])) == 2
    one = np.array([1], np.int32)
    nine = np.array([0] * 9, np.int32)
    refused = [lambda: L.rgrid_batch_texture_submit(m._h, None, 1), lambda: L.rgrid_batch_texture_submit(m._h, one.ctypes.data, -1),
               lambda: L.rgrid_batch_texture_submit(m._h, nine.ctypes.data, m.max_scans + 1),
               lambda: m.submit_texture_code([8]), lambda: m.submit_texture_code([-1]), lambda: m.submit_texture_code([1, 5]),
               lambda: m.submit_texture_code([0, 1, 2, 3, 4])]
    for k, call in enumerate(refused):
        assert call() == INVALID, k
        assert m.collect_texture_code() == (INVALID, [])                           # nothing is pending
        assert good(), k
    assert m.set_slots() == [0, 1, 2, 3]
    # one pending submit: a texture submit over a pending insert, an insert's collect over a pending texture submit
    scan = (1, np.array([0.1, 0.1], np.float32), np.array([[0.2, 0.3]], np.float32), None)
    inserted = IC.oracle_pair(grids[1], scan)
    assert m.submit_insert_code([scan]) == OK
    assert m.submit_texture_code([0]) == INVALID and m.collect_texture_code() == (INVALID, [])
    assert m.collect_insert_code() == (OK, [OK])                                   # ... and it was left pending
    want[1] = TC.oracle_texture((inserted[0], grids[1][1], (inserted[1][3], inserted[1][4])))
    assert good()
    assert m.submit_texture_code([3, 1]) == OK
    assert m.collect_insert_code() == (INVALID, []) and m.collect_code() == (INVALID, []) and m.collect_filter_code()[0] == INVALID
    assert m.submit_texture_code([0]) == INVALID and m.submit_insert_code([scan]) == INVALID
    assert m.GetGrid_code(0)[0] == INVALID and m.GetLimits_code(0)[0] == INVALID and m.SetGrid_code(0, *grids[0]) == INVALID
    rc, got = m.collect_texture_code()                                             # ... and it was left pending
    assert rc == OK and TC.same_texture(got[0], want[3]) and TC.same_texture(got[1], want[1])
    assert good()
    # count == 0 is a submit with nothing launched
    assert m.submit_texture_code([]) == OK and m.submit_texture_code([]) == INVALID
    assert m.collect_texture_code() == (OK, []) and m.collect_texture_code() == (INVALID, [])
    assert m.draw_textures([]) == [] and good()
    m.close()


def test_submap_textures_equal_the_map_builders(oracle_lib):
    from reflector_ekf_slam_amd.map_builder import MapBuilder, RangeData
    scans = TC.submap_scene()
    mb = MapBuilder(max_points=512, max_cells=TC.SUBMAP_MAX_CELLS)
    m = fleet(2, TC.SUBMAP_MAX_CELLS)
    origin = scans[0][0]
    n, res = TC.SUBMAP_N, float(np.float32(mb.options_.resolution))                 # CreateGrid (map_builder.cc:115-126)
    m.SetGrid(1, np.zeros((n, n), np.uint16), res, (float(origin[0]) + 0.5 * n * res, float(origin[1]) + 0.5 * n * res))
    where = (float(origin[0]), float(origin[1]))
    for org, ret, mis in scans:
        mb.InsertIntoSubmap(RangeData(org, ret, mis))
        assert m.insert([(1, org, ret, mis)]) == [OK]
        want = mb.ToSubmapTexture()
        got = m.submap_textures([1], [where])
        assert len(got) == 1 and set(got[0]) == set(want)
        for key in ("width", "height", "resolution", "slice_pose", "global_pose"):
            assert got[0][key] == want[key], (key, got[0][key], want[key])
        assert got[0]["cells"].shape == want["cells"].shape and np.array_equal(got[0]["cells"], want["cells"])
    assert want["width"] > TC.SUBMAP_N and np.count_nonzero(want["cells"]) > 2000
    mb._fe.close(); m.close()
