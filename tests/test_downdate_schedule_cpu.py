"""The tile schedule of k_downdate2 (csrc/ekf_kernels.hip), restated in Python: for every tile count T and CU count the
workgroups' tile lists must cover the lower triangle {(I, J): I >= J} exactly once, a class-A workgroup must end on its
diagonal tile, class B must hold none, and a workgroup never gets more tiles than the host planned.  The HIP code is the
product; this mirrors its index arithmetic (host: rekf_launch_downdate, device: the classA / tri_IJ / cursor logic) so that an
off-by-one there shows up without a GPU.  The GPU suite checks the numbers; this checks the bookkeeping for sizes the GPU
tests do not reach (T up to 64 = n up to 4096).  The restatement itself is tests/downdate_schedule.py, shared with the range
cases (tests/ekf_range_cases.py), whose GPU tests check the numbers of multi-tile ranges."""
import pytest

from tests.downdate_schedule import device_tiles, host_plan, kernel_plan, queue_items


@pytest.mark.parametrize("slots", [256, 304, 64, 239, 223, 199])     # (the odd ones: the downdate as a ROLE of k_mid's grid, 256 - K - mid workgroups)
def test_every_lower_triangle_tile_exactly_once(slots):
    for T in range(1, 65):
        grid, lo, x, sub = host_plan(T, slots)
        seen = {}
        busy = 0
        for b in range(grid):
            tl = device_tiles(T, grid, lo, x, sub, b)
            busy += bool(tl)
            assert len(tl) <= max(lo + 1, 2), (T, b, tl)
            diag = [t for t in tl if t[0] == t[1]]
            assert len(diag) <= 1 and (not diag or tl[-1] == diag[0]), (T, b, tl)      # the diagonal tile comes last
            for t in tl:
                assert t not in seen, (T, t, b, seen[t])
                seen[t] = b
        want = {(i, j) for i in range(T) for j in range(i + 1)}
        assert set(seen) == want, (T, sorted(want - set(seen))[:5], sorted(set(seen) - want)[:5])
        if T >= 24 and slots >= T + 8:
            assert busy >= min(slots, len(want) // 2) - 8, (T, busy)                   # no CU is left idle once there is work for all


def test_host_bound_of_T_may_exceed_the_kernels():
    """The host sizes the grid from an upper bound of n (T_host >= T_kernel) and then passes no schedule: the kernel derives
    (lo, x, sub) from its own T and the grid it finds; its own T must still be covered exactly once."""
    for T_k in range(1, 40):
        for T_h, slots in [(T_k, 256), (T_k + 1, 256), (T_k + 7, 256), (2 * T_k, 256), (T_k + 1, 223), (T_k + 3, 199)]:
            grid, _, _, _ = host_plan(T_h, slots)
            lo, x, sub = kernel_plan(T_k, grid)
            seen = set()
            for b in range(grid):
                for t in device_tiles(T_k, grid, lo, x, sub, b):
                    assert t not in seen
                    seen.add(t)
            assert seen == {(i, j) for i in range(T_k) for j in range(i + 1)}, (T_k, T_h)


def test_the_queue_hands_every_tile_out_exactly_once():
    for T in range(1, 70):
        seen = set()
        for tl in queue_items(T):
            assert 1 <= len(tl) <= 3
            diag = [t for t in tl if t[0] == t[1]]
            assert len(diag) <= 1 and (not diag or tl[-1] == diag[0])      # a diagonal tile ends its item (the mirror reuses the panels' LDS)
            for t in tl:
                assert t not in seen, (T, t)
                seen.add(t)
        assert seen == {(i, j) for i in range(T) for j in range(i + 1)}, T
