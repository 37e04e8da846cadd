"""The grid's write path on the CPU: oracle/grid_oracle.c (GrowAsNeeded + Insert, the text the kernels were written from) against
the independent witnesses of tests/witness/grid_witness.py on every case of tests/grid_write_cases.py; that each family reaches
the boundary it is named after, from the witness' own intermediate values; and the teeth -- the convention transposed in one place
is seen on every non-square map and growth grid, and cannot be seen on a square one.  Every comparison is exact."""
from __future__ import annotations

import numpy as np
import pytest

from tests import grid_write_cases as WC
from tests.witness import grid_witness as W

S = W.S


@pytest.mark.parametrize("family", list(WC.FAMILIES))
def test_oracle_equals_witness(oracle_lib, family):
    """oracle_grow == grow_witness in cells, maxima and offsets, oracle_insert == insert_witness, step by step along every chain:
    each side runs its own chain, so the pair is compared too; every point is judged inside by both."""
    chains = WC.FAMILIES[family]()
    assert (len(chains), sum(len(c.steps) for c in chains)) == WC.SIZES[family]
    assert [c.slot for c in chains] == list(range(len(chains))) and len({c.name for c in chains}) == len(chains)
    for ch in chains:
        want, got = WC.witness_chain(ch), WC.oracle_chain(ch)
        for k, ((wc, wl, wo), (oc, ol, oo)) in enumerate(zip(want, got)):
            assert ol == wl and oo == wo, (ch.name, k, ol, wl, oo, wo)
            assert np.array_equal(oc, wc), WC.diff_report(f"{ch.name} step {k}", oc, wc)
            assert (wc < W.MARK).all(), (ch.name, k)
            before = WC.grid_before(ch, k)[0]
            if ch.grow:                                                            # the growth alone, before the insert covers it
                from oracle.binding import oracle_grow
                _, origin, ret, mis = ch.steps[k]
                g_o, g_w = oracle_grow(*WC.grid_before(ch, k), origin, ret, mis), W.grow_witness(*WC.grid_before(ch, k), origin, ret, mis)
                assert np.array_equal(g_o[0], g_w[0]) and tuple(g_o[1]) == tuple(g_w[1]) and tuple(g_o[2]) == tuple(g_w[2]) == wo, (ch.name, k)
            n = ch.steps[k][2].shape[0] + (0 if ch.steps[k][3] is None else ch.steps[k][3].shape[0])
            changed = wc.shape != before.shape or not np.array_equal(wc, before)
            assert changed == (n > 0), (ch.name, k, n)


def test_counts_are_the_listed_counts():
    got = [(s[2].shape[0], 0 if s[3] is None else s[3].shape[0]) for s in (c.steps[0] for c in WC.counts())]
    assert tuple(got) == WC.COUNTS
    rays = [a + b for a, b in got]
    for edge in (4, 16, 256, 1024):                                                # waves of kg_rays and kgb_insert, threads of kg_ends and kgb_insert
        assert {edge - 1, edge, edge + 1} <= set(rays), edge
    assert all((c.grid[0] == 0).all() == (k % 2 == 0) for k, c in enumerate(WC.counts()))


def test_thin_rays_cross_a_pixel_border():
    ch = WC.thin()[0]
    origin, ends = WC.super_of(ch.grid, ch.steps[0])
    assert origin == WC.THIN_ORIGIN and origin[0] % S == S - 1 and origin[1] % S == 0
    assert len(ends) == 401 and ends[200] == origin                                # the zero-length ray
    assert sum(abs(ex - origin[0]) <= 3 for ex, _ in ends[:200]) == 200 and sum(abs(ey - origin[1]) <= 3 for _, ey in ends[201:]) == 200
    shapes = WC.ray_shapes(ch.grid, ch.steps[0])
    two_columns = [s for s in shapes if s[0] and s[1] <= 3]
    assert len(two_columns) >= 50 and all(s[2] == 2 for s in two_columns)
    assert {s[1] for s in two_columns} == {1, 2, 3}
    assert any(ey // S != origin[1] // S for _, ey in ends[201:])                  # thin in y across a pixel-row border too
    assert shapes[200][2:] == (1, 1)


def test_border_ends_lie_in_the_listed_sub_pixels():
    ch = WC.border()[0]
    ny, nx = ch.grid[0].shape
    _, ends = WC.super_of(ch.grid, ch.steps[0])
    want = [(ix, iy) for ix in WC.border_values(nx) for iy in WC.border_values(ny)]
    assert len(want) == 49 and ends[:49] == want and ends[49:] == want[::-1]
    assert {0, nx * S - 1} <= {e[0] for e in ends} and {0, ny * S - 1} <= {e[1] for e in ends}


def test_ties_lie_on_borders_corners_and_centres():
    ny, nx, res, (mx, my) = WC.TIES_MAP
    for slot, ch in enumerate(WC.ties()):
        _, origin, ret, mis = ch.steps[0]
        assert ret.shape[0] == WC.TIES_RETURNS and ret.shape[0] + mis.shape[0] == (2 * ny - 1) * (2 * nx - 1)
        pts = np.concatenate([ret, mis]).astype(np.float64)
        half = np.stack([(mx - pts[:, 0]) / (res / 2), (my - pts[:, 1]) / (res / 2)], 1)
        assert np.array_equal(half, np.rint(half)) and len({tuple(h) for h in half}) == pts.shape[0]      # every node once, exactly
        assert (half[:, 0] % 2 == 0).sum() > 1000 and (half.sum(1) % 2 == 1).sum() > 1000
        o = np.array([(mx - float(origin[0])) / (res / 2), (my - float(origin[1])) / (res / 2)])
        assert np.array_equal(o % 2, [0, 0] if slot == 0 else [1, 1])               # a cell corner, a cell centre


def test_long_rays_exceed_one_pass_of_lanes_and_two_of_columns():
    tall, wide = [], []
    for ch in WC.long():
        shapes = WC.ray_shapes(ch.grid, ch.steps[0])
        ny, nx = ch.grid[0].shape
        (bx, by), ends = WC.super_of(ch.grid, ch.steps[0])
        assert bx // S in (0, nx - 1) and by // S in (0, ny - 1)                   # the origin's corner cell
        assert any(ex == bx and abs(ey - by) > (ny - 2) * S for ex, ey in ends) and any(ey == by and abs(ex - bx) > (nx - 2) * S for ex, ey in ends)
        assert any(s[2] == nx and s[3] >= 1 and abs(ey - by) > (ny - 2) * S for s, (ex, ey) in zip(shapes, ends))     # corner to corner
        tall += [s for s in shapes if s[0] and s[1] <= 3 and s[3] > 64]             # X0 != X1, one column of more than 64 rows
        wide += [s for s in shapes if s[2] > 128]
    assert len(tall) >= 12 and {s[1] for s in tall} == {1, 2, 3} and len(wide) >= 4 * 6
    assert sorted({ch.grid[0].shape for ch in WC.long()}) == [(40, 150), (150, 40)]


def test_growth_reaches_the_factors_and_the_chunk_boundaries():
    chains = WC.growth()
    assert sorted({c.grid[0].size for c in chains}) == sorted({33 * 57, 8190, 8192, 8281, 16512})
    assert {8190, 8192, 8281} == {c.grid[0].size for c in chains if abs(c.grid[0].size - WC.GROW_CHUNK) < 100}
    factors, largest = {}, 0
    for ch in chains:
        first, total = set(), 1
        now = ch.grid[0].shape
        for cells, lim, offset in WC.witness_chain(ch):
            f = cells.shape[0] // now[0]
            assert f > 1 and cells.shape == (f * now[0], f * now[1])                # every scan of the family grows
            total *= f
            first.add(f)
            now = cells.shape
            largest = max(largest, cells.size)
        factors.setdefault(ch.grid[0].shape, set()).update(first | {total})
    assert all({2, 4} <= f for f in factors.values())
    assert [shape for shape, f in factors.items() if 8 in f] == [(33, 57), (57, 33)]
    assert largest == WC.GROWTH_MAX_CELLS
    moved = {c.size for ch in chains for c, _, _ in WC.witness_chain(ch)[:-1]}     # cells a SECOND growth moves: many chunks
    assert max(moved) > 8 * WC.GROW_CHUNK
    offsets = {o for ch in chains for _, _, o in WC.witness_chain(ch)}
    assert len(offsets) > 12 and all(ox > 0 and oy > 0 for ox, oy in offsets)


def test_loop_grows_twice_and_matches(oracle_lib):
    from oracle.binding import oracle_match
    ch = WC.loop()[0]
    steps = WC.witness_chain(ch)
    assert [s[0].shape for s in steps] == [(120, 200), (240, 400), (240, 400)] and steps[-1][0].size <= WC.LOOP_MAX_CELLS
    cells, lim, _ = steps[-1]
    assert lim[3] != lim[4] and np.count_nonzero(cells) > 5000
    _, prediction, pts = WC.loop_match_scan()
    w = W.match_witness(prediction, pts, cells, lim[2], (lim[3], lim[4]), angular_search_window=WC.MATCH_ANGULAR_WINDOW)
    score, pose, best, _ = oracle_match(prediction, pts, cells, lim[2], (lim[3], lim[4]))
    assert tuple(best) == w[2] and np.float32(score) == w[0] and np.abs(pose - np.array(w[1])).max() < 1e-12
    assert w[0] > 0.3 and np.abs(np.array(w[1]) - WC.LOOP_TRUE).max() < 0.11     # a real match: near the true pose, not a flat map


# ---- teeth ------------------------------------------------------------------------------------------------------------------
def _insert(ch, mutant=None):
    _, origin, ret, mis = ch.steps[0]
    return W.insert_witness(*ch.grid, origin, ret, mis, mutant=mutant)


@pytest.mark.parametrize("mutant", W.MUTANTS)
def test_every_non_square_map_sees_each_insert_mutant(mutant):
    for ch in WC.geometry()[:4]:
        want = WC.witness_chain(ch)[0][0]
        assert np.array_equal(_insert(ch), want)
        got = _insert(ch, mutant)
        assert got is None or (got.shape == want.shape and not np.array_equal(got, want)), (ch.name, mutant)
    for ch in (c for family in ("thin", "border", "ties", "long") for c in WC.FAMILIES[family]()):     # the edge families' maps too
        got = _insert(ch, mutant)
        assert got is None or not np.array_equal(got, WC.witness_chain(ch)[0][0]), (ch.name, mutant)


def test_every_non_square_growth_grid_sees_the_growth_mutant():
    seen = {}
    for ch in WC.growth():
        _, origin, ret, mis = ch.steps[0]
        cells, new_max, offset = W.grow_witness(*ch.grid, origin, ret, mis)
        m_cells, m_max, m_offset = W.grow_witness(*ch.grid, origin, ret, mis, mutant="maxima")
        assert np.array_equal(m_cells, cells) and m_offset == offset
        # the two offsets are what the mutant swaps: 91 x 91 never tells, and one doubling of 90 x 91 or 128 x 129 does not
        # either (floor(90 / 2) == floor(91 / 2)) -- their chains of two doublings do
        differs = m_max[0] != new_max[0] and m_max[1] != new_max[1]
        assert differs == (offset[0] != offset[1]) and (differs or m_max == new_max), ch.name
        seen.setdefault(ch.grid[0].shape, []).append(differs)
        for other in ("bounds", "stride"):
            assert W.grow_witness(*ch.grid, origin, ret, mis, mutant=other)[1] == new_max
    assert len(seen) == len(WC.GROWTH_GRIDS)
    for (ny, nx), differs in seen.items():
        assert any(differs) == (ny != nx), (ny, nx)
    assert all(seen[(33, 57)]) and all(seen[(57, 33)]) and all(seen[(64, 128)])


def test_the_square_control_cannot_tell():
    """120 x 120 with maxima (6, 6), like the one committed witness fixture of the inserter (160 x 160, (4, 4)): every mutant
    computes the convention itself."""
    ch = WC.geometry()[4]
    assert ch.grid[0].shape == (120, 120) and ch.grid[2] == (6.0, 6.0)
    want = WC.witness_chain(ch)[0][0]
    assert not np.array_equal(want, ch.grid[0])
    for mutant in W.MUTANTS:
        assert np.array_equal(_insert(ch, mutant), want), mutant
    far = np.array([[9.5, 1.0], [-1.0, -13.0]], np.float32)
    base = W.grow_witness(*ch.grid, (0.5, 0.5), far)
    assert base[0].shape == (480, 480)
    mutated = W.grow_witness(*ch.grid, (0.5, 0.5), far, mutant="maxima")
    assert mutated[1] == base[1] and mutated[2] == base[2] and np.array_equal(mutated[0], base[0])


# ---- the closed form of the ray walk, and which family sees which slip in it --------------------------------------------------
SLIPS = ("corner", "first_pixel", "last_pixel", "one_pass_of_rows", "two_passes_of_columns")


def closed_form_pixels(bx, by, ex, ey, slip=None):
    """The arithmetic kg_rays and kgb_insert replace the reference's sub-pixel recurrence by (csrc/rgrid.hip, the comment above
    kg_rays), restated with Python integers; `slip`: one plausible error in it.  "corner": ceil(a / den) as a / den + 1, wrong
    where a ray passes exactly through a pixel corner; "first_pixel" / "last_pixel": the half sub-pixel of the first column left
    out, the last column taken as a full one; "one_pass_of_rows": a column's rows beyond the first 64 are lost;
    "two_passes_of_columns": the columns beyond the first 128 are lost."""
    if bx > ex:
        bx, by, ex, ey = ex, ey, bx, by
    X0, X1 = bx // S, ex // S
    lanes = 64 if slip == "one_pass_of_rows" else None
    if X0 == X1:
        return [(X0, y) for y in range(min(by, ey) // S, max(by, ey) // S + 1)][:lanes]
    dx, dy = ex - bx, ey - by
    den = 2 * S * dx
    a0 = (2 * (by % S) + 1) * dx + (by // S) * den
    first_pixel = 2 * S - 2 * (bx % S) - (0 if slip == "first_pixel" else 1)
    last_pixel = 2 * S if slip == "last_pixel" else 2 * (ex % S) + 1
    a_out = lambda X: a0 + dy * (first_pixel + 2 * S * (X - X0) + (last_pixel - 2 * S if X == X1 else 0))
    fdiv = lambda a: a // den
    cdiv = (lambda a: a // den + 1) if slip == "corner" else (lambda a: (a + den - 1) // den)
    out = []
    for X in range(X0, min(X1, X0 + 127) + 1 if slip == "two_passes_of_columns" else X1 + 1):
        if dy > 0:
            r_in, r_out, step = (by // S if X == X0 else fdiv(a_out(X - 1))), cdiv(a_out(X)) - 1, 1
        else:
            r_in, r_out, step = (by // S if X == X0 else cdiv(a_out(X - 1)) - 1), fdiv(a_out(X)), -1
        cnt = max(1, (r_out - r_in) * step + 1)
        out += [(X, r_in + step * k) for k in range(cnt)][:lanes]
    return out


def test_the_closed_form_is_the_walk_and_every_slip_is_seen_by_its_family():
    """Without a slip the closed form gives the witness' pixels on every ray of the edge families; each slip changes the pixels
    of some ray, and the two slips that need a long ray are seen by the family built for them."""
    seen = {slip: set() for slip in SLIPS}
    for family in ("geometry", "thin", "border", "ties", "long"):
        for ch in WC.FAMILIES[family]():
            (bx, by), ends = WC.super_of(ch.grid, ch.steps[0])
            for ex, ey in ends:
                want = set(W.ray_pixels(bx, by, ex, ey))
                assert set(closed_form_pixels(bx, by, ex, ey)) == want, (ch.name, (bx, by), (ex, ey))
                for slip in SLIPS:
                    if set(closed_form_pixels(bx, by, ex, ey, slip)) != want:
                        seen[slip].add(family)
    assert seen["corner"] >= {"ties"} and seen["first_pixel"] >= {"thin", "long"} and seen["last_pixel"] >= {"thin", "long"}, seen
    # more than 64 rows need the 150 x 40 map: the long family by construction, a random ray of the geometry family by chance;
    # more than 128 columns are also reached on the 40 x 300 map of thin and border
    assert "long" in seen["one_pass_of_rows"] and seen["one_pass_of_rows"] <= {"long", "geometry"}, seen
    assert "long" in seen["two_passes_of_columns"], seen
