"""Cases of the downdate's multi-tile ranges, shared by tests/test_ekf_ranges_cpu.py (the table of forms, the FP64 floor, the
planted defects) and tests/test_ekf_ranges_gpu.py (dd_body of csrc/ekf_kernels.hip as k_downdate2, as k_dd_front and as the
queue-fed role inside k_mid, against the longdouble witness).

A workgroup of the downdate gets a RANGE of 64 x 64 tiles.  The shape sweep (tests/ekf_shape_cases.py, L <= 200) hands every
workgroup one tile on 256 CUs, so everything that concerns a longer range -- the rotation of the register blocks, the panel
that is re-fetched only when the row or column changes, the straight-line forms for 2, 3 and 4 tiles, the generic loop, class A
with two tiles, the pending Predict on a column-0 tile in the middle of a range -- is out of its reach.  The library has no hook
that lowers the CU budget; these cases reach each form through the state size, at the smallest tile count T that
tests/downdate_schedule.py finds for it on the device's CU count, and at the first n with T tile rows, n = 64 (T - 1) + 1.

A case is built with ekf_shape_cases.Builder on a larger lattice: a dense SPD state (fleet_cases.dense_spd, the sweep's scale
range), a non-zero vt (so a Predict is pending on column 0), scans 0.1 s apart, both association margins of every observation
asserted at generation.  Two scans:
    scan 1   K observations of the case's matched set              nothing pending
    scan 2   another matched set of the same size                  scan 1's downdate runs in the form the call pattern selects
                                                                   (tests/test_ekf_ranges_gpu.py), scan 2's own at the final read
The matched sets hold reflector 0, reflector L - 1 (n is odd and the last tile row holds ONE row: its x is the last row of tile
row T - 2, its y is the last, partly filled tile row), the 16-row straddler (6), the 64-row straddler (30) and L - 2.

On 256 CUs (k_downdate2: all of them; k_dd_front with K = 8: 248 for the schedule, which moves the switch to sub = 2 down to
T = 31 -- `form_front` of the case says what that pattern runs):
    form                                                       T    L     n
    sub1_range2   sub = 1, longest range 2                      23   703   1409     also with K = 16, 24, 32 (k-chunks 32, 48, 64)
    sub1_range3   sub = 1, longest range 3                      31   959   1921     (k_dd_front: sub2_range3)
    sub2_range3   sub = 2, ranges 2 and 3, class A of two       32   991   1985
    sub2_range4   sub = 2, longest range 4                      38   1183  2369     the last straight-line form
    sub2_range5   sub = 2, longest range 5                      43   1343  2689     the first trip of the generic loop
and one growing case at T = 31: cap = L + 8, auto-grow off, scan 1 with 5 matched and N2 = 3 new observations (K = 8); the host
plans from its bound of n and the kernel may derive the schedule itself (dd_sub = 0), k_augment's rows are appended behind
multi-tile ranges, and scan 2 matches what scan 1 appended.

K = 8 (16 rows, k-chunk 16) keeps the longdouble witness to about 16 n^2 multiply-adds per product; its dense products take
0.5 - 4 s per case, so the witness of the sweep is used as it is (no gathering variant)."""
from __future__ import annotations

from types import SimpleNamespace as NS

from tests import downdate_schedule as DS
from tests import ekf_shape_cases as EC
from tests.ekf_shape_cases import Builder, matched_sets
from tests.fleet_cases import DIFF, OMNI

L_MAX = 1500
N_CU_PINNED = 256
# form -> (T, L) on 256 CUs with every CU in the schedule (k_downdate2); pinned by tests/test_ekf_ranges_cpu.py
TABLE_256 = {"sub1_range2": (23, 703), "sub1_range3": (31, 959), "sub2_range3": (32, 991), "sub2_range4": (38, 1183), "sub2_range5": (43, 1343)}
K_DEFAULT = 8
K_CHUNKS = (16, 24, 32)                      # further K of the sub1_range2 case: k-chunks 32, 48 (both with the transpose scratch) and 64
GROW_FORM, GROW_MM, GROW_N2 = "sub1_range3", 5, 3

# ---- the FP64 noise floor of these cases -------------------------------------------------------------------------------------
# Measured by tests/test_ekf_ranges_cpu.py::test_fp64_floor exactly as tests/test_ekf_shapes_cpu.py::test_fp64_floor does: the larger
# error of oracle/ekf_oracle.c (its structured path, the binding's default: O(n^2 m)) and oracle/ekf_numpy.py (dense, literal)
# against the longdouble witness over both scans of every case, as max|dsigma| / max|sigma_ref| and max|dmu| / max(1, max|mu_ref|).
# Recorded = measured, rounded up to two digits; the test fails when a re-measurement exceeds it or falls below half of it.
FP64_FLOOR_SIGMA = 2.2e-11    # measured 2.126e-11
FP64_FLOOR_MU = 2.1e-16       # measured 2.051e-16
FP64_FLOOR_SIGMA_CASE = "range_grow_T31_L959_MM5_N3_diff scan 1 (oracle)"
FP64_FLOOR_MU_CASE = "range_grow_T31_L959_MM5_N3_diff scan 1 (oracle)"

SUITE = NS(name="ranges", floor_sigma=FP64_FLOOR_SIGMA, floor_mu=FP64_FLOOR_MU, witnesses={"witness": EC.witness_of})


def L_of(T):
    """The first state with T tile rows: n = 3 + 2 L is odd, so n = 64 (T - 1) + 1."""
    return (DS.DT * (T - 1) + 1 - 3 + 1) // 2


def lattice_of(L):
    g = 17
    while g * g < L + 128:
        g += 1
    return g


def table(n_cu):
    """form -> (T, L) for a device of n_cu CUs: the search of tests/downdate_schedule.py (None where the form does not exist)."""
    out = {}
    for form in DS.FORMS:
        T = DS.smallest_T(form, DS.slots_of(n_cu, 0))
        out[form] = None if T is None else (T, L_of(T))
    return out


def _m(model):
    return "diff" if model == DIFF else "omni"


def _tags(n_cu, T, K):
    """What the patterns of tests/test_ekf_ranges_gpu.py run scan 1's downdate as, from the restatement."""
    n = DS.DT * (T - 1) + 1
    # the host decides on the one-launch form with its own K as the bound of the front end behind the mid role; the launch that
    # carries scan 1's downdate is scan 2's, behind which the host holds no scan: no speculative front end, K_front = 0
    fits = DS.role_wgs(n_cu, n, K)[2]
    wgs, items, _ = DS.role_wgs(n_cu, n, 0)
    return dict(T=T, n_cu=n_cu, slots_alone=DS.slots_of(n_cu, 0), slots_front=DS.slots_of(n_cu, K),
                form_alone=DS.form_of(T, DS.slots_of(n_cu, 0)), form_front=DS.form_of(T, DS.slots_of(n_cu, K)),
                role_wgs=wgs, role_items=items, one_launch_fits=fits, second_item=fits and items > wgs)


def range_case(i, form, T, K, n_cu):
    L = L_of(T)
    assert L <= L_MAX, (form, T, L)
    model = DIFF if i % 2 == 0 else OMNI
    b = Builder(L, model, 9700 + i, cap=L, grid=lattice_of(L))
    b.cond = {}
    first, second = matched_sets(L, K, b.rng)
    b.scan(first)
    b.scan(second)
    b.sets = (first, second, None)
    c = b.case(f"range_{form}_T{T}_L{L}_K{K}_{_m(model)}", "range", K=K, MM=K, N2=0, form=form, **_tags(n_cu, T, K))
    assert c.n == DS.DT * (T - 1) + 1 and DS.tiles_of(c.n) == T and DS.tiles_of(c.n - 1) == T - 1
    return c


def growing_range_case(i, T, n_cu):
    L = L_of(T)
    model = DIFF if i % 2 == 0 else OMNI
    MM, N2 = GROW_MM, GROW_N2
    b = Builder(L, model, 9700 + i, cap=L + 8, grid=lattice_of(L + 8))
    b.cond = {}
    first, second = matched_sets(L, MM, b.rng)
    b.scan(first, N2)
    assert b.L() == L + N2
    # the grown state: scan 2 matches the last reflector scan 1 appended and the first one (as ekf_shape_cases.four_scans does)
    pos = MM - 1
    for j in (L + N2 - 1, L):
        if j not in second:
            second[pos] = j
            pos -= 1
    b.scan(second)
    b.sets = (first, second, None)
    K = MM + N2
    c = b.case(f"range_grow_T{T}_L{L}_MM{MM}_N{N2}_{_m(model)}", "range_grow", K=K, MM=MM, N2=N2, form=GROW_FORM, **_tags(n_cu, T, K))
    # the host plans from its bound 3 + 2 cap, the kernel derives (lo, x, sub) from its own T and the grid it finds
    c.T_host = DS.tiles_of(3 + 2 * c.cap)
    c.T_grown = DS.tiles_of(3 + 2 * (L + N2))
    return c


_cases = {}


def specs(n_cu=N_CU_PINNED):
    """-> [(name, a function that builds the case)] for a device of n_cu CUs, without building a state.  A form that no T with
    L <= L_MAX has is an error (the GPU test fails, it does not skip)."""
    tab = table(n_cu)
    missing = [f for f, v in tab.items() if v is None or v[1] > L_MAX]
    assert not missing, f"no state of L <= {L_MAX} reaches {missing} on {n_cu} CUs: {tab}"
    todo = [(i, form, tab[form][0], K_DEFAULT) for i, form in enumerate(DS.FORMS)]
    todo += [(5 + i, "sub1_range2", tab["sub1_range2"][0], K) for i, K in enumerate(K_CHUNKS)]
    out = [(f"range_{form}_T{T}_L{L_of(T)}_K{K}_{_m(i % 2)}", lambda i=i, form=form, T=T, K=K: range_case(i, form, T, K, n_cu))
           for i, form, T, K in todo]
    T = tab[GROW_FORM][0]
    out.append((f"range_grow_T{T}_L{L_of(T)}_MM{GROW_MM}_N{GROW_N2}_{_m(0)}", lambda: growing_range_case(8, T, n_cu)))
    return out


def names(n_cu=N_CU_PINNED):
    return [name for name, _ in specs(n_cu)]


def case_named(name, n_cu=N_CU_PINNED):
    """One case, built when first asked for and kept."""
    if (n_cu, name) not in _cases:
        c = dict(specs(n_cu))[name]()
        assert c.name == name, (c.name, name)
        _cases[(n_cu, name)] = c
    return _cases[(n_cu, name)]


def cases(n_cu=N_CU_PINNED):
    return [case_named(name, n_cu) for name in names(n_cu)]
