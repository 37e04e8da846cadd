"""rfleet_get_reflectors, what can be checked without a GPU: the C ABI and its refusals that come before any HIP call, the lazy
loader, the saved map's text writer against the bytes save_map_txt wrote before it was split out, the coverage of the cases of
tests/fleet_reflector_cases.py, and the FP64 floor that sets the bound of the GPU test's eigen-solver comparison."""
from __future__ import annotations

import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from reflector_ekf_slam_amd import ekf_slam as E
from reflector_ekf_slam_amd import fleet
from reflector_ekf_slam_amd.ekf_slam import loaded_map_rows, reflector_map_txt
from reflector_ekf_slam_amd.fleet import _reflectors_lib
from tests import fleet_reflector_cases as RC
from tests.fleet_harness import HEADER

# The largest |R diag(l0, l1) R^T - block| / max|block| of oracle/ekf_oracle.c's marker ellipses over the positive definite crafted
# blocks of fleets A and B (test_witness_floor measures it): what FP64 leaves of a block after the ellipse's sqrt, atan2, cos and
# sin.  The GPU's rows are held to GPU_FACTOR x this.
ELLIPSE_FLOOR = 6.4e-16
GPU_FACTOR = 16.0


def test_header_declares_the_call_and_keeps_the_abi_version():
    text = open(HEADER).read()
    assert re.search(r"int\s+rfleet_get_reflectors\s*\(\s*rfleet_t\s*\*\s*f\s*,\s*const\s+int\s*\*\s*members\s*,\s*int\s+count\s*,[^;]*"
                     r"int\s*\*\s*counts[^;]*double\s*\*\s*ellipses5\s*,\s*double\s*\*\s*xy2\s*,\s*double\s*\*\s*cov4\s*,\s*long\s+cap_rows\s*\)\s*;", text)
    assert re.search(r"#define\s+RFLEET_ABI_VERSION\s+2\b", text)
    scope = text[text.index("Deliberately OUT OF SCOPE"):]
    scope = scope[:scope.index("\n *\n")]
    assert "marker ellipses" not in scope
    for kept in ("a map per member", "auto-grow", "PredictState's landmark part", "wider than RFLEET_MAX_OBS"):
        assert kept in " ".join(scope.replace("\n *", " ").split()), kept
    assert fleet.rfleet().rfleet_abi_version() == 2 == fleet.RFLEET_ABI_VERSION


def test_library_exports_the_call():
    from reflector_ekf_slam_amd import _lib as base
    path = base.lib_path("librfleet.so")
    assert hasattr(C.CDLL(path), "rfleet_get_reflectors")
    names = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT rfleet_get_reflectors\b", names)


def test_refusals_come_before_any_hip_call():
    """Every refusal that rfleet.h places before any HIP call and before the handle is read, with its code, on a machine without a
    device.  The handle is a dummy that the library must not look into before it has refused."""
    L = _reflectors_lib()
    text = open(HEADER.replace("rfleet.h", "rekf.h")).read()
    INVALID = int(re.search(r"REKF_ERR_INVALID\s*=\s*(-?\d+)", text).group(1))
    assert INVALID < 0
    counts = np.full(4, 77, np.int32)
    out = np.full(40, -5.0)
    mem = np.arange(4, dtype=np.int32)
    dummy = C.c_void_p(1)
    call = L.rfleet_get_reflectors
    assert call(None, mem.ctypes.data, 4, counts.ctypes.data, out.ctypes.data, None, None, 8) == INVALID          # a null handle
    assert call(None, None, 0, None, None, None, None, 0) == INVALID
    assert call(dummy, mem.ctypes.data, -1, counts.ctypes.data, out.ctypes.data, None, None, 8) == INVALID        # count < 0
    assert call(dummy, mem.ctypes.data, 4, None, out.ctypes.data, None, None, 8) == INVALID                       # no counts
    assert call(dummy, mem.ctypes.data, 4, counts.ctypes.data, out.ctypes.data, None, None, -1) == INVALID        # cap_rows < 0
    for which in range(3):                                                # an output given with no room for a row
        ptrs = [None, None, None]
        ptrs[which] = out.ctypes.data
        assert call(dummy, mem.ctypes.data, 4, counts.ctypes.data, *ptrs, 0) == INVALID
        assert call(dummy, None, 4, counts.ctypes.data, *ptrs, 0) == INVALID
    assert (counts == 77).all() and (out == -5.0).all()


def test_the_binding_looks_the_call_up_lazily(monkeypatch):
    """rfleet() does not ask for the new symbol (a library of ABI version 2 without it keeps serving everything else, the map calls
    included); _reflectors_lib() does, once, and raises LibraryMissing when it is absent."""
    from reflector_ekf_slam_amd import _lib as base

    real = fleet.rfleet()

    class Old:
        """A library handle of ABI version 2 from before rfleet_get_reflectors."""
        def __getattr__(self, name):
            if name == "rfleet_get_reflectors":
                raise AttributeError(name)
            return getattr(real, name)

    old = Old()
    monkeypatch.setattr(fleet._reflectors_lib, "ready", None)
    monkeypatch.setattr(fleet._map_lib, "ready", None)
    monkeypatch.setattr(fleet.rfleet, "ready", old)
    with pytest.raises(base.LibraryMissing) as e:
        fleet._reflectors_lib()
    assert "rfleet_get_reflectors" in str(e.value) and "librfleet.so" in str(e.value) and fleet._reflectors_lib.ready is None
    assert fleet._map_lib() is old and fleet.rfleet().rfleet_abi_version() == 2          # every other call keeps working
    assert fleet.rfleet().rfleet_size(None, None, None) < 0
    monkeypatch.setattr(fleet._map_lib, "ready", None)
    monkeypatch.setattr(fleet.rfleet, "ready", real)
    got = fleet._reflectors_lib()
    assert got is real and fleet._reflectors_lib.ready is real and got.rfleet_get_reflectors.argtypes is not None
    for name in ("marker_ellipses", "landmarks", "save_map_txt", "reflectors"):
        assert callable(getattr(fleet.ReflectorEKFSLAMFleet, name)), name
    assert callable(fleet.FleetMember.marker_ellipses)
    assert "fleet.submit -> marker_ellipses" in " ".join(fleet.__doc__.split())


# ---- the saved map's text -------------------------------------------------------------------------------------------------------
def _save_map_txt_before_the_split(path, state, loaded=None, reference_bytes=False):
    """ekf_slam.save_map_txt as it stood before reflector_map_txt was split out of it, word for word: the witness of the bytes."""
    pts, covs = [], []
    n_loaded = 0
    if loaded is not None:
        for p, c in zip(loaded.reflector_map_, loaded.reflector_map_coviarance_):
            pts.append((float(np.float32(p[0])), float(np.float32(p[1]))))
            covs.append(np.asarray(c, dtype=np.float64).reshape(4))
            n_loaded += 1
    L = (state.mu.shape[0] - 3) // 2
    for j in range(L):
        pts.append((state.mu[3 + 2 * j], state.mu[4 + 2 * j]))
        covs.append(state.sigma[3 + 2 * j: 5 + 2 * j, 3 + 2 * j: 5 + 2 * j].reshape(4))
    if not reference_bytes:
        with open(path, "w") as f:
            f.write(",".join(f"{v:.17g}" for p in pts for v in p) + "\n")
            f.write(",".join(f"{v:.17g}" for c in covs for v in c) + "\n")
        return

    def line(groups):
        old = ",".join("%g" % v for g in groups[:n_loaded] for v in g)
        new = ",".join("%g" % v for g in groups[n_loaded:] for v in g)
        return old + (("," + new) if L > 0 else "")
    with open(path, "w") as f:
        f.write(line(pts) + "\n")
        f.write(line(covs) + "\n")


@pytest.mark.parametrize("reference_bytes", [False, True])
@pytest.mark.parametrize("L,M", [(0, 0), (5, 0), (0, 4), (5, 4)], ids=["nothing", "reflectors_only", "map_only", "both"])
def test_reflector_map_txt_is_todays_save_map_txt(L, M, reference_bytes, tmp_path):
    m = RC.member(L, 31 + L)
    state = E.State(m.t, m.mu, RC.mirrored(m.sigma))
    rng = np.random.default_rng(8)
    loaded = E.Map(rng.uniform(-30, 30, size=(M, 2)).astype(np.float32), rng.uniform(0.001, 0.1, size=(M, 2, 2))) if M else None
    a, b = str(tmp_path / "before.txt"), str(tmp_path / "now.txt")
    _save_map_txt_before_the_split(a, state, loaded, reference_bytes)
    E.save_map_txt(b, state, loaded, reference_bytes)
    want = open(a, "rb").read()
    assert open(b, "rb").read() == want and want.count(b"\n") == 2
    pts, covs = loaded_map_rows(loaded)
    xy, cov = RC.expected_landmarks(m)
    got = reflector_map_txt(pts + list(xy), covs + list(cov.reshape(-1, 4)), M, reference_bytes)
    assert isinstance(got, bytes) and got == want
    if reference_bytes:                                    # the reference's leading comma in front of the filter's own reflectors
        assert want.startswith(b",") == (L > 0 and M == 0)


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def test_cases_cover_what_they_claim():
    A, B = RC.fleet_a(), RC.fleet_b()
    assert [m.L for m in A] == [0, 1, 63, 64, 65, 128, 0, 2] and [m.L for m in B] == [5, 0, 3]
    assert {0, 1, 64, 65, 128} <= {m.L for m in A} and RC.ML_A == 128 and RC.ML_B == 5
    kinds, branches, nan_lengths = set(), set(), 0
    for m in A + B:
        assert m.mu.shape == (3 + 2 * m.L,) and m.sigma.shape == (3 + 2 * m.L,) * 2
        outside = np.ones_like(m.sigma, bool)
        for i, (a, c, d) in enumerate(m.blocks):
            j = 3 + 2 * i
            outside[j:j + 2, j:j + 2] = False
            assert (m.sigma[j, j], m.sigma[j + 1, j], m.sigma[j + 1, j + 1]) == (a, c, d)
            assert m.sigma[j, j + 1] != m.sigma[j + 1, j]                              # the wrong triangle shows
            kinds.add(m.kinds[i])
            branches.add(RC.branch_of(a, c, d))
            p = 0.5 * (a - d)
            lam = [d + p + s * np.sqrt(p * p + c * c) for s in (1, -1)]
            nan_lengths += RC.branch_of(a, c, d) != "negligible" and min(lam) < -1e-3
        assert (m.sigma[outside] != 0).all()                                           # pose rows and cross terms: a wrong index shows
        if m.L:
            assert not np.array_equal(np.triu(m.sigma, 1), np.tril(m.sigma, -1).T)
    assert kinds == set(RC.KINDS)
    assert branches == {"negligible", "p_positive", "p_negative", "p_zero", "pz_zero"}
    assert nan_lengths >= 2
    # one ulp either side of the negligible-sub-diagonal threshold, and the kinds fall where they are meant to
    for kind, want in (("c_below", "negligible"), ("c_above", "p_positive"), ("zero", "negligible"), ("c_zero", "negligible"),
                       ("a_eq_d", "p_zero"), ("a_lt_d", "p_negative"), ("a_gt_d", "p_positive"), ("negative", "p_zero"), ("pz_zero", "pz_zero")):
        a, c, d = RC.block_of(kind, np.random.default_rng(2))
        assert RC.branch_of(a, c, d) == want, kind
        if kind.startswith("c_b") or kind.startswith("c_a"):
            thr = RC.EPS * (abs(a) + abs(d))
            assert abs(c) == (np.nextafter(thr, 0.0) if kind == "c_below" else np.nextafter(thr, np.inf)) and c != 0.0
    for kind in RC.SPD_KINDS:
        a, c, d = RC.block_of(kind, np.random.default_rng(3))
        assert a > 0 and a * d - c * c > 0, kind
    # members of both fleets hold positive definite blocks for the eigen-solver comparison
    assert sum(int(RC.spd_rows(m).sum()) for m in A) > 100 and sum(int(RC.spd_rows(m).sum()) for m in B) >= 4
    ss = RC.sessions()
    assert len(ss) == 2 and all(s.config.n_landmarks == 24 for s in ss)
    assert all(15 <= int((s.ev_type == 1).sum()) <= 25 for s in ss)


def test_oracle_rows_of_the_cases(oracle_lib):
    """The oracle's rows on the crafted states: the means are the state's, an SPD block's lengths are finite, a block with a
    negative eigenvalue has a NaN length, the all-zero block an ellipse of length 0."""
    for m in RC.fleet_a() + RC.fleet_b():
        rows = RC.oracle_rows(m)
        assert rows.shape == (m.L, 5)
        if not m.L:
            continue
        assert np.array_equal(rows[:, :2], m.mu[3:].reshape(-1, 2))
        for r, kind in zip(rows, m.kinds):
            if kind in RC.SPD_KINDS:
                assert np.isfinite(r).all() and (r[3:] > 0).all()
            elif kind == "negative":
                assert np.isnan(r[3:]).sum() == 1
            elif kind in ("zero", "pz_zero"):
                assert (r[3:] == 0).all()
                assert r[2] == (0.0 if kind == "zero" else np.pi / 2)


def test_witness_floor(oracle_lib):
    """The floor of the GPU test's eigen-solver comparison: the oracle's ellipses, drawn, against the blocks themselves.  Neither
    figure comes from the code under test."""
    worst = 0.0
    n = 0
    for m in RC.fleet_a() + RC.fleet_b():
        keep = RC.spd_rows(m)
        if keep.any():
            worst = max(worst, RC.ellipse_error(RC.oracle_rows(m)[keep], m.blocks[keep]))
            n += int(keep.sum())
    print(f"\noracle ellipses against {n} positive definite blocks: largest relative error {worst:.3e}; recorded {ELLIPSE_FLOOR:.3e}")
    assert np.isfinite(worst) and worst < 1e-13
    assert ELLIPSE_FLOOR / 2 <= worst <= ELLIPSE_FLOOR, "the recorded floor is stale"
