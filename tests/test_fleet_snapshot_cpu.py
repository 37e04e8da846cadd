"""Snapshot and restore of the fleet filter, what can be checked without a GPU: the C ABI and the refusals that come before any HIP
call, the lazy loader, the numpy witness of the blob against itself and against FleetSnapshot, the coverage of the cases of
tests/fleet_snapshot_cases.py, and that the comparison the GPU file uses catches each planted defect of the witness."""
from __future__ import annotations

import ctypes as C
import re
import struct
import subprocess

import numpy as np
import pytest

from reflector_ekf_slam_amd import fleet
from reflector_ekf_slam_amd.fleet import FleetSnapshot, _snapshot_lib  # noqa: F401  (a tree without the calls fails here, every test with it)
from tests import fleet_cases as FC
from tests import fleet_snapshot_cases as SC
from tests.fleet_harness import HEADER
from tests.witness import fleet_snapshot_witness as W

CALLS = ("rfleet_snapshot", "rfleet_restore", "rfleet_snapshot_peek", "rfleet_sizeof_snapshot_member", "rfleet_sizeof_snapshot_hdr")


def _codes():
    text = open(HEADER.replace("rfleet.h", "rekf.h")).read()
    return {k: int(re.search(rf"REKF_ERR_{k}\s*=\s*(-?\d+)", text).group(1)) for k in ("INVALID", "BUFFER", "HIP")}


def same_blob(got, want) -> bool:
    """The comparison of the GPU file: byte for byte."""
    as_bytes = lambda b: b if isinstance(b, bytes) else np.asarray(b, np.uint8).tobytes()       # noqa: E731
    return as_bytes(got) == as_bytes(want)


def test_header_declares_the_calls_and_keeps_the_abi_version():
    text = open(HEADER).read()
    flat = " ".join(text.split())
    assert "int rfleet_snapshot(rfleet_t *f, const int *members, int count, void *out, long cap_bytes, long *bytes);" in flat
    assert "int rfleet_restore(rfleet_t *f, const void *blob, long bytes, const int *members, int count);" in flat
    assert "int rfleet_snapshot_peek(const void *blob, long bytes, int *count, int *max_n);" in flat
    assert "int rfleet_sizeof_snapshot_member(void);" in flat and "int rfleet_sizeof_snapshot_hdr(void);" in flat
    assert re.search(r"#define\s+RFLEET_ABI_VERSION\s+2\b", text)
    assert re.search(r'#define\s+RFLEET_SNAPSHOT_MAGIC\s+"RFLTSNAP"', text) and re.search(r"#define\s+RFLEET_SNAPSHOT_VERSION\s+1\b", text)
    assert fleet.rfleet().rfleet_abi_version() == 2 == fleet.RFLEET_ABI_VERSION
    # the structures as the header spells them, against the witness's and the binding's
    hdr = re.search(r"typedef struct rfleet_snapshot_hdr \{(.*?)\}", text, re.S).group(1)
    ent = re.search(r"typedef struct rfleet_snapshot_member \{(.*?)\}", text, re.S).group(1)
    fields = lambda body: re.findall(r"^\s*(char|int|long|double)\s+(\w+(?:\[\d+\])?);", body, re.M)       # noqa: E731
    assert fields(hdr) == [("char", "magic[8]"), ("int", "version"), ("int", "count"), ("long", "bytes")]
    assert fields(ent) == [("double", "t"), ("double", "vt[3]"), ("int", "member"), ("int", "n"), ("int", "flags"), ("int", "pad_"), ("long", "off")]
    L = fleet._snapshot_lib()
    assert L.rfleet_sizeof_snapshot_hdr() == W.HDR.size == C.sizeof(fleet.RfleetSnapshotHdr) == 24
    assert L.rfleet_sizeof_snapshot_member() == W.ENTRY.size == C.sizeof(fleet.RfleetSnapshotMember) == 56
    assert fleet.SNAPSHOT_MAGIC == W.MAGIC and fleet.SNAPSHOT_VERSION == W.VERSION


def test_library_exports_the_calls():
    from reflector_ekf_slam_amd import _lib as base
    path = base.lib_path("librfleet.so")
    names = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    for call in CALLS:
        assert hasattr(C.CDLL(path), call) and re.search(rf"\bT {call}\b", names), call
    for kernel in ("k_fleet_pack", "k_fleet_unpack"):                      # the launch stubs of the two kernels
        assert kernel in names, kernel


def _peek(L, blob):
    count, max_n = C.c_int(-7), C.c_int(-7)
    buf = np.frombuffer(blob, np.uint8).copy() if len(blob) else np.zeros(1, np.uint8)
    rc = L.rfleet_snapshot_peek(buf.ctypes.data, len(blob), C.byref(count), C.byref(max_n))
    return rc, count.value, max_n.value


def _entry_bytes(blob, g, **change):
    """blob with fields of entry g replaced."""
    names = ("t", "v0", "v1", "v2", "member", "n", "flags", "pad", "off")
    at = W.HDR.size + W.ENTRY.size * g
    vals = dict(zip(names, W.ENTRY.unpack_from(blob, at)))
    vals.update(change)
    return blob[:at] + W.ENTRY.pack(*(vals[k] for k in names)) + blob[at + W.ENTRY.size:]


def test_peek_validates_a_blob_on_the_host():
    """rfleet_snapshot_peek needs no handle and no device: a good blob's count and widest n, and every malformed blob refused."""
    L = fleet._snapshot_lib()
    INVALID = _codes()["INVALID"]
    entries = SC.coded_entries((3, 5, 17))
    good = W.pack(entries)
    assert _peek(L, good) == (0, 3, 17)
    assert _peek(L, W.pack([])) == (0, 0, 0)
    assert L.rfleet_snapshot_peek(None, len(good), None, None) == INVALID
    size = len(good)
    off1 = W.ENTRY.unpack_from(good, W.HDR.size + W.ENTRY.size)[8]
    bad = {
        "wrong magic": b"RFLTSNAQ" + good[8:],
        "wrong version": good[:8] + struct.pack("<i", 2) + good[12:],
        "negative count": good[:12] + struct.pack("<i", -1) + good[16:],
        "truncated": good[:-8],
        "header says more bytes": good[:16] + struct.pack("<q", size + 8) + good[24:],
        "shorter than a header": good[:16],
        "count beyond the blob": good[:12] + struct.pack("<i", 1 << 20) + good[16:],
        "overlapping offsets": _entry_bytes(good, 1, off=off1 - 8),
        "offset inside the entries": _entry_bytes(good, 0, off=W.HDR.size),
        "offset out of range": _entry_bytes(good, 2, off=size),
        "payload runs past the end": _entry_bytes(good, 2, n=19),
        "negative offset": _entry_bytes(good, 0, off=-8),
        "offset not a multiple of 8": _entry_bytes(good, 2, off=W.ENTRY.unpack_from(good, W.HDR.size + 2 * W.ENTRY.size)[8] + 4),
        "even n": _entry_bytes(good, 1, n=4),
        "n < 3": _entry_bytes(good, 0, n=1),
        "n beyond any fleet": _entry_bytes(good, 0, n=261),
        "negative member": _entry_bytes(good, 0, member=-1),
    }
    for what, blob in bad.items():
        rc, count, max_n = _peek(L, blob)
        assert rc == INVALID and (count, max_n) == (-7, -7), what
    # a gap between payloads is a valid blob (the entries are in order and inside); rfleet_snapshot itself never leaves one
    gap = good + bytes(8)
    gap = gap[:16] + struct.pack("<q", len(gap)) + gap[24:]
    assert _peek(L, gap)[0] == 0


def test_refusals_come_before_any_hip_call():
    """Every refusal that rfleet.h places before any HIP call and before the handle is read, on a machine without a device.  The
    handle is a dummy that the library must not look into before it has refused."""
    L = fleet._snapshot_lib()
    INVALID = _codes()["INVALID"]
    dummy = C.c_void_p(1)
    mem = np.arange(4, dtype=np.int32)
    out = np.full(4096, 0xAB, np.uint8)
    size = C.c_long(-5)
    snap = L.rfleet_snapshot
    assert snap(None, mem.ctypes.data, 4, out.ctypes.data, out.size, C.byref(size)) == INVALID          # a null handle
    assert snap(None, None, 0, None, 0, C.byref(size)) == INVALID
    assert snap(dummy, mem.ctypes.data, -1, out.ctypes.data, out.size, C.byref(size)) == INVALID        # count < 0
    assert snap(dummy, mem.ctypes.data, 4, out.ctypes.data, out.size, None) == INVALID                  # null bytes
    assert snap(dummy, mem.ctypes.data, 4, out.ctypes.data, -1, C.byref(size)) == INVALID               # cap_bytes < 0
    assert size.value == -5 and (out == 0xAB).all()
    good = np.frombuffer(W.pack(SC.coded_entries((3, 5))), np.uint8).copy()
    rest = L.rfleet_restore
    assert rest(None, good.ctypes.data, good.size, None, 2) == INVALID                                  # a null handle
    assert rest(dummy, None, good.size, None, 2) == INVALID                                             # a null blob
    assert rest(dummy, good.ctypes.data, good.size, None, -1) == INVALID                                # count < 0
    assert rest(dummy, good.ctypes.data, -1, None, 2) == INVALID                                        # bytes < 0
    for what in (b"RFLTSNAQ" + good.tobytes()[8:], good.tobytes()[:-8], _entry_bytes(good.tobytes(), 1, n=4)):      # a malformed blob
        b = np.frombuffer(what, np.uint8).copy()
        assert rest(dummy, b.ctypes.data, b.size, None, 2) == INVALID


def test_the_binding_looks_the_calls_up_lazily(monkeypatch):
    """rfleet() does not ask for the new symbols: a library of ABI version 2 without them keeps serving everything else, and the
    snapshot methods raise LibraryMissing, as the other lazily declared calls do."""
    from reflector_ekf_slam_amd import _lib as base
    real = fleet.rfleet()

    class Old:
        """A library handle of ABI version 2 from before the snapshot calls."""
        def __getattr__(self, name):
            if name in CALLS:
                raise AttributeError(name)
            return getattr(real, name)

    old = Old()
    monkeypatch.setattr(fleet._snapshot_lib, "ready", None)
    monkeypatch.setattr(fleet._reflectors_lib, "ready", None)
    monkeypatch.setattr(fleet.rfleet, "ready", old)
    with pytest.raises(base.LibraryMissing) as e:
        fleet._snapshot_lib()
    assert "rfleet_snapshot" in str(e.value) and "rfleet_restore" in str(e.value) and "librfleet.so" in str(e.value)
    assert fleet._snapshot_lib.ready is None
    assert fleet._reflectors_lib() is old and fleet.rfleet().rfleet_abi_version() == 2        # every other call keeps working
    fl = object.__new__(fleet.ReflectorEKFSLAMFleet)
    fl.B = 2
    for call in (lambda: fl.snapshot(), lambda: fl.restore(np.zeros(24, np.uint8)), lambda: fleet.FleetSnapshot(np.zeros(24, np.uint8))):
        with pytest.raises(base.LibraryMissing):
            call()
    monkeypatch.setattr(fleet._reflectors_lib, "ready", None)
    monkeypatch.setattr(fleet.rfleet, "ready", real)
    got = fleet._snapshot_lib()
    assert got is real and fleet._snapshot_lib.ready is real and got.rfleet_snapshot.argtypes is not None
    for name in ("snapshot", "snapshot_code", "restore", "restore_code"):
        assert callable(getattr(fleet.ReflectorEKFSLAMFleet, name)), name
    assert not hasattr(fleet.FleetMember, "snapshot") and not hasattr(fleet.FleetMember, "restore")


# ---- the witness and FleetSnapshot ---------------------------------------------------------------------------------------------------
def _all_coded_lists():
    for name, ml, dims in SC.CODED_FLEETS:
        entries = SC.coded_entries(dims)
        for which, members in SC.lists_for(len(dims)).items():
            yield f"{name}/{which}", ml, SC.listed(entries, members)


def test_witness_round_trips_every_case():
    for what, ml, entries in _all_coded_lists():
        blob = W.pack(entries)
        back = W.parse(blob)
        assert len(back) == len(entries), what
        for a, b in zip(entries, back):
            assert (a.member, a.n, a.flags, a.t) == (b.member, b.n, b.flags, b.t), what
            assert np.array_equal(a.vt, b.vt) and np.array_equal(a.mu, b.mu) and np.array_equal(SC.mirrored(a.sigma), b.sigma), what
        assert W.pack(back) == blob, what
        assert len(blob) == 24 + sum(56 + 8 * (e.n + e.n * (e.n + 1) // 2) for e in entries)


def test_fleet_snapshot_parses_witness_blobs(tmp_path):
    for k, (what, ml, entries) in enumerate(_all_coded_lists()):
        blob = W.pack(entries)
        snap = fleet.FleetSnapshot(blob)
        assert len(snap) == len(entries) and snap.blob.dtype == np.uint8 and snap.blob.tobytes() == blob
        assert snap.members.tolist() == [e.member for e in entries] and snap.n.tolist() == [e.n for e in entries]
        assert snap.flags.tolist() == [e.flags for e in entries] and snap.t.tolist() == [e.t for e in entries]
        assert snap.max_n == max(e.n for e in entries)
        for g, e in enumerate(entries):
            assert np.array_equal(snap.vt[g], e.vt) and np.array_equal(snap.mu(g), e.mu), what
            assert np.array_equal(snap.triangle(g), W.triangle_of(e.sigma)), what
            assert np.array_equal(snap.sigma(g), SC.mirrored(e.sigma)), what
            st = snap.state(g)
            assert st.time == e.t and np.array_equal(st.mu, e.mu) and np.array_equal(st.sigma, SC.mirrored(e.sigma))
            assert np.shares_memory(snap.mu(g), snap.blob) and np.shares_memory(snap.triangle(g), snap.blob)       # views, not copies
        if k % 4 == 0:
            path = tmp_path / f"snap{k}.bin"
            snap.save(path)
            assert open(path, "rb").read() == blob
            assert fleet.FleetSnapshot.load(path).blob.tobytes() == blob
    bad = tmp_path / "bad.bin"
    bad.write_bytes(W.pack(SC.coded_entries((3, 5)))[:-8])
    with pytest.raises(fleet.RekfError):
        fleet.FleetSnapshot.load(bad)
    assert len(fleet.FleetSnapshot(W.pack([]))) == 0


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def test_cases_cover_what_they_claim(oracle_lib):
    assert SC.NS == (3, 5, 15, 17, 31, 33, 257, 259)
    by_name = {name: (ml, dims) for name, ml, dims in SC.CODED_FLEETS}
    assert by_name["ml128_B8"] == (128, SC.NS) and {ml for ml, _ in by_name.values()} == {128, 7, 8}
    assert {len(d) for _, d in by_name.values()} == {1, 8}
    for name, (ml, dims) in by_name.items():
        n_max = 3 + 2 * ml
        assert all(3 <= n <= n_max and n % 2 for n in dims), name
        assert n_max in dims or name == "ml8_B1", name                     # a member at capacity: the last panel as full as it gets
    assert (3 + 2 * 128 + 15) // 16 * 16 == 272 and (3 + 2 * 7 + 15) // 16 * 16 == 32 and 3 + 2 * 8 == 19
    assert {n % 16 for n in SC.NS} >= {15, 1, 3} and {(n + 15) // 16 for n in (15, 17)} == {1, 2} and {(n + 15) // 16 for n in (257, 259)} == {17}
    assert SC.LISTS["all"] is None and len(SC.LISTS["one"]) == 1
    perm = SC.LISTS["permuted"]
    assert perm == [5, 2, 7] and perm != sorted(perm) and len(set(perm)) == 3
    # index-coded: every value of a fleet is distinct, exact, and the wrong triangle shows
    for name, (ml, dims) in by_name.items():
        entries = SC.coded_entries(dims)
        vals = np.concatenate([np.concatenate([e.mu, W.triangle_of(e.sigma)]) for e in entries])
        assert np.unique(vals).shape[0] == vals.shape[0], name
        for e in entries:
            i, j = np.tril_indices(e.n)
            assert np.array_equal(e.sigma[i, j], 1e6 * (e.member + 1) + 1e3 * i + j + 0.5)
            if e.n > 1:
                iu, ju = np.triu_indices(e.n, 1)
                assert (e.sigma[iu, ju] == -e.sigma[ju, iu]).all() and (e.sigma[iu, ju] < 0).all()
        other = SC.coded_entries(dims, salt=7)
        assert not any(np.array_equal(a.mu, b.mu) or a.t == b.t for a, b in zip(entries, other))
    # real: the oracle on every member's ticks -- reflectors are appended before AND after the snapshot, scans also match, a fleet
    # of max_landmarks 7 overflows at once (REKF_FLAGBIT_CAPACITY), one of 128 never does
    from tests.helpers import make_oracle, norm_match
    B = 8
    tk = SC.ticks(B)
    assert len(tk) == 2 * SC.T and SC.T >= 3
    fixes = [ev for tick in SC.ticks(B, pose_fix=True) for ev in tick if len(ev) == 6]
    assert len(fixes) == B * SC.SESSION_SCANS // 2
    t_end, vt_end = SC.last_stamp_and_velocity(tk[: SC.T], B, SC.options(B))
    xy, cov = SC.shared_map(B)
    assert SC.sessions(B)[0].config.odom_model != SC.sessions(B)[1].config.odom_model      # DIFF and OMNI
    for m in range(B):
        s = SC.sessions(B)[m]
        cfg = s.config
        for with_map in ((False, True) if m == 0 else (False,)):
            o = make_oracle(cfg.odom_model, s.init_time, s.init_pose, cfg.sigma_v ** 2, cfg.sigma_w ** 2, cfg.sigma_obs ** 2)
            if with_map:
                o.set_map(xy, cov)
            n_at, matched, appended, map_matched = [], [0, 0], [0, 0], [0, 0]
            for k, tick in enumerate(tk):
                for ev in tick:
                    if ev[0] != m:
                        continue
                    FC.feed(o, ev[1:5])
                    if ev[1] == FC.EV_SCAN:
                        sp, mp, nw = norm_match(o.last_match())
                        half = k // SC.T
                        matched[half] += sp.shape[0]
                        appended[half] += nw.shape[0]
                        map_matched[half] += mp.shape[0]
                n_at.append(o.state()[0].shape[0])
            o.close()
            assert min(matched) > 0 and min(appended) > 0, (m, matched, appended)
            assert n_at[-1] <= 3 + 2 * 128 and n_at[-1] > n_at[SC.T - 1], (m, n_at)
            assert with_map or n_at[SC.T - 1] > 3 + 2 * 7, (m, n_at)          # (a map-matched observation appends nothing)
            if with_map and m == 0:
                assert min(map_matched) > 0, map_matched
        assert t_end[m] == max(ev[2] for tick in tk[: SC.T] for ev in tick if ev[0] == m) and np.abs(vt_end[m]).max() > 0
    assert SC.wide_cloud(0).shape == (40, 2) and 40 > fleet.MAX_OBS
    # the crafted growth of the restore-over-a-used-member test
    grow = SC.grow_events(0, 5.0, (1, 4, 9, 16))
    assert [ev[1][4].shape[0] for ev in grow] == [1, 4, 9, 16] and 3 + 2 * 16 >= 33
    pts = SC.lattice_scan(20, 0).astype(np.float64)
    d = np.linalg.norm(pts[:, None] - pts[None], axis=-1) + 10 * np.eye(20)
    assert d.min() > 1.2                                                   # twice the 0.6 gate: every point its own reflector


# ---- the measurement describes the tree ----------------------------------------------------------------------------------------------
SNAPSHOT_BENCH_SOURCES = ["include/rfleet.h", "reflector_ekf_slam_amd/csrc/fleet_dev.h", "reflector_ekf_slam_amd/csrc/fleet_host.h", "reflector_ekf_slam_amd/csrc/fleet_snapshot.h",
                          "reflector_ekf_slam_amd/csrc/fleet_snapshot.hip", "reflector_ekf_slam_amd/csrc/rfleet_api.hip",
                          "reflector_ekf_slam_amd/fleet.py", "scripts/fleet_snapshot_bench.py"]


@pytest.mark.parametrize("record", ["fleet_snapshot_bench.json", "fleet_snapshot_bench_reversed.json"])
def test_fleet_snapshot_bench_describes_the_tree(record):
    """The committed records were measured on the snapshot sources of this tree (SHA-256 by content), their ratios are their legs', and
    README and DESIGN quote the default-order record."""
    import hashlib
    import json
    import os
    from tests.fleet_harness import ROOT
    rec = json.load(open(os.path.join(ROOT, "profiles", record)))
    sums = rec["_sources_sha256"]
    assert sorted(sums) == sorted(SNAPSHOT_BENCH_SOURCES)
    for rel in SNAPSHOT_BENCH_SOURCES:
        have = hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest()
        assert have == sums[rel], f"{rel} changed since profiles/{record} was measured: measure again (scripts/fleet_snapshot_bench.py)"
    assert sorted(rec["dims"]) == ["259", "67"] and rec["reps"] == 5
    for n, d in rec["dims"].items():
        assert sorted(d["snapshot"]) == ["256", "4", "64"]
        for B in d["snapshot"]:
            for leg in ("snapshot", "get_state", "restore", "set_state"):
                s = d[leg][B]
                assert 0 < s["min"] <= s["median"] <= s["max"]
            assert d["get_state_min_over_snapshot_max"][B] == d["get_state"][B]["min"] / d["snapshot"][B]["max"]
            assert d["set_state_min_over_restore_max"][B] == d["set_state"][B]["min"] / d["restore"][B]["max"]
            assert d["snapshot_is_faster"][B] == (d["snapshot"][B]["max"] < d["get_state"][B]["min"])
            assert d["restore_is_faster"][B] == (d["restore"][B]["max"] < d["set_state"][B]["min"])
            n_i = int(n)
            assert d["blob_bytes"][B] == 24 + int(B) * (56 + 8 * (n_i + n_i * (n_i + 1) // 2))
    if record == "fleet_snapshot_bench.json":
        big = rec["dims"]["259"]
        for text in (open(os.path.join(ROOT, "README.md")).read(), open(os.path.join(ROOT, "DESIGN.md")).read()):
            flat = " ".join(text.split())
            for B in ("64", "256"):
                assert f"{big['get_state_min_over_snapshot_max'][B]:.2f}" in flat and f"{big['set_state_min_over_restore_max'][B]:.1f}" in flat
            assert "fleet_snapshot_bench.json" in flat and "10.14" in flat


# ---- planted defects -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defect", W.DEFECTS)
def test_planted_defects_are_caught(defect):
    """Each defect of the witness's packer changes the blob of the permuted list of the large index-coded fleet, so the byte-for-byte
    comparison of the GPU file fails on it; without a defect the comparison passes."""
    assert set(W.DEFECTS) == {"row_major", "strict_triangle", "off_by_one_entry", "index_order"}
    entries = SC.listed(SC.coded_entries(SC.NS), SC.LISTS["permuted"])
    want = W.pack(entries)
    assert same_blob(np.frombuffer(want, np.uint8), want) and same_blob(W.pack(W.parse(want)), want)
    assert not same_blob(W.pack(entries, defect=defect), want)
    small = SC.listed(SC.coded_entries(SC.CODED_FLEETS[1][2]), SC.LISTS["permuted"])
    assert not same_blob(W.pack(small, defect=defect), W.pack(small))
