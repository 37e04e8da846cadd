"""The 3D detector sweep on the GPU (cases: tests/detect3d_sweep_cases.py, and with them every cloud of tests/fleet_detect3d_cases.py):
both kernel chains of csrc/det3d.hip forced (the long one: k3_filter_count / k3_filter_write / k3_scatter / k3_boxes, the sweeps,
k3_finish_a + k3_clusters; the short one: k3f_front, the sweeps, k3f_clusters), the default mode forwards and backwards, two clouds on
their way, and all sweep cases as members of one k_det3d_batch launch -- against oracle/detect3d_oracle.c with np.array_equal on the
centres' bits.  There is no tolerance anywhere.  Reference: src/reflector_detect/point_cloud/point_cloud_reflector_detect.cc:9-106."""
import numpy as np
import pytest

from tests import detect3d_sweep_cases as SC
from tests import fleet_detect3d_cases as FC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def table(oracle_lib):
    """-> the cases in table order: the sweep, then the fleet suite's; the oracle's answers are computed once and shared."""
    cases = list(SC.cases()) + list(FC.cases())
    for c in cases:
        SC.oracle_single(c)
    by = {c["name"]: SC.oracle_single(c) for c in cases}
    assert by["lattice_257"][0] == by["rank_K_257"][0] == FC.CAPACITY
    assert by["max_bright_plus_1"][0] == 0 and by["max_bright_plus_1"][2] == FC.MAX_BRIGHT + 1 and by["max_bright_plus_1"][1].shape[0] > 90
    assert sum(by[c["name"]][2] > FC.MAX_BRIGHT for c in cases) == 5           # (5121 twice, 8191, 8192, 8193)
    return cases


class _Handles:
    """One PointCloudReflectorDetect per distinct (gate, transform) of the table, all in one chain mode; a fresh one on request."""

    def __init__(self, mode):
        self.mode, self.shared, self.all = mode, {}, []

    def fresh(self, case):
        from reflector_ekf_slam_amd.detect import PointCloudOptions, PointCloudReflectorDetect
        g = PointCloudReflectorDetect(PointCloudOptions(case["intensity_min"]), max_points=65536, sensor_to_base_link=case["s2b"])
        g.debug_set_path(self.mode)
        self.all.append(g)
        return g

    def of(self, case):
        key = (case["intensity_min"], case["s2b"])
        if key not in self.shared:
            self.shared[key] = self.fresh(case)
        return self.shared[key]

    def close(self):
        for g in self.all:
            g.close()


def _same(obs, case, stamp):
    status, want, _ = SC.oracle_single(case)
    assert status == 0, case["name"]
    assert obs.time_ == stamp and obs.cloud_.shape == want.shape, (case["name"], obs.cloud_.shape, want.shape)
    assert np.array_equal(obs.cloud_.view(np.uint32), want.view(np.uint32)), case["name"]


def _handle(g, case, stamp):
    """One synchronous call: the oracle's centres bit for bit, or the refusal for more than 256 clusters."""
    from reflector_ekf_slam_amd.detect import RdetError
    if SC.oracle_single(case)[0]:
        with pytest.raises(RdetError) as e:
            g.HandlePointCloud(stamp, case["cloud"])
        assert e.value.code == FC.CAPACITY, case["name"]
        return
    _same(g.HandlePointCloud(stamp, case["cloud"]), case, stamp)


def _forced(cases, mode):
    """Every case through the chain `mode`: a fresh handle per `stretch` case (its first cloud is sorted on the initial grid, which is
    what the stretch claims are stated for), one handle per (gate, transform) for the rest.  -> [(case, counts before, counts after)]"""
    hs = _Handles(mode)
    log = []
    try:
        for k, c in enumerate(cases):
            g = hs.fresh(c) if c["name"].startswith("stretch_") else hs.of(c)
            before = g.debug_path_counts()
            _handle(g, c, 2.0 + k)
            log.append((c, before, g.debug_path_counts()))
        assert len(hs.all) >= 4 + 2
    finally:
        hs.close()
    return log


def test_long_chain_every_case(table):
    for c, before, after in _forced(table, 1):
        assert before == after == (0, 0), c["name"]


def test_short_chain_forced_every_case(table):
    n_again = 0
    for c, before, after in _forced(table, 2):
        m = SC.oracle_single(c)[2]
        assert after[0] == before[0] + (1 if c["cloud"].shape[0] else 0), c["name"]
        assert after[1] - before[1] == (1 if m > FC.MAX_BRIGHT else 0), (c["name"], m, before, after)   # sent again iff it did not fit
        n_again += after[1] - before[1]
    assert n_again == 5


@pytest.mark.parametrize("backwards", [False, True])
def test_default_mode_forwards_and_reversed(table, backwards):
    """One handle per (gate, transform) takes the whole list in table order, another set takes it reversed: every cloud inherits the
    sorting grid and the count hint of a foreign cloud (the `stretch` claims mean nothing here; the centres must match all the same)."""
    hs = _Handles(0)
    try:
        for k, c in enumerate(table[::-1] if backwards else table):
            _handle(hs.of(c), c, 1.0 + k)
        short = sum(g.debug_path_counts()[0] for g in hs.all)
        assert 0 < short < len(table)                                             # (both front ends were taken)
    finally:
        hs.close()


def test_two_in_flight(table):
    """SubmitPointCloud / CollectObservation, always two clouds on their way (the list of every (gate, transform) through its own handle;
    all but five clouds share one): results and stamps are those of the synchronous calls, a refusal is its own cloud's."""
    from reflector_ekf_slam_amd.detect import RdetError
    lists = {}
    for c in table:
        lists.setdefault((c["intensity_min"], c["s2b"]), []).append(c)
    assert max(len(v) for v in lists.values()) >= len(SC.cases()) + 30 and len(lists) >= 4
    hs = _Handles(0)
    try:
        for cases in lists.values():
            g = hs.of(cases[0])
            got = []

            def collect():
                try:
                    got.append(g.CollectObservation())
                except RdetError as e:
                    got.append(e.code)

            g.SubmitPointCloud(0.0, cases[0]["cloud"])
            for k in range(1, len(cases)):
                g.SubmitPointCloud(float(k), cases[k]["cloud"])
                collect()
            collect()
            assert len(got) == len(cases)
            for k, (c, obs) in enumerate(zip(cases, got)):
                if SC.oracle_single(c)[0]:
                    assert obs == FC.CAPACITY, c["name"]
                else:
                    assert not isinstance(obs, int), (c["name"], obs)
                    _same(obs, c, float(k))
    finally:
        hs.close()


@pytest.mark.parametrize("backwards", [False, True])
def test_batch_every_case_in_one_launch(oracle_lib, backwards):
    """All sweep cases as members of one rdet3d_batch call: the oracle's centres, M and K up to MAX_BRIGHT survivors, that member's
    RDET_ERR_CAPACITY with the true M beyond, the capacity refusal for 257 clusters."""
    from reflector_ekf_slam_amd import PointCloudReflectorDetectFleet
    from reflector_ekf_slam_amd.detect import PointCloudOptions
    cases = list(SC.cases())
    fl = PointCloudReflectorDetectFleet([PointCloudOptions(c["intensity_min"]) for c in cases], max_points=max(c["cloud"].shape[0] for c in cases),
                                        sensor_to_base_link=np.array([c["s2b"] for c in cases], dtype=np.float64))
    try:
        members = list(range(len(cases)))[::-1] if backwards else list(range(len(cases)))
        got = fl.detect([(m, 5.0 + 0.5 * i, cases[m]["cloud"]) for i, m in enumerate(members)])
        assert len(got) == len(members) == len(fl.last_n_bright)
        n_refused = 0
        for i, m in enumerate(members):
            c = cases[m]
            status, want, m1, _ = SC.oracle(c)
            st, obs = got[i]
            assert fl.last_n_bright[i] == m1 == c["claims"]["M"], (c["name"], fl.last_n_bright[i], m1)
            assert st == status and obs.time_ == 5.0 + 0.5 * i, (c["name"], st, status)
            assert (status == FC.CAPACITY) == (m1 > FC.MAX_BRIGHT or c["name"] == "rank_K_257"), c["name"]
            assert obs.cloud_.shape == want.shape and np.array_equal(obs.cloud_.view(np.uint32), want.view(np.uint32)), c["name"]
            if "K" in c["claims"] and status == 0:
                assert obs.cloud_.shape[0] == c["claims"]["K"], c["name"]
            n_refused += status != 0
        assert n_refused == 5                                                     # (5121, 8191, 8192, 8193 and the 257 clusters)
    finally:
        fl.close()
