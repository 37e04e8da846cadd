"""What the pose track's GPU tests share (tests/test_fleet_track_gpu.py): the UNTRACKED TWIN and the comparison with it.

The expected value of a record is never computed by the tracked path: it is what a second, untracked fleet holds after the same
event, given ONE event per ``submit`` with ``poses()``, ``n()`` and ``last_match()`` behind each
(tests/test_fleet_edges_gpu.py::test_several_scans_per_launch: an untracked fleet gives the same bits in any chunking).  Records are
compared bit for bit in ``mu``, ``sigma`` and ``n``.  numpy only; nothing here needs a GPU to import."""
from __future__ import annotations

from types import SimpleNamespace as NS

import numpy as np

from tests import fleet_cases as FC


def twin_records(tw, feed, use_imu=()):
    """``feed``: [(member, event)] in the order given to the twin fleet ``tw`` (untracked), one event per submit.  -> per member the
    list of expected records: the message's stamp, kind, K, whether the host drops it (decided here from the twin's state time and
    the member's use_imu switch), and the twin's pose, pose covariance, n, flags and match counts behind it."""
    out = {}
    for member, ev in feed:
        t_state = float(tw.poses()[0][member])
        tw.submit([FC.fev(member, ev)])
        t, mu, sg = tw.poses()
        kind = int(ev[0])
        dropped = int(kind == FC.EV_ODOM and (member in use_imu or ev[1] < t_state))
        K = int(np.asarray(ev[3]).reshape(-1, 2).shape[0]) if kind == FC.EV_SCAN and ev[3] is not None else 0
        ns = nm = nn = 0
        if kind == FC.EV_SCAN:
            rec = tw.last_match(member)
            ns, nm, nn = rec.state_obs_match_ids.shape[0], rec.map_obs_match_ids.shape[0], rec.new_ids.shape[0]
        out.setdefault(member, []).append(NS(t=float(ev[1]), kind=kind, K=K, dropped=dropped, mu=mu[member].copy(), sigma=sg[member].copy(),
                                             n=int(tw.n()[member]), flags=int(tw.flags()[member]), n_state=ns, n_map=nm, n_new=nn,
                                             state_time=float(t[member])))
    return out


def assert_records(track, want, who=""):
    """A MemberTrack against the twin's records of the same messages: every field, the floating-point ones bit for bit."""
    assert len(track) == len(want), (who, len(track), len(want))
    for r, w in enumerate(want):
        where = (who, r, w.kind, w.t)
        assert track.t[r] == w.t and track.kind[r] == w.kind and track.K[r] == w.K and track.dropped[r] == w.dropped, where
        assert track.mu[r].tobytes() == w.mu.tobytes(), (where, track.mu[r], w.mu)
        assert track.sigma[r].tobytes() == w.sigma.tobytes(), (where, track.sigma[r], w.sigma)
        assert track.n[r] == w.n and track.flags[r] == w.flags, (where, track.n[r], w.n, track.flags[r], w.flags)
        assert (track.n_state[r], track.n_map[r], track.n_new[r]) == (w.n_state, w.n_map, w.n_new), where


def last_record_is_the_slot(fl, track, member):
    """The last record of a launch against ``poses()`` / ``n()`` / ``flags()`` behind it."""
    _, mu, sg = fl.poses()
    return (track.mu[-1].tobytes() == mu[member].tobytes() and track.sigma[-1].tobytes() == sg[member].tobytes()
            and track.n[-1] == fl.n()[member] and track.flags[-1] == fl.flags()[member])


def concat(parts):
    """Several takes of one member, in order, as one record of arrays (``lost`` summed)."""
    from reflector_ekf_slam_amd.fleet import MemberTrack
    names = ("t", "kind", "K", "dropped", "mu", "sigma", "n", "flags", "n_state", "n_map", "n_new")
    return MemberTrack(*(np.concatenate([getattr(p, k) for p in parts]) for k in names), lost=sum(p.lost for p in parts))
