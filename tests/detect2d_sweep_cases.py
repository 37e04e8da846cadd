"""Cases of the 2D detector sweep: lidar geometries, beam-boundary placements, threshold ties, non-finite data and odometry that
the other detector fixtures (full circles from -pi, scan_time 0.1, odometry from yaw 0 with vy = 0) never produce.
tests/test_detect2d_sweep_cpu.py holds the C oracle to the witness on every case and every case to its claims;
tests/test_detect2d_sweep_gpu.py holds k_det2d, k_det2d_batch and k_det2d_batch_range_data to the witness.

A case is ``dict(name, scan, odom, opts, s2b, claims)``:
  scan    a namespace with the LaserScan fields;
  odom    [(t, px, py, qz, qw, vx, vy, wz)], fed before the scan;
  opts    ReflectorDetectOptions keywords that differ from the defaults;
  s2b     sensor_to_base_link (x, y, yaw);
  claims  [(kind, ...)]: the facts that make the case worth having, checked by ``check_claims`` from the WITNESS's outputs
          (centres, member beam lists, returns), so that a later change to a helper cannot quietly make the case an easy one.

Plates whose bridge / gate decision is under test pass the length gate themselves (and their wrong outcome does not, or gives
another number of clusters), so the decision shows in the centres and not only in the run count.

A note on "circle": the reference's test is (angle_max - angle_min - 2 pi) < 1e-6 without an absolute value, so every scan that
spans LESS than a full turn -- a 270 degree scanner included -- is a circle scan; only a span beyond 2 pi + 1e-6 is not."""
from __future__ import annotations

import math
from types import SimpleNamespace as NS

import numpy as np

f32 = np.float32
BAD_SCAN = -3                       # RDET_ERR_BAD_SCAN
DEG = math.pi / 180.0
BRIGHT, DIM = 200.0, 50.0
STAMP = 5.0
S2B = (0.13686, 0.0, 0.0)           # launch/slam.launch:27
S2B_TURNED = (0.2, -0.1, 0.7)
DEFAULTS = dict(intensity_min=160.0, reflector_min_length=0.18, reflector_length_error=0.06, range_min=0.3, range_max=10.0)
QUARTER_DEG = 0.25 * DEG            # the increment of the 270 degree scanner; 2 pi / 1440 is the same angle


# ---------------------------------------------------------------------------------------------------------------- builders
def make_scan(N, angle_min, angle_increment, angle_max=None, scan_time=0.1, stamp=STAMP, range_min=0.05, range_max=30.0,
              base_range=20.0, base_int=DIM):
    """Any geometry: N beams from angle_min in steps of angle_increment; angle_max defaults to the last beam's angle.  Every
    beam far (outside the detector's gate, inside the message's) and dim."""
    amin, inc = f32(angle_min), f32(angle_increment)
    amax = f32(amin + inc * f32(N - 1)) if angle_max is None else f32(angle_max)
    return NS(stamp=float(stamp), angle_min=float(amin), angle_max=float(amax), angle_increment=float(inc), scan_time=float(scan_time),
              range_min=float(range_min), range_max=float(range_max), ranges=np.full(N, base_range, f32), intensities=np.full(N, base_int, f32))


def a1(N=1081, **kw):
    """The 270 degree scanner: from -135 degrees in steps of 0.25 degrees (1081 beams)."""
    return make_scan(N, -135.0 * DEG, QUARTER_DEG, **kw)


def a2(**kw):
    """A scanner that counts from 0 to 2 pi: 1440 beams."""
    return make_scan(1440, 0.0, 2.0 * math.pi / 1440, **kw)


def range_for(nb, inc=QUARTER_DEG, width=0.18):
    """The range at which nb adjacent beams span `width` metres end to end."""
    return width / (2.0 * math.sin((nb - 1) * abs(inc) / 2.0))


R15, R17, R21 = range_for(15), range_for(17), range_for(21)


def put(sc, first, n, rng, inten=BRIGHT):
    """A plate: n bright beams from `first` at range rng.  -> its beam ids."""
    sc.ranges[first:first + n] = rng
    sc.intensities[first:first + n] = inten
    return list(range(first, first + n))


def dim(sc, *beams, inten=DIM):
    for b in beams:
        sc.intensities[b] = inten


def odom_track(times, x0=300.0, y0=-200.0, th0=2.0, vx=1.0, vy=0.3, wz=2.0):
    """Samples of one motion: far from the origin, sideways velocity, a fast turn.  The quaternion is (sin(th / 2), cos(th / 2))
    of the unwrapped yaw, so qw < 0 occurs and 2 atan2(qz, qw) leaves [-pi, pi]."""
    out = []
    for t in times:
        dt = t - times[0]
        th = th0 + wz * dt
        x = x0 + (vx * math.cos(th0) - vy * math.sin(th0)) * dt
        y = y0 + (vx * math.sin(th0) + vy * math.cos(th0)) * dt
        out.append((float(t), x, y, math.sin(th / 2), math.cos(th / 2), vx, vy, wz))
    return out


def ticks(stamp, k0, k1, hz=50.0):
    """Sample times stamp + k / hz for k0 <= k <= k1: exact multiples, no accumulated step."""
    return [stamp + k / hz for k in range(k0, k1 + 1)]


def drive(stamp=STAMP):
    """The family A odometry: 50 Hz from 0.3 s before the stamp to 0.04 s after it, a gentle left turn near the origin."""
    return odom_track(ticks(stamp, -15, 2), x0=1.0, y0=2.0, th0=0.4, vx=1.0, vy=0.0, wz=0.3)


def case(name, scan, claims, odom=(), opts=None, s2b=S2B):
    return dict(name=name, scan=scan, odom=list(odom), opts=dict(opts or {}), s2b=tuple(s2b), claims=list(claims))


def with_odom(c, odom=None, more=()):
    """The same scan, moving: claims the de-skewed returns differ from the still twin's."""
    return case(c["name"] + "_odom", c["scan"], c["claims"] + [("returns_differ", c["name"])] + list(more),
                odom=drive(c["scan"].stamp) if odom is None else odom, opts=c["opts"], s2b=c["s2b"])


# ---------------------------------------------------------------------------------------------------------------- family A
def family_a():
    out = []
    # A1: the 270 degree scanner; plates at beam 0, across the 256-beam edge, mid scan, across the 1024-thread edge, ending at N - 1
    sc = a1()
    ids = [put(sc, 0, 17, R17), put(sc, 254, 17, R17), put(sc, 500, 17, R17), put(sc, 1022, 15, R15), put(sc, 1081 - 17, 17, R17)]
    c = case("A1", sc, [("circle",), ("min_centres", 4), ("n_centres", 5)] + [("cluster", i) for i in ids])
    out += [c, with_odom(c)]
    # A2: 0 -> 2 pi, a bridged gap in each quadrant (the gap beam's angle goes through every branch of the sin / cos range reduction)
    sc = a2()
    ids = [put(sc, 100, 17, R17), put(sc, 500, 17, R17), put(sc, 860, 18, R17), put(sc, 1220, 18, R17)]
    dim(sc, 108, 508, 868, 869, 1228, 1229)
    c = case("A2", sc, [("circle",), ("n_centres", 4), ("gap_angle_gt", math.pi / 2), ("gap_angle_gt", math.pi), ("gap_angle_gt", 1.5 * math.pi)]
             + [("cluster", i) for i in ids])
    out += [c, with_odom(c)]
    # A3: more than a full turn: NOT a circle.  A wrong-width run at beam 0, a good plate, a wrong-width run that ends at N - 1 within
    # 0.1 m of beam 0's point: neither the beam-0 clause nor the seam union may fire.  Relabelled as a circle, both do.
    n3 = 1460
    sc = make_scan(n3, -3.2, 2.0 * math.pi / 1440)
    first, mid, last = put(sc, 0, 3, 1.0), put(sc, 700, 17, R17), put(sc, n3 - 3, 3, 1.0)
    c = case("A3", sc, [("not_circle",), ("n_centres", 1), ("cluster", mid), ("no_cluster_with", 0), ("no_cluster_with", n3 - 1)])
    out += [c, with_odom(c)]
    sc = make_scan(n3, -3.2, 2.0 * math.pi / 1440, angle_max=-3.2 + 6.0)
    put(sc, 0, 3, 1.0), put(sc, 700, 17, R17), put(sc, n3 - 3, 3, 1.0)
    out.append(case("A3_as_circle", sc, [("circle",), ("n_centres", 2), ("cluster", first + last), ("cluster", mid), ("centres_differ", "A3")]))
    # ... and the union asks for the last run to END at N - 1: a run that stops three beams short stays out, and fails the length gate
    sc = a2()
    first, mid, short = put(sc, 0, 3, 1.0), put(sc, 700, 17, R17), put(sc, 1440 - 6, 3, 1.0)
    out.append(case("A3_seam_run_short_of_the_end", sc, [("circle",), ("n_centres", 2), ("cluster", first), ("cluster", mid), ("no_cluster_with", 1440 - 4)]))
    # A4: the circle threshold, ulp by ulp.  angle_max - angle_min is a float32 difference: k = 0..3 round to at most 2 pi + 6.6e-7,
    # k = 4, 5 to 2 pi + 1.13e-6.  The 2-beam run at beam 0 is a reflector only on a circle.
    for k in range(6):
        amax = f32(math.pi)
        for _ in range(k):
            amax = np.nextafter(amax, f32(4.0))
        sc = make_scan(1440, f32(-math.pi), 2.0 * math.pi / 1440, angle_max=amax)
        two, p1, p2 = put(sc, 0, 2, R17), put(sc, 400, 17, R17), put(sc, 1000, 17, R17)
        circle = k <= 3
        out.append(case(f"A4_ulp{k}", sc, [("circle",) if circle else ("not_circle",), ("n_centres", 3 if circle else 2), ("cluster", p1), ("cluster", p2),
                                            ("cluster", two) if circle else ("no_cluster_with", 0)]))
    # A5: a negative increment with angle_max > angle_min is accepted (and every gap beam's angle is angle - inc * k with inc < 0)
    sc = make_scan(1081, 2.0, -QUARTER_DEG, angle_max=2.5)
    ids = [put(sc, 200, 17, R17), put(sc, 600, 18, R17), put(sc, 1000, 17, R17)]
    dim(sc, 208, 608, 609)
    c = case("A5", sc, [("circle",), ("n_centres", 3)] + [("cluster", i) for i in ids])
    out += [c, with_odom(c)]
    # ... the real clockwise message is refused on all sides
    sc = make_scan(1081, 2.0, -QUARTER_DEG, angle_max=2.0 - 270.0 * DEG)
    put(sc, 200, 17, R17)
    out.append(case("A5_clockwise_refused", sc, [("bad_scan",)]))
    # A6: scan_time = 0: every beam has the stamp's time
    sc = a1(scan_time=0.0)
    ids = [put(sc, 254, 17, R17), put(sc, 500, 17, R17), put(sc, 1022, 15, R15)]
    dim(sc, 508)
    c = case("A6", sc, [("n_centres", 3)] + [("cluster", i) for i in ids])
    out += [c, case("A6_odom", sc, c["claims"], odom=drive())]
    # A7: the LDS maximum, eight beams per thread: plates across 1023 / 1024 and 4095 / 4096, a bridged gap further on
    inc7 = 2.0 * math.pi / 8192
    r40 = range_for(40, inc7)
    sc = make_scan(8192, -math.pi, inc7)
    ids = [put(sc, 1004, 40, r40), put(sc, 4076, 40, r40), put(sc, 7000, 40, r40)]
    dim(sc, 7020)
    c = case("A7", sc, [("n_centres", 3)] + [("cluster", i) for i in ids], s2b=S2B_TURNED)
    out += [c, with_odom(c)]
    return out


# ---------------------------------------------------------------------------------------------------------------- family B
def family_b():
    out = []
    # i - 1 bright, i dim, i + 1 bright on every mask, halo and thread-stride edge: a bridged one-beam gap, the gap beam a member
    for i in (63, 64, 255, 256, 257, 1023, 1024):
        sc = a1()
        ids = put(sc, i - 8, 17, R17)
        dim(sc, i)
        out.append(case(f"B_dim_{i}", sc, [("n_centres", 1), ("cluster", ids), ("gap_member", i)]))
    # two-beam gaps on the workgroup edge are bridged (i - last = 3) ...
    for g in ((255, 256), (254, 255)):
        sc = a1()
        ids = put(sc, g[0] - 8, 18, R17)
        dim(sc, *g)
        out.append(case(f"B_gap2_{g[0]}_{g[1]}", sc, [("n_centres", 1), ("cluster", ids), ("gap_member", g[0]), ("gap_member", g[1])]))
    # ... a three-beam gap (i - last = 4) is not: two reflectors, each of which passes the gate alone
    sc = a1()
    left, right = put(sc, 241, 14, R17), put(sc, 258, 14, R17)
    put(sc, 255, 3, R17, DIM)
    out.append(case("B_gap3_255_257", sc, [("n_centres", 2), ("cluster", left), ("cluster", right), ("no_cluster_with", 256)]))
    # a bridge whose bright beam is the scan's last beam (its "next beam" is itself), and one whose bright beam is N - 2
    n = 1081
    sc = a1()
    ids = put(sc, n - 17, 17, R17)
    dim(sc, n - 2)
    out.append(case("B_bridge_at_last_beam", sc, [("n_centres", 1), ("cluster", ids), ("gap_member", n - 2)]))
    sc = a1()
    ids = put(sc, n - 17, 17, R17)
    dim(sc, n - 3)
    out.append(case("B_bridge_at_last_but_one", sc, [("n_centres", 1), ("cluster", ids), ("gap_member", n - 3)]))
    sc = a1()
    ids = put(sc, n - 17, 14, R17)                  # N - 17 .. N - 4 bright, N - 3 dim, N - 2 bright, N - 1 dim: the bridge is refused
    put(sc, n - 3, 3, R17, DIM)
    dim(sc, n - 2, inten=BRIGHT)
    out.append(case("B_bridge_at_last_but_one_refused", sc, [("n_centres", 1), ("cluster", ids), ("no_cluster_with", n - 2)]))
    # clusters longer than a wave: 84 beams across beam 256 with a bridged gap behind the 64th member; 150 beams with two
    r84, r150 = range_for(84), range_for(150)
    sc = a1()
    ids = put(sc, 200, 84, r84)
    dim(sc, 270)
    out.append(case("B_cluster_84", sc, [("n_centres", 1), ("cluster", ids), ("gap_member", 270), ("size_gt", 200, 64)]))
    sc = a1()
    ids = put(sc, 180, 150, r150)
    dim(sc, 250, 310, 311)
    out.append(case("B_cluster_150", sc, [("n_centres", 1), ("cluster", ids), ("gap_member", 311), ("size_gt", 180, 128)], opts=dict(range_min=0.1)))
    # a seam cluster whose two segments are 3 and 70 beams, either way round
    sc = a2()
    head, tail = put(sc, 0, 3, 0.5), put(sc, 1440 - 70, 70, 0.5)
    out.append(case("B_seam_3_and_70", sc, [("n_centres", 1), ("cluster", head + tail)]))
    sc = a2()
    head, tail = put(sc, 0, 70, 0.5), put(sc, 1440 - 3, 3, 0.5)
    dim(sc, 66)
    out.append(case("B_seam_70_and_3", sc, [("n_centres", 1), ("cluster", head + tail), ("gap_member", 66)]))
    # beams per thread 2, 2, 1, 1; a workgroup / mask edge + 1: the last plate ends at N - 1
    for n in (1081, 1025, 257, 65):
        sc = a1(N=n)
        ids = [put(sc, 20, 17, R17), put(sc, n - 17, 17, R17)]
        dim(sc, n - 9)
        out.append(case(f"B_N{n}", sc, [("n_centres", 2), ("cluster", ids[0]), ("cluster", ids[1])]))
    # the first and the last beam inside the message's range on a 64-beam probe edge and one beyond it.  Bright beams in front of the
    # first valid beam have no point (skipped); bright beams behind the last one repeat its point (point_cloud.back())
    n = 1081
    for s in (0, 1):
        fv, lv = 64 + s, n - 65 + s
        sc = a1(range_max=5.0, base_range=4.0)
        sc.ranges[:fv] = 8.0
        sc.ranges[lv + 1:] = 8.0
        head, tail = put(sc, fv, 17, R17), put(sc, lv - 16, 17, R17)
        dim(sc, *range(fv - 6, fv), inten=BRIGHT)
        dim(sc, *range(lv + 1, lv + 6), inten=BRIGHT)
        out.append(case(f"B_valid_from_{fv}_to_{lv}", sc, [("n_centres", 2), ("cluster", head), ("cluster", tail + list(range(lv + 1, lv + 6))),
                                                           ("no_cluster_with", fv - 1), ("bright_member", lv + 5), ("n_returns", lv - fv + 1)]))
    return out


# ---------------------------------------------------------------------------------------------------------------- family C
WIDE_GATE = dict(reflector_min_length=0.35, reflector_length_error=0.25)     # 0.10 .. 0.60 m: a plate with a 0.3 m range step passes


def width_sweep_plates():
    """[(first beam, nb)] of C_width_sweep: nb = 1 .. 34 (twice the nominal 17) at one range, six far dim beams between two plates."""
    out, first = [], 5
    for nb in range(1, 35):
        out.append((first, nb))
        first += nb + 6
    return out


def family_c():
    out = []
    # intensity == intensity_min is NOT bright: inside a plate it is a bridged gap beam ...
    sc = a1()
    ids, other = put(sc, 300, 17, R17), put(sc, 700, 21, R21)
    dim(sc, 308, inten=160.0)
    out.append(case("C_intensity_tie_inside", sc, [("n_centres", 2), ("cluster", ids), ("gap_member", 308), ("cluster", other)]))
    # ... behind a plate's last beam it stays out of the reflector (as a bright beam it would be its 18th member) ...
    sc = a1()
    ids, other = put(sc, 300, 17, R17), put(sc, 700, 21, R21)
    put(sc, 317, 1, R17, 160.0)
    out.append(case("C_intensity_tie_behind_a_plate", sc, [("n_centres", 2), ("cluster", ids), ("no_cluster_with", 317), ("cluster", other)]))
    # ... and as the beam after a bridge candidate it refuses the bridge: 300..313 | 314 dim | 315 candidate, 316 at the tie, 317..328
    sc = a1()
    left, right = put(sc, 300, 14, R17), put(sc, 315, 14, R17)
    put(sc, 314, 1, R17, DIM)
    dim(sc, 316, inten=160.0)
    out.append(case("C_intensity_tie_after_candidate", sc, [("n_centres", 2), ("cluster", left), ("cluster", right), ("gap_member", 316), ("no_cluster_with", 314)]))
    # the detector's gate is inclusive at both ends, and so are the message's limits
    sc = a1()
    ids, other = put(sc, 300, 84, 0.5), put(sc, 700, 21, R21)
    out.append(case("C_range_at_detector_min", sc, [("n_centres", 2), ("cluster", ids), ("cluster", other)], opts=dict(range_min=0.5)))
    sc = a1()
    ids, other = put(sc, 300, 17, 2.5), put(sc, 700, 21, R21)
    out.append(case("C_range_at_detector_max", sc, [("n_centres", 2), ("cluster", ids), ("cluster", other)], opts=dict(range_max=2.5)))
    sc = a1(range_min=0.5)
    ids, other = put(sc, 300, 84, 0.5), put(sc, 700, 21, R21)
    out.append(case("C_range_at_message_min", sc, [("n_centres", 2), ("cluster", ids), ("cluster", other), ("n_returns", 1081)]))
    sc = a1(range_max=2.5, base_range=2.0)
    ids, other = put(sc, 300, 17, 2.5), put(sc, 700, 21, R21)
    out.append(case("C_range_at_message_max", sc, [("n_centres", 2), ("cluster", ids), ("cluster", other), ("n_returns", 1081)]))
    # the width gate: nb = 1 .. 34 beams at the range where 17 are nominal
    sc = a1()
    plates = width_sweep_plates()
    for first, nb in plates:
        put(sc, first, nb, R17)
    out.append(case("C_width_sweep", sc, [("width_sweep", plates, 17)]))
    # the bridge's range step |r_i - r_last| < 0.3 in float32: 3.0 against 3.29, 3.3 (float32: 0.29999995), 3.3000002, 3.31
    for label, far, bridged in (("3.29", 3.29, True), ("3.3", 3.3, True), ("3.3000002", 3.3000002, False), ("3.31", 3.31, False)):
        sc = a1()
        left, right = put(sc, 300, 12, 3.0), put(sc, 313, 12, f32(far))
        put(sc, 312, 1, 3.0, DIM)
        claims = [("n_centres", 1), ("cluster", left + [312] + right)] if bridged else [("n_centres", 2), ("cluster", left), ("cluster", right)]
        out.append(case(f"C_range_step_{label}", sc, claims, opts=WIDE_GATE))
    # a bridged gap beam with a NaN range is pushed (the reference skips isinf only): a NaN centre
    sc = a1()
    ids, other = put(sc, 300, 17, R17), put(sc, 700, 21, R21)
    put(sc, 308, 1, np.nan, DIM)
    out.append(case("C_nan_range_at_gap_beam", sc, [("nan_centre",), ("n_centres", 2), ("cluster", ids), ("cluster", other), ("n_returns", 1080)]))
    # ... +inf and -inf are skipped
    for label, v in (("pos", np.inf), ("neg", -np.inf)):
        sc = a1()
        ids, other = put(sc, 300, 18, R17), put(sc, 700, 21, R21)
        put(sc, 308, 1, v, DIM)
        out.append(case(f"C_{label}_inf_range_at_gap_beam", sc, [("n_centres", 2), ("cluster", [b for b in ids if b != 308]), ("cluster", other), ("n_returns", 1080)]))
    # a NaN range under a bright intensity is outside the gate: a gap beam, bridged, pushed: NaN centre
    sc = a1()
    ids, other = put(sc, 300, 17, R17), put(sc, 700, 21, R21)
    sc.ranges[309] = np.nan
    out.append(case("C_nan_range_at_bright_beam", sc, [("nan_centre",), ("n_centres", 2), ("cluster", ids), ("gap_member", 309), ("cluster", other)]))
    # a NaN intensity is not bright (a gap beam); +inf is
    sc = a1()
    ids, other = put(sc, 300, 17, R17), put(sc, 700, 21, R21)
    sc.intensities[307] = np.nan
    out.append(case("C_nan_intensity", sc, [("n_centres", 2), ("cluster", ids), ("gap_member", 307), ("cluster", other)]))
    sc = a1()
    left, right = put(sc, 300, 8, R17), put(sc, 309, 8, R17)       # 308 dim, 309 bright, 310 +inf: the bridge needs 310 bright
    put(sc, 308, 1, R17, DIM)
    sc.intensities[310] = np.inf
    out.append(case("C_inf_intensity", sc, [("n_centres", 1), ("cluster", left + [308] + right), ("bright_member", 310)]))
    # a negative range under a bright intensity: outside the gate and the message range, finite: a gap beam with a mirrored point
    sc = a1()
    ids, other = put(sc, 300, 17, R17), put(sc, 700, 21, R21)
    sc.ranges[305] = -R17
    out.append(case("C_negative_range", sc, [("n_centres", 2), ("cluster", ids), ("gap_member", 305), ("cluster", other), ("n_returns", 1080)]))
    # bright beams beyond the message's range_max, inside the detector's gate: they take point_cloud.back(), the point of a beam
    # on the other side of the 256-beam workgroup edge
    r23 = range_for(23)
    sc = a1(range_max=2.0, base_range=1.0)
    ids = put(sc, 245, 23, r23)
    sc.ranges[256] = sc.ranges[257] = 2.1
    out.append(case("C_bright_beyond_message_max_at_256", sc, [("n_centres", 1), ("cluster", ids), ("bright_member", 256), ("n_returns", 1079)]))
    return out


# ---------------------------------------------------------------------------------------------------------------- family D
def _d_scan(geo):
    if geo == "A1":
        sc = a1()
        ids = [put(sc, 100, 17, R17), put(sc, 500, 17, R17), put(sc, 900, 21, R21)]
        dim(sc, 508)
    else:
        sc = a2()
        ids = [put(sc, 200, 17, R17), put(sc, 700, 17, R17), put(sc, 1200, 21, R21)]
        dim(sc, 708)
    return sc, [("n_centres", 3)] + [("cluster", i) for i in ids]


def family_d():
    out = []
    for geo in ("A1", "A2"):
        sc, claims = _d_scan(geo)
        still = f"D_{geo}_still"
        out.append(case(still, sc, claims))
        moving = claims + [("returns_differ", still), ("centres_differ", still)]
        t_first = sc.stamp - sc.scan_time                     # (scan_time is float32(0.1) as a double: what the trim compares with)
        # start yaw beyond +-pi (qw < 0 for 3.5 and 5.5), a sideways velocity, |wz| = 2, far from the origin
        for th0, wz in ((2.0, 2.0), (3.5, 2.0), (5.5, -2.0), (-3.0, -2.0)):
            out.append(case(f"D_{geo}_yaw{th0}", sc, moving, odom=odom_track(ticks(sc.stamp, -15, 2), th0=th0, wz=wz)))
        # every sample after the stamp; one sample, inside the sweep; 4 Hz samples that straddle the sweep (a time between two
        # samples takes the LAST one); samples the trim must drop, and the twin that never had them
        out.append(case(f"D_{geo}_samples_after", sc, moving, odom=odom_track(ticks(sc.stamp, 1, 3), th0=3.5)))
        out.append(case(f"D_{geo}_one_sample_inside", sc, moving, odom=odom_track([sc.stamp - 0.04], th0=5.5, wz=-2.0)))
        out.append(case(f"D_{geo}_4hz_straddle", sc, moving, odom=odom_track([sc.stamp - 0.30, sc.stamp - 0.05, sc.stamp + 0.20], th0=2.0)))
        full = odom_track(ticks(sc.stamp, -50, 2), th0=-3.0, wz=2.0)
        kept = [o for o in full if o[0] >= t_first]
        assert 3 <= len(kept) < len(full) - 10
        out.append(case(f"D_{geo}_trimmed", sc, moving, odom=kept))
        out.append(case(f"D_{geo}_trim", sc, moving + [("same_as", f"D_{geo}_trimmed")], odom=full))
    return out


FAMILIES = dict(A=family_a, B=family_b, C=family_c, D=family_d)


def all_cases():
    return [c for fam in FAMILIES.values() for c in fam()]


# ---------------------------------------------------------------------------------------------------------------- the witness side
def options(c):
    return dict(DEFAULTS, **c["opts"])


def run_witness(c):
    """-> (centres, members, returns) of tests/witness/detect2d_witness.py, or BAD_SCAN where it refuses the message."""
    from tests.witness.detect2d_witness import Extrapolator, detect2d_witness
    ex = Extrapolator()
    for o in c["odom"]:
        ex.add(o)
    o = options(c)
    try:
        return detect2d_witness(c["scan"], ex, intensity_min=o["intensity_min"], reflector_min_length=o["reflector_min_length"],
                                reflector_length_error=o["reflector_length_error"], det_range_min=o["range_min"], det_range_max=o["range_max"],
                                s2b=c["s2b"])
    except ValueError:
        return BAD_SCAN


def witness_results(cases):
    return {c["name"]: run_witness(c) for c in cases}


def claims_nan(c):
    return ("nan_centre",) in c["claims"]


def is_circle(sc):
    return (float(f32(f32(sc.angle_max) - f32(sc.angle_min))) - 2.0 * math.pi) < 1e-6


def _bright(c):
    """Inside the detector's gate with an intensity above the threshold (the reference's :77-82)."""
    o, sc = options(c), c["scan"]
    return (f32(o["range_min"]) <= sc.ranges) & (sc.ranges <= f32(o["range_max"])) & (sc.intensities.astype(np.float64) > o["intensity_min"])


def check_claims(c, results):
    """Asserts every claim of case c on the witness's results (``results``: name -> run_witness output, all cases)."""
    name, sc = c["name"], c["scan"]
    res = results[name]
    if ("bad_scan",) in c["claims"]:
        assert res == BAD_SCAN, name
        return
    assert res != BAD_SCAN, name
    centres, members, returns = res
    lists = [m.tolist() for m in members]
    assert len(lists) == centres.shape[0], name
    with np.errstate(invalid="ignore"):
        bright = _bright(c)
    if not claims_nan(c):
        assert np.isfinite(centres).all() and np.isfinite(returns).all(), name
    holding = lambda b: [m for m in lists if b in m]
    for claim in c["claims"]:
        kind, a = claim[0], claim[1:]
        where = (name, claim)
        if kind == "circle":
            assert is_circle(sc), where
        elif kind == "not_circle":
            assert not is_circle(sc), where
        elif kind == "n_centres":
            assert centres.shape[0] == a[0], where + (centres.shape[0],)
        elif kind == "min_centres":
            assert centres.shape[0] >= a[0], where
        elif kind == "n_returns":
            assert returns.shape[0] == a[0], where + (returns.shape[0],)
        elif kind == "cluster":                               # exactly these beams, in this order
            assert list(a[0]) in lists, where
        elif kind == "no_cluster_with":
            assert not holding(a[0]), where
        elif kind == "gap_member":                            # a member that is not a bright beam
            assert holding(a[0]) and not bright[a[0]], where
        elif kind == "bright_member":
            assert holding(a[0]) and bright[a[0]], where
        elif kind == "size_gt":
            assert len(holding(a[0])) == 1 and len(holding(a[0])[0]) > a[1], where
        elif kind == "gap_angle_gt":
            ang = sc.angle_min + sc.angle_increment * np.arange(sc.ranges.shape[0])
            assert any(not bright[b] and ang[b] > a[0] for m in lists for b in m), where
        elif kind == "nan_centre":
            assert np.isnan(centres).any(), where
        elif kind == "returns_differ":
            other = results[a[0]][2]
            assert other.shape == returns.shape and not np.array_equal(other, returns), where
        elif kind == "centres_differ":
            other = results[a[0]][0]
            assert other.shape != centres.shape or not np.array_equal(other, centres), where
        elif kind == "same_as":
            assert np.array_equal(results[a[0]][0], centres) and np.array_equal(results[a[0]][2], returns), where
        elif kind == "width_sweep":                           # both outcomes occur, the accepted widths are an interval that holds the nominal one
            accepted = [nb for first, nb in a[0] if list(range(first, first + nb)) in lists]
            assert accepted and len(accepted) < len(a[0]) and accepted == list(range(accepted[0], accepted[-1] + 1)) and a[1] in accepted, where + (accepted,)
            assert len(lists) == len(accepted), where
        elif kind != "bad_scan":
            raise AssertionError(f"unknown claim {claim!r} in {name}")


# the cases every family must hold (tests/test_detect2d_sweep_cpu.py)
REQUIRED = dict(
    A=["A1", "A1_odom", "A2", "A2_odom", "A3", "A3_odom", "A3_as_circle", "A3_seam_run_short_of_the_end", "A4_ulp0", "A4_ulp1", "A4_ulp2", "A4_ulp3", "A4_ulp4", "A4_ulp5",
       "A5", "A5_odom", "A5_clockwise_refused", "A6", "A6_odom", "A7", "A7_odom"],
    B=[f"B_dim_{i}" for i in (63, 64, 255, 256, 257, 1023, 1024)] + ["B_gap2_255_256", "B_gap2_254_255", "B_gap3_255_257", "B_bridge_at_last_beam",
       "B_bridge_at_last_but_one", "B_bridge_at_last_but_one_refused", "B_cluster_84", "B_cluster_150", "B_seam_3_and_70", "B_seam_70_and_3",
       "B_N1081", "B_N1025", "B_N257", "B_N65", "B_valid_from_64_to_1016", "B_valid_from_65_to_1017"],
    C=["C_intensity_tie_inside", "C_intensity_tie_behind_a_plate", "C_intensity_tie_after_candidate", "C_range_at_detector_min", "C_range_at_detector_max", "C_range_at_message_min",
       "C_range_at_message_max", "C_width_sweep", "C_range_step_3.29", "C_range_step_3.3", "C_range_step_3.3000002", "C_range_step_3.31",
       "C_nan_range_at_gap_beam", "C_pos_inf_range_at_gap_beam", "C_neg_inf_range_at_gap_beam", "C_nan_range_at_bright_beam", "C_nan_intensity",
       "C_inf_intensity", "C_negative_range", "C_bright_beyond_message_max_at_256"],
    D=[f"D_{g}_{k}" for g in ("A1", "A2") for k in ("still", "yaw2.0", "yaw3.5", "yaw5.5", "yaw-3.0", "samples_after", "one_sample_inside",
                                                    "4hz_straddle", "trim")],
)
