"""An independent statement of the reference's voxel filters (sensor/voxel_filter.cc, common/math.h), written from reading the
reference and from nothing else: not from oracle/grid_oracle.c, not from the kernels.  It is slow and plain on purpose.

What the reference's text says, and how it is said here:

* ``GetCellIndex``: the point is a ``Vector3f``, the resolution a ``float``: the quotient is ONE IEEE float32 division.  numpy's
  float32 ``/`` is that division.  ``RoundToInt`` is ``lround`` of the float: to nearest, ties away from zero, exactly.  A float32
  ``q`` has 24 significant bits, so ``|q| + 0.5`` is exact in float64 for every ``|q| < 2**28`` (far beyond any voxel index that
  fits an int), and ``floor`` of it is the tie-away rounding without a rounding of its own.
* ``IndexToKey``: each int index is cast to uint32 (two's complement wrap) and the three are packed, x highest, into 96 bits.  Here it
  is a Python integer; z is 0.
* ``VoxelFilter::Filter``: one pass in input order, a point stays iff its key was not in the set yet.  A Python ``set``.  The points
  are copied, never recomputed: the output's bit patterns are the input's (-0.0 stays -0.0).  The set is a member of the filter
  object, and the callers build one object per cloud: returns and misses do not share voxels.
* ``AdaptiveVoxelFilter::Filter``: ``point.norm() <= max_range`` with ``max_range`` passed as ``float`` and a ``Vector2f`` norm, so
  everything in float32; ``size() <= min_num_points`` and ``size() >= min_num_points`` with a ``double`` option, so the counts are
  compared in double (a fractional min_num_points means what it says); ``VoxelFilter(options.max_length)`` narrows the double to
  float; ``high_length`` and ``low_length`` are floats, halved and averaged in float32; the ladder's bound
  ``1e-2f * options.max_length`` is a float times a DOUBLE, so that comparison is in double; the bisection's
  ``(high - low) / low > 1e-1f`` is all float32.  The ladder and the bisection run one filter at a time, as written.

``mutant=`` plants one defect, for tests/test_voxel_witness_cpu.py to show that the cases would notice it.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
MUTANTS = ("half_even", "truncate", "floor_half", "double_division", "last_occurrence", "shared_set", "gate_lt", "gate_double",
           "size_lt", "count_gt", "ladder_ge", "reject_overwrites", "tolerance_double")
_MASK = 0xFFFFFFFF


def _cloud(points):
    return np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 2)


def cell_index(v, size, mutant=None):
    """RoundToInt(v / size) for float32 ``v`` (any shape) and a float32 ``size`` -> int64."""
    v, size = np.asarray(v, np.float32), F32(size)
    if mutant == "double_division":
        q = v.astype(np.float64) / np.float64(size)
    else:
        q = (v / size).astype(np.float64)             # the float32 quotient, then held exactly
    if mutant == "half_even":
        r = np.rint(q)
    elif mutant == "truncate":
        r = np.trunc(q)
    elif mutant == "floor_half":
        r = np.floor(q + 0.5)
    else:
        r = np.copysign(np.floor(np.abs(q) + 0.5), q)
    return r.astype(np.int64)


def index_to_key(ix, iy, iz=0):
    """The 96-bit key of an index, as a Python integer."""
    return ((int(ix) & _MASK) << 64) | ((int(iy) & _MASK) << 32) | (int(iz) & _MASK)


def keys_of(points, size, mutant=None):
    idx = cell_index(_cloud(points), size, mutant)
    return [index_to_key(ix, iy) for ix, iy in idx.tolist()]


def voxel_filter(points, size, mutant=None, voxel_set=None):
    """VoxelFilter(size).Filter(points) -> the kept points, float32 (m, 2).  ``voxel_set`` is the filter object's set."""
    p = _cloud(points)
    seen = set() if voxel_set is None else voxel_set
    keys = keys_of(p, size, mutant)
    kept = []
    if mutant == "last_occurrence":
        for i in range(len(keys) - 1, -1, -1):
            if keys[i] not in seen:
                seen.add(keys[i])
                kept.append(i)
        kept.reverse()
    else:
        for i, k in enumerate(keys):
            if k not in seen:
                seen.add(k)
                kept.append(i)
    return p[np.asarray(kept, dtype=np.int64)].copy() if kept else np.zeros((0, 2), np.float32)


def range_gate(points, max_range, mutant=None):
    p = _cloud(points)
    limit = F32(max_range)
    if mutant == "gate_double":
        d = p.astype(np.float64)
        norm = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    else:
        norm = np.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1])        # float32 products, sum and root
    return p[norm < limit] if mutant == "gate_lt" else p[norm <= limit]


def _keep_going(high, low, mutant):
    ratio = F32(F32(high - low) / low)
    if mutant == "tolerance_double":                  # `> 1e-1` for `> 1e-1f`: the float ratio against the double constant
        return np.float64(ratio) > 0.1
    return ratio > F32(1e-1)


def adaptive_voxel_filter(points, max_length=0.9, min_num_points=500.0, max_range=100.0, mutant=None):
    """AdaptiveVoxelFilter(options).Filter(points) -> (cloud, label).  Labels: ("sparse",), ("first",),
    ("ladder", rung, trace) -- rung counts the ladder's iterations from 1, trace has a letter per bisection step, A for a candidate
    that was dense enough and became the result, R for one that was not -- and ("nothing", rungs tried)."""
    with np.errstate(over="ignore", invalid="ignore"):
        p = range_gate(points, max_range, mutant)
        minimum = float(min_num_points)
        n = float(p.shape[0])
        if (n < minimum) if mutant == "size_lt" else (n <= minimum):
            return p.copy(), ("sparse",)

        def dense(c):
            return float(c.shape[0]) > minimum if mutant == "count_gt" else float(c.shape[0]) >= minimum

        result = voxel_filter(p, F32(max_length), mutant)
        if dense(result):
            return result, ("first",)
        bound = np.float64(F32(1e-2)) * np.float64(max_length)
        high, rung = F32(max_length), 0
        while (np.float64(high) >= bound) if mutant == "ladder_ge" else (np.float64(high) > bound):
            rung += 1
            low = F32(high / F32(2))
            result = voxel_filter(p, low, mutant)
            if dense(result):
                trace = ""
                while _keep_going(high, low, mutant):
                    mid = F32(F32(low + high) / F32(2))
                    candidate = voxel_filter(p, mid, mutant)
                    if dense(candidate):
                        low, result, trace = mid, candidate, trace + "A"
                    else:
                        high, trace = mid, trace + "R"
                        if mutant == "reject_overwrites":
                            result = candidate
                return result, ("ladder", rung, trace)
            high = F32(high / F32(2))
        return result, ("nothing", rung)


def filter_scan(returns, misses, size=0.025, max_length=0.9, min_num_points=500.0, max_range=100.0, mutant=None):
    """What the map builder does with one scan: VoxelFilter(size) of the returns, another VoxelFilter(size) of the misses, the
    adaptive filter of the first -> (returns, misses, filtered, label)."""
    shared = set() if mutant == "shared_set" else None
    fr = voxel_filter(returns, size, mutant, shared)
    fm = voxel_filter(np.zeros((0, 2), np.float32) if misses is None else misses, size, mutant, shared)
    av, label = adaptive_voxel_filter(fr, max_length, min_num_points, max_range, mutant)
    return fr, fm, av, label
