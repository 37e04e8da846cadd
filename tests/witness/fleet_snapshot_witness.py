"""The snapshot blob of include/rfleet.h, written and parsed in numpy from the header's text alone: rfleet_snapshot_hdr (8 bytes of
magic, int version, int count, long bytes), `count` rfleet_snapshot_member entries (double t, double vt[3], int member, int n, int
flags, int pad_, long off) in the order listed, and at byte offset `off` of each entry mu[0:n] followed by the packed lower triangle
of the covariance, n (n + 1) / 2 doubles, column-major (column j holds rows j .. n-1), the payloads one behind the other without
gaps.  Shares no code with reflector_ekf_slam_amd/fleet.py.

An entry is a record with the fields member, t, vt [3], n, flags, mu [n] and sigma [n, n] (dense; only its lower triangle counts).
``pack(entries, defect=...)`` plants one of DEFECTS, for the tests that show the comparison catches it."""
from __future__ import annotations

import struct
from types import SimpleNamespace as NS

import numpy as np

MAGIC = b"RFLTSNAP"
VERSION = 1
HDR = struct.Struct("<8siiq")
ENTRY = struct.Struct("<ddddiiiiq")
DEFECTS = ("row_major", "strict_triangle", "off_by_one_entry", "index_order")


def triangle_of(sigma, defect=None):
    low = np.tril(np.asarray(sigma, np.float64))
    n = low.shape[0]
    if defect == "row_major":
        return np.concatenate([low[i, : i + 1] for i in range(n)])
    if defect == "strict_triangle":
        return np.concatenate([low[j + 1:, j] for j in range(n)] + [np.zeros(0)])
    return np.concatenate([low[j:, j] for j in range(n)])


def pack(entries, defect=None) -> bytes:
    entries = list(entries)
    if defect == "index_order":
        entries = sorted(entries, key=lambda e: e.member)
    at = HDR.size + ENTRY.size * len(entries)
    heads, payloads = [], []
    for e in entries:
        mu = np.asarray(e.mu, np.float64).reshape(-1)
        assert mu.shape[0] == e.n and np.asarray(e.sigma).shape == (e.n, e.n)
        pay = np.concatenate([mu, triangle_of(e.sigma, defect)]).astype("<f8").tobytes()
        off = at + (ENTRY.size if defect == "off_by_one_entry" and heads else 0)
        heads.append(ENTRY.pack(float(e.t), *(float(v) for v in e.vt), int(e.member), int(e.n), int(e.flags), 0, off))
        payloads.append(pay)
        at += len(pay)
    return HDR.pack(MAGIC, VERSION, len(entries), at) + b"".join(heads) + b"".join(payloads)


def parse(blob):
    """-> the entries of a blob, sigma mirrored.  Asserts the layout the header promises."""
    blob = bytes(blob)
    magic, version, count, size = HDR.unpack_from(blob, 0)
    assert magic == MAGIC and version == VERSION and size == len(blob) and count >= 0
    out = []
    end = HDR.size + ENTRY.size * count
    for g in range(count):
        t, v0, v1, v2, member, n, flags, pad, off = ENTRY.unpack_from(blob, HDR.size + ENTRY.size * g)
        assert n >= 3 and n % 2 == 1 and pad == 0 and off == end and off % 8 == 0, (g, n, pad, off, end)
        k = n * (n + 1) // 2
        vals = np.frombuffer(blob, "<f8", n + k, off)
        end = off + 8 * (n + k)
        low = np.zeros((n, n))
        at = n
        for j in range(n):
            low[j:, j] = vals[at: at + n - j]
            at += n - j
        sigma = low + np.tril(low, -1).T
        out.append(NS(member=member, t=t, vt=np.array([v0, v1, v2]), n=n, flags=flags, mu=vals[:n].copy(), sigma=sigma))
    assert end == len(blob)
    return out
