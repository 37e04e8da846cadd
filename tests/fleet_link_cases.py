"""Scan builders shared by tests/test_fleet_link_cpu.py (which holds their reflector counts against the CPU oracle) and
tests/test_fleet_link_gpu.py (which needs members that see exactly 1, 31, 32, 33, 64 or 65 centres)."""
from tests.detect_cases import beams_for_width


def plates(k, n_beams, first=10, r0=3.0):
    """k plates of 0.18 m for ``detect_cases.plate_scan`` that the 2D detector accepts with its default options: none at the scan's
    ends, each at its own range between r0 and r0 + 0.36, 20 beams apart in a 720-beam scan and 30 otherwise."""
    stride = 20 if n_beams == 720 else 30
    assert first + k * stride < n_beams - 10
    out = []
    for j in range(k):
        r = r0 + 0.04 * ((j * 7) % 10)
        out.append((first + j * stride, beams_for_width(0.18, r, n_beams), r, 200.0))
    return out
