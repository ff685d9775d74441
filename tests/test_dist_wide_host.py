"""The reach of get_dist as the interface states it (no GPU needed): the limit in the header and its mirror in hip.py,
and the window the reference's rule (sobel.f90:129-137) picks on a km-scale grid."""
import os
import re

import numpy as np
import pytest

from seabreeze_param_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_limit_matches_the_header():
    with open(os.path.join(ROOT, "include", "seabreeze_hip.h")) as f:
        m = re.search(r"^#define\s+SB_DIST_MAX_WINDOW\s+(\d+)\s*$", f.read(), re.M)
    assert m, "include/seabreeze_hip.h does not define SB_DIST_MAX_WINDOW"
    assert hip.SB_DIST_MAX_WINDOW == int(m.group(1)) == 255


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_window_of_a_regional_grid(dt):
    """0.0135 degrees near 70 N, 180 km: 113 cells, within the limit"""
    lon = (10.0 + 0.0135 * np.arange(704)).astype(dt)
    lat = (68.0 + 0.0135 * np.arange(200)).astype(dt)
    assert hip.dist_window(lon, lat) == 113 <= hip.SB_DIST_MAX_WINDOW
