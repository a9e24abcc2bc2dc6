"""The four ordering helpers over Context.visibility()'s arrays (monocularsfm_amd/_lib.py: next_images, local_window,
initial_first_images, initial_second_images) on hand-made arrays, and the route function msfm_vis::vis_route through the host
library.  No GPU."""
import numpy as np
import pytest

import visibility_twin as vtw
from monocularsfm_amd import _lib

P, Q = _lib.VIS_POSED, _lib.VIS_QUERIED


def records(rows):
    """rows: (image_id, flags, n_elements, n_visible, n_points)"""
    r = np.zeros(len(rows), _lib.VISIBILITY)
    for k, row in enumerate(rows):
        r[k] = tuple(row) + (0,)
    return r


REC = records([(2, P, 90, 80, 70), (3, 0, 50, 40, 0), (5, 0, 60, 40, 0), (7, P | Q, 30, 25, 20), (8, 0, 20, 15, 0), (9, 0, 20, 14, 0),
               (11, P, 10, 9, 9), (12, 0, 90, 0, 0)])
ROW = np.asarray([12, 7, 0, 20, 3, 0, 12, 0], np.uint32)   # the row of image 7


def test_next_images():
    assert _lib.next_images(REC) == [3, 5, 8]                      # the tie 40 / 40 by id; 9 sees 14 < 15; posed images never
    assert _lib.next_images(REC, min_visible=14) == [3, 5, 8, 9]   # ... the edge
    assert _lib.next_images(REC, min_visible=16) == [3, 5]
    assert _lib.next_images(REC, min_visible=0) == [3, 5, 8, 9, 12]
    assert _lib.next_images(REC, min_visible=41) == []
    assert _lib.next_images(REC[[0, 3, 6]], min_visible=0) == []   # every image posed
    assert all(isinstance(i, int) for i in _lib.next_images(REC))


def test_local_window():
    assert _lib.local_window(ROW, REC, 7) == [2, 11]               # the tie 12 / 12 by id; itself and the unposed left out
    assert _lib.local_window(ROW, REC, 7, size=1) == [2]
    assert _lib.local_window(ROW, REC, 7, size=50) == [2, 11]      # size larger than the candidates
    assert _lib.local_window(ROW, REC, 7, size=0) == []
    zero = ROW.copy()
    zero[0] = 0
    assert _lib.local_window(zero, REC, 7) == [11]                 # zeros left out
    assert _lib.local_window(ROW, REC, 11) == [7, 2]               # (read as another image's row: 20 for image 7 beats 12)
    assert _lib.local_window(np.zeros(8, np.uint32), REC, 7) == []


def test_initial_first_images():
    assert _lib.initial_first_images(REC) == [2, 12, 5, 3, 7, 8, 9, 11]   # 90 / 90 and 20 / 20 by id
    assert _lib.initial_first_images(REC[:0]) == []


def test_initial_second_images():
    assert _lib.initial_second_images(ROW, REC, 7) == [2, 11, 3, 8]       # posed or not; itself and zeros left out
    assert _lib.initial_second_images(ROW, REC, 2) == [7, 11, 3, 8]
    assert _lib.initial_second_images(np.zeros(8, np.uint32), REC, 7) == []


@pytest.fixture(scope="module")
def host():
    return vtw.load_host()


SHAPES = [(n, q, T, O) for n in (1, 2, 65, 300, 2730, 5461, 5462, 10000) for q in (0, 1, 5, 300) if q <= n
          for (T, O) in ((0, 0), (10, 30), (1000, 4095), (1000, 4096), (200000, 10 ** 6))]


def test_route_function(host):
    A, G, L = _lib.VIS_ROUTE_AUTO, _lib.VIS_ROUTE_GLOBAL, _lib.VIS_ROUTE_LDS
    for n, q, T, O in SHAPES:
        g = vtw.route(host, G, n, q, T, O)
        assert g == {"route": G, "lds_bytes": 0, "matrix_in_lds": 0, "wgs_per_cu": 0}
        lds = vtw.route(host, L, n, q, T, O)
        fits = 12 * n <= 64 * 1024   # the 3 n per-image words in the 64 KiB one workgroup gets
        assert (lds["route"] == L) == fits, (n, q)
        if fits:
            with_matrix = q > 0 and 12 * n + 4 * q * n <= 32 * 1024
            assert lds["matrix_in_lds"] == int(with_matrix)
            assert lds["lds_bytes"] == 12 * n + (4 * q * n if with_matrix else 0)
            assert lds["wgs_per_cu"] == min(8, 160 * 1024 // lds["lds_bytes"]) >= 2
        else:
            assert lds == dict.fromkeys(vtw.ROUTE_KEYS, 0)   # refused: exactly where it reports no fit
        auto = vtw.route(host, A, n, q, T, O)
        assert auto in (g, lds) and auto["route"] in (G, L)
        assert auto == (lds if fits else g)   # the rule of DESIGN.md section 24: privatise wherever the counters fit
