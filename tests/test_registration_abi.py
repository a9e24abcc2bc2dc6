"""The image registration's ABI surface: the structs of include/msfm_match.h have the sizes the binding and the twin assume, no
implicit padding, and the header declares what the library and the host twin export.  CPU only."""
import ctypes as C
import os
import re

from monocularsfm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_sizes_and_layout():
    assert _lib.REGISTRATION.itemsize == 128 and C.sizeof(_lib.RegisterParams) == 32 and C.sizeof(_lib.RegisterStats) == 48
    off = {k: v[1] for k, v in _lib.REGISTRATION.fields.items()}
    assert [off[k] for k in ("image_id", "status", "n_correspondences", "n_inliers", "hypotheses", "reserved", "R", "t", "mean_residual")] == \
        [0, 4, 8, 12, 16, 20, 24, 96, 120]
    assert _lib.RegisterStats.correspondences.offset == 16 and _lib.RegisterStats.register_ms.offset == 40
    assert (_lib.REG_ATTEMPTED, _lib.REG_POSE, _lib.REG_SUCCEEDED, _lib.REG_REFINED) == (1, 2, 4, 8)


def test_header_declares_the_entry_points_and_sizes():
    text = open(os.path.join(ROOT, "include", "msfm_match.h")).read()
    for name in ("msfm_register_images", "msfm_fetch_registrations"):
        assert re.search(r"\bint %s\(msfm_ctx\* ctx" % name, text), name
        assert name in _lib.EXPORTS, name
    assert "MSFM_REG_ATTEMPTED = 1, MSFM_REG_POSE = 2, MSFM_REG_SUCCEEDED = 4, MSFM_REG_REFINED = 8" in text
    for struct, size in (("msfm_register_params", 32), ("msfm_registration", 128), ("msfm_register_stats", 48)):
        assert re.search(r"typedef struct %s \{\s+/\* %d bytes, no implicit padding \*/" % (struct, size), text), struct


def test_host_twin_exports():
    import registration_twin as tw
    host = tw.load_host()
    for name in ("host_register_images", "host_register_counts", "host_register_sample3", "host_p3p", "host_register_refine"):
        assert hasattr(host, name), name


def test_helpers():
    import numpy as np
    rec = np.zeros(3, _lib.REGISTRATION)
    rec["image_id"] = [4, 7, 9]
    rec["status"] = [15, 3, 7]
    rec["R"][:] = np.eye(3).reshape(9)
    rec["t"][:, 2] = [1.0, 2.0, 3.0]
    assert _lib.registered(rec).tolist() == [True, False, True]
    old = {1: (np.eye(3), np.zeros(3)), 4: None}
    poses = _lib.registered_poses(rec, old)
    assert sorted(poses) == [1, 4, 9] and poses[4][1].tolist() == [0.0, 0.0, 1.0] and poses[9][0].shape == (3, 3) and old[4] is None
