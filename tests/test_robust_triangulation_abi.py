"""The robust track triangulation's ABI surface: the structs of include/msfm_match.h have the sizes the binding and the twin assume,
no implicit padding, and the header declares what the library and the host twin export.  CPU only."""
import ctypes as C
import os
import re
import subprocess

from monocularsfm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_sizes_and_layout():
    P, S = _lib.RobustTriangulationParams, _lib.RobustStats
    assert C.sizeof(P) == 24 and C.sizeof(S) == 40 and _lib.TRI_ROBUST == 32
    assert [getattr(P, k).offset for k in ("max_error", "min_angle", "min_views", "max_hypotheses")] == [0, 8, 16, 20]
    assert [getattr(S, k).offset for k in ("retried", "rescued", "observations_rejected", "hypotheses", "robust_ms")] == [0, 8, 16, 24, 32]


def test_header_declares_the_entry_points_and_sizes(tmp_path):
    text = open(os.path.join(ROOT, "include", "msfm_match.h")).read()
    for name in ("msfm_triangulate_tracks_robust", "msfm_fetch_point_inliers"):
        assert re.search(r"\bint %s\(msfm_ctx\* ctx" % name, text), name
        assert name in _lib.EXPORTS, name
    assert "MSFM_TRI_ROBUST = 32" in text
    for struct, size in (("msfm_robust_triangulation_params", 24), ("msfm_robust_stats", 40)):
        assert re.search(r"typedef struct %s \{\s+/\* %d bytes, no implicit padding \*/" % (struct, size), text), struct
    src = tmp_path / "sizes.cpp"
    src.write_text('#include <cstddef>\n#include "msfm_match.h"\n'
                   'static_assert(sizeof(msfm_robust_triangulation_params) == 24 && sizeof(msfm_robust_stats) == 40, "sizes");\n'
                   'static_assert(offsetof(msfm_robust_triangulation_params, max_hypotheses) == 20 && offsetof(msfm_robust_stats, robust_ms) == 32, "offsets");\n'
                   'int main() { return MSFM_TRI_ROBUST == 32 ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sizes")])
    assert subprocess.run([str(tmp_path / "sizes")]).returncode == 0


def test_library_exports(built_lib):
    for name in ("msfm_triangulate_tracks_robust", "msfm_fetch_point_inliers"):
        assert hasattr(built_lib, name), name
    assert built_lib.msfm_triangulate_tracks_robust(None, None, None, None, 0, None, None, None) == 1   # MSFM_E_INVALID: no context
    assert built_lib.msfm_fetch_point_inliers(None, None) == 1


def test_host_twin_exports():
    import robust_triangulation_twin as rtw
    host = rtw.load_host()
    for name in ("host_triangulate_tracks_robust", "host_tri_sample2"):
        assert hasattr(host, name), name
