"""The map extension's ABI surface: the structs of include/msfm_match.h have the sizes the binding and the twin assume, no implicit
padding, and the header declares what the library and the host twin export.  CPU only."""
import ctypes as C
import os
import re
import subprocess

from monocularsfm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS_KEYS = ("images_added", "tracks_touched", "continued", "observations_added", "observations_rejected", "created_attempted",
              "created", "retried", "succeeded", "observations_used", "extend_ms", "prepare_ms")


def test_struct_sizes_and_layout():
    P, S = _lib.ExtendParams, _lib.ExtendStats
    assert C.sizeof(P) == 8 and C.sizeof(S) == 96 and _lib.TRI_EXTENDED == 256
    assert [getattr(P, k).offset for k in ("max_hypotheses", "reserved")] == [0, 4]
    assert [getattr(S, k).offset for k in STATS_KEYS] == list(range(0, 96, 8))
    assert [k for k, _ in S._fields_] == list(STATS_KEYS)
    pts = _lib.np.zeros(3, _lib.POINT3D)
    pts["status"] = (0, 256, 14 | 256)
    assert _lib.extended(pts).tolist() == [False, True, True]


def test_header_declares_the_entry_point_and_sizes(tmp_path):
    text = open(os.path.join(ROOT, "include", "msfm_match.h")).read()
    assert re.search(r"\bint msfm_extend_points\(msfm_ctx\* ctx, const int32_t\* image_ids, const msfm_pose_rt\* poses, int n_poses,\s+"
                     r"const msfm_extend_params\* params, msfm_extend_stats\* stats\);", text)
    assert "msfm_extend_points" in _lib.EXPORTS
    assert "enum { MSFM_TRI_EXTENDED = 256 };" in text
    for struct, size in (("msfm_extend_params", 8), ("msfm_extend_stats", 96)):
        assert re.search(r"typedef struct %s \{\s+/\* %d bytes, no implicit padding \*/" % (struct, size), text), struct
    src = tmp_path / "sizes.cpp"
    src.write_text('#include <cstddef>\n#include "msfm_match.h"\n'
                   'static_assert(sizeof(msfm_extend_params) == 8 && sizeof(msfm_extend_stats) == 96, "sizes");\n'
                   'static_assert(offsetof(msfm_extend_params, max_hypotheses) == 0 && offsetof(msfm_extend_params, reserved) == 4 && '
                   + " && ".join("offsetof(msfm_extend_stats, %s) == %d" % (k, 8 * i) for i, k in enumerate(STATS_KEYS)) + ', "offsets");\n'
                   'int main() { return MSFM_TRI_EXTENDED == 256 ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sizes")])
    assert subprocess.run([str(tmp_path / "sizes")]).returncode == 0


def test_library_exports(built_lib):
    assert hasattr(built_lib, "msfm_extend_points")
    assert built_lib.msfm_extend_points(None, None, None, 0, None, None) == 1   # MSFM_E_INVALID: no context


def test_host_twin_exports():
    import extend_twin as etw
    host = etw.load_host()
    assert hasattr(host, "host_extend_points")
    assert etw.TRACE.itemsize == 16
