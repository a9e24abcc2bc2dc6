"""The map filtering's ABI surface: the structs of include/msfm_match.h have the sizes the binding and the twin assume, no implicit
padding, and the header declares what the library and the host twin export.  CPU only."""
import ctypes as C
import os
import re
import subprocess

from monocularsfm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS_KEYS = ("eligible", "dropped_by_depth", "dropped_by_error", "trimmed", "regained", "removed_by_views", "removed_by_angle",
              "succeeded", "observations_used", "filter_ms", "prepare_ms")


def test_struct_sizes_and_layout():
    P, S = _lib.FilterParams, _lib.FilterStats
    assert C.sizeof(P) == 16 and C.sizeof(S) == 88 and _lib.TRI_FILTERED == 512
    assert [getattr(P, k).offset for k in ("max_error", "min_angle")] == [0, 8]
    assert [getattr(S, k).offset for k in STATS_KEYS] == list(range(0, 88, 8))
    assert [k for k, _ in S._fields_] == list(STATS_KEYS)
    pts = _lib.np.zeros(3, _lib.POINT3D)
    pts["status"] = (0, 1 | 512, 14 | 512)
    assert _lib.filtered(pts).tolist() == [False, True, True]


def test_header_declares_the_entry_point_and_sizes(tmp_path):
    text = open(os.path.join(ROOT, "include", "msfm_match.h")).read()
    assert re.search(r"\bint msfm_filter_points\(msfm_ctx\* ctx, const msfm_filter_params\* params, const int32_t\* image_ids, int n_images,\s+"
                     r"msfm_filter_stats\* stats\);", text)
    assert "msfm_filter_points" in _lib.EXPORTS
    assert "enum { MSFM_TRI_FILTERED = 512 };" in text
    for struct, size in (("msfm_filter_params", 16), ("msfm_filter_stats", 88)):
        assert re.search(r"typedef struct %s \{\s+/\* %d bytes, no implicit padding \*/" % (struct, size), text), struct
    src = tmp_path / "sizes.cpp"
    src.write_text('#include <cstddef>\n#include "msfm_match.h"\n'
                   'static_assert(sizeof(msfm_filter_params) == 16 && sizeof(msfm_filter_stats) == 88, "sizes");\n'
                   'static_assert(offsetof(msfm_filter_params, max_error) == 0 && offsetof(msfm_filter_params, min_angle) == 8 && '
                   + " && ".join("offsetof(msfm_filter_stats, %s) == %d" % (k, 8 * i) for i, k in enumerate(STATS_KEYS)) + ', "offsets");\n'
                   'int main() { return MSFM_TRI_FILTERED == 512 ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sizes")])
    assert subprocess.run([str(tmp_path / "sizes")]).returncode == 0


def test_library_exports(built_lib):
    assert hasattr(built_lib, "msfm_filter_points")
    assert built_lib.msfm_filter_points(None, None, None, 0, None) == 1   # MSFM_E_INVALID: no context


def test_host_twin_exports():
    import filter_twin as ftw
    host = ftw.load_host()
    assert hasattr(host, "host_filter_points")
    assert ftw.TRACE.itemsize == 16


def test_the_binding_has_the_calls():
    assert callable(_lib.Context.filter_points) and callable(_lib.Context.reconstruct)
