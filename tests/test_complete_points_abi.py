"""The map completion's ABI surface: the structs of include/msfm_match.h have the sizes the binding and the twin assume, no implicit
padding, and the header declares what the library and the host twin export.  CPU only."""
import ctypes as C
import os
import re
import subprocess

from monocularsfm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS_KEYS = ("eligible", "candidates", "admitted", "rejected_by_depth", "rejected_by_error", "completed", "succeeded",
              "observations_used", "complete_ms", "prepare_ms")


def test_struct_sizes_and_layout():
    P, S = _lib.CompleteParams, _lib.CompleteStats
    assert C.sizeof(P) == 8 and C.sizeof(S) == 80 and _lib.TRI_COMPLETED == 1024
    assert P.max_error.offset == 0 and [k for k, _ in P._fields_] == ["max_error"]
    assert [getattr(S, k).offset for k in STATS_KEYS] == list(range(0, 80, 8))
    assert [k for k, _ in S._fields_] == list(STATS_KEYS)
    pts = _lib.np.zeros(4, _lib.POINT3D)
    pts["status"] = (0, 1 | 512, 15 | 1024, 15 | 512 | 1024)
    assert _lib.completed(pts).tolist() == [False, False, True, True] and _lib.filtered(pts).tolist() == [False, True, False, True]


def test_header_declares_the_entry_point_and_sizes(tmp_path):
    text = open(os.path.join(ROOT, "include", "msfm_match.h")).read()
    assert re.search(r"\bint msfm_complete_points\(msfm_ctx\* ctx, const msfm_complete_params\* params, const int32_t\* image_ids, "
                     r"int n_images,\s+msfm_complete_stats\* stats\);", text)
    assert "msfm_complete_points" in _lib.EXPORTS
    assert "enum { MSFM_TRI_COMPLETED = 1024 };" in text
    assert text.index("int msfm_filter_points(") < text.index("enum { MSFM_TRI_COMPLETED") < text.index("int msfm_register_images(")
    for struct, size in (("msfm_complete_params", 8), ("msfm_complete_stats", 80)):
        assert re.search(r"typedef struct %s \{\s+/\* %d bytes, no implicit padding \*/" % (struct, size), text), struct
    src = tmp_path / "sizes.cpp"
    src.write_text('#include <cstddef>\n#include "msfm_match.h"\n'
                   'static_assert(sizeof(msfm_complete_params) == 8 && sizeof(msfm_complete_stats) == 80, "sizes");\n'
                   'static_assert(offsetof(msfm_complete_params, max_error) == 0 && '
                   + " && ".join("offsetof(msfm_complete_stats, %s) == %d" % (k, 8 * i) for i, k in enumerate(STATS_KEYS)) + ', "offsets");\n'
                   'int main() { return MSFM_TRI_COMPLETED == 1024 ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sizes")])
    assert subprocess.run([str(tmp_path / "sizes")]).returncode == 0


def test_library_exports(built_lib):
    assert hasattr(built_lib, "msfm_complete_points")
    assert built_lib.msfm_complete_points(None, None, None, 0, None) == 1   # MSFM_E_INVALID: no context


def test_host_twin_exports():
    import complete_twin as ctw
    host = ctw.load_host()
    assert hasattr(host, "host_complete_points")
    assert ctw.TRACE.itemsize == 16


def test_the_binding_has_the_calls():
    import inspect
    assert callable(_lib.Context.complete_points) and callable(_lib.Context.reconstruct)
    assert list(inspect.signature(_lib.Context.complete_points).parameters) == ["self", "max_error", "image_ids"]
    assert inspect.signature(_lib.Context.reconstruct).parameters["complete_params"].default is None
