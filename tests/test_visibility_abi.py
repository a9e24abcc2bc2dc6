"""The map visibility's ABI surface: the structs of include/msfm_match.h have the sizes the binding and the twin assume (8 / 24 / 56
bytes), no implicit padding, the enum values, and the header declares what the library and the host twin export.  CPU only."""
import ctypes as C
import inspect
import os
import re
import subprocess

from monocularsfm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD_KEYS = ("image_id", "flags", "n_elements", "n_visible", "n_points", "reserved")
STATS_OFFSETS = (("tracks_counted", 0), ("elements_counted", 8), ("pair_increments", 16), ("device_bytes", 24), ("images", 32), ("posed", 36),
                 ("query", 40), ("route", 44), ("visibility_ms", 48))
ENUMS = (("MSFM_VIS_TRACKS", 0), ("MSFM_VIS_MAP", 1), ("MSFM_VIS_ROUTE_AUTO", 0), ("MSFM_VIS_ROUTE_GLOBAL", 1), ("MSFM_VIS_ROUTE_LDS", 2),
         ("MSFM_VIS_POSED", 1), ("MSFM_VIS_QUERIED", 2))


def test_struct_sizes_and_layout():
    P, S, R = _lib.VisibilityParams, _lib.VisibilityStats, _lib.VISIBILITY
    assert C.sizeof(P) == 8 and R.itemsize == 24 and C.sizeof(S) == 56
    assert [(k, getattr(P, k).offset) for k, _ in P._fields_] == [("basis", 0), ("route", 4)]
    assert R.names == RECORD_KEYS and [R.fields[k][1] for k in RECORD_KEYS] == list(range(0, 24, 4))
    assert [(k, getattr(S, k).offset) for k, _ in S._fields_] == list(STATS_OFFSETS)
    assert (_lib.VIS_TRACKS, _lib.VIS_MAP) == (0, 1) and (_lib.VIS_ROUTE_AUTO, _lib.VIS_ROUTE_GLOBAL, _lib.VIS_ROUTE_LDS) == (0, 1, 2)
    assert (_lib.VIS_POSED, _lib.VIS_QUERIED) == (1, 2)


def test_header_declares_the_entry_point_and_sizes(tmp_path):
    text = open(os.path.join(ROOT, "include", "msfm_match.h")).read()
    assert re.search(r"\bint msfm_map_visibility\(msfm_ctx\* ctx, const msfm_visibility_params\* params, const int32_t\* query_ids, "
                     r"int n_query,\s+msfm_image_visibility\* out_images, uint32_t\* out_covisible, msfm_visibility_stats\* stats\);", text)
    assert "msfm_map_visibility" in _lib.EXPORTS
    assert text.index("int msfm_complete_points(") < text.index("int msfm_map_visibility(") < text.index("int msfm_register_images(")
    for struct, size in (("msfm_visibility_params", 8), ("msfm_image_visibility", 24), ("msfm_visibility_stats", 56)):
        assert re.search(r"typedef struct %s \{\s+/\* %d bytes, no implicit padding \*/" % (struct, size), text), struct
    src = tmp_path / "sizes.cpp"
    src.write_text('#include <cstddef>\n#include "msfm_match.h"\n'
                   'static_assert(sizeof(msfm_visibility_params) == 8 && sizeof(msfm_image_visibility) == 24 && '
                   'sizeof(msfm_visibility_stats) == 56, "sizes");\n'
                   'static_assert(' + " && ".join("offsetof(msfm_visibility_stats, %s) == %d" % kv for kv in STATS_OFFSETS) + ', "stats");\n'
                   'static_assert(' + " && ".join("offsetof(msfm_image_visibility, %s) == %d" % (k, 4 * i) for i, k in enumerate(RECORD_KEYS))
                   + ', "record");\n'
                   'static_assert(' + " && ".join("%s == %d" % kv for kv in ENUMS) + ', "enums");\n'
                   'int main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sizes")])
    assert subprocess.run([str(tmp_path / "sizes")]).returncode == 0


def test_library_exports(built_lib):
    assert hasattr(built_lib, "msfm_map_visibility")
    assert built_lib.msfm_map_visibility(None, None, None, 0, None, None, None) == 1   # MSFM_E_INVALID: no context


def test_host_twin_exports():
    import visibility_twin as vtw
    host = vtw.load_host()
    assert hasattr(host, "host_map_visibility") and hasattr(host, "host_vis_route")


def test_the_binding_has_the_calls():
    sig = inspect.signature
    assert list(sig(_lib.Context.visibility).parameters) == ["self", "query", "basis", "route"]
    assert [sig(_lib.Context.visibility).parameters[k].default for k in ("query", "basis", "route")] == [(), "map", "auto"]
    assert sig(_lib.Context.grow).parameters["max_images"].default is None and sig(_lib.Context.grow).parameters["window"].default is None
    ini = sig(_lib.Context.initialize).parameters
    assert list(ini)[:5] == ["self", "camera", "two_view", "max_trials", "min_points"] and ini["max_trials"].default == 100
    assert ini["min_points"].default == sig(_lib.Context.set_two_view_geometry).parameters["min_num_inliers"].default
    assert sig(_lib.next_images).parameters["min_visible"].default == sig(_lib.Context.register_images).parameters["min_inliers"].default
    assert sig(_lib.local_window).parameters["size"].default == 5
    assert callable(_lib.initial_first_images) and callable(_lib.initial_second_images)
