"""The pose refinement's ABI surface: the structs of include/msfm_match.h have the sizes the binding and the twin assume, no implicit
padding, and the header declares what the library and the host twin export.  CPU only."""
import ctypes as C
import os
import re
import subprocess

from monocularsfm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS_KEYS = ("images", "eligible", "refined", "rejected_by_inliers", "iterations", "observations", "points_reposed", "points_lost",
              "points_gained", "cost_before", "cost_after", "refine_ms", "prepare_ms")
RECORD_KEYS = ("image_id", "status", "n_observations", "iterations", "stop", "inliers_before", "inliers_after", "reserved")


def test_struct_sizes_and_layout():
    P, S, R = _lib.PoseRefineParams, _lib.PoseRefineStats, _lib.POSE_REFINEMENT
    assert C.sizeof(P) == 16 and C.sizeof(S) == 104 and R.itemsize == 48 and _lib.TRI_REPOSED == 128
    assert (_lib.POSE_ATTEMPTED, _lib.POSE_REFINED, _lib.POSE_FIXED) == (1, 2, 4)
    assert [getattr(P, k).offset for k in ("step_tol", "max_iters", "min_observations")] == [0, 8, 12]
    assert [getattr(S, k).offset for k in STATS_KEYS] == list(range(0, 104, 8))
    assert [R.fields[k][1] for k in RECORD_KEYS + ("cost_before", "cost_after")] == list(range(0, 32, 4)) + [32, 40]


def test_header_declares_the_entry_points_and_sizes(tmp_path):
    text = open(os.path.join(ROOT, "include", "msfm_match.h")).read()
    assert re.search(r"\bint msfm_refine_poses\(msfm_ctx\* ctx, const msfm_pose_refine_params\* params, const int32_t\* fixed_image_ids, "
                     r"int n_fixed,\s+msfm_pose_refine_stats\* stats\);", text)
    assert re.search(r"\bint msfm_fetch_poses\(msfm_ctx\* ctx, int32_t\* out_ids, msfm_pose_rt\* out_poses, int\* n\);", text)
    assert re.search(r"\bint msfm_fetch_pose_refinements\(msfm_ctx\* ctx, msfm_pose_refinement\* out\);", text)
    for name in ("msfm_refine_poses", "msfm_fetch_poses", "msfm_fetch_pose_refinements"):
        assert name in _lib.EXPORTS
    assert "MSFM_TRI_REPOSED = 128" in text and "MSFM_POSE_ATTEMPTED = 1, MSFM_POSE_REFINED = 2, MSFM_POSE_FIXED = 4" in text
    for struct, size in (("msfm_pose_refine_params", 16), ("msfm_pose_refine_stats", 104), ("msfm_pose_refinement", 48)):
        assert re.search(r"typedef struct %s \{\s+/\* %d bytes, no implicit padding \*/" % (struct, size), text), struct
    src = tmp_path / "sizes.cpp"
    src.write_text('#include <cstddef>\n#include "msfm_match.h"\n'
                   'static_assert(sizeof(msfm_pose_refine_params) == 16 && sizeof(msfm_pose_refine_stats) == 104 && '
                   'sizeof(msfm_pose_refinement) == 48, "sizes");\n'
                   'static_assert(offsetof(msfm_pose_refine_params, max_iters) == 8 && offsetof(msfm_pose_refine_params, min_observations) == 12 && '
                   'offsetof(msfm_pose_refine_stats, points_gained) == 64 && offsetof(msfm_pose_refine_stats, cost_before) == 72 && '
                   'offsetof(msfm_pose_refine_stats, prepare_ms) == 96 && offsetof(msfm_pose_refinement, inliers_after) == 24 && '
                   'offsetof(msfm_pose_refinement, cost_before) == 32 && offsetof(msfm_pose_refinement, cost_after) == 40, "offsets");\n'
                   'int main() { return MSFM_TRI_REPOSED == 128 && MSFM_POSE_ATTEMPTED == 1 && MSFM_POSE_REFINED == 2 && MSFM_POSE_FIXED == 4 ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sizes")])
    assert subprocess.run([str(tmp_path / "sizes")]).returncode == 0


def test_library_exports(built_lib):
    for name in ("msfm_refine_poses", "msfm_fetch_poses", "msfm_fetch_pose_refinements"):
        assert hasattr(built_lib, name)
    assert built_lib.msfm_refine_poses(None, None, None, 0, None) == 1   # MSFM_E_INVALID: no context
    assert built_lib.msfm_fetch_poses(None, None, None, None) == 1
    assert built_lib.msfm_fetch_pose_refinements(None, None) == 1


def test_host_twin_exports():
    import refine_poses_twin as ptw
    host = ptw.load_host()
    assert hasattr(host, "host_refine_poses")
    assert ptw.TRACE.itemsize == 40
