"""The camera refinement's ABI surface: the structs of include/msfm_match.h have the sizes the binding and the twin assume (24 / 248
bytes), no implicit padding, the enum values, the declarations sit directly behind msfm_fetch_pose_refinements, and the header
declares what the library and the host twin export.  The binding's defaults: alternate, grow and reconstruct with camera_params=None
make exactly the calls they made before the camera refinement existed (a stub context that records calls).  CPU only."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

from monocularsfm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS_OFFSETS = (("step_tol", 0), ("mask", 8), ("max_iters", 12), ("min_observations", 16), ("reserved", 20))
STATS_OFFSETS = tuple((k, 8 * i) for i, k in enumerate(
    ("observations", "behind", "iterations", "accepted_steps", "stop", "refined", "rejected_by_inliers", "inliers_before", "inliers_after",
     "points_recalibrated", "points_lost", "points_gained", "cost_before", "cost_after"))) + \
    (("camera_before", 112), ("camera_after", 176), ("refine_ms", 240))
ENUMS = (("MSFM_TRI_RECALIBRATED", 2048), ("MSFM_CAM_FX_FY", 1), ("MSFM_CAM_F", 2), ("MSFM_CAM_CX_CY", 4), ("MSFM_CAM_K1_K2", 8))


def test_struct_sizes_and_layout():
    P, S = _lib.CameraRefineParams, _lib.CameraRefineStats
    assert C.sizeof(P) == 24 and C.sizeof(S) == 248 and C.sizeof(_lib.Camera) == 64
    assert [(k, getattr(P, k).offset) for k, _ in P._fields_] == list(PARAMS_OFFSETS)
    assert [(k, getattr(S, k).offset) for k, _ in S._fields_] == list(STATS_OFFSETS)
    assert _lib.TRI_RECALIBRATED == 2048 and (_lib.CAM_FX_FY, _lib.CAM_F, _lib.CAM_CX_CY, _lib.CAM_K1_K2) == (1, 2, 4, 8)
    assert _lib.camera_mask(("fx_fy", "cx_cy", "k1_k2")) == 13 and _lib.camera_mask("f") == 2 and _lib.camera_mask(10) == 10
    pts = np.zeros(3, _lib.POINT3D)
    pts["status"] = (15, 15 | 2048, 2048)
    assert list(_lib.recalibrated(pts)) == [False, True, True]


def test_header_declares_the_entry_points_and_sizes(tmp_path):
    text = open(os.path.join(ROOT, "include", "msfm_match.h")).read()
    assert re.search(r"\bint msfm_refine_camera\(msfm_ctx\* ctx, const msfm_camera_refine_params\* params, "
                     r"msfm_camera_refine_stats\* stats\);", text)
    assert re.search(r"\bint msfm_fetch_camera\(msfm_ctx\* ctx, msfm_camera\* out\);", text)
    assert "msfm_refine_camera" in _lib.EXPORTS and "msfm_fetch_camera" in _lib.EXPORTS
    assert (text.index("int msfm_fetch_pose_refinements(") < text.index("int msfm_refine_camera(") < text.index("int msfm_fetch_camera(")
            < text.index("int msfm_extend_points("))
    at = _lib.EXPORTS.index("msfm_fetch_pose_refinements")
    assert _lib.EXPORTS[at + 1:at + 4] == ["msfm_refine_camera", "msfm_fetch_camera", "msfm_extend_points"]
    for struct, size in (("msfm_camera_refine_params", 24), ("msfm_camera_refine_stats", 248)):
        assert re.search(r"typedef struct %s \{\s+/\* %d bytes, no implicit padding \*/" % (struct, size), text), struct
    src = tmp_path / "sizes.cpp"
    src.write_text('#include <cstddef>\n#include "msfm_match.h"\n'
                   'static_assert(sizeof(msfm_camera_refine_params) == 24 && sizeof(msfm_camera_refine_stats) == 248 && '
                   'sizeof(msfm_camera) == 64, "sizes");\n'
                   'static_assert(' + " && ".join("offsetof(msfm_camera_refine_params, %s) == %d" % kv for kv in PARAMS_OFFSETS) + ', "params");\n'
                   'static_assert(' + " && ".join("offsetof(msfm_camera_refine_stats, %s) == %d" % kv for kv in STATS_OFFSETS) + ', "stats");\n'
                   'static_assert(' + " && ".join("%s == %d" % kv for kv in ENUMS) + ', "enums");\n'
                   'int main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sizes")])
    assert subprocess.run([str(tmp_path / "sizes")]).returncode == 0


def test_library_exports(built_lib):
    assert hasattr(built_lib, "msfm_refine_camera") and hasattr(built_lib, "msfm_fetch_camera")
    assert built_lib.msfm_refine_camera(None, None, None) == 1   # MSFM_E_INVALID: no context
    assert built_lib.msfm_fetch_camera(None, None) == 1


def test_host_twin_exports():
    import refine_camera_twin as ctw
    host = ctw.load_host()
    assert hasattr(host, "host_refine_camera") and hasattr(host, "host_rc_reduce")
    assert (ctw.FX_FY, ctw.F, ctw.CX_CY, ctw.K1_K2) == (_lib.CAM_FX_FY, _lib.CAM_F, _lib.CAM_CX_CY, _lib.CAM_K1_K2)


def test_the_binding_has_the_calls():
    sig = inspect.signature
    p = sig(_lib.Context.refine_camera).parameters
    assert list(p) == ["self", "mask", "max_iters", "step_tol", "min_observations"]
    assert [p[k].default for k in list(p)[1:]] == [("fx_fy",), 10, 1e-6, 100]
    assert list(sig(_lib.Context.camera).parameters) == ["self"]
    for fn in (_lib.Context.alternate, _lib.Context.grow):
        assert sig(fn).parameters["camera_params"].default is None and list(sig(fn).parameters)[-1] == "camera_params"


class Recorder(_lib.Context):
    """a Context without a library behind it: every call the drivers make is recorded and answered with what they read"""

    def __init__(self, registers=1):   # noqa: D107 (no device, no handle)
        self.calls, self.left = [], registers
        self._track_ids = [1, 4, 7]

    def _note(self, name, *args, **kw):
        self.calls.append((name, args, tuple(sorted(kw.items()))))

    def refine_points(self, **kw):
        self._note("refine_points", **kw)
        return {"refined": 0}

    def refine_poses(self, fixed=(), **kw):
        self._note("refine_poses", fixed=tuple(fixed), **kw)
        return {"refined": 0}

    def refine_camera(self, **kw):
        self._note("refine_camera", **kw)
        return {"refined": 1 if len(self.calls) < 6 else 0}

    def camera(self):
        self._note("camera")
        return {"fx": 1.0, "fy": 2.0, "cx": 3.0, "cy": 4.0, "k1": 0.0, "k2": 0.0, "p1": 0.0, "p2": 0.0}

    def poses(self):
        self._note("poses")
        return {1: (np.eye(3), np.zeros(3))}

    def register_images(self, camera, image_ids, **kw):
        self._note("register_images", camera if not isinstance(camera, dict) else tuple(sorted(camera.items())), tuple(image_ids), **kw)
        return {"succeeded": 1}

    def registrations(self):
        self._note("registrations")
        rec = np.zeros(1, _lib.REGISTRATION)
        if self.left > 0:
            rec["image_id"], rec["status"] = 4, _lib.REG_ATTEMPTED | _lib.REG_POSE | _lib.REG_SUCCEEDED
            rec["R"] = np.eye(3).reshape(9)
        self.left -= 1
        return (rec,)

    def extend_points(self, poses, max_hypotheses=None):
        self._note("extend_points", tuple(sorted(poses)))
        return {"continued": 0}

    def filter_points(self, **kw):
        self._note("filter_points", **kw)
        return {"trimmed": 0}


BEFORE_ALTERNATE = [("refine_points", (), ()), ("refine_poses", (), (("fixed", (7,)),))]
CAMERA = (9.0, 9.0, 1.0, 1.0)


def test_defaults_make_the_calls_they_made_before():
    r = Recorder()
    out = r.alternate(3, fixed=[7])
    assert out == [({"refined": 0}, {"refined": 0})] and r.calls == BEFORE_ALTERNATE          # 2-tuples, the early stop on two zeros
    r = Recorder()
    reg, ext, alt, new = r.grow(CAMERA, rounds=1, fixed=[7])
    before_grow = [("poses", (), ()), ("register_images", (CAMERA, (4, 7)), ()), ("registrations", (), ()), ("extend_points", ((4,),), ())]
    assert r.calls == before_grow + BEFORE_ALTERNATE and alt == [({"refined": 0}, {"refined": 0})] and new == [4]
    r = Recorder()
    out = r.reconstruct(CAMERA, fixed=[7])
    second = [("poses", (), ()), ("register_images", (CAMERA, (4, 7)), ()), ("registrations", (), ())]
    assert r.calls == before_grow + BEFORE_ALTERNATE + [("filter_points", (), ())] + second and len(out) == 1
    assert not any(c[0] in ("refine_camera", "camera") for c in r.calls)


def test_camera_params_add_the_camera_call_and_the_sessions_camera():
    r = Recorder()
    out = r.alternate(5, fixed=[7], camera_params={"mask": ("f",)})
    assert [len(o) for o in out] == [3, 3] and out[0][2] == {"refined": 1} and out[1][2] == {"refined": 0}   # stops when all three are 0
    assert r.calls == (BEFORE_ALTERNATE + [("refine_camera", (), (("mask", ("f",)),))]) * 2
    r = Recorder()
    reg, ext, alt, new = r.grow(CAMERA, fixed=[7], camera_params={})
    session = tuple(sorted(r.camera().items()))
    assert ("register_images", (session, (4, 7)), ()) in r.calls and not any(c[0] == "register_images" and c[1][0] == CAMERA for c in r.calls)
    assert [c[0] for c in r.calls[-4:-1]] == ["refine_points", "refine_poses", "refine_camera"] and len(alt[0]) == 3
    r = Recorder()
    out = r.reconstruct(CAMERA, fixed=[7], camera_params={})
    assert len(out) == 1 and len(out[0]["alternate"][0]) == 3 and sum(c[0] == "refine_camera" for c in r.calls) >= 1
