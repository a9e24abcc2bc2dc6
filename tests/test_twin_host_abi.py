"""The one thing the twins' argument block can get wrong: the ctypes mirror of host_map (tests/twin_host.py) against the C struct
(monocularsfm_amd/host/HostTwinMap.h), field by field, the loader's table against the library's exports, and each raw-argument export against its twin.  CPU only."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import twin_host as th
from monocularsfm_amd import _lib

HEADER = os.path.join(th.HOST, "HostTwinMap.h")


def test_the_mirror_has_the_layout_of_the_struct(tmp_path):
    M = th.HostMap
    names = [k for k, _ in M._fields_]
    ends = [getattr(M, k).offset + getattr(M, k).size for k in names]
    assert C.sizeof(M) == 208 and getattr(M, names[0]).offset == 0
    assert ends[:-1] == [getattr(M, k).offset for k in names[1:]] and ends[-1] == C.sizeof(M), "implicit padding"
    text = open(HEADER).read()
    assert re.search(r"typedef struct host_map \{\s+/\* %d bytes, no implicit padding" % C.sizeof(M), text)
    body = text[text.index("typedef struct host_map {"):text.index("} host_map;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)(?:\[\d+\])?;", body) == names, "the fields and their order"
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include "HostTwinMap.h"\n'
                   'static_assert(sizeof(host_map) == %d, "size");\n' % C.sizeof(M)
                   + "".join('static_assert(offsetof(host_map, %s) == %d && sizeof(host_map::%s) == %d, "%s");\n'
                             % (k, getattr(M, k).offset, k, getattr(M, k).size, k) for k in names)
                   + "int main() { return 0; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(th.ROOT, "include"), "-I", th.HOST, str(src), "-o", str(tmp_path / "layout")])
    assert subprocess.run([str(tmp_path / "layout")]).returncode == 0


def test_every_declared_export_is_in_the_library():
    host = th.load()
    assert host is th.load(), "one handle per process"
    missing = [name for name in th.EXPORTS if not hasattr(host, name)]
    assert not missing, missing
    takes_map = sorted(name for name, (_, a) in th.EXPORTS.items() if a[0] is C.POINTER(th.HostMap))
    assert takes_map == sorted(["twin_triangulate_tracks", "twin_triangulate_tracks_robust", "twin_refine_points", "twin_refine_poses",
                                "twin_refine_camera", "twin_extend_points", "twin_filter_points", "twin_complete_points",
                                "twin_map_visibility"])


def test_the_slices_are_todays():
    """four slices per worker, rounded up and never empty; one job per selected track; the results keyed by `first`"""
    seen = th.run_sliced(1000, lambda f, c: (f, c), workers=16)
    assert list(seen) == list(range(0, 1000, 16)) and seen[992] == (992, 8) and all(v == (f, 16) for f, v in seen.items() if f < 992)
    assert th.run_sliced(0, lambda f, c: (f, c)) == {} and th.run_sliced(3, lambda f, c: (f, c)) == {0: (0, 1), 1: (1, 1), 2: (2, 1)}
    assert th.run_sliced(1000, lambda f, c: c, select=[7, 3]) == {7: 1, 3: 1}
    assert th.run_sliced(100, lambda f, c: (f, c), workers=1) == {f: (f, 25) for f in (0, 25, 50, 75)}


# ---- the host_* exports with raw argument lists against their twins -----------------------------------------------------------------------
# A list names the block's fields in the export's order; anything that is not a field name is the call's own argument.
_LEAD = ("offsets", "image_ids", "point_idx", "consistent", "ids", "n_images", "kxy", "pose_ids", "poses", "n_poses")
_ALL = ("offsets", "image_ids", "point_idx", "n_tracks") + _LEAD[4:]
_TRI = ("cam", "max_error", "min_angle", "min_views")
_STATE = ("first", "count", "points", "residuals", "mask")


def _raw(block, items):
    kinds = dict(th.HostMap._fields_)
    cam = C.c_void_p(C.addressof(block) + th.HostMap.cam.offset)
    return [it if not isinstance(it, str) else cam if it == "cam" else kinds[it](getattr(block, it)) for it in items]


def _cases():
    """name of the export, of its twin, and own(): fresh outputs -> (the twin's own arguments, the export's list, the outputs)"""
    i, d, T, P = C.c_int, C.c_double, 72, 8
    p = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    z = lambda n, t=np.int64: np.zeros(n, t)   # noqa: E731
    ids3 = np.asarray([1, 4, 7, 1], np.int32)   # the scene's first three ids and a sentinel

    def robust(trace):
        def own():
            c, tr = z(4), z(12 * T, np.int32)
            return (i(8), p(c), p(tr) if trace else None), _LEAD + _TRI + (i(8),) + _STATE + (p(c),) + ((p(tr),) if trace else ()), (c, tr)
        return own

    def points():
        c, c2, tr = z(5), z(2, np.float64), z(40 * T, np.uint8)
        return (d(1e-10), i(10), p(c), p(c2), p(tr)), _LEAD[:3] + _LEAD[4:] + _TRI[:3] + (d(1e-10), i(10)) + _STATE + (p(c), p(c2), p(tr)), (c, c2, tr)

    def poses():
        rec, c, c2, tr = z(P, _lib.POSE_REFINEMENT), z(9), z(2, np.float64), z(40 * P, np.uint8)
        mine = (d(1e-6), i(10), i(15), p(ids3), i(1))
        return mine + (p(rec), p(c), p(c2), p(tr)), _ALL + _TRI[:3] + mine + _STATE[2:] + (p(rec), p(c), p(c2), p(tr)), (rec, c, c2, tr)

    def camera():
        c, c2, tr = z(12), z(2, np.float64), z(40, np.uint8)
        mine = (d(1e-6), i(1 | 4), i(10), i(100))
        return mine + (p(c), p(c2), p(tr)), _ALL + _TRI[:3] + mine + _STATE[2:] + (p(c), p(c2), p(tr)), (c, c2, tr)

    def edit(n_counts, before_cam, after_angle, own_twin):
        def own():
            c, tr = z(n_counts), z(4 * T, np.int32)
            return (own_twin + (p(c), p(tr)), _LEAD + before_cam + _TRI[:3] + after_angle + _STATE + ("have_mask", p(c), p(tr)), (c, tr))
        return own

    def visibility():
        rec, mat, c = z(P, _lib.VISIBILITY), z(3 * P, np.uint32), z(3)
        mine = (p(ids3), i(3), i(_lib.VIS_MAP))
        lead = ("offsets", "image_ids", "consistent", "n_tracks", "ids", "n_images", "pose_ids", "poses", "n_poses")
        return mine + (p(rec), p(mat), p(c)), lead + mine + ("points", "mask", p(rec), p(mat), p(c)), (rec, mat, c)

    scope = (p(ids3), i(3))
    return [("host_triangulate_tracks", "twin_triangulate_tracks", lambda: ((), _LEAD + _TRI + _STATE[:4], ())),
            ("host_triangulate_tracks_robust", "twin_triangulate_tracks_robust", robust(False)),
            ("host_triangulate_tracks_robust_trace", "twin_triangulate_tracks_robust", robust(True)),
            ("host_refine_points", "twin_refine_points", points), ("host_refine_poses", "twin_refine_poses", poses),
            ("host_refine_camera", "twin_refine_camera", camera),
            ("host_extend_points", "twin_extend_points", edit(7, (p(ids3), i(1)), ("min_views", i(8)), (p(ids3), i(1), i(8)))),
            ("host_filter_points", "twin_filter_points", edit(7, scope, (d(0.45), d(1.5)), scope + (d(0.45), d(1.5)))),
            ("host_complete_points", "twin_complete_points", edit(6, scope, (d(1.0),), scope + (d(1.0),))),
            ("host_map_visibility", "twin_map_visibility", visibility)]


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c[0])
def test_a_raw_argument_export_computes_what_its_twin_computes(case):
    """Both forms on one scene (72 tracks, 8 images, 0.3 px of noise) from the same state, the robust triangulation's: every array the
    call may write -- records, residuals, inlier bytes, pose list, camera, counters, records and traces of its own -- byte for byte."""
    import nonfinite_fixtures as nf
    import robust_triangulation_twin as robtw
    name, twin, own = case
    host = th.load()
    sc = nf.images()[0]
    assert len(sc.tracks[0]) - 1 == 72 and len(sc.ids) == 8 and [int(v) for v in sc.ids[:3]] == [1, 4, 7]
    args = (sc.tracks, sc.ids, sc.kps, sc.poses, nf.CAM_D)
    pts, res, mask, _ = robtw.run(host, *args, nf.THR + (8,))
    assert ((pts["status"] & 14) == 14).sum() > 36
    start = [np.zeros_like(a) for a in (pts, res, mask)] if "triangulate" in name else [pts, res, mask]   # (those three write all of it)
    got = []
    for raw in (False, True):
        block, held = th.pack(*args, nf.THR, *start, exact=True)
        mine, items, outputs = own()
        f = getattr(host, name if raw else twin)
        rc = f(*_raw(block, items)) if raw else f(block, *mine)
        assert rc == 0, (name, raw, rc)
        state = (held.points, held.residuals, held.mask, held.poses, np.asarray(list(block.cam))) + tuple(outputs)
        got.append([a.tobytes() for a in state])
    assert got[0] == got[1], [k for k, (a, b) in enumerate(zip(*got)) if a != b]
    assert got[0][:3] != [a.tobytes() for a in start] or any(a.view(np.uint8).any() for a in outputs), "nothing was computed"
