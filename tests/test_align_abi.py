"""The map alignment's ABI surface: the structs of include/msfm_match.h have the sizes the binding and the twins assume (104 / 24 / 144 /
16 / 48 bytes), no implicit padding, the enum values, the declarations sit behind msfm_map_visibility and before msfm_register_images,
the header declares what the library and the host twins export, and the binding has the three calls with their defaults while
alternate, grow and reconstruct keep their signatures.  CPU only."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

from monocularsfm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM = (("s", 0), ("Q", 8), ("d", 80))
PARAMS = (("max_error", 0), ("confidence", 8), ("max_hypotheses", 16), ("min_inliers", 20))
RECORD = (("status", 0), ("n_listed", 4), ("n_used", 8), ("n_inliers", 12), ("hypotheses", 16), ("refits", 20), ("similarity", 24),
          ("rms", 128), ("estimate_ms", 136))
RESIDUAL = (("flags", 0), ("reserved", 4), ("error", 8))
STATS = tuple((k, 8 * i) for i, k in enumerate(("poses_transformed", "points_transformed", "points_lost", "points_gained", "succeeded",
                                                "transform_ms")))
STRUCTS = (("msfm_similarity", 104, SIM), ("msfm_alignment_params", 24, PARAMS), ("msfm_alignment", 144, RECORD),
           ("msfm_alignment_residual", 16, RESIDUAL), ("msfm_transform_stats", 48, STATS))
ENUMS = (("MSFM_TRI_ALIGNED", 4096), ("MSFM_ALN_ATTEMPTED", 1), ("MSFM_ALN_MODEL", 2), ("MSFM_ALN_SUCCEEDED", 4), ("MSFM_ALN_REFIT", 8),
         ("MSFM_ALN_LEAST_SQUARES", 16), ("MSFM_ALN_USED", 1), ("MSFM_ALN_INLIER", 2))


def test_struct_sizes_and_layout():
    for cls, (_, size, offsets) in zip((_lib.Similarity, _lib.AlignmentParams, _lib.Alignment, None, _lib.TransformStats), STRUCTS):
        if cls is None:
            continue
        assert C.sizeof(cls) == size, cls
        assert [(k, getattr(cls, k).offset) for k, _ in cls._fields_] == list(offsets), cls
    d = _lib.ALIGNMENT_RESIDUAL
    assert d.itemsize == 16 and [(k, d.fields[k][1]) for k in d.names] == list(RESIDUAL)
    assert _lib.TRI_ALIGNED == 4096 and _lib.TRI_ALIGNED not in (_lib.TRI_RECALIBRATED, _lib.TRI_COMPLETED)
    assert (_lib.ALN_ATTEMPTED, _lib.ALN_MODEL, _lib.ALN_SUCCEEDED, _lib.ALN_REFIT, _lib.ALN_LEAST_SQUARES) == (1, 2, 4, 8, 16)
    assert (_lib.ALN_USED, _lib.ALN_INLIER) == (1, 2)
    pts = np.zeros(3, _lib.POINT3D)
    pts["status"] = (15, 15 | 4096, 4096 | 1)
    assert list(_lib.aligned(pts)) == [False, True, True]
    ids, pos = _lib.prior_table({7: (1, 2, 3), 1: (4.5, 5, 6)})
    assert ids.dtype == np.int32 and list(ids) == [1, 7] and pos.dtype == np.float64 and pos.tolist() == [[4.5, 5, 6], [1, 2, 3]]
    g = _lib.similarity_struct(2.0, np.arange(9.0).reshape(3, 3), (7, 8, 9))
    assert g.s == 2.0 and list(g.Q) == list(range(9)) and list(g.d) == [7, 8, 9]


def test_header_declares_the_entry_points_and_sizes(tmp_path):
    text = open(os.path.join(ROOT, "include", "msfm_match.h")).read()
    assert re.search(r"\bint msfm_estimate_alignment\(msfm_ctx\* ctx, const int32_t\* image_ids, const double\* positions, int n, "
                     r"const msfm_alignment_params\* params,\s+msfm_alignment\* out, msfm_alignment_residual\* out_per_prior\);", text)
    assert re.search(r"\bint msfm_transform_map\(msfm_ctx\* ctx, const msfm_similarity\* similarity, msfm_transform_stats\* stats\);", text)
    assert (text.index("int msfm_map_visibility(") < text.index("int msfm_estimate_alignment(") < text.index("int msfm_transform_map(")
            < text.index("int msfm_register_images("))
    at = _lib.EXPORTS.index("msfm_map_visibility")
    assert _lib.EXPORTS[at + 1:at + 4] == ["msfm_estimate_alignment", "msfm_transform_map", "msfm_register_images"]
    for struct, size, _ in STRUCTS:
        assert re.search(r"typedef struct %s \{\s+/\* %d bytes, no implicit padding \*/" % (struct, size), text), struct
    src = tmp_path / "sizes.cpp"
    src.write_text('#include <cstddef>\n#include "msfm_match.h"\n'
                   + "".join('static_assert(sizeof(%s) == %d && %s, "%s");\n'
                             % (s, size, " && ".join("offsetof(%s, %s) == %d" % (s, k, o) for k, o in offs), s) for s, size, offs in STRUCTS)
                   + 'static_assert(' + " && ".join("%s == %d" % kv for kv in ENUMS) + ', "enums");\n'
                   'int main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sizes")])
    assert subprocess.run([str(tmp_path / "sizes")]).returncode == 0


def test_library_exports(built_lib):
    assert hasattr(built_lib, "msfm_estimate_alignment") and hasattr(built_lib, "msfm_transform_map")
    assert built_lib.msfm_estimate_alignment(None, None, None, 0, None, None, None) == 1   # MSFM_E_INVALID: no context
    assert built_lib.msfm_transform_map(None, None, None) == 1


def test_host_twin_exports():
    import align_twin as atw
    host = atw.load_host()
    assert all(hasattr(host, name) for name in atw.EXPORTS)
    assert (atw.K_REFITS, atw.K_MIN_SPREAD, atw.K_ROUND) == (4, 1e-6, 256)
    text = open(os.path.join(ROOT, "monocularsfm_amd", "csrc", "msfm_align.h")).read()
    assert "kRefits = 4;" in text and "kMinSpread = 1e-6;" in text and "kAlnRound = 256;" in text and "kAlnTile = 256;" in text


def test_the_binding_has_the_calls():
    sig = inspect.signature
    p = sig(_lib.Context.estimate_alignment).parameters
    assert list(p) == ["self", "positions", "max_error", "confidence", "max_hypotheses", "min_inliers"]
    assert [p[k].default for k in list(p)[2:]] == [None, 0.9999, 1024, 3]
    assert list(sig(_lib.Context.transform_map).parameters) == ["self", "s", "Q", "d"]
    p = sig(_lib.Context.align).parameters
    assert list(p) == ["self", "positions", "estimate_kwargs"] and p["estimate_kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    # the drivers are untouched: no alignment argument, the last ones those of the camera refinement
    for fn in (_lib.Context.alternate, _lib.Context.grow):
        assert list(sig(fn).parameters)[-1] == "camera_params"
    assert list(sig(_lib.Context.reconstruct).parameters) == ["self", "camera", "rounds", "filter_params", "max_increments",
                                                              "complete_params", "grow_kwargs"]


class Recorder(_lib.Context):
    """a Context without a library behind it: estimate_alignment answers what it is told to"""

    def __init__(self, status):   # noqa: D107 (no device, no handle)
        self.calls, self.status = [], status

    def estimate_alignment(self, positions, **kw):
        self.calls.append(("estimate_alignment", tuple(sorted(positions)), tuple(sorted(kw.items()))))
        return dict(status=self.status, s=2.0, Q=np.eye(3), d=np.ones(3)), np.zeros(2, _lib.ALIGNMENT_RESIDUAL)

    def transform_map(self, s, Q, d):
        self.calls.append(("transform_map", float(s), np.asarray(Q).tolist(), np.asarray(d).tolist()))
        return {"points_lost": 0}


def test_align_transforms_iff_the_estimate_succeeded():
    r = Recorder(_lib.ALN_ATTEMPTED | _lib.ALN_MODEL | _lib.ALN_SUCCEEDED)
    a, rec, st = r.align({4: (0, 0, 0), 1: (1, 1, 1)}, max_error=0.5)
    assert st == {"points_lost": 0} and a["s"] == 2.0 and len(rec) == 2
    assert r.calls == [("estimate_alignment", (1, 4), (("max_error", 0.5),)), ("transform_map", 2.0, np.eye(3).tolist(), [1.0, 1.0, 1.0])]
    r = Recorder(_lib.ALN_ATTEMPTED | _lib.ALN_MODEL)
    a, rec, st = r.align({4: (0, 0, 0)})
    assert st is None and [c[0] for c in r.calls] == ["estimate_alignment"]
