"""A whole reconstruction on the device, descriptors to map: upload, set_verification_model(VERIFY_ESSENTIAL), set_two_view_geometry,
tracks_begin, match_pairs_verified (or the verified stream under forced cuts), tracks_finish, initialize, reconstruct -- the chain of
tests/test_reconstruction_reference.py with the same fixtures (tests/reconstruction_fixtures.py, 24 x 600) and the same parameters, on a
real Context(0).  Two comparisons per variant, independent of each other:

  * against the stand-in (tests/twin_context.TwinContext, which runs the SAME chain on the host twins from its OWN state, not from the
    device's): the verified lists, the two-view records and the tracks; the pair initialize chose and its trial count; then, stepping
    reconstruct(max_increments=1) on both sides, after EVERY increment the registered ids, every integer of the stats dicts and the
    bytes of points3d(), point_inliers(), pose_list() and camera().  The stage tests establish equality for one call from equal
    state; this is equality over the whole run -- drift, a stale flag or a camera that does not reach the next call would show.  The
    one exception: refine_points' cost_before / cost_after, which the device adds per wave and the twin in track order
    (tests/test_gpu_refine_points.py): 1e-9 relative.  Every other double of the stats is bit-equal.
  * against the ground truth: all 24 images posed, and the accuracy figures after the similarity alignment within 2 x the figures
    that were measured on the CPU chain (reconstruction_fixtures.MEASURED) -- a bound that does not come from the device's output and
    that a wrong map fails whatever happens to the byte comparison.

Every visibility() call that initialize and grow make is watched: points3d() and pose_list() are byte-identical before and after."""
import functools
import itertools

import numpy as np
import pytest

import reconstruction_fixtures as rfx
import tracks_ref
from monocularsfm_amd import _lib
from test_gpu_refine_camera import bad
from twin_context import TwinContext

pytestmark = pytest.mark.gpu
CAMERA_PARAMS = dict(mask=("fx_fy",))
LOOSE = {("points", "cost_before"), ("points", "cost_after")}      # refine_points' two sums: information only, 1e-9 relative
DEVICE_FIGURES = {}


@pytest.fixture()
def tctx(built_lib):
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


def start_camera(cap, off):
    return bad(cap["cam"]) if off else cap["cam"]


@functools.lru_cache(maxsize=None)
def twin_run(name, off=False):
    """the stand-in's run of one variant, computed once: what every stage must give"""
    cap = rfx.variant(name)
    cam = start_camera(cap, off)
    ctx = TwinContext()
    lists, records, stats = rfx.open_session(ctx, cap, cam)
    pair, trials, init = ctx.initialize(cam, rfx.two_view_dict(cap, records), min_points=rfx.MIN_POINTS)
    w = dict(lists=lists, records=records, track_stats=stats, tracks=ctx.tracks(), pair=pair, trials=trials, init=init,
             init_state=rfx.snapshot(ctx))
    w["steps"] = [(inc, rfx.snapshot(ctx)) for inc in rfx.increments(ctx, cam, CAMERA_PARAMS if off else None)]
    w["posed"] = sorted(ctx.poses())
    return w


def same_stats(got, want, stage):
    """every key the stand-in computes: integers equal, doubles bit-equal (LOOSE: 1e-9 relative), nested camera dicts equal"""
    for k, w in want.items():
        g = got[k]
        if isinstance(w, dict):
            same_stats(g, w, stage)
        elif isinstance(w, float):
            if (stage, k) in LOOSE:
                assert abs(g - w) <= 1e-9 * max(abs(w), 1e-300), (stage, k, g, w)
            else:
                assert np.float64(g).tobytes() == np.float64(w).tobytes(), (stage, k, g, w)
        else:
            assert int(g) == int(w), (stage, k, g, w)


def same_increment(got, want, n):
    assert got["registered"] == want["registered"], (n, got["registered"], want["registered"])
    same_stats(got["register"], want["register"], "register")
    same_stats(got["extend"], want["extend"], "extend")
    assert len(got["alternate"]) == len(want["alternate"]), n
    for a, b in zip(got["alternate"], want["alternate"]):
        assert len(a) == len(b)
        for stage, x, y in zip(("points", "poses", "camera"), a, b):
            same_stats(x, y, stage)
    same_stats(got["filter"], want["filter"], "filter")
    same_stats(got["complete"], want["complete"], "complete")


def same_snapshot(got, want, where):
    for k in ("pose_ids", "poses", "camera", "inliers", "points", "residuals"):
        assert got[k] == want[k], (where, k)


def watch_visibility(ctx, log):
    """every visibility() call of the glue between two reads of the map: the call is read-only"""
    real = ctx.visibility

    def read():
        try:
            return [a.tobytes() for a in ctx.points3d() + ctx.pose_list()]
        except _lib.MsfmError as e:                                  # (initialize's calls: no map yet)
            assert e.code == _lib.E_STATE
            return None

    def spy(*a, **k):
        before = read()
        out = real(*a, **k)
        assert read() == before, "visibility() changed the map"
        log.append(before is not None)
        return out

    ctx.visibility = spy


def device_run(ctx, name, off=False, stream=False):
    """the chain on the device against the stand-in's, stage by stage and increment by increment -> (the figures against ground truth,
    the camera the session ends with)"""
    cap, want = rfx.variant(name), twin_run(name, off)
    cam = start_camera(cap, off)
    lists, records, stats = rfx.open_session(ctx, cap, cam, stream)
    assert all(np.array_equal(a, b) for a, b in zip(lists[:2], want["lists"][:2]))
    assert np.asarray(lists[2], np.float32).tobytes() == want["lists"][2].tobytes()
    assert records.tobytes() == want["records"].tobytes(), np.nonzero(records != want["records"])[0][:8]
    assert {k: int(stats[k]) for k in tracks_ref.COUNT_KEYS} == want["track_stats"]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(ctx.tracks(), want["tracks"]))
    seen = []
    watch_visibility(ctx, seen)
    pair, trials, init = ctx.initialize(cam, rfx.two_view_dict(cap, records), min_points=rfx.MIN_POINTS)
    assert (pair, trials) == (want["pair"], want["trials"])
    same_stats(init, want["init"], "triangulate")
    first, second, rec = ctx.poses()[pair[0]], ctx.poses()[pair[1]], rfx.two_view_dict(cap, records)[pair]
    assert np.array_equal(first[0], np.eye(3)) and not first[1].any()              # the record's image 1, as the pair was given
    assert np.array_equal(second[0], rec["R"].reshape(3, 3)) and np.array_equal(second[1], rec["t"]) and init["succeeded"] >= rfx.MIN_POINTS
    same_snapshot(rfx.snapshot(ctx), want["init_state"], "initialize")
    calls = len(seen)
    n = 0
    for n, (inc, step) in enumerate(itertools.zip_longest(rfx.increments(ctx, cam, CAMERA_PARAMS if off else None), want["steps"]), 1):
        assert inc is not None and step is not None, "the device and the stand-in ran different numbers of increments"
        winc, wsnap = step
        same_increment(inc, winc, n)
        same_snapshot(rfx.snapshot(ctx), wsnap, "increment %d" % n)
    assert n == len(want["steps"]) == 22
    assert len(seen) - calls >= 2 * n and all(seen[calls:])          # (grow: one call for the candidates, one for the window)
    del ctx.visibility
    # ---- against the ground truth, whatever the stand-in said ----
    assert sorted(ctx.poses()) == sorted(int(i) for i in cap["ids"]) == want["posed"], "every one of the 24 images must end posed"
    f = rfx.measure(cap, ctx)
    print("figures[%s%s] %s" % (name, "-offcamera" if off else "", {k: float("%.4g" % v) for k, v in f.items()}))
    assert rfx.within(f, name + ("-offcamera" if off else "")) == []
    end = ctx.camera()
    ctx.tracks_end()
    return f, end


@pytest.mark.parametrize("name", ("s77", "s5", "s77-clean", "s77-distorted", "s77-permuted", "s77-swapped"))
def test_the_device_reconstructs_the_scene(tctx, name):
    DEVICE_FIGURES[name] = device_run(tctx, name)[0]


def test_streamed_under_forced_cuts(tctx):
    """set_limits(max_pairs_per_batch=23): 12 sub-batches, three in flight, their folds on three streams; the verified streaming form
    hands the records out chunk by chunk.  The same records, tracks and map."""
    tctx.set_limits(max_pairs_per_batch=23)
    device_run(tctx, "s77", stream=True)
    assert tctx.profile()["sub_batches"] >= 12


def test_a_camera_that_is_off_reaches_every_stage(tctx):
    """started from bad(CAM) with refine_camera on fx, fy in every round: every increment registers under the camera the round before
    left (camera() is part of the bytes compared after every increment) and the camera ends closer to the true one"""
    cap = rfx.variant("s77")
    start, end = bad(cap["cam"]), device_run(tctx, "s77", off=True)[1]
    for j, k in enumerate(("fx", "fy")):
        assert abs(end[k] - cap["cam"][j]) < abs(start[j] - cap["cam"][j]), (k, start[j], end[k])


def test_relabelling_reaches_the_same_map(built_lib):
    """permuted ids, every second pair given as (b, a): the same set of images posed (device_run asserts all 24) and the figures of the
    three runs inside one bound, 2 x the largest the CPU chain recorded among them"""
    family = ("s77", "s77-permuted", "s77-swapped")
    common = {k: max(rfx.MEASURED[n][k] for n in family) for k in rfx.FIGURES}
    common["share_succeeded"] = min(rfx.MEASURED[n]["share_succeeded"] for n in family)
    for n in family:
        if n not in DEVICE_FIGURES:
            with _lib.Context(0) as ctx:
                DEVICE_FIGURES[n] = device_run(ctx, n)[0]
        assert rfx.within(DEVICE_FIGURES[n], n, {n: common}) == []
