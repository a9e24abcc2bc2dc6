"""A whole reconstruction, descriptors to map, on the CPU stand-in (tests/twin_context.TwinContext: the host twins behind _lib.Context's
own glue) against the GROUND TRUTH of the capture (tests/reconstruction_fixtures.py).  No GPU.  What the stage tests cannot see is
asserted here: that the stages compose.

The chain, per fixture variant: verified matching under VERIFY_ESSENTIAL with two-view records (30, 2.0, 4.0) over all 276 pairs inside
a track session; tracks; initialize(min_points=65); reconstruct(max_images=1, window=5, rounds=2, complete_params={}) -- the
reference's loop; reconstruct(rounds=2, complete_params={}) once more with grow's default batching.

Parameters for which EVERY one of the 24 images ends posed (the completion condition), found on the twin chain alone.  A pair of this
capture shares 60 .. 75 scene points and an unposed image sees 15 .. 20 points of a young map, so two of the library's defaults are too
high for it:
  * register_params = {min_inliers: 8} (default 15): with 15 no image of seed 77 registers at all behind the initial pair;
  * initialize(min_points=65) (default 100 can never be reached).  With min_points 30 seed 77 starts from the pair (10, 1), whose noisy
    record is 3.3 degrees off: 10 of its 70 tracks fail the 2 px test, nothing registers one at a time, and the batched call then poses
    all 24 on a map that is 11 degrees and 1.9 scene units off.  65 passes that pair over (60 points) for (13, 10) (68 points).
Seeds 77 and 5 both reach 24 of 24 under these parameters, in every variant below; all of them register inside the reference's loop.

The accuracy figures (reconstruction_fixtures.align: Umeyama on the camera centres, then per-image centre and rotation error, per-point
error over the succeeded points whose fitting observations belong to one prototype) were MEASURED on this chain and are recorded in
reconstruction_fixtures.MEASURED and in DESIGN.md; the bound is 2 x the recorded value (reconstruction_fixtures.within).  Every test
prints its figures before it asserts.

Camera: started from test_gpu_refine_camera.bad(CAM) -- the verification, the initialisation and the registrations all run under it --
with camera_params={"mask": ("fx_fy",)}.  Measured (seed 77 / seed 5): fx 2550 -> 2549.07 / 2548.34, fy 2450 -> 2453.44 / 2452.02
against the true 2500: closer, by 2 .. 7 % of the error.  The map is built under the wrong camera and absorbs it; refine_camera, which
holds poses and points, then finds its minimum next to where it started.  With "cx_cy" or "k1_k2" in the mask the refined centre and
distortion do NOT all end closer (seed 77: cy 1144 -> 1143.99 against 1152, k2 -0.005 -> 0.105 against 0): those masks are not asserted."""
import functools

import numpy as np
import pytest

import reconstruction_fixtures as rfx
import tracks_fixtures
from test_gpu_refine_camera import bad
from twin_context import TwinContext

NOISY = ("s77", "s5", "s77-distorted", "s5-distorted", "s77-permuted", "s77-swapped")
CLEAN = ("s77-clean", "s5-clean")
OFF_CAMERA = ("s77", "s5")
CAMERA_PARAMS = dict(mask=("fx_fy",))


def run_chain(cap, cam=None, camera_params=None):
    ctx = TwinContext()
    lists, records, stats = rfx.open_session(ctx, cap, cam)
    cam = cap["cam"] if cam is None else cam
    two_view = rfx.two_view_dict(cap, records)
    pair, trials, init = ctx.initialize(cam, two_view, min_points=rfx.MIN_POINTS)
    c = dict(cap=cap, ctx=ctx, lists=lists, records=records, track_stats=stats, two_view=two_view, pair=pair, trials=trials, init=init,
             init_poses=ctx.poses(), camera_start=ctx.camera())
    extra = {} if camera_params is None else dict(camera_params=camera_params)
    c["loop"] = ctx.reconstruct(cam, **rfx.LOOP, **extra)
    c["batch"] = ctx.reconstruct(cam, **rfx.BATCH, **extra)
    c["figures"] = rfx.measure(cap, ctx)
    return c


@functools.lru_cache(maxsize=None)
def chain(name):
    return run_chain(rfx.variant(name))


@functools.lru_cache(maxsize=None)
def off_camera_chain(name):
    cap = rfx.variant(name)
    return run_chain(cap, bad(cap["cam"]), CAMERA_PARAMS)


def record_errors(cap, records, pairs=None):
    """every valid record against the true relative pose of the pair AS GIVEN -> (rotation errors, translation direction errors)"""
    rot, tra = [], []
    for p, (a, b) in enumerate(cap["pairs"] if pairs is None else pairs):
        if records[p]["valid"]:
            R, t = rfx.relative_pose(cap, a, b)
            rot.append(rfx.angle_deg(records[p]["R"], R))
            tra.append(rfx.direction_deg(records[p]["t"], t))
    return np.asarray(rot), np.asarray(tra)


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", (77, 5))
@pytest.mark.parametrize("cam", (rfx.CAM, rfx.CAM_D), ids=("pinhole", "distorted"))
def test_ground_truth_reprojects_to_the_keypoints(seed, cam):
    """X through the true poses and the camera reproduces the keypoints of a noise-free capture to float32 rounding: half a unit in the
    last place of the stored coordinate (the double computation itself is exact to 1e-9 px)."""
    cap = rfx.capture(seed, 0.0, cam)
    n = 0
    for i in cap["ids"]:
        rows, want = rfx.reprojection(cap, i)
        got = cap["kps"][int(i)][rows, :2]
        assert np.all(np.abs(got.astype(np.float64) - want) <= 0.5 * np.spacing(np.abs(got)).astype(np.float64) + 1e-9), int(i)
        n += len(rows)
    assert n == 24 * 300


def test_variants_are_the_same_capture():
    ids, imgs, kps, pairs = tracks_fixtures.scene_job(seed=77)
    cap = rfx.variant("s77")
    assert np.array_equal(cap["ids"], ids) and np.array_equal(cap["pairs"], pairs)
    assert all(np.array_equal(a, b) for a, b in zip(cap["imgs"], imgs)) and all(np.array_equal(cap["kps"][int(i)], k) for i, k in zip(ids, kps))
    per, swp = rfx.variant("s77-permuted"), rfx.variant("s77-swapped")
    assert sorted(per["ids"]) == sorted(ids) and not np.array_equal(per["ids"], ids)
    assert all(np.array_equal(per["kps"][int(per["ids"][k])], kps[k]) for k in range(24))           # position k: the same image
    assert (per["pairs"][:, 0] < per["pairs"][:, 1]).any() and (per["pairs"][:, 0] > per["pairs"][:, 1]).any()
    assert np.array_equal(swp["pairs"][0::2], pairs[0::2]) and np.array_equal(swp["pairs"][1::2], pairs[1::2, ::-1])
    assert {frozenset(p) for p in per["pairs"].tolist()} == {frozenset(p) for p in pairs.tolist()}


# ---- conventions, per record ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NOISY + CLEAN)
def test_two_view_records_follow_the_pair_as_given(name):
    """Every valid record's (R, t) against x2 ~ R x1 + t of the pair as it was GIVEN (image 1 = the pair's first id).  Bounds: 2 x the
    figures recorded in reconstruction_fixtures.RECORDS (median and maximum of the rotation and of the translation direction error, in
    degrees); seed 77 with noise also the figures first measured for it (0.79 / 5.0 / 0.82 / 10.5 at that precision).  A record
    with the roles swapped or R transposed is off by the pair's relative rotation, tens of degrees for most pairs."""
    c = chain(name)
    rec = c["records"]
    assert rec["valid"].all() and len(rec) == 276
    rot, tra = record_errors(c["cap"], rec)
    got = (float(np.median(rot)), float(rot.max()), float(np.median(tra)), float(tra.max()))
    print("records[%s] rotation median %.4g max %.4g, direction median %.4g max %.4g degrees" % ((name,) + got))
    want = rfx.RECORDS[name]
    assert all(g <= 2.0 * w for g, w in zip(got, want)), (got, want)
    if name == "s77":
        assert got[0] < 0.795 and got[1] < 5.05 and got[2] < 0.825 and got[3] < 10.55, got
    if name in CLEAN:
        assert got[0] < 1e-3 and got[2] < 1e-3, got
    assert abs(np.linalg.norm(rec["t"], axis=1) - 1.0).max() < 1e-9


def test_a_pair_given_both_ways_yields_inverse_poses():
    """All 276 pairs of the noise-free capture given as (b, a) -- another list, so another RANSAC draw per pair: R' = R^T and
    t' ~ -R^T t.  The reversed records are held against the truth like the others (RECORDS["s77-clean-reversed"]); each pair's two
    records are then within the sum of their bounds of each other, and the median pair within 1e-3 degrees (float32 rounding of the
    keypoints is all that separates either record from the truth)."""
    c = chain("s77-clean")
    cap = c["cap"]
    rev = dict(cap, pairs=np.ascontiguousarray(cap["pairs"][:, ::-1]))
    _, records, _ = rfx.open_session(TwinContext(), rev)
    rot, tra = record_errors(rev, records)
    got = (float(np.median(rot)), float(rot.max()), float(np.median(tra)), float(tra.max()))
    print("records[s77-clean-reversed] rotation median %.4g max %.4g, direction median %.4g max %.4g degrees" % got)
    assert records["valid"].all() and all(g <= 2.0 * w for g, w in zip(got, rfx.RECORDS["s77-clean-reversed"])), got
    assert got[0] < 1e-3 and got[2] < 1e-3
    rmax = 2.0 * (rfx.RECORDS["s77-clean"][1] + rfx.RECORDS["s77-clean-reversed"][1])
    tmax = 2.0 * (rfx.RECORDS["s77-clean"][3] + rfx.RECORDS["s77-clean-reversed"][3])
    both = np.asarray([(rfx.angle_deg(b["R"], a["R"].reshape(3, 3).T), rfx.direction_deg(b["t"], -a["R"].reshape(3, 3).T @ a["t"]))
                       for a, b in zip(c["records"], records)])
    assert both[:, 0].max() <= rmax and both[:, 1].max() <= tmax + rmax, both.max(axis=0)
    assert np.median(both[:, 0]) < 1e-3 and np.median(both[:, 1]) < 1e-3, np.median(both, axis=0)


# ---- initialisation ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("s77", "s5", "s77-clean", "s77-permuted", "s77-swapped"))
def test_initialize_stands_on_a_real_record(name):
    c = chain(name)
    pair, rec = c["pair"], c["two_view"].get(c["pair"])
    assert rec is not None, "initialize must return the pair under the key it was given"
    assert rec["valid"] and rec["is_initial_candidate"] and 1 <= c["trials"] <= 100 and c["init"]["succeeded"] >= rfx.MIN_POINTS
    poses = c["init_poses"]
    assert sorted(poses) == sorted(pair)
    assert np.array_equal(poses[pair[0]][0], np.eye(3)) and not poses[pair[0]][1].any()            # the record's image 1 at (I, 0)
    assert np.array_equal(poses[pair[1]][0], rec["R"].reshape(3, 3)) and np.array_equal(poses[pair[1]][1], rec["t"])
    R, t = rfx.relative_pose(c["cap"], *pair)
    print("initialize[%s] pair %s, trial %d, %d points, record %.3g / %.3g degrees off" % (name, pair, c["trials"], c["init"]["succeeded"],
                                                                                           rfx.angle_deg(rec["R"], R), rfx.direction_deg(rec["t"], t)))
    if name in ("s77-permuted", "s77-swapped"):
        assert pair[0] < pair[1], "these two variants are there to start from a pair that is not (high, low)"
    else:
        assert pair[0] > pair[1]


# ---- completion and accuracy ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NOISY + CLEAN)
def test_every_image_ends_posed_and_the_map_is_the_scene(name):
    c = chain(name)
    ctx, cap = c["ctx"], c["cap"]
    print("figures[%s] %s" % (name, {k: float("%.4g" % v) for k, v in c["figures"].items()}))
    assert sorted(ctx.poses()) == sorted(int(i) for i in cap["ids"]), "every one of the 24 images must end posed"
    assert all(len(o["registered"]) == 1 for o in c["loop"]) and len(c["loop"]) + sum(len(o["registered"]) for o in c["batch"]) == 22
    assert rfx.within(c["figures"], name) == []


@pytest.mark.parametrize("seed", (77, 5))
def test_without_noise_the_errors_are_orders_of_magnitude_smaller(seed):
    """float32 keypoint rounding (1e-4 px) against 0.7 px of noise: nothing else may limit the accuracy, a convention that is only
    nearly right included"""
    noisy, clean = chain("s%d" % seed)["figures"], chain("s%d-clean" % seed)["figures"]
    for k in ("centre_max", "rotation_max", "point_median", "point_p95"):
        assert clean[k] <= noisy[k] / 100.0, (k, clean[k], noisy[k])


def test_relabelling_reaches_the_same_map():
    """the same capture under permuted ids and with every second pair given as (b, a): the same set of images posed, and the figures of
    all three inside ONE bound, 2 x the largest recorded among them (another initial pair, other RANSAC draws: the maps agree as far
    as the chain is accurate, not bit for bit)"""
    family = ("s77", "s77-permuted", "s77-swapped")
    common = {k: max(rfx.MEASURED[n][k] for n in family) for k in rfx.FIGURES}
    common["share_succeeded"] = min(rfx.MEASURED[n]["share_succeeded"] for n in family)
    posed = [sorted(chain(n)["ctx"].poses()) for n in family]
    assert posed[0] == posed[1] == posed[2] and len(posed[0]) == 24
    for n in family:
        assert rfx.within(chain(n)["figures"], n, {n: common}) == []
    assert chain("s77")["track_stats"] == chain("s77-permuted")["track_stats"]      # (the same matches under other names)


# ---- camera --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", OFF_CAMERA)
def test_a_camera_that_is_off_ends_closer(name):
    c = off_camera_chain(name)
    cap, ctx = c["cap"], c["ctx"]
    start, end, true = c["camera_start"], ctx.camera(), dict(zip(("fx", "fy", "cx", "cy"), cap["cam"]))
    print("camera[%s] %s -> %s; figures %s" % (name, {k: start[k] for k in ("fx", "fy")}, {k: float("%.7g" % end[k]) for k in ("fx", "fy")},
                                               {k: float("%.4g" % v) for k, v in c["figures"].items()}))
    assert tuple(start[k] for k in ("fx", "fy", "cx", "cy", "k1", "k2")) == bad(cap["cam"])[:6]
    assert sorted(ctx.poses()) == sorted(int(i) for i in cap["ids"])
    assert sum(a[2]["refined"] for o in c["loop"] + c["batch"] for a in o["alternate"]) > 0
    for k in ("fx", "fy"):
        assert abs(end[k] - true[k]) < abs(start[k] - true[k]), (k, start[k], end[k])
    assert all(end[k] == start[k] for k in ("cx", "cy", "k1", "k2", "p1", "p2"))                    # not in the mask
    assert rfx.within(c["figures"], name + "-offcamera") == []
