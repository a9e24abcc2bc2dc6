"""Device time of the geometric verification, fundamental matrix (model 0) against the staged essential matrix (model 1), on the
workloads the verification runs on:

    e2e      the end_to_end job's database contents (synth.south_building_database: 128 images x ~5000 float32 descriptors,
             keypoints observing scene points through synth.scene_cameras), all 8 128 pairs
    config4  the config-4-shaped byte images (synth.u8_database's contents: planted near-duplicates observe scene points), --images of
             them (default 256 of the 1329), seeded as synth.u8_database, all pairs

    python tools/verify_e_bench.py [--workload e2e|config4|both] [--images 256] [--model 0|1|both] > verify_e.json

One msfm_match_pairs_verified call per (workload, model) after an untimed warm-up call; the camera of model 1 is the synthetic
scene's (focal 2500, principal point at the image centre, no distortion).  The byte workload is matched without the distance
cut (its distances are in byte units).  Prints one JSON object."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from monocularsfm_amd import _lib, synth  # noqa: E402

CAMERA = (2500.0, 2500.0, 1536.0, 1152.0)


def e2e_data():
    with tempfile.TemporaryDirectory() as tmp:
        descs, kps = synth.south_building_database(os.path.join(tmp, "e2e.db"))
    return descs, kps


def config4_data(n_images):
    imgs, planted = synth.u8_images(n_images, 8192, seed=1329, as_float=False, return_planted=True)
    n_pool = max(len(r) for r in planted)
    cams = synth.scene_cameras(n_images, seed=1329 + 7)
    descs, kps = [], []
    for i in range(n_images):
        d = imgs[i]
        ids = np.full(len(d), -1, np.int64)
        ids[planted[i]] = np.arange(len(planted[i]))
        k = synth.scene_keypoints([ids], [cams[i]], n_pool, seed=1329 + 9, base=[synth.keypoints(len(d), seed=1329 + 50 + i)])[0]
        descs.append(d)
        kps.append(k)
    return descs, kps


def run(descs, kps, model, max_distance):
    out = {}
    with _lib.Context(0) as ctx:
        for i, (d, k) in enumerate(zip(descs, kps)):
            ctx.upload_image(i, d)
            ctx.upload_keypoints(i, k)
        if model == 1:
            ctx.set_verification_model(1, CAMERA)
        pairs = synth.all_pairs(len(descs))
        ctx.match_pairs_verified(pairs, max_distance=max_distance, fetch=False)   # warm-up: buffers, plan hints
        t0 = time.perf_counter()
        offs, _, _ = ctx.match_pairs_verified(pairs, max_distance=max_distance, fetch=False)
        wall = time.perf_counter() - t0
        prof = ctx.profile()
        raw = ctx.match_pairs(pairs, max_distance=max_distance, fetch=False)[0]
        solved, rounds = ctx.verification_stats()
        out = {"model": model, "pairs": int(len(pairs)), "wall_s": wall, "total_device_ms": prof["total_device_ms"],
               "verify_ms": prof["verify_ms"], "matches_in": int(raw[-1]), "matches_kept": int(offs[-1]),
               "pairs_with_5_or_more": int((np.diff(raw) >= 5).sum())}
        if model == 1:
            out.update(hypotheses_solved=solved, max_rounds=rounds,
                       hypotheses_per_verified_pair=solved / max(1, out["pairs_with_5_or_more"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="both", choices=["e2e", "config4", "both"])
    ap.add_argument("--images", type=int, default=256, help="config4: images of the subset")
    ap.add_argument("--model", default="both", choices=["0", "1", "both"])
    a = ap.parse_args()
    models = [0, 1] if a.model == "both" else [int(a.model)]
    res = {}
    for w in (["e2e", "config4"] if a.workload == "both" else [a.workload]):
        descs, kps = e2e_data() if w == "e2e" else config4_data(a.images)
        # (byte descriptors: distances are in byte units, the reference's 0.7 cut is for RootSIFT -- no cut, as bench.py's u8 jobs)
        res[w] = [run(descs, kps, m, 0.7 if w == "e2e" else 1e9) for m in models]
        print(json.dumps({w: res[w]}), file=sys.stderr, flush=True)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
