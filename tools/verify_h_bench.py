"""Device time of the geometric verification, fundamental matrix (model 0) against the staged homography (model 2), on three
workloads:

    e2e      the end_to_end job's database contents (synth.south_building_database: 128 images x ~5000 float32 descriptors,
             keypoints observing the points of a 3-D box), all 8 128 pairs -- a general scene: only near-planar subsets agree with an H
    planar   the same descriptors with the keypoints of one facade (synth.south_building_planar): one H explains each pair
    config4  the config-4-shaped byte images (synth.u8_database's contents, as tools/verify_e_bench.py builds them), --images of
             them (default 256 of the 1329), all pairs

    python tools/verify_h_bench.py [--workload e2e|planar|config4|all] [--images 256] [--model 0|2|both] [--out profiles/verify_h_bench.json]

One msfm_match_pairs_verified call per (workload, model) after an untimed warm-up call.  The byte workload is matched without the
distance cut (its distances are in byte units).  Prints one JSON object and writes it to --out."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

from monocularsfm_amd import _lib, synth  # noqa: E402
from verify_e_bench import config4_data, e2e_data  # noqa: E402


def run(descs, kps, model, max_distance):
    with _lib.Context(0) as ctx:
        for i, (d, k) in enumerate(zip(descs, kps)):
            ctx.upload_image(i, d)
            ctx.upload_keypoints(i, k)
        if model:
            ctx.set_verification_model(model)
        pairs = synth.all_pairs(len(descs))
        ctx.match_pairs_verified(pairs, max_distance=max_distance, fetch=False)   # warm-up: buffers, plan hints
        t0 = time.perf_counter()
        offs, _, _ = ctx.match_pairs_verified(pairs, max_distance=max_distance, fetch=False)
        wall = time.perf_counter() - t0
        prof = ctx.profile()
        raw = ctx.match_pairs(pairs, max_distance=max_distance, fetch=False)[0]
        solved, rounds = ctx.verification_stats()
        out = {"model": model, "pairs": int(len(pairs)), "wall_s": wall, "total_device_ms": prof["total_device_ms"],
               "verify_ms": prof["verify_ms"], "matches_in": int(raw[-1]), "matches_kept": int(offs[-1])}
        if model == 0:
            # (F evaluates all max_iters = 1000 hypotheses of every pair with >= 8 matches at once)
            verified = int((np.diff(raw) >= 8).sum())
            out.update(pairs_verified=verified, hypotheses_solved=1000 * verified, hypotheses_per_verified_pair=1000.0)
        else:
            verified = int((np.diff(raw) >= 4).sum())
            out.update(pairs_verified=verified, hypotheses_solved=solved, max_rounds=rounds,
                       hypotheses_per_verified_pair=solved / max(1, verified))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="all", choices=["e2e", "planar", "config4", "all"])
    ap.add_argument("--images", type=int, default=256, help="config4: images of the subset")
    ap.add_argument("--model", default="both", choices=["0", "2", "both"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    models = [0, 2] if a.model == "both" else [int(a.model)]
    res = {}
    for w in (["e2e", "planar", "config4"] if a.workload == "all" else [a.workload]):
        if w == "e2e":
            descs, kps = e2e_data()
        elif w == "planar":
            descs, kps = synth.south_building_planar()
        else:
            descs, kps = config4_data(a.images)
        res[w] = [run(descs, kps, m, 1e9 if w == "config4" else 0.7) for m in models]
        print(json.dumps({w: res[w]}), file=sys.stderr, flush=True)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
