#!/usr/bin/env python
"""Pose refinement at the production shape: synth.triangulation_job, 1329 images x 8192 keypoints, ~1.78 M
tracks, folded from synthetic lists through tracks_add (no matching); every pose but the first is turned by --rot radians and moved by
--trans units (seeded), the first is held fixed.  Reports --reps warm rounds behind --warmup untimed ones, a round being
msfm_triangulate_tracks followed by ONE msfm_refine_poses: median (minimum) of refine_ms and of its split prepare (pose table,
per-observation array, image-major list: key, radix sort, offsets, fill) | the image kernel and the re-verdict, beside the counters;
then six rounds of Context.alternate from fresh DLT points: per round the two calls' times and the RMS reprojection error over the
fitting observations before and after the pose call.  Not a pass criterion: nothing earlier exists to compare with.

    python tools/refine_poses_bench.py --out profiles/refine_poses_bench.json [--images 1329] [--rows 8192]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from monocularsfm_amd import _lib, synth  # noqa: E402

CAM = (2500.0, 2500.0, 1536.0, 1152.0)
COUNTERS = ("images", "eligible", "refined", "rejected_by_inliers", "iterations", "observations", "points_reposed", "points_lost", "points_gained")


def rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0.0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def perturbed(poses, rot, trans, seed=1):
    rng = np.random.default_rng(seed)
    out = {}
    for n, i in enumerate(sorted(poses)):
        w, d = rng.normal(size=3), rng.normal(size=3)
        R, t = poses[i]
        out[i] = (R, t) if n == 0 else (rodrigues(w * rot / np.linalg.norm(w)) @ np.asarray(R, np.float64),
                                        np.asarray(t, np.float64) + d * trans / np.linalg.norm(d))
    return out


def rms(st, key):
    return float(np.sqrt(st[key] / max(st["observations"], 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1329)
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rot", type=float, default=2e-4)
    ap.add_argument("--trans", type=float, default=1e-3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    long_len = min(300, (a.images - 2) // 3)
    ids, kps, poses, lists = synth.triangulation_job(a.images, a.rows, CAM, window=a.rows - 192, step=(a.rows - 192) // 6, long_len=long_len)
    bad = perturbed(poses, a.rot, a.trans)
    fixed = [min(bad)]
    doc = {"tool": "tools/refine_poses_bench.py", "images": a.images, "rows_per_image": a.rows, "reps": a.reps, "warmup": a.warmup,
           "rot": a.rot, "trans": a.trans}
    d = np.random.default_rng(1).integers(0, 256, (a.rows, 128), dtype=np.uint8)
    with _lib.Context(0) as ctx:
        for k, i in enumerate(ids):
            ctx.upload_image(int(i), d)
            ctx.upload_keypoints(int(i), kps[k])
        ctx.tracks_begin(ids, add_only=True)
        for l in lists:
            ctx.tracks_add(*l)
        ts = ctx.tracks_finish()
        dev = ctx.device_info()
        doc["device"] = dev["name"].strip() or "gfx950"
        doc["cu_count"] = dev["cu_count"]
        doc["tracks"] = {k: ts[k] for k in ("tracks_kept", "observations_kept", "longest_track")}
        runs = []
        for k in range(a.warmup + a.reps):
            tri = ctx.triangulate_tracks(CAM, bad)
            st = ctx.refine_poses(fixed=fixed)
            if k >= a.warmup:
                runs.append((tri["triangulate_ms"], st))
        one = {"stats": runs[-1][1], "rms_before_px": rms(runs[-1][1], "cost_before"), "rms_after_px": rms(runs[-1][1], "cost_after")}
        series = {"triangulate_ms": [r[0] for r in runs], "refine_ms": [r[1]["refine_ms"] for r in runs],
                  "prepare_ms": [r[1]["prepare_ms"] for r in runs], "image_and_verdict_ms": [r[1]["refine_ms"] - r[1]["prepare_ms"] for r in runs]}
        for key, ms in series.items():
            one.update({key: ms, key + "_median": float(np.median(ms)), key + "_min": float(min(ms))})
        doc["one_call"] = one
        print(json.dumps({k: one[k] for k in one if k.endswith("_median") or k.endswith("_min") or k.startswith("rms")} |
                         {k: one["stats"][k] for k in COUNTERS}), flush=True)
        ctx.triangulate_tracks(CAM, bad)
        doc["alternate"] = []
        for n, (p, q) in enumerate(ctx.alternate(6, fixed=fixed, point_params=dict(max_iters=5, step_tol=1e-6))):
            r = {"round": n, "refine_points_ms": p["refine_ms"], "points_refined": p["refined"], "refine_poses_ms": q["refine_ms"],
                 "prepare_ms": q["prepare_ms"], "poses_refined": q["refined"], "rejected_by_inliers": q["rejected_by_inliers"],
                 "iterations": q["iterations"], "rms_before_px": rms(q, "cost_before"), "rms_after_px": rms(q, "cost_after"),
                 "points_lost": q["points_lost"], "points_gained": q["points_gained"]}
            doc["alternate"].append(r)
            print(json.dumps(r), flush=True)
        ctx.tracks_end()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
