#!/usr/bin/env python
"""Point refinement at the production shape: synth.triangulation_job, 1329 images x 8192 keypoints, ~1.78 M
tracks, folded from synthetic lists through tracks_add (no matching).  Per max_iters in 1, 10, 0: --reps warm rounds behind --warmup
untimed ones, a round being msfm_triangulate_tracks (the refinement starts from DLT points every time) followed by
msfm_refine_points: median (minimum) of refine_ms beside the same rounds' triangulate_ms, the split prepare (pose table +
per-observation array) | refine kernel, the counters.  Then the same with the long tracks filtered out (tracks_finish(max_length=100)):
the difference of the refine kernel's medians is what the long tracks' tail costs.  Not a pass criterion.

    python tools/refine_points_bench.py --out profiles/refine_points_bench.json [--images 1329] [--rows 8192]
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


def rounds(ctx, poses, max_iters, reps, warmup):
    runs = []
    for k in range(warmup + reps):
        tri = ctx.triangulate_tracks(CAM, poses)
        st = ctx.refine_points(max_iters=max_iters)
        if k >= warmup:
            runs.append((tri["triangulate_ms"], st))
    out = {"max_iters": max_iters, "stats": runs[-1][1]}
    series = {"triangulate_ms": [r[0] for r in runs], "refine_ms": [r[1]["refine_ms"] for r in runs],
              "prepare_ms": [r[1]["prepare_ms"] for r in runs], "refine_kernel_ms": [r[1]["refine_ms"] - r[1]["prepare_ms"] for r in runs]}
    for key, ms in series.items():
        out.update({key: ms, key + "_median": float(np.median(ms)), key + "_min": float(min(ms))})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1329)
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    long_len = min(300, (a.images - 2) // 3)
    ids, kps, poses, lists = synth.triangulation_job(a.images, a.rows, CAM, window=a.rows - 192, step=(a.rows - 192) // 6, long_len=long_len)
    doc = {"tool": "tools/refine_points_bench.py", "images": a.images, "rows_per_image": a.rows, "reps": a.reps, "warmup": a.warmup}
    d = np.random.default_rng(1).integers(0, 256, (a.rows, 128), dtype=np.uint8)
    with _lib.Context(0) as ctx:
        for k, i in enumerate(ids):
            ctx.upload_image(int(i), d)
            ctx.upload_keypoints(int(i), kps[k])
        ctx.tracks_begin(ids, add_only=True)
        for l in lists:
            ctx.tracks_add(*l)
        dev = ctx.device_info()
        doc["device"] = dev["name"].strip() or "gfx950"
        doc["cu_count"] = dev["cu_count"]
        doc["jobs"] = []
        for name, flt in (("all tracks", {}), ("without the long tracks", {"max_length": 100})):
            ts = ctx.tracks_finish(**flt)
            job = {"job": name, "tracks": {k: ts[k] for k in ("tracks_kept", "observations_kept", "longest_track")}, "runs": []}
            for mi in (1, 10, 0):
                r = rounds(ctx, poses, mi, a.reps, a.warmup)
                job["runs"].append(r)
                print(json.dumps({"job": name, "max_iters": mi} | {k: r[k] for k in r if k.endswith("_median") or k.endswith("_min")} |
                                 {k: r["stats"][k] for k in ("eligible", "refined", "gained_error_ok", "rejected_by_verdict", "iterations")}), flush=True)
            doc["jobs"].append(job)
        doc["long_track_tail_ms"] = {str(x["max_iters"]): x["refine_kernel_ms_median"] - y["refine_kernel_ms_median"]
                                     for x, y in zip(doc["jobs"][0]["runs"], doc["jobs"][1]["runs"])}
        print(json.dumps({"long_track_tail_ms": doc["long_track_tail_ms"]}), flush=True)
        ctx.tracks_end()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
