#!/usr/bin/env python
"""Track triangulation at the production shape: synth.triangulation_job, 1329 images x 8192 keypoints, ~1.78 M
tracks of six or seven views plus eight tracks through 294 posed views, ~10.5 M used observations, folded from synthetic lists through
tracks_add (no matching).  Reports, per setting, triangulate_ms (the library's HIP events around tri_pose_kernel + tri_track_kernel;
median, minimum and all of --reps warm calls behind --warmup untimed ones), used observations per second, and the bytes the kernel
gathers per second against the achievable HBM figure (6.3 TB/s): per used observation the 8 bytes of the CSR element, the 16-byte table
entry, the 8-byte keypoint and the 128-byte prepared pose, each read in the DLT pass and again in the error pass (the parallax scan's
reads come on top and are not counted), plus the 8-byte residual and, per track, 48 bytes of record and 17 of offsets and flag.
Settings: the defaults (2 px, 1.5 degrees, 2 views); min_angle = 180, which no pair reaches, so that EVERY track scans all its pairs --
the long tracks 43 071 each -- the worst case of the one-lane-per-track mapping; and both again on the result filtered to max_length
below the long tracks, to see what the long tracks cost.  Beside it, for scale only, the host twin's time on 16 threads.

    python tools/triangulation_bench.py --out profiles/triangulation_bench.json [--images 1329] [--rows 8192] [--reps 7] [--warmup 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from monocularsfm_amd import _lib, synth  # noqa: E402

HBM_ACHIEVABLE = 6.3e12   # bytes/s, float4 copy on one MI355X
CAM = (2500.0, 2500.0, 1536.0, 1152.0)
PER_OBS = 2 * (8 + 16 + 8 + 128) + 8
PER_TRACK = 48 + 17


def timed(ctx, poses, params, reps, warmup):
    for _ in range(warmup):
        ctx.triangulate_tracks(CAM, poses, *params)
    ms, st = [], None
    for _ in range(reps):
        st = ctx.triangulate_tracks(CAM, poses, *params)
        ms.append(st["triangulate_ms"])
    med = float(np.median(ms))
    gathered = PER_OBS * st["observations_used"] + PER_TRACK * st["tracks"]
    return {"params": {"max_error": params[0], "min_angle": params[1], "min_views": params[2]}, "triangulate_ms": ms,
            "triangulate_ms_median": med, "triangulate_ms_min": float(min(ms)), "stats": st,
            "observations_per_s": st["observations_used"] / (med * 1e-3), "gathered_bytes": gathered,
            "gathered_bytes_per_s": gathered / (med * 1e-3), "share_of_hbm_achievable": gathered / (med * 1e-3) / HBM_ACHIEVABLE}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1329)
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-twin", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    long_len = min(300, (a.images - 2) // 3)
    t0 = time.perf_counter()
    ids, kps, poses, lists = synth.triangulation_job(a.images, a.rows, CAM, window=a.rows - 192, step=(a.rows - 192) // 6, long_len=long_len)
    doc = {"tool": "tools/triangulation_bench.py", "images": a.images, "rows_per_image": a.rows, "synth_s": round(time.perf_counter() - t0, 2),
           "reps": a.reps, "warmup": a.warmup, "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE, "bytes_per_used_observation": PER_OBS,
           "bytes_per_track": PER_TRACK}
    d = np.random.default_rng(1).integers(0, 256, (a.rows, 128), dtype=np.uint8)
    with _lib.Context(0) as ctx:
        for k, i in enumerate(ids):
            ctx.upload_image(int(i), d)
            ctx.upload_keypoints(int(i), kps[k])
        ctx.tracks_begin(ids, add_only=True)
        for l in lists:
            ctx.tracks_add(*l)
        ts = ctx.tracks_finish()
        doc["tracks"] = {k: ts[k] for k in ("tracks_kept", "observations_kept", "longest_track", "finish_ms")}
        dev = ctx.device_info()
        doc["device"] = dev["name"].strip() or "gfx950"
        doc["cu_count"] = dev["cu_count"]
        runs = []
        for name, prm in (("defaults", (2.0, 1.5, 2)), ("full_scan_min_angle_180", (2.0, 180.0, 2)), ("defaults_again", (2.0, 1.5, 2))):
            r = timed(ctx, poses, prm, a.reps, a.warmup)
            r["setting"] = name
            runs.append(r)
            print(json.dumps({k: r[k] for k in ("setting", "triangulate_ms_median", "triangulate_ms_min", "observations_per_s", "share_of_hbm_achievable")}), flush=True)
        # the long tracks' cost: they are filtered out (a finish with max_length below them), then the same calls
        ctx.tracks_finish(max_length=long_len - 1)
        for name, prm in (("defaults_without_long_tracks", (2.0, 1.5, 2)), ("full_scan_without_long_tracks", (2.0, 180.0, 2))):
            r = timed(ctx, poses, prm, a.reps, a.warmup)
            r["setting"] = name
            runs.append(r)
            print(json.dumps({k: r[k] for k in ("setting", "triangulate_ms_median", "triangulate_ms_min", "observations_per_s", "share_of_hbm_achievable")}), flush=True)
        doc["runs"] = runs
        ctx.tracks_finish()
        tracks = ctx.tracks()
        ctx.tracks_end()
    if not a.no_twin:
        import triangulation_twin as tw
        host = tw.load_host()
        kp = {int(i): k for i, k in zip(ids, kps)}
        twin = {}
        for name, prm in (("defaults", (2.0, 1.5, 2)), ("full_scan_min_angle_180", (2.0, 180.0, 2))):
            t0 = time.perf_counter()
            pts, _ = tw.run(host, tracks, ids, kp, poses, CAM, prm, workers=16)
            twin[name] = {"wall_ms_16_threads": (time.perf_counter() - t0) * 1e3, "counts": tw.counts(pts)}
        doc["host_twin_for_scale_only"] = twin
        print(json.dumps(twin), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
