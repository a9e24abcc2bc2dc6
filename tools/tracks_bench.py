#!/usr/bin/env python
"""What an open track session costs a matching call: warm msfm_match_pairs_verified calls on one context, with
the session closed and open in one process, on the e2e job (128 x ~5000 f32, 8 128 pairs) and the config-4-shaped byte job (256 x 8192
u8, 32 640 pairs).  Per job: wall and total device ms of the call both ways (medians of --reps), the summed fold-kernel time, the
finish time, edges per second of the fold, tracks, observations, inconsistent tracks.  One JSON document on stdout / --out.

    python tools/tracks_bench.py --out profiles/tracks_bench.json [--jobs e2e,u8] [--reps 5] [--modes closed,open,keep,closed]
                                 [--off-path-log lines_of_bench_py]

Under `rocprofv3 --kernel-trace --stats -- python tools/tracks_bench.py --jobs u8 --modes closed` (and `--modes keep`) the per-kernel
totals of the two runs say which launches an open session stretches.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from monocularsfm_amd import _lib, synth  # noqa: E402


def e2e_job():
    imgs, pairs, name = synth.job("south-building")
    counts = [len(x) for x in imgs]
    same, protos = synth.rootsift_images(len(imgs), counts, seed=1234, n_proto=20000, sigma=0.05, return_proto=True)
    assert all(np.array_equal(a, b) for a, b in zip(imgs, same))
    kps = synth.scene_keypoints(protos, synth.scene_cameras(len(imgs), seed=1234), 20000, seed=1234)
    return name, imgs, kps, pairs, dict(ratio=0.8, cross_check=True, max_distance=0.7)


def u8_job(n_images=256, n_desc=8192):
    imgs, planted = synth.u8_images(n_images, n_desc, seed=1234, as_float=False, return_planted=True)
    n_pool = max(len(p) for p in planted)
    point_ids = []
    for k, rows in enumerate(planted):
        ids = np.full(len(imgs[k]), -1, np.int64)
        ids[rows] = np.arange(len(rows))
        point_ids.append(ids)
    kps = synth.scene_keypoints(point_ids, synth.scene_cameras(n_images, seed=1234), n_pool, seed=1234)
    name = "synthetic u8 descriptors: %d images x %d desc, brute-force all pairs" % (n_images, n_desc)
    return name, imgs, kps, synth.all_pairs(n_images), dict(ratio=0.8, cross_check=True, max_distance=1e9)


def measure(ctx, pairs, prm, reps, session_ids=None, min_pair=10, keep_open=False):
    """reps warm calls -> (timings, the last session's stats).  session_ids: a session is open during every call -- one per call
    (begin / call / finish / end, the begin and the finish outside the clock), or with keep_open ONE session across all the calls
    (what a run does), finished once behind the last."""
    wall, dev, stats = [], [], None
    if session_ids is not None and keep_open:
        ctx.tracks_begin(session_ids, min_pair_matches=min_pair)
    for _ in range(reps):
        if session_ids is not None and not keep_open:
            ctx.tracks_begin(session_ids, min_pair_matches=min_pair)
        t0 = time.perf_counter()
        offs, _, _ = ctx.match_pairs_verified(pairs, fetch=False, **prm)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(ctx.profile()["total_device_ms"])
        if session_ids is not None and not keep_open:
            t0 = time.perf_counter()
            stats = ctx.tracks_finish()
            stats["finish_wall_ms"] = (time.perf_counter() - t0) * 1e3
            ctx.tracks_end()
    if session_ids is not None and keep_open:
        t0 = time.perf_counter()
        stats = ctx.tracks_finish()
        stats["finish_wall_ms"] = (time.perf_counter() - t0) * 1e3
        stats["calls_folded"] = reps
        ctx.tracks_end()
    return {"wall_ms": wall, "device_ms": dev, "wall_ms_median": float(np.median(wall)), "device_ms_median": float(np.median(dev)),
            "matches": int(offs[-1])}, stats


def run(job, reps, modes):
    name, imgs, kps, pairs, prm = job
    phases = []
    with _lib.Context(0) as ctx:
        ids = np.arange(len(imgs), dtype=np.int32)
        for i in ids:
            ctx.upload_image(int(i), imgs[i])
            ctx.upload_keypoints(int(i), kps[i])
        for _ in range(2):
            ctx.match_pairs_verified(pairs, fetch=False, **prm)
        for mode in modes:
            t, st = measure(ctx, pairs, prm, reps, None if mode == "closed" else ids, keep_open=(mode == "keep"))
            t["mode"] = mode
            if st:
                t["session"] = st
                calls = st.get("calls_folded", 1)
                t["fold_ms_per_call"] = st["fold_ms"] / calls
                t["fold_edges_per_s"] = st["edges"] / (st["fold_ms"] * 1e-3) if st["fold_ms"] > 0 else None
            phases.append(t)
        dev = ctx.device_info()
    closed = [t["device_ms_median"] for t in phases if t["mode"] == "closed"]
    for t in phases:
        if t["mode"] != "closed" and closed:
            t["device_ms_over_closed"] = t["device_ms_median"] - min(closed)
    return {"job": name, "pairs": int(len(pairs)), "device": dev["name"].strip() or "gfx950", "cu_count": dev["cu_count"], "phases": phases}


def off_path(log):
    """bench.py result lines prefixed `parent N ` / `tree N ` (parent commit and tree interleaved on one box) -> the off-path block."""
    out = {"command": "bench.py --gpus 1 --steps 20 --warmup 5, parent commit and tree interleaved on one box",
           "parent_ms_per_step": [], "tree_ms_per_step": []}
    for line in open(log):
        who, _, rest = line.partition(" ")
        if who in ("parent", "tree") and "{" in rest:
            out[who + "_ms_per_step"].append(round(json.loads(rest[rest.index("{"):])["ms_per_step"], 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", default="e2e,u8")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--modes", default="closed,open,keep,closed",
                    help="phases in order: closed (no session), open (a session per call), keep (one session across the calls)")
    ap.add_argument("--off-path-log", default=None, help="interleaved bench.py lines to record as the off-path block")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = []
    for j in a.jobs.split(","):
        res.append(run(e2e_job() if j == "e2e" else u8_job(), a.reps, a.modes.split(",")))
        print(json.dumps(res[-1]), flush=True)
    if a.out:
        doc = {"tool": "tools/tracks_bench.py", "reps": a.reps, "results": res}
        if a.off_path_log:
            doc["off_path"] = off_path(a.off_path_log)
        elif os.path.exists(a.out):   # (a re-run of the on-path part keeps the recorded off-path figures)
            try:
                old = json.load(open(a.out))
                if "off_path" in old:
                    doc["off_path"] = old["off_path"]
            except ValueError:
                pass
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
