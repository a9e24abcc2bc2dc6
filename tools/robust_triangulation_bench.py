#!/usr/bin/env python
"""Robust track triangulation at the production shape: synth.triangulation_job, 1329 images x 8192 keypoints,
~1.78 M tracks, folded from synthetic lists through tracks_add (no matching), with 0 %, 1 % and 10 % of the tracks corrupted by
synth.corrupt_observations (one observation moved by 40 px, the first, a middle and the last position in turn).  Per share: the plain
call and the robust call in the same process, --reps warm calls behind --warmup untimed ones each: median (minimum) of triangulate_ms
and robust_ms, the retried / rescued / rejected counts, the succeeded count beside the plain call's, the retry kernel's time per
retried track and per hypothesis (robust_ms - triangulate_ms: the retry kernel plus the one host wait).

THE ACCEPTANCE TEST: at 0 % the robust call does the plain kernel's work plus one byte stored per observation and one ballot per wave;
the median of its robust_ms may be at most 1.10 x the plain call's median triangulate_ms.  The tool exits with status 1 otherwise.
Beside it, for scale only, the host twin's time on 16 threads at 10 %.

    python tools/robust_triangulation_bench.py --out profiles/robust_triangulation_bench.json [--images 1329] [--rows 8192]
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

CAM = (2500.0, 2500.0, 1536.0, 1152.0)
BOUND = 1.10


def timed(ctx, poses, reps, warmup, **kw):
    for _ in range(warmup):
        ctx.triangulate_tracks(CAM, poses, **kw)
    runs = [ctx.triangulate_tracks(CAM, poses, **kw) for _ in range(reps)]
    out = {"stats": runs[-1]}
    for key in ("triangulate_ms", "robust_ms"):
        if key in runs[-1]:
            ms = [r[key] for r in runs]
            out.update({key: ms, key + "_median": float(np.median(ms)), key + "_min": float(min(ms))})
    return out


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
    ids, kps, poses, lists = synth.triangulation_job(a.images, a.rows, CAM, window=a.rows - 192, step=(a.rows - 192) // 6, long_len=long_len)
    doc = {"tool": "tools/robust_triangulation_bench.py", "images": a.images, "rows_per_image": a.rows, "reps": a.reps, "warmup": a.warmup,
           "bound_robust_over_plain_at_0_percent": BOUND}
    d = np.random.default_rng(1).integers(0, 256, (a.rows, 128), dtype=np.uint8)
    twin_input = None
    with _lib.Context(0) as ctx:
        for k, i in enumerate(ids):
            ctx.upload_image(int(i), d)
            ctx.upload_keypoints(int(i), kps[k])
        ctx.tracks_begin(ids, add_only=True)
        for l in lists:
            ctx.tracks_add(*l)
        ts = ctx.tracks_finish()
        tracks = ctx.tracks()
        T = int(ts["tracks_kept"])
        doc["tracks"] = {k: ts[k] for k in ("tracks_kept", "observations_kept", "longest_track")}
        dev = ctx.device_info()
        doc["device"] = dev["name"].strip() or "gfx950"
        doc["cu_count"] = dev["cu_count"]
        runs = []
        for percent in (0, 1, 10):
            cur = kps
            if percent:
                o = tracks[0]
                every = 100 // percent
                chosen = [(t, (0, int(o[t + 1] - o[t]) // 2, int(o[t + 1] - o[t]) - 1)[n % 3]) for n, t in enumerate(range(0, T, every))]
                cur, _ = synth.corrupt_observations(ids, kps, tracks, chosen)
                for k, i in enumerate(ids):
                    if cur[k] is not kps[k]:
                        ctx.upload_keypoints(int(i), cur[k])
            plain = timed(ctx, poses, a.reps, a.warmup)
            robust = timed(ctx, poses, a.reps, a.warmup, robust=True)
            st = robust["stats"]
            retry_ms = robust["robust_ms_median"] - robust["triangulate_ms_median"]
            r = {"percent_corrupted": percent, "plain": plain, "robust": robust,
                 "robust_over_plain_median": robust["robust_ms_median"] / plain["triangulate_ms_median"],
                 "first_pass_over_plain_median": robust["triangulate_ms_median"] / plain["triangulate_ms_median"],
                 "succeeded_plain": plain["stats"]["succeeded"], "succeeded_robust": st["succeeded"],
                 "retry_ms_median": retry_ms,
                 "retry_us_per_retried_track": 1e3 * retry_ms / st["retried"] if st["retried"] else None,
                 "retry_ns_per_hypothesis": 1e6 * retry_ms / st["hypotheses"] if st["hypotheses"] else None}
            runs.append(r)
            print(json.dumps({k: r[k] for k in r if k not in ("plain", "robust")} | {
                "plain_ms_median": plain["triangulate_ms_median"], "plain_ms_min": plain["triangulate_ms_min"],
                "robust_ms_median": robust["robust_ms_median"], "robust_ms_min": robust["robust_ms_min"],
                "retried": st["retried"], "rescued": st["rescued"], "observations_rejected": st["observations_rejected"]}), flush=True)
            if percent == 10:
                twin_input = cur
        doc["runs"] = runs
        ctx.tracks_end()
    if not a.no_twin:
        import robust_triangulation_twin as rtw
        host = rtw.load_host()
        t0 = time.perf_counter()
        _, _, _, cnt = rtw.run(host, tracks, ids, twin_input, poses, CAM, workers=16)
        doc["host_twin_for_scale_only"] = {"percent_corrupted": 10, "wall_ms_16_threads": (time.perf_counter() - t0) * 1e3, "counts": cnt}
        print(json.dumps(doc["host_twin_for_scale_only"]), flush=True)
    ratio = runs[0]["robust_over_plain_median"]
    doc["acceptance"] = {"ratio": ratio, "bound": BOUND, "passed": bool(ratio <= BOUND)}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    print(json.dumps(doc["acceptance"]), flush=True)
    return 0 if ratio <= BOUND else 1


if __name__ == "__main__":
    sys.exit(main())
