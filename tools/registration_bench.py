#!/usr/bin/env python
"""Image registration at the production shape: synth.triangulation_job, 1329 images x 8192 keypoints, triangulated
under its poses (every 50th image unposed), then (a) the unposed images and (b) all images registered in one call each.  Reports
register_ms (the library's HIP events around the launches; median, minimum and all of --reps warm calls behind --warmup untimed ones),
the correspondences, the hypotheses solved and the rounds.  If the unposed images have no correspondences with succeeded tracks the
tool says so and (a) carries no time.  Beside it, for scale only, the host twin's time on 16 threads.

    python tools/registration_bench.py --out profiles/registration_bench.json [--images 1329] [--rows 8192] [--reps 7] [--warmup 2]
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


def timed(ctx, image_ids, reps, warmup):
    for _ in range(warmup):
        ctx.register_images(CAM, image_ids)
    ms, st = [], None
    for _ in range(reps):
        st = ctx.register_images(CAM, image_ids)
        ms.append(st["register_ms"])
    return {"images": len(image_ids), "register_ms": ms, "register_ms_median": float(np.median(ms)), "register_ms_min": float(min(ms)), "stats": st}


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
    unposed = [int(i) for i in ids if int(i) not in poses or poses[int(i)] is None]
    doc = {"tool": "tools/registration_bench.py", "images": a.images, "rows_per_image": a.rows, "reps": a.reps, "warmup": a.warmup,
           "unposed_images": len(unposed)}
    d = np.random.default_rng(1).integers(0, 256, (a.rows, 128), dtype=np.uint8)
    with _lib.Context(0) as ctx:
        for k, i in enumerate(ids):
            ctx.upload_image(int(i), d)
            ctx.upload_keypoints(int(i), kps[k])
        ctx.tracks_begin(ids, add_only=True)
        for l in lists:
            ctx.tracks_add(*l)
        ctx.tracks_finish()
        ts = ctx.triangulate_tracks(CAM, poses)
        doc["triangulation"] = {k: ts[k] for k in ("tracks", "succeeded", "triangulate_ms")}
        dev = ctx.device_info()
        doc["device"] = dev["name"].strip() or "gfx950"
        doc["cu_count"] = dev["cu_count"]
        runs = {}
        for name, lst in (("unposed", unposed), ("all", [int(i) for i in ids])):
            r = timed(ctx, lst, a.reps, a.warmup)
            if r["stats"]["correspondences"] == 0:
                r["note"] = "these images have no observations on succeeded tracks: nothing to time"
            runs[name] = r
            print(json.dumps({"run": name, "register_ms_median": r["register_ms_median"], "register_ms_min": r["register_ms_min"],
                              **{k: r["stats"][k] for k in ("attempted", "succeeded", "correspondences", "hypotheses", "rounds")}}), flush=True)
        doc["runs"] = runs
        tracks, points = ctx.tracks(), ctx.points3d()[0]
        ctx.tracks_end()
    if not a.no_twin:
        import registration_twin as tw
        host = tw.load_host()
        kp = {int(i): k for i, k in zip(ids, kps)}
        t0 = time.perf_counter()
        rec = tw.run(host, tracks, points, [int(i) for i in ids], kp, CAM, workers=16)[0]
        doc["host_twin_for_scale_only"] = {"run": "all", "wall_ms_16_threads": (time.perf_counter() - t0) * 1e3,
                                           "succeeded": int(_lib.registered(rec).sum())}
        print(json.dumps(doc["host_twin_for_scale_only"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
