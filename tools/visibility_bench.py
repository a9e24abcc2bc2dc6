#!/usr/bin/env python
"""Map visibility at production-like shapes: synth.triangulation_job with a few hundred images, folded from
synthetic lists through tracks_add (no matching), robustly triangulated (so the session has inlier bytes).  Per shape (one per entry
of --rows) and per query -- none, one image, every image -- msfm_map_visibility's visibility_ms (HIP events around its launches) and
the call's wall time under MSFM_VIS_ROUTE_GLOBAL and MSFM_VIS_ROUTE_LDS forced and under AUTO: --warmup untimed calls, then the median
(minimum) of --reps.  Beside them the wall time of the host route the call replaces: the tracks() + points3d() + point_inliers() +
pose_list() fetches plus tests/visibility_ref.py's numpy counting on the same data (the query = none and query = one forms; its
full matrix is the same product).  One process, one context.  Not a pass criterion: nothing earlier exists to compare with.

    python tools/visibility_bench.py --out profiles/visibility_bench.json [--images 300] [--rows 64,256,2048]
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
import visibility_ref as vref  # noqa: E402

CAM = (2500.0, 2500.0, 1536.0, 1152.0)


def timed(ctx, query, route, warmup, reps):
    ms, wall, st = [], [], None
    for k in range(warmup + reps):
        t0 = time.perf_counter()
        _, _, st = ctx.visibility(query, "map", route)
        t1 = time.perf_counter()
        if k >= warmup:
            ms.append(st["visibility_ms"])
            wall.append((t1 - t0) * 1e3)
    return {"visibility_ms_median": float(np.median(ms)), "visibility_ms_min": float(min(ms)), "wall_ms_median": float(np.median(wall)),
            "route_ran": st["route"], "device_bytes": st["device_bytes"], "pair_increments": st["pair_increments"]}


def host_route(ctx, ids, query, reps):
    fetch, count = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        tracks = ctx.tracks()
        pts, _ = ctx.points3d()
        mask = ctx.point_inliers()
        lst = ctx.pose_list()
        t1 = time.perf_counter()
        vref.run(tracks, ids, lst, pts, mask, query)
        t2 = time.perf_counter()
        fetch.append((t1 - t0) * 1e3)
        count.append((t2 - t1) * 1e3)
    return {"fetch_ms_median": float(np.median(fetch)), "numpy_ms_median": float(np.median(count)),
            "wall_ms_median": float(np.median(np.add(fetch, count)))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=300)
    ap.add_argument("--rows", default="64,256,2048")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    doc = {"tool": "tools/visibility_bench.py", "images": a.images, "reps": a.reps, "warmup": a.warmup, "shapes": []}
    with _lib.Context(0) as ctx:
        dev = ctx.device_info()
        doc["device"], doc["cu_count"] = dev["name"].strip() or "gfx950", dev["cu_count"]
        for rows in [int(r) for r in a.rows.split(",")]:
            window = rows - 8
            ids, kps, poses, lists = synth.triangulation_job(a.images, rows, CAM, window=window, step=max(window // 6, 1), n_long=8,
                                                             long_len=min(300, (a.images - 2) // 3))
            d = np.random.default_rng(1).integers(0, 256, (rows, 128), dtype=np.uint8)
            ctx.clear_images()
            for k, i in enumerate(ids):
                ctx.upload_image(int(i), d)
                ctx.upload_keypoints(int(i), kps[k])
            ctx.tracks_begin(ids, add_only=True)
            for l in lists:
                ctx.tracks_add(*l)
            ts = ctx.tracks_finish()
            tri = ctx.triangulate_tracks(CAM, poses, robust=True, max_hypotheses=16)
            ids = [int(i) for i in ids]
            shape = {"rows_per_image": rows, "tracks": {k: ts[k] for k in ("tracks_kept", "observations_kept", "longest_track")},
                     "succeeded": tri["succeeded"], "queries": {}}
            for name, query in (("none", []), ("one", ids[len(ids) // 2:len(ids) // 2 + 1]), ("all", ids)):
                q = {route: timed(ctx, query, route, a.warmup, a.reps) for route in ("global", "lds", "auto")}
                if name != "all":
                    q["host"] = host_route(ctx, ids, query, max(a.reps // 3, 1))
                shape["queries"][name] = q
                print(json.dumps({"rows": rows, "O": ts["observations_kept"], "query": name,
                                  **{r: round(q[r]["visibility_ms_median"], 4) for r in ("global", "lds", "auto")},
                                  "auto_ran": q["auto"]["route_ran"], "call_wall_ms": round(q["auto"]["wall_ms_median"], 3),
                                  "host_wall_ms": round(q["host"]["wall_ms_median"], 3) if "host" in q else None}), flush=True)
            doc["shapes"].append(shape)
            ctx.tracks_end()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
