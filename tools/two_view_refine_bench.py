"""Device time of the two-view pose refinement (msfm_set_two_view_refinement) behind the two-view geometry
under the essential-matrix verification (model 1), refinement off against on in one process, on the two workloads of
tools/two_view_geometry_bench.py:

    e2e      the end_to_end job's database contents (128 images x ~5000 float32 descriptors, a 3-D box)
    config4  the config-4-shaped byte images, --images of them (default 256), all pairs

    python tools/two_view_refine_bench.py [--workload e2e|config4|all] [--images 256] [--rows off,on]
                                          [--out profiles/two_view_refine_bench.json]

Per workload one context holds the images, the two-view geometry is on in both rows; per row an untimed warm-up call, then one timed
msfm_match_pairs_verified.  Rows: verify_ms, total_device_ms, matches kept, valid records; with the refinement on also the eligible
and refined pairs, the evaluated steps and how the loops ended.  Prints one JSON object and writes it to --out."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

from monocularsfm_amd import _lib, synth  # noqa: E402
from verify_e_bench import CAMERA, config4_data, e2e_data  # noqa: E402

ROWS = (("off", False), ("on", True))


def run(descs, kps, max_distance, rows=ROWS):
    out = []
    with _lib.Context(0) as ctx:
        for i, (d, k) in enumerate(zip(descs, kps)):
            ctx.upload_image(i, d)
            ctx.upload_keypoints(i, k)
        pairs = synth.all_pairs(len(descs))
        ctx.set_verification_model(1, CAMERA)
        ctx.set_two_view_geometry(True)
        for name, on in rows:
            ctx.set_two_view_refinement(on)
            ctx.match_pairs_verified(pairs, max_distance=max_distance, fetch=False)   # warm-up: buffers, plan hints
            t0 = time.perf_counter()
            offs, _, _ = ctx.match_pairs_verified(pairs, max_distance=max_distance, fetch=False)
            wall = time.perf_counter() - t0
            prof = ctx.profile()
            rec = ctx.two_view_geometry(len(pairs))
            valid = rec["valid"] == 1
            row = {"row": name, "two_view_refinement": on, "pairs": int(len(pairs)), "wall_s": wall,
                   "total_device_ms": prof["total_device_ms"], "verify_ms": prof["verify_ms"], "matches_kept": int(offs[-1]),
                   "sub_batches": prof["sub_batches"], "valid_records": int(valid.sum()),
                   "initial_candidates": int(rec["is_initial_candidate"].sum()),
                   "kept_per_valid_pair": float(rec["n_kept"][valid].mean()) if valid.any() else 0.0,
                   "mean_residual_px": float(rec["mean_residual"][valid].mean()) if valid.any() else 0.0}
            if on:
                rf = ctx.two_view_refinements(len(pairs))
                el = (rf["status"] & _lib.TVR_ELIGIBLE) != 0
                row.update(eligible=int(el.sum()), refined=int(_lib.two_view_refined(rf).sum()), steps=int(rf["steps"].sum()),
                           accepted=int(rf["accepted"].sum()), stops=np.bincount(rf["stop"][el], minlength=4).tolist(),
                           cost_before=float(rf["cost_before"].sum()), cost_after=float(rf["cost_after"].sum()))
            out.append(row)
        ctx.set_two_view_refinement(False)
    if len(out) == 2:
        out[1]["verify_ms_over_off"] = out[1]["verify_ms"] / max(1e-9, out[0]["verify_ms"])
        out[1]["total_device_ms_over_off"] = out[1]["total_device_ms"] / max(1e-9, out[0]["total_device_ms"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="all", choices=["e2e", "config4", "all"])
    ap.add_argument("--images", type=int, default=256, help="config4: images of the subset")
    ap.add_argument("--rows", default="off,on", help="which of off, on to run (a kernel trace of one of them)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = [r for r in ROWS if r[0] in a.rows.split(",")]
    res = {}
    for w in (["e2e", "config4"] if a.workload == "all" else [a.workload]):
        descs, kps = e2e_data() if w == "e2e" else config4_data(a.images)
        res[w] = run(descs, kps, 1e9 if w == "config4" else 0.7, rows)
        print(json.dumps({w: res[w]}), file=sys.stderr, flush=True)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
