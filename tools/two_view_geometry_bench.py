"""Device time of the two-view geometry (msfm_set_two_view_geometry) under the essential-matrix
verification (model 1), feature off against on in one process, on the section-10 workloads:

    e2e      the end_to_end job's database contents (tools/verify_e_bench.py: 128 images x ~5000 float32 descriptors, a 3-D box)
    config4  the config-4-shaped byte images (tools/verify_e_bench.py), --images of them (default 256), all pairs

    python tools/two_view_geometry_bench.py [--workload e2e|config4|all] [--images 256] [--rows off,on]
                                            [--out profiles/two_view_geometry_bench.json]

Per workload one context holds the images; per row an untimed warm-up call, then one timed msfm_match_pairs_verified.  Rows:
verify_ms, total_device_ms, matches kept; with the feature on also the valid records, the initial candidates and the kept matches
per valid pair.  Prints one JSON object and writes it to --out."""
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
        for name, on in rows:
            ctx.set_two_view_geometry(on)
            ctx.match_pairs_verified(pairs, max_distance=max_distance, fetch=False)   # warm-up: buffers, plan hints
            t0 = time.perf_counter()
            offs, _, _ = ctx.match_pairs_verified(pairs, max_distance=max_distance, fetch=False)
            wall = time.perf_counter() - t0
            prof = ctx.profile()
            solved, rounds = ctx.verification_stats()
            row = {"row": name, "two_view_geometry": on, "pairs": int(len(pairs)), "wall_s": wall,
                   "total_device_ms": prof["total_device_ms"], "verify_ms": prof["verify_ms"], "matches_kept": int(offs[-1]),
                   "hypotheses_solved_staged": solved, "max_rounds": rounds, "sub_batches": prof["sub_batches"]}
            if on:
                rec = ctx.two_view_geometry(len(pairs))
                valid = rec["valid"] == 1
                row.update(valid_records=int(valid.sum()), initial_candidates=int(rec["is_initial_candidate"].sum()),
                           kept_per_valid_pair=float(rec["n_kept"][valid].mean()) if valid.any() else 0.0,
                           largest_n_kept=int(rec["n_kept"].max()), records_equal_list_lengths=bool(
                               np.array_equal(rec["n_kept"][valid], np.diff(offs)[valid])))
            out.append(row)
        ctx.set_two_view_geometry(False)
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
