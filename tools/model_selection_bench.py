"""Device time and outcome of the two-view model selection (msfm_set_model_selection) against the fundamental
matrix (model 0) and the homography (model 2) alone, in one process, on four workloads:

    e2e      the end_to_end job's database contents (tools/verify_e_bench.py: 128 images x ~5000 float32 descriptors, a 3-D box)
    planar   the same descriptors with the keypoints of one facade (synth.south_building_planar)
    mixed    synth.mixed_capture: 64 facade images and 64 images of a 3-D scene, cross pairs sharing no point
    config4  the config-4-shaped byte images (tools/verify_e_bench.py), --images of them (default 256), all pairs

    python tools/model_selection_bench.py [--workload e2e|planar|mixed|config4|all] [--images 256] [--rows F,H,select]
                                          [--out profiles/model_selection_bench.json]

Per workload one context holds the images; per row (model 0, model 2, the selection under model 0) an untimed warm-up call, then one
timed msfm_match_pairs_verified.  Rows: verify_ms, total_device_ms, matches kept, pairs that kept the homography's list.  Prints one
JSON object and writes it to --out."""
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

ROWS = (("F", 0, False), ("H", 2, False), ("select", 0, True))


def run(descs, kps, max_distance, rows=ROWS):
    out = []
    with _lib.Context(0) as ctx:
        for i, (d, k) in enumerate(zip(descs, kps)):
            ctx.upload_image(i, d)
            ctx.upload_keypoints(i, k)
        pairs = synth.all_pairs(len(descs))
        raw = ctx.match_pairs(pairs, max_distance=max_distance, fetch=False)[0]
        for name, model, select in rows:
            ctx.set_verification_model(model)
            ctx.set_model_selection(select)
            ctx.match_pairs_verified(pairs, max_distance=max_distance, fetch=False)   # warm-up: buffers, plan hints
            t0 = time.perf_counter()
            offs, _, _ = ctx.match_pairs_verified(pairs, max_distance=max_distance, fetch=False)
            wall = time.perf_counter() - t0
            prof = ctx.profile()
            solved, rounds = ctx.verification_stats()
            row = {"row": name, "model": model, "selection": select, "pairs": int(len(pairs)), "wall_s": wall,
                   "total_device_ms": prof["total_device_ms"], "verify_ms": prof["verify_ms"], "matches_in": int(raw[-1]),
                   "matches_kept": int(offs[-1]), "hypotheses_solved_staged": solved, "max_rounds": rounds}
            if select:
                m, ne, nh = ctx.model_selection(len(pairs))
                row.update(pairs_took_h=int((m == 2).sum()), matches_kept_by_f_of_those=int(ne[m == 2].sum()))
            else:
                row.update(pairs_took_h=int((np.diff(raw) >= 4).sum()) if model == 2 else 0)
            out.append(row)
        ctx.set_model_selection(False)
    if len(out) == 3:
        f, h, s = out
        s["verify_ms_over_f_plus_h"] = s["verify_ms"] / max(1e-9, f["verify_ms"] + h["verify_ms"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="all", choices=["e2e", "planar", "mixed", "config4", "all"])
    ap.add_argument("--images", type=int, default=256, help="config4: images of the subset")
    ap.add_argument("--rows", default="F,H,select", help="which of F, H, select to run (a kernel trace of one of them)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = [r for r in ROWS if r[0] in a.rows.split(",")]
    res = {}
    for w in (["e2e", "planar", "mixed", "config4"] if a.workload == "all" else [a.workload]):
        if w == "e2e":
            descs, kps = e2e_data()
        elif w == "planar":
            descs, kps = synth.south_building_planar()
        elif w == "mixed":
            descs, kps, _ = synth.mixed_capture()
        else:
            descs, kps = config4_data(a.images)
        res[w] = run(descs, kps, 1e9 if w == "config4" else 0.7, rows)
        print(json.dumps({w: res[w]}), file=sys.stderr, flush=True)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
