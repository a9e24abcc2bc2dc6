"""Vocabulary retrieval (matching mode 2) at a given shape: phase times of training and retrieval, the assignment kernel's share of the
dense int8 peak, and optionally the ComputeMatches executable in mode 2 against mode 1 on one synthetic database.

    python tools/retrieval_bench.py --images 1329 --rows 8192 --words 16384 --k 50 --out profiles/retrieval_config4.json
    python tools/retrieval_bench.py --cli-images 256 --cli-rows 2048 --skip-library --out profiles/retrieval_cli.json

Phase times are the library's HIP events (msfm_get_retrieval_profile); the wall times are around calls that return synchronised."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from monocularsfm_amd import _lib, synth  # noqa: E402

PEAK_INT8_OPS = 5.0e15   # dense int8 matrix-core peak of one MI355X, ops/s


def library(args):
    t0 = time.perf_counter()
    imgs = synth.u8_images(args.images, [args.rows] * args.images, seed=1329, as_float=False)
    gen_s = time.perf_counter() - t0
    ids = list(range(args.images))
    res = {"images": args.images, "rows_per_image": args.rows, "words": args.words, "k": args.k, "synth_s": round(gen_s, 2)}
    with _lib.Context(0) as ctx:
        t0 = time.perf_counter()
        for i, x in enumerate(imgs):
            ctx.upload_image(i, x)
        ctx.finalize_store()
        res["upload_s"] = round(time.perf_counter() - t0, 3)
        runs = []
        for rep in range(args.reps):
            t0 = time.perf_counter()
            words = ctx.train_vocabulary(ids, num_words=args.words)
            train_wall = time.perf_counter() - t0
            tp = ctx.retrieval_profile()
            t0 = time.perf_counter()
            pairs, _ = ctx.retrieve_pairs(ids, args.k)
            ret_wall = time.perf_counter() - t0
            p = ctx.retrieval_profile()
            rows = p["rows"]
            ops = 2.0 * 128 * rows * p["num_words"]
            runs.append({
                "train_wall_s": round(train_wall, 4), "train_ms": round(tp["train_ms"], 3), "train_iterations": tp["train_iterations"],
                "retrieve_wall_s": round(ret_wall, 4), "assign_ms": round(p["assign_ms"], 3), "hist_and_scores_ms": round(p["score_ms"], 3),
                "topk_ms": round(p["topk_ms"], 3), "rows": rows, "num_words": p["num_words"], "pairs": int(len(pairs)),
                "assign_int8_ops": ops, "assign_tops": round(ops / (p["assign_ms"] * 1e-3) / 1e12, 1),
                "assign_share_of_5_pops": round(ops / (p["assign_ms"] * 1e-3) / PEAK_INT8_OPS, 3),
            })
            print(json.dumps(runs[-1]), flush=True)
        res["runs"] = runs
        res["vocabulary_rows"] = int(len(words))
    return res


def cli(args):
    exe = os.path.join(ROOT, "monocularsfm_amd", "host", "ComputeMatches")
    subprocess.check_call(["make", "-C", os.path.dirname(exe), "-s"])
    out = {"cli_images": args.cli_images, "cli_rows": args.cli_rows}
    with tempfile.TemporaryDirectory() as d:
        base = os.path.join(d, "base.db")
        synth.u8_database(base, n_images=args.cli_images, n_desc=args.cli_rows)
        for mt in (2, 1):
            db = os.path.join(d, "m%d.db" % mt)
            subprocess.check_call(["cp", base, db])
            cfg = os.path.join(d, "m%d.yaml" % mt)
            with open(cfg, "w") as f:
                f.write('%%YAML:1.0\ndatabase_path : "%s"\nSIFTmatch.match_type : %d\nSIFTmatch.num_nearest_images : %d\n' % (db, mt, args.k))
            t0 = time.perf_counter()
            r = subprocess.run([exe, cfg], capture_output=True, text=True, timeout=args.cli_timeout)
            wall = time.perf_counter() - t0
            if r.returncode != 0:
                raise SystemExit("ComputeMatches mode %d failed: %s" % (mt, r.stderr[-2000:]))
            m = re.search(r"Vocabulary retrieval: .*", r.stdout)
            import sqlite3
            n_rows = sqlite3.connect(db).execute("SELECT COUNT(*) FROM matches").fetchone()[0]
            out["mode%d" % mt] = {"wall_s": round(wall, 3), "rows_written": n_rows, "summary": m.group(0) if m else None}
            print(json.dumps(out["mode%d" % mt]), flush=True)
    out["speedup_mode2_over_mode1"] = round(out["mode1"]["wall_s"] / out["mode2"]["wall_s"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1329)
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--words", type=int, default=16384)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--skip-library", action="store_true")
    ap.add_argument("--cli-images", type=int, default=0)
    ap.add_argument("--cli-rows", type=int, default=2048)
    ap.add_argument("--cli-timeout", type=int, default=900)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    res = {}
    if not args.skip_library:
        res["library"] = library(args)
    if args.cli_images:
        res["cli"] = cli(args)
    with _lib.Context(0) as ctx:
        res["device"] = ctx.device_info()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
