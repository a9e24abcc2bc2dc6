"""CPU model (float64) of the candidate thresholds of sweep 2 on a job shaped like the bench workload: what the reverse direction
collects under today's bound -- the upper bound U1 of the SECOND distance -- and under the ratio cap min(U1, U0 / ratio)
(csrc/msfm_hostutil.h: msfm_ratio_cap_*; U0: the upper bound of the best distance).

    python tools/ratio_cap_study.py [--images 6] [--pairs 8] [--ratio 0.8] [--max-distance 0.7]

Per direction of every pair: rows that are not provably dead (L0 < ratio U1 and L0 <= max_distance, with the twins' slack
e_q + E_2 ~ 2 x 0.0056 on both bounds), the candidates a live row collects (elements within the bound + the fp16 sweep's eps, ~0.003
in distance terms), and for the reverse direction the density of the block masks (512-row blocks of image 1 whose nearest row lies
within the bound).  The model has no roundings and one slack for every row: it reproduces the measured figures to ~10 %
(live rows 0.060-0.062, 4.9 candidates per live row, mask density 0.50 on the 128-image job), which is what it is for."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from monocularsfm_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=6)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--ratio", type=float, default=0.8)
    ap.add_argument("--max-distance", type=float, default=0.7)
    ap.add_argument("--seed", type=int, default=1234)
    args = ap.parse_args()
    imgs, pairs, name = synth.job("south-building", args.images, None, seed=args.seed)
    ratio, maxd = args.ratio, args.max_distance
    slack, eps_d = 2 * 0.0056, 0.003
    tot = dict(rows=0, live=0, c_now=0, c_cap=0, m_now=0, m_cap=0, blocks=0, rev_live=0)
    for (i, j) in pairs[:args.pairs]:
        A, B = imgs[i].astype(np.float64), imgs[j].astype(np.float64)
        S = (A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2 * A @ B.T
        D = np.sqrt(np.maximum(S, 0))
        for rev, M in ((0, D), (1, D.T)):
            part = np.partition(M, 1, axis=1)
            d0, d1 = part[:, 0], part[:, 1]
            L0, U0, U1 = np.maximum(d0 - slack, 0), d0 + slack, d1 + slack
            live = ~((L0 >= ratio * U1) | (L0 > maxd))
            cap = np.minimum(U1, U0 / ratio)
            Ml = M[live]
            tot["rows"] += len(d0)
            tot["live"] += int(live.sum())
            tot["c_now"] += int((Ml <= (U1 + eps_d)[live, None]).sum())
            tot["c_cap"] += int((Ml <= (cap + eps_d)[live, None]).sum())
            if rev:
                nb = (M.shape[1] + 511) // 512
                lower = np.maximum(np.stack([Ml[:, p * 512:(p + 1) * 512].min(1) for p in range(nb)], 1) - slack, 0)
                tot["m_now"] += int((lower <= U1[live, None]).sum())
                tot["m_cap"] += int((lower <= cap[live, None]).sum())
                tot["blocks"] += int(live.sum()) * nb
                tot["rev_live"] += int(live.sum())
    print("# %s, first %d pairs, ratio %g, max_distance %g" % (name, min(args.pairs, len(pairs)), ratio, maxd))
    print("live rows / columns:            %.3f of %d" % (tot["live"] / tot["rows"], tot["rows"]))
    print("candidates per live row:        bound U1 %.2f    bound min(U1, U0 / ratio) %.2f" % (tot["c_now"] / tot["live"], tot["c_cap"] / tot["live"]))
    print("reverse block-mask density:     bound U1 %.3f   bound min(U1, U0 / ratio) %.3f" % (tot["m_now"] / tot["blocks"], tot["m_cap"] / tot["blocks"]))
    print("blocks per live column:         bound U1 %.2f    bound min(U1, U0 / ratio) %.2f" % (tot["m_now"] / tot["rev_live"], tot["m_cap"] / tot["rev_live"]))


if __name__ == "__main__":
    main()
