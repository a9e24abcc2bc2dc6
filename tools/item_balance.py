"""How evenly sweep 1's work items keep the workgroups busy: the bench job (config 2) with MSFM_WG_TRACE=1, once with the pipeline off
(MSFM_PIPELINE=1: one sweep-1 launch over the whole job) and once at the default (two halves).

    make -C monocularsfm_amd/csrc trace
    python tools/item_balance.py [--lib path/to/libmsfm_match_trace.so] [--images N] [--calls K] 2>&1 | tee profiles/item_balance_X.txt

The stamps exist in the diagnostic build only (-DMSFM_WG_TRACE: the library that ships reads no clock).  There the integer sweep 1
stamps every workgroup's start and end with the 100 MHz wall clock and the library prints, per launch (stderr, "[msfm wg]"): the event
time, the span first start .. last end, and the workgroups' end times as fractions of the span -- mean, earliest, and the mean per XCD
(workgroup index mod 8).  1 - mean is the drain: the share of the launch's CU time spent idle behind a workgroup's last item."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from monocularsfm_amd import _lib, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(os.path.dirname(_lib.LIB_PATH), "libmsfm_match_trace.so"), help="the diagnostic build")
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--calls", type=int, default=3, help="calls per setting; the last ones are the warm ones")
    args = ap.parse_args()
    _lib.LIB_PATH = args.lib
    imgs, pairs, name = synth.job("south-building", args.images)
    os.environ["MSFM_WG_TRACE"] = "1"
    for pipeline in ("1", None):
        if pipeline:
            os.environ["MSFM_PIPELINE"] = pipeline
        else:
            os.environ.pop("MSFM_PIPELINE", None)
        print("# %s, %d pairs, MSFM_PIPELINE=%s, library %s" % (name, len(pairs), pipeline or "default", _lib.LIB_PATH), flush=True)
        with _lib.Context(0) as ctx:
            for i, im in enumerate(imgs):
                ctx.upload_image(i, im)
            for call in range(args.calls):
                print("# call %d" % call, flush=True)
                sys.stdout.flush()
                ctx.match_pairs(pairs, fetch="view")
                p = ctx.profile()
                print("#   sub-batches %d, sweep 1 %.3f ms, device span %.3f ms" % (p["sub_batches"], p["approx_kernel_ms"], p["total_device_ms"]), flush=True)


if __name__ == "__main__":
    main()
