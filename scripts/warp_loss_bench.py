"""Forward + backward of WARP (csrc/loss_warp.hip) next to WMRB (csrc/loss.hip) and BPR (csrc/loss_sampled.hip) at the BASELINE fit
shape, in one process: the method of scripts/sampled_loss_bench.py.

Shape: 1,000,000 users, about 20 positive interactions each (Poisson, at least 1), S = 100 sampled predictions per user, 2,700,000
items (WARP's rank weight, WMRB's n_items / S ratio); predictions, samples and the upstream gradient are seeded random numbers
(synthetic: no model is fitted -- with N(0, 1) predictions three in four trials violate, so a WARP scan stops within the first few
samples; a fitted model's scans run longer).  The [n_users, S] arrays are 400 MB each, beyond the 256 MB Infinity Cache.

Method: every call is warmed up, then WARP, WMRB and BPR are timed in turn, round after round, each forward + backward pair between
two device events on the current stream; the record holds the median, the minimum and the maximum of the rounds per loss.  Times are
call times (kernels + launch), not kernel times from a trace.

    python scripts/warp_loss_bench.py --out profiles/warp_loss.json [--users 1000000 --samples 100 --rounds 20]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tensorrec_amd import _native as N  # noqa: E402


def clocks():
    """what the box reports about its clocks (read-only query; None if the tool is missing)"""
    try:
        return subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=60).stdout.strip() or None
    except Exception:
        return None


def commit():
    try:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        return subprocess.run(["git", "-C", root, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, timeout=60).stdout.strip() or None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--positives", type=float, default=20.0)
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--items", type=int, default=2_700_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--commit", default=None, help="the commit to record (default: asked of git; for a tree without its .git)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    box_clocks = clocks()                                     # (a child process, before this one opens the GPU)
    N.require_gpu()
    N.load()
    rng = np.random.default_rng(0)
    nu, S = args.users, args.samples
    counts = np.maximum(rng.poisson(args.positives, nu), 1)
    indptr_h = np.zeros(nu + 1, np.int64)
    np.cumsum(counts, out=indptr_h[1:])
    P = int(indptr_h[-1])
    indptr = torch.from_numpy(indptr_h).cuda()
    pos_slot = torch.arange(P, dtype=torch.int32, device="cuda")          # every interaction is a positive
    gen = torch.Generator(device="cuda").manual_seed(0)
    pred = torch.randn(P, device="cuda", generator=gen)
    samp = torch.randn(nu, S, device="cuda", generator=gen)
    go = torch.rand(P, device="cuda", generator=gen) + 0.5
    loss, aux = torch.empty(P, device="cuda"), torch.empty(P, device="cuda")
    first = torch.empty(P, dtype=torch.int32, device="cuda")
    d_pred, d_samp = torch.empty_like(pred), torch.empty_like(samp)
    p = N.ptr

    def warp():
        N.call("trec_warp_fwd", p(indptr), None, p(pos_slot), p(pred), p(samp), None, nu, args.items, S, 0, p(loss), p(first), p(aux))
        N.call("trec_warp_bwd", p(indptr), p(pos_slot), p(first), p(aux), p(go), nu, S, p(d_pred), p(d_samp))

    def wmrb():
        N.call("trec_wmrb_fwd", p(indptr), p(pos_slot), None, p(pred), p(samp), nu, args.items, S, p(loss), p(aux))
        N.call("trec_wmrb_bwd", p(indptr), p(pos_slot), None, p(pred), p(samp), p(aux), p(go), nu, args.items, S, p(d_pred), p(d_samp))

    def bpr():
        N.call("trec_bpr_fwd", p(indptr), p(pos_slot), p(pred), p(samp), nu, S, p(loss))
        N.call("trec_bpr_bwd", p(indptr), p(pos_slot), p(pred), p(samp), p(go), nu, S, p(d_pred), p(d_samp))

    calls = [("warp", warp), ("wmrb", wmrb), ("bpr", bpr)]
    for _ in range(args.warmup):
        for _, fn in calls:
            fn()
    torch.cuda.synchronize()
    warp()
    torch.cuda.synchronize()
    stopped = first >= 0
    scan = {"positives_with_a_violator": float("%.4g" % stopped.float().mean().item()),
            "mean_first": float("%.4g" % first[stopped].float().mean().item()), "max_first": int(first.max().item())}
    times = {name: [] for name, _ in calls}
    for _ in range(args.rounds):
        for name, fn in calls:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b))
    # bytes the algorithm needs per forward + backward.  WMRB and BPR: the samples read twice and their gradient written once, the
    # predictions read twice, their gradient and the loss written once, go read once, indptr and pos_slot read twice.  WARP: the samples
    # read ONCE (the backward pass reads no prediction) and their gradient written once, the predictions read once, first and weight
    # written and read, the loss and d pred written, go read, indptr and pos_slot read twice.
    need = {"wmrb": 3 * nu * S * 4 + 5 * P * 4 + 2 * (nu * 8 + P * 4), "warp": 2 * nu * S * 4 + 8 * P * 4 + 2 * (nu * 8 + P * 4)}
    need["bpr"] = need["wmrb"]
    rec = {"what": "forward + backward call time of WARP, WMRB and BPR at the BASELINE fit shape, one process, losses timed in turn per "
                   "round between device events (scripts/warp_loss_bench.py); synthetic N(0, 1) predictions",
           "device": torch.cuda.get_device_name(0), "commit": args.commit or commit(), "clocks": box_clocks,
           "shape": {"n_users": nu, "n_interactions": P, "n_sampled": S, "n_items": args.items},
           "warp_scan": scan, "rounds": args.rounds, "warmup": args.warmup, "bytes_needed_per_call_pair": need, "ms": {}}
    for name, _ in calls:
        t = np.array(times[name])
        rec["ms"][name] = {"median": float("%.4g" % np.median(t)), "min": float("%.4g" % t.min()), "max": float("%.4g" % t.max()),
                           "needed_bytes_over_median_GBps": float("%.4g" % (need[name] / np.median(t) / 1e6))}
    w, m = rec["ms"]["warp"], rec["ms"]["wmrb"]
    rec["warp_below_wmrb_ranges_apart"] = bool(w["median"] < m["median"] and w["max"] < m["min"])
    line = json.dumps(rec, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
