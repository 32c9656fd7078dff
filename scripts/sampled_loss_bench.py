"""Forward + backward of the three sampled ranking losses at the BASELINE fit shape, in one process: sampled softmax and BPR
(csrc/loss_sampled.hip) and, as the yardstick, WMRB (trec_wmrb_fwd + trec_wmrb_bwd, csrc/loss.hip).

Shape: 1,000,000 users, about 20 positive interactions each (Poisson, at least 1), S = 100 sampled predictions per user, 2,700,000 items
for WMRB's n_items / S ratio; predictions, samples and the upstream gradient are seeded random numbers (synthetic: no model is fitted).
The [n_users, S] arrays are 400 MB each, beyond the 256 MB Infinity Cache.

Method: every call is warmed up, then the three losses are timed in turn, round after round, each forward + backward pair between two
device events on the current stream; the record holds the median, the minimum and the maximum of the rounds per loss.  Times are call
times (kernels + launch), not kernel times from a trace.

    python scripts/sampled_loss_bench.py --out profiles/sampled_losses.json [--users 1000000 --samples 100 --rounds 20]
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
    ap.add_argument("--temperature", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=20)
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
    row_max, row_sum = torch.empty(nu, device="cuda"), torch.empty(nu, device="cuda")
    d_pred, d_samp = torch.empty_like(pred), torch.empty_like(samp)
    p = N.ptr
    inv_t = 1.0 / args.temperature

    def softmax():
        N.call("trec_sampled_softmax_fwd", p(indptr), p(pos_slot), p(pred), p(samp), nu, S, inv_t, p(loss), p(row_max), p(row_sum))
        N.call("trec_sampled_softmax_bwd", p(indptr), p(pos_slot), p(pred), p(samp), p(row_max), p(row_sum), p(go), nu, S, inv_t,
               p(d_pred), p(d_samp))

    def bpr():
        N.call("trec_bpr_fwd", p(indptr), p(pos_slot), p(pred), p(samp), nu, S, p(loss))
        N.call("trec_bpr_bwd", p(indptr), p(pos_slot), p(pred), p(samp), p(go), nu, S, p(d_pred), p(d_samp))

    def wmrb():
        N.call("trec_wmrb_fwd", p(indptr), p(pos_slot), None, p(pred), p(samp), nu, args.items, S, p(loss), p(aux))
        N.call("trec_wmrb_bwd", p(indptr), p(pos_slot), None, p(pred), p(samp), p(aux), p(go), nu, args.items, S, p(d_pred), p(d_samp))

    calls = [("sampled_softmax", softmax), ("bpr", bpr), ("wmrb", wmrb)]
    for _ in range(args.warmup):
        for _, fn in calls:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in calls}
    for _ in range(args.rounds):
        for name, fn in calls:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b))
    # bytes the algorithm needs per forward + backward: the samples read twice and their gradient written once, the predictions read
    # twice, their gradient and the loss written once, go read once, indptr and pos_slot read twice
    need = 3 * nu * S * 4 + 5 * P * 4 + 2 * (nu * 8 + P * 4)
    rec = {"what": "forward + backward call time of the sampled ranking losses at the BASELINE fit shape, one process, losses timed in "
                   "turn per round between device events (scripts/sampled_loss_bench.py); synthetic predictions",
           "device": torch.cuda.get_device_name(0), "commit": commit(), "clocks": box_clocks,
           "shape": {"n_users": nu, "n_interactions": P, "n_sampled": S, "n_items_for_wmrb_ratio": args.items,
                     "temperature": args.temperature},
           "rounds": args.rounds, "warmup": args.warmup, "bytes_needed_per_call_pair": need, "ms": {}}
    for name, _ in calls:
        t = np.array(times[name])
        rec["ms"][name] = {"median": float("%.4g" % np.median(t)), "min": float("%.4g" % t.min()), "max": float("%.4g" % t.max()),
                           "needed_bytes_over_median_GBps": float("%.4g" % (need / np.median(t) / 1e6))}
    line = json.dumps(rec, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
