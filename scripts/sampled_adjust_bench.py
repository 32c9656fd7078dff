"""Forward + backward of the sampled softmax and BPR with and without the adjustments (accidental hits removed, logQ correction), and the
alias sampler against K7, at the BASELINE fit shape, in one process (csrc/loss_sampled.hip, csrc/sampler_alias.hip).

Shape: 1,000,000 users, about 20 positive interactions each (Poisson, at least 1; items drawn from a Zipf(1) popularity over 1,000,000
items, duplicates within a user removed), S = 100 samples per user drawn by the alias sampler from count ** 0.75, so accidental hits
occur at the rate such a fit would see.  Predictions and the upstream gradient are seeded random numbers (synthetic: no model is fitted).

Method: every call is warmed up, then the variants are timed in turn, round after round, each between two device events on the current
stream; the record holds the median, the minimum and the maximum of the rounds per variant.  Times are call times (kernels + launch), not
kernel times from a trace.
    a  trec_sampled_softmax_fwd + _bwd (the plain entry points)      b  trec_sampled_softmax_adj_fwd + _bwd, both options, log_q table
    c  trec_bpr_fwd + _bwd                                           d  trec_bpr_adj_fwd + _bwd, hits removed
    e  trec_sample_items_alias                                       f  trec_sample_items, replace = 0 (K7's keyed kernel)

    python scripts/sampled_adjust_bench.py --out profiles/sampled_adjust.json [--users 1000000 --samples 100 --rounds 20]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tensorrec_amd import _native as N, PopularitySampler  # noqa: E402
from sampled_loss_bench import clocks, commit  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--positives", type=float, default=20.0)
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--temperature", type=float, default=0.5)
    ap.add_argument("--power", type=float, default=0.75)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    box_clocks = clocks()                                     # (a child process, before this one opens the GPU)
    N.require_gpu()
    N.load()
    rng = np.random.default_rng(0)
    nu, S, ni = args.users, args.samples, args.items
    counts = np.maximum(rng.poisson(args.positives, nu), 1)
    zipf = 1.0 / np.arange(1, ni + 1)
    cdf = np.cumsum(zipf / zipf.sum())
    cols = np.minimum(np.searchsorted(cdf, rng.random(int(counts.sum()))), ni - 1).astype(np.int64)
    key = np.unique(np.repeat(np.arange(nu, dtype=np.int64), counts) * ni + cols)          # sorted by (user, item), duplicates removed
    rows, cols = key // ni, (key % ni).astype(np.int32)
    indptr_h = np.zeros(nu + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=nu), out=indptr_h[1:])
    P = int(indptr_h[-1])
    item_counts = np.bincount(cols, minlength=ni)
    sampler = PopularitySampler(item_counts, power=args.power, seed=1)
    indptr, x_item = torch.from_numpy(indptr_h).cuda(), torch.from_numpy(cols).cuda()
    pos_slot = torch.arange(P, dtype=torch.int32, device="cuda")          # every interaction is a positive
    samples = sampler.sample(ni, nu, S, True, 1, "cuda")
    log_q = sampler.log_q("cuda")
    thr, alias, _ = sampler._on("cuda")
    gen = torch.Generator(device="cuda").manual_seed(0)
    pred = torch.randn(P, device="cuda", generator=gen)
    samp = torch.randn(nu, S, device="cuda", generator=gen)
    go = torch.rand(P, device="cuda", generator=gen) + 0.5
    loss = torch.empty(P, device="cuda")
    rows3 = torch.empty(3, nu, device="cuda")
    d_pred, d_samp = torch.empty_like(pred), torch.empty_like(samp)
    out_ids = torch.empty_like(samples)
    p = N.ptr
    inv_t = 1.0 / args.temperature
    r0, r1, r2 = rows3[0], rows3[1], rows3[2]

    def softmax():
        N.call("trec_sampled_softmax_fwd", p(indptr), p(pos_slot), p(pred), p(samp), nu, S, inv_t, p(loss), p(r1), p(r2))
        N.call("trec_sampled_softmax_bwd", p(indptr), p(pos_slot), p(pred), p(samp), p(r1), p(r2), p(go), nu, S, inv_t, p(d_pred), p(d_samp))

    def softmax_adj():
        N.call("trec_sampled_softmax_adj_fwd", p(indptr), p(x_item), p(pos_slot), p(pred), p(samp), p(samples), p(log_q), 0.0, nu, ni, S,
               inv_t, 1, 1, p(loss), p(r0), p(r1), p(r2))
        N.call("trec_sampled_softmax_adj_bwd", p(indptr), p(x_item), p(pos_slot), p(pred), p(samp), p(samples), p(log_q), 0.0, p(r0), p(r1),
               p(r2), p(go), nu, ni, S, inv_t, 1, 1, p(d_pred), p(d_samp))

    def bpr():
        N.call("trec_bpr_fwd", p(indptr), p(pos_slot), p(pred), p(samp), nu, S, p(loss))
        N.call("trec_bpr_bwd", p(indptr), p(pos_slot), p(pred), p(samp), p(go), nu, S, p(d_pred), p(d_samp))

    def bpr_adj():
        N.call("trec_bpr_adj_fwd", p(indptr), p(x_item), p(pos_slot), p(pred), p(samp), p(samples), nu, S, 1, p(loss))
        N.call("trec_bpr_adj_bwd", p(indptr), p(x_item), p(pos_slot), p(pred), p(samp), p(samples), p(go), nu, S, 1, p(d_pred), p(d_samp))

    def draw_alias():
        N.call("trec_sample_items_alias", nu, 0, ni, S, p(thr), p(alias), 1, 2, p(out_ids))

    def draw_k7():
        N.call("trec_sample_items", nu, 0, ni, S, 0, 1, 2, p(out_ids))

    calls = [("a_sampled_softmax", softmax), ("b_sampled_softmax_adjusted", softmax_adj), ("c_bpr", bpr), ("d_bpr_adjusted", bpr_adj),
             ("e_sample_items_alias", draw_alias), ("f_sample_items_k7", draw_k7)]
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
    # accidental hits of the drawn table, counted on the host with the CSR (a check of the shape, not part of the timing)
    sub = min(nu, 20000)
    ids, hit = samples[:sub].cpu().numpy(), 0
    for u in range(sub):
        hit += int(np.isin(ids[u], cols[indptr_h[u]:indptr_h[u + 1]]).sum())
    need = 3 * nu * S * 4 + 5 * P * 4 + 2 * (nu * 8 + P * 4)          # as scripts/sampled_loss_bench.py
    rec = {"what": "call times of the sampled softmax / BPR with and without the adjustments (hits removed, logQ) and of the alias sampler "
                   "against K7, one process, variants timed in turn per round between device events (scripts/sampled_adjust_bench.py); "
                   "synthetic predictions, Zipf item popularity, samples from the alias sampler",
           "device": torch.cuda.get_device_name(0), "commit": commit(), "clocks": box_clocks,
           "shape": {"n_users": nu, "n_interactions": P, "n_sampled": S, "n_items": ni, "temperature": args.temperature,
                     "power": args.power, "hit_fraction_of_samples_first_%d_users" % sub: float("%.4g" % (hit / (sub * S)))},
           "rounds": args.rounds, "warmup": args.warmup, "bytes_needed_per_plain_call_pair": need,
           "extra_bytes_of_the_id_table_read_twice": 2 * nu * S * 4, "ms": {}}
    for name, _ in calls:
        t = np.array(times[name])
        rec["ms"][name] = {"median": float("%.4g" % np.median(t)), "min": float("%.4g" % t.min()), "max": float("%.4g" % t.max())}
    med = {k: v["median"] for k, v in rec["ms"].items()}
    rec["ratios"] = {"b_over_a": float("%.4g" % (med["b_sampled_softmax_adjusted"] / med["a_sampled_softmax"])),
                     "d_over_c": float("%.4g" % (med["d_bpr_adjusted"] / med["c_bpr"])),
                     "e_over_f": float("%.4g" % (med["e_sample_items_alias"] / med["f_sample_items_k7"]))}
    line = json.dumps(rec, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
