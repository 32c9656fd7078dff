"""One optimiser step of a BPRLossGraph fit on the one-pass fused route (csrc/bpr_fused.hip, opt-in: tuning bpr_fused = 1) against
the generic route (K3 scores of both pair lists, trec_bpr_fwd / _bwd of csrc/loss_sampled.hip, autograd back through K3 and K1), in
one process on one GPU.  The generic route is the reference for the time: it is the code path a BPR fit took before the fused step
existed, measured in the same run.

Shape: the fit leg of bench.py -- 1,000,000 users x 1,000,000 items, identity features, d = 128, biased dot scores, 20 uniform-random
positive interactions per user (duplicates merged) -- with S = 100, the default uniform sampler.  Two arms:
    a  BPRLossGraph()
    b  BPRLossGraph(remove_accidental_hits=True)

Method (scripts/warp_fused_bench.py's, unchanged): the model is built and stepped once through fit_partial; then
TensorRec._train_step -- the whole step: sampling, scores, loss, gradients, Adam on every variable -- is timed between two device
events on the current stream, with tuning bpr_fused at 0 and at 1 in alternating rounds, so both routes see the same box state;
warm-up rounds first, then the timed rounds; the record holds median, minimum and maximum per route and which kernel the model
reported.  Times are step times as the host sees them on the stream, not kernel times from a trace.  After the timed rounds one more
fused step runs with the event brackets of ops on, only to read ops.LAST_FUSED_STATS: the grouping route the item side took and the
share of sampled pairs whose coefficient is exactly 0.

    python scripts/bpr_fused_bench.py --out profiles/bpr_fused.json [--users 1000000 --items 1000000 --rounds 20]
"""
import argparse
import gc
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tensorrec_amd as T  # noqa: E402
from tensorrec_amd import _native as N, ops  # noqa: E402
from tensorrec_amd.sparse import Interactions, SparseFeatures  # noqa: E402
from sampled_loss_bench import clocks, commit  # noqa: E402
from softmax_fused_bench import fit_leg_data  # noqa: E402


def time_arm(name, model, data, args):
    inter, uf, itf = data
    S = args.samples
    model.fit_partial(inter, uf, itf, epochs=1, n_sampled_items=S)           # builds the variables and the Adam slots; one step
    dev = model._store.device
    d_inter = Interactions(inter, n_users=uf.shape[0], n_items=itf.shape[0], device=dev)
    d_uf, d_itf = SparseFeatures(uf, dev), SparseFeatures(itf, dev)
    times, kernels = {0: [], 1: []}, {}
    try:
        for r in range(args.warmup + args.rounds):
            for fused in (0, 1):
                N.set_tuning("bpr_fused", fused)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                model._train_step(d_inter, d_uf, d_itf, 0.1, 0.0, S)
                b.record()
                b.synchronize()
                kernels[fused] = model.last_step_kernel
                if r >= args.warmup:
                    times[fused].append(a.elapsed_time(b))
        ops.KERNEL_EVENTS = []                                    # one untimed fused step: what the item side saw
        try:
            model._train_step(d_inter, d_uf, d_itf, 0.1, 0.0, S)
            torch.cuda.synchronize()
            st = dict(ops.LAST_FUSED_STATS)
        finally:
            ops.KERNEL_EVENTS = None
    finally:
        N.clear_tuning("bpr_fused")
    assert kernels == {0: None, 1: "bpr_fused"}, kernels
    out = {"interactions": int(inter.nnz), "longest_row": int(np.diff(inter.indptr).max())}
    for fused, key in ((0, "generic"), (1, "fused")):
        t = np.array(times[fused])
        out[key] = {"median": float("%.4g" % np.median(t)), "min": float("%.4g" % t.min()), "max": float("%.4g" % t.max()),
                    "last_step_kernel": kernels[fused]}
    out["fused_over_generic"] = float("%.4g" % (out["fused"]["median"] / out["generic"]["median"]))
    out["ranges_overlap"] = bool(out["fused"]["max"] >= out["generic"]["min"])
    out["ranges_apart_in_favour_of_fused"] = bool(out["fused"]["max"] < out["generic"]["min"])
    pairs = int(st["sampled_pairs"])
    out["item_side"] = {"grouping_route": st["route"], "drop_zero": bool(st["drop_zero"]), "sampled_pairs": pairs,
                        "sampled_pairs_kept": int(st["sampled_pairs_kept"].item()),
                        "share_of_sampled_pairs_with_coefficient_0": float("%.5g" % (int(st["sampled_pairs_with_coefficient_0"].item()) / pairs))}
    print(name, json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--components", type=int, default=128)
    ap.add_argument("--positives", type=int, default=20)
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    box_clocks = clocks()                                     # (a child process, before this one opens the GPU)
    N.require_gpu()
    N.load()
    data = fit_leg_data(args.users, args.items, args.positives)
    BPR = T.loss_graphs.BPRLossGraph
    arms = [("a_plain_uniform", lambda: T.TensorRec(n_components=args.components, loss_graph=BPR(), seed=0)),
            ("b_hits_removed_uniform", lambda: T.TensorRec(n_components=args.components, loss_graph=BPR(remove_accidental_hits=True), seed=0))]
    rec = {"what": "one optimiser step (TensorRec._train_step: sampling, scores, loss, gradients, Adam) of a BPR fit on the one-pass "
                   "fused route (opt-in) against the generic route, tuning bpr_fused 0 / 1 in alternating rounds of one process, each "
                   "step between device events (scripts/bpr_fused_bench.py); the fit leg's shape of bench.py",
           "device": torch.cuda.get_device_name(0), "commit": commit(), "clocks": box_clocks,
           "shape": {"n_users": args.users, "n_items": args.items, "d": args.components, "n_sampled": args.samples,
                     "positives_per_user": args.positives},
           "rounds": args.rounds, "warmup": args.warmup, "ms": {}}
    for name, make in arms:
        model = make()
        rec["ms"][name] = time_arm(name, model, data, args)
        del model
        gc.collect()
        torch.cuda.empty_cache()
    rec["ranges_apart_in_both_arms"] = bool(all(v["ranges_apart_in_favour_of_fused"] for v in rec["ms"].values()))
    line = json.dumps(rec, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
