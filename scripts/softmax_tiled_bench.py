"""One optimiser step of a SampledSoftmaxLossGraph fit on the tiled one-pass route (csrc/softmax_tiled.hip) against the generic route
(K3 scores, the loss kernels of csrc/loss_sampled.hip, autograd back through K3 and K1), in one process on one GPU.

Shape: the synthetic model of scripts/softmax_full_bench.py -- 138,493 users x 26,744 items, Zipf-distributed items, about 144
positives per user (the longest row is far beyond what the per-user fused step covers), identity features, d = 128, biased scores.
Three arms:
    a  dot scores, S = 100
    b  dot scores, S = 2,674 (10 % of the items)
    c  Euclidean scores, S = 100

Method (scripts/softmax_fused_bench.py's): the model is built and stepped once through fit_partial; then TensorRec._train_step -- the
whole step: sampling, scores, loss, gradients, Adam on every variable -- is timed between two device events on the current stream, with
tuning softmax_tiled at 0 and at 1 in alternating rounds, so both routes see the same box state; warm-up rounds first, then the timed
rounds; every round asserts the route it took; the record holds median, minimum and maximum per route.  Times are step times as the
host sees them on the stream, not kernel times from a trace.

    python scripts/softmax_tiled_bench.py --out profiles/softmax_tiled.json [--arms a,b,c --users 138493 --items 26744 --rounds 20]

With --out and a subset of the arms, the arms already in the file are kept.
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
from tensorrec_amd import _native as N  # noqa: E402
from tensorrec_amd import ops  # noqa: E402
from tensorrec_amd.sparse import Interactions, SparseFeatures  # noqa: E402
from sampled_loss_bench import clocks, commit  # noqa: E402
from softmax_full_bench import zipf_data  # noqa: E402

ARMS = {"a": ("a_dot_S100", "dot", 100), "b": ("b_dot_S2674", "dot", 2674), "c": ("c_euclid_S100", "euclid", 100)}


def time_arm(name, model, data, S, args):
    inter, uf, itf = data
    model.fit_partial(inter[:256], uf[:256], itf, epochs=1, n_sampled_items=S)     # builds the variables and the Adam slots; one small step
    dev = model._store.device
    d_inter = Interactions(inter, n_users=uf.shape[0], n_items=itf.shape[0], device=dev)
    d_uf, d_itf = SparseFeatures(uf, dev), SparseFeatures(itf, dev)
    times, item_side = {0: [], 1: []}, None
    try:
        for r in range(args.warmup + args.rounds):
            for tiled in (0, 1):
                N.set_tuning("softmax_tiled", tiled)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                model._train_step(d_inter, d_uf, d_itf, 0.1, 0.0, S)
                b.record()
                b.synchronize()
                assert model.last_step_kernel == ("softmax_tiled" if tiled else None), (r, tiled, model.last_step_kernel)
                if tiled:
                    item_side = ops.LAST_FUSED_STATS["route"]
                if r >= args.warmup:
                    times[tiled].append(a.elapsed_time(b))
    finally:
        N.clear_tuning("softmax_tiled")
    out = {"interactions": int(inter.nnz), "longest_row": int(np.diff(inter.indptr).max()), "n_sampled": S, "item_side": item_side}
    for tiled, key in ((0, "generic"), (1, "tiled")):
        t = np.array(times[tiled])
        out[key] = {"median": float("%.4g" % np.median(t)), "min": float("%.4g" % t.min()), "max": float("%.4g" % t.max()),
                    "last_step_kernel": "softmax_tiled" if tiled else None}
    out["tiled_over_generic"] = float("%.4g" % (out["tiled"]["median"] / out["generic"]["median"]))
    out["ranges_overlap"] = bool(out["tiled"]["max"] >= out["generic"]["min"] and out["generic"]["max"] >= out["tiled"]["min"])
    print(name, json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", default="a,b,c")
    ap.add_argument("--users", type=int, default=138_493)
    ap.add_argument("--items", type=int, default=26_744)
    ap.add_argument("--components", type=int, default=128)
    ap.add_argument("--positives", type=int, default=144)
    ap.add_argument("--temperature", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    box_clocks = clocks()                                     # (a child process, before this one opens the GPU)
    N.require_gpu()
    N.load()
    data = zipf_data(args.users, args.items, args.positives)
    graphs = {"dot": T.prediction_graphs.DotProductPredictionGraph, "euclid": T.prediction_graphs.EuclideanSimilarityPredictionGraph}
    rec = {"what": "one optimiser step (TensorRec._train_step: sampling, scores, loss, gradients, Adam) of a sampled-softmax fit on the "
                   "tiled one-pass route against the generic route, tuning softmax_tiled 0 / 1 in alternating rounds of one process, each "
                   "step between device events (scripts/softmax_tiled_bench.py); the synthetic Zipf model of scripts/softmax_full_bench.py",
           "device": torch.cuda.get_device_name(0), "commit": commit(), "clocks": box_clocks,
           "shape": {"n_users": args.users, "n_items": args.items, "d": args.components, "positives_per_user": args.positives,
                     "temperature": args.temperature},
           "rounds": args.rounds, "warmup": args.warmup, "ms": {}}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            rec["ms"] = json.load(f).get("ms", {})
    for key in args.arms.split(","):
        name, kind, S = ARMS[key]
        model = T.TensorRec(n_components=args.components, prediction_graph=graphs[kind](), seed=0,
                            loss_graph=T.loss_graphs.SampledSoftmaxLossGraph(args.temperature))
        rec["ms"][name] = time_arm(name, model, data, S, args)
        del model
        gc.collect()
        torch.cuda.empty_cache()
    line = json.dumps(rec, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
