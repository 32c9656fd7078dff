"""One optimiser step of a SampledSoftmaxLossGraph(shared_negatives=True, remove_accidental_hits=True, log_q_correction=True) fit under
a PopularitySampler: the masked MFMA route (csrc/softmax_shared.hip, tuning softmax_shared_hits = 1) against the expanded generic
step (tuning 0, the default), and against the unmasked MFMA route (hits kept) -- in one process on one GPU.

    100,000 users x 1,000,000 items, d = 128, biased dot scores, about 20 positives per user, S = 1024.
    a  hits removed, tuning softmax_shared_hits at 0 and at 1 in alternating rounds.  The 0 arm expands the shared row to the [U, S]
       table and runs K3 scores, the adjusted loss kernels and autograd back through K3 and K1.
    b  tuning 1: the model of (a) against a second model that differs in remove_accidental_hits=False alone (the unmasked MFMA
       route), alternating.  The ratio is the price of the mask: the hit ranges, the cursors and the sorted gather.

Method (scripts/softmax_shared_bench.py's): each model is built and stepped once through fit_partial; then TensorRec._train_step --
the whole step: sampling, scores, loss, gradients, Adam on every variable -- is timed between two device events on the current
stream; 3 warm-up rounds, then the timed rounds.  The record holds median, minimum and maximum per arm, the kernel the model reported
and whether the ranges overlap.  Times are step times as the host sees them on the stream, not kernel times from a trace.

    python scripts/softmax_shared_hits_bench.py --out profiles/softmax_shared_hits.json [--rounds 20]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tensorrec_amd as T  # noqa: E402
from tensorrec_amd import _native as N  # noqa: E402
from tensorrec_amd.sparse import Interactions, SparseFeatures  # noqa: E402
from sampled_loss_bench import clocks, commit  # noqa: E402
from softmax_fused_bench import fit_leg_data  # noqa: E402
from softmax_shared_bench import summary  # noqa: E402


def build(data, args, hits):
    inter, uf, itf = data
    graph = T.loss_graphs.SampledSoftmaxLossGraph(args.temperature, shared_negatives=True, remove_accidental_hits=hits,
                                                  log_q_correction=True)
    model = T.TensorRec(n_components=args.components, seed=0, loss_graph=graph,
                        sampler=T.PopularitySampler(inter, power=0.75, smoothing=1.0, seed=5))
    model.fit_partial(inter, uf, itf, epochs=1, n_sampled_items=args.samples)      # builds the variables and the Adam slots; one step
    return model


def time_arms(arms, device_data, args):
    """{label: summary} of _train_step over ``arms`` -- (label, model, value of tuning softmax_shared_hits) --, alternating inside
    every round"""
    d_inter, d_uf, d_itf = device_data
    times, kernels = {a[0]: [] for a in arms}, {}
    try:
        for r in range(args.warmup + args.rounds):
            for label, model, tuning in arms:
                N.set_tuning("softmax_shared_hits", tuning)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                model._train_step(d_inter, d_uf, d_itf, 0.1, 0.0, args.samples)
                b.record()
                b.synchronize()
                kernels[label] = model.last_step_kernel
                if r >= args.warmup:
                    times[label].append(a.elapsed_time(b))
    finally:
        N.clear_tuning("softmax_shared_hits")
    return {label: summary(times[label], kernels[label]) for label, _, _ in arms}


def compare(out, new, old):
    rec = {old: out[old], new: out[new]}
    rec["%s_over_%s" % (new, old)] = float("%.4g" % (out[new]["median"] / out[old]["median"]))
    rec["ranges_overlap"] = bool(out[new]["max"] >= out[old]["min"] and out[old]["max"] >= out[new]["min"])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=100_000)
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--components", type=int, default=128)
    ap.add_argument("--positives", type=int, default=20)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--temperature", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    box_clocks = clocks()                                     # (a child process, before this one opens the GPU)
    N.require_gpu()
    N.load()
    rec = {"what": "one optimiser step (TensorRec._train_step: sampling, scores, loss, gradients, Adam) of a sampled-softmax fit with "
                   "shared negatives from a PopularitySampler, the logQ correction and accidental hits removed: the masked MFMA route "
                   "against the expanded generic step (arm a, tuning softmax_shared_hits 0 / 1 alternating) and against the unmasked "
                   "MFMA route with hits kept (arm b); each step between device events (scripts/softmax_shared_hits_bench.py)",
           "device": torch.cuda.get_device_name(0), "commit": commit(), "clocks": box_clocks, "rounds": args.rounds, "warmup": args.warmup,
           "ms": {}}
    data = fit_leg_data(args.users, args.items, args.positives)
    inter, uf, itf = data
    masked, unmasked = build(data, args, True), build(data, args, False)
    dev = masked._store.device
    device_data = (Interactions(inter, n_users=uf.shape[0], n_items=itf.shape[0], device=dev), SparseFeatures(uf, dev),
                   SparseFeatures(itf, dev))
    rec["shape"] = {"n_users": args.users, "n_items": args.items, "d": args.components, "n_sampled": args.samples,
                    "interactions": int(inter.nnz), "temperature": args.temperature, "sampler": "PopularitySampler(power=0.75)",
                    "log_q_correction": True}
    out = time_arms([("generic", masked, 0), ("masked", masked, 1)], device_data, args)
    assert out["generic"]["last_step_kernel"] is None and out["masked"]["last_step_kernel"] == "softmax_shared_hits", out
    a = compare(out, "masked", "generic")
    a["masked_wins"] = bool(a["masked_over_generic"] < 1.0 and not a["ranges_overlap"])
    rec["ms"]["a"] = a
    print("a", json.dumps(a), flush=True)
    out = time_arms([("unmasked", unmasked, 1), ("masked", masked, 1)], device_data, args)
    assert out["unmasked"]["last_step_kernel"] == "softmax_shared" and out["masked"]["last_step_kernel"] == "softmax_shared_hits", out
    b = compare(out, "masked", "unmasked")
    rec["ms"]["b"] = b
    print("b", json.dumps(b), flush=True)
    rec["default_softmax_shared_hits"] = 0                    # opt-in whatever the figures say (docs/sampled_losses.md)
    line = json.dumps(rec, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
