"""The hard-negative selection (csrc/sampler_hard.hip) alone, and one whole sampled-softmax step with and without it, on one GPU.

1. The kernel alone: 1,000,000 users x 1,000,000 items, d = 128, item biases, M candidates per user drawn by DeviceSampler, S = 100 (all
   hard), hits excluded against 20 positives per user -- ops.select_hard_negatives between two device events, warm-up calls first, then
   the timed calls; median, minimum and maximum per M.  The time is the CALL's as the stream sees it (one kernel launch; no trace was
   taken).  Bytes are counted from the shape by ``gather_bytes``: the M item rows of 4 d bytes per user, which is what the kernel has
   to move (the candidate table, biases and outputs add M * 8 + S * 4 bytes per user and are listed apart).  The achieved rate stands
   beside the repository's measured ceiling of bare random row gathers from a 512 MB table (profiles/r05_gather_ceiling_512.jsonl).
2. One optimiser step (TensorRec._train_step: sampling, scores, loss, gradients, Adam) of a SampledSoftmaxLossGraph fit at the fit
   leg's shape of bench.py with sampler = DeviceSampler (the base alone) and with HardNegativeSampler(n_candidates = M_step) over the
   same base, two models stepped in alternating rounds of one process, each step between device events.

    python scripts/hard_negatives_bench.py --out profiles/hard_negatives.json [--users 1000000 --items 1000000 --rounds 20]
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

GATHER_CEILING_TBS = 7.42        # bare random 512-byte row gathers from a 512 MB table (profiles/r05_gather_ceiling_512.jsonl)


def gather_bytes(n_users, M, d):
    """the item rows the kernel has to read: M rows of 4 d bytes per user"""
    return n_users * M * d * 4


def other_bytes(n_users, M, S, d):
    """what else a call moves: the user row, the candidate ids, a bias per candidate, the output row"""
    return n_users * (d * 4 + M * 4 + M * 4 + S * 4)


def summary(times):
    t = np.array(times)
    return {"median": float("%.4g" % np.median(t)), "min": float("%.4g" % t.min()), "max": float("%.4g" % t.max())}


def time_kernel(args, inter, M):
    dev = "cuda"
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    U = torch.randn((args.users, args.components), generator=g, device=dev)
    V = torch.randn((args.items, args.components), generator=g, device=dev)
    ib = torch.randn((args.items,), generator=g, device=dev)
    C = ops.sample_items(args.users, args.items, M, False, 1, 1, dev)
    times = []
    for r in range(args.warmup + args.rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = ops.select_hard_negatives(U, V, ib, inter, C, args.samples, None, exclude=True)
        b.record()
        b.synchronize()
        if r >= args.warmup:
            times.append(a.elapsed_time(b))
    assert tuple(out.shape) == (args.users, args.samples)
    rec = summary(times)
    rec["gather_bytes"] = gather_bytes(args.users, M, args.components)
    rec["other_bytes"] = other_bytes(args.users, M, args.samples, args.components)
    rec["gather_TB_per_s_at_median"] = float("%.4g" % (rec["gather_bytes"] / (rec["median"] * 1e-3) / 1e12))
    rec["share_of_gather_ceiling"] = float("%.3g" % (rec["gather_TB_per_s_at_median"] / GATHER_CEILING_TBS))
    rec["ms_at_the_gather_ceiling"] = float("%.4g" % (rec["gather_bytes"] / (GATHER_CEILING_TBS * 1e12) * 1e3))
    print("kernel M", M, json.dumps(rec), flush=True)
    del U, V, ib, C, out
    return rec


def time_steps(args, data):
    inter, uf, itf = data
    S = args.samples
    SSM = T.loss_graphs.SampledSoftmaxLossGraph
    samplers = {"base_alone": T.DeviceSampler(1), "scored": T.HardNegativeSampler(args.step_candidates, base=T.DeviceSampler(1))}
    models, times, kernels, forms = {}, {k: [] for k in samplers}, {}, {}
    for name, sampler in samplers.items():
        models[name] = T.TensorRec(n_components=args.components, loss_graph=SSM(args.temperature), seed=0, sampler=sampler)
        models[name].fit_partial(inter, uf, itf, epochs=1, n_sampled_items=S)      # builds the variables and the Adam slots; one step
        forms[name] = models[name].last_step_form
    dev = models["scored"]._store.device
    d_inter = Interactions(inter, n_users=uf.shape[0], n_items=itf.shape[0], device=dev)
    d_uf, d_itf = SparseFeatures(uf, dev), SparseFeatures(itf, dev)
    for r in range(args.warmup + args.rounds):
        for name, model in models.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            model._train_step(d_inter, d_uf, d_itf, 0.1, 0.0, S)
            b.record()
            b.synchronize()
            kernels[name] = model.last_step_kernel
            if r >= args.warmup:
                times[name].append(a.elapsed_time(b))
    out = {name: dict(summary(t), last_step_kernel=kernels[name], first_step_form=forms[name]) for name, t in times.items()}
    out["n_candidates"] = args.step_candidates
    out["scored_over_base_alone"] = float("%.4g" % (out["scored"]["median"] / out["base_alone"]["median"]))
    out["ranges_overlap"] = bool(out["base_alone"]["max"] >= out["scored"]["min"])
    print("step", json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--components", type=int, default=128)
    ap.add_argument("--positives", type=int, default=20)
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--candidates", type=int, nargs="+", default=[128, 256, 1024])
    ap.add_argument("--step-candidates", type=int, default=256)
    ap.add_argument("--temperature", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    box_clocks = clocks()                                     # (a child process, before this one opens the GPU)
    N.require_gpu()
    N.load()
    data = fit_leg_data(args.users, args.items, args.positives)
    rec = {"what": "ops.select_hard_negatives alone (call time between device events; bytes counted from the shape) and one optimiser "
                   "step of a sampled-softmax fit with HardNegativeSampler against its base sampler alone, alternating rounds of one "
                   "process (scripts/hard_negatives_bench.py)",
           "device": torch.cuda.get_device_name(0), "commit": commit(), "clocks": box_clocks,
           "shape": {"n_users": args.users, "n_items": args.items, "d": args.components, "n_sampled": args.samples, "n_hard": args.samples,
                     "positives_per_user": args.positives, "temperature": args.temperature},
           "gather_ceiling_TB_per_s": GATHER_CEILING_TBS, "rounds": args.rounds, "warmup": args.warmup, "kernel_ms": {}, "step_ms": None}
    inter = Interactions(data[0], n_users=args.users, n_items=args.items, device="cuda")
    for M in args.candidates:
        rec["kernel_ms"]["M%d" % M] = time_kernel(args, inter, M)
        gc.collect()
        torch.cuda.empty_cache()
    del inter
    rec["step_ms"] = time_steps(args, data)
    line = json.dumps(rec, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
