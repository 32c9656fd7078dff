"""One optimiser step of a SampledSoftmaxLossGraph(shared_negatives=True) fit: the MFMA route (csrc/softmax_shared.hip) against the
expanded generic step, in one process on one GPU.

    a  100,000 users x 1,000,000 items, d = 128, biased dot scores, about 20 positives per user, S = 1024; tuning softmax_shared at 0
       and at 1 in alternating rounds.  The 0 arm expands the shared row to the [U, S] table and runs K3 scores, the loss kernels and
       autograd back through K3 and K1: its [U, S] tensors are 400 MB each.
    b  the fit leg of bench.py, 1,000,000 x 1,000,000, the MFMA route only, at S = 1024 and S = 4096.

Method (scripts/softmax_fused_bench.py's): the model is built and stepped once through fit_partial; then TensorRec._train_step -- the
whole step: sampling, scores, loss, gradients, Adam on every variable -- is timed between two device events on the current stream; 3
warm-up rounds, then the timed rounds, the arms of (a) alternating so both see the same box state.  The record holds median, minimum and
maximum per arm, the kernel the model reported and, for the MFMA route, the achieved share of 5 * 2 U S d flop at 155 TF (the fp32
MFMA rate).  Times are step times as the host sees them on the stream, not kernel times from a trace.

    python scripts/softmax_shared_bench.py --out profiles/softmax_shared.json [--rounds 20]
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
from tensorrec_amd.sparse import Interactions, SparseFeatures  # noqa: E402
from sampled_loss_bench import clocks, commit  # noqa: E402
from softmax_fused_bench import fit_leg_data  # noqa: E402

MFMA_FP32_TFLOPS = 155.0


def summary(times, kernel):
    t = np.array(times)
    return {"median": float("%.4g" % np.median(t)), "min": float("%.4g" % t.min()), "max": float("%.4g" % t.max()),
            "last_step_kernel": kernel}


def share(ms, n_users, S, d):
    """achieved share of five GEMM-equivalents (scores forward, scores + product in both backward directions) at the fp32 MFMA rate"""
    return float("%.3g" % (5.0 * 2.0 * n_users * S * d / (ms * 1e-3) / (MFMA_FP32_TFLOPS * 1e12)))


def time_steps(data, args, S, tunings):
    """{tuning: summary} of _train_step at the given values of tuning softmax_shared, alternating inside every round"""
    inter, uf, itf = data
    model = T.TensorRec(n_components=args.components, seed=0,
                        loss_graph=T.loss_graphs.SampledSoftmaxLossGraph(args.temperature, shared_negatives=True))
    N.set_tuning("softmax_shared", tunings[-1])
    try:
        model.fit_partial(inter, uf, itf, epochs=1, n_sampled_items=S)       # builds the variables and the Adam slots; one step
        dev = model._store.device
        d_inter = Interactions(inter, n_users=uf.shape[0], n_items=itf.shape[0], device=dev)
        d_uf, d_itf = SparseFeatures(uf, dev), SparseFeatures(itf, dev)
        times, kernels = {v: [] for v in tunings}, {}
        for r in range(args.warmup + args.rounds):
            for v in tunings:
                N.set_tuning("softmax_shared", v)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                model._train_step(d_inter, d_uf, d_itf, 0.1, 0.0, S)
                b.record()
                b.synchronize()
                kernels[v] = model.last_step_kernel
                if r >= args.warmup:
                    times[v].append(a.elapsed_time(b))
    finally:
        N.clear_tuning("softmax_shared")
    assert all(kernels[v] == ("softmax_shared" if v else None) for v in tunings), kernels
    out = {v: summary(times[v], kernels[v]) for v in tunings}
    del model, d_inter, d_uf, d_itf
    gc.collect()
    torch.cuda.empty_cache()
    return out, int(inter.nnz)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users-a", type=int, default=100_000)
    ap.add_argument("--users-b", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--components", type=int, default=128)
    ap.add_argument("--positives", type=int, default=20)
    ap.add_argument("--samples-a", type=int, default=1024)
    ap.add_argument("--samples-b", type=int, nargs="*", default=[1024, 4096])
    ap.add_argument("--temperature", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    box_clocks = clocks()                                     # (a child process, before this one opens the GPU)
    N.require_gpu()
    N.load()
    d = args.components
    rec = {"what": "one optimiser step (TensorRec._train_step: sampling, scores, loss, gradients, Adam) of a sampled-softmax fit with "
                   "shared negatives: the MFMA route against the expanded generic step (arm a, tuning softmax_shared 0 / 1 alternating), "
                   "and the MFMA route alone at the fit leg's shape of bench.py (arm b); each step between device events "
                   "(scripts/softmax_shared_bench.py)",
           "device": torch.cuda.get_device_name(0), "commit": commit(), "clocks": box_clocks, "rounds": args.rounds, "warmup": args.warmup,
           "flop_model": "5 * 2 U S d at %g TF" % MFMA_FP32_TFLOPS, "ms": {}}
    data = fit_leg_data(args.users_a, args.items, args.positives)
    out, nnz = time_steps(data, args, args.samples_a, (0, 1))
    a = {"shape": {"n_users": args.users_a, "n_items": args.items, "d": d, "n_sampled": args.samples_a, "interactions": nnz,
                   "temperature": args.temperature}, "generic": out[0], "shared": out[1]}
    a["shared"]["share_of_fp32_mfma_rate"] = share(out[1]["median"], args.users_a, args.samples_a, d)
    a["shared_over_generic"] = float("%.4g" % (out[1]["median"] / out[0]["median"]))
    a["ranges_overlap"] = bool(out[1]["max"] >= out[0]["min"])
    a["shared_wins"] = bool(out[1]["median"] < out[0]["median"] and not a["ranges_overlap"])
    rec["ms"]["a"] = a
    print("a", json.dumps(a), flush=True)
    del data
    gc.collect()
    if args.samples_b:
        data = fit_leg_data(args.users_b, args.items, args.positives)
        for S in args.samples_b:
            out, nnz = time_steps(data, args, S, (1,))
            b = {"shape": {"n_users": args.users_b, "n_items": args.items, "d": d, "n_sampled": S, "interactions": nnz,
                           "temperature": args.temperature}, "shared": out[1]}
            b["shared"]["share_of_fp32_mfma_rate"] = share(out[1]["median"], args.users_b, S, d)
            rec["ms"]["b_S%d" % S] = b
            print("b_S%d" % S, json.dumps(b), flush=True)
    rec["default_softmax_shared"] = 1 if a["shared_wins"] else 0
    line = json.dumps(rec, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
