"""One optimiser step of a full-softmax fit (SoftmaxDenseLossGraph) at the shape of BASELINE.json configs[4]: a synthetic 138,493 x
26,744 model, Zipf-distributed items, about 144 positives per user, d = 128, biased dot scores; in one process on one GPU.

    p  what the code could already run: a custom is_dense torch loss graph (torch.logsumexp on tf_prediction), defined below.  It
       materialises the [U, I] predictions, their exponentials and their gradient.  The trainer also ranks the predictions for a
       user-defined dense loss (tf_rankings, a U * I^2 counting kernel no softmax reads): the baseline is spared that by declaring its
       connect_loss_graph a built-in one, so the arm times the loss the way a careful user would have written it.
    g  SoftmaxDenseLossGraph with tuning softmax_full = 0: the generic kernels of csrc/loss_dense.hip on the dense predictions.
    s  SoftmaxDenseLossGraph with tuning softmax_full = 1: the item representation streamed as MFMA tiles (csrc/softmax_shared.hip).
    p, g and s run on a user batch of 16,384 so that the [U, I] arms fit, alternating inside every round;
    s_whole: the streamed route once more on the whole 138,493-user batch, alone.

Method (scripts/softmax_shared_bench.py's): each model is built and stepped once through fit_partial; then TensorRec._train_step --
the whole step: scores, loss, gradients, Adam on every variable -- is timed between two device events on the current stream; 3 warm-up
rounds, then the timed rounds.  The record holds median, minimum and maximum per arm and the kernel the model reported.  Times are step
times as the host sees them on the stream, not kernel times from a trace.

    python scripts/softmax_full_bench.py --out profiles/softmax_full.json [--rounds 20]
"""
import argparse
import gc
import json
import os
import sys

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tensorrec_amd as T  # noqa: E402
from tensorrec_amd import _native as N  # noqa: E402
from tensorrec_amd.loss_graphs import AbstractLossGraph, SoftmaxDenseLossGraph  # noqa: E402
from tensorrec_amd.sparse import Interactions, SparseFeatures  # noqa: E402
from sampled_loss_bench import clocks, commit  # noqa: E402
from softmax_shared_bench import summary  # noqa: E402


class TorchFullSoftmax(AbstractLossGraph):
    """the full softmax as a user would write it in torch: the baseline arm"""
    is_dense = True

    def __init__(self, temperature):
        self.temperature = float(temperature)

    def connect_loss_graph(self, tf_prediction, tf_interactions, **kwargs):
        w = tf_prediction / self.temperature
        lse = torch.logsumexp(w, dim=1)
        pos = tf_interactions.values > 0
        xu, xi = tf_interactions.x_user[pos], tf_interactions.x_item[pos]
        return lse[xu] - w[xu, xi]


TorchFullSoftmax.connect_loss_graph.__module__ = AbstractLossGraph.__module__        # (no tf_rankings: see arm p above)


def zipf_data(n_users, n_items, positives, exponent=1.0, seed=1000):
    """Zipf-distributed items, about `positives` distinct ones per user: the smallest number of draws k whose expected number of
    distinct items, sum_i 1 - (1 - p_i)^k, reaches `positives` (duplicates are folded); identity features"""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, n_items + 1) ** exponent
    p /= p.sum()
    per_user = positives
    while (1.0 - (1.0 - p) ** per_user).sum() < positives:
        per_user += 1
    cdf = np.cumsum(p)
    perm = rng.permutation(n_items)                            # popularity is not the item order
    cols = perm[np.minimum(np.searchsorted(cdf, rng.random((n_users, per_user))), n_items - 1)].astype(np.int32)
    indptr = np.arange(0, (n_users + 1) * per_user, per_user, dtype=np.int64)
    inter = sp.csr_matrix((np.ones(n_users * per_user, np.float32), cols.reshape(-1), indptr), shape=(n_users, n_items))
    inter.sum_duplicates()
    inter.data[:] = 1.0
    return inter, sp.identity(n_users, dtype=np.float32, format="csr"), sp.identity(n_items, dtype=np.float32, format="csr")


def build(loss_graph, data, args):
    inter, uf, itf = data
    model = T.TensorRec(n_components=args.components, seed=0, loss_graph=loss_graph)
    model.fit_partial(inter[:256], uf[:256], itf, epochs=1)    # builds the variables and the Adam slots; one small step
    return model


def time_arms(arms, batch, args, dev):
    """{arm: summary}; arms: [(name, model, tuning softmax_full or None)], alternating inside every round on one device batch"""
    inter, uf, itf = batch
    d_inter = Interactions(inter, n_users=uf.shape[0], n_items=itf.shape[0], device=dev)
    d_uf, d_itf = SparseFeatures(uf, dev), SparseFeatures(itf, dev)
    times, kernels = {name: [] for name, _, _ in arms}, {}
    try:
        for r in range(args.warmup + args.rounds):
            for name, model, tuning in arms:
                if tuning is not None:
                    N.set_tuning("softmax_full", tuning)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                model._train_step(d_inter, d_uf, d_itf, 0.1, 0.0, None)
                b.record()
                b.synchronize()
                kernels[name] = model.last_step_kernel
                if r >= args.warmup:
                    times[name].append(a.elapsed_time(b))
    finally:
        N.clear_tuning("softmax_full")
    out = {name: summary(times[name], kernels[name]) for name, _, _ in arms}
    del d_inter, d_uf, d_itf
    gc.collect()
    torch.cuda.empty_cache()
    return out, int(inter.nnz)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=138_493)
    ap.add_argument("--items", type=int, default=26_744)
    ap.add_argument("--batch", type=int, default=16_384)
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
    inter, uf, itf = data
    rec = {"what": "one optimiser step (TensorRec._train_step: scores, loss, gradients, Adam) of a full-softmax fit: a custom torch "
                   "is_dense loss graph (p, the baseline), SoftmaxDenseLossGraph on the generic kernels (g, tuning softmax_full 0) and on "
                   "the streamed MFMA route (s, tuning 1), alternating on one user batch; the streamed route alone on the whole user "
                   "batch (s_whole); each step between device events (scripts/softmax_full_bench.py)",
           "device": torch.cuda.get_device_name(0), "commit": commit(), "clocks": box_clocks, "rounds": args.rounds, "warmup": args.warmup,
           "shape": {"n_users": args.users, "n_items": args.items, "d": args.components, "user_batch": args.batch,
                     "temperature": args.temperature, "interactions": int(inter.nnz),
                     "positives_per_user": float("%.4g" % (inter.nnz / args.users)),
                     "most_popular_item": int(np.bincount(inter.indices).max())}, "ms": {}}
    torch_model = build(TorchFullSoftmax(args.temperature), data, args)
    model = build(SoftmaxDenseLossGraph(args.temperature), data, args)
    dev = model._store.device
    batch = (inter[:args.batch], uf[:args.batch], itf)
    out, nnz = time_arms([("p", torch_model, None), ("g", model, 0), ("s", model, 1)], batch, args, dev)
    assert out["p"]["last_step_kernel"] is None and out["g"]["last_step_kernel"] is None and out["s"]["last_step_kernel"] == "softmax_full", out
    out["batch_interactions"] = nnz
    out["s_over_p"] = float("%.4g" % (out["s"]["median"] / out["p"]["median"]))
    out["g_over_p"] = float("%.4g" % (out["g"]["median"] / out["p"]["median"]))
    out["ranges_overlap"] = bool(out["s"]["max"] >= out["p"]["min"])
    out["s_wins"] = bool(out["s"]["median"] < out["p"]["median"] and not out["ranges_overlap"])
    rec["ms"]["batch"] = out
    print("batch", json.dumps(out), flush=True)
    del torch_model
    gc.collect()
    torch.cuda.empty_cache()
    whole, nnz = time_arms([("s_whole", model, 1)], data, args, dev)
    assert whole["s_whole"]["last_step_kernel"] == "softmax_full", whole
    rec["ms"]["whole"] = whole
    print("whole", json.dumps(whole), flush=True)
    rec["default_softmax_full"] = 1 if out["s_wins"] else 0
    line = json.dumps(rec, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
