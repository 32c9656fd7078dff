"""Cost of predict_top_k(candidates=...) (docs/candidate_sets.md) on one MI355X, one process, device-event timing.

200k users x 1M items, identity features, d = 128, biased dot product, 101 and 1,000 candidates per user drawn uniformly.
Per density, variants alternated after a warm-up, ROUNDS timed rounds each (median, minimum and maximum are recorded):
 1. kernel A (trec_candset_scores) against trec_pair_score_exact on the same pairs: ms, bytes/s with nnz * (kpad * 4 + 8) bytes,
    the fraction of the 7.4-7.9 TB/s the microarchitecture guide measures for an LDS row gather beyond the Infinity Cache, and
    whether the two outputs agree bit for bit;
 2. kernels B (trec_candset_topk, k = 10) and C (trec_candset_rank_count, one target per user) in ms;
 3. the whole predict_top_k(candidates=) call, the host share (CSR canonicalisation, upload of the CSR) split out, and the same
    call forced onto the slab form for the first 2,000 users.

Usage: python scripts/candidate_sets_bench.py [OUT_JSON]  (default profiles/candidate_sets.json)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
import torch

import tensorrec_amd as T
from tensorrec_amd import candidate_sets, ops
from tensorrec_amd.prediction_graphs import DotProductPredictionGraph
from tensorrec_amd.representation_graphs import LinearRepresentationGraph

NU, NI, D, K = int(os.environ.get("NU", 200_000)), int(os.environ.get("NI", 1_000_000)), 128, 10
NU_SLAB = int(os.environ.get("NU_SLAB", 2_000))
ROUNDS = int(os.environ.get("ROUNDS", 5))
GATHER_TBS = (7.4, 7.9)


def model(n_users, n_items):
    m = T.TensorRec(n_components=D, prediction_graph=DotProductPredictionGraph(), user_repr_graph=LinearRepresentationGraph(),
                    item_repr_graph=LinearRepresentationGraph(), seed=0)
    m.build(n_users, n_items)
    w = m.get_weights()
    rng = np.random.default_rng(1)
    for name in ("user_feature_biases", "item_feature_biases"):
        w[name] = (0.05 * rng.standard_normal(w[name].shape)).astype(np.float32)
    m.set_weights(w)
    return m


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    out = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e), out


def stats(ms):
    return {"ms_per_call": ms, "ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms))}


def one_density(m, uf, itf, per_user, rng):
    cols = rng.integers(0, NI, size=(NU, per_user), dtype=np.int64)
    cand = sp.csr_matrix((np.ones(NU * per_user, np.float32), cols.reshape(-1), np.arange(0, NU * per_user + 1, per_user, dtype=np.int64)),
                         shape=(NU, NI))
    t0 = time.perf_counter()
    ptr, idx = candidate_sets.candidate_csr(cand, NU, NI)
    host_ms = (time.perf_counter() - t0) * 1e3
    up_ms, (ptr_d, idx_d) = timed(lambda: (torch.from_numpy(ptr).cuda(), torch.from_numpy(idx).cuda()))
    nnz = int(len(idx))
    rec = {"candidates_per_user_drawn": per_user, "nnz": nnz, "csr_host_ms": host_ms, "csr_upload_ms": up_ms}
    print(per_user, "canonical CSR: nnz", nnz, "host ms", round(host_ms), flush=True)
    # the operands of the pairs form
    dev = idx_d.device
    w = m.get_weights()
    # (identity features: the representations are the weight matrices themselves)
    u_op, _, kpad = ops.score_prep(torch.from_numpy(w["linear_weights_user_0"]).to(dev), ops.DTYPE_F32)
    i_op, _, _ = ops.score_prep(torch.from_numpy(w["linear_weights_item"]).to(dev), ops.DTYPE_F32)
    ub = torch.from_numpy(w["user_feature_biases"].reshape(-1)).to(dev)
    ib = torch.from_numpy(w["item_feature_biases"].reshape(-1)).to(dev)
    xu = torch.from_numpy(np.repeat(np.arange(NU, dtype=np.int32), np.diff(ptr))).to(dev)
    out_a = torch.zeros(nnz, dtype=torch.float32, device=dev)
    run_a = lambda: ops.candset_scores(u_op, i_op, kpad, D, ptr_d, idx_d, nnz, ub, ib, out=out_a)  # noqa: E731
    run_p = lambda: ops.pair_scores_exact(u_op, i_op, kpad, D, xu, idx_d, ub, ib)  # noqa: E731
    lr = candidate_sets.long_rows(ptr)
    lr_d = torch.from_numpy(lr).to(dev) if len(lr) else None
    run_b = lambda: ops.candset_topk(out_a, ptr_d, idx_d, K, long_rows=lr_d)  # noqa: E731
    t_idx = torch.from_numpy(idx[ptr[:-1]]).to(dev)                     # one target per user: its first candidate
    t_sc = out_a[ptr_d[:-1]].contiguous()
    pair_ptr = torch.arange(NU + 1, dtype=torch.int64, device=dev)
    run_c = lambda: ops.candset_rank_count(pair_ptr, t_idx, t_sc, ptr_d, idx_d, out_a)  # noqa: E731
    run_call = lambda: m.predict_top_k(uf, itf, k=K, candidates=cand, return_device=True, return_route=True)  # noqa: E731
    variants = {"kernel_A": run_a, "pair_score_exact": run_p, "kernel_B": run_b, "kernel_C": run_c, "predict_top_k": run_call}
    for fn in variants.values():                                        # warm-up
        fn()
    ms = {n: [] for n in variants}
    for _ in range(ROUNDS):
        for n, fn in variants.items():
            ms[n].append(timed(fn)[0])
        print(per_user, "round", {n: round(t[-1], 3) for n, t in ms.items()}, flush=True)
    rec["bit_identical_A_vs_pair_score_exact"] = bool(torch.equal(run_a().view(torch.int32), run_p().view(torch.int32)))
    nbytes = nnz * (kpad * 4 + 8)
    for n in variants:
        rec[n] = stats(ms[n])
    for n in ("kernel_A", "pair_score_exact"):
        tbs = nbytes / (rec[n]["ms_median"] * 1e-3) / 1e12
        rec[n].update(bytes=nbytes, tb_per_s=tbs, fraction_of_gather_figure=[tbs / GATHER_TBS[1], tbs / GATHER_TBS[0]])
    rec["predict_top_k"]["route"] = run_call()[2]
    # the slab form on the first NU_SLAB users (what a density switch would weigh against the pairs form)
    form = m._candidate_form
    try:
        m._candidate_form = lambda: "slab"
        sl = lambda: m.predict_top_k(uf[:NU_SLAB], itf, k=K, candidates=cand[:NU_SLAB], return_device=True, return_route=True)  # noqa: E731
        sl()
        t = [timed(sl)[0] for _ in range(ROUNDS)]
        rec["predict_top_k_slab_form"] = dict(stats(t), users=NU_SLAB, route=sl()[2])
    finally:
        m._candidate_form = form
    pt = [timed(lambda: m.predict_top_k(uf[:NU_SLAB], itf, k=K, candidates=cand[:NU_SLAB], return_device=True))[0]
          for _ in range(ROUNDS + 1)][1:]
    rec["predict_top_k_pairs_form_same_users"] = dict(stats(pt), users=NU_SLAB)
    return rec


def main():
    out = {"device": torch.cuda.get_device_name(0), "users": NU, "items": NI, "d": D, "k": K, "rounds": ROUNDS}
    m = model(NU, NI)
    uf, itf = sp.identity(NU, dtype=np.float32, format="csr"), sp.identity(NI, dtype=np.float32, format="csr")
    rng = np.random.default_rng(0)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                             "profiles", "candidate_sets.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    for per_user in (101, 1000):
        out["candidates_%d" % per_user] = one_density(m, uf, itf, per_user, rng)
        print(per_user, json.dumps(out["candidates_%d" % per_user]), flush=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
