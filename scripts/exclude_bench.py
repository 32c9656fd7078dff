"""Cost of predict_top_k(exclude=...) (docs/exclusion.md) on one MI355X, one process, device-event timing.

A. configs[2] (1M users x 1M items, identity features, d = 128, top-10): no exclude / 64 random exclusions per user / 64 exclusions
   per user that include the user's true top-3 -- alternated after a warm-up; ms per call, k', route, users re-done on masked slabs,
   and a check of 256 sampled users against the dense prediction (model.predict, bit-exact vs the oracle elsewhere) with the
   excluded ids dropped.  Breakdown of the difference: the same call at k = 16 without exclusions (the over-fetch alone), the host
   CSR preparation and the upload of the CSR.
B. 200k users x 1M items with each user's own top-50 excluded: every user falls to tier 2 (the all-fallback cost).

Usage: python scripts/exclude_bench.py [OUT_JSON]  (default profiles/exclude_topk.json)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
import torch

import tensorrec_amd as T
from tensorrec_amd import exclusion
from tensorrec_amd.prediction_graphs import DotProductPredictionGraph
from tensorrec_amd.representation_graphs import LinearRepresentationGraph

NU, NI, D, K = int(os.environ.get("NU", 1_000_000)), int(os.environ.get("NI", 1_000_000)), 128, 10
NU_B = int(os.environ.get("NU_B", 200_000))
ROUNDS = int(os.environ.get("ROUNDS", 3))


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


def excl_csr(cols_per_user, n_items):
    """csr [n, n_items] from an int64 [n, e] array of ids (duplicates within a row merged)."""
    n, e = cols_per_user.shape
    m = sp.csr_matrix((np.ones(n * e, np.float32), cols_per_user.reshape(-1), np.arange(0, n * e + 1, e, dtype=np.int64)),
                      shape=(n, n_items))
    m.sum_duplicates()
    return m


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    out = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e), out


def check(m, uf, itf, users, excl, vals, idx):
    """sampled users against the dense prediction's order with the excluded ids dropped: number of users that differ"""
    bad = 0
    for s in range(0, len(users), 64):
        us = users[s:s + 64]
        pred = m.predict(uf[us], itf)
        for r, u in enumerate(us):
            row = pred[r].copy()
            ex = excl.indices[excl.indptr[u]:excl.indptr[u + 1]]
            keep = np.ones(row.shape[0], bool)
            keep[ex] = False
            cols = np.nonzero(keep)[0]
            v = row[cols]
            t = np.partition(v, -K)[-K]                                  # the k-th largest: its ties included below
            c = cols[v >= t]
            o = np.lexsort((c, -row[c]))[:K]
            bad += not (np.array_equal(idx[u], c[o].astype(np.int32)) and np.array_equal(vals[u], row[c[o]]))
    return bad


def main():
    out = {"device": torch.cuda.get_device_name(0), "users": NU, "items": NI, "d": D, "k": K}
    m = model(NU, NI)
    uf, itf = sp.identity(NU, dtype=np.float32, format="csr"), sp.identity(NI, dtype=np.float32, format="csr")
    rng = np.random.default_rng(0)
    _, (tv, ti) = timed(lambda: m.predict_top_k(uf, itf, k=K))
    rand64 = rng.integers(0, NI, size=(NU, 64), dtype=np.int64)
    with_top3 = rand64.copy()
    with_top3[:, :3] = ti[:, :3]
    variants = {"none": None, "random64": excl_csr(rand64, NI), "top3_plus61": excl_csr(with_top3, NI)}
    times = {n: [] for n in variants}
    times["none_k16"] = []
    reps, results = {}, {}
    for n, ex in variants.items():                                      # warm-up
        m.predict_top_k(uf, itf, k=K, exclude=ex, return_device=True)
    for _ in range(ROUNDS):
        for n, ex in variants.items():
            ms, (v, i, rep) = timed(lambda: m.predict_top_k(uf, itf, k=K, exclude=ex, return_device=True, return_route=True))
            times[n].append(ms)
            reps[n] = rep
            results[n] = (v, i)
        ms, _ = timed(lambda: m.predict_top_k(uf, itf, k=16, return_device=True))
        times["none_k16"].append(ms)
    sample = np.sort(rng.choice(NU, 256, replace=False))
    a = {}
    for n, ex in variants.items():
        v, i = (x.cpu().numpy() for x in results[n])
        rec = {"ms_per_call": times[n], "ms_median": float(np.median(times[n])), "route": reps[n]["route"],
               "user_batch_size": reps[n]["user_batch_size"]}
        if ex is not None:
            rec.update(reps[n]["exclude"])
            rec["sampled_users_differing"] = check(m, uf, itf, sample, ex, v, i)
        else:
            rec["sampled_users_differing"] = check(m, uf, itf, sample, sp.csr_matrix((NU, NI), dtype=np.float32), v, i)
        a[n] = rec
        print(n, {k_: rec[k_] for k_ in rec if k_ != "ms_per_call"}, flush=True)
    a["none_k16"] = {"ms_per_call": times["none_k16"], "ms_median": float(np.median(times["none_k16"])),
                     "note": "no exclude at k = 16: the cost of the over-fetch alone"}
    t0 = time.perf_counter()
    ptr, idx = exclusion.exclusion_csr(variants["random64"], NU, NI)
    host_ms = (time.perf_counter() - t0) * 1e3
    up_ms, _ = timed(lambda: (torch.from_numpy(ptr).cuda(), torch.from_numpy(idx).cuda()))
    a["random64_csr_host_ms"], a["random64_csr_upload_ms"] = host_ms, up_ms
    print("none_k16", a["none_k16"]["ms_median"], "csr host", host_ms, "upload", up_ms, flush=True)
    out["A_configs2"] = a
    del m, results
    torch.cuda.empty_cache()

    mb = model(NU_B, NI)
    ufb = sp.identity(NU_B, dtype=np.float32, format="csr")
    _, (_, t50) = timed(lambda: mb.predict_top_k(ufb, itf, k=50))
    exb = excl_csr(t50.astype(np.int64), NI)
    mb.predict_top_k(ufb[:256], itf, k=K, exclude=exb[:256])             # warm-up of the tier-2 path
    ms_b, (vb, ib, repb) = timed(lambda: mb.predict_top_k(ufb, itf, k=K, exclude=exb, return_device=True, return_route=True))
    vb, ib = vb.cpu().numpy(), ib.cpu().numpy()
    sample_b = np.sort(rng.choice(NU_B, 64, replace=False))
    out["B_all_fallback"] = {"users": NU_B, "ms_per_call": ms_b, "route": repb["route"], **repb["exclude"],
                             "ms_per_1k_fallback_users": ms_b / max(1, repb["exclude"]["n_fallback"]) * 1e3,
                             "sampled_users": len(sample_b), "sampled_users_differing": check(mb, ufb, itf, sample_b, exb, vb, ib)}
    print("B", out["B_all_fallback"], flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                             "profiles", "exclude_topk.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
