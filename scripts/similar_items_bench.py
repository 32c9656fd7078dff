"""Cost of predict_similar_items_top_k (docs/similar_items.md) on one MI355X, one process, device-event timing.

A. The "related items" table of a whole catalogue: every item's cosine top-10 among 1M items, d = 128 (item_ids=None), with and
   without exclude_self, next to predict_top_k at 1M users x 1M items on the same model in the same run -- the query side goes
   through the same kernels, so about the same time per call is the expectation this file records instead of assuming.  Calls are
   alternated after a warm-up; 64 sampled rows of each table are checked against the dense rows of predict_similar_items.
B. Serving: 256 query items against the 1M items through the new method (host arrays returned) and through the old
   predict_similar_items (a [256, 1M] matrix to the host, argpartition + sorted per query), wall-clock ms per call.

No threshold is attached to any number.  Usage: python scripts/similar_items_bench.py [OUT_JSON]  (default
profiles/similar_items.json)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
import torch

import tensorrec_amd as T
from tensorrec_amd import recommendation_graphs as R
from tensorrec_amd.prediction_graphs import CosineSimilarityPredictionGraph
from tensorrec_amd.representation_graphs import LinearRepresentationGraph

NI, D, K = int(os.environ.get("NI", 1_000_000)), 128, 10
NQ = int(os.environ.get("NQ", 256))
ROUNDS = int(os.environ.get("ROUNDS", 3))


def model(n_users, n_items):
    m = T.TensorRec(n_components=D, prediction_graph=CosineSimilarityPredictionGraph(), user_repr_graph=LinearRepresentationGraph(),
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


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def differing_rows(m, itf, ids, vals, idx, exclude_self):
    """rows of (vals, idx) [len(ids), K] that differ from the dense rows' order (score desc, id asc)"""
    item_repr = torch.from_numpy(m.predict_item_representation(itf)).cuda()
    dense = R.predict_similar_items(m.prediction_graph_factory, item_repr, np.asarray(ids, np.int64)).cpu().numpy()
    bad = 0
    for r, q in enumerate(ids):
        row = dense[r]
        if exclude_self:
            row[q] = -np.inf
        t = np.partition(row, -K)[-K]
        c = np.nonzero(row >= t)[0]
        o = np.lexsort((c, -row[c]))[:K]
        bad += not (np.array_equal(idx[r], c[o].astype(np.int32)) and np.array_equal(vals[r], row[c[o]]))
    return bad


def main():
    out = {"device": torch.cuda.get_device_name(0), "items": NI, "d": D, "k": K, "graph": "cosine"}
    m = model(NI, NI)
    uf = itf = sp.identity(NI, dtype=np.float32, format="csr")
    rng = np.random.default_rng(0)
    calls = {
        "predict_top_k_users_x_items": lambda: m.predict_top_k(uf, itf, k=K, return_device=True, return_route=True),
        "similar_all_items": lambda: m.predict_similar_items_top_k(itf, k=K, return_device=True, return_route=True),
        "similar_all_items_exclude_self": lambda: m.predict_similar_items_top_k(itf, k=K, exclude_self=True, return_device=True,
                                                                                return_route=True),
    }
    for fn in calls.values():                                            # warm-up
        fn()
    times, last = {n: [] for n in calls}, {}
    for _ in range(ROUNDS):
        for n, fn in calls.items():
            ms, last[n] = timed(fn)
            times[n].append(ms)
    sample = np.sort(rng.choice(NI, 64, replace=False))
    a = {}
    for n in calls:
        v, i, rep = last[n]
        rec = {"ms_per_call": times[n], "ms_median": float(np.median(times[n])), "route": rep["route"],
               "user_batch_size": rep["user_batch_size"]}
        if "similar" in rep:
            rec.update(rep["similar"])
            rec["sampled_rows"] = len(sample)
            rec["sampled_rows_differing"] = differing_rows(m, itf, sample, v[sample].cpu().numpy(), i[sample].cpu().numpy(),
                                                           rep["similar"]["exclude_self"])
        a[n] = rec
        print(n, {k_: rec[k_] for k_ in rec if k_ != "ms_per_call"}, flush=True)
    out["A_whole_catalogue"] = a
    del last
    torch.cuda.empty_cache()

    ids = rng.integers(0, NI, NQ)
    b = {"query_items": NQ}
    m.predict_similar_items_top_k(itf, ids, k=K)
    m.predict_similar_items(itf, ids[:8], K)
    new_ms, old_ms = [], []
    for _ in range(ROUNDS):
        ms, (nv, ni, rep) = wall(lambda: m.predict_similar_items_top_k(itf, ids, k=K, return_route=True))
        new_ms.append(ms)
        ms, old = wall(lambda: m.predict_similar_items(itf, ids, K))
        old_ms.append(ms)
    b["predict_similar_items_top_k"] = {"wall_ms_per_call": new_ms, "wall_ms_median": float(np.median(new_ms)), "route": rep["route"],
                                        "rows_differing": differing_rows(m, itf, ids, nv, ni, False)}
    b["predict_similar_items"] = {"wall_ms_per_call": old_ms, "wall_ms_median": float(np.median(old_ms)),
                                  "rows_with_other_ids": int(sum([int(i) for i, _ in row] != ni[r].tolist()
                                                                 for r, row in enumerate(old)))}
    print("B", {n: (r["wall_ms_median"] if isinstance(r, dict) else r) for n, r in b.items()}, flush=True)
    out["B_serving_256_queries"] = b
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                             "profiles", "similar_items.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
