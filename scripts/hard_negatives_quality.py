"""The quality A/B of scripts/sampled_adjust_quality.py for dynamic negative sampling: BPR under uniform negatives against BPR under
HardNegativeSampler(n_candidates=4 S, n_hard=S // 2).  The same data (tensorrec_amd.synth.planted_cluster_interactions, a held-out
share of every user's pairs), identity features, the same epochs, learning rate and seed for both arms.  Metric: recall@k on the
held-out pairs (ranks among ALL items, training items not excluded).  One run per arm: a record, not a claim.

    python scripts/hard_negatives_quality.py --out profiles/hard_negatives_quality.json
"""
import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tensorrec_amd as T  # noqa: E402
from tensorrec_amd.eval import recall_at_k  # noqa: E402
from tensorrec_amd.loss_graphs import BPRLossGraph  # noqa: E402
from tensorrec_amd.synth import planted_cluster_interactions  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=6000)
    ap.add_argument("--items", type=int, default=3000)
    ap.add_argument("--clusters", type=int, default=32)
    ap.add_argument("--epochs", type=int, default=60)
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    train, held, _, _ = planted_cluster_interactions(args.users, args.items, n_clusters=args.clusters, per_user=20, seed=1, holdout=0.2)
    train, held = sp.csr_matrix(train), sp.csr_matrix(held)
    uf = sp.identity(args.users, dtype=np.float32, format="csr")
    itf = sp.identity(args.items, dtype=np.float32, format="csr")
    S = args.samples
    arms = {"uniform": T.DeviceSampler(1),
            "hard_4S_candidates_half_hard": T.HardNegativeSampler(n_candidates=4 * S, n_hard=S // 2, seed=1)}
    rec = {"what": "recall@k on held-out pairs, BPR, one fit per arm (scripts/hard_negatives_quality.py); no claim attached",
           "shape": {"n_users": args.users, "n_items": args.items, "clusters": args.clusters, "train_pairs": int(train.nnz),
                     "held_out_pairs": int(held.nnz), "epochs": args.epochs, "n_sampled": S, "n_candidates": 4 * S, "n_hard": S // 2,
                     "k": args.k, "n_components": 32, "learning_rate": 0.05},
           "recall_at_k": {}, "last_step_form": {}}
    for name, sampler in arms.items():
        model = T.TensorRec(n_components=32, loss_graph=BPRLossGraph(), seed=3, sampler=sampler)
        model.fit(train, uf, itf, epochs=args.epochs, learning_rate=0.05, n_sampled_items=S)
        ranks = model.predict_rank(uf, itf)
        rec["recall_at_k"][name] = float("%.4g" % np.nanmean(recall_at_k(ranks, held, k=args.k)))
        rec["last_step_form"][name] = model.last_step_form
    line = json.dumps(rec, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
