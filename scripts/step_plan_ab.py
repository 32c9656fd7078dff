"""A/B record of the training-step route choice moving into tensorrec_amd/step_plan.py (host-side only): the same fits with the package
of the commit before and with this one, on one libtensorrec_hip.so, in one call on one box.

  python scripts/step_plan_ab.py run --tree <checkout> --out <run.json>      one run: per case the launch form, the step kernel, the
                                                                             grouping route and a SHA-256 of every weight array
                                                                             (the arrays go to <run>.npz), the per-step wall time and
                                                                             Python call count of the launch-bound eager fits,
                                                                             bench_records.config1_record
  python scripts/step_plan_ab.py merge <parent1> <head1> <parent2> <head2> --out profiles/step_plan_ab.json

Cases: one tiny fit per route (48 x 96, d = 8, S = 4, rows of at most 6 interactions -- those of tests/test_gpu_step_plan.py) and
BASELINE.json configs[1]; the generic, fused and tiled cases also with ``deterministic=True``, where equal bits mean something."""
import argparse
import cProfile
import hashlib
import json
import os
import pstats
import sys
import time

import numpy as np
import scipy.sparse as sp

N_USERS, N_ITEMS, D, S, LONGEST = 48, 96, 8, 4, 6
TIMED_EPOCHS = 300


def cases(T):
    LG, PG = T.loss_graphs, T.prediction_graphs
    softmax = lambda **kw: (lambda: LG.SampledSoftmaxLossGraph(0.5, **kw))    # noqa: E731
    base = {
        "wmrb_dot": (LG.WMRBLossGraph, dict(hip_graphs=False), False, 3),
        "wmrb_euclid": (LG.WMRBLossGraph, dict(hip_graphs=False, prediction_graph=PG.EuclideanSimilarityPredictionGraph()), False, 3),
        "softmax": (softmax(), dict(hip_graphs=False), False, 3),
        "softmax_shared": (softmax(shared_negatives=True), {}, False, 3),
        "softmax_shared_no_hits": (softmax(shared_negatives=True, remove_accidental_hits=True), {}, False, 3),
        "bpr": (LG.BPRLossGraph, dict(hip_graphs=False), False, 3),
        "wmrb_identity_users": (LG.WMRBLossGraph, {}, True, 3),
        "softmax_graph": (softmax(), dict(hip_graphs=True), False, 4),
    }
    for name in ("wmrb_dot", "wmrb_euclid", "softmax", "softmax_shared_no_hits", "bpr"):
        loss, options, identity, epochs = base[name]
        base[name + "_deterministic"] = (loss, dict(options, deterministic=True), identity, epochs)
    return base


def tiny_data(identity_users):
    rng = np.random.default_rng(5)
    dense = np.zeros((N_USERS, N_ITEMS), np.float32)
    for u in range(N_USERS):
        dense[u, rng.choice(N_ITEMS, size=1 + u % LONGEST, replace=False)] = 1.0
    uf = sp.identity(N_USERS, dtype=np.float32, format="csr")
    if not identity_users:
        uf = sp.hstack([uf, sp.csr_matrix((np.arange(N_USERS) % 3 == 0).astype(np.float32).reshape(-1, 1))], format="csr")
    return sp.csr_matrix(dense), uf, sp.identity(N_ITEMS, dtype=np.float32, format="csr")


def record(model, ops, arrays, name):
    weights = model.get_weights()
    for k, v in weights.items():
        arrays["%s/%s" % (name, k)] = v
    return {"last_step_form": model.last_step_form, "last_step_kernel": model.last_step_kernel,
            "grouping_route": ops.LAST_FUSED_STATS.get("route"),
            "sha256": {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in sorted(weights.items())}}


def run(tree, out):
    sys.path.insert(0, os.path.abspath(tree))
    import torch
    import tensorrec_amd as T
    from tensorrec_amd import ops
    import bench_records
    assert os.path.abspath(T.__file__).startswith(os.path.abspath(tree)), T.__file__
    result, arrays = {"tree": tree, "cases": {}}, {}
    for name, (loss, options, identity, epochs) in sorted(cases(T).items()):
        inter, uf, itf = tiny_data(identity)
        ops.LAST_FUSED_STATS.clear()
        model = T.TensorRec(n_components=D, loss_graph=loss(), seed=3, **options)
        model.fit(inter, uf, itf, epochs=epochs, learning_rate=0.05, n_sampled_items=S)
        rec = result["cases"][name] = record(model, ops, arrays, name)
        if options.get("hip_graphs") is False and not options.get("deterministic"):      # launch-bound eager steps: the host's share
            torch.cuda.synchronize()
            laps = []
            for _ in range(3):
                t0 = time.perf_counter()
                model.fit_partial(inter, uf, itf, epochs=TIMED_EPOCHS, learning_rate=0.05, n_sampled_items=S)
                torch.cuda.synchronize()
                laps.append(1e3 * (time.perf_counter() - t0) / TIMED_EPOCHS)
            rec["eager_ms_per_step"] = laps
            prof = cProfile.Profile()                  # (what the clock cannot resolve on a shared box: the host's work as a count)
            prof.enable()
            model.fit_partial(inter, uf, itf, epochs=100, learning_rate=0.05, n_sampled_items=S)
            prof.disable()
            rec["python_calls_per_step"] = pstats.Stats(prof).total_calls / 100.0
            assert model.last_step_form == "eager"
    # BASELINE.json configs[1] (943 x 1682, d = 64, S = 168): labels and hashes of a 3-epoch fit, then the bench record's fit figure
    rng = np.random.default_rng(0)
    inter = bench_records._zipf_interactions(943, 1682, 160, rng, exponent=1.0)
    uf, itf = sp.identity(943, dtype=np.float32, format="csr"), bench_records._side_features(1682, 19, 3, rng)
    ops.LAST_FUSED_STATS.clear()
    model = T.TensorRec(n_components=64, loss_graph=T.loss_graphs.WMRBLossGraph(), seed=0)
    model.fit(inter, uf, itf, epochs=3, learning_rate=0.05, n_sampled_items=168)
    result["cases"]["config1"] = record(model, ops, arrays, "config1")
    bench = bench_records.config1_record("cuda")
    result["bench_config1"] = {k: bench.get(k) for k in ("ms_per_epoch", "fit_epochs_per_sec", "step_form") if k in bench}
    np.savez(os.path.splitext(out)[0] + ".npz", **arrays)
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
    print(json.dumps({name: (c["last_step_form"], c["last_step_kernel"], c["grouping_route"]) for name, c in result["cases"].items()}))


def merge(paths, out):
    """paths: parent1 head1 parent2 head2, the order the runs were made in."""
    runs = [json.load(open(p)) for p in paths]
    arrays = [np.load(os.path.splitext(p)[0] + ".npz") for p in paths]
    p1, h1, p2, h2 = runs
    a_p1, a_h1, a_p2, a_h2 = arrays
    labels = ("last_step_form", "last_step_kernel", "grouping_route")

    def max_abs(a, b, name):
        return max(float(np.abs(a[k] - b[k]).max()) for k in a.files if k.startswith(name + "/"))
    table = {}
    for name in sorted(h1["cases"]):
        c1, c2, ch, ch2 = p1["cases"][name], p2["cases"][name], h1["cases"][name], h2["cases"][name]
        row = {k: ch[k] for k in labels}
        row["labels_equal_parent"] = all(c1[k] == c2[k] == ch[k] == ch2[k] for k in labels)
        row["parent_reproduces_its_hashes"] = c1["sha256"] == c2["sha256"]
        if row["parent_reproduces_its_hashes"]:
            row["head_hashes_equal_parent"] = ch["sha256"] == c1["sha256"] and ch2["sha256"] == c1["sha256"]
        else:
            row["note"] = ("the parent's two runs differ (atomic-ordered sums / graph replay): compared by "
                           "the largest weight difference.  Adam divides by the gradient's own size, so a weight whose gradient is "
                           "rounding noise moves by up to the learning rate per step whichever way the noise points: differences up to "
                           "2 x 0.05 x epochs say nothing; the deterministic twin of the case is the bitwise check")
            row["max_abs_parent_vs_parent"] = max_abs(a_p1, a_p2, name)
            row["max_abs_head_vs_head"] = max_abs(a_h1, a_h2, name)
            row["max_abs_head_vs_parent"] = max(max_abs(h, p, name) for h in (a_h1, a_h2) for p in (a_p1, a_p2))
        if "eager_ms_per_step" in ch:                 # (laps of 300 steps each; later laps cost more on both sides: the float32 beta
            k = "eager_ms_per_step"                   # powers are multiplied out from 1 every eager step)
            row[k] = {"parent1": c1[k], "head1": ch[k], "parent2": c2[k], "head2": ch2[k]}
            row["eager_ms_head_within_parent_laps_or_better"] = [min(a, b) <= max(x, y) for a, b, x, y in zip(ch[k], ch2[k], c1[k], c2[k])]
            row["python_calls_per_step"] = {"parent1": c1.get("python_calls_per_step"), "head1": ch.get("python_calls_per_step"),
                                            "parent2": c2.get("python_calls_per_step"), "head2": ch2.get("python_calls_per_step")}
        table[name] = row
    bench = {"parent1": p1["bench_config1"], "head1": h1["bench_config1"], "parent2": p2["bench_config1"], "head2": h2["bench_config1"]}
    spread = sorted(b["ms_per_epoch"] for b in (p1["bench_config1"], p2["bench_config1"]))
    bench["parent_ms_per_epoch_range"] = spread
    bench["head_within_parent_range_or_better"] = min(h["bench_config1"]["ms_per_epoch"] for h in (h1, h2)) <= spread[1]
    result = {"what": "parent / head / parent / head of the Python package (one libtensorrec_hip.so) in one call on one MI355X: the "
                      "training step's route choice moved into step_plan.py against the commit before; the change is host-side only",
              "command": "python scripts/step_plan_ab.py run --tree <checkout> --out <run.json> (four times), then merge",
              "caching": "none: the plan is asked once per step, as the predicates were",
              "cases": table, "bench_config1_fit": bench,
              "all_labels_equal": all(r["labels_equal_parent"] for r in table.values()),
              "all_reproducible_hashes_equal": all(r.get("head_hashes_equal_parent", True) for r in table.values())}
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
    print(json.dumps({k: result[k] for k in ("all_labels_equal", "all_reproducible_hashes_equal")}))
    print(json.dumps({n: (r["eager_ms_per_step"], r["python_calls_per_step"]) for n, r in table.items() if "eager_ms_per_step" in r}))
    print(json.dumps(bench))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["run", "merge"])
    ap.add_argument("paths", nargs="*")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    run(args.tree, args.out) if args.mode == "run" else merge(args.paths, args.out)
