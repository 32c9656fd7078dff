"""A/B record of the sampled-loss family moving onto one copy of what it shares (csrc/sampled_common.hpp, the host section of
csrc/user_fused_body.hpp, the gather helpers of ops_base.py): the same calls with the tree of the commit before (its own package and
its own libtensorrec_hip.so) and with this one, in one call on one box.

  python scripts/step_family_ab.py run --tree <checkout> --out <run.json>    one run: every case twice, a SHA-256 of every returned
                                                                             array; the per-step wall time of the launch-bound eager
                                                                             tiny fits, as scripts/step_plan_ab.py measures them
  python scripts/step_family_ab.py merge <parent1> <head1> <parent2> <head2> --out profiles/step_family_ab.json
                                         [--kernel-timings <label>:<call>,<call> <parent1> <head1> <parent2> <head2>] ...
                                                                             per-kernel timings to judge and carry along: the raw
                                                                             records of one bench script (scripts/warp_loss_bench.py,
                                                                             scripts/sampled_adjust_bench.py) run with the library of
                                                                             the parent and of the head in turn (TREC_HIP_LIB), in the
                                                                             order given; <call>: the timed calls whose kernels
                                                                             changed (the others are controls); may be repeated

The acceptance rule for a time, per-step or per-kernel: the head's mean is not above the parent's mean by more than the two parent runs
differ from each other.

Cases, each called directly through ``ops`` under ops.deterministic_grouping(): 48 x 96, d = 8, S = 4, rows of 1..6 interactions (the
shape of tests/test_gpu_step_plan.py); every fifth interaction carries a non-positive value (pos_slot = -1); in every third user's
table slot 0 is one of the user's positives (a hit) and, where there is one, slot 1 the item of a non-positive interaction (no hit)."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import step_plan_ab as SP  # noqa: E402

N_USERS, N_ITEMS, D, S, LONGEST = SP.N_USERS, SP.N_ITEMS, SP.D, SP.S, SP.LONGEST
S_SHARED, S_WORKGROUP = 65, 300


def data(n_sampled):
    """(interaction matrix, U, V, ub, ib, samples [U, n_sampled], log q [n_items])"""
    rng = np.random.default_rng(11)
    rows, cols, vals = [], [], []
    samples = rng.integers(0, N_ITEMS, size=(N_USERS, n_sampled)).astype(np.int32)
    k = 0
    for u in range(N_USERS):
        items = np.sort(rng.choice(N_ITEMS, size=1 + u % LONGEST, replace=False))
        value = np.ones(len(items), np.float32)
        for j in range(len(items)):
            k += 1
            if k % 5 == 0 and len(items) > 1:
                value[j] = -1.0
        if not (value > 0).any():
            value[0] = 1.0
        if u % 3 == 0:
            samples[u, 0] = items[value > 0][0]
            if (value <= 0).any() and n_sampled > 1:
                samples[u, 1] = items[value <= 0][0]
        rows += [u] * len(items)
        cols += list(items)
        vals += list(value)
    matrix = sp.csr_matrix((np.array(vals, np.float32), (rows, cols)), shape=(N_USERS, N_ITEMS))
    f = lambda *shape: (0.5 * rng.standard_normal(shape)).astype(np.float32)    # noqa: E731
    q = rng.random(N_ITEMS) + 0.1
    return matrix, f(N_USERS, D), f(N_ITEMS, D), f(N_USERS), f(N_ITEMS), samples, np.log(q / q.sum()).astype(np.float32)


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def step_cases(ops, torch, Interactions):
    matrix, U, V, ub, ib, samples, log_q = data(S)
    dev = lambda a: torch.from_numpy(a).cuda()    # noqa: E731
    inter = Interactions(matrix, N_USERS, N_ITEMS, "cuda")
    u, v, bu, bi, sm, lq = dev(U), dev(V), dev(ub), dev(ib), dev(samples), dev(log_q)
    shared = dev(np.random.default_rng(12).integers(0, N_ITEMS, size=S_SHARED).astype(np.int32))
    out = {"wmrb_fused": lambda: ops.wmrb_fused_step(u, v, bu, bi, inter, sm),
           "wmrb_fused_balanced": lambda: ops.wmrb_fused_step(u, v, bu, bi, inter, sm, balanced=True)}
    for name, kw in (("", {}), ("_logq", dict(sample_log_q=lq, log_q_correction=True)), ("_no_hits", dict(remove_accidental_hits=True)),
                     ("_logq_no_hits", dict(sample_log_q=lq, log_q_correction=True, remove_accidental_hits=True))):
        out["softmax_fused" + name] = lambda kw=kw: ops.softmax_fused_step(u, v, bu, bi, inter, sm, 0.5, **kw)
    out["warp_fused"] = lambda: ops.warp_fused_step(u, v, bu, bi, inter, sm, return_first=True)
    out["warp_fused_no_hits"] = lambda: ops.warp_fused_step(u, v, bu, bi, inter, sm, remove_accidental_hits=True, return_first=True)
    out["softmax_shared"] = lambda: ops.softmax_shared_step(u, v, bu, bi, inter, shared, 0.5)
    out["softmax_shared_logq"] = lambda: ops.softmax_shared_step(u, v, bu, bi, inter, shared, 0.5, sample_log_q=lq, log_q_correction=True)
    out["softmax_full"] = lambda: ops.softmax_full_step(u, v, bu, bi, inter, 0.5)
    return out


def loss_cases(ops, torch, Interactions, n_sampled):
    """forward and backward of every loss kernel pair: (loss, d pred_serial, d sample_pred)"""
    matrix, _, _, _, _, samples, log_q = data(n_sampled)
    inter = Interactions(matrix, N_USERS, N_ITEMS, "cuda")
    rng = np.random.default_rng(13)
    dev = lambda a: torch.from_numpy(a).cuda()    # noqa: E731
    pred = dev(rng.standard_normal(inter.nnz).astype(np.float32))
    samp = dev(rng.standard_normal((N_USERS, n_sampled)).astype(np.float32))
    go = dev((rng.random(inter.n_positive) + 0.5).astype(np.float32))
    items, lq = dev(samples), dev(log_q)
    hits = dict(sample_items=items, remove_accidental_hits=True)
    losses = {"wmrb": lambda p, s: ops.wmrb_loss(p, s, inter), "wmrb_balanced": lambda p, s: ops.wmrb_loss(p, s, inter, balanced=True),
              "sampled_softmax": lambda p, s: ops.sampled_softmax_loss(p, s, inter, 0.5),
              "sampled_softmax_logq": lambda p, s: ops.sampled_softmax_loss(p, s, inter, 0.5, sample_items=items, sample_log_q=lq,
                                                                            log_q_correction=True),
              "sampled_softmax_no_hits": lambda p, s: ops.sampled_softmax_loss(p, s, inter, 0.5, **hits),
              "sampled_softmax_logq_no_hits": lambda p, s: ops.sampled_softmax_loss(p, s, inter, 0.5, sample_log_q=lq,
                                                                                    log_q_correction=True, **hits),
              "bpr": lambda p, s: ops.bpr_loss(p, s, inter), "bpr_no_hits": lambda p, s: ops.bpr_loss(p, s, inter, **hits),
              "warp": lambda p, s: ops.warp_loss(p, s, inter), "warp_no_hits": lambda p, s: ops.warp_loss(p, s, inter, **hits)}

    def both(fn):
        p, s = pred.clone().requires_grad_(True), samp.clone().requires_grad_(True)
        loss = fn(p, s)
        return (loss,) + torch.autograd.grad(loss, (p, s), grad_outputs=go)
    return {"%s_loss_S%d" % (name, n_sampled): (lambda fn=fn: both(fn)) for name, fn in losses.items()}


def run(tree, out):
    sys.path.insert(0, os.path.abspath(tree))
    import torch
    import tensorrec_amd as T
    from tensorrec_amd import ops, _native
    from tensorrec_amd.sparse import Interactions
    assert os.path.abspath(T.__file__).startswith(os.path.abspath(tree)), T.__file__
    assert os.path.abspath(_native.LIB_PATH).startswith(os.path.abspath(tree)), _native.LIB_PATH
    result = {"tree": tree, "library": os.path.relpath(_native.LIB_PATH, os.path.abspath(tree)), "cases": {}, "eager_ms_per_step": {}}
    cases = step_cases(ops, torch, Interactions)
    cases.update(loss_cases(ops, torch, Interactions, S))
    cases.update(loss_cases(ops, torch, Interactions, S_WORKGROUP))
    with ops.deterministic_grouping():
        for name, fn in sorted(cases.items()):
            result["cases"][name] = [[sha(t) for t in fn() if t is not None] for _ in range(2)]
    # the launch-bound eager tiny fits of scripts/step_plan_ab.py: the host's share of a step
    for name, (loss, options, identity, epochs) in sorted(SP.cases(T).items()):
        if options.get("hip_graphs") is not False or options.get("deterministic"):
            continue
        inter, uf, itf = SP.tiny_data(identity)
        model = T.TensorRec(n_components=D, loss_graph=loss(), seed=3, **options)
        model.fit(inter, uf, itf, epochs=epochs, learning_rate=0.05, n_sampled_items=S)
        torch.cuda.synchronize()
        laps = []
        for _ in range(3):
            t0 = time.perf_counter()
            model.fit_partial(inter, uf, itf, epochs=SP.TIMED_EPOCHS, learning_rate=0.05, n_sampled_items=S)
            torch.cuda.synchronize()
            laps.append(1e3 * (time.perf_counter() - t0) / SP.TIMED_EPOCHS)
        assert model.last_step_form == "eager"
        result["eager_ms_per_step"][name] = laps
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
    print(json.dumps({"cases": len(result["cases"]), "eager_ms_per_step": result["eager_ms_per_step"]}))


def kernel_timing(label, paths):
    """the records of one bench script (parent1 head1 parent2 head2), one row per timed call.  ``label`` is "<name>:<call>,<call>": the
    calls whose kernels changed stand under the acceptance rule; the others run the same device code in both libraries and show what
    two builds of one kernel differ by on the box (``control``)."""
    judged = label.split(":")[1].split(",")
    recs = [json.load(open(p)) for p in paths]
    assert all(name in recs[0]["ms"] for name in judged), (judged, sorted(recs[0]["ms"]))
    rows = {}
    for name in sorted(recs[0]["ms"]):
        med = [r["ms"][name]["median"] for r in recs]
        slower_by = 0.5 * (med[1] + med[3]) - 0.5 * (med[0] + med[2])
        rows[name] = {"median_ms": dict(zip(("parent1", "head1", "parent2", "head2"), med)), "head_slower_by_ms": slower_by,
                      "parent_runs_differ_by_ms": abs(med[0] - med[2])}
        if name in judged:
            rows[name]["accepted"] = slower_by <= abs(med[0] - med[2])
        else:
            rows[name]["control"] = "the same device code in both libraries"
    return {"shape": recs[0].get("shape"), "remove_hits": recs[0].get("remove_hits"), "ms": rows}


def merge(paths, out, kernel_timings):
    """paths: parent1 head1 parent2 head2, the order the runs were made in."""
    p1, h1, p2, h2 = [json.load(open(p)) for p in paths]
    table = {}
    for name in sorted(p1["cases"]):
        parent = p1["cases"][name] + p2["cases"][name]
        head = h1["cases"][name] + h2["cases"][name]
        row = {"arrays": len(parent[0]), "parent_reproduces_its_hashes": all(r == parent[0] for r in parent)}
        if row["parent_reproduces_its_hashes"]:
            row["head_hashes_equal_parent"] = all(r == parent[0] for r in head)
        row["sha256_head"] = head[0]
        table[name] = row
    eager = {}
    for name in sorted(p1["eager_ms_per_step"]):
        best = [min(r["eager_ms_per_step"][name]) for r in (p1, h1, p2, h2)]          # (the fastest lap of three per run)
        slower_by = 0.5 * (best[1] + best[3]) - 0.5 * (best[0] + best[2])
        eager[name] = {"laps": {"parent1": p1["eager_ms_per_step"][name], "head1": h1["eager_ms_per_step"][name],
                                "parent2": p2["eager_ms_per_step"][name], "head2": h2["eager_ms_per_step"][name]},
                       "head_slower_by_ms": slower_by, "parent_runs_differ_by_ms": abs(best[0] - best[2]),
                       "accepted": slower_by <= abs(best[0] - best[2])}
    result = {"what": "parent / head / parent / head, each tree with its own package and its own libtensorrec_hip.so, in one call on one "
                      "MI355X: the sampled-loss kernels and one-pass steps on one copy of what they share against the commit before",
              "command": "python scripts/step_family_ab.py run --tree <checkout> --out <run.json> (four times), then merge",
              "libraries": ["%s of %s" % (r["library"], "the parent" if r is p1 or r is p2 else "the head") for r in (p1, h1, p2, h2)], "cases": table, "eager_ms_per_step": eager,
              "every_parent_case_reproduces": all(r["parent_reproduces_its_hashes"] for r in table.values()),
              "all_hashes_equal": all(r.get("head_hashes_equal_parent", False) for r in table.values()),
              "all_eager_accepted": all(r["accepted"] for r in eager.values())}
    if kernel_timings:
        result["kernel_timings"] = {"what": "forward + backward call times in ms (the median of each bench run's rounds), the parent's "
                                            "and the head's library in turn (TREC_HIP_LIB) under one bench script per label",
                                    "labels": {g[0].split(":")[0]: kernel_timing(g[0], g[1:]) for g in kernel_timings}}
        result["all_kernel_timings_accepted"] = all(r.get("accepted", True) for t in result["kernel_timings"]["labels"].values()
                                                    for r in t["ms"].values())
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
    print(json.dumps({k: result[k] for k in ("every_parent_case_reproduces", "all_hashes_equal", "all_eager_accepted",
                                             "all_kernel_timings_accepted") if k in result}))
    for label, t in result.get("kernel_timings", {}).get("labels", {}).items():
        print(label, json.dumps({n: (r["head_slower_by_ms"], r["parent_runs_differ_by_ms"], r.get("accepted", "control")) for n, r in t["ms"].items()}))
    print(json.dumps({n: (r["head_slower_by_ms"], r["parent_runs_differ_by_ms"]) for n, r in eager.items()}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["run", "merge"])
    ap.add_argument("paths", nargs="*")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--kernel-timings", nargs=5, action="append", metavar=("LABEL", "PARENT1", "HEAD1", "PARENT2", "HEAD2"))
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    run(args.tree, args.out) if args.mode == "run" else merge(args.paths, args.out, args.kernel_timings)
