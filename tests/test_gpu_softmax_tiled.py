"""The tiled one-pass sampled-softmax step (csrc/softmax_tiled.hip, ops.softmax_tiled_step) against the float64 step of
tests/softmax_tiled_reference.py, per element and per output, within the bars derived there (tests/test_softmax_tiled_reference_host.py
shows on the CPU that float32 restatements lie inside them and seeded defects outside), and the route inside a TensorRec fit.

* kernel   trec_softmax_tiled_step itself: every instantiation <ITERS, RB, MODE, LPR, ADJ> (d in {4, 36, 64, 128, 256, 512} x dot /
           Euclidean x plain / hits / logQ table / logQ null table / both, with and without biases), S in {1, 255, 256, 257, 1023, 1025},
           a launch with more than 64 KB of LDS, rows of 0, non-positives only, 1, 255, 256, 257, 1,025 and 2,600 interactions, the planted
           users of softmax_tiled_reference.tiled_case, a dyadic family with exact dot scores; every output (loss, pred_serial, dU,
           d b_u, the values, the raw coefficients, the dense G and the row sums); exact zeros; two calls bit for bit (G apart);
* op       ops.softmax_tiled_step on both item-side routes, uncovered shapes, the step against ops.softmax_fused_step where both cover;
* model    one captured step against the float64 composition (dot with / without biases, cosine, Euclidean with biases) on a matrix
           with a 300-interaction user, and at S = 1,025; the kernel a fit reports; a 30-step fit; HIP-graph replay.

Tuning softmax_tiled is set by the fixture `tiled` and cleared in its finally.  The largest error / bar per output is kept in RATIOS;
with TREC_SOFTMAX_TILED_RATIOS_OUT=<file> it is written there at the end (profiles/softmax_tiled_reference_ratios.json)."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import softmax_step_reference as SR
import softmax_tiled_reference as R
from pair_reference import MODE_DOT, MODE_EUCLID, f64
from test_gpu_pair_kernels import check, dev, tunings
from test_gpu_softmax_fused import normalised, through_norm

pytestmark = pytest.mark.gpu

RATIOS = {}
TREC_ERR_UNSUPPORTED = 3                                # include/tensorrec_hip.h
MODES = [MODE_DOT, MODE_EUCLID]
MODE_IDS = ["dot", "euclid"]


@pytest.fixture(scope="module")
def ops():
    from tensorrec_amd import ops as _ops, _native
    _native.require_gpu()
    _native.load()
    yield _ops
    out = os.environ.get("TREC_SOFTMAX_TILED_RATIOS_OUT")
    if out:
        write_ratios(out)


@pytest.fixture(scope="module")
def N(ops):
    from tensorrec_amd import _native
    return _native


@pytest.fixture()
def tiled(N):
    """the opt-in route switched on for one test"""
    N.set_tuning("softmax_tiled", 1)
    try:
        yield
    finally:
        N.clear_tuning("softmax_tiled")


def write_ratios(path):
    """profiles/softmax_tiled_reference_ratios.json: the ratios of this run, merged (as maxima) into the record the file already holds"""
    rec = {"what": "largest |result - float64 reference| / bar per kernel variant (or route, or model configuration) and output over the "
                   "cases of tests/test_gpu_softmax_tiled.py (bars: tests/softmax_tiled_reference.py); a bar of 0 asks for equality and "
                   "records 0",
           "command": "TREC_SOFTMAX_TILED_RATIOS_OUT=<this file> python -m pytest -m gpu tests/test_gpu_softmax_tiled.py", "ratios": {}}
    if os.path.exists(path):
        with open(path) as f:
            rec["ratios"] = json.load(f).get("ratios", {})
    for k, r in RATIOS.items():
        for n, v in r.items():
            rec["ratios"].setdefault(k, {})[n] = max(rec["ratios"].get(k, {}).get(n, 0.0), float("%.4g" % v))
    rec["ratios"] = {k: dict(sorted(r.items())) for k, r in sorted(rec["ratios"].items())}
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


def held(key, name, got, want, bar, what):
    """check(), with the largest error / bar kept per key and output (a bar of 0 asks for equality); the figure is printed first"""
    g, w, b = f64(got).reshape(-1), f64(want).reshape(-1), f64(bar).reshape(-1)
    if g.shape == w.shape and g.size and np.isfinite(g).all():
        err = np.abs(g - w)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = float(np.where(err == 0, 0.0, err / b).max())
        RATIOS.setdefault(key, {})[name] = max(RATIOS.get(key, {}).get(name, 0.0), r)
        print("%s | %s | %s: error / bar %.4g" % (key, what, name, r))
    check(got, want, bar, "%s %s: %s" % (key, what, name))


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def interactions_of(case):
    from tensorrec_amd.sparse import Interactions
    inter = Interactions(case.matrix, case.n_users, case.n_items, "cuda")
    assert np.array_equal(inter.indptr.cpu().numpy(), case.indptr) and np.array_equal(inter.values.cpu().numpy(), case.values)
    assert np.array_equal(inter.x_item32.cpu().numpy(), case.x_item) and inter.max_row_nnz == case.max_pos
    return inter


def abi_step(N, case, inter, t, biased, temperature, variant, dense=False):
    """trec_softmax_tiled_step on device tensors `t`: every output it can write (dU and d b_u, or with `dense` G and the row sums; the
    raw coefficients for Euclidean scores with biases), NaN-filled first"""
    use_q, no_hits, lq = R.VARIANTS[variant]
    nu, ni, S, d = case.n_users, case.n_items, case.S, case.d
    raw = case.mode == MODE_EUCLID and biased
    ldg = (ni + 3) // 4 * 4
    o = SimpleNamespace(loss=nan(inter.n_positive), pred_serial=nan(inter.nnz), dU=None if dense else nan(nu, d), d_ub=nan(nu) if biased else None,
                        val_s=nan(nu, S), val_p=nan(inter.nnz), raw_s=nan(nu, S) if raw else None, raw_p=nan(inter.nnz) if raw else None,
                        G=torch.zeros((nu, ldg), dtype=torch.float32, device="cuda") if dense else None, rowsum=nan(nu) if dense else None)
    N.call("trec_softmax_tiled_step", N.ptr(t.U), N.ptr(t.V), N.ptr(t.ub) if biased else None, N.ptr(t.ib) if biased else None,
           N.ptr(inter.indptr), N.ptr(inter.x_item32), N.ptr(inter.pos_slot), N.ptr(t.samples), nu, ni, S, d, int(case.mode),
           int(inter.max_row_nnz), 1.0 / temperature, N.ptr(t.log_q) if lq == "case" else None, -float(np.log(ni)), int(use_q), int(no_hits),
           N.ptr(o.loss), N.ptr(o.pred_serial), N.ptr(o.dU), N.ptr(o.d_ub), N.ptr(o.val_s), N.ptr(o.val_p), N.ptr(o.raw_s), N.ptr(o.raw_p),
           N.ptr(o.G), ldg, N.ptr(o.rowsum))
    torch.cuda.synchronize()
    return SimpleNamespace(**{k: (v.cpu().numpy() if v is not None else None) for k, v in vars(o).items()})


def check_kernel(N, spec, mode, exact, runs, dense_runs=()):
    case = R.cached_case(spec, mode, exact)
    assert N.query("trec_softmax_tiled_lds_bytes", case.S, case.max_pos, case.d) == R.lds_bytes(case.S, case.max_pos, case.d) > 0
    inter = interactions_of(case)
    t = SimpleNamespace(U=dev(case.U), V=dev(case.V), ub=dev(case.ub), ib=dev(case.ib), samples=dev(case.samples), log_q=dev(case.log_q))
    nnz, nu, S = case.x_item.size, case.n_users, case.S
    pos = case.values > 0
    slot = np.cumsum(pos) - 1
    no_pos = [R.U_NONE, R.U_NONPOS]
    for variant, biased in runs:
        ref = R.cached_ref(spec, mode, exact, biased, R.TEMPERATURE, variant)
        got = abi_step(N, case, inter, t, biased, R.TEMPERATURE, variant)
        inst = R.instantiation(case.d, mode, variant)
        key = "kernel %s %s" % (MODE_IDS[mode], "plain" if not inst[4] else "adjusted")
        what = "S %d d %d rows %s <%d,%d,%d,%d,%d> %s %s bias %d" % ((case.S, case.d, case.rows) + inst + ("dyadic" if exact else "real", variant, biased))
        g_p, g_s = ref.g[:nnz], ref.g[nnz:].reshape(nu, S)
        wants = [("loss", got.loss, ref.loss, ref.b_loss), ("pred_serial", got.pred_serial, ref.pred_serial, ref.b_pred_serial),
                 ("dU", got.dU, ref.dU, ref.b_dU), ("val_pairs", got.val_p, ref.val[:nnz], ref.b_val[:nnz]),
                 ("val_samples", got.val_s, ref.val[nnz:], ref.b_val[nnz:])]
        if biased:
            wants.append(("d_ub", got.d_ub, ref.d_ub, ref.b_d_ub))
        if got.raw_s is not None:
            wants += [("raw_pairs", got.raw_p, g_p, ref.b_g[:nnz]), ("raw_samples", got.raw_s, g_s, ref.b_g[nnz:])]
        for name, a, w, b in wants:
            held(key, name, a, w, b, what)
        # the exact zeros of the contract: users without positives, non-positive interactions, hits, a user whose samples are all hits
        assert not got.dU[no_pos].any() and not got.val_s[no_pos].any() and (not biased or not got.d_ub[no_pos].any()), what
        assert not got.val_p[~pos].any() and np.isfinite(got.pred_serial).all(), what
        if R.VARIANTS[variant][1]:
            assert ref.hits.any() and not got.val_s[ref.hits].any(), what
            u = R.U_ALLHITS
            row = np.arange(case.indptr[u], case.indptr[u + 1])
            assert not got.dU[u].any() and not got.val_p[row].any() and not got.loss[slot[row[pos[row]]]].any(), what
        if mode == MODE_EUCLID:
            assert got.val_p[case.indptr[R.U_CLAMP + 1] - 1] == 0 and got.val_s[R.U_CLAMP, S - 1] == 0, what
        if exact:
            assert np.array_equal(got.pred_serial, ref.pred_serial.astype(np.float32)), what
        again = abi_step(N, case, inter, t, biased, R.TEMPERATURE, variant)
        for name in vars(got):
            a, b = getattr(got, name), getattr(again, name)
            assert (a is None and b is None) or np.array_equal(a, b), "two calls differ in %s (%s)" % (name, what)
        if (variant, biased) in dense_runs:
            dg = abi_step(N, case, inter, t, biased, R.TEMPERATURE, variant, dense=True)
            G, bG = R.dense_G(case, ref)
            held(key, "G", dg.G[:, :case.n_items], G, bG, what)
            held(key, "val_rowsum", dg.rowsum, ref.rowsum, ref.b_rowsum, what)
            assert not dg.G[:, case.n_items:].any()
            for name in ("loss", "pred_serial", "val_s", "val_p", "d_ub", "raw_s", "raw_p"):       # the second sweep is all that is skipped
                a, b = getattr(got, name), getattr(dg, name)
                assert (a is None and b is None) or np.array_equal(a, b), "%s differs with dense_g (%s)" % (name, what)


ALL_RUNS = [(v, b) for v in R.VARIANTS for b in (False, True)]
FEW_RUNS = [("plain", True), ("both", True), ("hits", False)]


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("spec", R.D_CASES, ids=lambda s: "S%d-d%d" % s[:2])
def test_every_instantiation_against_float64(N, spec, mode):
    check_kernel(N, spec, mode, False, ALL_RUNS, dense_runs=[("both", True), ("plain", False)])


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("spec", R.S_CASES, ids=lambda s: "S%d-d%d" % s[:2])
def test_sample_counts_at_the_stride_edges(N, spec, mode):
    check_kernel(N, spec, mode, False, FEW_RUNS + [("logq-uniform", True)])


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_long_rows(N, mode):
    """rows of 255, 256, 257, 1,025 and 2,600 interactions beside the short ones: several passes of 256 in the loss phase, a binary
    search through 2,600 columns per sample"""
    check_kernel(N, R.LONG_ROWS, mode, False, FEW_RUNS, dense_runs=[("both", True)])


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_more_than_64_kb_of_lds(N, mode):
    case = R.cached_case(R.BIG_LDS, mode)
    assert R.lds_bytes(case.S, case.max_pos, case.d) > 64 * 1024
    check_kernel(N, R.BIG_LDS, mode, False, [("plain", True), ("both", True)])


@pytest.mark.parametrize("spec", [R.D_CASES[3], R.S_CASES[3]], ids=lambda s: "S%d-d%d" % s[:2])
def test_dyadic_family_has_exact_scores(N, spec):
    """dot scores on multiples of 1/8 are exact in float32 in any order: pred_serial bit for bit, the loss phase alone within its bars"""
    check_kernel(N, spec, MODE_DOT, True, ALL_RUNS)


def test_planted_rows_are_what_they_mean():
    """with biases: the positive FAR above its samples has a loss that underflows towards 0, the one FAR below a loss of about FAR t;
    a hit that is the maximum leaves M with the kept samples -- read from the float64 reference the kernel is held to"""
    for mode in MODES:
        case = R.cached_case(R.D_CASES[1], mode)
        slot = np.cumsum(case.values > 0) - 1
        ref = R.cached_ref(R.D_CASES[1], mode, False, True, R.TEMPERATURE, "plain")
        assert ref.loss[slot[case.planted.above]] < 1e-30 and ref.loss[slot[case.planted.below]] >= R.FAR / R.TEMPERATURE
        both = R.cached_ref(R.D_CASES[1], mode, False, True, R.TEMPERATURE, "both")
        row = np.arange(case.indptr[R.U_HITMAX], case.indptr[R.U_HITMAX + 1])
        q = row[case.values[row] > 0]
        q = q[case.x_item[q] != case.hit_max]                        # (the lifted item's own interaction stands above every sample)
        assert both.hits[R.U_HITMAX, 0] and q.size >= 2 and (ref.loss[slot[q]] > both.loss[slot[q]] + 30.0).all()


# ------------------------------------------------------------------------------------------------ the op
def run_op(ops, case, inter, biased, temperature, variant, mode=None):
    use_q, no_hits, lq = R.VARIANTS[variant]
    out = ops.softmax_tiled_step(dev(case.U), dev(case.V), dev(case.ub) if biased else None, dev(case.ib) if biased else None, inter,
                                 dev(case.samples), temperature, sample_log_q=dev(case.log_q) if lq == "case" else None,
                                 log_q_correction=use_q, remove_accidental_hits=no_hits, mode=case.mode if mode is None else mode)
    torch.cuda.synchronize()
    return SimpleNamespace(**{k: (v.cpu().numpy() if v is not None else None) for k, v in zip(R.OP_RESULTS, out)})


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("spec", [R.D_CASES[1], R.D_CASES[3], R.S_CASES[5]], ids=lambda s: "S%d-d%d" % s[:2])
def test_op_on_both_item_side_routes(ops, N, spec, mode):
    """all six results of ops.softmax_tiled_step with the grouped gathers and with the dense-G GEMMs (fp32 operands: the split-bf16
    default holds gradients to 1e-4 of their terms, include/tensorrec_hip.h); the user side bit for bit between two calls"""
    case = R.cached_case(spec, mode)
    inter = interactions_of(case)
    for variant, biased in (("plain", False), ("both", True), ("hits", True)):
        ref = R.cached_ref(spec, mode, False, biased, R.TEMPERATURE, variant)
        what = "S %d d %d %s bias %d" % (case.S, case.d, variant, biased)
        with tunings(N, wmrb_dense_g=0):
            got = run_op(ops, case, inter, biased, R.TEMPERATURE, variant)
            assert ops.LAST_FUSED_STATS["route"] == "tiled+grouped"
            again = run_op(ops, case, inter, biased, R.TEMPERATURE, variant)
        assert (got.d_ub is None) == (not biased) and (got.d_ib is None) == (not biased)
        for name in R.OUTPUTS:
            if getattr(got, name) is not None:
                held("op grouped %s" % MODE_IDS[mode], name, getattr(got, name), getattr(ref, name), getattr(ref, "b_" + name), what)
        for name in ("loss", "pred_serial", "dU") + (("d_ub",) if biased else ()):
            assert np.array_equal(getattr(got, name), getattr(again, name)), "two calls differ in %s (%s)" % (name, what)
        with tunings(N, wmrb_dense_g=1, dense_g_split_bf16=0):
            dg = run_op(ops, case, inter, biased, R.TEMPERATURE, variant)
            assert ops.LAST_FUSED_STATS["route"] == "tiled+dense_g"
        bU, bV, bib = R.dense_bars(case, ref)
        bars = dict(loss=ref.b_loss, pred_serial=ref.b_pred_serial, dU=bU, dV=bV, d_ub=ref.b_d_ub, d_ib=bib)
        for name in R.OUTPUTS:
            if getattr(dg, name) is not None:
                held("op dense_g %s" % MODE_IDS[mode], name, getattr(dg, name), getattr(ref, name), bars[name], what)
        for name in ("loss", "pred_serial"):
            assert np.array_equal(getattr(got, name), getattr(dg, name)), name


def test_uncovered_shapes_return_unsupported(ops, N):
    lib = N.load()
    for S, L, d in R.UNCOVERED:
        assert N.query("trec_softmax_tiled_lds_bytes", S, L, d) == -1
        with tunings(N, softmax_tiled=1):
            assert not ops.softmax_tiled_supported(S, SimpleNamespace(max_row_nnz=L), d)
    case = R.cached_case(R.D_CASES[1], MODE_DOT)
    inter = interactions_of(case)
    nu, ni, S = case.n_users, case.n_items, case.S
    outs = [nan(inter.n_positive), nan(inter.nnz), nan(nu, 516), nan(nu), nan(nu, S), nan(inter.nnz)]
    wide_u, wide_v = nan(nu, 516), nan(ni, 516)
    code = lib.trec_softmax_tiled_step(N.ptr(wide_u), N.ptr(wide_v), N.ptr(dev(case.ub)), N.ptr(dev(case.ib)), N.ptr(inter.indptr),
                                       N.ptr(inter.x_item32), N.ptr(inter.pos_slot), N.ptr(dev(case.samples)), nu, ni, S, 516, 0,
                                       int(inter.max_row_nnz), 1.0, None, 0.0, 0, 0, N.ptr(outs[0]), N.ptr(outs[1]), N.ptr(outs[2]),
                                       N.ptr(outs[3]), N.ptr(outs[4]), N.ptr(outs[5]), None, None, None, 0, None, N.stream())
    torch.cuda.synchronize()
    assert code == TREC_ERR_UNSUPPORTED and b"not covered" in lib.trec_last_error()
    assert all(bool(torch.isnan(o).all()) for o in outs)              # nothing was launched


@pytest.mark.parametrize("variant", ["plain", "both"])
@pytest.mark.parametrize("spec", R.SHARED_WITH_FUSED, ids=lambda s: "S%d-L%d-d%d" % s)
def test_against_the_fused_step_where_both_cover(ops, N, spec, variant):
    """on the inputs of tests/softmax_step_reference.py: each step within its bars of the float64 step (the two references are the same
    numbers there: tests/test_softmax_tiled_reference_host.py), hence within the sum of the two bars of each other"""
    case = SR.cached_case(spec, False)
    inter = interactions_of(case)
    ref = SR.cached_ref(spec, False, True, 0.25, variant)
    use_q, no_hits, lq = SR.VARIANTS[variant]
    args = (dev(case.U), dev(case.V), dev(case.ub), dev(case.ib), inter, dev(case.samples), 0.25)
    kw = dict(sample_log_q=dev(case.log_q) if lq == "case" else None, log_q_correction=use_q, remove_accidental_hits=no_hits)
    assert ops.step_covers("softmax_fused", case.S, case.max_pos, case.d) and ops.step_covers("softmax_tiled", case.S, case.max_pos, case.d)
    fused = ops.softmax_fused_step(*args, **kw)
    with tunings(N, wmrb_dense_g=0):
        tiled_out = ops.softmax_tiled_step(*args, mode=MODE_DOT, **kw)
    torch.cuda.synchronize()
    for name, a, b in zip(SR.OP_RESULTS, tiled_out, fused):
        bar = getattr(ref, "b_" + name)
        held("op against fused", name, a.cpu().numpy(), getattr(ref, name), bar, "%s %s" % (spec, variant))
        check(a.cpu().numpy(), b.cpu().numpy(), 2.0 * f64(bar), "tiled against fused %s %s: %s" % (spec, variant, name))


# ------------------------------------------------------------------------------------------------ model level
N_USERS, N_ITEMS = 24, 400
MODEL_CONFIGS = {"dot-biased": ("dot", True, 8, 7), "dot-unbiased": ("dot", False, 8, 7), "cosine": ("cosine", True, 8, 7),
                 "euclid-biased": ("euclid", True, 8, 7), "dot-S1025": ("dot", True, 8, 1025), "euclid-S1025": ("euclid", True, 12, 1025)}


def model_data(S):
    """24 x 400 with a user of 300 interactions (beyond the fused step at any S), one without interactions, one with negative ones only"""
    rng = np.random.default_rng(23)
    dense = (rng.random((N_USERS, N_ITEMS)) < 0.03).astype(np.float32)
    dense *= np.where(rng.random(dense.shape) < 0.85, 1.0, -1.0).astype(np.float32)
    dense[0, :] = 0
    dense[0, rng.choice(N_ITEMS, size=300, replace=False)] = 1.0
    dense[0, np.flatnonzero(dense[0])[::9]] = -1.0
    dense[4, :] = 0                                   # a user without interactions
    dense[9, :] = -np.abs(dense[9, :])                # a user with negative interactions only
    dense[9, 3] = -1.0
    inter = sp.csr_matrix(dense)
    assert int(np.diff(inter.indptr).max()) == 300
    uf = sp.identity(N_USERS, dtype=np.float32, format="csr")
    itf = sp.identity(N_ITEMS, dtype=np.float32, format="csr")
    table = rng.integers(0, N_ITEMS, size=(N_USERS, S)).astype(np.int32)
    return inter, uf, itf, table


def make_model(T, kind, biased, d, options, sampler, temperature=0.5, graph=None, **kw):
    """options: accidental hits removed (the samplers used here are uniform: no logQ table)"""
    from tensorrec_amd.loss_graphs import SampledSoftmaxLossGraph
    from tensorrec_amd.prediction_graphs import (DotProductPredictionGraph, CosineSimilarityPredictionGraph,
                                                 EuclideanSimilarityPredictionGraph)
    graph = graph if graph is not None else SampledSoftmaxLossGraph(temperature, remove_accidental_hits=options)
    pred = {"dot": DotProductPredictionGraph, "cosine": CosineSimilarityPredictionGraph, "euclid": EuclideanSimilarityPredictionGraph}[kind]()
    return T.TensorRec(n_components=d, prediction_graph=pred, loss_graph=graph, biased=biased, seed=3, sampler=sampler, **kw)


def float64_model_step(N, w, inter, table, kind, biased, d, options, temperature):
    """(output, float64 value, bar) of one step from the weights: softmax_tiled_reference.ref_step on the tables the step is handed --
    the weights themselves (identity features) or, for cosine, their float32 normalised rows, whose backward is through_norm"""
    U, V = w["linear_weights_user_0"], w["linear_weights_item"]
    norms = None
    if kind == "cosine":
        (U, inv_u), (V, inv_v) = normalised(N, U), normalised(N, V)
        norms = (inv_u, inv_v)
    m = sp.csr_matrix(inter)
    case = SimpleNamespace(U=U, V=V, ub=w["user_feature_biases"].reshape(-1) if biased else None,
                           ib=w["item_feature_biases"].reshape(-1) if biased else None, indptr=m.indptr.astype(np.int64),
                           x_item=m.indices.astype(np.int32), values=m.data.astype(np.float32), samples=table, log_q=None, S=table.shape[1],
                           d=d, n_users=N_USERS, n_items=N_ITEMS, exact=False, mode=MODE_EUCLID if kind == "euclid" else MODE_DOT)
    ref = R.ref_step(case, biased, temperature, "hits" if options else "plain")
    dU, bU, dV, bV = ref.dU, ref.b_dU, ref.dV, ref.b_dV
    if norms is not None:
        dU, bU = through_norm(U, norms[0], dU, bU)
        dV, bV = through_norm(V, norms[1], dV, bV)
    wants = [("pred_serial", ref.pred_serial, ref.b_pred_serial), ("loss", ref.loss, ref.b_loss),
             ("d linear_weights_user_0", dU, bU), ("d linear_weights_item", dV, bV)]
    if biased:
        wants += [("d user_feature_biases", ref.d_ub, ref.b_d_ub), ("d item_feature_biases", ref.d_ib, ref.b_d_ib)]
    return wants, ref


def one_step(T, N, kind, biased, d, S, options):
    """one captured fit_partial step of the 24 x 400 model on the grouped item side (the reference's bars are the fp32 sums')"""
    inter, uf, itf, table = model_data(S)
    model = make_model(T, kind, biased, d, options, T.ReplaySampler([table]))
    model.build(N_USERS, N_ITEMS)
    w = model.get_weights()
    if biased:
        r2 = np.random.default_rng(7)
        w["user_feature_biases"] = (0.1 * r2.standard_normal(w["user_feature_biases"].shape)).astype(np.float32)
        w["item_feature_biases"] = (0.1 * r2.standard_normal(w["item_feature_biases"].shape)).astype(np.float32)
        model.set_weights(w)
    w = {k: v.copy() for k, v in model.get_weights().items()}
    model._capture = {}
    with tunings(N, wmrb_dense_g=0):
        model.fit_partial(inter, uf, itf, epochs=1, learning_rate=0.05, alpha=1e-4, n_sampled_items=S)
    return model, w, inter, table


@pytest.mark.parametrize("options", [False, True], ids=["plain", "hits-removed"])
@pytest.mark.parametrize("config", sorted(MODEL_CONFIGS))
def test_one_fit_step_against_float64(ops, N, tiled, config, options):
    """the tiled route inside a fit -- a 300-interaction user; Euclidean scores; S = 1,025 -- within the bars of the float64 composition"""
    import tensorrec_amd as T
    kind, biased, d, S = MODEL_CONFIGS[config]
    model, w, inter, table = one_step(T, N, kind, biased, d, S, options)
    assert model.last_step_form == "eager" and model.last_step_kernel == "softmax_tiled"
    assert ops.LAST_FUSED_STATS["route"] == "tiled+grouped"
    wants, ref = float64_model_step(N, w, inter, table, kind, biased, d, options, 0.5)
    if options:
        assert 0 < ref.hits.sum() < ref.hits.size
    for name, want, bar in wants:
        got = model._capture[name] if name in model._capture else model._capture["grads"][name[2:]]
        held("model %s" % config, name, np.asarray(got).reshape(-1), want, bar, "options %d" % options)


def test_which_kernel_a_fit_reports(ops, N):
    """with the switch on: the tiled kernel where the fused one does not cover the fit (a long row, Euclidean scores, S above 256), the
    fused one where it does, nothing for a subclass; with the switch off (the default): the generic step, as before"""
    import tensorrec_amd as T
    inter, uf, itf, table = model_data(7)
    short = sp.csr_matrix(inter.toarray()[1:])                      # without the 300-interaction user
    short_uf = sp.identity(N_USERS - 1, dtype=np.float32, format="csr")

    def fit(kind, rows=(inter, uf), S=7, graph=None):
        m = make_model(T, kind, True, 8, False, T.ReplaySampler([model_data(S)[3][:rows[0].shape[0]]]), graph=graph)
        m.fit_partial(rows[0], rows[1], itf, epochs=1, n_sampled_items=S)
        return m.last_step_kernel

    assert fit("dot") is None and fit("euclid") is None and fit("dot", S=1025) is None            # the default: off
    N.set_tuning("softmax_tiled", 1)
    try:
        assert fit("dot") == "softmax_tiled"                        # the longest row exceeds the fused coverage
        assert fit("dot", rows=(short, short_uf)) == "softmax_fused"
        assert fit("euclid", rows=(short, short_uf)) == "softmax_tiled" and fit("cosine") == "softmax_tiled"
        assert fit("dot", rows=(short, short_uf), S=1025) == "softmax_tiled"

        class Mine(T.loss_graphs.SampledSoftmaxLossGraph):         # a subclass may override anything: the generic step
            pass
        assert fit("dot", graph=Mine(0.5)) is None
        assert fit("dot", graph=T.loss_graphs.BPRLossGraph()) is None
    finally:
        N.clear_tuning("softmax_tiled")
    assert fit("dot") is None


def dummy(n_users=60, n_items=90, seed=3):
    import tensorrec_amd as T
    inter, uf, itf = T.util.generate_dummy_data(num_users=n_users, num_items=n_items, interaction_density=.08, num_user_features=40,
                                                num_item_features=50, n_features_per_user=6, n_features_per_item=7, random_state=seed)
    return sp.csr_matrix(inter), sp.csr_matrix(uf), sp.csr_matrix(itf)


def test_thirty_steps_lower_the_loss(ops, tiled):
    import tensorrec_amd as T
    inter, uf, itf = dummy()
    graph = T.loss_graphs.SampledSoftmaxLossGraph(0.5, log_q_correction=True, remove_accidental_hits=True)
    model = make_model(T, "euclid", True, 16, True, T.PopularitySampler(inter, power=0.75, smoothing=1.0, seed=5), graph=graph)
    means = []
    for _ in range(30):
        model._capture = {}
        model.fit_partial(inter, uf, itf, epochs=1, learning_rate=0.05, n_sampled_items=12)
        assert model.last_step_kernel == "softmax_tiled"
        means.append(float(np.asarray(model._capture["loss"]).mean()))
    model._capture = None
    assert np.isfinite(means).all() and means[-1] < means[0], means


def test_hip_graph_replay_equals_eager_steps(ops, tiled):
    """tests/test_gpu_softmax_fused.py::test_hip_graph_replay_equals_eager_steps on the tiled route (Euclidean scores): same tolerance,
    user biases left out for the reason given in tests/test_gpu_sampled_losses.py"""
    import tensorrec_amd as T
    inter, uf, itf = dummy()
    out = []
    for graphs in (True, False):
        model = make_model(T, "euclid", True, 16, False, None, hip_graphs=graphs)
        model.fit(inter, uf, itf, epochs=6, learning_rate=0.05, n_sampled_items=12)
        assert model.last_step_form == ("graph" if graphs else "eager") and model.last_step_kernel == "softmax_tiled"
        out.append((model.get_weights(), model._opt_step, model._sample_step))
    (wa, oa, sa), (wb, ob, sb) = out
    assert (oa, sa) == (ob, sb)
    for k in wa:
        if k != "user_feature_biases":
            assert np.allclose(wa[k], wb[k], rtol=1e-3, atol=2e-3), k
