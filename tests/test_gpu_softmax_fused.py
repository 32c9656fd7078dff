"""The one-pass sampled-softmax step (csrc/softmax_fused.hip, ops.softmax_fused_step) against the float64 step of
tests/softmax_step_reference.py, per element and per output, within the bars derived there (tests/test_softmax_step_reference_host.py
shows on the CPU that a float32 restatement lies inside them and seeded defects outside), and the route inside a TensorRec fit.

* kernel   every instantiation <ITERS, RMAX, SURE> at the smallest shapes that reach each edge (rows at the register capacity, d with
           zeroed columns), plain and adjusted, with and without biases, temperatures 1 and 0.25, real-valued tables and dyadic ones
           (exact scores: the loss phase alone); the planted rows of softmax_step_reference.softmax_case; exact zeros; repeats bit for
           bit; the ABI's histogram and ranks, its coverage answer and its argument checks;
* model    one captured step against the float64 composition (dot with / without biases, cosine; plain, and both options under a
           PopularitySampler), the generic route beside it, which kernel a fit reports, a 30-step fit, HIP-graph replay.

The largest error / bar per output is kept in RATIOS; with TREC_SOFTMAX_FUSED_RATIOS_OUT=<file> it is written there at the end
(profiles/softmax_fused_reference_ratios.json)."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import softmax_step_reference as R
from pair_reference import MODE_DOT, MODE_EUCLID, U32, f64
from test_gpu_pair_kernels import check, dev, tunings

pytestmark = pytest.mark.gpu

RATIOS = {}
TREC_ERR_INVALID, TREC_ERR_UNSUPPORTED = 1, 3          # include/tensorrec_hip.h


@pytest.fixture(scope="module")
def ops():
    from tensorrec_amd import ops as _ops, _native
    _native.require_gpu()
    _native.load()
    yield _ops
    out = os.environ.get("TREC_SOFTMAX_FUSED_RATIOS_OUT")
    if out:
        write_ratios(out)


@pytest.fixture(scope="module")
def N(ops):
    from tensorrec_amd import _native
    return _native


def write_ratios(path):
    """profiles/softmax_fused_reference_ratios.json: the ratios of this run, merged (as maxima) into the record the file already holds"""
    rec = {"what": "largest |result - float64 reference| / bar per kernel variant (or model configuration) and output over the cases of "
                   "tests/test_gpu_softmax_fused.py (bars: tests/softmax_step_reference.py); a bar of 0 asks for equality and records 0",
           "command": "TREC_SOFTMAX_FUSED_RATIOS_OUT=<this file> python -m pytest -m gpu tests/test_gpu_softmax_fused.py", "ratios": {}}
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
    """check(), with the largest error / bar kept per key and output (a bar of 0 asks for equality)"""
    g, w, b = f64(got).reshape(-1), f64(want).reshape(-1), f64(bar).reshape(-1)
    if g.shape == w.shape and g.size and np.isfinite(g).all():
        err = np.abs(g - w)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = float(np.where(err == 0, 0.0, err / b).max())
        RATIOS.setdefault(key, {})[name] = max(RATIOS.get(key, {}).get(name, 0.0), r)
    check(got, want, bar, "%s %s: %s" % (key, what, name))


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def interactions_of(case):
    from tensorrec_amd.sparse import Interactions
    inter = Interactions(case.matrix, case.n_users, case.n_items, "cuda")
    assert np.array_equal(inter.indptr.cpu().numpy(), case.indptr) and np.array_equal(inter.values.cpu().numpy(), case.values)
    assert np.array_equal(inter.x_item32.cpu().numpy(), case.x_item) and inter.max_row_nnz == case.max_pos
    return inter


def run_step(ops, case, inter, biased, temperature, variant):
    use_q, no_hits, lq = R.VARIANTS[variant]
    out = ops.softmax_fused_step(dev(case.U), dev(case.V), dev(case.ub) if biased else None, dev(case.ib) if biased else None, inter,
                                 dev(case.samples), temperature, sample_log_q=dev(case.log_q) if lq == "case" else None,
                                 log_q_correction=use_q, remove_accidental_hits=no_hits)
    torch.cuda.synchronize()
    return SimpleNamespace(**{k: (v.cpu().numpy() if v is not None else None) for k, v in zip(R.OP_RESULTS, out)})


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("exact", [False, True], ids=["real", "dyadic"])
@pytest.mark.parametrize("spec", R.GPU_CASES, ids=lambda s: "S%d-L%d-d%d" % s)
def test_fused_step_against_float64(ops, N, spec, exact):
    """all six results of ops.softmax_fused_step for every variant, with and without biases, at both temperatures; the exact zeros of
    the contract; user-side outputs of a second call bit for bit, item-side ones under the deterministic grouping"""
    case = R.cached_case(spec, exact)
    inst = R.instantiation(case.S, case.max_pos, case.d)
    assert inst is not None and N.query("trec_softmax_fused_lds_bytes", case.S, case.max_pos, case.d) == R.lds_bytes(case.S, case.max_pos, case.d)
    assert N.query("trec_softmax_fused_lds_bytes", case.S, R.rows_capacity(case.d) - case.S + 1, case.d) == -1
    inter = interactions_of(case)
    assert ops.softmax_fused_supported(case.S, inter, case.d)
    pos = case.values > 0
    no_pos = [R.U_NONE, R.U_NONPOS]
    for variant in R.VARIANTS:
        for biased in (False, True):
            for T in R.TEMPERATURES:
                ref = R.cached_ref(spec, exact, biased, T, variant)
                got = run_step(ops, case, inter, biased, T, variant)
                assert ops.LAST_FUSED_STATS["route"] == "ranked"
                what = "%s <%d,%d,%d> %s bias %d T %g" % ((spec,) + inst + ("dyadic" if exact else "real", biased, T))
                assert (got.d_ub is None) == (not biased) and (got.d_ib is None) == (not biased)
                key = "fused %s" % ("plain" if variant == "plain" else "adjusted")
                for name in R.OUTPUTS:
                    if getattr(got, name) is not None:
                        held(key, name, getattr(got, name), getattr(ref, name), getattr(ref, "b_" + name), "%s %s" % (what, variant))
                assert not got.dU[no_pos].any() and (not biased or not got.d_ub[no_pos].any())
                if R.VARIANTS[variant][1]:
                    # hits: a user whose samples are all hits; item rows whose terms are all exact zeros
                    assert not got.dU[R.U_ALLHITS].any()
                    sl = (np.cumsum(pos) - 1)[case.indptr[R.U_ALLHITS]:case.indptr[R.U_ALLHITS + 1]]
                    assert not got.loss[sl[pos[case.indptr[R.U_ALLHITS]:case.indptr[R.U_ALLHITS + 1]]]].any()
                    zero_rows = ~ref.b_dV.any(1) & ~ref.dV.any(1)
                    assert not got.dV[zero_rows].any()
    # two more calls of one variant: the same bits
    with ops.deterministic_grouping(True):
        a = run_step(ops, case, inter, True, 0.25, "both")
        b = run_step(ops, case, inter, True, 0.25, "both")
    c = run_step(ops, case, inter, True, 0.25, "both")
    for name in R.OUTPUTS:
        assert np.array_equal(getattr(a, name), getattr(b, name)), "two deterministic calls differ in %s" % name
    for name in ("loss", "pred_serial", "dU", "d_ub"):
        assert np.array_equal(getattr(a, name), getattr(c, name)), "two calls differ in %s" % name


def test_a_hit_has_a_coefficient_of_exactly_zero(ops):
    """an item that one user samples (a hit there) and nobody else touches but through that user's own interaction: its d item_in row is
    the interaction's term alone -- coefficient of the pair times the user's row, one product per entry -- and the sample adds an exact 0"""
    spec = (7, 20, 36)
    case = R.cached_case(spec, False)
    inter = interactions_of(case)
    u = R.U_NONPOS_ITEM
    item = case.hit_item
    assert item == case.samples[u, 1] and (case.samples == item).sum() == 1 and (case.x_item == item).sum() == 1
    k = int(np.flatnonzero(case.x_item == item)[0])
    assert case.indptr[u] <= k < case.indptr[u + 1] and case.values[k] > 0
    got = run_step(ops, case, inter, True, 1.0, "hits")
    ref = R.cached_ref(spec, False, True, 1.0, "hits")
    assert ref.hits[u, 1]
    g = got.d_ib[item]                                            # the pair's coefficient: the only term of the item's bias gradient
    assert g < 0 and np.array_equal(got.dV[item], (np.float32(g) * case.U[u]).astype(np.float32))
    plain = run_step(ops, case, inter, True, 1.0, "plain")
    assert plain.d_ib[item] != g                                  # without the option the sample is a negative with a coefficient


def test_planted_rows_are_what_they_mean(ops):
    """with biases: the positive FAR above its samples has a loss that underflows towards 0 and a vanishing coefficient, the one FAR below
    a loss of about FAR t, the positive equal to M a loss of log(1 + Z) with a = b = 1 -- read from the float64 reference the kernel
    is held to, so that the plants are known to be in force"""
    spec = (33, 20, 128)
    for exact in (False, True):
        case = R.cached_case(spec, exact)
        for T in R.TEMPERATURES:
            ref = R.cached_ref(spec, exact, True, T, "plain")
            slot = np.cumsum(case.values > 0) - 1
            p = case.planted
            assert ref.loss[slot[p.above]] < 1e-30 and ref.loss[slot[p.below]] >= R.FAR / T
            u = R.U_EQUAL
            ys = ref.scores.scores[case.x_item.size:].reshape(case.n_users, case.S)[u]
            assert abs(ref.loss[slot[p.equal]] - np.log1p(np.exp((ys - ys.max()) / T).sum())) < 1e-9


@pytest.mark.parametrize("spec", [(7, 20, 36), (100, 28, 128), (128, 128, 64), (64, 64, 256)], ids=lambda s: "S%d-L%d-d%d" % s)
def test_abi_histogram_ranks_and_coefficients(N, spec):
    """trec_softmax_fused_step with sample_hist / sample_rank: the histogram is bincount(samples), the ranks of every item a permutation
    of 0 .. count - 1 (users without interactions included); the per-pair coefficients within their bars, a hit's exactly 0"""
    case = R.cached_case(spec, False)
    ref = R.cached_ref(spec, False, True, 0.25, "both")
    inter = interactions_of(case)
    nu, ni, S, d = case.n_users, case.n_items, case.S, case.d
    loss, pred, d_u, d_ub, coef_s, coef_p = nan(inter.n_positive), nan(inter.nnz), nan(nu, d), nan(nu), nan(nu, S), nan(inter.nnz)
    hist = torch.zeros(ni, dtype=torch.int32, device="cuda")
    ranks = torch.full((nu, S), -1, dtype=torch.int32, device="cuda")
    U, V, ub, ib, samples, lq = dev(case.U), dev(case.V), dev(case.ub), dev(case.ib), dev(case.samples), dev(case.log_q)
    N.call("trec_softmax_fused_step", N.ptr(U), N.ptr(V), N.ptr(ub), N.ptr(ib), N.ptr(inter.indptr), N.ptr(inter.x_item32),
           N.ptr(inter.pos_slot), N.ptr(samples), nu, ni, S, d, int(inter.max_row_nnz), 4.0, N.ptr(lq), -float(np.log(ni)), 1, 1,
           N.ptr(loss), N.ptr(pred), N.ptr(d_u), N.ptr(d_ub), N.ptr(coef_s), N.ptr(coef_p), N.ptr(hist), N.ptr(ranks))
    torch.cuda.synchronize()
    assert np.array_equal(hist.cpu().numpy(), np.bincount(case.samples.reshape(-1), minlength=ni))
    rk, flat = ranks.cpu().numpy().reshape(-1), case.samples.reshape(-1)
    order = np.lexsort((rk, flat))
    want = np.concatenate([np.arange(c) for c in np.bincount(flat, minlength=ni)])
    assert np.array_equal(rk[order], want), "the ranks of an item are no permutation of 0 .. count - 1"
    nnz = case.x_item.size
    what = "%s abi" % (spec,)
    for name, got, want_, bar in (("loss", loss, ref.loss, ref.b_loss), ("pred_serial", pred, ref.pred_serial, ref.b_pred_serial),
                                  ("dU", d_u, ref.dU, ref.b_dU), ("d_ub", d_ub, ref.d_ub, ref.b_d_ub),
                                  ("coef_samples", coef_s, ref.g[nnz:], ref.b_g[nnz:]), ("coef_pairs", coef_p, ref.g[:nnz], ref.b_g[:nnz])):
        held("fused adjusted", name, got.cpu().numpy(), want_, bar, what)
    cs = coef_s.cpu().numpy()
    assert ref.hits.any() and not cs[ref.hits].any() and not cs[[R.U_NONE, R.U_NONPOS, R.U_ALLHITS]].any()
    assert not coef_p.cpu().numpy()[case.values <= 0].any()


def abi_args(N, case, inter, **over):
    """the argument list of trec_softmax_fused_step for `case` with biases and both options, entries replaced by name"""
    nu, ni, S, d = case.n_users, case.n_items, case.S, case.d
    keep = dict(U=dev(case.U), V=dev(case.V), ub=dev(case.ub), ib=dev(case.ib), samples=dev(case.samples), lq=dev(case.log_q),
                loss=nan(inter.n_positive), pred=nan(inter.nnz), d_u=nan(nu, d), d_ub=nan(nu), coef_s=nan(nu, S), coef_p=nan(inter.nnz),
                hist=torch.zeros(ni, dtype=torch.int32, device="cuda"), ranks=torch.zeros((nu, S), dtype=torch.int32, device="cuda"),
                indptr=inter.indptr, x_item=inter.x_item32, pos_slot=inter.pos_slot)
    v = dict(n_users=nu, n_items=ni, S=S, d=d, max_pos=int(inter.max_row_nnz), t=1.0, log_uniform=-float(np.log(ni)), use_q=1, no_hits=1)
    for k, val in over.items():
        if k in keep:
            keep[k] = val
        else:
            v[k] = val
    p = lambda k: N.ptr(keep[k])
    args = [p("U"), p("V"), p("ub"), p("ib"), p("indptr"), p("x_item"), p("pos_slot"), p("samples"), v["n_users"], v["n_items"], v["S"],
            v["d"], v["max_pos"], v["t"], p("lq"), v["log_uniform"], v["use_q"], v["no_hits"], p("loss"), p("pred"), p("d_u"), p("d_ub"),
            p("coef_s"), p("coef_p"), p("hist"), p("ranks")]
    return args, keep


def test_uncovered_shapes_and_argument_checks(ops, N):
    """the four uncovered shapes of the issue answer -1 / False; the entry point on the first returns TREC_ERR_UNSUPPORTED and on every
    bad argument TREC_ERR_INVALID, in both cases before any launch (the outputs keep their NaN fill)"""
    lib = N.load()
    for S, L, d in R.UNCOVERED:
        assert N.query("trec_softmax_fused_lds_bytes", S, L, d) == -1
        assert not ops.softmax_fused_supported(S, SimpleNamespace(max_row_nnz=L), d)
    assert ops.softmax_fused_supported(3, SimpleNamespace(max_row_nnz=125), 132)
    with tunings(N, softmax_fused=0):
        assert not ops.softmax_fused_supported(3, SimpleNamespace(max_row_nnz=125), 132)
    case = R.cached_case((7, 20, 36), False)
    inter = interactions_of(case)

    def rc(**over):
        args, keep = abi_args(N, case, inter, **over)
        code = lib.trec_softmax_fused_step(*args, N.stream())
        torch.cuda.synchronize()
        outputs = [keep[k] for k in ("loss", "pred", "d_u", "d_ub", "coef_s", "coef_p") if keep[k] is not None]
        assert code == 0 or all(bool(torch.isnan(o).all()) for o in outputs), over
        return code

    assert rc() == 0
    S, L, d = R.UNCOVERED[0]
    assert rc(S=S, max_pos=L, d=d) == TREC_ERR_UNSUPPORTED and b"not covered" in lib.trec_last_error()
    for over in (dict(U=None), dict(samples=None), dict(loss=None), dict(coef_p=None), dict(indptr=None),
                 dict(t=0.0), dict(t=-1.0), dict(t=float("inf")), dict(t=float("nan")),
                 dict(ub=None), dict(d_ub=None), dict(hist=None),
                 dict(n_items=0), dict(n_items=1 << 31), dict(x_item=None), dict(pos_slot=None)):
        assert rc(**over) == TREC_ERR_INVALID, over
    assert rc(n_users=0, U=None) == TREC_ERR_INVALID and rc(n_users=0) == 0


# ------------------------------------------------------------------------------------------------ model level
N_USERS, N_ITEMS, S_MODEL = 37, 53, 7
MODEL_CONFIGS = {"dot-biased": ("dot", True, 8), "dot-unbiased": ("dot", False, 8), "cosine": ("cosine", True, 8)}


def model_data():
    rng = np.random.default_rng(17)
    dense = (rng.random((N_USERS, N_ITEMS)) < 0.15).astype(np.float32)
    dense *= np.where(rng.random(dense.shape) < 0.85, 1.0, -1.0).astype(np.float32)
    dense[4, :] = 0                                   # a user without interactions
    dense[9, :] = -np.abs(dense[9, :])                # a user with negative interactions only
    dense[9, 3] = -1.0
    inter = sp.csr_matrix(dense)
    uf = sp.identity(N_USERS, dtype=np.float32, format="csr")
    itf = sp.identity(N_ITEMS, dtype=np.float32, format="csr")
    table = np.stack([rng.choice(N_ITEMS, size=S_MODEL, replace=False) for _ in range(N_USERS)]).astype(np.int32)
    return inter, uf, itf, table


def make_model(T, kind, biased, d, options, sampler, temperature=0.5, **kw):
    from tensorrec_amd.loss_graphs import SampledSoftmaxLossGraph
    from tensorrec_amd.prediction_graphs import (DotProductPredictionGraph, CosineSimilarityPredictionGraph,
                                                 EuclideanSimilarityPredictionGraph)
    graph = SampledSoftmaxLossGraph(temperature, log_q_correction=options, remove_accidental_hits=options)
    pred = {"dot": DotProductPredictionGraph, "cosine": CosineSimilarityPredictionGraph, "euclid": EuclideanSimilarityPredictionGraph}[kind]()
    return T.TensorRec(n_components=d, prediction_graph=pred, loss_graph=graph, biased=biased, seed=3, sampler=sampler, **kw)


def normalised(N, w):
    """the float32 rows and inverse norms trec_row_l2norm_fwd gives for a table: what a cosine model hands to the step"""
    x = dev(w)
    y, inv = torch.empty_like(x), torch.empty((x.shape[0],), dtype=torch.float32, device="cuda")
    N.call("trec_row_l2norm_fwd", N.ptr(x), x.shape[0], x.shape[1], N.ptr(y), N.ptr(inv))
    torch.cuda.synchronize()
    return y.cpu().numpy(), inv.cpu().numpy()


def through_norm(y, inv, dy, b_dy):
    """trec_row_l2norm_bwd in float64 on the SAVED float32 (y, inv): dx = inv (dy - y (y . dy)), and its bar: the bar of dy through the
    same linear map entry by entry, plus the kernel's own roundings -- the dot product (d terms, a chain or a tree: d + 6 at most),
    the product with y, the difference, the product with inv: (d + 10) u on the sum of the absolute terms"""
    y, inv, dy = f64(y), f64(inv)[:, None], f64(dy)
    d = y.shape[1]
    dx = inv * (dy - y * (y * dy).sum(1, keepdims=True))
    mag = inv * (np.abs(dy) + np.abs(y) * (np.abs(y) * np.abs(dy)).sum(1, keepdims=True))
    bar = inv * (b_dy + np.abs(y) * (np.abs(y) * b_dy).sum(1, keepdims=True)) + (d + 10.0) * U32 * mag
    return dx, bar


def float64_model_step(N, w, inter, table, log_q, kind, biased, d, options, temperature):
    """(output, float64 value, bar) of one step from the weights: softmax_step_reference.ref_step on the tables the step is handed --
    the weights themselves (identity features) or, for cosine, their float32 normalised rows, whose backward is through_norm"""
    U, V = w["linear_weights_user_0"], w["linear_weights_item"]
    norms = None
    if kind == "cosine":
        (U, inv_u), (V, inv_v) = normalised(N, U), normalised(N, V)
        norms = (inv_u, inv_v)
    m = sp.csr_matrix(inter)
    case = SimpleNamespace(U=U, V=V, ub=w["user_feature_biases"].reshape(-1) if biased else None,
                           ib=w["item_feature_biases"].reshape(-1) if biased else None, indptr=m.indptr.astype(np.int64),
                           x_item=m.indices.astype(np.int32), values=m.data.astype(np.float32), samples=table, log_q=log_q, S=S_MODEL, d=d,
                           n_users=N_USERS, n_items=N_ITEMS, exact=False)
    variant = "plain" if not options else ("both" if log_q is not None else "both-uniform")
    ref = R.ref_step(case, biased, temperature, variant)
    dU, bU, dV, bV = ref.dU, ref.b_dU, ref.dV, ref.b_dV
    if norms is not None:
        dU, bU = through_norm(U, norms[0], dU, bU)
        dV, bV = through_norm(V, norms[1], dV, bV)
    wants = [("pred_serial", ref.pred_serial, ref.b_pred_serial), ("loss", ref.loss, ref.b_loss),
             ("d linear_weights_user_0", dU, bU), ("d linear_weights_item", dV, bV)]
    if biased:
        wants += [("d user_feature_biases", ref.d_ub, ref.b_d_ub), ("d item_feature_biases", ref.d_ib, ref.b_d_ib)]
    return wants, ref


def one_step(T, N, kind, biased, d, options, fused=True):
    """one captured fit_partial step of the 37 x 53 model; options: both on, under a PopularitySampler whose first table and log q
    are read from a second sampler built the same way"""
    inter, uf, itf, table = model_data()
    log_q = None
    if options:
        pop = lambda: T.PopularitySampler(inter, power=0.75, smoothing=1.0, seed=5)
        sampler, twin = pop(), pop()
        table = twin.sample(N_ITEMS, N_USERS, S_MODEL, True, 1, "cuda", 0).cpu().numpy().astype(np.int32)
        log_q = twin.log_q("cuda").cpu().numpy()
    else:
        sampler = T.ReplaySampler([table])
    model = make_model(T, kind, biased, d, options, sampler)
    model.build(N_USERS, N_ITEMS)
    w = model.get_weights()
    if biased:
        r2 = np.random.default_rng(7)
        w["user_feature_biases"] = (0.1 * r2.standard_normal(w["user_feature_biases"].shape)).astype(np.float32)
        w["item_feature_biases"] = (0.1 * r2.standard_normal(w["item_feature_biases"].shape)).astype(np.float32)
        model.set_weights(w)
    w = {k: v.copy() for k, v in model.get_weights().items()}
    model._capture = {}
    try:
        if not fused:
            N.set_tuning("softmax_fused", 0)
        model.fit_partial(inter, uf, itf, epochs=1, learning_rate=0.05, alpha=1e-4, n_sampled_items=S_MODEL)
    finally:
        N.clear_tuning("softmax_fused")
    return model, w, inter, table, log_q


@pytest.mark.parametrize("options", [False, True], ids=["plain", "popularity-both"])
@pytest.mark.parametrize("config", sorted(MODEL_CONFIGS))
def test_one_fit_step_against_float64(ops, N, config, options):
    """the fused route inside a fit, and the generic route (tuning softmax_fused = 0) beside it: each within the bars of the float64
    composition, hence the two within the sum of their bars of each other"""
    import tensorrec_amd as T
    kind, biased, d = MODEL_CONFIGS[config]
    caps = {}
    for fused in (True, False):
        model, w, inter, table, log_q = one_step(T, N, kind, biased, d, options, fused=fused)
        assert model.last_step_form == "eager" and model.last_step_kernel == ("softmax_fused" if fused else None)
        caps[fused] = model._capture
        wants, ref = float64_model_step(N, w, inter, table, log_q, kind, biased, d, options, 0.5)
        if options:
            assert 0 < ref.hits.sum() < ref.hits.size
        key = "model %s %s" % (config, "fused" if fused else "generic")
        for name, want, bar in wants:
            got = caps[fused][name] if name in caps[fused] else caps[fused]["grads"][name[2:]]
            held(key, name, np.asarray(got).reshape(-1), want, bar, "options %d" % options)
    for name, want, bar in wants:
        a, b = (np.asarray(c[name] if name in c else c["grads"][name[2:]]).reshape(-1) for c in (caps[True], caps[False]))
        check(a, b, 2.0 * f64(bar).reshape(-1), "fused against generic: %s" % name)


def test_which_kernel_a_fit_reports(ops):
    import tensorrec_amd as T
    inter, uf, itf, table = model_data()
    m = make_model(T, "euclid", False, 8, False, T.ReplaySampler([table]))
    m.fit_partial(inter, uf, itf, epochs=1, n_sampled_items=S_MODEL)
    assert m.last_step_kernel is None
    m = T.TensorRec(n_components=8, loss_graph=T.loss_graphs.WMRBLossGraph(), seed=3, sampler=T.ReplaySampler([table]))
    assert m.last_step_kernel is None
    m.fit_partial(inter, uf, itf, epochs=1, n_sampled_items=S_MODEL)
    assert m.last_step_kernel == "wmrb_fused"

    class Mine(T.loss_graphs.SampledSoftmaxLossGraph):             # a subclass may override anything: the generic step
        pass
    m = T.TensorRec(n_components=8, loss_graph=Mine(0.5), seed=3, sampler=T.ReplaySampler([table]))
    m.fit_partial(inter, uf, itf, epochs=1, n_sampled_items=S_MODEL)
    assert m.last_step_kernel is None


def dummy(n_users=60, n_items=90, seed=3):
    import tensorrec_amd as T
    inter, uf, itf = T.util.generate_dummy_data(num_users=n_users, num_items=n_items, interaction_density=.08, num_user_features=40,
                                                num_item_features=50, n_features_per_user=6, n_features_per_item=7, random_state=seed)
    return sp.csr_matrix(inter), sp.csr_matrix(uf), sp.csr_matrix(itf)


def test_thirty_steps_with_the_popularity_sampler_lower_the_loss(ops):
    import tensorrec_amd as T
    inter, uf, itf = dummy()
    model = make_model(T, "dot", True, 16, True, T.PopularitySampler(inter, power=0.75, smoothing=1.0, seed=5))
    means = []
    for _ in range(30):
        model._capture = {}
        model.fit_partial(inter, uf, itf, epochs=1, learning_rate=0.05, n_sampled_items=12)
        assert model.last_step_kernel == "softmax_fused"
        means.append(float(np.asarray(model._capture["loss"]).mean()))
    model._capture = None
    assert np.isfinite(means).all() and means[-1] < means[0], means


def test_hip_graph_replay_equals_eager_steps(ops):
    """tests/test_gpu_sampled_losses.py::test_hip_graph_replay_equals_eager_steps on the fused route: same tolerance, user biases left
    out for the reason given there (their gradient is 0 in exact arithmetic and Adam steps on its rounding noise)"""
    import tensorrec_amd as T
    inter, uf, itf = dummy()
    out = []
    for graphs in (True, False):
        model = make_model(T, "dot", True, 16, False, None, hip_graphs=graphs)
        model.fit(inter, uf, itf, epochs=6, learning_rate=0.05, n_sampled_items=12)
        assert model.last_step_form == ("graph" if graphs else "eager") and model.last_step_kernel == "softmax_fused"
        out.append((model.get_weights(), model._opt_step, model._sample_step))
    (wa, oa, sa), (wb, ob, sb) = out
    assert (oa, sa) == (ob, sb)
    for k in wa:
        if k != "user_feature_biases":
            assert np.allclose(wa[k], wb[k], rtol=1e-3, atol=2e-3), k
