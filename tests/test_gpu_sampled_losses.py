"""The sampled softmax and BPR kernels (csrc/loss_sampled.hip) against the float64 references of tests/sampled_loss_reference.py, per
element, within the bars derived there (tests/test_sampled_loss_reference_host.py shows on the CPU that float32 restatements lie inside
them and seeded defects outside), and the two loss graphs inside a TensorRec fit.

* kernels   S on both sides of the wave-per-user limit with tuning wmrb_wave at its default and at 0 (both forms below 257 samples, the
            workgroup form above), users with 0 / 65 / 1,025 / 2,600 positives, temperatures 1 and 0.25, the planted edge cases of
            sampled_loss_reference.loss_case; exact zeros where the contract asks for them; a repeated run bit for bit;
* model     one captured step against a float64 composition (scores from the weights, the loss reference, the pair-gradient reference of
            tests/pair_reference.py), a 30-step fit whose loss goes down, a HIP-graph fit against the eager fit.

The largest error / bar per loss, form and output is kept in RATIOS; with TREC_SAMPLED_RATIOS_OUT=<file> it is written there at the end
(profiles/sampled_loss_reference_ratios.json)."""
import functools
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import pair_reference as PR
import sampled_loss_reference as R
from pair_reference import MODE_DOT, MODE_EUCLID, f64
from test_gpu_pair_kernels import check, dev, tunings

pytestmark = pytest.mark.gpu

RATIOS = {}


@pytest.fixture(scope="module")
def ops():
    from tensorrec_amd import ops as _ops, _native
    _native.require_gpu()
    _native.load()
    yield _ops
    out = os.environ.get("TREC_SAMPLED_RATIOS_OUT")
    if out:
        write_ratios(out)


@pytest.fixture(scope="module")
def N(ops):
    from tensorrec_amd import _native
    return _native


def write_ratios(path):
    """profiles/sampled_loss_reference_ratios.json: the ratios of this run, merged (as maxima) into the record the file already holds"""
    rec = {"what": "largest |result - float64 reference| / bar per loss, kernel form (or model configuration) and output over the cases of "
                   "tests/test_gpu_sampled_losses.py (bars: tests/sampled_loss_reference.py); a bar of 0 asks for equality and records 0",
           "command": "TREC_SAMPLED_RATIOS_OUT=<this file> python -m pytest -m gpu tests/test_gpu_sampled_losses.py", "ratios": {}}
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
        print("%s %s %s: largest error / bar %.4g" % (key, what, name, r))
    check(got, want, bar, "%s %s: %s" % (key, what, name))


# ------------------------------------------------------------------------------------------------ kernels
LOSSES = ["softmax-1", "softmax-0.25", "bpr"]


@functools.lru_cache(maxsize=2)
def case_and_refs(S):
    """the case and its three references, computed once per S and left unchanged"""
    case = R.loss_case(S)
    refs = {"bpr": R.ref_bpr(case.indptr, case.values, case.pred, case.samp, case.go)}
    for temperature in R.TEMPERATURES:
        refs["softmax-%g" % temperature] = R.ref_sampled_softmax(case.indptr, case.values, case.pred, case.samp, case.go, temperature)
    return case, refs


def run_loss(ops, loss, case, inter):
    pt, st = dev(case.pred).requires_grad_(), dev(case.samp).requires_grad_()
    if loss == "bpr":
        out = ops.bpr_loss(pt, st, inter)
    else:
        out = ops.sampled_softmax_loss(pt, st, inter, temperature=float(loss.split("-")[1]))
    out.backward(dev(case.go))
    torch.cuda.synchronize()
    return out.detach().cpu().numpy(), pt.grad.cpu().numpy(), st.grad.cpu().numpy()


def check_losses(ops, N, S, loss, repeat=False):
    from tensorrec_amd.sparse import Interactions
    case, refs = case_and_refs(S)
    ref = refs[loss]
    inter = Interactions(case.matrix, case.n_users, case.n_items, "cuda")
    assert np.array_equal(inter.indptr.cpu().numpy(), case.indptr) and np.array_equal(inter.values.cpu().numpy(), case.values)
    pos = case.values > 0
    assert (np.diff(case.indptr)[:2] == [0, 3]).all() and not pos[case.indptr[1]:case.indptr[2]].any()
    for wave in ((1, 0) if S <= 256 else (1,)):                   # (above 256 samples the knob has no effect: the workgroup kernels run)
        with tunings(N, wmrb_wave=wave):
            got = run_loss(ops, loss, case, inter)
            again = run_loss(ops, loss, case, inter) if repeat else None
        form = "wave" if (wave and S <= 256) else "workgroup"
        for name, g, want, bar in zip(("loss", "d_pred", "d_samp"), got, (ref.loss, ref.d_pred, ref.d_samp), R.bars(ref)):
            held("%s %s" % (loss.split("-")[0], form), name, g, want, bar, "S %d %s" % (S, loss))
        _, d_pred, d_samp = got
        assert (d_pred[~pos] == 0).all(), "d_pred of a non-positive interaction is not exactly 0"
        assert (d_samp[:2] == 0).all(), "the d_samp row of a user without positives is not exactly 0"
        if again is not None:
            for name, a, b in zip(("loss", "d_pred", "d_samp"), got, again):
                assert np.array_equal(a, b), "S %d %s %s: two runs differ in %s" % (S, loss, form, name)


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("S", R.SAMPLE_COUNTS)
def test_sample_counts(ops, N, S, loss):
    """S = 1 .. 256: the wave-per-user kernels and (wmrb_wave = 0) the workgroup kernels; 257, 300: the workgroup kernels.  Users with 0,
    65, 1,025 and 2,600 positives ride along at every S."""
    check_losses(ops, N, S, loss)


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("S", R.SAMPLE_COUNTS_MANY)
def test_many_positives_and_repeat(ops, N, S, loss):
    """0 / 65 / 1,025 / 2,600 positives per user at S = 40 (wave kernels: 64 positives per pass; workgroup kernels: 1,024 staged per
    pass) and S = 300 (workgroup kernels only); every run is made twice and must give the same bits"""
    check_losses(ops, N, S, loss, repeat=True)


# ------------------------------------------------------------------------------------------------ model level
N_USERS, N_ITEMS, S_MODEL = 37, 53, 7
CONFIGS = {"dot-biased-8": (MODE_DOT, True, 8), "dot-biased-5": (MODE_DOT, True, 5),
           "euclid-unbiased-8": (MODE_EUCLID, False, 8), "euclid-unbiased-5": (MODE_EUCLID, False, 5)}


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


def make_model(T, loss, mode, biased, d, table=None, **kw):
    from tensorrec_amd.loss_graphs import SampledSoftmaxLossGraph, BPRLossGraph
    from tensorrec_amd.prediction_graphs import DotProductPredictionGraph, EuclideanSimilarityPredictionGraph
    graph = BPRLossGraph() if loss == "bpr" else SampledSoftmaxLossGraph(float(loss.split("-")[1]))
    pred = DotProductPredictionGraph() if mode == MODE_DOT else EuclideanSimilarityPredictionGraph()
    if table is not None:
        kw["sampler"] = T.ReplaySampler([table])
    return T.TensorRec(n_components=d, prediction_graph=pred, loss_graph=graph, biased=biased, seed=3, **kw)


def scatter_bar(rows, n_rows, weight):
    out = np.zeros((n_rows,) + weight.shape[1:])
    np.add.at(out, rows, weight)
    return out


def float64_step(w, inter, table, mode, biased, d, loss):
    """(output, float64 value, bar) of one step from the weights ``w``: see test_one_fit_step_against_float64"""
    wants = []
    U, V = w["linear_weights_user_0"], w["linear_weights_item"]
    ub = w["user_feature_biases"].reshape(-1) if biased else None
    ib = w["item_feature_biases"].reshape(-1) if biased else None
    coo = inter.tocoo()                                           # row-major: the serial order of Interactions
    xu, xi = coo.row.astype(np.int64), coo.col.astype(np.int64)
    xus, xis = np.repeat(np.arange(N_USERS), S_MODEL), table.reshape(-1).astype(np.int64)
    sc, scs = PR.ref_pair_scores(U, V, xu, xi, mode, ub, ib), PR.ref_pair_scores(U, V, xus, xis, mode, ub, ib)
    indptr, values = inter.indptr.astype(np.int64), inter.data
    go = np.ones(int((values > 0).sum()))
    samp = scs.scores.reshape(N_USERS, S_MODEL)
    if loss == "bpr":
        ref = R.ref_bpr(indptr, values, sc.scores, samp, go)
    else:
        ref = R.ref_sampled_softmax(indptr, values, sc.scores, samp, go, float(loss.split("-")[1]))
    delta_p, delta_s = PR.score_bar(sc, d), PR.score_bar(scs, d).reshape(N_USERS, S_MODEL)
    delta_u = delta_s.max(1)
    np.maximum.at(delta_u, xu, delta_p)
    pos = values > 0
    n_u = np.bincount(xu[pos], minlength=N_USERS)
    if loss == "bpr":
        bar_loss = ref.bar_loss + 2.0 * delta_u[xu[pos]]
        bar_gp = ref.bar_d_pred + np.where(pos, delta_u[xu] / 2.0, 0.0)
        bar_gs = ref.bar_d_samp + ((n_u / S_MODEL) * delta_u / 2.0)[:, None] * (n_u > 0)[:, None]
    else:
        f = np.expm1(2.0 * delta_u / float(loss.split("-")[1]))
        bar_loss = ref.bar_loss + f[xu[pos]]
        bar_gp = ref.bar_d_pred + np.abs(ref.d_pred) * f[xu]
        bar_gs = ref.bar_d_samp + np.abs(ref.d_samp) * f[:, None]
    wants.append(("pred_serial", sc.scores, delta_p))
    wants.append(("loss", ref.loss, bar_loss))

    ax, ai = np.concatenate([xu, xus]), np.concatenate([xi, xis])
    g, bar_g = np.concatenate([ref.d_pred, ref.d_samp.reshape(-1)]), np.concatenate([bar_gp, bar_gs.reshape(-1)])
    pg = PR.ref_pair_grads(U, V, ax, ai, g, mode)
    bU, bV, bub, bib = PR.grad_bars(pg, d)
    x, y = f64(U)[ax], f64(V)[ai]
    if mode == MODE_DOT:
        su, sv = np.abs(y), np.abs(x)
    else:
        su = np.where((pg.D >= PR.EPS)[:, None], np.abs(x - y) / np.sqrt(np.maximum(pg.D, 1e-300))[:, None], 0.0)
        sv = su
    bU = bU + scatter_bar(ax, N_USERS, bar_g[:, None] * su)
    bV = bV + scatter_bar(ai, N_ITEMS, bar_g[:, None] * sv)
    wants.append(("d linear_weights_user_0", pg.dU, bU))
    wants.append(("d linear_weights_item", pg.dV, bV))
    if biased:
        bub = bub + scatter_bar(ax, N_USERS, bar_g)
        bib = bib + scatter_bar(ai, N_ITEMS, bar_g)
        wants.append(("d user_feature_biases", pg.dub, bub))
        wants.append(("d item_feature_biases", pg.dib, bib))
    return wants, pg


@pytest.mark.parametrize("loss", ["softmax-0.5", "bpr"])
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_one_fit_step_against_float64(ops, config, loss):
    """One fit_partial step (37 users x 53 items, identity features, so the representations ARE the weight tables; S = 7 replayed samples)
    with the loss vector, the serial predictions and every variable's raw gradient captured, against a float64 composition: scores from
    the weights (pair_reference.ref_pair_scores), the loss reference on those scores with go = 1, pair_reference.ref_pair_grads fed
    with the reference d_pred / d_samp.

    Bars.  The loss kernels are handed float32 scores that are off by at most delta = pair_reference.score_bar; with delta_u the largest
    delta among a user's interactions and samples:
      * sampled softmax: loss_p, b Z / D and every softmax weight E_s K are functions of the logits y t alone; moving every logit by at
        most eps = t delta_u multiplies each exponential ratio by a factor within exp(+-2 eps), so loss_p moves by at most 2 eps and
        d y_p, d y_us by a relative f = expm1(2 t delta_u) (go = 1: all terms of d y_us have one sign);
      * BPR: x = y_s - y_p moves by at most 2 delta_u; softplus has slope sigma <= 1 and sigma has slope <= 1/4: loss_p moves by
        2 delta_u, d y_p = -(1/S) sum_s sigma by delta_u / 2, d y_us = (1/S) sum_p sigma by (n_u / S) delta_u / 2.
    These are added to the kernels' own bars (sampled_loss_reference) to give bar_g per pair.  A variable's gradient is a sum over pairs of
    g_p times d score_p / d entry: pair_reference.grad_bars for the sums themselves, plus bar_g propagated through |g| |row|:
    sum_p bar_g_p |d score_p / d entry| (dot: |v_c| resp. |u_c|; Euclidean: |u_c - v_c| / sqrt(D_p), 0 for a clamped pair; biases: 1)."""
    import tensorrec_amd as T
    mode, biased, d = CONFIGS[config]
    inter, uf, itf, table = model_data()
    model = make_model(T, loss, mode, biased, d, table)
    model.build(N_USERS, N_ITEMS)
    w = model.get_weights()
    if biased:
        r2 = np.random.default_rng(7)
        w["user_feature_biases"] = (0.1 * r2.standard_normal(w["user_feature_biases"].shape)).astype(np.float32)
        w["item_feature_biases"] = (0.1 * r2.standard_normal(w["item_feature_biases"].shape)).astype(np.float32)
        model.set_weights(w)
    w = {k: v.copy() for k, v in model.get_weights().items()}
    model._capture = {}
    model.fit_partial(inter, uf, itf, epochs=1, learning_rate=0.05, alpha=1e-4, n_sampled_items=S_MODEL)
    cap = model._capture
    assert model.last_step_form == "eager"

    key = "model %s %s" % (loss.split("-")[0], config)
    wants, pg = float64_step(w, inter, table, mode, biased, d, loss)
    for name, want, bar in wants:
        got = cap[name] if name in cap else cap["grads"][name[2:]]
        held(key, name, np.asarray(got).reshape(-1), want, bar, loss)
    assert np.abs(pg.dU).max() > 1e-3 and not pg.dU[4].any() and not cap["grads"]["linear_weights_user_0"][[4, 9]].any()


def dummy(n_users=60, n_items=90, seed=3):
    import tensorrec_amd as T
    inter, uf, itf = T.util.generate_dummy_data(num_users=n_users, num_items=n_items, interaction_density=.08, num_user_features=40,
                                                num_item_features=50, n_features_per_user=6, n_features_per_item=7, random_state=seed)
    return sp.csr_matrix(inter), sp.csr_matrix(uf), sp.csr_matrix(itf)


@pytest.mark.parametrize("loss", ["softmax-0.5", "bpr"])
def test_thirty_steps_lower_the_loss(ops, loss):
    import tensorrec_amd as T
    inter, uf, itf = dummy()
    model = make_model(T, loss, MODE_DOT, True, 16)
    means = []
    for _ in range(30):
        model._capture = {}
        model.fit_partial(inter, uf, itf, epochs=1, learning_rate=0.05, n_sampled_items=12)
        means.append(float(np.asarray(model._capture["loss"]).mean()))
    model._capture = None
    assert np.isfinite(means).all() and means[-1] < means[0], means


@pytest.mark.parametrize("loss", ["softmax-0.5", "bpr"])
def test_hip_graph_replay_equals_eager_steps(ops, loss):
    """tests/test_gpu_model.py::test_hip_graph_replay_equals_eager_steps for the two new losses: a fit whose later steps are HIP-graph
    replays reports last_step_form "graph" and ends with the weights of the all-eager fit, up to the summation order of the counting-sort
    buckets (user_feature_biases left out: their gradient is 0 in exact arithmetic -- b_u cancels in every y_s - y_p -- and Adam steps on
    its rounding noise)."""
    import tensorrec_amd as T
    inter, uf, itf = dummy()
    out = []
    for graphs in (True, False):
        model = make_model(T, loss, MODE_DOT, True, 16, hip_graphs=graphs)
        model.fit(inter, uf, itf, epochs=6, learning_rate=0.05, n_sampled_items=12)
        assert model.last_step_form == ("graph" if graphs else "eager")
        out.append((model.get_weights(), model._opt_step, model._sample_step))
    (wa, oa, sa), (wb, ob, sb) = out
    assert (oa, sa) == (ob, sb)
    for k in wa:
        if k != "user_feature_biases":
            assert np.allclose(wa[k], wb[k], rtol=1e-3, atol=2e-3), k
