"""The adjusted sampled softmax and BPR kernels (csrc/loss_sampled.hip: accidental hits removed, logQ correction) against the float64
references of tests/sampled_adjust_reference.py, per element, within the bars derived there
(tests/test_sampled_adjust_reference_host.py shows on the CPU that float32 restatements lie inside them and seeded defects outside), and
the options inside a TensorRec fit.

* kernels   S on both sides of the wave-per-user limit with tuning wmrb_wave at its default and at 0 (both forms below 257 samples, the
            workgroup form above), users with 0 / 1 / 65 / 1,025 positives, temperatures 1 and 0.25, each option alone and both, log_q
            from a table spanning -2 ... -14 and None, the planted rows of sampled_adjust_reference.adjust_case; exact zeros where the
            contract asks for them; repeated runs bit for bit; options off through the new keywords bit for bit the plain ops;
* model     one captured step against a float64 composition, a 30-step fit with the PopularitySampler and both options, HIP-graph
            fits against eager fits with the sampler inside and outside the graph, WMRB under a PopularitySampler.

The largest error / bar per loss, form and output is kept in RATIOS; with TREC_SAMPLED_ADJUST_RATIOS_OUT=<file> it is written there at
the end (profiles/sampled_adjust_reference_ratios.json)."""
import functools
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import pair_reference as PR
import sampled_adjust_reference as R
from pair_reference import MODE_DOT, MODE_EUCLID, f64
from test_gpu_pair_kernels import check, dev, tunings
from test_gpu_sampled_losses import CONFIGS as MODEL_CONFIGS, N_USERS, N_ITEMS, S_MODEL, model_data, scatter_bar, dummy

pytestmark = pytest.mark.gpu

RATIOS = {}


@pytest.fixture(scope="module")
def ops():
    from tensorrec_amd import ops as _ops, _native
    _native.require_gpu()
    _native.load()
    yield _ops
    out = os.environ.get("TREC_SAMPLED_ADJUST_RATIOS_OUT")
    if out:
        write_ratios(out)


@pytest.fixture(scope="module")
def N(ops):
    from tensorrec_amd import _native
    return _native


def write_ratios(path):
    """profiles/sampled_adjust_reference_ratios.json: the ratios of this run, merged (as maxima) into the record the file already holds"""
    rec = {"what": "largest |result - float64 reference| / bar per loss, kernel form (or model configuration) and output over the cases of "
                   "tests/test_gpu_sampled_adjust.py (bars: tests/sampled_adjust_reference.py); a bar of 0 asks for equality and records 0",
           "command": "TREC_SAMPLED_ADJUST_RATIOS_OUT=<this file> python -m pytest -m gpu tests/test_gpu_sampled_adjust.py", "ratios": {}}
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
LOSSES = ["%s-%g" % (c, t) for c in R.CONFIGS for t in R.TEMPERATURES] + ["bpr"]


@functools.lru_cache(maxsize=2)
def cached_case(S):
    return R.adjust_case(S)


@functools.lru_cache(maxsize=None)
def cached_ref(S, loss):
    """computed once per (S, loss) and left unchanged"""
    case = cached_case(S)
    if loss == "bpr":
        return R.ref_bpr_adj(case)
    config, temperature = loss.rsplit("-", 1)
    use_q, no_hits, log_q = R.CONFIGS[config]
    return R.ref_sampled_softmax_adj(case, float(temperature), use_q, no_hits, log_q)


def run_loss(ops, loss, case, inter):
    pt, st = dev(case.pred).requires_grad_(), dev(case.samp).requires_grad_()
    items = dev(case.items)
    if loss == "bpr":
        out = ops.bpr_loss(pt, st, inter, sample_items=items, remove_accidental_hits=True)
    else:
        config, temperature = loss.rsplit("-", 1)
        use_q, no_hits, log_q = R.CONFIGS[config]
        out = ops.sampled_softmax_loss(pt, st, inter, temperature=float(temperature), sample_items=items,
                                       sample_log_q=dev(case.log_q) if log_q == "case" else None, log_q_correction=use_q,
                                       remove_accidental_hits=no_hits)
    out.backward(dev(case.go))
    torch.cuda.synchronize()
    return out.detach().cpu().numpy(), pt.grad.cpu().numpy(), st.grad.cpu().numpy()


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("S", R.SAMPLE_COUNTS)
def test_sample_counts(ops, N, S, loss):
    """S = 1 .. 256: the wave-per-user kernels and (wmrb_wave = 0) the workgroup kernels; 257, 300: the workgroup kernels.  Every
    run is made twice and must give the same bits."""
    from tensorrec_amd.sparse import Interactions
    case, ref = cached_case(S), cached_ref(S, loss)
    inter = Interactions(case.matrix, case.n_users, case.n_items, "cuda")
    assert np.array_equal(inter.indptr.cpu().numpy(), case.indptr) and np.array_equal(inter.values.cpu().numpy(), case.values)
    assert np.array_equal(inter.x_item32.cpu().numpy(), case.cols)
    pos = case.values > 0
    removes = loss == "bpr" or R.CONFIGS[loss.rsplit("-", 1)[0]][1]
    for wave in ((1, 0) if S <= 256 else (1,)):
        with tunings(N, wmrb_wave=wave):
            got = run_loss(ops, loss, case, inter)
            again = run_loss(ops, loss, case, inter)
        form = "wave" if (wave and S <= 256) else "workgroup"
        for name, g, want, bar in zip(("loss", "d_pred", "d_samp"), got, (ref.loss, ref.d_pred, ref.d_samp), R.bars(ref)):
            held("%s %s" % ("bpr" if loss == "bpr" else "softmax", form), name, g, want, bar, "S %d %s" % (S, loss))
        lo, d_pred, d_samp = got
        assert (d_pred[~pos] == 0).all(), "d_pred of a non-positive interaction is not exactly 0"
        assert (d_samp[:2] == 0).all(), "the d_samp row of a user without positives is not exactly 0"
        if removes:
            assert (d_samp[ref.hits] == 0).all(), "d_samp of a hit is not exactly 0"
            u = R.U_ALL_HITS
            mine = np.arange(case.indptr[u], case.indptr[u + 1])
            slots = (np.cumsum(pos) - 1)[mine[pos[mine]]]
            assert (lo[slots] == 0).all() and (d_pred[mine] == 0).all() and (d_samp[u] == 0).all(), "every sample a hit: not all 0"
        for name, a, b in zip(("loss", "d_pred", "d_samp"), got, again):
            assert np.array_equal(a, b), "S %d %s %s: two runs differ in %s" % (S, loss, form, name)


@pytest.mark.parametrize("S", [65, 300])
def test_options_off_is_the_plain_op_bit_for_bit(ops, S):
    """the new keywords at their defaults (ids and log_q handed over all the same) take the plain Functions: equal bits"""
    from tensorrec_amd.sparse import Interactions
    case = cached_case(S)
    inter = Interactions(case.matrix, case.n_users, case.n_items, "cuda")
    items, log_q, go = dev(case.items), dev(case.log_q), dev(case.go)
    for which in ("softmax", "bpr"):
        outs = []
        for new in (False, True):
            pt, st = dev(case.pred).requires_grad_(), dev(case.samp).requires_grad_()
            kw = dict(sample_items=items, sample_log_q=log_q, log_q_correction=False, remove_accidental_hits=False) if new else {}
            out = ops.sampled_softmax_loss(pt, st, inter, temperature=0.25, **kw) if which == "softmax" else ops.bpr_loss(pt, st, inter, **kw)
            out.backward(go)
            outs.append((out.detach().cpu().numpy(), pt.grad.cpu().numpy(), st.grad.cpu().numpy()))
        for a, b in zip(*outs):
            assert np.array_equal(a, b), which
    with pytest.raises(ValueError):
        ops.sampled_softmax_loss(dev(case.pred), dev(case.samp), inter, remove_accidental_hits=True)       # no ids
    with pytest.raises(ValueError):
        ops.bpr_loss(dev(case.pred), dev(case.samp), inter, sample_items=items, log_q_correction=True)     # BPR has no logQ term


# ------------------------------------------------------------------------------------------------ model level
def replay_sampler(T, tables, log_q=None):
    """a ReplaySampler that also reports log q (None: the class has no such method, which means uniform)"""
    if log_q is None:
        return T.ReplaySampler(tables)

    class ReplayWithLogQ(T.ReplaySampler):
        def log_q(self, device):
            return torch.from_numpy(log_q).to(device)
    return ReplayWithLogQ(tables)


def make_model(T, loss, mode, biased, d, sampler=None, **kw):
    from tensorrec_amd.loss_graphs import SampledSoftmaxLossGraph, BPRLossGraph
    from tensorrec_amd.prediction_graphs import DotProductPredictionGraph, EuclideanSimilarityPredictionGraph
    graph = BPRLossGraph(remove_accidental_hits=True) if loss == "bpr" else \
        SampledSoftmaxLossGraph(float(loss.split("-")[1]), log_q_correction=True, remove_accidental_hits=True)
    pred = DotProductPredictionGraph() if mode == MODE_DOT else EuclideanSimilarityPredictionGraph()
    if sampler is not None:
        kw["sampler"] = sampler
    return T.TensorRec(n_components=d, prediction_graph=pred, loss_graph=graph, biased=biased, seed=3, **kw)


def model_log_q():
    return np.random.default_rng(23).permutation(np.linspace(-2.0, -6.0, N_ITEMS)).astype(np.float32)


def float64_step(w, inter, table, log_q, mode, biased, d, loss):
    """(output, float64 value, bar) of one step from the weights ``w``: tests/test_gpu_sampled_losses.py::float64_step with the adjusted
    references.  The hit mask and c are functions of the ids alone, so the argument for the bars there carries over unchanged: every
    logit moves by at most t delta_u, every kept exponential ratio by a factor within exp(+-2 t delta_u)."""
    from types import SimpleNamespace
    wants = []
    U, V = w["linear_weights_user_0"], w["linear_weights_item"]
    ub = w["user_feature_biases"].reshape(-1) if biased else None
    ib = w["item_feature_biases"].reshape(-1) if biased else None
    coo = inter.tocoo()
    xu, xi = coo.row.astype(np.int64), coo.col.astype(np.int64)
    xus, xis = np.repeat(np.arange(N_USERS), S_MODEL), table.reshape(-1).astype(np.int64)
    sc, scs = PR.ref_pair_scores(U, V, xu, xi, mode, ub, ib), PR.ref_pair_scores(U, V, xus, xis, mode, ub, ib)
    indptr, values = inter.indptr.astype(np.int64), inter.data
    case = SimpleNamespace(indptr=indptr, values=values, cols=inter.indices, pred=sc.scores, samp=scs.scores.reshape(N_USERS, S_MODEL),
                           go=np.ones(int((values > 0).sum())), items=table, log_q=log_q, n_items=N_ITEMS)
    ref = R.ref_bpr_adj(case) if loss == "bpr" else R.ref_sampled_softmax_adj(case, float(loss.split("-")[1]), True, True)
    delta_p, delta_s = PR.score_bar(sc, d), PR.score_bar(scs, d).reshape(N_USERS, S_MODEL)
    delta_u = delta_s.max(1)
    np.maximum.at(delta_u, xu, delta_p)
    pos = values > 0
    n_u = np.bincount(xu[pos], minlength=N_USERS)
    if loss == "bpr":
        bar_loss = ref.bar_loss + 2.0 * delta_u[xu[pos]]
        bar_gp = ref.bar_d_pred + np.where(pos, delta_u[xu] / 2.0, 0.0)
        bar_gs = (ref.bar_d_samp + ((n_u / S_MODEL) * delta_u / 2.0)[:, None] * (n_u > 0)[:, None]) * ~ref.hits
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
    wants.append(("d linear_weights_user_0", pg.dU, bU + scatter_bar(ax, N_USERS, bar_g[:, None] * su)))
    wants.append(("d linear_weights_item", pg.dV, bV + scatter_bar(ai, N_ITEMS, bar_g[:, None] * sv)))
    if biased:
        wants.append(("d user_feature_biases", pg.dub, bub + scatter_bar(ax, N_USERS, bar_g)))
        wants.append(("d item_feature_biases", pg.dib, bib + scatter_bar(ai, N_ITEMS, bar_g)))
    return wants, ref


@pytest.mark.parametrize("loss", ["softmax-0.5", "bpr"])
@pytest.mark.parametrize("config", ["dot-biased-8", "euclid-unbiased-5"])
def test_one_fit_step_against_float64(ops, config, loss):
    """One fit_partial step as in tests/test_gpu_sampled_losses.py (37 users x 53 items, identity features, S = 7 replayed samples, drawn
    WITH replacement here) with both options on and a sampler that reports a log_q table, against the float64 composition."""
    import tensorrec_amd as T
    mode, biased, d = MODEL_CONFIGS[config]
    inter, uf, itf, _ = model_data()
    table = np.random.default_rng(29).integers(0, N_ITEMS, size=(N_USERS, S_MODEL)).astype(np.int32)
    log_q = model_log_q()
    model = make_model(T, loss, mode, biased, d, replay_sampler(T, [table], log_q))
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
    wants, ref = float64_step(w, inter, table, log_q, mode, biased, d, loss)
    assert 0 < ref.hits.sum() < ref.hits.size
    for name, want, bar in wants:
        got = cap[name] if name in cap else cap["grads"][name[2:]]
        held(key, name, np.asarray(got).reshape(-1), want, bar, loss)


def test_a_graph_without_the_flag_gets_todays_kwargs(ops):
    """a user-defined sample-based graph WITHOUT **kwargs and without the flag is called with exactly the old keywords; with the flag it
    receives the ids and the sampler's log q"""
    import tensorrec_amd as T
    from tensorrec_amd.loss_graphs import AbstractLossGraph
    seen = {}

    class Strict(AbstractLossGraph):
        is_sample_based = True

        def connect_loss_graph(self, tf_prediction_serial, tf_interactions_serial, tf_interactions, tf_n_users, tf_n_items,
                               tf_sample_predictions, tf_n_sampled_items):
            return ops.bpr_loss(tf_prediction_serial, tf_sample_predictions, tf_interactions)

    class Wants(AbstractLossGraph):
        is_sample_based = True
        wants_sample_items = True

        def connect_loss_graph(self, tf_prediction_serial, tf_interactions, tf_sample_predictions, tf_sample_items, tf_sample_log_q,
                               **kwargs):
            seen["items"], seen["log_q"] = tf_sample_items, tf_sample_log_q
            return ops.bpr_loss(tf_prediction_serial, tf_sample_predictions, tf_interactions)

    inter, uf, itf = dummy()
    T.TensorRec(n_components=4, loss_graph=Strict()).fit_partial(inter, uf, itf, epochs=1, n_sampled_items=5)
    T.TensorRec(n_components=4, loss_graph=Wants()).fit_partial(inter, uf, itf, epochs=1, n_sampled_items=5)
    assert seen["items"].dtype == torch.int32 and tuple(seen["items"].shape) == (inter.shape[0], 5) and seen["log_q"] is None
    sampler = T.PopularitySampler(inter, power=0.75, smoothing=1.0)
    T.TensorRec(n_components=4, loss_graph=Wants(), sampler=sampler).fit_partial(inter, uf, itf, epochs=1, n_sampled_items=5)
    assert seen["log_q"] is sampler.log_q("cuda") and tuple(seen["log_q"].shape) == (inter.shape[1],)


@pytest.mark.parametrize("loss", ["softmax-0.5", "bpr"])
def test_thirty_steps_with_the_popularity_sampler_lower_the_loss(ops, loss):
    import tensorrec_amd as T
    inter, uf, itf = dummy()
    model = make_model(T, loss, MODE_DOT, True, 16, T.PopularitySampler(inter, power=0.75, smoothing=1.0, seed=5))
    means = []
    for _ in range(30):
        model._capture = {}
        model.fit_partial(inter, uf, itf, epochs=1, learning_rate=0.05, n_sampled_items=12)
        means.append(float(np.asarray(model._capture["loss"]).mean()))
    model._capture = None
    assert np.isfinite(means).all() and means[-1] < means[0], means


@pytest.mark.parametrize("sampler", ["device", "popularity"])
@pytest.mark.parametrize("loss", ["softmax-0.5", "bpr"])
def test_hip_graph_replay_equals_eager_steps(ops, loss, sampler):
    """tests/test_gpu_sampled_losses.py::test_hip_graph_replay_equals_eager_steps with the options on: the DeviceSampler is captured
    inside the graph, the PopularitySampler fills the static table before each replay and its log_q is a constant tensor"""
    import tensorrec_amd as T
    inter, uf, itf = dummy()
    out = []
    for graphs in (True, False):
        s = T.PopularitySampler(inter, power=0.75, smoothing=1.0, seed=5) if sampler == "popularity" else None
        model = make_model(T, loss, MODE_DOT, True, 16, s, hip_graphs=graphs)
        model.fit(inter, uf, itf, epochs=6, learning_rate=0.05, n_sampled_items=12)
        assert model.last_step_form == ("graph" if graphs else "eager")
        out.append((model.get_weights(), model._opt_step, model._sample_step))
    (wa, oa, sa), (wb, ob, sb) = out
    assert (oa, sa) == (ob, sb)
    for k in wa:
        if k != "user_feature_biases":
            assert np.allclose(wa[k], wb[k], rtol=1e-3, atol=2e-3), k


def test_wmrb_with_a_popularity_sampler_equals_the_replayed_tables(ops):
    """WMRB is untouched: under a PopularitySampler it takes the paths of any sampler that is not the DeviceSampler, and ends where a
    ReplaySampler fed the same tables ends"""
    import tensorrec_amd as T
    from tensorrec_amd.loss_graphs import WMRBLossGraph
    inter, uf, itf = dummy()
    S, steps = 12, 4
    pop = T.PopularitySampler(inter, power=0.75, smoothing=1.0, seed=5)
    tables = [pop.sample(inter.shape[1], inter.shape[0], S, False, step, "cuda").cpu().numpy() for step in range(1, steps + 1)]
    ends = []
    for sampler in (T.PopularitySampler(inter, power=0.75, smoothing=1.0, seed=5), T.ReplaySampler(tables),
                    T.PopularitySampler(inter, power=0.75, smoothing=1.0, seed=6)):
        model = T.TensorRec(n_components=16, loss_graph=WMRBLossGraph(), sampler=sampler, seed=3)
        model.fit(inter, uf, itf, epochs=steps, learning_rate=0.05, n_sampled_items=S)
        ends.append((model.get_weights(), model.last_step_form))
    (wa, fa), (wb, fb), (wc, _) = ends
    assert fa == fb
    # (the WMRB steps add floats with atomics: equal up to the summation order, the tolerance of the graph-replay tests; user biases
    # left out as there.  Another seed -- other tables -- ends elsewhere.)
    for k in wa:
        if k != "user_feature_biases":
            assert np.allclose(wa[k], wb[k], rtol=1e-3, atol=2e-3), k
    assert not np.allclose(wa["linear_weights_item"], wc["linear_weights_item"], rtol=1e-3, atol=2e-3)
