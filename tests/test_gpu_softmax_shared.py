"""The sampled-softmax step with shared negatives (csrc/softmax_shared.hip, ops.softmax_shared_step) against the float64 step of
tests/softmax_shared_reference.py -- softmax_step_reference.ref_step on the table that repeats the shared row -- per element and per
output, within the bars derived there (tests/test_softmax_shared_reference_host.py shows on the CPU that a float32 restatement lies
inside them and seeded defects outside), and the route inside a TensorRec fit.

* kernel   users 1 ... 300 (wave and workgroup edges), S 1 ... 1000 (tile edges, many tiles), d 4 / 36 / 64 / 128; with and without
           biases, temperatures 1 and 0.25, plain / logQ with a table / logQ uniform (cycling over the cases, all crossed on the core
           case); forced slice counts 1, 2, 3 on 300 users; the planted rows of softmax_shared_reference.shared_case; all samples equal;
           samples spanning +-30; exact zeros; the dyadic family bit for bit on pred_serial; two calls bit-identical;
* model    one captured step (dot with / without biases, cosine) at 129 x 200, S = 65, d = 36 on the new route and on the expanded
           generic step (tuning softmax_shared = 0), each against the float64 step; the kernel and the form a fit reports on covered
           and uncovered configurations; the samplers draw one [1, S] row per step; a 30-step fit; shared_negatives=False untouched.

The largest error / bar per output is kept in RATIOS; with TREC_SOFTMAX_SHARED_RATIOS_OUT=<file> it is written there at the end
(profiles/softmax_shared_reference_ratios.json)."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import softmax_shared_reference as R
from pair_reference import f64
from test_gpu_pair_kernels import check, dev, tunings
from test_gpu_softmax_fused import normalised, through_norm

pytestmark = pytest.mark.gpu

RATIOS = {}
IDS = lambda s: "U%d-S%d-d%d%s" % (s[0], s[1], s[2], "-" + s[3] if s[3] else "")


@pytest.fixture(scope="module")
def ops():
    from tensorrec_amd import ops as _ops, _native
    _native.require_gpu()
    _native.load()
    _native.set_tuning("softmax_shared", 1)             # the route under test, whatever the shipped default is
    yield _ops
    _native.clear_tuning("softmax_shared")
    out = os.environ.get("TREC_SOFTMAX_SHARED_RATIOS_OUT")
    if out:
        write_ratios(out)


@pytest.fixture(scope="module")
def N(ops):
    from tensorrec_amd import _native
    return _native


def write_ratios(path):
    """profiles/softmax_shared_reference_ratios.json: the ratios of this run, merged (as maxima) into the record the file already holds"""
    rec = {"what": "largest |result - float64 reference| / bar per configuration and output over the cases of "
                   "tests/test_gpu_softmax_shared.py (bars: tests/softmax_shared_reference.py); a bar of 0 asks for equality and records 0",
           "command": "TREC_SOFTMAX_SHARED_RATIOS_OUT=<this file> python -m pytest -m gpu tests/test_gpu_softmax_shared.py", "ratios": {}}
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
    """check(), with the figure printed and the largest error / bar kept per key and output (a bar of 0 asks for equality)"""
    g, w, b = f64(got).reshape(-1), f64(want).reshape(-1), f64(bar).reshape(-1)
    if g.shape == w.shape and g.size and np.isfinite(g).all():
        err = np.abs(g - w)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = float(np.where(err == 0, 0.0, err / b).max())
        print("ratio %-28s %-24s %-12s %.4g" % (key, what, name, r))
        RATIOS.setdefault(key, {})[name] = max(RATIOS.get(key, {}).get(name, 0.0), r)
    check(got, want, bar, "%s %s: %s" % (key, what, name))


def interactions_of(case):
    from tensorrec_amd.sparse import Interactions
    inter = Interactions(case.matrix, case.n_users, case.n_items, "cuda")
    assert np.array_equal(inter.indptr.cpu().numpy(), case.indptr) and np.array_equal(inter.values.cpu().numpy(), case.values)
    assert np.array_equal(inter.x_item32.cpu().numpy(), case.x_item)
    return inter


def run_step(ops, case, inter, biased, temperature, variant):
    out = ops.softmax_shared_step(dev(case.U), dev(case.V), dev(case.ub) if biased else None, dev(case.ib) if biased else None, inter,
                                  dev(case.row), temperature, sample_log_q=dev(case.log_q) if variant == "logq" else None,
                                  log_q_correction=variant != "plain")
    torch.cuda.synchronize()
    return SimpleNamespace(**{k: (v.cpu().numpy() if v is not None else None) for k, v in zip(R.OP_RESULTS, out)})


def hold_step(key, what, case, got, ref, biased):
    assert (got.d_ub is None) == (not biased) and (got.d_ib is None) == (not biased)
    for name in R.OUTPUTS:
        if name in ("d_ub", "d_ib") and not biased:
            continue
        held(key, name, getattr(got, name), getattr(ref, name), getattr(ref, "b_" + name), what)
    # exact zeros: where every term is zero
    pos = case.values > 0
    lens = np.diff(case.indptr)
    users_without = [u for u in range(case.n_users) if not pos[case.indptr[u]:case.indptr[u + 1]].any()]
    for u in users_without:
        assert not got.dU[u].any() and (not biased or got.d_ub[u] == 0), u
    untouched = np.setdiff1d(np.arange(case.n_items), np.concatenate([case.x_item, case.row]))
    assert not got.dV[untouched].any() and (not biased or not got.d_ib[untouched].any())
    if case.planted:
        assert lens[R.U_NONE] == 0 and R.U_NONE in users_without
        nonpos = np.flatnonzero(~pos)
        assert nonpos.size >= 2                                      # (pos_slot < 0: they reach no output but the zero d_pred)


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("exact", [False, True], ids=["real", "dyadic"])
@pytest.mark.parametrize("spec", R.GPU_CASES, ids=IDS)
def test_shared_step_against_float64(ops, N, spec, exact):
    """all six results of ops.softmax_shared_step; the options cycle over the cases and are all crossed on the core case; the dyadic
    family holds pred_serial bit for bit; a second call is bit-identical (slot 1 repeats the id of slot 0 in every case with S >= 2)"""
    case = R.cached_case(spec, exact)
    inter = interactions_of(case)
    assert ops.softmax_shared_supported(case.S, inter, case.d) and R.supported(case.S, case.d)
    assert N.query("trec_softmax_shared_slices", case.n_users, case.S, case.d) == R.slices(case.n_users, case.S, case.d)
    k = R.GPU_CASES.index(spec)
    for biased, T, variant in (R.ALL_OPTIONS if spec == R.CORE else [R.options_of(k)]):
        ref = R.cached_ref(spec, exact, biased, T, variant)
        got = run_step(ops, case, inter, biased, T, variant)
        what = "%s bias %d T %g" % (IDS(spec), biased, T)
        hold_step("kernel %s %s" % (variant, "dyadic" if exact else "real"), what, case, got, ref, biased)
        if exact:
            assert not ref.b_pred_serial.any() and np.array_equal(got.pred_serial.astype(np.float64), ref.pred_serial)
        again = run_step(ops, case, inter, biased, T, variant)
        for name in R.OUTPUTS:
            a, b = getattr(got, name), getattr(again, name)
            assert (a is None and b is None) or np.array_equal(a, b), (what, name)
    if case.S >= 2:
        assert case.row[0] == case.row[1]


@pytest.mark.parametrize("n_slices", [1, 2, 3])
def test_forced_slice_counts(ops, N, n_slices):
    """the dV role with the user range cut into 1, 2 and 3 slices (the last one ragged: 300 = 128 + 128 + 44 = 160 + 140)"""
    case = R.cached_case(R.SLICED, False)
    inter = interactions_of(case)
    biased, T, variant = True, 0.25, "logq"
    ref = R.cached_ref(R.SLICED, False, biased, T, variant)
    with tunings(N, softmax_shared_slices=n_slices):
        assert N.query("trec_softmax_shared_slices", case.n_users, case.S, case.d) == n_slices
        got = run_step(ops, case, inter, biased, T, variant)
        again = run_step(ops, case, inter, biased, T, variant)
    hold_step("kernel slices %d" % n_slices, IDS(R.SLICED), case, got, ref, biased)
    for name in R.OUTPUTS:
        assert np.array_equal(getattr(got, name), getattr(again, name)), name


def test_uncovered_shapes_are_refused(ops, N):
    case = R.cached_case((31, 31, 36, ""), False)
    inter = interactions_of(case)
    for S, d in R.UNCOVERED:
        assert not ops.softmax_shared_supported(S, inter, d)
    with tunings(N, softmax_shared=0):
        assert not ops.softmax_shared_supported(case.S, inter, case.d)
    with pytest.raises(ValueError, match="covers"):
        ops.softmax_shared_step(dev(np.zeros((31, 132), np.float32)), dev(np.zeros((case.n_items, 132), np.float32)), None, None, inter,
                                dev(case.row), 1.0)
    with pytest.raises(ValueError, match="temperature"):
        ops.softmax_shared_step(dev(case.U), dev(case.V), None, None, inter, dev(case.row), 0.0)
    with pytest.raises(ValueError, match="vector"):
        ops.softmax_shared_step(dev(case.U), dev(case.V), None, None, inter, dev(case.samples), 1.0)


# ------------------------------------------------------------------------------------------------ the model
N_USERS, N_ITEMS, S_MODEL, D_MODEL = 129, 200, 65, 36
MODEL_CONFIGS = {"dot-bias": ("dot", True), "dot-nobias": ("dot", False), "cosine-bias": ("cosine", True)}


def model_data():
    rng = np.random.default_rng(23)
    dense = (rng.random((N_USERS, N_ITEMS)) < 0.06).astype(np.float32)
    dense *= np.where(rng.random(dense.shape) < 0.85, 1.0, -1.0).astype(np.float32)
    dense[4, :] = 0                                   # a user without interactions
    dense[9, :] = -np.abs(dense[9, :])                # a user with negative interactions only
    dense[9, 3] = -1.0
    inter = sp.csr_matrix(dense)
    uf = sp.identity(N_USERS, dtype=np.float32, format="csr")
    itf = sp.identity(N_ITEMS, dtype=np.float32, format="csr")
    row = rng.choice(N_ITEMS, size=S_MODEL, replace=False).astype(np.int32)
    row[1] = row[0]                                   # a duplicated id
    return inter, uf, itf, row.reshape(1, S_MODEL)


def make_model(T, kind, biased, sampler, d=D_MODEL, temperature=0.5, shared=True, hits=False, cls=None, **kw):
    from tensorrec_amd.loss_graphs import SampledSoftmaxLossGraph
    from tensorrec_amd.prediction_graphs import (DotProductPredictionGraph, CosineSimilarityPredictionGraph,
                                                 EuclideanSimilarityPredictionGraph)
    graph = (cls or SampledSoftmaxLossGraph)(temperature, remove_accidental_hits=hits, shared_negatives=shared)
    pred = {"dot": DotProductPredictionGraph, "cosine": CosineSimilarityPredictionGraph, "euclid": EuclideanSimilarityPredictionGraph}[kind]()
    return T.TensorRec(n_components=d, prediction_graph=pred, loss_graph=graph, biased=biased, seed=3, sampler=sampler, **kw)


def float64_model_step(N, w, inter, row, kind, biased, temperature):
    """(output, float64 value, bar) of one step from the weights: softmax_shared_reference.ref_step on the tables the step is handed --
    the weights themselves (identity features) or, for cosine, their float32 normalised rows, whose backward is through_norm"""
    U, V = w["linear_weights_user_0"], w["linear_weights_item"]
    norms = None
    if kind == "cosine":
        (U, inv_u), (V, inv_v) = normalised(N, U), normalised(N, V)
        norms = (inv_u, inv_v)
    m = sp.csr_matrix(inter)
    samples = np.ascontiguousarray(np.broadcast_to(row.reshape(-1), (N_USERS, S_MODEL)))
    case = SimpleNamespace(U=U, V=V, ub=w["user_feature_biases"].reshape(-1) if biased else None,
                           ib=w["item_feature_biases"].reshape(-1) if biased else None, indptr=m.indptr.astype(np.int64),
                           x_item=m.indices.astype(np.int32), cols=m.indices.astype(np.int32), values=m.data.astype(np.float32),
                           samples=samples, items=samples, row=row.reshape(-1), log_q=None, S=S_MODEL, d=D_MODEL, n_users=N_USERS,
                           n_items=N_ITEMS, exact=False)
    ref = R.ref_step(case, biased, temperature, "plain")
    dU, bU, dV, bV = ref.dU, ref.b_dU, ref.dV, ref.b_dV
    if norms is not None:
        dU, bU = through_norm(U, norms[0], dU, bU)
        dV, bV = through_norm(V, norms[1], dV, bV)
    wants = [("pred_serial", ref.pred_serial, ref.b_pred_serial), ("loss", ref.loss, ref.b_loss),
             ("d linear_weights_user_0", dU, bU), ("d linear_weights_item", dV, bV)]
    if biased:
        wants += [("d user_feature_biases", ref.d_ub, ref.b_d_ub), ("d item_feature_biases", ref.d_ib, ref.b_d_ib)]
    return wants


def one_step(T, N, kind, biased, mfma=True):
    inter, uf, itf, row = model_data()
    model = make_model(T, kind, biased, T.ReplaySampler([row]))
    model.build(N_USERS, N_ITEMS)
    w = model.get_weights()
    if biased:
        r2 = np.random.default_rng(7)
        w["user_feature_biases"] = (0.1 * r2.standard_normal(w["user_feature_biases"].shape)).astype(np.float32)
        w["item_feature_biases"] = (0.1 * r2.standard_normal(w["item_feature_biases"].shape)).astype(np.float32)
        model.set_weights(w)
    w = {k: v.copy() for k, v in model.get_weights().items()}
    model._capture = {}
    with tunings(N, softmax_shared=1 if mfma else 0):
        model.fit_partial(inter, uf, itf, epochs=1, learning_rate=0.05, alpha=1e-4, n_sampled_items=S_MODEL)
    return model, w, inter, row


@pytest.mark.parametrize("config", sorted(MODEL_CONFIGS))
def test_one_fit_step_against_float64(ops, N, config):
    """the MFMA route inside a fit, and the expanded generic step (tuning softmax_shared = 0) beside it: each within the bars of the
    float64 step"""
    import tensorrec_amd as T
    kind, biased = MODEL_CONFIGS[config]
    for mfma in (True, False):
        model, w, inter, row = one_step(T, N, kind, biased, mfma=mfma)
        assert model.last_step_form == "eager" and model.last_step_kernel == ("softmax_shared" if mfma else None)
        wants = float64_model_step(N, w, inter, row, kind, biased, 0.5)
        key = "model %s %s" % (config, "shared" if mfma else "generic")
        for name, want, bar in wants:
            cap = model._capture
            got = cap[name] if name in cap else cap["grads"][name[2:]]
            held(key, name, np.asarray(got).reshape(-1), want, bar, "")


def test_which_kernel_and_form_a_fit_reports(ops, N):
    import tensorrec_amd as T
    inter, uf, itf, row = model_data()
    fit = lambda m, **kw: m.fit(inter, uf, itf, epochs=4, n_sampled_items=S_MODEL, **kw)
    for kind in ("dot", "cosine"):
        m = make_model(T, kind, True, T.ReplaySampler([row]))
        assert m.last_step_kernel is None
        fit(m)                                                       # four epochs: a per-user fit of this size would replay a graph
        assert m.last_step_kernel == "softmax_shared" and m.last_step_form == "eager"

    class Mine(T.loss_graphs.SampledSoftmaxLossGraph):               # a subclass may override anything: the generic step
        pass
    for m in (make_model(T, "euclid", False, T.ReplaySampler([row])), make_model(T, "dot", True, T.ReplaySampler([row]), hits=True),
              make_model(T, "dot", True, T.ReplaySampler([row]), cls=Mine), make_model(T, "dot", True, T.ReplaySampler([row]), d=6)):
        fit(m)
        assert m.last_step_kernel is None and m.last_step_form == "eager"
    with tunings(N, softmax_shared=0):
        m = make_model(T, "dot", True, T.ReplaySampler([row]))
        fit(m)
        assert m.last_step_kernel is None and m.last_step_form == "eager"


def test_shared_negatives_off_takes_the_route_it_took(ops, N):
    """the flag off: the per-user table, the fused kernel, graph replay -- and, in a deterministic fit, the same weights bit for bit
    whatever softmax_shared says"""
    import tensorrec_amd as T
    inter, uf, itf, _ = model_data()
    rec = Recording(T.DeviceSampler(seed=11))
    out = []
    for tuning in (1, 0):
        with tunings(N, softmax_shared=tuning):
            m = make_model(T, "dot", True, None, d=16, shared=False)
            m.fit(inter, uf, itf, epochs=6, learning_rate=0.05, n_sampled_items=12)
            assert m.last_step_kernel == "softmax_fused" and m.last_step_form == "graph"
            m = make_model(T, "dot", True, rec, d=16, shared=False, deterministic=True)
            m.fit(inter, uf, itf, epochs=3, learning_rate=0.05, n_sampled_items=12)
            assert m.last_step_kernel == "softmax_fused" and m.last_step_form == "eager"
        out.append(m.get_weights())
    assert [(c[0], c[3].shape) for c in rec.calls] == [(N_USERS, (N_USERS, 12))] * 6
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k


class Recording(object):
    """a sampler that keeps what the wrapped sampler was asked for and what it drew"""

    def __init__(self, inner):
        self.inner, self.calls = inner, []
        if hasattr(inner, "log_q"):
            self.log_q = inner.log_q

    def sample(self, n_items, n_users, n_sampled_items, replace, step, device, user_base=0):
        t = self.inner.sample(n_items, n_users, n_sampled_items, replace, step, device, user_base)
        self.calls.append((n_users, user_base, step, t.cpu().numpy().copy()))
        return t


@pytest.mark.parametrize("which", ["device", "popularity"])
def test_samplers_draw_one_row_per_step(ops, which):
    import tensorrec_amd as T
    inter, uf, itf, _ = model_data()
    inner = T.DeviceSampler(seed=11) if which == "device" else T.PopularitySampler(inter, power=0.75, smoothing=1.0, seed=5)
    rec = Recording(inner)
    from tensorrec_amd.loss_graphs import SampledSoftmaxLossGraph
    m = T.TensorRec(n_components=D_MODEL, loss_graph=SampledSoftmaxLossGraph(0.5, log_q_correction=which == "popularity",
                                                                            shared_negatives=True), seed=3, sampler=rec)
    for _ in range(3):
        m.fit_partial(inter, uf, itf, epochs=1, n_sampled_items=S_MODEL)
        assert m.last_step_kernel == "softmax_shared"
    assert [(c[0], c[1]) for c in rec.calls] == [(1, 0)] * 3 and [c[2] for c in rec.calls] == [1, 2, 3]
    rows = [c[3] for c in rec.calls]
    assert all(r.shape == (1, S_MODEL) and (r >= 0).all() and (r < N_ITEMS).all() for r in rows)
    assert not np.array_equal(rows[0], rows[1]) and not np.array_equal(rows[1], rows[2])
    if which == "device":
        assert all(np.unique(r).size == S_MODEL for r in rows)       # without replacement: S distinct items


def test_thirty_steps_lower_the_loss(ops):
    import tensorrec_amd as T
    inter, uf, itf = T.util.generate_dummy_data(num_users=60, num_items=90, interaction_density=.08, num_user_features=40,
                                                num_item_features=50, n_features_per_user=6, n_features_per_item=7, random_state=3)
    inter, uf, itf = sp.csr_matrix(inter), sp.csr_matrix(uf), sp.csr_matrix(itf)
    model = make_model(T, "dot", True, None, d=16)
    sums = []
    for _ in range(30):
        model._capture = {}
        model.fit_partial(inter, uf, itf, epochs=1, learning_rate=0.05, n_sampled_items=40)
        assert model.last_step_kernel == "softmax_shared"
        sums.append(float(np.asarray(model._capture["loss"]).sum()))
    model._capture = None
    assert np.isfinite(sums).all() and sums[-1] < sums[0], sums
