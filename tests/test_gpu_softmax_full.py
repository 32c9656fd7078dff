"""The full softmax over the catalogue (SoftmaxDenseLossGraph) against the float64 references of tests/softmax_full_reference.py, per
element and per output, within the bars derived there (tests/test_softmax_full_reference_host.py shows on the CPU that float32
restatements lie inside them and seeded defects outside), and both routes inside a TensorRec fit.

* generic   ops.softmax_dense_loss (csrc/loss_dense.hip) on dense predictions: n_items 1 ... 1000 with 512 | 513, the wave / workgroup
            boundary, n_users 1 / 3 / 300, a padded row stride, temperatures 1 and 0.25, a non-constant upstream gradient of both
            signs; the planted rows of softmax_full_reference.dense_case (no interaction, values <= 0 only, every item positive,
            duplicate pairs, one item 100 above the rest, all scores equal, scores spanning +-30); exact zeros; repeats bit for bit.
* streamed  ops.softmax_full_step (csrc/softmax_shared.hip): users and items 1 ... 1000 over the tile and workgroup edges, d 4 / 36 /
            64 / 128, with and without biases, forced slice counts 1, 2, 3; the same planted rows; d user_bias and the dU row of a user
            without positives exactly 0; the dyadic family bit for bit on pred_serial; repeats bit for bit.
* model     one captured step (dot with / without biases, cosine) on the streamed route and on the generic one (tuning softmax_full
            = 1 / 0), each against the float64 composition, and against each other through it; Euclidean scores on the generic route
            (loss and serial predictions); the kernel a fit reports; a user_batch_size fit; a 30-step fit; a saved and reloaded model.

The largest error / bar per output is kept in RATIOS; with TREC_SOFTMAX_FULL_RATIOS_OUT=<file> it is written there at the end
(profiles/softmax_full_reference_ratios.json)."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import softmax_full_reference as R
from pair_reference import f64, U32, MODE_EUCLID, ref_pair_scores, score_bar
from test_gpu_pair_kernels import check, dev, tunings
from test_gpu_softmax_fused import normalised, through_norm

pytestmark = pytest.mark.gpu

RATIOS = {}
IDS = lambda s: "x".join(str(v) for v in s)


@pytest.fixture(scope="module")
def ops():
    from tensorrec_amd import ops as _ops, _native
    _native.require_gpu()
    _native.load()
    _native.set_tuning("softmax_full", 1)               # the route under test, whatever the shipped default is
    yield _ops
    _native.clear_tuning("softmax_full")
    out = os.environ.get("TREC_SOFTMAX_FULL_RATIOS_OUT")
    if out:
        write_ratios(out)


@pytest.fixture(scope="module")
def N(ops):
    from tensorrec_amd import _native
    return _native


def write_ratios(path):
    """profiles/softmax_full_reference_ratios.json: the ratios of this run, merged (as maxima) into the record the file already holds"""
    rec = {"what": "largest |result - float64 reference| / bar per configuration and output over the cases of "
                   "tests/test_gpu_softmax_full.py (bars: tests/softmax_full_reference.py); a bar of 0 asks for equality and records 0",
           "command": "TREC_SOFTMAX_FULL_RATIOS_OUT=<this file> python -m pytest -m gpu tests/test_gpu_softmax_full.py", "ratios": {}}
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


class RawInteractions(object):
    """what the ops read of a sparse.Interactions, built from CSR arrays as they are: duplicate (user, item) entries stay (the class
    itself sums them at upload), each its own positive"""

    def __init__(self, case):
        self.shape = (case.n_users, case.n_items)
        self.nnz, self.n_positive = int(case.x_item.size), int(case.n_positive)
        lens = np.diff(case.indptr)
        self.max_row_nnz = int(lens.max()) if lens.size and self.nnz else 0
        self.max_col_nnz = int(np.bincount(case.x_item, minlength=1).max()) if self.nnz else 0
        self.indptr, self.pos_slot = dev(case.indptr), dev(case.pos_slot)
        self.x_item32, self.x_user32 = dev(case.x_item), dev(case.xu.astype(np.int32))
        order = np.argsort(case.x_item, kind="stable")
        indptr_t = np.zeros(case.n_items + 1, np.int64)
        indptr_t[1:] = np.cumsum(np.bincount(case.x_item, minlength=case.n_items))
        self._t = (dev(indptr_t), dev(case.xu[order].astype(np.int32)), dev(order.astype(np.int32)))

    def transposed(self):
        return self._t


def users_without_positives(case):
    pos = case.values > 0
    return [u for u in range(case.n_users) if not pos[case.indptr[u]:case.indptr[u + 1]].any()]


# ------------------------------------------------------------------------------------------------ the generic kernels
def run_dense(ops, case, inter, temperature, pad=0):
    """(loss, d_pred) of ops.softmax_dense_loss under the upstream gradient case.go; pad > 0: the prediction is a view of a tensor
    with `pad` more columns (their gradient must stay 0)"""
    wide = torch.full((case.n_users, case.n_items + pad), 1e30, dtype=torch.float32, device="cuda")
    wide[:, :case.n_items] = dev(case.pred)
    wide.requires_grad_(True)
    pred = wide[:, :case.n_items] if pad else wide
    loss = ops.softmax_dense_loss(pred, inter, temperature)
    loss.backward(dev(case.go))
    torch.cuda.synchronize()
    g = wide.grad.cpu().numpy()
    assert not g[:, case.n_items:].any()
    return loss.detach().cpu().numpy(), g[:, :case.n_items]


@pytest.mark.parametrize("spec", R.DENSE_CASES, ids=IDS)
def test_dense_kernels_against_float64(ops, spec):
    case = R.cached_dense_case(spec)
    inter = RawInteractions(case)
    for T in R.TEMPERATURES:
        ref = R.cached_dense_ref(spec, T)
        loss, d_pred = run_dense(ops, case, inter, T)
        key, what = "generic T %g" % T, IDS(spec)
        held(key, "loss", loss, ref.loss, ref.b_loss, what)
        held(key, "d_pred", d_pred, ref.d_pred, ref.b_d_pred, what)
        no = users_without_positives(case)
        assert not d_pred[no].any()
        loss2, d_pred2 = run_dense(ops, case, inter, T)
        assert np.array_equal(loss, loss2) and np.array_equal(d_pred, d_pred2)
    if case.planted:
        assert R.U_NONE in no and R.U_NONPOS in no and (np.diff(case.x_item[case.indptr[R.U_DUP]:case.indptr[R.U_DUP + 1]]) == 0).any()


def test_dense_kernels_honour_a_padded_row_stride(ops):
    case = R.cached_dense_case(R.DENSE_PADDED)
    inter = RawInteractions(case)
    ref = R.cached_dense_ref(R.DENSE_PADDED, 0.25)
    plain = run_dense(ops, case, inter, 0.25)
    padded = run_dense(ops, case, inter, 0.25, pad=7)
    held("generic padded", "loss", padded[0], ref.loss, ref.b_loss, IDS(R.DENSE_PADDED))
    held("generic padded", "d_pred", padded[1], ref.d_pred, ref.b_d_pred, IDS(R.DENSE_PADDED))
    assert np.array_equal(plain[0], padded[0]) and np.array_equal(plain[1], padded[1])


def test_dense_loss_refuses_what_it_cannot_take(ops):
    case = R.cached_dense_case((3, 257))
    inter = RawInteractions(case)
    with pytest.raises(ValueError, match="shape"):
        ops.softmax_dense_loss(dev(case.pred[:, :200]), inter, 1.0)
    with pytest.raises(ValueError, match="temperature"):
        ops.softmax_dense_loss(dev(case.pred), inter, 0.0)


# ------------------------------------------------------------------------------------------------ the streamed step
def run_step(ops, case, inter, biased, temperature):
    out = ops.softmax_full_step(dev(case.U), dev(case.V), dev(case.ub) if biased else None, dev(case.ib) if biased else None, inter,
                                temperature)
    torch.cuda.synchronize()
    return SimpleNamespace(**{k: (v.cpu().numpy() if v is not None else None) for k, v in zip(R.OP_RESULTS, out)})


def hold_step(key, what, case, got, ref, biased):
    assert (got.d_ub is None) == (not biased) and (got.d_ib is None) == (not biased)
    for name in R.OUTPUTS:
        if name in ("d_ub", "d_ib") and not biased:
            continue
        held(key, name, getattr(got, name), getattr(ref, name), getattr(ref, "b_" + name), what)
    if biased:
        assert not got.d_ub.view(np.uint32).any()                    # 0.f exactly, every user
    no = users_without_positives(case)
    assert not got.dU[no].any()
    if case.planted:
        assert R.U_NONE in no and R.U_NONPOS in no


@pytest.mark.parametrize("exact", [False, True], ids=["real", "dyadic"])
@pytest.mark.parametrize("spec", R.GPU_CASES, ids=IDS)
def test_full_step_against_float64(ops, N, spec, exact):
    case = R.cached_case(spec, exact)
    inter = RawInteractions(case)
    assert R.tile_supported(case.n_items, case.d) and ops.step_covers("softmax_shared", case.n_items, 0, case.d)
    assert N.query("trec_softmax_shared_slices", case.n_users, case.n_items, case.d) == R.slices(case.n_users, case.n_items, case.d)
    k = R.GPU_CASES.index(spec)
    options = [(b, T) for b in (True, False) for T in R.TEMPERATURES] if spec == (33, 33, 128) else [R.options_of(k)]
    for biased, T in options:
        ref = R.cached_ref(spec, exact, biased, T)
        got = run_step(ops, case, inter, biased, T)
        what = "%s bias %d T %g" % (IDS(spec), biased, T)
        hold_step("streamed %s" % ("dyadic" if exact else "real"), what, case, got, ref, biased)
        if exact:
            assert not ref.b_pred_serial.any() and np.array_equal(got.pred_serial.astype(np.float64), ref.pred_serial)
        again = run_step(ops, case, inter, biased, T)
        for name in R.OUTPUTS:
            a, b = getattr(got, name), getattr(again, name)
            assert (a is None and b is None) or np.array_equal(a, b), (what, name)


@pytest.mark.parametrize("spec", R.LONG_CASES, ids=IDS)
def test_long_rows_and_popular_items(ops, spec):
    """a user with more than 2,048 positives, an item more than 2,048 users hold: the positives' K1 gathers take their chunked form,
    over the items accumulating onto what the tiles wrote"""
    case = R.cached_case(spec, False)
    inter = RawInteractions(case)
    assert (inter.max_col_nnz if spec[3] == "popular" else inter.max_row_nnz) > ops.SPLIT_T == R.SPLIT_T
    ref = R.cached_ref(spec, False, True, 0.25)
    got = run_step(ops, case, inter, True, 0.25)
    hold_step("streamed long", IDS(spec), case, got, ref, True)
    again = run_step(ops, case, inter, True, 0.25)
    for name in R.OUTPUTS:
        assert np.array_equal(getattr(got, name), getattr(again, name)), name


@pytest.mark.parametrize("n_slices", [1, 2, 3])
def test_forced_slice_counts(ops, N, n_slices):
    case = R.cached_case(R.SLICED, False)
    inter = RawInteractions(case)
    ref = R.cached_ref(R.SLICED, False, True, 0.25)
    with tunings(N, softmax_shared_slices=n_slices):
        assert N.query("trec_softmax_shared_slices", case.n_users, case.n_items, case.d) == n_slices
        got = run_step(ops, case, inter, True, 0.25)
        again = run_step(ops, case, inter, True, 0.25)
    hold_step("streamed slices %d" % n_slices, IDS(R.SLICED), case, got, ref, True)
    for name in R.OUTPUTS:
        assert np.array_equal(getattr(got, name), getattr(again, name)), name


def test_both_routes_agree_through_the_reference(ops):
    """the generic kernels on the float64-rounded scores of a streamed case against the streamed step: each within its own bars of
    the same float64 loss"""
    spec = (129, 127, 128)
    case = R.cached_case(spec, True)                                 # dyadic: the float32 scores are exact, both routes see the same
    inter = RawInteractions(case)
    ref = R.cached_ref(spec, True, True, 0.25)
    got = run_step(ops, case, inter, True, 0.25)
    dense = SimpleNamespace(pred=ref.scores.astype(np.float32), go=np.ones(case.n_positive, np.float32), **{
        k: getattr(case, k) for k in ("n_users", "n_items", "indptr", "x_item", "values", "pos_slot", "xu", "n_positive")})
    assert np.array_equal(dense.pred.astype(np.float64), ref.scores)
    dref = R.ref_dense(dense.pred, dense, dense.go, 0.25)
    loss, d_pred = run_dense(ops, dense, inter, 0.25)
    held("routes agree", "loss generic", loss, dref.loss, dref.b_loss, IDS(spec))
    held("routes agree", "loss streamed", got.loss, ref.loss, ref.b_loss, IDS(spec))
    assert (np.abs(dref.loss - ref.loss) <= 1e-12 * np.maximum(1.0, np.abs(ref.loss))).all()
    assert (np.abs(f64(loss) - f64(got.loss)) <= dref.b_loss + ref.b_loss).all()
    held("routes agree", "d_pred generic", d_pred, ref.g, dref.b_d_pred, IDS(spec))
    dU = f64(d_pred) @ f64(case.V)
    assert (np.abs(dU - f64(got.dU)) <= ref.b_dU + dref.b_d_pred @ np.abs(f64(case.V))).all()


def test_uncovered_shapes_are_refused(ops):
    case = R.cached_case((31, 31, 36), False)
    inter = RawInteractions(case)
    with pytest.raises(ValueError, match="covers"):
        ops.softmax_full_step(dev(np.zeros((31, 132), np.float32)), dev(np.zeros((31, 132), np.float32)), None, None, inter, 1.0)
    with pytest.raises(ValueError, match="temperature"):
        ops.softmax_full_step(dev(case.U), dev(case.V), None, None, inter, 0.0)
    with pytest.raises(ValueError, match="shape"):
        ops.softmax_full_step(dev(case.U[:30]), dev(case.V), None, None, inter, 1.0)


# ------------------------------------------------------------------------------------------------ the model
N_USERS, N_ITEMS, D_MODEL = R.MODEL
MODEL_CONFIGS = {"dot-bias": ("dot", True), "dot-nobias": ("dot", False), "cosine-bias": ("cosine", True)}
TEMPERATURE = 0.5


def model_data():
    rng = np.random.default_rng(23)
    dense = (rng.random((N_USERS, N_ITEMS)) < 0.06).astype(np.float32)
    dense *= np.where(rng.random(dense.shape) < 0.85, 1.0, -1.0).astype(np.float32)
    dense[4, :] = 0                                   # a user without interactions
    dense[9, :] = -np.abs(dense[9, :])                # a user with negative interactions only
    dense[9, 3] = -1.0
    dense[11, :] = 2.0                                # a user with every item positive
    return (sp.csr_matrix(dense), sp.identity(N_USERS, dtype=np.float32, format="csr"),
            sp.identity(N_ITEMS, dtype=np.float32, format="csr"))


def make_model(T, kind, biased, d=D_MODEL, cls=None, **kw):
    from tensorrec_amd.loss_graphs import SoftmaxDenseLossGraph
    from tensorrec_amd.prediction_graphs import (DotProductPredictionGraph, CosineSimilarityPredictionGraph,
                                                 EuclideanSimilarityPredictionGraph)
    pred = {"dot": DotProductPredictionGraph, "cosine": CosineSimilarityPredictionGraph, "euclid": EuclideanSimilarityPredictionGraph}[kind]()
    return T.TensorRec(n_components=d, prediction_graph=pred, loss_graph=(cls or SoftmaxDenseLossGraph)(TEMPERATURE), biased=biased,
                       seed=3, **kw)


def case_of(w, inter, U, V, biased):
    m = sp.csr_matrix(inter)
    values = m.data.astype(np.float32)
    pos = values > 0
    return SimpleNamespace(U=U, V=V, ub=w["user_feature_biases"].reshape(-1) if biased else None,
                           ib=w["item_feature_biases"].reshape(-1) if biased else None, indptr=m.indptr.astype(np.int64),
                           x_item=m.indices.astype(np.int32), values=values, d=U.shape[1], n_users=N_USERS, n_items=N_ITEMS,
                           pos_slot=np.where(pos, np.cumsum(pos) - 1, -1).astype(np.int32), exact=False, n_positive=int(pos.sum()),
                           xu=np.repeat(np.arange(N_USERS), np.diff(m.indptr)).astype(np.int64))


def float64_model_step(N, w, inter, kind, biased, route):
    """(output, float64 value, bar) of one step from the weights: softmax_full_reference.ref_step on the tables the step is handed --
    the weights themselves (identity features) or, for cosine, their float32 normalised rows, whose backward is through_norm"""
    U, V = w["linear_weights_user_0"], w["linear_weights_item"]
    norms = None
    if kind == "cosine":
        (U, inv_u), (V, inv_v) = normalised(N, U), normalised(N, V)
        norms = (inv_u, inv_v)
    ref = R.ref_step(case_of(w, inter, U, V, biased), biased, TEMPERATURE, route)
    dU, bU, dV, bV = ref.dU, ref.b_dU, ref.dV, ref.b_dV
    if norms is not None:
        dU, bU = through_norm(U, norms[0], dU, bU)
        dV, bV = through_norm(V, norms[1], dV, bV)
    wants = [("pred_serial", ref.pred_serial, ref.b_pred_serial), ("loss", ref.loss, ref.b_loss),
             ("d linear_weights_user_0", dU, bU), ("d linear_weights_item", dV, bV)]
    if biased:
        wants += [("d user_feature_biases", ref.d_ub, ref.b_d_ub), ("d item_feature_biases", ref.d_ib, ref.b_d_ib)]
    return wants


def one_step(T, N, kind, biased, streamed):
    inter, uf, itf = model_data()
    model = make_model(T, kind, biased)
    model.build(N_USERS, N_ITEMS)
    w = model.get_weights()
    if biased:
        r2 = np.random.default_rng(7)
        w["user_feature_biases"] = (0.1 * r2.standard_normal(w["user_feature_biases"].shape)).astype(np.float32)
        w["item_feature_biases"] = (0.1 * r2.standard_normal(w["item_feature_biases"].shape)).astype(np.float32)
        model.set_weights(w)
    w = {k: v.copy() for k, v in model.get_weights().items()}
    model._capture = {}
    with tunings(N, softmax_full=1 if streamed else 0):
        model.fit_partial(inter, uf, itf, epochs=1, learning_rate=0.05, alpha=1e-4)
    return model, w, inter


def captured(model, name):
    cap = model._capture
    return np.asarray(cap[name] if name in cap else cap["grads"][name[2:]]).reshape(-1)


@pytest.mark.parametrize("config", sorted(MODEL_CONFIGS))
def test_one_fit_step_against_float64(ops, N, config):
    """the streamed route inside a fit and the generic one (tuning softmax_full = 0) beside it: each within the bars of the float64
    step, and within the sum of both bars of each other"""
    import tensorrec_amd as T
    kind, biased = MODEL_CONFIGS[config]
    seen = {}
    for streamed in (True, False):
        model, w, inter = one_step(T, N, kind, biased, streamed)
        assert model.last_step_form == "eager" and model.last_step_kernel == ("softmax_full" if streamed else None)
        route = "streamed" if streamed else "generic"
        for name, want, bar in float64_model_step(N, w, inter, kind, biased, route):
            got = captured(model, name)
            held("model %s %s" % (config, route), name, got, want, bar, "")
            seen.setdefault(name, []).append((f64(got), f64(bar).reshape(-1)))
        if streamed and biased:
            assert not captured(model, "d user_feature_biases").view(np.uint32).any()
    for name, ((a, ba), (b, bb)) in seen.items():
        assert (np.abs(a - b) <= ba + bb).all(), name


def test_euclidean_scores_take_the_generic_route(ops, N):
    """loss and serial predictions of one captured step on Euclidean scores against float64.  The dense score is the composition
    -sqrt(max((r_u - 2 u.v) + r_i, 1e-16)): its squared distance is off by (d + 10) u (r_u + 2 sum |u v| + r_i), the root halves the
    relative error and rounds once more; the biases round once each."""
    import tensorrec_amd as T
    inter, uf, itf = model_data()
    model = make_model(T, "euclid", True)
    model.build(N_USERS, N_ITEMS)
    w = {k: v.copy() for k, v in model.get_weights().items()}
    model._capture = {}
    model.fit_partial(inter, uf, itf, epochs=1, learning_rate=0.05, alpha=1e-4)
    assert model.last_step_kernel is None and model.last_step_form == "eager"
    U, V = f64(w["linear_weights_user_0"]), f64(w["linear_weights_item"])
    ub, ib = f64(w["user_feature_biases"]).reshape(-1), f64(w["item_feature_biases"]).reshape(-1)
    c = case_of(w, inter, U, V, True)
    ru, ri = (U ** 2).sum(1)[:, None], (V ** 2).sum(1)[None, :]
    D = np.maximum(ru - 2.0 * (U @ V.T) + ri, 1e-16)
    raw = -np.sqrt(D)
    with_ub = raw + ub[:, None]
    Y = with_ub + ib[None, :]
    delta = (c.d + 10.0) * U32 * (ru + 2.0 * (np.abs(U) @ np.abs(V).T) + ri) / (2.0 * np.sqrt(D)) + U32 * (np.abs(raw) + np.abs(with_ub) + np.abs(Y))
    ref = R.ref_dense(Y, c, np.ones(c.n_positive), TEMPERATURE, delta=delta)
    held("model euclid generic", "loss", captured(model, "loss"), ref.loss, ref.b_loss, "")
    sc = ref_pair_scores(U, V, c.xu, c.x_item, MODE_EUCLID, ub, ib)
    held("model euclid generic", "pred_serial", captured(model, "pred_serial"), sc.scores, score_bar(sc, c.d), "")
    for name, g in model._capture["grads"].items():
        assert g is not None and np.isfinite(g).all(), name


def test_which_kernel_a_fit_reports(ops, N):
    import tensorrec_amd as T
    inter, uf, itf = model_data()
    fit = lambda m, **kw: m.fit(inter, uf, itf, epochs=3, **kw)
    for kind in ("dot", "cosine"):
        m = make_model(T, kind, True)
        assert m.last_step_kernel is None
        fit(m)
        assert m.last_step_kernel == "softmax_full" and m.last_step_form == "eager"
        fit(m, user_batch_size=50)                                   # 129 users in batches of 50: every batch takes the route
        assert m.last_step_kernel == "softmax_full" and m.last_step_form == "eager"
        assert all(np.isfinite(v).all() for v in m.get_weights().values())

    class Mine(T.loss_graphs.SoftmaxDenseLossGraph):                 # a subclass may override anything: the dense path
        pass
    for m in (make_model(T, "euclid", False), make_model(T, "dot", True, cls=Mine), make_model(T, "dot", True, d=6),
              make_model(T, "dot", True, d=132)):
        fit(m)
        assert m.last_step_kernel is None and m.last_step_form == "eager"
    with tunings(N, softmax_full=0):
        m = make_model(T, "dot", True)
        fit(m, user_batch_size=50)
        assert m.last_step_kernel is None and m.last_step_form == "eager"


@pytest.mark.parametrize("streamed", [True, False], ids=["streamed", "generic"])
def test_thirty_steps_lower_the_loss(ops, N, streamed):
    import tensorrec_amd as T
    inter, uf, itf = T.util.generate_dummy_data(num_users=60, num_items=90, interaction_density=.08, num_user_features=40,
                                                num_item_features=50, n_features_per_user=6, n_features_per_item=7, random_state=3)
    inter, uf, itf = sp.csr_matrix(inter), sp.csr_matrix(uf), sp.csr_matrix(itf)
    model = make_model(T, "dot", True, d=16)
    sums = []
    with tunings(N, softmax_full=1 if streamed else 0):
        for _ in range(30):
            model._capture = {}
            model.fit_partial(inter, uf, itf, epochs=1, learning_rate=0.05)
            assert model.last_step_kernel == ("softmax_full" if streamed else None)
            sums.append(float(np.asarray(model._capture["loss"]).sum()))
    model._capture = None
    assert np.isfinite(sums).all() and sums[-1] < sums[0], sums


def test_a_reloaded_model_goes_on(ops, tmp_path):
    import tensorrec_amd as T
    inter, uf, itf = model_data()
    model = make_model(T, "dot", True)
    model.fit(inter, uf, itf, epochs=2)
    model.save_model(str(tmp_path))
    back = T.TensorRec.load_model(str(tmp_path))
    assert type(back.loss_graph_factory) is T.loss_graphs.SoftmaxDenseLossGraph and back.loss_graph_factory.temperature == TEMPERATURE
    assert np.array_equal(back.predict(uf, itf), model.predict(uf, itf))
    for m in (model, back):
        m.fit_partial(inter, uf, itf, epochs=1)
        assert m.last_step_kernel == "softmax_full"
    wa, wb = model.get_weights(), back.get_weights()
    for k in wa:
        assert np.array_equal(wa[k], wb[k]), k
