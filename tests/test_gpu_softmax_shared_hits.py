"""The sampled-softmax step with shared negatives and ACCIDENTAL HITS REMOVED (csrc/softmax_shared.hip's masked instantiations,
ops.softmax_shared_hits_step) against the float64 step of tests/softmax_shared_hits_reference.py -- softmax_step_reference.ref_step,
hits removed, on the table that repeats the shared row -- per element and per output, within the bars derived there
(tests/test_softmax_shared_hits_reference_host.py shows on the CPU that a float32 restatement lies inside them and seeded defects
outside), and the route inside a TensorRec fit.

* kernel   users 1 / 31 / 33 / 129 / 300, S 1 / 31 / 32 / 33 / 65 / 1000, d 4 / 36 / 64 / 128; with and without biases, temperatures 1
           and 0.25, plain / logQ with a table / logQ uniform (cycling over the cases, all crossed on the core case); forced slice
           counts 1, 2, 3 on 300 users with hit users on both sides of every slice boundary; the planted rows of
           softmax_shared_hits_reference.hits_case (a hit at sorted column 0, at column S - 1, in the last partial tile, on a run of
           three duplicates across a tile edge, on every column, a match of value <= 0 only, a user without positives); an item that
           is a hit for every user; no hits at all against the unmasked route; exact zeros; the dyadic family bit for bit on
           pred_serial; two calls bit-identical; the hit ranges and the transposed positives integer for integer;
* model    one captured step (dot with / without biases, cosine; DeviceSampler, PopularitySampler + logQ) at 129 x 200, S = 65,
           d = 36 on the new route (tuning softmax_shared_hits = 1) and on the expanded generic step (tuning off), each against the
           float64 step; the kernel a fit reports with the tuning on and off; a 20-step fit.

The largest error / bar per output is kept in RATIOS; with TREC_SOFTMAX_SHARED_HITS_RATIOS_OUT=<file> it is written there at the end
(profiles/softmax_shared_hits_reference_ratios.json)."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import softmax_shared_hits_reference as H
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
    _native.set_tuning("softmax_shared", 1)             # the MFMA route as such, whatever the shipped default is
    yield _ops
    _native.clear_tuning("softmax_shared")
    out = os.environ.get("TREC_SOFTMAX_SHARED_HITS_RATIOS_OUT")
    if out:
        write_ratios(out)


@pytest.fixture(scope="module")
def N(ops):
    from tensorrec_amd import _native
    return _native


@pytest.fixture
def hits_on(N):
    """tuning softmax_shared_hits = 1 for one test; what was set before (nothing: the default, 0) comes back"""
    with tunings(N, softmax_shared_hits=1):
        yield


def write_ratios(path):
    """profiles/softmax_shared_hits_reference_ratios.json: the ratios of this run, merged (as maxima) into the record the file holds"""
    rec = {"what": "largest |result - float64 reference| / bar per configuration and output over the cases of "
                   "tests/test_gpu_softmax_shared_hits.py (bars: tests/softmax_shared_hits_reference.py); a bar of 0 asks for equality "
                   "and records 0",
           "command": "TREC_SOFTMAX_SHARED_HITS_RATIOS_OUT=<this file> python -m pytest -m gpu tests/test_gpu_softmax_shared_hits.py",
           "ratios": {}}
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


def as_results(out):
    torch.cuda.synchronize()
    return SimpleNamespace(**{k: (v.cpu().numpy() if v is not None else None) for k, v in zip(H.OP_RESULTS, out)})


def step_args(case, inter, biased, temperature, variant, row=None):
    return (dev(case.U), dev(case.V), dev(case.ub) if biased else None, dev(case.ib) if biased else None, inter,
            dev(case.row if row is None else row), temperature), dict(sample_log_q=dev(case.log_q) if variant == "logq" else None,
                                                                      log_q_correction=variant != "plain")


def run_step(ops, case, inter, biased, temperature, variant):
    args, kw = step_args(case, inter, biased, temperature, variant)
    return as_results(ops.softmax_shared_hits_step(*args, **kw))


def run_kernels(ops, N, case, inter, biased, temperature):
    """the entry points themselves on the sorted columns (no logQ): M, Z, tK, dVs, d b_s, the hit ranges and their counts"""
    S, d, nu, nnz = case.S, case.d, case.n_users, case.x_item.size
    u, v = dev(case.U), dev(case.V)
    ub, ib = (dev(case.ub), dev(case.ib)) if biased else (None, None)
    ids = torch.sort(dev(case.row.astype(np.int32)), stable=True)[0]
    vs = v.index_select(0, ids.long())
    bs = ib.index_select(0, ids.long()) if biased else None
    f = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    rng = torch.full((max(nnz, 1), 2), -1, dtype=torch.int32, device="cuda")
    cnt = torch.full((nu,), -1, dtype=torch.int32, device="cuda")
    N.call("trec_softmax_shared_hit_ranges", N.ptr(inter.indptr), N.ptr(inter.x_item32), N.ptr(inter.pos_slot), N.ptr(ids), nu, S,
           N.ptr(rng), N.ptr(cnt))
    M, Z, tK, pred, d_pred = f(nu), f(nu), f(nu), f(max(nnz, 1)), f(max(nnz, 1))
    loss = f(max(inter.n_positive, 1))
    inv_t = 1.0 / temperature
    N.call("trec_softmax_shared_hits_stats", N.ptr(u), N.ptr(vs), N.ptr(ub), N.ptr(bs), None, N.ptr(inter.indptr), N.ptr(rng),
           N.ptr(cnt), nu, S, d, inv_t, N.ptr(M), N.ptr(Z))
    if nnz:
        N.call("trec_pair_score_fwd", N.ptr(u), N.ptr(v), N.ptr(inter.x_user32), N.ptr(inter.x_item32), nnz, 0, d, ops.MODE_DOT,
               N.ptr(ub), N.ptr(ib), N.ptr(pred), None)
    N.call("trec_softmax_shared_positives", N.ptr(inter.indptr), N.ptr(inter.pos_slot), N.ptr(pred), N.ptr(M), N.ptr(Z), nu, inv_t,
           N.ptr(loss), N.ptr(d_pred), N.ptr(tK), None)
    n_slices = int(N.query("trec_softmax_shared_slices", nu, S, d))
    ws = f(n_slices * S * (d + 1)) if n_slices > 1 else None
    dU, dVs, dbs = torch.zeros((nu, d), dtype=torch.float32, device="cuda"), f(S, d), f(S)
    indptr_tp, users_tp = inter.transposed_positive()
    N.call("trec_softmax_shared_hits_grads", N.ptr(u), N.ptr(vs), N.ptr(ub), N.ptr(bs), None, N.ptr(M), N.ptr(tK),
           N.ptr(inter.indptr), N.ptr(rng), N.ptr(cnt), N.ptr(ids), N.ptr(indptr_tp), N.ptr(users_tp), case.n_items, nu, S, d, inv_t,
           n_slices, N.ptr(ws), N.ptr(dU), N.ptr(dVs), N.ptr(dbs))
    torch.cuda.synchronize()
    return SimpleNamespace(M=M.cpu().numpy(), Z=Z.cpu().numpy(), tK=tK.cpu().numpy(), dU=dU.cpu().numpy(), dVs=dVs.cpu().numpy(),
                           dbs=dbs.cpu().numpy(), rng=rng.cpu().numpy(), cnt=cnt.cpu().numpy(), loss=loss.cpu().numpy(),
                           d_pred=d_pred.cpu().numpy())


def hold_step(key, what, case, got, ref, biased):
    assert (got.d_ub is None) == (not biased) and (got.d_ib is None) == (not biased)
    for name in H.OUTPUTS:
        if name in ("d_ub", "d_ib") and not biased:
            continue
        assert np.isfinite(getattr(got, name)).all(), (what, name)                  # no NaN, no inf, anywhere
        held(key, name, getattr(got, name), getattr(ref, name), getattr(ref, "b_" + name), what)
    # exact zeros: a user without positives, and a user whose samples are all hits (its loss is an exact 0 as well)
    pos = case.values > 0
    slot = np.cumsum(pos) - 1
    hits = H.hit_mask(case)
    for u in range(case.n_users):
        b, e = case.indptr[u], case.indptr[u + 1]
        if not pos[b:e].any() or hits[u].all():
            assert not got.dU[u].any() and (not biased or got.d_ub[u] == 0), u
            assert not got.loss[slot[b:e][pos[b:e]]].any(), u
    untouched = np.setdiff1d(np.arange(case.n_items), np.concatenate([case.x_item, case.row]))
    assert not got.dV[untouched].any() and (not biased or not got.d_ib[untouched].any())


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("exact", [False, True], ids=["real", "dyadic"])
@pytest.mark.parametrize("spec", H.GPU_CASES, ids=IDS)
def test_hits_step_against_float64(ops, N, spec, exact):
    """all six results of ops.softmax_shared_hits_step; the options cycle over the cases and are all crossed on the core case; the
    dyadic family holds pred_serial bit for bit; a second call is bit-identical"""
    case = H.cached_case(spec, exact)
    inter = interactions_of(case)
    assert ops.step_covers("softmax_shared_hits", case.S, 0, case.d) and H.supported(case.S, case.d)
    assert not ops.softmax_shared_hits_supported(case.S, inter, case.d)             # the tuning is off unless somebody sets it
    k = H.GPU_CASES.index(spec)
    for biased, T, variant in (H.ALL_OPTIONS if spec == H.CORE else [H.options_of(k)]):
        ref = H.cached_ref(spec, exact, biased, T, variant)
        got = run_step(ops, case, inter, biased, T, variant)
        what = "%s bias %d T %g" % (IDS(spec), biased, T)
        hold_step("kernel %s %s" % (variant, "dyadic" if exact else "real"), what, case, got, ref, biased)
        if exact:
            assert not ref.b_pred_serial.any() and np.array_equal(got.pred_serial.astype(np.float64), ref.pred_serial)
        again = run_step(ops, case, inter, biased, T, variant)
        for name in H.OUTPUTS:
            a, b = getattr(got, name), getattr(again, name)
            assert (a is None and b is None) or np.array_equal(a, b), (what, name)


@pytest.mark.parametrize("n_slices", [1, 2, 3])
def test_forced_slice_counts(ops, N, n_slices):
    """the dV role with the user range cut into 1, 2 and 3 slices; users 127 | 128, 159 | 160, 255 | 256 all have a hit"""
    case = H.cached_case(H.SLICED, False)
    inter = interactions_of(case)
    assert H.hit_mask(case)[list(H.BOUNDARY_USERS)].any(1).all()
    biased, T, variant = True, 0.25, "logq"
    ref = H.cached_ref(H.SLICED, False, biased, T, variant)
    with tunings(N, softmax_shared_slices=n_slices):
        assert N.query("trec_softmax_shared_slices", case.n_users, case.S, case.d) == n_slices
        got = run_step(ops, case, inter, biased, T, variant)
        again = run_step(ops, case, inter, biased, T, variant)
    hold_step("kernel slices %d" % n_slices, IDS(H.SLICED), case, got, ref, biased)
    for name in H.OUTPUTS:
        assert np.array_equal(getattr(got, name), getattr(again, name)), name


@pytest.mark.parametrize("spec", H.GPU_CASES, ids=IDS)
def test_hit_ranges_and_transposed_lists_equal_the_host_mirror(ops, N, spec):
    """integer for integer; and the statistics of a user whose samples are all hits: M = -inf, Z = 0, tK = 0"""
    case = H.cached_case(spec, False)
    inter = interactions_of(case)
    got = run_kernels(ops, N, case, inter, True, 0.5)
    want, cnt = H.hit_ranges(case)
    assert np.array_equal(got.cnt, cnt)
    for u in range(case.n_users):
        b = int(case.indptr[u])
        assert np.array_equal(got.rng[b:b + cnt[u]], want[u]), u
    indptr_tp, users_tp = inter.transposed_positive()
    w_ptr, w_users = H.transposed_positive(case)
    assert indptr_tp.dtype == torch.int64 and users_tp.dtype == torch.int32
    assert np.array_equal(indptr_tp.cpu().numpy(), w_ptr) and np.array_equal(users_tp.cpu().numpy(), w_users)
    hits = H.hit_mask(case)
    assert np.isfinite(got.Z).all() and not np.isnan(got.M).any() and np.isfinite(got.tK).all()
    assert np.isfinite(got.dVs).all() and np.isfinite(got.dbs).all() and np.isfinite(got.dU).all()
    for u in np.flatnonzero(hits.all(1)):
        assert got.M[u] == -np.inf and got.Z[u] == 0 and got.tK[u] == 0 and not got.dU[u].any(), u
    assert (got.M[~hits.all(1)] > -np.inf).all()


def test_an_item_that_is_a_hit_for_every_user_gets_exact_zero_rows(ops, N):
    """its rows of dVs and d b_s are 0.0 exactly, in the real and in the dyadic family, and d item_in of the item is the positives' part"""
    for exact in (False, True):
        case = H.cached_case(H.EVERYONE, exact)
        inter = interactions_of(case)
        cols = np.flatnonzero(H.hit_mask(case)[:, np.argsort(case.row, kind="stable")].all(0))
        assert cols.size >= 1
        got = run_kernels(ops, N, case, inter, True, 0.5)
        assert (got.dVs[cols] == 0).all() and (got.dbs[cols] == 0).all()
        assert got.dVs.any() and got.dbs.any()


def test_no_hits_equals_the_unmasked_route(ops, N):
    """nothing to mask: both routes lie within the bars of the unmasked reference (which then equals the masked one); the row maxima
    are the same floats whatever the column order; and on a row that is sorted already the two routes do the same operations in the
    same order: all six outputs are bit-equal"""
    case = H.cached_case(H.NOHITS, False)
    inter = interactions_of(case)
    assert not H.hit_mask(case).any()
    srt = np.sort(case.row)
    for biased, T, variant in ((True, 0.25, "logq"), (False, 1.0, "plain")):
        ref = R.ref_step(case, biased, T, variant)
        masked_ref = H.cached_ref(H.NOHITS, False, biased, T, variant)
        args, kw = step_args(case, inter, biased, T, variant)
        masked, plain = as_results(ops.softmax_shared_hits_step(*args, **kw)), as_results(ops.softmax_shared_step(*args, **kw))
        for name in H.OUTPUTS:
            assert np.array_equal(getattr(ref, name), getattr(masked_ref, name)), name
            if name in ("d_ub", "d_ib") and not biased:
                continue
            held("kernel nohits masked", name, getattr(masked, name), getattr(ref, name), getattr(ref, "b_" + name), variant)
            held("kernel nohits plain", name, getattr(plain, name), getattr(ref, name), getattr(ref, "b_" + name), variant)
        assert np.array_equal(masked.pred_serial, plain.pred_serial)
        args, kw = step_args(case, inter, biased, T, variant, row=srt)
        masked_s, plain_s = as_results(ops.softmax_shared_hits_step(*args, **kw)), as_results(ops.softmax_shared_step(*args, **kw))
        for name in H.OUTPUTS:
            a, b, c = getattr(masked_s, name), getattr(plain_s, name), getattr(masked, name)
            assert (a is None and b is None) or (np.array_equal(a, b) and np.array_equal(a, c)), (variant, name)
    got = run_kernels(ops, N, case, inter, True, 0.5)
    u, vs = dev(case.U), dev(case.V).index_select(0, dev(case.row.astype(np.int64)))
    bs = dev(case.ib).index_select(0, dev(case.row.astype(np.int64)))
    M, Z = torch.empty(case.n_users, device="cuda"), torch.empty(case.n_users, device="cuda")
    N.call("trec_softmax_shared_stats", N.ptr(u), N.ptr(vs), N.ptr(dev(case.ub)), N.ptr(bs), None, case.n_users, case.S, case.d, 2.0,
           N.ptr(M), N.ptr(Z))
    torch.cuda.synchronize()
    assert np.array_equal(M.cpu().numpy(), got.M) and not got.cnt.any()


def test_uncovered_shapes_are_refused(ops, N):
    case = H.cached_case((31, 31, 36, ""), False)
    inter = interactions_of(case)
    for S, d in R.UNCOVERED:
        assert not ops.step_covers("softmax_shared_hits", S, 0, d)
    with tunings(N, softmax_shared_hits=1):
        assert ops.softmax_shared_hits_supported(case.S, inter, case.d) and not ops.softmax_shared_hits_supported(case.S, inter, 132)
    with pytest.raises(ValueError, match="covers"):
        ops.softmax_shared_hits_step(dev(np.zeros((31, 132), np.float32)), dev(np.zeros((case.n_items, 132), np.float32)), None, None,
                                     inter, dev(case.row), 1.0)
    with pytest.raises(ValueError, match="temperature"):
        ops.softmax_shared_hits_step(dev(case.U), dev(case.V), None, None, inter, dev(case.row), 0.0)
    with pytest.raises(ValueError, match="vector"):
        ops.softmax_shared_hits_step(dev(case.U), dev(case.V), None, None, inter, dev(case.samples), 1.0)


# ------------------------------------------------------------------------------------------------ the model
N_USERS, N_ITEMS, S_MODEL, D_MODEL = 129, 200, 65, 36
MODEL_CONFIGS = {"dot-bias-device": ("dot", True, "device"), "dot-nobias-device": ("dot", False, "device"),
                 "cosine-bias-device": ("cosine", True, "device"), "dot-bias-popularity": ("dot", True, "popularity"),
                 "dot-nobias-popularity": ("dot", False, "popularity"), "cosine-bias-popularity": ("cosine", True, "popularity")}


def model_data():
    rng = np.random.default_rng(23)
    dense = (rng.random((N_USERS, N_ITEMS)) < 0.06).astype(np.float32)
    dense *= np.where(rng.random(dense.shape) < 0.85, 1.0, -1.0).astype(np.float32)
    dense[4, :] = 0                                   # a user without interactions
    dense[9, :] = -np.abs(dense[9, :])                # a user with negative interactions only
    dense[9, 3] = -1.0
    dense[:, 17] = np.where(dense[:, 17] == 0, 1.0, dense[:, 17])     # a popular item: PopularitySampler draws it, many users hit
    dense[4, :] = 0
    inter = sp.csr_matrix(dense)
    uf = sp.identity(N_USERS, dtype=np.float32, format="csr")
    itf = sp.identity(N_ITEMS, dtype=np.float32, format="csr")
    return inter, uf, itf


class Recording(object):
    """a sampler that keeps what the wrapped sampler drew"""

    def __init__(self, inner):
        self.inner, self.rows = inner, []
        if hasattr(inner, "log_q"):
            self.log_q = inner.log_q

    def sample(self, n_items, n_users, n_sampled_items, replace, step, device, user_base=0):
        t = self.inner.sample(n_items, n_users, n_sampled_items, replace, step, device, user_base)
        self.rows.append(t.cpu().numpy().copy())
        return t


def make_model(T, kind, biased, which, inter, d=D_MODEL, temperature=0.5, hits=True):
    from tensorrec_amd.loss_graphs import SampledSoftmaxLossGraph
    from tensorrec_amd.prediction_graphs import DotProductPredictionGraph, CosineSimilarityPredictionGraph
    inner = T.DeviceSampler(seed=11) if which == "device" else T.PopularitySampler(inter, power=0.75, smoothing=1.0, seed=5)
    graph = SampledSoftmaxLossGraph(temperature, remove_accidental_hits=hits, shared_negatives=True,
                                    log_q_correction=which == "popularity")
    pred = {"dot": DotProductPredictionGraph, "cosine": CosineSimilarityPredictionGraph}[kind]()
    return T.TensorRec(n_components=d, prediction_graph=pred, loss_graph=graph, biased=biased, seed=3, sampler=Recording(inner))


def float64_model_step(N, w, inter, row, log_q, kind, biased, temperature):
    """(output, float64 value, bar) of one step from the weights: softmax_shared_hits_reference.ref_step on the tables the step is
    handed -- the weights themselves (identity features) or, for cosine, their float32 normalised rows, whose backward is through_norm"""
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
                           samples=samples, items=samples, row=row.reshape(-1), log_q=log_q, S=S_MODEL, d=D_MODEL, n_users=N_USERS,
                           n_items=N_ITEMS, exact=False)
    ref = H.ref_step(case, biased, temperature, "plain" if log_q is None else "logq")
    dU, bU, dV, bV = ref.dU, ref.b_dU, ref.dV, ref.b_dV
    if norms is not None:
        dU, bU = through_norm(U, norms[0], dU, bU)
        dV, bV = through_norm(V, norms[1], dV, bV)
    wants = [("pred_serial", ref.pred_serial, ref.b_pred_serial), ("loss", ref.loss, ref.b_loss),
             ("d linear_weights_user_0", dU, bU), ("d linear_weights_item", dV, bV)]
    if biased:
        wants += [("d user_feature_biases", ref.d_ub, ref.b_d_ub), ("d item_feature_biases", ref.d_ib, ref.b_d_ib)]
    return wants, ref.hits


def one_step(T, N, kind, biased, which, masked_route):
    inter, uf, itf = model_data()
    model = make_model(T, kind, biased, which, inter)
    model.build(N_USERS, N_ITEMS)
    w = model.get_weights()
    if biased:
        r2 = np.random.default_rng(7)
        w["user_feature_biases"] = (0.1 * r2.standard_normal(w["user_feature_biases"].shape)).astype(np.float32)
        w["item_feature_biases"] = (0.1 * r2.standard_normal(w["item_feature_biases"].shape)).astype(np.float32)
        model.set_weights(w)
    w = {k: v.copy() for k, v in model.get_weights().items()}
    model._capture = {}
    with tunings(N, softmax_shared_hits=1 if masked_route else 0):
        model.fit_partial(inter, uf, itf, epochs=1, learning_rate=0.05, alpha=1e-4, n_sampled_items=S_MODEL)
    return model, w, inter


@pytest.mark.parametrize("config", sorted(MODEL_CONFIGS))
def test_one_fit_step_against_float64(ops, N, config):
    """the masked MFMA route inside a fit (tuning softmax_shared_hits = 1) and the expanded generic step (tuning off) beside it, on
    the same drawn row: each within the bars of the float64 step -- and so within twice the bars of each other"""
    import tensorrec_amd as T
    kind, biased, which = MODEL_CONFIGS[config]
    rows, caps = [], []
    for masked_route in (True, False):
        model, w, inter = one_step(T, N, kind, biased, which, masked_route)
        assert model.last_step_form == "eager" and model.last_step_kernel == ("softmax_shared_hits" if masked_route else None)
        assert len(model.sampler.rows) == 1 and model.sampler.rows[0].shape == (1, S_MODEL)
        row = model.sampler.rows[0]
        log_q = model.sampler.log_q(torch.device("cuda")).cpu().numpy() if which == "popularity" else None
        wants, hits = float64_model_step(N, w, inter, row, log_q, kind, biased, 0.5)
        assert hits.any() and not hits.all()
        key = "model %s %s" % (config, "masked" if masked_route else "generic")
        cap = model._capture
        for name, want, bar in wants:
            got = cap[name] if name in cap else cap["grads"][name[2:]]
            held(key, name, np.asarray(got).reshape(-1), want, bar, "")
        rows.append(row)
        caps.append((cap, wants))
    assert np.array_equal(rows[0], rows[1])
    for name, _, bar in caps[0][1]:
        a, b = [np.asarray(c[name] if name in c else c["grads"][name[2:]], np.float64).reshape(-1) for c in (caps[0][0], caps[1][0])]
        assert (np.abs(a - b) <= 2.0 * f64(bar).reshape(-1)).all(), name


def test_which_kernel_a_fit_reports(ops, N, hits_on):
    import tensorrec_amd as T
    inter, uf, itf = model_data()
    fit = lambda m, **kw: m.fit(inter, uf, itf, epochs=3, n_sampled_items=S_MODEL, **kw)
    for kind in ("dot", "cosine"):
        m = make_model(T, kind, True, "popularity", inter)
        assert m.last_step_kernel is None
        fit(m)
        assert m.last_step_kernel == "softmax_shared_hits" and m.last_step_form == "eager"
    m = make_model(T, "dot", True, "device", inter, hits=False)                 # hits kept: the unmasked route, as ever
    fit(m)
    assert m.last_step_kernel == "softmax_shared" and m.last_step_form == "eager"
    m = make_model(T, "dot", True, "device", inter, d=6)                        # an uncovered width: the generic step
    fit(m)
    assert m.last_step_kernel is None and m.last_step_form == "eager"
    with tunings(N, softmax_shared=0):                                           # the MFMA route as such switched off
        m = make_model(T, "dot", True, "device", inter)
        fit(m)
        assert m.last_step_kernel is None
    with tunings(N, softmax_shared_hits=0):
        m = make_model(T, "dot", True, "device", inter)
        fit(m)
        assert m.last_step_kernel is None and m.last_step_form == "eager"


def test_the_tuning_is_off_by_default(ops, N):
    import tensorrec_amd as T
    assert ops.SOFTMAX_SHARED_HITS_DEFAULT == 0 and not ops.step_switch("softmax_shared_hits")
    inter, uf, itf = model_data()
    m = make_model(T, "dot", True, "device", inter)
    m.fit(inter, uf, itf, epochs=2, n_sampled_items=S_MODEL)
    assert m.last_step_kernel is None and m.last_step_form == "eager"


def test_twenty_steps_lower_the_loss(ops, N, hits_on):
    import tensorrec_amd as T
    inter, uf, itf = T.util.generate_dummy_data(num_users=60, num_items=90, interaction_density=.08, num_user_features=40,
                                                num_item_features=50, n_features_per_user=6, n_features_per_item=7, random_state=3)
    inter, uf, itf = sp.csr_matrix(inter), sp.csr_matrix(uf), sp.csr_matrix(itf)
    model = make_model(T, "dot", True, "popularity", inter, d=16)
    sums = []
    for _ in range(20):
        model._capture = {}
        model.fit_partial(inter, uf, itf, epochs=1, learning_rate=0.05, n_sampled_items=40)
        assert model.last_step_kernel == "softmax_shared_hits"
        sums.append(float(np.asarray(model._capture["loss"]).sum()))
    model._capture = None
    assert np.isfinite(sums).all() and sums[-1] < sums[0], sums
