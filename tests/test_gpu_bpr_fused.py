"""The one-pass BPR step (csrc/bpr_fused.hip, trec_bpr_fused_step, ops.bpr_fused_step) against the float64 step of
tests/bpr_step_reference.py, per element and per output, within the bars derived there (tests/test_bpr_step_reference_host.py
shows on the CPU that a float32 restatement lies inside them and seeded defects outside), against the unfused BPR kernels bit for
bit where a sum has one term, and the opt-in route inside a TensorRec fit.

* kernel   every instantiation <ITERS, RMAX, SURE> x {plain, hits removed} and every edge of the loss phase (bpr_step_reference.SPECS)
           at the smallest shapes that reach them, with and without biases, real-valued tables and dyadic ones (exact scores:
           pred_serial bit for bit); the planted rows of softmax_step_reference.softmax_case; exact zeros; repeats bit for bit; the
           histogram and ranks; the coverage answer;
* model    which kernel a fit reports with the tuning on and off, one captured step against the float64 composition, HIP-graph
           replay against eager steps bit for bit, one step with a HardNegativeSampler.

Every test runs with tuning bpr_fused = 1, set by a fixture that clears it again in a ``finally``: the route is opt-in and the files
that pin the generic route for a BPR fit see the default whatever the order.  The largest error / bar per output is kept in RATIOS;
with TREC_BPR_FUSED_RATIOS_OUT=<file> it is written there at the end (profiles/bpr_fused_reference_ratios.json)."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import bpr_step_reference as R
from pair_reference import f64
from test_gpu_pair_kernels import check, dev, tunings

pytestmark = pytest.mark.gpu

RATIOS = {}
TREC_ERR_UNSUPPORTED = 3                                          # include/tensorrec_hip.h
IDS = lambda s: "S%d-L%d-d%d" % s
USER_SIDE = ("loss", "pred_serial", "coef_pairs", "coef_samples", "dU", "d_ub")


@pytest.fixture(scope="module")
def ops():
    from tensorrec_amd import ops as _ops, _native
    _native.require_gpu()
    _native.load()
    yield _ops
    out = os.environ.get("TREC_BPR_FUSED_RATIOS_OUT")
    if out:
        write_ratios(out)


@pytest.fixture(scope="module")
def N(ops):
    from tensorrec_amd import _native
    return _native


@pytest.fixture(autouse=True)
def bpr_fused_on(N):
    N.set_tuning("bpr_fused", 1)
    try:
        yield
    finally:
        N.clear_tuning("bpr_fused")


def write_ratios(path):
    """profiles/bpr_fused_reference_ratios.json: the ratios of this run"""
    rec = {"what": "largest |result - float64 reference| / bar per kernel variant (or model configuration) and output over the cases of "
                   "tests/test_gpu_bpr_fused.py (bars: tests/bpr_step_reference.py); a bar of 0 asks for equality and records 0",
           "command": "TREC_BPR_FUSED_RATIOS_OUT=<this file> python -m pytest -m gpu tests/test_gpu_bpr_fused.py",
           "ratios": {k: {n: float("%.4g" % v) for n, v in sorted(r.items())} for k, r in sorted(RATIOS.items())}}
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
        print("%s %s %s: largest error / bar %.4g" % (key, what, name, r))
    check(got, want, bar, "%s %s: %s" % (key, what, name))


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def interactions_of(case):
    from tensorrec_amd.sparse import Interactions
    inter = Interactions(case.matrix, case.n_users, case.n_items, "cuda")
    assert np.array_equal(inter.indptr.cpu().numpy(), case.indptr) and np.array_equal(inter.values.cpu().numpy(), case.values)
    assert np.array_equal(inter.x_item32.cpu().numpy(), case.x_item) and inter.max_row_nnz == case.max_pos
    return inter


def abi_buffers(case, inter, biased, buffers=True):
    nu, ni, S, d = case.n_users, case.n_items, case.S, case.d
    return dict(U=dev(case.U), V=dev(case.V), ub=dev(case.ub) if biased else None, ib=dev(case.ib) if biased else None,
                samples=dev(case.samples), loss=nan(inter.n_positive), pred_serial=nan(inter.nnz), dU=nan(nu, d),
                d_ub=nan(nu) if biased else None, coef_samples=nan(nu, S), coef_pairs=nan(inter.nnz),
                hist=torch.zeros(ni, dtype=torch.int32, device="cuda") if buffers else None,
                ranks=torch.full((nu, S), -1, dtype=torch.int32, device="cuda") if buffers else None)


def abi_call(N, case, inter, t, hits, S=None, max_pos=None, d=None):
    """the return code of trec_bpr_fused_step on the buffers ``t`` (shape arguments replaceable: the uncovered shapes)"""
    p = lambda k: N.ptr(t[k])
    code = N.load().trec_bpr_fused_step(
        p("U"), p("V"), p("ub"), p("ib"), N.ptr(inter.indptr), N.ptr(inter.x_item32), N.ptr(inter.pos_slot), p("samples"), case.n_users,
        case.n_items, case.S if S is None else S, case.d if d is None else d, int(inter.max_row_nnz) if max_pos is None else max_pos,
        1 if hits else 0, p("loss"), p("pred_serial"), p("dU"), p("d_ub"), p("coef_samples"), p("coef_pairs"), p("hist"), p("ranks"),
        N.stream())
    torch.cuda.synchronize()
    return code


def run_abi(N, case, inter, biased, hits, buffers=True):
    t = abi_buffers(case, inter, biased, buffers)
    assert abi_call(N, case, inter, t, hits) == 0, N.load().trec_last_error()
    return SimpleNamespace(**{k: (v.cpu().numpy() if v is not None else None) for k, v in t.items()})


def run_step(ops, case, inter, biased, hits):
    out = ops.bpr_fused_step(dev(case.U), dev(case.V), dev(case.ub) if biased else None, dev(case.ib) if biased else None, inter,
                             dev(case.samples), remove_accidental_hits=hits)
    torch.cuda.synchronize()
    names = ("loss", "pred_serial", "dU", "dV", "d_ub", "d_ib")
    return SimpleNamespace(**{k: (v.cpu().numpy() if v is not None else None) for k, v in zip(names, out)})


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("biased", [True, False], ids=["biased", "unbiased"])
@pytest.mark.parametrize("hits", [False, True], ids=["plain", "hits"])
@pytest.mark.parametrize("exact", [False, True], ids=["real", "dyadic"])
@pytest.mark.parametrize("spec", R.SPECS, ids=IDS)
def test_fused_step_against_float64(ops, N, spec, exact, hits, biased):
    """pred_serial, loss, coef_pairs, coef_samples, dU, d b_u from the entry point and dV, d b_i (and the others again) from
    ops.bpr_fused_step, per element against the float64 step; every entry the reference says is 0 is an exact 0; on the dyadic
    family pred_serial is bit-exact, and with S = 1 loss and coef_pairs equal the unfused kernels' (ops.bpr_loss on the same scores,
    upstream gradient 1) bit for bit: sums of one term through the shared cell function"""
    case = R.cached_case(spec, exact)
    inst = R.instantiation(case.S, case.max_pos, case.d)
    assert inst is not None and N.query("trec_bpr_fused_lds_bytes", case.S, case.max_pos, case.d) == R.lds_bytes(case.S, case.max_pos, case.d)
    inter = interactions_of(case)
    assert ops.bpr_fused_supported(case.S, inter, case.d)
    ref = R.cached_ref(spec, exact, biased, hits)
    abi = run_abi(N, case, inter, biased, hits)
    got = run_step(ops, case, inter, biased, hits)
    assert ops.LAST_FUSED_STATS["route"] == "ranked"
    key = "fused %s" % ("hits" if hits else "plain")
    what = "%s <%d,%d,%d> %s bias %d" % ((spec,) + inst + ("dyadic" if exact else "real", biased))
    assert (got.d_ub is None) == (not biased) and (got.d_ib is None) == (not biased)
    pos = case.values > 0
    for name in R.OUTPUTS:
        src = got if name in ("dV", "d_ib") else abi
        if getattr(src, name) is not None:
            held(key, name, getattr(src, name), getattr(ref, name), getattr(ref, "b_" + name), what)
    for name in ("loss", "pred_serial", "dU", "d_ub"):            # the same kernel through ops: the same bits
        if getattr(got, name) is not None:
            assert np.array_equal(getattr(got, name), getattr(abi, name)), name
    # every entry the reference says is 0 is an exact 0 (the sums dU, dV, d b_u, d b_i: wherever all their terms are 0, which is
    # where their bar is 0 -- held() asked for equality there)
    for name in ("loss", "coef_pairs", "coef_samples"):
        assert not getattr(abi, name)[getattr(ref, name) == 0].any(), "%s: the zero pattern of %s" % (what, name)
    zero_rows = ~ref.b_dV.any(1) & ~ref.dV.any(1)
    assert not got.dV[zero_rows].any()                            # (sigma > 0: only untouched items, and items only hits touch)
    assert not abi.coef_pairs[~pos].any()
    no_pos = [R.U_NONE, R.U_NONPOS]
    assert not abi.dU[no_pos].any() and not abi.coef_samples[no_pos].any() and (not biased or not abi.d_ub[no_pos].any())
    if hits:
        assert ref.hits[R.U_ALLHITS].all() and not abi.coef_samples[ref.hits].any() and not abi.dU[R.U_ALLHITS].any()
        assert not abi.loss[np.cumsum(pos)[case.indptr[R.U_ALLHITS]:case.indptr[R.U_ALLHITS + 1]] - 1].any()
    if exact:
        assert np.array_equal(abi.pred_serial, ref.pred_serial.astype(np.float32))
    if exact and case.S == 1:
        nnz = case.x_item.size
        samp = ref.scores.scores[nnz:].reshape(case.n_users, case.S)
        assert np.array_equal(samp.astype(np.float32).astype(np.float64), samp)
        pt, st = dev(abi.pred_serial).requires_grad_(), dev(samp.astype(np.float32)).requires_grad_()
        out = ops.bpr_loss(pt, st, inter, sample_items=dev(case.samples) if hits else None, remove_accidental_hits=hits)
        out.backward(torch.ones_like(out))
        torch.cuda.synchronize()
        for name, a in (("loss", out.detach()), ("coef_pairs", pt.grad)):
            assert np.array_equal(getattr(abi, name), a.cpu().numpy()), "%s: %s differs from the unfused kernels" % (what, name)


@pytest.mark.parametrize("hits", [False, True], ids=["plain", "hits"])
@pytest.mark.parametrize("spec", [(7, 20, 36), (100, 28, 128), (128, 128, 64), (255, 1, 36), (64, 64, 256), (192, 20, 64)], ids=IDS)
def test_histogram_ranks_and_repeats(ops, N, spec, hits):
    """with sample_hist / sample_rank: the histogram is bincount(samples), the ranks of every item a permutation of 0 .. count - 1 (users
    without interactions included); without the buffers the same bits in every other output; a second call the same bits in every
    output (the ranks are atomic arrival orders and excepted); ops.bpr_fused_step twice under the deterministic grouping likewise"""
    case = R.cached_case(spec, False)
    inter = interactions_of(case)
    a, b, c = run_abi(N, case, inter, True, hits), run_abi(N, case, inter, True, hits), run_abi(N, case, inter, True, hits, buffers=False)
    ni = case.n_items
    flat = case.samples.reshape(-1)
    want = np.concatenate([np.arange(k) for k in np.bincount(flat, minlength=ni)])
    for r in (a, b):
        assert np.array_equal(r.hist, np.bincount(flat, minlength=ni))
        rk = r.ranks.reshape(-1)
        assert np.array_equal(rk[np.lexsort((rk, flat))], want), "the ranks of an item are no permutation of 0 .. count - 1"
    for name in USER_SIDE:
        assert np.array_equal(getattr(a, name), getattr(b, name)), "two calls differ in %s" % name
        assert np.array_equal(getattr(a, name), getattr(c, name)), "with and without the histogram buffers: %s differs" % name
    with ops.deterministic_grouping(True):
        x, y = run_step(ops, case, inter, True, hits), run_step(ops, case, inter, True, hits)
    for name in ("loss", "pred_serial", "dU", "dV", "d_ub", "d_ib"):
        assert np.array_equal(getattr(x, name), getattr(y, name)), "two deterministic calls differ in %s" % name
    assert np.array_equal(x.dU, a.dU) and np.array_equal(x.loss, a.loss)


def test_uncovered_shapes_launch_nothing(ops, N):
    """the uncovered shapes answer -1 / False; the entry point returns TREC_ERR_UNSUPPORTED before any launch (the outputs keep their
    fill); with the tuning off or cleared ops.bpr_fused_supported says no to a covered shape too"""
    lib = N.load()
    for S, L, d in R.UNCOVERED:
        assert N.query("trec_bpr_fused_lds_bytes", S, L, d) == -1
        assert not ops.bpr_fused_supported(S, SimpleNamespace(max_row_nnz=L), d)
    assert ops.bpr_fused_supported(3, SimpleNamespace(max_row_nnz=125), 132)
    with tunings(N, bpr_fused=0):
        assert not ops.bpr_fused_supported(3, SimpleNamespace(max_row_nnz=125), 132)
    N.clear_tuning("bpr_fused")
    assert not ops.bpr_fused_supported(3, SimpleNamespace(max_row_nnz=125), 132)        # the default is off
    N.set_tuning("bpr_fused", 1)
    case = R.cached_case((7, 20, 36), False)
    inter = interactions_of(case)
    for S, L, d in R.UNCOVERED:
        t = abi_buffers(case, inter, True)
        assert abi_call(N, case, inter, t, True, S=S, max_pos=L, d=d) == TREC_ERR_UNSUPPORTED and b"not covered" in lib.trec_last_error()
        for k in ("loss", "pred_serial", "dU", "d_ub", "coef_samples", "coef_pairs"):
            assert bool(torch.isnan(t[k]).all()), k
        assert not bool(t["hist"].any()) and bool((t["ranks"] == -1).all())


# ------------------------------------------------------------------------------------------------ model level
N_USERS, N_ITEMS, S_MODEL = 37, 53, 7


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


def make_model(T, kind, biased, d, table=None, loss=None, **kw):
    from tensorrec_amd.loss_graphs import BPRLossGraph
    from tensorrec_amd.prediction_graphs import (DotProductPredictionGraph, CosineSimilarityPredictionGraph,
                                                 EuclideanSimilarityPredictionGraph)
    pred = {"dot": DotProductPredictionGraph, "cosine": CosineSimilarityPredictionGraph, "euclid": EuclideanSimilarityPredictionGraph}[kind]()
    if table is not None:
        kw["sampler"] = T.ReplaySampler([table])
    return T.TensorRec(n_components=d, prediction_graph=pred, loss_graph=loss or BPRLossGraph(), biased=biased, seed=3, **kw)


def test_which_kernel_a_fit_reports(ops, N):
    import tensorrec_amd as T
    inter, uf, itf, table = model_data()

    def kernel_of(kind, biased, loss=None, data=inter, **kw):
        m = make_model(T, kind, biased, 8, table, loss=loss, **kw)
        assert m.last_step_kernel is None
        m.fit_partial(data, uf, itf, epochs=1, n_sampled_items=S_MODEL)
        assert m.last_step_form == "eager"
        return m.last_step_kernel

    class Mine(T.loss_graphs.BPRLossGraph):                        # a subclass may override anything: the generic step
        pass
    assert kernel_of("dot", True) == "bpr_fused" and kernel_of("dot", False) == "bpr_fused"
    assert kernel_of("cosine", True) == "bpr_fused" and kernel_of("cosine", False) == "bpr_fused"
    assert kernel_of("dot", True, T.loss_graphs.BPRLossGraph(remove_accidental_hits=True)) == "bpr_fused"
    assert kernel_of("euclid", False) is None and kernel_of("dot", True, Mine()) is None
    assert kernel_of("dot", True, n_tastes=2) is None
    # an uncovered row length: one user interacts with every item of a catalogue of 300 (S + 300 > 256)
    wide = sp.csr_matrix(np.vstack([np.ones((1, 300), np.float32), np.eye(N_USERS - 1, 300, dtype=np.float32)]))
    m = make_model(T, "dot", True, 8)
    m.fit_partial(wide, uf, sp.identity(300, dtype=np.float32, format="csr"), epochs=1, n_sampled_items=S_MODEL)
    assert m.last_step_kernel is None
    with tunings(N, bpr_fused=0):
        assert kernel_of("dot", True) is None
    N.clear_tuning("bpr_fused")                                    # the default: off
    try:
        assert kernel_of("dot", True) is None and kernel_of("cosine", True) is None
    finally:
        N.set_tuning("bpr_fused", 1)


@pytest.mark.parametrize("hits", [False, True], ids=["plain", "hits"])
def test_one_fit_step_against_float64(ops, N, hits):
    """One fit_partial step of a small model (37 users x 53 items, identity features, so the representations ARE the weight tables;
    S = 7 replayed samples; dot scores with biases) on the fused route, every captured output against bpr_step_reference.ref_step on
    the weights -- the float64 composition and its bars"""
    import tensorrec_amd as T
    biased, d = True, 8
    inter, uf, itf, table = model_data()
    model = make_model(T, "dot", biased, d, table, loss=T.loss_graphs.BPRLossGraph(remove_accidental_hits=hits))
    model.build(N_USERS, N_ITEMS)
    w = model.get_weights()
    r2 = np.random.default_rng(7)
    for k in w:                                                   # scores of order 1: softplus and sigma away from their flat ends
        scale = 0.1 if k.endswith("biases") else 0.6
        w[k] = (scale * r2.standard_normal(w[k].shape)).astype(np.float32)
    model.set_weights(w)
    w = {k: v.copy() for k, v in model.get_weights().items()}
    model._capture = {}
    model.fit_partial(inter, uf, itf, epochs=1, learning_rate=0.05, alpha=1e-4, n_sampled_items=S_MODEL)
    cap = model._capture
    assert model.last_step_form == "eager" and model.last_step_kernel == "bpr_fused"
    m = sp.csr_matrix(inter)
    case = SimpleNamespace(U=w["linear_weights_user_0"], V=w["linear_weights_item"], ub=w["user_feature_biases"].reshape(-1),
                           ib=w["item_feature_biases"].reshape(-1), indptr=m.indptr.astype(np.int64), x_item=m.indices.astype(np.int32),
                           values=m.data.astype(np.float32), samples=table, S=S_MODEL, d=d, n_users=N_USERS, n_items=N_ITEMS, exact=False)
    ref = R.ref_step(case, biased, hits)
    assert ref.hits.any() == hits
    wants = [("pred_serial", ref.pred_serial, ref.b_pred_serial), ("loss", ref.loss, ref.b_loss),
             ("d linear_weights_user_0", ref.dU, ref.b_dU), ("d linear_weights_item", ref.dV, ref.b_dV),
             ("d user_feature_biases", ref.d_ub, ref.b_d_ub), ("d item_feature_biases", ref.d_ib, ref.b_d_ib)]
    for name, want, bar in wants:
        got = cap[name] if name in cap else cap["grads"][name[2:]]
        held("model dot-biased-8 %s" % ("hits" if hits else "plain"), name, np.asarray(got).reshape(-1), want, bar, "bpr fused")
    assert np.abs(ref.dU).max() > 1e-3 and not ref.dU[4].any() and not cap["grads"]["linear_weights_user_0"][[4, 9]].any()


def disjoint_data(n_users=24, n_pos=3, S=6):
    """every item is the column of at most one pair of a step -- user u's positives are items 9 u .. 9 u + 2, its replayed samples the six
    behind them -- so no sum of the step has more than one term whose order the counting-sort buckets could change (they order a bucket
    by atomic arrival): graph replays and eager steps can be compared bit for bit.  User 5 has no interaction, user 7 a negative one."""
    per = n_pos + S
    rows, cols, vals = [], [], []
    for u in range(n_users):
        if u == 5:
            continue
        for j in range(n_pos):
            rows.append(u)
            cols.append(per * u + j)
            vals.append(-1.0 if (u == 7 and j == 1) else 1.0)
    n_items = per * n_users
    inter = sp.csr_matrix((np.array(vals, np.float32), (rows, cols)), shape=(n_users, n_items))
    table = np.stack([per * u + n_pos + np.arange(S) for u in range(n_users)]).astype(np.int32)
    return inter, sp.identity(n_users, dtype=np.float32, format="csr"), sp.identity(n_items, dtype=np.float32, format="csr"), table


def test_hip_graph_replay_equals_eager_steps_bit_for_bit(ops):
    """a 6-epoch fit whose later steps are HIP-graph replays reports last_step_form "graph", takes bpr_fused and ends with the weights
    of the all-eager fit, bit for bit (disjoint_data: no sum of the step depends on the order inside an item's bucket)"""
    import tensorrec_amd as T
    inter, uf, itf, table = disjoint_data()
    out = []
    for graphs in (True, False):
        model = make_model(T, "dot", True, 8, table, hip_graphs=graphs)
        model.fit(inter, uf, itf, epochs=6, learning_rate=0.05, n_sampled_items=table.shape[1])
        assert model.last_step_form == ("graph" if graphs else "eager") and model.last_step_kernel == "bpr_fused"
        out.append((model.get_weights(), model._opt_step, model._sample_step))
    (wa, oa, sa), (wb, ob, sb) = out
    assert (oa, sa) == (ob, sb) == (6, 6)
    for k in wa:
        assert np.array_equal(wa[k], wb[k]), k
    assert any(np.abs(wa[k]).max() > 0 for k in wa)


def test_one_step_with_hard_negatives_stays_eager(ops):
    """a HardNegativeSampler reads the step's representations: the step takes bpr_fused and stays eager, also where a graph would
    engage for any other sampler"""
    import tensorrec_amd as T
    inter, uf, itf, _ = model_data()
    model = make_model(T, "dot", True, 8, sampler=T.HardNegativeSampler(12, n_hard=3, seed=4))
    for _ in range(2):
        model.fit_partial(inter, uf, itf, epochs=3, n_sampled_items=S_MODEL)
        assert model.last_step_kernel == "bpr_fused" and model.last_step_form == "eager"
