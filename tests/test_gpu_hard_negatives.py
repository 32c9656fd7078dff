"""The hard-negative selection on the GPU (csrc/sampler_hard.hip, trec_select_hard_negatives, ops.select_hard_negatives,
tensorrec.HardNegativeSampler) against the float64 definition of tests/hard_negative_reference.py.

* kernel   EXACT equality of the table (and of the scores, wherever asked for) on dyadic inputs, where every float32 summation order is
           exact: M in {1, 63, 64, 65, 256, 257, 1023, 1024, 1025, 4096} x S in {1, M/2, M} x H in {1, S/2, S}, d in {4, 64, 128, 132,
           256}, with and without bias, exclude on and off; interaction rows of 0, 1, 64, 65, 300, 512 and 513 entries (the last two
           sit on either side of the length up to which the kernel searches the row in LDS), some with pos_slot < 0, hits planted
           among the candidates, a user all of whose candidates are hits, duplicate candidates, an all-equal-score row, a NaN and a
           -inf score, n_users = 0.  Generic Gaussian inputs (d = 128, M = 512, S = 100) within the bar derived in the reference
           module.  Two calls give equal bits.  Every error code.
* model    one fit_partial step with a HardNegativeSampler over replayed candidates for WMRB, BPR, sampled softmax and WARP on dot
           scores, a cosine model, and the one-pass routes: the table the sampler returned is the reference selection from the
           pre-step representations, the step is eager, takes the kernel a model B stepped with ReplaySampler([that table]) takes, and
           leaves B's weights (the models are deterministic=True fits, whose steps repeat to the bit on the routes without float
           atomics; bit-equal where two runs of B are bit-equal, else within four times their largest difference -- kept
           in RATIOS and, with TREC_HARD_NEGATIVES_RATIOS_OUT=<file>, written there: profiles/hard_negatives_reference_ratios.json);
           every ValueError of the wiring by a two-user model; save_model / load_model."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import hard_negative_reference as R
from test_gpu_pair_kernels import dev, tunings

pytestmark = pytest.mark.gpu

TREC_OK, TREC_ERR_INVALID, TREC_ERR_UNSUPPORTED = 0, 1, 3          # include/tensorrec_hip.h
RATIOS = {}
N_ITEMS = 700
ROW_LENGTHS = [0, 1, 64, 65, 300, 512, 513, 40, 10]                # users 0..8; user 7: every candidate a hit; user 8: a zero row of U
ALL_HITS_USER, ZERO_USER = 7, 8
MS = [1, 63, 64, 65, 256, 257, 1023, 1024, 1025, 4096]
DS = [4, 64, 128, 132, 256]


@pytest.fixture(scope="module")
def ops():
    from tensorrec_amd import ops as _ops, _native
    _native.require_gpu()
    _native.load()
    yield _ops
    out = os.environ.get("TREC_HARD_NEGATIVES_RATIOS_OUT")
    if out:
        rec = {"what": "model level of tests/test_gpu_hard_negatives.py: largest |weight of model B - weight of a second run of model B| "
                       "after one step, per configuration (0: bit-equal, and the scored model is then held to bit-equality with B; "
                       "otherwise it is held to four times this figure), and the scored model's largest difference from B",
               "command": "TREC_HARD_NEGATIVES_RATIOS_OUT=<this file> python -m pytest -m gpu tests/test_gpu_hard_negatives.py",
               "figures": {k: {n: float("%.4g" % v) for n, v in sorted(r.items())} for k, r in sorted(RATIOS.items())}}
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


@pytest.fixture(scope="module")
def N(ops):
    from tensorrec_amd import _native
    return _native


# ------------------------------------------------------------------------------------------------ kernel level
_CASES = {}


def kernel_case(M, d, biased):
    """Dyadic tables, the interaction rows of ROW_LENGTHS and an [n_users, M] candidate table with planted hits and duplicates; the
    float64 scores and hits are computed ONCE per case and shared, unchanged, by every (S, H, exclude) of it"""
    key = (M, d, biased)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * M + 10 * d + biased)
        U, V, ib = R.dyadic_tables(rng, len(ROW_LENGTHS), N_ITEMS, d, biased)
        U[ZERO_USER] = 0                                           # every score of this user is the bias: all equal without one
        indptr, x_item, pos_slot = R.interaction_rows(rng, N_ITEMS, ROW_LENGTHS)
        C = R.candidates_with_planted_hits(rng, N_ITEMS, indptr, x_item, M)
        b, e = indptr[ALL_HITS_USER], indptr[ALL_HITS_USER + 1]
        C[ALL_HITS_USER] = rng.choice(x_item[b:e][pos_slot[b:e] >= 0], size=M)
        y = R.scores64(U, V, ib, C)
        hit = R.hits_of(indptr, x_item, pos_slot, C)
        assert hit[ALL_HITS_USER].all() and (M < 63 or hit[2:ALL_HITS_USER].any(axis=1).all())
        assert (pos_slot < 0).sum() > 50
        inter = SimpleNamespace(indptr=dev(indptr), x_item32=dev(x_item), pos_slot=dev(pos_slot), nnz=len(x_item))
        _CASES[key] = SimpleNamespace(U=U, V=V, ib=ib, C=C, y=y, hit=hit, inter=inter, dU=dev(U), dV=dev(V),
                                      dib=dev(ib) if biased else None, dC=dev(C))
    return _CASES[key]


def sizes(M):
    """(S, H): S in {1, M/2, M} x H in {1, S/2, S}, without repeats"""
    out = []
    for S in sorted({1, max(M // 2, 1), M}):
        for H in sorted({1, max(S // 2, 1), S}):
            out.append((S, H))
    return out


def run_exact(ops, case, S, H, exclude, scores):
    got = ops.select_hard_negatives(case.dU, case.dV, case.dib, case.inter, case.dC, S, H, exclude=exclude, return_scores=scores)
    table, y32 = got if scores else (got, None)
    hit = case.hit if exclude else np.zeros_like(case.hit)
    want, _ = R.select(case.y, hit, case.C, S, H)
    table = table.cpu().numpy()
    assert table.dtype == np.int32 and table.shape == want.shape
    bad = np.flatnonzero((table != want).any(axis=1))
    assert not len(bad), "M %d S %d H %d exclude %d: users %s differ; first: got %s, want %s" % (
        case.C.shape[1], S, H, exclude, bad.tolist(), table[bad[0]].tolist()[:12], want[bad[0]].tolist()[:12])
    if scores:
        assert np.array_equal(y32.cpu().numpy().astype(np.float64), case.y, equal_nan=True), "out_scores"


@pytest.mark.parametrize("M", MS)
def test_exact_on_dyadic_inputs(ops, M):
    """every (S, H) of an M, exclude on and off; d and the bias walk their lists with M (every d and both bias settings are also
    crossed at M = 65 below)"""
    at = MS.index(M)
    case = kernel_case(M, DS[at % len(DS)], at % 2 == 0)
    for n, (S, H) in enumerate(sizes(M)):
        run_exact(ops, case, S, H, exclude=True, scores=n % 2 == 0)
        if n % 2 == 1 or M <= 65:
            run_exact(ops, case, S, H, exclude=False, scores=n % 4 == 1)


@pytest.mark.parametrize("biased", [False, True], ids=["plain", "bias"])
@pytest.mark.parametrize("d", DS)
def test_exact_for_every_width(ops, d, biased):
    case = kernel_case(65, d, biased)
    if not biased:
        assert len(set(case.y[ZERO_USER])) == 1                    # the all-equal-score row
    for S, H, exclude in [(32, 16, True), (65, 65, True), (65, 1, False), (7, 7, False)]:
        run_exact(ops, case, S, H, exclude, scores=True)


def test_nan_and_minus_inf_scores(ops):
    """a NaN and a -inf score in one row: the NaN counts as -inf, so the two are ordered by position, after every finite score"""
    rng = np.random.default_rng(9)
    n_users, n_items, d, M = 3, 50, 64, 40
    U, V, _ = R.dyadic_tables(rng, n_users, n_items, d, False)
    U[0] = 1.0
    V[11], V[12] = 0.0, 0.0
    V[11, 5], V[12, 7] = np.nan, -np.inf
    C = np.stack([rng.permutation(n_items)[:M] for _ in range(n_users)]).astype(np.int32)
    C[0][np.isin(C[0], (11, 12))] = 13
    C[0, 30], C[0, 4] = 11, 12                                     # the -inf BEFORE the NaN by position
    y = R.scores64(U, V, None, C)
    assert np.isnan(y[0, 30]) and y[0, 4] == -np.inf and np.isfinite(np.delete(y[0], [4, 30])).all()
    hit = np.zeros(C.shape, bool)
    for S, H in [(M, M), (M, M - 1), (20, 10)]:
        want, pos = R.select(y, hit, C, S, H)
        table, y32 = ops.select_hard_negatives(dev(U), dev(V), None, None, dev(C), S, H, exclude=False, return_scores=True)
        assert np.array_equal(table.cpu().numpy(), want)
        assert np.array_equal(y32.cpu().numpy().astype(np.float64), y, equal_nan=True)
    assert R.select(y, hit, C, M, M)[1][0].tolist()[-2:] == [4, 30]


def test_no_users(ops, N):
    table = ops.select_hard_negatives(torch.zeros((0, 8), device="cuda"), torch.zeros((5, 8), device="cuda"), None, None,
                                      torch.zeros((0, 6), dtype=torch.int32, device="cuda"), 3, 2, exclude=False)
    assert tuple(table.shape) == (0, 3) and table.dtype == torch.int32
    case = kernel_case(63, 64, False)
    out = torch.full((9, 8), -7, dtype=torch.int32, device="cuda")
    assert abi(N, case, out, n_users=0) == TREC_OK and (out == -7).all()          # no launch: nothing written


GAUSS = dict(n_users=48, n_items=2000, d=128, M=512, S=100)


@pytest.fixture(scope="module")
def gaussian():
    rng = np.random.default_rng(77)
    g = SimpleNamespace(**GAUSS)
    g.U = rng.standard_normal((g.n_users, g.d)).astype(np.float32)
    g.V = rng.standard_normal((g.n_items, g.d)).astype(np.float32)
    g.ib = rng.standard_normal(g.n_items).astype(np.float32)
    g.indptr, g.x_item, g.pos_slot = R.interaction_rows(rng, g.n_items, [int(x) for x in rng.integers(0, 80, size=g.n_users)])
    g.C = R.candidates_with_planted_hits(rng, g.n_items, g.indptr, g.x_item, g.M, share=0.1)
    g.y, g.bar = R.scores64(g.U, g.V, g.ib, g.C), R.score_bar(g.U, g.V, g.ib, g.C)
    g.hit = R.hits_of(g.indptr, g.x_item, g.pos_slot, g.C)
    g.inter = SimpleNamespace(indptr=dev(g.indptr), x_item32=dev(g.x_item), pos_slot=dev(g.pos_slot), nnz=len(g.x_item))
    return g


@pytest.mark.parametrize("H", [100, 50, 1])
def test_gaussian_inputs_within_the_bar(ops, gaussian, H):
    g = gaussian
    table, y32 = ops.select_hard_negatives(dev(g.U), dev(g.V), dev(g.ib), g.inter, dev(g.C), g.S, H, return_scores=True)
    err = np.abs(y32.cpu().numpy().astype(np.float64) - g.y)
    print("largest score error / bar %.4g" % (err / g.bar).max())
    assert (err <= g.bar).all()
    worst = R.check_within_bar(table.cpu().numpy(), g.C, g.y, g.bar, g.hit, g.S, H)          # (no row is left out: it raises or counts)
    print("H %d: largest threshold excess / bar %.4g" % (H, worst))
    assert worst <= 1.0


def test_two_calls_give_equal_bits(ops, gaussian):
    g = gaussian
    args = (dev(g.U), dev(g.V), dev(g.ib), g.inter, dev(g.C), g.S, 50)
    a, ya = ops.select_hard_negatives(*args, return_scores=True)
    b, yb = ops.select_hard_negatives(*args, return_scores=True)
    assert torch.equal(a, b) and torch.equal(ya.view(torch.int32), yb.view(torch.int32))
    assert torch.equal(a, ops.select_hard_negatives(*args))                               # (and without the scores)


def abi(N, case, buf, **kw):
    """the return code of trec_select_hard_negatives on a kernel case, any argument replaceable"""
    a = dict(U=case.dU, V=case.dV, ib=case.dib, indptr=case.inter.indptr, x_item=case.inter.x_item32, pos_slot=case.inter.pos_slot,
             C=case.dC, n_users=case.C.shape[0], n_items=N_ITEMS, M=case.C.shape[1], S=8, H=4, d=case.U.shape[1], exclude=1, out=buf,
             scores=None)
    a.update(kw)
    code = N.load().trec_select_hard_negatives(
        N.ptr(a["U"]), N.ptr(a["V"]), N.ptr(a["ib"]), N.ptr(a["indptr"]), N.ptr(a["x_item"]), N.ptr(a["pos_slot"]), N.ptr(a["C"]),
        a["n_users"], a["n_items"], a["M"], a["S"], a["H"], a["d"], a["exclude"], N.ptr(a["out"]), N.ptr(a["scores"]), N.stream())
    torch.cuda.synchronize()
    return code


def test_error_codes(ops, N):
    case = kernel_case(63, 64, False)
    out = torch.full((9, 8), -7, dtype=torch.int32, device="cuda")
    assert abi(N, case, out) == TREC_OK and (out >= 0).all()
    out.fill_(-7)
    for name in ("U", "V", "C", "out"):
        assert abi(N, case, out, **{name: None}) == TREC_ERR_INVALID, name
    for name in ("indptr", "x_item", "pos_slot"):
        assert abi(N, case, out, **{name: None}) == TREC_ERR_INVALID, name
    invalid = [dict(n_items=0), dict(n_items=2 ** 31), dict(n_users=-1), dict(M=0), dict(S=0), dict(S=64), dict(H=0), dict(H=9),
               dict(d=0), dict(M=5000, S=5001)]
    for kw in invalid:
        assert abi(N, case, out, **kw) == TREC_ERR_INVALID, kw
        assert b"trec_select_hard_negatives" in N.load().trec_last_error()
    for kw in [dict(M=4097), dict(d=6), dict(d=260), dict(d=2)]:                          # (no launch: the sizes are never used)
        assert abi(N, case, out, **kw) == TREC_ERR_UNSUPPORTED, kw
        assert not ops.hard_negatives_supported(kw.get("M", 63), 8, kw.get("d", 64))
    assert (out == -7).all()                                                              # every refusal came before any launch
    assert abi(N, case, out, indptr=None, x_item=None, pos_slot=None, exclude=0) == TREC_OK and (out >= 0).all()
    assert N.load().trec_abi_version() == 1


# ------------------------------------------------------------------------------------------------ model level
N_USERS, N_MODEL_ITEMS, S_MODEL, M_MODEL, D_MODEL = 37, 53, 7, 28, 8


def model_data():
    rng = np.random.default_rng(17)
    dense = (rng.random((N_USERS, N_MODEL_ITEMS)) < 0.15).astype(np.float32)
    dense *= np.where(rng.random(dense.shape) < 0.85, 1.0, -1.0).astype(np.float32)
    dense[4, :] = 0                                   # a user without interactions
    inter = sp.csr_matrix(dense)
    uf = sp.identity(N_USERS, dtype=np.float32, format="csr")
    itf = sp.identity(N_MODEL_ITEMS, dtype=np.float32, format="csr")
    C = rng.integers(0, N_MODEL_ITEMS, size=(N_USERS, M_MODEL)).astype(np.int32)
    return inter, uf, itf, C


def dyadic_weights(model, seed=5):
    rng = np.random.default_rng(seed)
    w = model.get_weights()
    for k in w:
        scale = 64.0 if k.endswith("biases") else 8.0
        w[k] = (rng.integers(-16, 17, size=w[k].shape) / scale).astype(np.float32)
    return w


def make_model(kind, loss, sampler, biased=True, **kw):
    import tensorrec_amd as T
    from tensorrec_amd.prediction_graphs import (DotProductPredictionGraph, CosineSimilarityPredictionGraph,
                                                 EuclideanSimilarityPredictionGraph)
    pred = {"dot": DotProductPredictionGraph, "cosine": CosineSimilarityPredictionGraph, "euclid": EuclideanSimilarityPredictionGraph}[kind]()
    kw.setdefault("n_components", D_MODEL)
    # deterministic=True: the item-side sums are added in pair order, so two runs of one step are bit-equal wherever the route has no
    # float atomics -- without it two runs of model B agree to the bit only by chance, which says nothing about the scored model
    kw.setdefault("deterministic", True)
    return T.TensorRec(prediction_graph=pred, loss_graph=loss, biased=biased, seed=3, sampler=sampler, **kw)


def losses():
    from tensorrec_amd import loss_graphs as L
    return {"wmrb": L.WMRBLossGraph, "bpr": L.BPRLossGraph, "softmax": L.SampledSoftmaxLossGraph, "warp": L.WARPLossGraph,
            "warp_hits": lambda: L.WARPLossGraph(remove_accidental_hits=True)}


# (configuration, prediction graph, loss, tunings, the kernel the step is expected to name)
MODEL_CONFIGS = [
    ("wmrb", "dot", "wmrb", {}, "wmrb_fused"),
    ("wmrb_tiled", "dot", "wmrb", {"wmrb_fused": 0}, "wmrb_tiled"),
    ("wmrb_generic", "dot", "wmrb", {"wmrb_fused": 0, "wmrb_tiled": 0}, None),
    ("bpr", "dot", "bpr", {}, None),
    ("softmax", "dot", "softmax", {}, "softmax_fused"),
    ("softmax_generic", "dot", "softmax", {"softmax_fused": 0}, None),
    ("warp", "dot", "warp", {}, None),
    ("warp_fused", "dot", "warp_hits", {"warp_fused": 1}, "warp_fused"),
    ("cosine", "cosine", "wmrb", {}, "wmrb_fused"),
]


def one_step(kind, loss_name, sampler, weights, data):
    inter, uf, itf, _ = data
    model = make_model(kind, losses()[loss_name](), sampler)
    model.build(N_USERS, N_MODEL_ITEMS)
    model.set_weights(weights if weights is not None else dyadic_weights(model))
    before = model.get_weights()
    model.fit_partial(inter, uf, itf, epochs=1, learning_rate=0.05, alpha=1e-4, n_sampled_items=S_MODEL)
    return model, before, model.get_weights()


@pytest.mark.parametrize("n_hard", [None, 3], ids=["all_hard", "mixed"])
@pytest.mark.parametrize("config", MODEL_CONFIGS, ids=[c[0] for c in MODEL_CONFIGS])
def test_one_fit_step(ops, N, config, n_hard):
    import tensorrec_amd as T
    from tensorrec_amd.sparse import Interactions
    name, kind, loss_name, tuning, kernel = config
    data = model_data()
    C = data[3]
    with tunings(N, **tuning):
        sampler = T.HardNegativeSampler(M_MODEL, base=T.ReplaySampler([C]), n_hard=n_hard, keep_last=True)
        a, w0, wa = one_step(kind, loss_name, sampler, None, data)
        table = sampler.last_table.cpu().numpy()
        assert np.array_equal(sampler.last_candidates.cpu().numpy(), C) and table.shape == (N_USERS, S_MODEL)
        assert a.last_step_form == "eager" and a.last_step_kernel == kernel
        b, _, wb = one_step(kind, loss_name, T.ReplaySampler([table]), w0, data)
        b2, _, wb2 = one_step(kind, loss_name, T.ReplaySampler([table]), w0, data)
        assert b.last_step_form == "eager" and b.last_step_kernel == a.last_step_kernel == b2.last_step_kernel

    # the table is the reference selection from the pre-step representations (identity features: the weight tables)
    U, V, ib = w0["linear_weights_user_0"], w0["linear_weights_item"], w0["item_feature_biases"].reshape(-1)
    it = Interactions(data[0], N_USERS, N_MODEL_ITEMS, "cuda")
    indptr, x_item, pos_slot = it.indptr.cpu().numpy(), it.x_item32.cpu().numpy(), it.pos_slot.cpu().numpy()
    H = S_MODEL if n_hard is None else n_hard
    hit = R.hits_of(indptr, x_item, pos_slot, C)
    assert hit.any() and (pos_slot < 0).any()
    if kind == "cosine":            # the operands are the normalised rows as the step computes them: generic float32 inputs
        Un, Vn = ops.l2_normalize_rows(dev(U)).cpu().numpy(), ops.l2_normalize_rows(dev(V)).cpu().numpy()
        y, bar = R.scores64(Un, Vn, ib, C), R.score_bar(Un, Vn, ib, C)
        assert R.check_within_bar(table, C, y, bar, hit, S_MODEL, H) <= 1.0
    else:
        want, _ = R.select(R.scores64(U, V, ib, C), hit, C, S_MODEL, H)
        assert np.array_equal(table, want)

    # the step is model B's
    noise = max(float(np.abs(wb[k].astype(np.float64) - wb2[k]).max()) for k in wb)
    diff = max(float(np.abs(wa[k].astype(np.float64) - wb[k]).max()) for k in wb)
    moved = max(float(np.abs(wa[k].astype(np.float64) - w0[k]).max()) for k in wb)
    RATIOS["%s-%s" % (name, "all_hard" if n_hard is None else "mixed")] = {"b_against_b": noise, "scored_against_b": diff}
    print("%s: B against B %.4g, scored against B %.4g, the step moved %.4g" % (name, noise, diff, moved))
    assert moved > 1e-3
    if noise == 0.0:
        for k in wb:
            assert np.array_equal(wa[k], wb[k]), k
    else:
        assert diff <= 4.0 * noise


def two_user_model(kind="dot", loss=None, sampler=None, **kw):
    import tensorrec_amd as T
    from tensorrec_amd.loss_graphs import WMRBLossGraph
    sampler = sampler or T.HardNegativeSampler(6)
    model = make_model(kind, loss or WMRBLossGraph(), sampler, **kw)
    inter = sp.csr_matrix(np.array([[1, 0, 0, 1, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0, 1, 0]], np.float32))
    feats = (sp.identity(2, dtype=np.float32, format="csr"), sp.identity(8, dtype=np.float32, format="csr"))
    return model, (inter,) + feats


def test_wiring_value_errors(ops, N, monkeypatch):
    import tensorrec_amd as T
    from tensorrec_amd import loss_graphs as L
    from tensorrec_amd.prediction_graphs import AbstractPredictionGraph
    from tensorrec_amd.representation_graphs import LinearRepresentationGraph

    def refused(match, S=3, **kw):
        model, data = two_user_model(**kw)
        with pytest.raises(ValueError, match=match):
            model.fit_partial(*data, epochs=1, n_sampled_items=S)
        return model

    model, data = two_user_model()                                  # the covered two-user model steps
    model.fit_partial(*data, epochs=3, n_sampled_items=3)
    assert model.last_step_form == "eager" and model.last_step_kernel == "wmrb_fused"

    refused("Euclidean", kind="euclid")

    class Mine(AbstractPredictionGraph):                            # a user-defined prediction graph
        def connect_dense_prediction_graph(self, tf_user_representation, tf_item_representation):
            return tf_user_representation @ tf_item_representation.T

        def connect_serial_prediction_graph(self, tf_user_representation, tf_item_representation, tf_x_user, tf_x_item):
            return (tf_user_representation[tf_x_user.long()] * tf_item_representation[tf_x_item.long()]).sum(1)
    model = T.TensorRec(n_components=8, prediction_graph=Mine(), loss_graph=L.WMRBLossGraph(), sampler=T.HardNegativeSampler(6))
    with pytest.raises(ValueError, match="built-in"):
        model.fit_partial(*data, epochs=1, n_sampled_items=3)
    refused("one taste", n_tastes=2)
    refused("one taste", n_tastes=2, attention_graph=LinearRepresentationGraph())

    class Wide(LinearRepresentationGraph):
        def connect_representation_graph(self, tf_features, n_components, n_features, node_name_ending):
            return super(Wide, self).connect_representation_graph(tf_features, 2 * n_components, n_features, node_name_ending)
    refused("equally wide", item_repr_graph=Wide())
    refused("shared negatives", loss=L.SampledSoftmaxLossGraph(shared_negatives=True))
    refused("log_q_correction", loss=L.SampledSoftmaxLossGraph(log_q_correction=True))
    refused("does not cover", n_components=6)
    refused("does not cover", sampler=T.HardNegativeSampler(5000), S=3)
    refused("n_candidates = 2 is below", sampler=T.HardNegativeSampler(2))
    refused("n_hard = 4 is above", sampler=T.HardNegativeSampler(6, n_hard=4))
    model, data = two_user_model()
    monkeypatch.setattr(model, "_dp_active", lambda: True)          # (a data-parallel fit needs a process group: only the answer is faked)
    with pytest.raises(ValueError, match="data-parallel"):
        model.fit_partial(*data, epochs=1, n_sampled_items=3)


def test_a_longer_fit_stays_eager(ops, N):
    """epochs enough for the HIP-graph and cooperative forms to engage for any other sampler: a scored one keeps every step eager"""
    import tensorrec_amd as T
    inter, uf, itf, _ = model_data()
    for scored in (True, False):
        sampler = T.HardNegativeSampler(M_MODEL, n_hard=3, seed=4) if scored else T.DeviceSampler(4)
        model = make_model("dot", losses()["wmrb"](), sampler, deterministic=False)       # (a deterministic fit is eager anyway)
        forms = set()
        for _ in range(2):
            model.fit_partial(inter, uf, itf, epochs=4, n_sampled_items=S_MODEL)
            forms.add(model.last_step_form)
        assert forms == {"eager"} if scored else forms & {"coop", "graph"}


def test_save_and_load(ops, N, tmp_path):
    import tensorrec_amd as T
    inter, uf, itf, C = model_data()
    sampler = T.HardNegativeSampler(M_MODEL, base=T.ReplaySampler([C]), n_hard=3, keep_last=True)
    model = make_model("dot", losses()["bpr"](), sampler)
    model.fit_partial(inter, uf, itf, epochs=2, n_sampled_items=S_MODEL)
    assert sampler.last_table is not None
    model.save_model(str(tmp_path / "m"))
    loaded = T.TensorRec.load_model(str(tmp_path / "m"))
    s = loaded.sampler
    assert type(s) is T.HardNegativeSampler and (s.n_candidates, s.n_hard, s.keep_last) == (M_MODEL, 3, True)
    assert s.last_table is None and s.last_candidates is None and sampler.last_table is not None
    for k, v in model.get_weights().items():
        assert np.array_equal(v, loaded.get_weights()[k])
    model.fit_partial(inter, uf, itf, epochs=1, n_sampled_items=S_MODEL)             # both go on from the same weights and step
    loaded.fit_partial(inter, uf, itf, epochs=1, n_sampled_items=S_MODEL)
    assert torch.equal(s.last_table, sampler.last_table) and loaded.last_step_form == "eager"
