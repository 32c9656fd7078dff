"""Euclidean WMRB fit under a common offset of the representations (BASELINE.json configs[4]: ReLU + Euclidean + WMRB).

Euclidean scores do not change when one vector m is added to every user and every item representation, and neither do the loss
and the gradients with respect to the representations.  On the dense-G route of the tiled step (ops_base.wmrb_tiled_step) both
representation gradients are the difference of two GEMM products that DO grow with |m| -- dU = rowsum(G) U - G . V,
dV = colsum(G) V - G^T . U -- and the GEMMs run on split-bf16 operands, whose error is relative to the product.  Trained rows drift
along that direction freely and ReLU towers put a positive hidden mean into every row, so the tests below move the rows far along
it: (1) the same step from shifted and unshifted weights must give the same raw gradients (no oracle needed); (2) one step at the
configs[4] shape against oracle/model.py, with and without an offset."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import oracle as O
from oracle.model import OracleTensorRec

pytestmark = pytest.mark.gpu

import tensorrec_amd as T  # noqa: E402
from tensorrec_amd import ops  # noqa: E402
from tensorrec_amd.loss_graphs import WMRBLossGraph, BalancedWMRBLossGraph  # noqa: E402
from tensorrec_amd.prediction_graphs import EuclideanSimilarityPredictionGraph  # noqa: E402
from tensorrec_amd.representation_graphs import LinearRepresentationGraph, ReLURepresentationGraph  # noqa: E402

LOSS = {"wmrb": WMRBLossGraph, "balanced_wmrb": BalancedWMRBLossGraph}
REPR = {"linear": LinearRepresentationGraph, "relu": ReLURepresentationGraph}


def _offset(rows, ratio, rng):
    """A vector of norm ``ratio`` x the spread of ``rows`` (RMS norm of the rows about their mean), in a random direction."""
    spread = float(np.sqrt(((rows - rows.mean(axis=0)) ** 2).sum(axis=1).mean()))
    m = rng.standard_normal(rows.shape[1])
    return (ratio * spread * m / np.linalg.norm(m)).astype(np.float32)


def _set_tunings(tunings):
    for k, v in tunings.items():
        T._native.set_tuning(k, v)


@pytest.mark.parametrize("ratio,route,biased", [(10, "tiled+dense_g", True), (100, "tiled+dense_g", True),
                                                (10, "tiled+grouped", True), (100, "tiled+grouped", True),
                                                (100, "tiled+dense_g", False)])
def test_euclidean_step_is_translation_invariant(ratio, route, biased):
    """One replayed-sample step of Linear (identity features on both sides: the weight rows ARE the representations) + Euclidean +
    WMRB, from weights W and from W + m on both tables (|m| = 10 / 100 x the rows' spread): the loss, the serial predictions and the
    raw gradients (before L2 and Adam, which do see m) are the same -- on the dense-G route (S = 10 % of the items) and on the
    grouped route (tuning wmrb_dense_g = 0)."""
    n_users, n_items, d = 150, 400, 64
    S = n_items // 10
    rng = np.random.default_rng(21)
    inter = sp.random(n_users, n_items, density=0.05, random_state=6, format="csr", dtype=np.float32)
    inter.data[:] = np.where(rng.random(inter.nnz) < 0.85, 1.0, -1.0)
    inter[5, :] = 0                                   # a user without interactions
    inter.eliminate_zeros()
    uf = sp.identity(n_users, dtype=np.float32, format="csr")
    itf = sp.identity(n_items, dtype=np.float32, format="csr")
    tables = [O.sample_items(n_items, n_users, S, False, np.random.RandomState(8))[:, 1].reshape(n_users, S)]
    base = None
    caps = []
    tunings = {"wmrb_fused": 0, "wmrb_tiled": 1, "wmrb_dense_g": 1 if route == "tiled+dense_g" else 0}
    for shift in (False, True):
        ops.LAST_FUSED_STATS.pop("route", None)
        _set_tunings(tunings)
        try:
            model = T.TensorRec(n_components=d, prediction_graph=EuclideanSimilarityPredictionGraph(), loss_graph=WMRBLossGraph(),
                                biased=biased, sampler=T.ReplaySampler(tables), seed=3)
            model.build(n_users, n_items)
            if base is None:
                base = model.get_weights()
                if biased:
                    r2 = np.random.default_rng(7)
                    base["user_feature_biases"] = (0.1 * r2.standard_normal(base["user_feature_biases"].shape)).astype(np.float32)
                    base["item_feature_biases"] = (0.1 * r2.standard_normal(base["item_feature_biases"].shape)).astype(np.float32)
                m = _offset(np.concatenate([base["linear_weights_user_0"], base["linear_weights_item"]]), ratio, rng)
            w = {k: v.copy() for k, v in base.items()}
            if shift:
                w["linear_weights_user_0"] += m
                w["linear_weights_item"] += m
            model.set_weights(w)
            model._capture = {}
            model.fit_partial(inter, uf, itf, epochs=1, learning_rate=0.05, alpha=1e-5, n_sampled_items=S)
            caps.append((model._capture, ops.LAST_FUSED_STATS.get("route")))
        finally:
            _set_tunings({"wmrb_fused": 1, "wmrb_tiled": 1, "wmrb_dense_g": 1})
    (a, route_a), (b, route_b) = caps
    assert route_a == route_b == route, (route_a, route_b)
    assert np.allclose(b["loss"], a["loss"], rtol=1e-5, atol=1e-6), np.abs(b["loss"] - a["loss"]).max()
    assert np.allclose(b["pred_serial"], a["pred_serial"], rtol=1e-5, atol=1e-6), np.abs(b["pred_serial"] - a["pred_serial"]).max()
    gmax = max(np.abs(g).max() for g in a["grads"].values() if g is not None)
    errs = {k: float(np.abs(b["grads"][k] - ga).max()) for k, ga in a["grads"].items() if ga is not None}
    print("offset %d x spread, %s, biased=%s: raw gradient max err over gmax %s" % (ratio, route, biased,
          {k: "%.3g" % (e / gmax) for k, e in errs.items()}))
    for k, ga in a["grads"].items():
        if ga is None:
            assert b["grads"][k] is None or not np.abs(b["grads"][k]).any(), k
            continue
        assert errs[k] <= 1e-4 * gmax, "%s: %g of gmax %g" % (k, errs[k] / gmax, gmax)
        # per tensor as well (test_single_kernel_step_equals_multi_launch_steps): Adam rescales every variable by its own history.
        # (the user biases: exactly 0 under WMRB -- b_u cancels inside every hinge -- only rounding noise is left)
        if k != "user_feature_biases":
            assert errs[k] <= 1e-3 * np.abs(ga).max(), "%s: %g of its max %g" % (k, errs[k] / np.abs(ga).max(), np.abs(ga).max())


@pytest.mark.parametrize("case", ["relu_offset_0", "relu_offset_0_balanced", "linear_offset_100", "linear_offset_100_fp32"])
def test_configs4_step_vs_oracle_under_an_offset(case):
    """One replayed step at the configs[4] shape (26,744 items, with identity (+) 1,148 indicator features under ReLU towers; d = 256,
    ReLU hidden 1,024, Euclidean, S = 2,674, biased; a tile of users on identity features) against oracle/model.py (per-pair u - v
    through autograd), at the 1e-4 bar of the config records:
      relu_offset_0            the weights as initialised (the bench record's parity, in the test tier);
      relu_offset_0_balanced   the same under BalancedWMRB;
      linear_offset_100        Linear towers on identity features (the weight rows are the representations: the cancellation in
                               its cleanest form), m = 100 x the spread added to both tables;
      linear_offset_100_fp32   the same with tuning dense_g_split_bf16 = 0 (exact fp32 GEMMs): the control that the bar can be met
                               on this route.
    (No offset through the ReLU graph -- a hidden unit held at 1 for every row, m added to its output row: the fp32 oracle itself is
    2-3e-4 of gmax away from an fp64 evaluation of that model on the hidden biases' gradients, at any offset from 3x to 30x.)"""
    import bench_records as BR
    rng = np.random.default_rng(4)
    n_users, n_items, d = 128, 26_744, 256
    S = n_items // 10
    kind = "relu" if case.startswith("relu") else "linear"
    loss = "balanced_wmrb" if "balanced" in case else "wmrb"
    ratio = 0 if kind == "relu" else 100
    inter = BR._zipf_interactions(n_users, n_items, 160, rng, exponent=0.8)
    uf = sp.identity(n_users, dtype=np.float32, format="csr")
    itf = BR._side_features(n_items, 1148, 8, rng)
    if kind == "linear":
        itf = sp.identity(n_items, dtype=np.float32, format="csr")
    table = np.stack([rng.permutation(n_items)[:S] for _ in range(n_users)]).astype(np.int64)
    oracle = OracleTensorRec(d, kind, kind, "euclidean", loss, True)
    oracle.init_weights(uf.shape[1], itf.shape[1], np.random.default_rng(42))
    w = oracle.weights
    r2 = np.random.default_rng(7)       # non-zero biases: the item-bias gradient is exercised too
    w["user_feature_biases"] = (0.1 * r2.standard_normal(w["user_feature_biases"].shape)).astype(np.float32)
    w["item_feature_biases"] = (0.1 * r2.standard_normal(w["item_feature_biases"].shape)).astype(np.float32)
    if ratio:
        reps = oracle.representations(uf, itf)
        m = _offset(np.concatenate([reps["user_repr"], reps["item_repr"]]), ratio, rng)
        w["linear_weights_user"] += m
        w["linear_weights_item"] += m

    def mk(tables):
        return T.TensorRec(n_components=d, user_repr_graph=REPR[kind](), item_repr_graph=REPR[kind](),
                           prediction_graph=EuclideanSimilarityPredictionGraph(), loss_graph=LOSS[loss](), seed=0,
                           sampler=T.ReplaySampler(tables))
    ops.LAST_FUSED_STATS.pop("route", None)
    T._native.set_tuning("dense_g_split_bf16", 0 if case.endswith("fp32") else 1)
    try:
        rec = BR._one_step_parity(mk, oracle, inter, uf, itf, table, 0.01, 1e-5, S, 1e-4)
    finally:
        T._native.set_tuning("dense_g_split_bf16", 1)
    print("%s: raw gradient max err over gmax %s" % (case, {k: "%.3g" % v for k, v in rec["raw_gradient_max_err_over_gmax"].items()}))
    assert ops.LAST_FUSED_STATS.get("route") == "tiled+dense_g", ops.LAST_FUSED_STATS.get("route")
    assert rec["green"], "%s: raw_gradient_max_err_over_gmax %s; %s" % (case, rec["raw_gradient_max_err_over_gmax"], rec)
