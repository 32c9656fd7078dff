"""One tiny fit per route of the training step: the kernel the last step reports is the one tensorrec_amd/step_plan.py names for that
model and batch, and the launch form is the one the plan's form functions allow.  The table itself is pinned on the host
(tests/test_step_plan_host.py); this file holds the model to it."""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

import tensorrec_amd as T  # noqa: E402
from tensorrec_amd import step_plan as P  # noqa: E402
from tensorrec_amd.loss_graphs import WMRBLossGraph, SampledSoftmaxLossGraph, BPRLossGraph  # noqa: E402
from tensorrec_amd.prediction_graphs import DotProductPredictionGraph, EuclideanSimilarityPredictionGraph  # noqa: E402

N_USERS, N_ITEMS, D, S, LONGEST = 48, 96, 8, 4, 6
# name: (loss graph, model options, identity user features, epochs, expected kernel, expected form)
ROUTES = {
    "wmrb_dot": (WMRBLossGraph, dict(hip_graphs=False), False, 3, "wmrb_fused", "eager"),
    "wmrb_euclid": (WMRBLossGraph, dict(hip_graphs=False, prediction_graph=EuclideanSimilarityPredictionGraph()), False, 3,
                    "wmrb_tiled", "eager"),
    "softmax": (lambda: SampledSoftmaxLossGraph(0.5), dict(hip_graphs=False), False, 3, "softmax_fused", "eager"),
    "softmax_shared": (lambda: SampledSoftmaxLossGraph(0.5, shared_negatives=True), {}, False, 3, "softmax_shared", "eager"),
    "softmax_shared_no_hits": (lambda: SampledSoftmaxLossGraph(0.5, shared_negatives=True, remove_accidental_hits=True), {}, False, 3,
                               None, "eager"),
    "bpr": (BPRLossGraph, dict(hip_graphs=False), False, 3, None, "eager"),
    "wmrb_identity_users": (WMRBLossGraph, {}, True, 3, "wmrb_fused", "coop"),        # (one cooperative kernel from step 2 on)
    "softmax_graph": (lambda: SampledSoftmaxLossGraph(0.5), dict(hip_graphs=True), False, 4, "softmax_fused", "graph"),
}


def data(identity_users):
    rng = np.random.default_rng(5)
    dense = np.zeros((N_USERS, N_ITEMS), np.float32)
    for u in range(N_USERS):
        dense[u, rng.choice(N_ITEMS, size=1 + u % LONGEST, replace=False)] = 1.0
    uf = sp.identity(N_USERS, dtype=np.float32, format="csr")
    if not identity_users:
        uf = sp.hstack([uf, sp.csr_matrix((np.arange(N_USERS) % 3 == 0).astype(np.float32).reshape(-1, 1))], format="csr")
    return sp.csr_matrix(dense), uf, sp.identity(N_ITEMS, dtype=np.float32, format="csr")


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_a_fit_takes_the_route_the_plan_names(route):
    loss, options, identity_users, epochs, kernel, form = ROUTES[route]
    inter, uf, itf = data(identity_users)
    assert int(np.diff(inter.indptr).max()) == LONGEST
    model = T.TensorRec(n_components=D, loss_graph=loss(), seed=3, **options)
    assert model.last_step_kernel is None and model.last_step_form is None
    model.fit(inter, uf, itf, epochs=epochs, learning_rate=0.05, n_sampled_items=S)
    graph, loss_graph = model.prediction_graph_factory, model.loss_graph_factory
    shared = bool(getattr(loss_graph, "shared_negatives", False))
    planned = P.kernel(P.loss_kind(loss_graph), True, graph.engine_mode, False, True, S, LONGEST, D, shared,
                       getattr(loss_graph, "remove_accidental_hits", False))
    assert planned == kernel
    assert model.last_step_kernel == planned
    assert model.last_step_form == form
    # the forms the plan allows this batch: "coop" first, then "graph" (a fit long enough to capture one), then "eager"
    coop = P.coop_covered(False, False, False, False, False, True, True, type(graph) is DotProductPredictionGraph,
                          P.loss_kind(loss_graph) in P.WMRB_KINDS, identity_users, uf.shape[0], N_USERS, N_ITEMS, D, S, LONGEST)
    graphed = P.graph_eligible(model.hip_graphs, False, False, False, shared, True, True, 0, inter.nnz, N_USERS, N_ITEMS, S, False)
    assert form == ("coop" if coop else "graph" if graphed and epochs >= 3 else "eager")
    assert all(np.isfinite(w).all() for w in model.get_weights().values())
