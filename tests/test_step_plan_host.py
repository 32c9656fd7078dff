"""The route table of the training step (tensorrec_amd/step_plan.py), pinned on the host: which one-pass kernel a step takes for its
loss, prediction graph, shape and tuning switches, and which launch form ("coop", "graph", "eager") a batch may take.  The expected
values were read off the predicates of TensorRec._train_step, TensorRec._graph_eligible and _CoopStep.plan as they stood before the
planner existed (``_predicates_before`` restates the first, word for word, on the native library's shape queries); the shapes the
GPU tests pin through ops.*_supported appear here with the answers they pin."""
from types import SimpleNamespace

import numpy as np
import pytest

from tensorrec_amd import _native as N
from tensorrec_amd import ops
from tensorrec_amd import step_plan as P
from tensorrec_amd import tensorrec as TT
from tensorrec_amd.loss_graphs import (WMRBLossGraph, BalancedWMRBLossGraph, SampledSoftmaxLossGraph, BPRLossGraph, RMSELossGraph)

DOT, EUCLID = ops.MODE_DOT, ops.MODE_EUCLIDEAN
ON = P.Switches(True, True, True, True, True)
KERNELS = ("wmrb_fused", "wmrb_tiled", "softmax_fused", "softmax_shared")


def _case(expected, loss, mode, S, row, d, engine=True, multi=False, same_width=True, shared=False, hits=False, **off):
    inputs = dict(loss=loss, engine=engine, engine_mode=mode, multi=multi, same_width=same_width, n_sampled=S, max_row_nnz=row, d=d,
                  shared_negatives=shared, remove_accidental_hits=hits, switches=ON._replace(**{name: False for name in off}))
    tags = [("engine", not engine), ("tastes", multi), ("unequal", not same_width), ("shared", shared), ("nohits", hits)]
    return pytest.param(inputs, expected, id="%s-%s-S%s-row%d-d%d-%s%s" % (
        loss, {DOT: "dot", EUCLID: "euclid", None: "custom"}[mode], S, row, d, expected,
        "".join("-" + t for t, on in tags if on) + "".join("-" + n + "_off" for n in off)))


# tests/test_gpu_model.py pins the fused side of the first three WMRB shapes; at d = 130 (d % 4 != 0) the tiled step's own query decides
TILED_130 = "wmrb_tiled" if N.query("trec_wmrb_tiled_lds_bytes", 100, 20, 130) >= 0 else None
CASES = (
    # WMRB on dot / cosine scores: rows in registers while S + the longest row fit, the tiled step beyond, nothing beyond d = 512
    [_case("wmrb_fused", "wmrb", DOT, 100, 100, 128), _case("wmrb_fused", "wmrb", DOT, 100, 20, 128),
     _case("wmrb_tiled", "wmrb", DOT, 300, 100, 128), _case("wmrb_tiled", "wmrb", DOT, 300, 20, 128),
     _case("wmrb_tiled", "wmrb", DOT, 40, 2600, 64), _case(TILED_130, "wmrb", DOT, 100, 20, 130),
     _case("wmrb_fused", "wmrb", DOT, 168, 88, 64), _case("wmrb_fused", "wmrb", DOT, 4, 6, 8),
     _case("wmrb_tiled", "wmrb", DOT, 100, 100, 512), _case(None, "wmrb", DOT, 100, 100, 516), _case(None, "wmrb", DOT, 100, 100, 1024)] +
    # Euclidean scores: the tiled step, never the fused one
    [_case("wmrb_tiled", "wmrb", EUCLID, 100, 100, 128), _case("wmrb_tiled", "wmrb", EUCLID, 4, 6, 8),
     _case("wmrb_tiled", "wmrb", EUCLID, 300, 100, 128), _case(None, "wmrb", EUCLID, 100, 100, 516),
     _case(None, "wmrb", EUCLID, 100, 100, 128, wmrb_tiled=False), _case("wmrb_tiled", "wmrb", EUCLID, 100, 100, 128, wmrb_fused=False)] +
    # BalancedWMRB: the same table
    [_case("wmrb_fused", "balanced_wmrb", DOT, 100, 100, 128), _case("wmrb_tiled", "balanced_wmrb", DOT, 300, 100, 128),
     _case("wmrb_tiled", "balanced_wmrb", DOT, 40, 2600, 64), _case("wmrb_tiled", "balanced_wmrb", EUCLID, 100, 100, 128),
     _case(None, "balanced_wmrb", DOT, 100, 100, 516)] +
    # a subclass of a built-in loss (no kind), another loss, a custom prediction graph, several tastes, unequal widths, no sample count
    [_case(None, None, DOT, 100, 100, 128), _case(None, None, EUCLID, 100, 100, 128),
     _case(None, "wmrb", None, 100, 100, 128, engine=False), _case(None, "sampled_softmax", None, 3, 125, 132, engine=False),
     _case(None, "wmrb", DOT, 100, 100, 128, multi=True), _case(None, "sampled_softmax", DOT, 3, 125, 132, multi=True),
     _case(None, "wmrb", DOT, 100, 100, 128, same_width=False), _case(None, "sampled_softmax", DOT, 3, 125, 132, same_width=False),
     _case(None, "wmrb", DOT, None, 100, 128), _case(None, "sampled_softmax", DOT, None, 100, 128)] +
    # sampled softmax on dot / cosine scores: the fused step and its uncovered neighbours (tests/softmax_step_reference.py UNCOVERED)
    [_case("softmax_fused", "sampled_softmax", DOT, 3, 125, 132), _case("softmax_fused", "sampled_softmax", DOT, 4, 6, 8),
     _case("softmax_fused", "sampled_softmax", DOT, 7, 20, 36), _case("softmax_fused", "sampled_softmax", DOT, 3, 125, 132, hits=True),
     _case(None, "sampled_softmax", DOT, 3, 126, 132), _case(None, "sampled_softmax", DOT, 1, 256, 128),
     _case(None, "sampled_softmax", DOT, 257, 1, 128), _case(None, "sampled_softmax", DOT, 7, 5, 6),
     _case(None, "sampled_softmax", EUCLID, 3, 125, 132), _case(None, "sampled_softmax", EUCLID, 4, 6, 8, shared=True)] +
    # one shared row of samples: the MFMA step for d % 4 == 0, 4 <= d <= 128 whatever the rows are -- and never the per-user kernel,
    # not with hits removed, not at an uncovered d, not with the switch off
    [_case("softmax_shared", "sampled_softmax", DOT, 65, 100, d, shared=True) for d in (4, 8, 128)] +
    [_case("softmax_shared", "sampled_softmax", DOT, 4096, 5000, 128, shared=True)] +
    [_case(None, "sampled_softmax", DOT, 65, 100, d, shared=True) for d in (2, 6, 132)] +
    [_case(None, "sampled_softmax", DOT, 3, 125, 132, shared=True),
     _case(None, "sampled_softmax", DOT, 65, 100, 128, shared=True, hits=True),
     _case(None, "sampled_softmax", DOT, 4, 6, 8, shared=True, hits=True),
     _case(None, "sampled_softmax", DOT, 4, 6, 8, shared=True, softmax_shared=False)] +
    # every switch off in turn: only its own route moves
    [_case("wmrb_tiled", "wmrb", DOT, 100, 100, 128, wmrb_fused=False),
     _case(None, "wmrb", DOT, 100, 100, 128, wmrb_fused=False, wmrb_tiled=False),
     _case("wmrb_fused", "wmrb", DOT, 100, 100, 128, wmrb_tiled=False), _case(None, "wmrb", DOT, 300, 100, 128, wmrb_tiled=False),
     _case(None, "sampled_softmax", DOT, 3, 125, 132, softmax_fused=False),
     _case("softmax_fused", "sampled_softmax", DOT, 3, 125, 132, softmax_shared=False),
     _case("softmax_shared", "sampled_softmax", DOT, 4, 6, 8, shared=True, softmax_fused=False),
     _case("wmrb_fused", "wmrb", DOT, 100, 100, 128, softmax_fused=False, softmax_shared=False, fit_step_coop=False),
     _case("softmax_fused", "sampled_softmax", DOT, 4, 6, 8, wmrb_fused=False, wmrb_tiled=False, fit_step_coop=False)]
)


def _predicates_before(loss, engine, engine_mode, multi, same_width, n_sampled, max_row_nnz, d, shared_negatives,
                       remove_accidental_hits, switches):
    """TensorRec._train_step's choice as it was written before step_plan existed: two guards, four flags, each decided by "the tuning
    is on and the native query says yes" -- restated here on the queries themselves."""
    def lds(name):
        return getattr(switches, name) and N.query("trec_%s_lds_bytes" % name, int(n_sampled), int(max_row_nnz), int(d)) >= 0
    fused = tiled = fused_softmax = shared_mfma = False
    if (engine and not multi and engine_mode in (DOT, EUCLID) and loss in ("wmrb", "balanced_wmrb")
            and n_sampled is not None and same_width):
        fused = engine_mode == DOT and lds("wmrb_fused")
        tiled = not fused and lds("wmrb_tiled")
    elif (engine and not multi and engine_mode == DOT and loss == "sampled_softmax" and n_sampled is not None and same_width):
        if not shared_negatives:
            fused_softmax = lds("softmax_fused")
        elif not remove_accidental_hits:
            shared_mfma = switches.softmax_shared and bool(N.query("trec_softmax_shared_supported", int(n_sampled), int(d)))
    return "wmrb_fused" if fused else "wmrb_tiled" if tiled else "softmax_fused" if fused_softmax else \
        "softmax_shared" if shared_mfma else None


@pytest.mark.parametrize("inputs,expected", CASES)
def test_kernel(inputs, expected):
    assert _predicates_before(**inputs) == expected
    assert P.kernel(**inputs) == expected
    if inputs["switches"] == ON:                      # (the library's defaults: reading them gives the same answer)
        assert P.kernel(**dict(inputs, switches=None)) == expected


@pytest.mark.parametrize("inputs,expected", CASES)
def test_supported_functions_agree_with_the_plan(inputs, expected):
    """ops.*_supported (switch on, and the shape query says yes) under the default switches: the plan names a kernel only where its
    function says yes, and a covered shape it passes over is one the route order or a rule of the table took away."""
    S, row, d = inputs["n_sampled"], inputs["max_row_nnz"], inputs["d"]
    if S is None:
        return
    inter = SimpleNamespace(max_row_nnz=row)
    says = {"wmrb_fused": ops.wmrb_fused_supported(S, inter, d), "wmrb_tiled": ops.wmrb_tiled_supported(S, inter, d),
            "softmax_fused": ops.softmax_fused_supported(S, inter, d), "softmax_shared": ops.softmax_shared_supported(S, inter, d)}
    assert says == {name: ops.step_covers(name, S, row, d) for name in KERNELS}
    assert says["wmrb_fused"] == says["softmax_fused"]                                      # (one coverage, user_fused_body.hpp)
    plan = P.kernel(**dict(inputs, switches=ON))
    assert plan is None or says[plan]
    plain = inputs["engine"] and not inputs["multi"] and inputs["same_width"]
    if plain and inputs["loss"] in P.WMRB_KINDS and inputs["engine_mode"] == DOT:
        assert plan == ("wmrb_fused" if says["wmrb_fused"] else "wmrb_tiled" if says["wmrb_tiled"] else None)
    if plain and inputs["loss"] in P.WMRB_KINDS and inputs["engine_mode"] == EUCLID:
        assert plan == ("wmrb_tiled" if says["wmrb_tiled"] else None)
    if plain and inputs["loss"] == "sampled_softmax" and inputs["engine_mode"] == DOT:
        if not inputs["shared_negatives"]:
            assert plan == ("softmax_fused" if says["softmax_fused"] else None)
        else:
            assert plan == ("softmax_shared" if says["softmax_shared"] and not inputs["remove_accidental_hits"] else None)


def test_loss_kinds_are_the_exact_builtin_classes():
    class MyWMRB(WMRBLossGraph):
        pass

    class MySoftmax(SampledSoftmaxLossGraph):
        pass

    assert P.loss_kind(WMRBLossGraph()) == "wmrb" and P.loss_kind(BalancedWMRBLossGraph()) == "balanced_wmrb"
    assert P.loss_kind(SampledSoftmaxLossGraph(0.5, shared_negatives=True)) == "sampled_softmax"
    assert [P.loss_kind(g) for g in (MyWMRB(), MySoftmax(), BPRLossGraph(), RMSELossGraph(), None)] == [None] * 5
    assert P.WMRB_KINDS == ("wmrb", "balanced_wmrb") and sorted(P.LOSS_KINDS.values()) == sorted(P.WMRB_KINDS + ("sampled_softmax",))


def test_switches_are_read_from_the_library():
    assert P.read_switches() == ON and ops.SOFTMAX_SHARED_DEFAULT == 1
    shapes = [c.values[0] for c in CASES if c.values[0]["switches"] == ON]
    for name in P.Switches._fields:
        N.set_tuning(name, 0)
        try:
            off = ON._replace(**{name: False})
            assert P.read_switches() == off
            for shape in shapes:
                assert P.kernel(**dict(shape, switches=None)) == P.kernel(**dict(shape, switches=off)) == \
                    _predicates_before(**dict(shape, switches=off))
        finally:
            N.clear_tuning(name)
    assert P.read_switches() == ON


# ---------------------------------------------------------------------------------------------------------------- launch forms
GRAPH_OK = dict(hip_graphs=True, dp=False, capturing=False, deterministic=False, shared_negatives=False, loss_capturable=True,
                engine_graph=True, n_graphs=0, nnz=90_000, n_users=943, n_items=1682, n_sampled=168, dense_loss=False)


@pytest.mark.parametrize("change,expected", [
    ({}, True),
    ({"hip_graphs": False}, False), ({"dp": True}, False), ({"capturing": True}, False), ({"deterministic": True}, False),
    ({"shared_negatives": True}, False), ({"loss_capturable": False}, False), ({"engine_graph": False}, False),
    # 64 graphs held by the fit call: the 65th batch runs eagerly
    ({"n_graphs": 63}, True), ({"n_graphs": 64}, False), ({"n_graphs": 65}, False),
    # interactions + sampled pairs: 4,000,000 is in, 4,000,001 out; no sample count counts as none
    ({"nnz": 4_000_000 - 943 * 168}, True), ({"nnz": 4_000_001 - 943 * 168}, False),
    ({"nnz": 4_000_000, "n_sampled": None}, True), ({"nnz": 4_000_001, "n_sampled": None}, False),
    ({"nnz": 4_000_000, "n_sampled": 0}, True), ({"nnz": 0, "n_users": 1000, "n_sampled": 4000}, True),
    ({"nnz": 1, "n_users": 1000, "n_sampled": 4000}, False),
    # a dense loss also holds [U, I] tensors: U * I within the same limit; a sampled loss does not care
    ({"dense_loss": True, "n_sampled": None}, True), ({"dense_loss": True, "n_sampled": None, "n_users": 2000, "n_items": 2000}, True),
    ({"dense_loss": True, "n_sampled": None, "n_users": 2000, "n_items": 2001}, False),
    ({"dense_loss": False, "n_sampled": None, "n_users": 2000, "n_items": 2001}, True),
], ids=lambda v: "-".join("%s=%s" % kv for kv in v.items()) or "baseline" if isinstance(v, dict) else str(v))
def test_graph_eligible(change, expected):
    assert P.graph_eligible(**dict(GRAPH_OK, **change)) is expected
    assert (P.MAX_GRAPHED_PAIRS, P.MAX_GRAPHED_BATCHES) == (4_000_000, 64)


def _config1_longest_row():
    """BASELINE.json configs[1] as tests/test_gpu_shapes.py generates it: 943 x 1682, 160 Zipf draws per user."""
    from test_gpu_shapes import zipf_interactions
    m = zipf_interactions(943, 1682, 160, np.random.default_rng(0))
    return int(np.diff(m.indptr).max())


COOP_OK = dict(dp=False, capturing=False, deterministic=False, multi=False, attention=False, linear_user=True, linear_item=True,
               dot_product=True, wmrb=True, identity_users=True, n_user_rows=943, n_users=943, n_items=1682, d=64, n_sampled=168,
               max_row_nnz=None, switches=ON)


@pytest.mark.parametrize("change,expected", [
    ({}, True),
    ({"dp": True}, False), ({"capturing": True}, False), ({"deterministic": True}, False), ({"multi": True}, False),
    ({"attention": True}, False), ({"linear_user": False}, False), ({"linear_item": False}, False), ({"dot_product": False}, False),
    ({"wmrb": False}, False), ({"identity_users": False}, False), ({"n_user_rows": 942}, False), ({"n_sampled": None}, False),
    ({"n_sampled": 0}, False), ({"switches": ON._replace(fit_step_coop=False)}, False),
    ({"switches": ON._replace(wmrb_fused=False, wmrb_tiled=False, softmax_fused=False, softmax_shared=False)}, True),
    # the sampler draws without replacement: no more samples than items
    ({"n_sampled": 1682, "max_row_nnz": 20}, True), ({"n_sampled": 1683, "max_row_nnz": 20}, False),
    ({"n_items": 168}, True), ({"n_items": 167}, False),
    # what the kernel's own workspace query refuses: d % 4 != 0, d > 128, LDS beyond 64 KB, G beyond 2^26 entries
    ({"d": 128}, True), ({"d": 132}, False), ({"d": 62}, False), ({"d": 2}, False), ({"max_row_nnz": 100_000}, False),
    ({"n_users": 1 << 14, "n_user_rows": 1 << 14, "n_items": (1 << 12) + 1}, False),
], ids=lambda v: ("-".join("%s=%s" % (k, "off" if k == "switches" else x) for k, x in v.items()) or "config1")
   if isinstance(v, dict) else str(v))
def test_coop_covered(change, expected):
    inputs = dict(COOP_OK, **change)
    if inputs["max_row_nnz"] is None:
        inputs["max_row_nnz"] = _config1_longest_row()
    assert P.coop_covered(**inputs) is expected
    if inputs["n_sampled"]:                            # the shape part alone is the workspace query's
        need = P.coop_workspace_floats(*(inputs[k] for k in ("n_users", "n_items", "d", "n_sampled", "max_row_nnz")))
        assert need == N.query("trec_fit_step_coop_workspace_floats", inputs["n_users"], inputs["n_items"], inputs["d"],
                               inputs["n_sampled"], inputs["max_row_nnz"])
        assert not expected or need > 0


def test_coop_switch_is_read_from_the_library():
    inputs = dict(COOP_OK, max_row_nnz=_config1_longest_row(), switches=None)
    assert P.coop_covered(**inputs) is True
    N.set_tuning("fit_step_coop", 0)
    try:
        assert P.coop_covered(**inputs) is False
    finally:
        N.clear_tuning("fit_step_coop")


# ---------------------------------------------------------------------------------------------------------------- Adam schedule
@pytest.mark.parametrize("t", [1, 2, 10, 1000])
def test_beta_powers_are_the_float32_running_products(t):
    b1p, b2p = np.float32(1.0), np.float32(1.0)
    for _ in range(t):
        b1p = np.float32(b1p * np.float32(0.9))
        b2p = np.float32(b2p * np.float32(0.999))
    lr_t = float(np.float32(np.float32(0.05) * np.sqrt(np.float32(1.0) - b2p) / (np.float32(1.0) - b1p)))
    got = TT._beta_powers(t)
    assert [type(x) for x in got] == [np.float32] * 2 and [x.tobytes() for x in got] == [b1p.tobytes(), b2p.tobytes()]
    assert TT._adam_lr_t(0.05, t) == lr_t and TT._adam_lr_t(0.05, t, got) == lr_t
    # going on from an earlier step (the cooperative step's cache) multiplies on in the same order: the same bits
    for t0 in {0, 1, t - 1, t}:
        on = TT._beta_powers(t, (t0,) + TT._beta_powers(t0))
        assert [x.tobytes() for x in on] == [b1p.tobytes(), b2p.tobytes()]
    coop = TT._CoopStep()
    coop.powers = None
    assert [coop._lr_t(0.05, s) for s in (t, t + 1)] == [lr_t, TT._adam_lr_t(0.05, t + 1)] and coop.powers[0] == t + 1
