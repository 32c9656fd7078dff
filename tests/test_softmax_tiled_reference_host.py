"""tests/softmax_tiled_reference.py held to itself on the CPU, and the host side of the tiled one-pass sampled-softmax step
(csrc/softmax_tiled.hip): the reference's gradients are central differences of its loss in both score modes; it equals
softmax_step_reference.ref_step on dot cases both cover; float32 restatements of the kernel's arithmetic -- in its strided summation
order and in plain order -- lie inside the bars on every GPU case, and six seeded defects leave them; the route table of
step_plan.softmax_tiled_kernel with every fallback; the native shape query against its mirror; the ABI's argument checks (they return
before any launch, so they need no GPU); the default tuning being off."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import softmax_step_reference as SR
import softmax_tiled_reference as R
from pair_reference import MODE_DOT, MODE_EUCLID, f64

MODES = [MODE_DOT, MODE_EUCLID]
TREC_ERR_INVALID, TREC_ERR_UNSUPPORTED = 1, 3          # include/tensorrec_hip.h


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("variant", ["plain", "both", "hits"])
@pytest.mark.parametrize("mode", MODES, ids=["dot", "euclid"])
def test_gradients_are_central_differences(mode, variant):
    """d(sum loss) / d(U, V, b_u, b_i) of the reference against central differences of its own loss, at entries away from the clamped
    pairs (the Euclidean score is not differentiable where the two rows are equal)"""
    case = R.tiled_case(6, 8, mode, rows=(7,), seed=1)
    T = 0.7
    ref = R.ref_step(case, True, T, variant)
    rng = np.random.default_rng(5)
    h = 1e-6
    users = [u for u in range(case.n_users) if u != R.U_CLAMP]
    items = [i for i in np.unique(np.concatenate([case.x_item, case.samples.reshape(-1)])) if i not in case.clamp]
    checked = 0
    for name, table, rows, grad in (("U", "U", users, ref.dU), ("V", "V", items, ref.dV), ("ub", "ub", users, ref.d_ub), ("ib", "ib", items, ref.d_ib)):
        for _ in range(12):
            r = int(rng.choice(rows))
            base = f64(getattr(case, table))
            k = (r, int(rng.integers(case.d))) if base.ndim == 2 else (r,)
            lo, hi = base.copy(), base.copy()
            lo[k] -= h
            hi[k] += h
            num = (R.loss_sum(case, True, T, variant, **{table: hi}) - R.loss_sum(case, True, T, variant, **{table: lo})) / (2 * h)
            assert abs(num - grad[k]) <= 2e-6 * max(1.0, abs(grad[k])), (name, k, num, grad[k])
            checked += abs(grad[k]) > 1e-8
    assert checked >= 20


@pytest.mark.parametrize("variant", ["plain", "hits", "logq", "logq-uniform", "both"])
@pytest.mark.parametrize("spec", R.SHARED_WITH_FUSED, ids=lambda s: "S%d-L%d-d%d" % s)
def test_equals_the_fused_steps_reference_on_dot_cases(spec, variant):
    """on the inputs of tests/softmax_step_reference.py the two float64 steps and their bars are the same numbers"""
    case = SR.cached_case(spec, False)
    a, b = R.ref_step(case, True, 0.25, variant), SR.cached_ref(spec, False, True, 0.25, variant)
    for name in ("loss", "pred_serial", "g", "dU", "dV", "d_ub", "d_ib"):
        assert np.allclose(getattr(a, name), getattr(b, name), rtol=1e-13, atol=0), name
        assert np.allclose(getattr(a, "b_" + name), getattr(b, "b_" + name), rtol=1e-12, atol=0), name
    assert np.array_equal(a.hits, b.hits) and np.array_equal(a.val, a.g)


@pytest.mark.parametrize("mode", MODES, ids=["dot", "euclid"])
def test_cases_hold_what_they_plant(mode):
    seen = set()
    for spec in R.ALL_CASES:
        case = R.cached_case(spec, mode)
        p = R.case_properties(case)
        assert p["no_interaction"] and p["nonpositive_only"] and p["one_positive"] and p["all_equal"] and p["all_hits"], spec
        assert p["far_above"] >= R.FAR - 0.125 and p["far_below"] >= R.FAR - 0.125 and p["span"] >= (2 * R.SPAN - 0.25 if case.S > 1 else 0), spec
        assert p["hit_is_max"] and p["nonpos_item_no_hit"] and p["duplicate"] and p["mixed_long"], spec
        assert p["rows"] == sorted(spec[2]) and case.n_users <= 24, spec
        if mode == MODE_EUCLID:
            assert p["clamp_pos"] == 0.0 and p["clamp_samp"] == 0.0, spec
        assert R.lds_bytes(case.S, case.max_pos, case.d) > 0
        seen |= {R.instantiation(case.d, mode, v) for v in R.VARIANTS}
    assert R.ALL_INSTANTIATIONS - seen == {i for i in R.ALL_INSTANTIATIONS if i[2] != mode}
    assert R.lds_bytes(R.BIG_LDS[0], R.cached_case(R.BIG_LDS, mode).max_pos, R.BIG_LDS[1]) > 64 * 1024
    assert sorted(R.LONG_ROWS[2]) == [255, 256, 257, 1025, 2600]
    dy = R.cached_case(R.D_CASES[3], MODE_DOT, True)
    assert R.scores_exact(dy) and not R.ref_step(dy, True, R.TEMPERATURE, "both").b_pred_serial.any()


# every GPU case once, spread over the variants and the two orders so that the file stays quick
def _restatement_runs():
    runs = []
    variants = list(R.VARIANTS)
    for k, spec in enumerate(R.ALL_CASES):
        for mode in MODES:
            runs.append((spec, mode, variants[(k + mode) % len(variants)], k % 2 == 0, "strided" if (k + mode) % 2 == 0 else "seq"))
            runs.append((spec, mode, variants[(k + mode + 2) % len(variants)], k % 2 == 1, "seq" if (k + mode) % 2 == 0 else "strided"))
    return runs


@pytest.mark.parametrize("spec,mode,variant,biased,order", _restatement_runs(),
                         ids=lambda v: ("S%d-d%d-%drows" % (v[0], v[1], len(v[2]))) if isinstance(v, tuple) else str(v))
def test_restatements_lie_inside_the_bars(spec, mode, variant, biased, order):
    case = R.cached_case(spec, mode)
    ref = R.cached_ref(spec, mode, False, biased, R.TEMPERATURE, variant)
    got = R.restate_f32(case, biased, R.TEMPERATURE, variant, order)
    r = R.ratios(got, ref, biased, R.OUTPUTS + ("g", "val"))
    assert max(r.values()) <= 1.0, r
    # the exact zeros of the contract
    zero_users = [R.U_NONE, R.U_NONPOS] + ([R.U_ALLHITS] if R.VARIANTS[variant][1] else [])
    assert not got.dU[zero_users].any() and not ref.b_dU[zero_users].any()
    nnz = case.x_item.size
    assert not got.val[nnz:].reshape(case.n_users, case.S)[ref.hits].any() and not ref.b_val[nnz:].reshape(case.n_users, case.S)[ref.hits].any()
    assert not got.val[:nnz][case.values <= 0].any()


DEFECT_RUNS = {"mask_ignored": (MODE_DOT, "hits"), "positive_corrected": (MODE_DOT, "logq"), "max_over_hits": (MODE_DOT, "both"),
               "euclid_unguarded": (MODE_EUCLID, "plain"), "k_over_nonpositives": (MODE_EUCLID, "plain"),
               "positive_without_t": (MODE_DOT, "plain")}


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_seeded_defects_fall_outside_the_bars(defect):
    spec = R.D_CASES[1]
    mode, variant = DEFECT_RUNS[defect]
    case = R.cached_case(spec, mode)
    ref = R.cached_ref(spec, mode, False, True, R.TEMPERATURE, variant)
    names = R.OUTPUTS + ("g", "val")
    good = R.ratios(R.restate_f32(case, True, R.TEMPERATURE, variant), ref, True, names)
    bad = R.ratios(R.restate_f32(case, True, R.TEMPERATURE, variant, defect=defect), ref, True, names)
    assert max(good.values()) <= 1.0 and max(bad.values()) > 1.0, (defect, bad)
    assert set(DEFECT_RUNS) == set(R.DEFECTS) and len(R.DEFECTS) >= 6


# ------------------------------------------------------------------------------------------------ the host side of the step
def test_shape_query_against_the_mirror():
    from tensorrec_amd import _native as N, ops
    for S in (0, 1, 3, 100, 255, 256, 257, 1025, 9000, 16000, 20000, 32000):
        for L in (0, 1, 20, 300, 2600, 16000, 32000):
            for d in (0, 2, 4, 6, 36, 64, 68, 128, 256, 512, 516):
                want = R.lds_bytes(S, L, d)
                assert N.query("trec_softmax_tiled_lds_bytes", S, L, d) == want, (S, L, d)
                assert ops.step_covers("softmax_tiled", S, L, d) == (want >= 0)
    assert N.query("trec_softmax_tiled_lds_bytes", 5, -1, 8) == -1
    for S, L, d in R.UNCOVERED:
        assert R.lds_bytes(S, L, d) == -1 and N.query("trec_softmax_tiled_lds_bytes", S, L, d) == -1
    # the edge of the 128 KB: the largest S at d = 128 without interactions, and one more
    S = (128 * 1024 // 4 - 8 * 128 - 24) // 3
    S -= S % 4
    assert R.lds_bytes(S, 0, 128) > 0 and R.lds_bytes(S + 4, 0, 128) == -1
    assert N.query("trec_softmax_tiled_lds_bytes", S, 0, 128) > 0 and N.query("trec_softmax_tiled_lds_bytes", S + 4, 0, 128) == -1
    # the ladder's mirror: sixteen kernels, the shapes of the WMRB step's ladder
    from step_reference import tiled_instantiation
    for d in (4, 64, 68, 128, 132, 256, 260, 512):
        for mode in MODES:
            assert R.instantiation(d, mode, "plain")[:4] == tiled_instantiation(d, mode) and R.instantiation(d, mode, "both")[4]
    assert len(R.ALL_INSTANTIATIONS) == 16


def test_default_tuning_is_off():
    from tensorrec_amd import _native as N, ops
    assert ops.SOFTMAX_TILED_DEFAULT == 0 and N.load().trec_get_tuning(b"softmax_tiled", -7) == -7
    assert not ops.step_switch("softmax_tiled")
    assert not ops.softmax_tiled_supported(100, SimpleNamespace(max_row_nnz=300), 128)
    N.set_tuning("softmax_tiled", 1)
    try:
        assert ops.step_switch("softmax_tiled") and ops.softmax_tiled_supported(100, SimpleNamespace(max_row_nnz=300), 128)
        assert not ops.softmax_tiled_supported(100, SimpleNamespace(max_row_nnz=300), 516)
    finally:
        N.clear_tuning("softmax_tiled")
    assert not ops.step_switch("softmax_tiled")


def _route(expected, loss="sampled_softmax", mode=MODE_DOT, S=100, row=300, d=128, engine=True, multi=False, same_width=True, shared=False,
           switch=True):
    return pytest.param(dict(loss=loss, engine=engine, engine_mode=mode, multi=multi, same_width=same_width, n_sampled=S, max_row_nnz=row,
                             d=d, shared_negatives=shared, switch=switch), expected)


ROUTES = [
    # what the step is for: a long row, S in the thousands, Euclidean scores, d up to 512
    _route("softmax_tiled"), _route("softmax_tiled", S=1025, row=20), _route("softmax_tiled", mode=1, S=4, row=6, d=8),
    _route("softmax_tiled", S=100, row=2600, d=512), _route("softmax_tiled", S=2674, row=3000, d=128),
    # (it also covers what the fused step covers: TensorRec asks only where kernel() said None)
    _route("softmax_tiled", S=7, row=20, d=36),
    # every fallback: the switch, another loss or a subclass (no kind), a custom prediction graph, a mode that is neither, several
    # tastes, unequal widths, no sample count, shared negatives, uncovered shapes
    _route(None, switch=False), _route(None, loss="wmrb"), _route(None, loss="warp"), _route(None, loss=None),
    _route(None, engine=False, mode=None), _route(None, mode=None), _route(None, mode=2), _route(None, multi=True),
    _route(None, same_width=False), _route(None, S=None), _route(None, shared=True), _route(None, mode=1, shared=True),
    _route(None, d=516), _route(None, d=130), _route(None, S=20000, row=5, d=8), _route(None, S=100, row=16000),
]


@pytest.mark.parametrize("inputs,expected", ROUTES)
def test_route_table(inputs, expected):
    from tensorrec_amd import step_plan as P
    assert P.softmax_tiled_kernel(**inputs) == expected
    if expected is not None:                # the library's switch is what None reads: off by default
        assert P.softmax_tiled_kernel(**dict(inputs, switch=None)) is None


def test_route_reads_the_library_switch_and_the_exact_class():
    from tensorrec_amd import _native as N, ops, step_plan as P
    from tensorrec_amd.loss_graphs import SampledSoftmaxLossGraph, BPRLossGraph

    class Sub(SampledSoftmaxLossGraph):
        pass
    args = dict(engine=True, engine_mode=ops.MODE_EUCLIDEAN, multi=False, same_width=True, n_sampled=100, max_row_nnz=300, d=128,
                shared_negatives=False)
    N.set_tuning("softmax_tiled", 1)
    try:
        assert P.softmax_tiled_kernel(P.loss_kind(SampledSoftmaxLossGraph(0.5)), **args) == "softmax_tiled"
        assert P.softmax_tiled_kernel(P.loss_kind(Sub(0.5)), **args) is None
        assert P.softmax_tiled_kernel(P.loss_kind(BPRLossGraph()), **args) is None
        # the existing table is untouched by the switch: the fused step keeps what it covers, Euclidean scores stay with kernel()'s None
        assert P.kernel("sampled_softmax", True, ops.MODE_DOT, False, True, 7, 20, 36, False, False) == "softmax_fused"
        assert P.kernel("sampled_softmax", True, ops.MODE_EUCLIDEAN, False, True, 7, 20, 36, False, False) is None
    finally:
        N.clear_tuning("softmax_tiled")
    assert "softmax_tiled" not in P.Switches._fields and set(P.LOSS_KINDS.values()) == {"wmrb", "balanced_wmrb", "sampled_softmax"}


def test_abi_argument_checks():
    """every check returns before any launch and before any pointer is read: made-up non-null addresses stand for the arrays"""
    from tensorrec_amd import _native as N
    lib = N.load()
    P = ctypes.c_void_p(4096)
    names = ("U", "V", "ub", "ib", "indptr", "x_item", "pos_slot", "samples", "n_users", "n_items", "S", "d", "mode", "max_pos", "t", "lq",
             "log_uniform", "use_q", "no_hits", "loss", "pred", "d_u", "d_ub", "val_s", "val_p", "raw_s", "raw_p", "G", "ldg", "rowsum")
    base = dict(U=P, V=P, ub=P, ib=P, indptr=P, x_item=P, pos_slot=P, samples=P, n_users=0, n_items=50, S=7, d=8, mode=0, max_pos=5, t=2.0,
                lq=P, log_uniform=-3.9, use_q=1, no_hits=1, loss=P, pred=P, d_u=P, d_ub=P, val_s=P, val_p=P, raw_s=None, raw_p=None, G=None,
                ldg=0, rowsum=None)

    def rc(**over):
        v = dict(base, **over)
        return lib.trec_softmax_tiled_step(*[v[k] for k in names], None)
    assert rc() == 0                                                # n_users == 0: TREC_OK, no launch
    for over in (dict(U=None), dict(V=None), dict(indptr=None), dict(samples=None), dict(loss=None), dict(pred=None), dict(val_s=None),
                 dict(val_p=None), dict(d_u=None), dict(d_u=None, G=P, ldg=50), dict(d_u=None, rowsum=P),
                 dict(mode=2), dict(mode=-1), dict(t=0.0), dict(t=-1.0), dict(t=float("inf")), dict(t=float("nan")),
                 dict(ub=None), dict(d_ub=None), dict(raw_s=P), dict(raw_p=P), dict(G=P, ldg=49),
                 dict(n_items=0), dict(n_items=1 << 31), dict(x_item=None), dict(pos_slot=None)):
        assert rc(**over) == TREC_ERR_INVALID, over
    assert rc(d_u=None, G=P, ldg=52, rowsum=P) == 0 and rc(raw_s=P, raw_p=P, mode=1) == 0 and rc(ub=None, d_ub=None) == 0
    assert rc(use_q=0, n_items=0) == 0 and rc(no_hits=0, x_item=None, pos_slot=None) == 0
    for S, L, d in R.UNCOVERED:
        assert rc(S=S, max_pos=L, d=d) == TREC_ERR_UNSUPPORTED and b"not covered" in lib.trec_last_error(), (S, L, d)
    assert rc(n_users=3, no_hits=0, x_item=None, pos_slot=None, max_pos=5) == TREC_ERR_INVALID     # rows without their arrays
