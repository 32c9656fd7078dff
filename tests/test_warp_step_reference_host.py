"""tests/warp_step_reference.py on the CPU: the cases hold what their docstrings say (every instantiation, every planted row, no
ambiguous positive in the real-valued family, exact scores in the dyadic one); away from the discontinuities the float64 step's
gradients are central differences of its own summed loss with L held fixed; a float32 restatement of the kernel's arithmetic
(csrc/warp_fused.hip) in two summation orders lies inside the bars on every case the GPU test runs and each seeded defect that CAN
show leaves them; the route table of step_plan.warp_loss_kind / warp_kernel; the library's shape query against the mirror; the entry
point's argument checks, which need no device."""
import ctypes
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import pytest

import warp_step_reference as R
import warp_reference as W
from pair_reference import f64

SMALL = [(1, 3, 4), (7, 20, 36), (33, 20, 128)]                   # the cases the slower checks run on
IDS = lambda s: "S%d-L%d-d%d" % s


@pytest.mark.parametrize("spec", R.GPU_CASES, ids=IDS)
@pytest.mark.parametrize("exact", [False, True], ids=["real", "dyadic"])
def test_case_properties(spec, exact):
    S, longest, d = spec
    case = R.cached_case(spec, exact)
    lens = np.diff(case.indptr)
    pos = case.values > 0
    row = lambda u: np.arange(case.indptr[u], case.indptr[u + 1])
    assert case.n_users == R.N_USERS and 13 <= case.n_users <= 24
    assert lens.max() == longest == case.max_pos == lens[R.U_LONG] and S + longest <= R.rows_capacity(d)
    assert lens[R.U_NONE] == 0 and lens[R.U_NONPOS] > 0 and not pos[row(R.U_NONPOS)].any()
    assert lens[R.U_ONE] == 1 and pos[row(R.U_ONE)].all()
    assert longest < 5 or (pos[row(R.U_LONG)].any() and not pos[row(R.U_LONG)].all())
    assert S < 2 or case.samples[R.U_LONG, 0] == case.samples[R.U_LONG, 1]
    assert (case.samples >= 0).all() and (case.samples < case.n_items).all() and (case.x_item < case.n_items).all()
    assert R.scores_exact(case) == exact
    for hits in (False, True):
        ref = R.cached_ref(spec, exact, True, hits)
        assert not ref.ambiguous, "ambiguous positives %s: choose another seed (warp_step_reference.SEEDS)" % ref.ambiguous
        for u, want in R.expected_first(case, hits).items():
            assert ref.first[row(u)].tolist() == want, (u, hits, ref.first[row(u)].tolist(), want)
        assert not R.cached_ref(spec, exact, False, hits).ambiguous
        if exact:
            assert not ref.b_pred_serial.any() and np.array_equal(ref.pred_serial.astype(np.float32).astype(np.float64), ref.pred_serial)
    ref, ref_h = R.cached_ref(spec, exact, True, False), R.cached_ref(spec, exact, True, True)
    w, wh = ref.warp, ref_h.warp
    one = lambda u: int(row(u)[0])
    # far above: every output of the positive an exact 0 with a bar of 0; far below: the first sample with the largest weight
    p = one(R.U_ABOVE)
    assert ref.first[p] == -1 and ref.coef_pairs[p] == 0 and ref.b_coef_pairs[p] == 0 and not ref.coef_samples[R.U_ABOVE].any()
    assert w.trials[one(R.U_BELOW)] == 1
    if exact and S >= 2:                                          # strictness: v_0 == 0 exactly does not violate
        yp = ref.pred_serial[one(R.U_STRICT)]
        ys = ref.scores.scores[case.x_item.size:].reshape(case.n_users, S)[R.U_STRICT]
        assert (1.0 - yp) + ys[0] == 0.0 and ref.first[one(R.U_STRICT)] == 1
    if longest >= 2:                                              # two stops on one slot: a sum of two terms
        a, b = row(R.U_TWO)
        k = ref.first[a]
        assert ref.first[b] == k and ref.coef_samples[R.U_TWO, k] == w.weight[a] + w.weight[b] and (w.weight[a] > 0 or S == 255)
    if S >= 3:                                                    # a duplicated item: only the first slot is stopped at
        assert case.samples[R.U_DUP, 1] == case.samples[R.U_DUP, 2] and ref.coef_samples[R.U_DUP, 1] > 0 == ref.coef_samples[R.U_DUP, 2]
    if S == 255:                                                  # the late row: a violator and a weight of exactly 0
        p = one(R.U_LAST)
        assert ref.first[p] == 254 and w.trials[p] == 255 > (case.n_items - 1) / 2 and w.weight[p] == 0 and ref.b_loss.size
        assert ref.coef_pairs[p] == 0 and ref.b_coef_pairs[p] == 0 and not ref.coef_samples[R.U_LAST].any()
        assert w.weight[one(R.U_B192)] > 0 and w.weight[one(R.U_B63)] > 0
    else:
        assert (w.weight[ref.first >= 0] > 0).all()
    # hit removal: a skipped hit is no trial; the only violator a hit; every sample a hit; a non-positive's column is no hit
    if S >= 2:
        p = one(R.U_HIT_BEFORE)
        assert (w.trials[p], wh.trials[p]) == (1, 1) and (ref.first[p], ref_h.first[p]) == (0, 1)
    assert ref_h.first[one(R.U_ONLY_HIT)] == -1 <= ref.first[one(R.U_ONLY_HIT)] - 1
    assert (ref_h.first[row(R.U_ALLHITS)] == -1).all() and not ref_h.coef_samples[R.U_ALLHITS].any() and not ref_h.dU[R.U_ALLHITS].any()
    if longest >= 2:
        assert case.samples[R.U_NONPOS_ITEM, 0] == case.x_item[row(R.U_NONPOS_ITEM)[1]] and not pos[row(R.U_NONPOS_ITEM)[1]]
        assert ref_h.first[one(R.U_NONPOS_ITEM)] == 0
    if S > 65:
        assert wh.trials[one(R.U_HIT63)] == 64 and ref_h.first[one(R.U_HIT63)] == 65


def test_cases_reach_every_instantiation_boundary_and_plant():
    assert {R.instantiation(S, L, d) for S, L, d in R.GPU_CASES} == R.ALL_INSTANTIATIONS
    reach = lambda k: any(S > k for S, _, _ in R.GPU_CASES)
    assert all(reach(k) for k in R.BOUNDARY.values()) and reach(65)
    assert any(S == 255 for S, _, _ in R.GPU_CASES) and any(S == 1 for S, _, _ in R.GPU_CASES)
    for S, L, d in R.UNCOVERED:
        assert R.instantiation(S, L, d) is None and R.lds_bytes(S, L, d) == -1


@pytest.mark.parametrize("hits", [False, True], ids=["plain", "hits"])
@pytest.mark.parametrize("biased", [False, True], ids=["nobias", "bias"])
def test_reference_gradients_are_central_differences(hits, biased):
    """d(sum_p L_p v_{f_p}) / d(entry) of U, V and the biases with f and L held fixed, h = 1e-6 in float64: the objective is linear in
    the scores, so the differences are exact up to rounding"""
    spec = (7, 20, 36)
    case = R.cached_case(spec, False)
    ref = R.ref_step(case, biased, hits)
    h = 1e-6
    rng = np.random.default_rng(3)
    U, V, ub, ib = f64(case.U), f64(case.V), f64(case.ub), f64(case.ib)

    def diff(name, index):
        out = []
        for sign in (1.0, -1.0):
            t = dict(U=U.copy(), V=V.copy(), ub=ub.copy(), ib=ib.copy())
            t[name][index] += sign * h
            out.append(R.loss_sum_fixed_weight(case, biased, ref, **t))
        return (out[0] - out[1]) / (2.0 * h)

    scale = 1.0 + np.abs(ref.coef_samples).max() * case.S
    touched = np.unique(np.concatenate([case.x_item, case.samples.reshape(-1)]))
    for u in range(case.n_users):
        c = int(rng.integers(case.d))
        assert abs(diff("U", (u, c)) - ref.dU[u, c]) <= 1e-6 * (scale + abs(ref.dU[u, c])), ("dU", u, c)
        if biased:
            assert abs(diff("ub", u) - ref.d_ub[u]) <= 1e-6 * scale, ("d_ub", u)
    for i in list(rng.choice(touched, size=12, replace=False)) + [case.n_reg + R.R_HIGH, case.n_reg + R.R_POS0]:
        c = int(rng.integers(case.d))
        assert abs(diff("V", (int(i), c)) - ref.dV[i, c]) <= 1e-6 * (scale + abs(ref.dV[i, c])), ("dV", i, c)
        if biased:
            assert abs(diff("ib", int(i)) - ref.d_ib[i]) <= 1e-6 * (scale + abs(ref.d_ib[i])), ("d_ib", i)
    no_pos = [R.U_NONE, R.U_NONPOS]
    assert not ref.dU[no_pos].any() and not ref.d_ub[no_pos].any() and not ref.b_dU[no_pos].any() and not ref.b_d_ub[no_pos].any()
    assert np.abs(ref.dU).max() > 1e-3


def outside(r):
    return max(r.values()) > 1.0


@pytest.mark.parametrize("spec", R.GPU_CASES, ids=IDS)
def test_float32_restatement_lies_inside_the_bars(spec):
    """both families, with and without hit removal; both summation orders and both bias settings on the small cases (the restatement
    is a Python loop over the pairs).  On the dyadic family pred_serial and first are the reference's bit for bit, and the loss phase
    equals warp_reference.f32_warp -- the restatement of the UNFUSED kernels -- on its own scores, bit for bit."""
    for exact in (False, True):
        case = R.cached_case(spec, exact)
        for hits in (False, True):
            for biased in ((False, True) if spec in SMALL else (True,)):
                ref = R.cached_ref(spec, exact, biased, hits)
                for order in (("seq", 8) if spec in SMALL else ("seq",)):
                    got = R.restate_f32(case, biased, hits, order)
                    r = R.ratios(got, ref, biased)
                    assert not outside(r), (spec, exact, hits, biased, order, r)
                    if exact:
                        assert np.array_equal(got.pred_serial, ref.pred_serial)
                unfused = W.f32_warp(as_loss_case(case, got), remove_hits=hits)
                for name, a in zip(("loss", "first", "coef_pairs", "coef_samples"), unfused):
                    assert np.array_equal(getattr(got, name), a), (spec, exact, hits, name)


def as_loss_case(case, got):
    """the input of the unfused loss kernels: the step's own float32 scores, upstream gradient 1"""
    return SimpleNamespace(indptr=case.indptr, values=case.values, pred=got.pred_serial, samp=got.sample_scores,
                           go=np.ones(int((case.values > 0).sum()), np.float32), n_items=case.n_items, n_users=case.n_users, S=case.S,
                           x_item=case.x_item, samples=case.samples)


@pytest.mark.parametrize("defect", [d for d in R.DEFECTS if d not in R.INVISIBLE_DEFECTS])
def test_seeded_defects_leave_the_bars(defect):
    worst = 0.0
    for spec in SMALL + [(100, 28, 128)]:
        for exact in (False, True):
            case = R.cached_case(spec, exact)
            for hits in (False, True):
                ref = R.cached_ref(spec, exact, True, hits)
                r = R.ratios(R.restate_f32(case, True, hits, "seq", defect=defect), ref, True)
                worst = max(worst, max(r.values()))
    assert worst > 1.0, (defect, worst)


def test_reverse_order_cannot_show_at_unit_gradient():
    """coef_s added in reverse interaction order: every term of a slot is the same float32 L (N_p is a function of f_p and of the
    user's mask alone), so the sum has one value in any order -- the restatement with the defect equals the one without, bit for bit,
    on a case where two positives do stop at one slot.  The order is pinned by the definition and by the unfused kernels, where the
    upstream gradient varies; at gradient 1 no test can see it."""
    assert R.INVISIBLE_DEFECTS == ("reverse",)
    spec = (33, 20, 128)
    for exact in (False, True):
        case = R.cached_case(spec, exact)
        ref = R.cached_ref(spec, exact, True, False)
        a, b = np.arange(case.indptr[R.U_TWO], case.indptr[R.U_TWO + 1])
        assert ref.first[a] == ref.first[b] >= 0 and ref.warp.weight[a] == ref.warp.weight[b] > 0
        good, bad = R.restate_f32(case, True, False), R.restate_f32(case, True, False, defect="reverse")
        for name in R.OUTPUTS:
            assert np.array_equal(getattr(good, name), getattr(bad, name)), name


# ------------------------------------------------------------------------------------------------ the route table
def test_route_table():
    from tensorrec_amd import ops, step_plan
    from tensorrec_amd.loss_graphs import WARPLossGraph, WMRBLossGraph, SampledSoftmaxLossGraph

    class Mine(WARPLossGraph):
        pass
    assert step_plan.warp_loss_kind(WARPLossGraph()) == "warp" and step_plan.warp_loss_kind(WARPLossGraph(True)) == "warp"
    assert step_plan.warp_loss_kind(Mine()) is None and step_plan.warp_loss_kind(WMRBLossGraph()) is None
    assert step_plan.warp_loss_kind(SampledSoftmaxLossGraph(1.0)) is None
    # what existing tests pin stays: no kind in kernel()'s table, five switches
    assert step_plan.loss_kind(WARPLossGraph()) is None and "warp" not in step_plan.LOSS_KINDS.values()
    assert step_plan.Switches._fields == ("wmrb_fused", "wmrb_tiled", "softmax_fused", "softmax_shared", "fit_step_coop")
    Row = namedtuple("Row", "loss engine engine_mode multi same_width n_sampled max_row_nnz d switch want")
    ok = dict(loss="warp", engine=True, engine_mode=ops.MODE_DOT, multi=False, same_width=True, n_sampled=100, max_row_nnz=28, d=128,
              switch=True, want="warp_fused")
    rows = [Row(**ok)]
    for change in (dict(loss=None), dict(loss="wmrb"), dict(engine=False), dict(engine_mode=ops.MODE_EUCLIDEAN), dict(engine_mode=None),
                   dict(multi=True), dict(same_width=False), dict(n_sampled=None), dict(switch=False), dict(switch=0)):
        rows.append(Row(**dict(ok, want=None, **change)))
    for S, L, d in R.UNCOVERED:
        rows.append(Row(**dict(ok, n_sampled=S, max_row_nnz=L, d=d, want=None)))
    for S, L, d in R.GPU_CASES:
        rows.append(Row(**dict(ok, n_sampled=S, max_row_nnz=L, d=d)))
    for row in rows:
        got = step_plan.warp_kernel(row.loss, row.engine, row.engine_mode, row.multi, row.same_width, row.n_sampled, row.max_row_nnz,
                                    row.d, switch=row.switch)
        assert got == row.want, row
    # the library's default reads as off; set, it is on; cleared, off again
    from tensorrec_amd import _native
    assert ops.WARP_FUSED_DEFAULT == 0 and not ops.step_switch("warp_fused")
    assert step_plan.warp_kernel(*ok_args(ok)) is None
    try:
        _native.set_tuning("warp_fused", 1)
        assert ops.step_switch("warp_fused") and step_plan.warp_kernel(*ok_args(ok)) == "warp_fused"
        assert step_plan.loss_kind(WARPLossGraph()) is None
    finally:
        _native.clear_tuning("warp_fused")
    assert not ops.step_switch("warp_fused")


def ok_args(ok):
    return [ok[k] for k in ("loss", "engine", "engine_mode", "multi", "same_width", "n_sampled", "max_row_nnz", "d")]


def test_shape_query_equals_the_mirror():
    from tensorrec_amd import _native, ops
    shapes = list(R.GPU_CASES) + list(R.UNCOVERED) + [(S, R.rows_capacity(d) - S + k, d) for S, _, d in R.GPU_CASES for k in (0, 1)]
    shapes += [(0, 1, 8), (8, -1, 8), (8, 8, 0), (8, 8, 260), (256, 0, 128), (129, 0, 256)]
    for S, L, d in shapes:
        want = R.lds_bytes(S, L, d)
        assert _native.query("trec_warp_fused_lds_bytes", S, L, d) == want == _native.query("trec_softmax_fused_lds_bytes", S, L, d)
        assert ops.step_covers("warp_fused", S, L, d) == (want >= 0)


def test_entry_point_refuses_bad_arguments_before_any_launch():
    from tensorrec_amd import _native
    lib = _native.load()
    p = ctypes.c_void_p(8)
    name = "trec_warp_fused_step"
    keys = ("U", "V", "ub", "ib", "indptr", "x_item", "pos_slot", "samples", "n_users", "n_items", "S", "d", "max_pos", "hits", "loss",
            "pred", "dU", "d_ub", "coef_s", "coef_p", "first", "hist", "rank")

    def rc(**over):
        a = dict(U=p, V=p, ub=p, ib=p, indptr=p, x_item=p, pos_slot=p, samples=p, n_users=0, n_items=500, S=7, d=36, max_pos=20, hits=1,
                 loss=p, pred=p, dU=p, d_ub=p, coef_s=p, coef_p=p, first=p, hist=p, rank=p)
        a.update(over)
        return lib.trec_warp_fused_step(*[a[k] for k in keys], None)

    assert rc() == 0                                               # n_users == 0: TREC_OK, no launch
    assert rc(first=None, hist=None, rank=None, ib=None, ub=None, d_ub=None) == 0
    for k in ("U", "V", "indptr", "samples", "loss", "pred", "dU", "coef_s", "coef_p"):
        assert rc(**{k: None}) == 1 and lib.trec_last_error() == (name + ": null pointer").encode(), k
    for k in ("ub", "d_ub"):
        assert rc(**{k: None}) == 1 and lib.trec_last_error() == (name + ": user_bias and d_user_bias go together").encode()
    assert rc(hist=None) == 1 and lib.trec_last_error() == (name + ": sample_rank needs sample_hist").encode()
    for n in (0, -1, 1 << 31):
        assert rc(n_items=n) == 1 and lib.trec_last_error() == (name + ": n_items must lie in [1, 2^31)").encode()
    assert rc(n_items=(1 << 31) - 1) == 0
    for k in ("x_item", "pos_slot"):
        assert rc(**{k: None}) == 1 and lib.trec_last_error() == (name + ": remove_hits needs the interaction arrays").encode()
        assert rc(**{k: None, "hits": 0}) == 0                    # (no user: the arrays are not read)
        assert rc(**{k: None, "hits": 0, "n_users": 1}) == 1 and lib.trec_last_error() == (name + ": null interaction arrays").encode()
    for S, L, d in R.UNCOVERED:                                    # before any launch, whatever n_users says
        assert rc(S=S, max_pos=L, d=d, n_users=5) == 3 and b"not covered" in lib.trec_last_error()
    assert rc(U=None, S=257) == 1                                  # an invalid argument wins over an uncovered shape
