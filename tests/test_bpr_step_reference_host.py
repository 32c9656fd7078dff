"""tests/bpr_step_reference.py on the CPU: the cases hold what the loss phase of csrc/bpr_fused.hip needs (every instantiation, every
wave count and group count, the planted rows, exact scores in the dyadic family); the float64 step's gradients are central
differences of its own summed loss; a float32 restatement of the kernel's arithmetic in the shipped summation order and in another
one lies inside the bars on every case the GPU test runs and each seeded defect leaves them; the route table of
step_plan.bpr_loss_kind / bpr_kernel; the library's shape query against the mirror; the entry point's argument checks, which need no
device."""
import ctypes
from collections import namedtuple

import numpy as np
import pytest

import bpr_step_reference as R
import softmax_step_reference as SR
from pair_reference import f64

SMALL = [(1, 3, 4), (7, 20, 36), (33, 20, 128), (40, 5, 32)]      # the cases the slower checks run on
IDS = lambda s: "S%d-L%d-d%d" % s


@pytest.mark.parametrize("spec", R.SPECS, ids=IDS)
@pytest.mark.parametrize("exact", [False, True], ids=["real", "dyadic"])
def test_case_properties(spec, exact):
    S, longest, d = spec
    case = R.cached_case(spec, exact)
    p = R.case_properties(case)
    assert case.n_users == R.N_USERS == 13 and p["longest"] == longest == case.max_pos and p["rows"] <= R.rows_capacity(d)
    assert p["no_interaction"] and p["nonpositive_only"] and p["one_positive"] and p["all_equal"] and p["all_hits"]
    assert p["far_above"] >= SR.FAR and p["far_below"] >= SR.FAR and p["equal"]
    assert p["nonpos_item_no_hit"] and p["a_hit"] and p["duplicate"] and (S == 1 or p["span"] >= 59.0)
    assert R.scores_exact(case) == exact
    ref, ref_h = R.cached_ref(spec, exact, True, False), R.cached_ref(spec, exact, True, True)
    pos = case.values > 0
    row = lambda u: np.arange(case.indptr[u], case.indptr[u + 1])
    for r in (ref, ref_h):
        assert not r.coef_pairs[~pos].any() and not r.b_coef_pairs[~pos].any()
        for u in (R.U_NONE, R.U_NONPOS):
            assert not r.coef_samples[u].any() and not r.b_coef_samples[u].any() and not r.dU[u].any() and not r.b_dU[u].any()
        assert (r.coef_pairs[pos] <= 0).all() and (r.coef_samples >= 0).all() and (r.loss >= 0).all()
        if exact:
            assert not r.b_pred_serial.any() and np.array_equal(r.pred_serial.astype(np.float32).astype(np.float64), r.pred_serial)
    # far above: softplus and sigma of -100 (about 4e-44: still a term, a denormal in float32); far below: sigma = 1 to the last bit
    assert ref.loss[np.cumsum(pos)[case.planted.above] - 1] < 1e-40 and abs(ref.coef_pairs[case.planted.below] + 1.0) < 1e-40
    # hit removal: a hit is an exact 0 with a bar of 0; every sample a hit: the whole user is zeros
    assert ref_h.hits[R.U_ALLHITS].all() and not ref_h.coef_samples[ref_h.hits].any() and not ref_h.b_coef_samples[ref_h.hits].any()
    assert not ref_h.coef_pairs[row(R.U_ALLHITS)].any() and not ref_h.dU[R.U_ALLHITS].any() and ref.coef_samples[R.U_ALLHITS].all()
    assert not ref.hits.any() and (ref_h.loss <= ref.loss).all()


def test_specs_reach_every_instantiation_and_every_edge_of_the_loss_phase():
    assert {R.instantiation(S, L, d) for S, L, d in R.GPU_CASES} == R.ALL_INSTANTIATIONS
    assert all(R.instantiation(*s) is not None for s in R.SPECS)
    assert {R.sample_waves(S) for S, _, _ in R.SPECS} == {1, 2, 4}
    sizes = {S for S, _, _ in R.SPECS}
    assert {1, 64, 65, 128, 129, 192, 255} <= sizes               # both sides of every change of W, the skipped wave's range, the ends
    for spec in ((40, 5, 32), (65, 5, 64)):                       # rows that are no multiple of the group count, rows shorter than it
        G = 4 // R.sample_waves(spec[0])
        lens = set(np.diff(R.cached_case(spec, False).indptr).tolist())
        assert {1, 2, 3, 5} <= lens and any(n % G for n in lens) and any(0 < n < G for n in lens)
    for S, L, d in R.UNCOVERED:
        assert R.instantiation(S, L, d) is None and R.lds_bytes(S, L, d) == -1


@pytest.mark.parametrize("hits", [False, True], ids=["plain", "hits"])
@pytest.mark.parametrize("biased", [False, True], ids=["nobias", "bias"])
def test_reference_gradients_are_central_differences(hits, biased):
    """d(sum_p loss_p) / d(entry) of U, V and the biases, h = 1e-5 in float64 (the loss is smooth: the error of a central
    difference is O(h^2) times a third derivative of order 1 / S per pair)"""
    spec = (7, 20, 36)
    case = R.cached_case(spec, False)
    ref = R.ref_step(case, biased, hits)
    h = 1e-5
    rng = np.random.default_rng(3)
    U, V, ub, ib = f64(case.U), f64(case.V), f64(case.ub), f64(case.ib)

    def diff(name, index):
        out = []
        for sign in (1.0, -1.0):
            t = dict(U=U.copy(), V=V.copy(), ub=ub.copy(), ib=ib.copy())
            t[name][index] += sign * h
            out.append(R.loss_sum(case, biased, hits, **t))
        return (out[0] - out[1]) / (2.0 * h)

    scale = 1.0 + np.abs(V).max() * case.max_pos
    touched = np.unique(np.concatenate([case.x_item, case.samples.reshape(-1)]))
    for u in range(case.n_users):
        c = int(rng.integers(case.d))
        assert abs(diff("U", (u, c)) - ref.dU[u, c]) <= 1e-7 * (scale + abs(ref.dU[u, c])), ("dU", u, c)
        if biased:
            assert abs(diff("ub", u) - ref.d_ub[u]) <= 1e-7 * scale, ("d_ub", u)
    for i in rng.choice(touched, size=14, replace=False):
        c = int(rng.integers(case.d))
        assert abs(diff("V", (int(i), c)) - ref.dV[i, c]) <= 1e-7 * (scale + abs(ref.dV[i, c])), ("dV", i, c)
        if biased:
            assert abs(diff("ib", int(i)) - ref.d_ib[i]) <= 1e-7 * (scale + abs(ref.d_ib[i])), ("d_ib", i)
    assert np.abs(ref.dU).max() > 1e-3 and np.abs(ref.dV).max() > 1e-3


def outside(r):
    return max(r.values()) > 1.0


@pytest.mark.parametrize("spec", R.SPECS, ids=IDS)
def test_float32_restatements_lie_inside_the_bars(spec):
    """both families, with and without hit removal, the shipped summation order and the sequential one; both bias settings on the
    small cases (the restatement is a Python loop over the pairs).  On the dyadic family pred_serial is the reference's bit for bit."""
    for exact in (False, True):
        case = R.cached_case(spec, exact)
        for hits in (False, True):
            for biased in ((False, True) if spec in SMALL else (True,)):
                ref = R.cached_ref(spec, exact, biased, hits)
                for order in ("shipped", "seq"):
                    got = R.restate_f32(case, biased, hits, order)
                    r = R.ratios(got, ref, biased)
                    assert not outside(r), (spec, exact, hits, biased, order, r)
                    if exact:
                        assert np.array_equal(got.pred_serial, ref.pred_serial)


def test_one_cell_shares_e():
    """the restated cell: softplus and sigma from one e equal the separate expressions (the claim the kernel's softplus_sigmoid_f makes
    against softplus_f / sigmoid_f), and the butterfly of one term is the term"""
    x = np.concatenate([np.linspace(-104, 104, 4001), [0.0, -0.0, 88.0, -88.0]]).astype(np.float32)
    sp, sg = R.cell_f32(x)
    e = np.exp(-np.abs(x)).astype(np.float32)
    assert np.array_equal(sp, (np.maximum(x, np.float32(0)) + np.log1p(e).astype(np.float32)).astype(np.float32))
    assert np.array_equal(sg, (np.where(x >= 0, np.float32(1), e) / (np.float32(1) + e)).astype(np.float32))
    assert (sg >= 0).all() and (sg <= 1).all() and sg[x == 0].tolist() == [0.5] * int((x == 0).sum())
    assert R._butterfly64(np.array([0.3], np.float32)) == np.float32(0.3)


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_seeded_defects_leave_the_bars(defect):
    worst = 0.0
    for spec in SMALL + [(100, 28, 128)]:
        for exact in (False, True):
            case = R.cached_case(spec, exact)
            for hits in (False, True):
                ref = R.cached_ref(spec, exact, True, hits)
                r = R.ratios(R.restate_f32(case, True, hits, "shipped", defect=defect), ref, True)
                worst = max(worst, max(r.values()))
    assert worst > 1.0, (defect, worst)


# ------------------------------------------------------------------------------------------------ the route table
def test_route_table():
    from tensorrec_amd import ops, step_plan
    from tensorrec_amd.loss_graphs import BPRLossGraph, WARPLossGraph, WMRBLossGraph, SampledSoftmaxLossGraph

    class Mine(BPRLossGraph):
        pass
    assert step_plan.bpr_loss_kind(BPRLossGraph()) == "bpr" and step_plan.bpr_loss_kind(BPRLossGraph(True)) == "bpr"
    assert step_plan.bpr_loss_kind(Mine()) is None and step_plan.bpr_loss_kind(WMRBLossGraph()) is None
    assert step_plan.bpr_loss_kind(SampledSoftmaxLossGraph(1.0)) is None and step_plan.bpr_loss_kind(WARPLossGraph()) is None
    # what existing tests pin stays: no kind in kernel()'s table, five switches
    assert step_plan.loss_kind(BPRLossGraph()) is None and "bpr" not in step_plan.LOSS_KINDS.values()
    assert step_plan.warp_loss_kind(BPRLossGraph()) is None
    assert step_plan.Switches._fields == ("wmrb_fused", "wmrb_tiled", "softmax_fused", "softmax_shared", "fit_step_coop")
    Row = namedtuple("Row", "loss engine engine_mode multi same_width n_sampled max_row_nnz d switch want")
    ok = dict(loss="bpr", engine=True, engine_mode=ops.MODE_DOT, multi=False, same_width=True, n_sampled=100, max_row_nnz=28, d=128,
              switch=True, want="bpr_fused")
    rows = [Row(**ok)]
    for change in (dict(loss=None), dict(loss="warp"), dict(loss="wmrb"), dict(engine=False), dict(engine_mode=ops.MODE_EUCLIDEAN),
                   dict(engine_mode=None), dict(multi=True), dict(same_width=False), dict(n_sampled=None), dict(switch=False),
                   dict(switch=0)):
        rows.append(Row(**dict(ok, want=None, **change)))
    for S, L, d in R.UNCOVERED:
        rows.append(Row(**dict(ok, n_sampled=S, max_row_nnz=L, d=d, want=None)))
    for S, L, d in R.SPECS:
        rows.append(Row(**dict(ok, n_sampled=S, max_row_nnz=L, d=d)))
    for row in rows:
        got = step_plan.bpr_kernel(row.loss, row.engine, row.engine_mode, row.multi, row.same_width, row.n_sampled, row.max_row_nnz,
                                   row.d, switch=row.switch)
        assert got == row.want, row
    # the library's default reads as off; set, it is on; cleared, off again
    from tensorrec_amd import _native
    args = [ok[k] for k in ("loss", "engine", "engine_mode", "multi", "same_width", "n_sampled", "max_row_nnz", "d")]
    assert ops.BPR_FUSED_DEFAULT == 0 and not ops.step_switch("bpr_fused")
    assert step_plan.bpr_kernel(*args) is None
    try:
        _native.set_tuning("bpr_fused", 1)
        assert ops.step_switch("bpr_fused") and step_plan.bpr_kernel(*args) == "bpr_fused"
        assert step_plan.loss_kind(BPRLossGraph()) is None and not ops.step_switch("warp_fused")
    finally:
        _native.clear_tuning("bpr_fused")
    assert not ops.step_switch("bpr_fused")


def test_shape_query_equals_the_mirror():
    from tensorrec_amd import _native, ops
    shapes = list(R.SPECS) + list(R.UNCOVERED) + [(S, R.rows_capacity(d) - S + k, d) for S, _, d in R.SPECS for k in (0, 1)]
    shapes += [(0, 1, 8), (8, -1, 8), (8, 8, 0), (8, 8, 260), (256, 0, 128), (129, 0, 256), (64, 192, 128), (65, 191, 128), (129, 127, 4)]
    for S, L, d in shapes:
        want = R.lds_bytes(S, L, d)
        assert _native.query("trec_bpr_fused_lds_bytes", S, L, d) == want, (S, L, d)
        assert (want >= 0) == (_native.query("trec_softmax_fused_lds_bytes", S, L, d) >= 0)        # the same coverage
        assert want < 0 or want >= _native.query("trec_softmax_fused_lds_bytes", S, L, d) - 64    # (16 reduction words it does not need)
        assert ops.step_covers("bpr_fused", S, L, d) == (want >= 0)
    assert max(R.lds_bytes(S, R.rows_capacity(d) - S, d) for S in range(1, 257) for d in (128, 256) if S < R.rows_capacity(d)) <= 16 * 1024


def test_entry_point_refuses_bad_arguments_before_any_launch():
    from tensorrec_amd import _native
    lib = _native.load()
    p = ctypes.c_void_p(8)
    name = "trec_bpr_fused_step"
    keys = ("U", "V", "ub", "ib", "indptr", "x_item", "pos_slot", "samples", "n_users", "n_items", "S", "d", "max_pos", "hits", "loss",
            "pred", "dU", "d_ub", "coef_s", "coef_p", "hist", "rank")

    def rc(**over):
        a = dict(U=p, V=p, ub=p, ib=p, indptr=p, x_item=p, pos_slot=p, samples=p, n_users=0, n_items=500, S=7, d=36, max_pos=20, hits=1,
                 loss=p, pred=p, dU=p, d_ub=p, coef_s=p, coef_p=p, hist=p, rank=p)
        a.update(over)
        return lib.trec_bpr_fused_step(*[a[k] for k in keys], None)

    assert rc() == 0                                               # n_users == 0: TREC_OK, no launch
    assert rc(hist=None, rank=None, ib=None, ub=None, d_ub=None) == 0
    for k in ("U", "V", "indptr", "samples", "loss", "pred", "dU", "coef_s", "coef_p"):
        assert rc(**{k: None}) == 1 and lib.trec_last_error() == (name + ": null pointer").encode(), k
    for k in ("ub", "d_ub"):
        assert rc(**{k: None}) == 1 and lib.trec_last_error() == (name + ": user_bias and d_user_bias go together").encode()
    assert rc(hist=None) == 1 and lib.trec_last_error() == (name + ": sample_rank needs sample_hist").encode()
    for k in ("x_item", "pos_slot"):
        assert rc(**{k: None}) == 1 and lib.trec_last_error() == (name + ": remove_hits needs the interaction arrays").encode()
        assert rc(**{k: None, "hits": 0}) == 0                    # (no user: the arrays are not read)
        assert rc(**{k: None, "hits": 0, "n_users": 1}) == 1 and lib.trec_last_error() == (name + ": null interaction arrays").encode()
    for S, L, d in R.UNCOVERED:                                    # before any launch, whatever n_users says
        assert rc(S=S, max_pos=L, d=d, n_users=5) == 3 and b"not covered" in lib.trec_last_error()
    assert rc(U=None, S=257) == 1                                  # an invalid argument wins over an uncovered shape
