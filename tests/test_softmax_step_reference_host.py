"""tests/softmax_step_reference.py on the CPU: the float64 step's gradients are central differences of its loss; a float32 restatement
of the kernel's arithmetic (csrc/softmax_fused.hip) in two summation orders lies inside the bars on every case the GPU test runs; each
seeded defect leaves them on at least one case; the case generator and the dispatch mirror hold what their docstrings say."""
import numpy as np
import pytest

import softmax_step_reference as R
from pair_reference import f64

SMALL = [(1, 3, 4), (7, 20, 36), (33, 20, 128)]                   # the cases the slower checks run on


@pytest.mark.parametrize("spec", R.GPU_CASES, ids=lambda s: "S%d-L%d-d%d" % s)
@pytest.mark.parametrize("exact", [False, True], ids=["real", "dyadic"])
def test_case_properties(spec, exact):
    S, longest, d = spec
    case = R.cached_case(spec, exact)
    p = R.case_properties(case)
    assert case.n_users == R.N_USERS and 9 <= case.n_users <= 40
    assert p["longest"] == longest == case.max_pos and p["rows"] == S + longest <= R.rows_capacity(d)
    assert p["no_interaction"] and p["nonpositive_only"] and p["one_positive"]
    assert p["mixed"] or longest < 3                              # (a row of one or two interactions cannot mix three signs)
    assert p["far_above"] >= R.FAR and p["far_below"] >= R.FAR and p["equal"] and p["all_equal"]
    assert p["span"] == (2 * R.SPAN if S > 1 else 0.0)
    assert p["all_hits"] and p["nonpos_item_no_hit"] and p["a_hit"] and p["duplicate"]
    assert (case.samples >= 0).all() and (case.samples < case.n_items).all() and (case.x_item < case.n_items).all()
    if exact:
        assert R.scores_exact(case)
        ref = R.cached_ref(spec, True, True, 1.0, "plain")
        assert not ref.b_pred_serial.any() and np.array_equal(ref.pred_serial.astype(np.float32).astype(np.float64), ref.pred_serial)
    else:
        assert not R.scores_exact(case)


def test_cases_reach_every_instantiation_and_edge():
    reached = {R.instantiation(S, L, d) for S, L, d in R.GPU_CASES}
    assert reached == R.ALL_INSTANTIATIONS
    rows = {(S + L, d <= 128) for S, L, d in R.GPU_CASES}
    assert (128, True) in rows and (256, True) in rows and (128, False) in rows
    assert {d for _, _, d in R.GPU_CASES} >= {4, 36, 128, 132, 256}
    for S, L, d in R.UNCOVERED:
        assert R.instantiation(S, L, d) is None and R.lds_bytes(S, L, d) == -1
    assert [S + L for S, L, d in R.UNCOVERED[:2]] == [129, 257]
    assert R.lds_bytes(7, 20, 36) == (4 * 28 + 16 + 8 * 36) * 4


@pytest.mark.parametrize("variant", list(R.VARIANTS))
@pytest.mark.parametrize("biased", [False, True], ids=["nobias", "bias"])
def test_reference_gradients_are_central_differences(variant, biased):
    """d(sum loss) / d(entry) of U, V and the biases at a handful of entries of every kind of user, h = 1e-6 in float64"""
    spec, T = (7, 20, 36), 0.5
    case = R.cached_case(spec, False)
    ref = R.ref_step(case, biased, T, variant)
    h = 1e-6
    rng = np.random.default_rng(3)
    U, V, ub, ib = f64(case.U), f64(case.V), f64(case.ub), f64(case.ib)

    def diff(name, index):
        out = []
        for sign in (1.0, -1.0):
            t = dict(U=U.copy(), V=V.copy(), ub=ub.copy(), ib=ib.copy())
            t[name][index] += sign * h
            out.append(R.loss_sum(case, biased, T, variant, **t))
        return (out[0] - out[1]) / (2.0 * h)

    touched = np.unique(np.concatenate([case.x_item, case.samples.reshape(-1)]))
    for u in range(case.n_users):
        c = int(rng.integers(case.d))
        assert abs(diff("U", (u, c)) - ref.dU[u, c]) <= 1e-6 * (1.0 + abs(ref.dU[u, c])), ("dU", u, c)
        if biased:
            assert abs(diff("ub", u) - ref.d_ub[u]) <= 1e-6 * (1.0 + np.abs(ref.g).max()), ("d_ub", u)
    for i in rng.choice(touched, size=12, replace=False):
        c = int(rng.integers(case.d))
        assert abs(diff("V", (int(i), c)) - ref.dV[i, c]) <= 1e-6 * (1.0 + abs(ref.dV[i, c])), ("dV", i, c)
        if biased:
            assert abs(diff("ib", int(i)) - ref.d_ib[i]) <= 1e-6 * (1.0 + abs(ref.d_ib[i])), ("d_ib", i)
    no_pos = [R.U_NONE, R.U_NONPOS]
    assert not ref.dU[no_pos].any() and not ref.d_ub[no_pos].any() and not ref.b_dU[no_pos].any() and not ref.b_d_ub[no_pos].any()
    if R.VARIANTS[variant][1]:
        assert not ref.dU[R.U_ALLHITS].any() and not ref.b_dU[R.U_ALLHITS].any()
        pos = case.values > 0
        sl = (np.cumsum(pos) - 1)[case.indptr[R.U_ALLHITS]:case.indptr[R.U_ALLHITS + 1]]
        assert not ref.loss[sl].any()


@pytest.mark.parametrize("spec", R.GPU_CASES, ids=lambda s: "S%d-L%d-d%d" % s)
def test_float32_restatement_lies_inside_the_bars(spec):
    """both summation orders, both families; all variants and both temperatures on the small cases, a rotating choice on the large ones
    (the restatement is a Python loop over the pairs)"""
    k = R.GPU_CASES.index(spec)
    variants = list(R.VARIANTS)
    combos = [(v, T) for v in variants for T in R.TEMPERATURES] if spec in SMALL else \
        [("plain", R.TEMPERATURES[k % 2]), (variants[1 + k % 5], R.TEMPERATURES[(k + 1) % 2])]
    for exact in (False, True):
        case = R.cached_case(spec, exact)
        for variant, T in combos:
            for biased in ((False, True) if spec in SMALL else (True,)):
                ref = R.cached_ref(spec, exact, biased, T, variant)
                for order in ("seq", 8):
                    r = R.ratios(R.restate_f32(case, biased, T, variant, order), ref, biased)
                    assert max(r.values()) <= 1.0, (spec, exact, variant, T, biased, order, r)


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_seeded_defects_leave_the_bars(defect):
    worst = 0.0
    for spec in SMALL:
        for exact in (False, True):
            case = R.cached_case(spec, exact)
            for variant in ("plain", "both", "hits", "logq"):
                for T in R.TEMPERATURES:
                    ref = R.cached_ref(spec, exact, True, T, variant)
                    r = R.ratios(R.restate_f32(case, True, T, variant, "seq", defect=defect), ref, True)
                    worst = max(worst, max(r.values()))
    assert worst > 1.0, (defect, worst)
