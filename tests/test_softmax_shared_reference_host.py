"""tests/softmax_shared_reference.py on the CPU: the float64 step's gradients are central differences of its loss; the shared
reference IS the per-user reference on the repeated table; a float32 restatement of the kernels' arithmetic (csrc/softmax_shared.hip)
in two summation orders lies inside the bars on every case the GPU test runs; each seeded defect leaves them; the constructor option,
an old pickle, the ABI's argument checks and the coverage mirror."""
import ctypes
import pickle

import numpy as np
import pytest

import softmax_shared_reference as R
import softmax_step_reference as SR
from pair_reference import f64

SMALL = [(33, 31, 64, "span"), (31, 31, 36, ""), (32, 32, 64, ""), (129, 65, 36, "")]      # the cases the seeded defects run on
IDS = lambda s: "U%d-S%d-d%d%s" % (s[0], s[1], s[2], "-" + s[3] if s[3] else "")


@pytest.mark.parametrize("spec", R.GPU_CASES, ids=IDS)
@pytest.mark.parametrize("exact", [False, True], ids=["real", "dyadic"])
def test_case_properties(spec, exact):
    nu, S, d, kind = spec
    case = R.cached_case(spec, exact)
    p = R.case_properties(case)
    assert (case.n_users, case.S, case.d) == (nu, S, d) and case.samples.shape == (nu, S) and R.supported(S, d)
    assert p["repeated"] and p["duplicate"]
    assert p["all_equal"] == (kind == "alleq" or S <= 2)
    if kind == "span":
        assert p["span"] == (2 * R.SPAN if S > 1 else 0.0)
    if case.planted:
        assert p["no_interaction"] and p["nonpositive"] and p["far_above"] >= R.FAR and p["far_below"] >= R.FAR
        assert p["sampled_positive"] or kind == "span"
    assert (case.row >= 0).all() and (case.row < case.n_items).all() and (case.x_item < case.n_items).all()
    if exact:
        assert R.scores_exact(case)
        ref = R.cached_ref(spec, True, True, 1.0, "plain")
        assert not ref.b_pred_serial.any()
    else:
        assert not R.scores_exact(case)


def test_cases_cover_every_edge():
    assert {s[0] for s in R.GPU_CASES} == {1, 31, 32, 33, 127, 128, 129, 300}
    assert {s[1] for s in R.GPU_CASES} == {1, 31, 32, 33, 64, 65, 257, 1000}
    assert {s[2] for s in R.GPU_CASES} == {4, 36, 64, 128}
    assert R.CORE in R.GPU_CASES and R.SLICED in R.GPU_CASES
    assert {R.options_of(i) for i in range(len(R.GPU_CASES))} >= {(True, 1.0, "plain"), (False, 1.0, "logq")}
    assert [R.slices(300, 65, 128, forced=n) for n in (1, 2, 3)] == [1, 2, 3] and 300 % 128 and 300 % 160   # ragged last slices


@pytest.mark.parametrize("variant", R.VARIANTS)
@pytest.mark.parametrize("biased", [False, True], ids=["nobias", "bias"])
def test_reference_gradients_are_central_differences(variant, biased):
    spec, T = (31, 31, 36, ""), 0.5
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

    touched = np.unique(np.concatenate([case.x_item, case.row]))
    for u in range(0, case.n_users, 3):
        c = int(rng.integers(case.d))
        assert abs(diff("U", (u, c)) - ref.dU[u, c]) <= 1e-6 * (1.0 + abs(ref.dU[u, c])), ("dU", u, c)
        if biased:
            assert abs(diff("ub", u) - ref.d_ub[u]) <= 1e-6 * (1.0 + np.abs(ref.g).max()), ("d_ub", u)
    for i in list(rng.choice(touched, size=8, replace=False)) + [int(case.row[0])]:
        c = int(rng.integers(case.d))
        assert abs(diff("V", (int(i), c)) - ref.dV[i, c]) <= 1e-6 * (1.0 + abs(ref.dV[i, c])), ("dV", i, c)
        if biased:
            assert abs(diff("ib", int(i)) - ref.d_ib[i]) <= 1e-6 * (1.0 + abs(ref.d_ib[i])), ("d_ib", i)
    assert not ref.dU[R.U_NONE].any() and not ref.b_dU[R.U_NONE].any() and not ref.d_ub[R.U_NONE] and not ref.b_d_ub[R.U_NONE]


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_shared_reference_equals_the_per_user_reference_on_the_repeated_table(variant):
    """the definition: the values are softmax_step_reference.ref_step's on a table whose rows all equal the shared row, exactly"""
    case = R.cached_case(R.CORE, False)
    assert (case.samples == case.row[None, :]).all()
    mine, theirs = R.ref_step(case, True, 0.25, variant), SR.ref_step(case, True, 0.25, variant)
    for name in R.OUTPUTS:
        assert np.array_equal(getattr(mine, name), getattr(theirs, name)), name


@pytest.mark.parametrize("spec", R.GPU_CASES, ids=IDS)
def test_float32_restatement_lies_inside_the_bars(spec):
    """both summation orders, both families, the options the GPU test runs on the case"""
    k = R.GPU_CASES.index(spec)
    combos = R.ALL_OPTIONS if spec == R.CORE else [R.options_of(k)]
    for exact in (False, True):
        case = R.cached_case(spec, exact)
        for biased, T, variant in combos:
            ref = R.cached_ref(spec, exact, biased, T, variant)
            for order, n_slices in (("natural", 1), ("paired", 3 if spec == R.SLICED else 2)):
                got = R.restate_f32(case, biased, T, variant, order, n_slices=n_slices)
                r = R.ratios(got, ref, biased)
                assert max(r.values()) <= 1.0, (spec, exact, biased, T, variant, order, r)
                if exact:
                    assert np.array_equal(got.pred_serial.astype(np.float64), ref.pred_serial)


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_seeded_defects_leave_the_bars(defect):
    worst = 0.0
    for spec in SMALL:
        case = R.cached_case(spec, False)
        for variant in ("plain", "logq"):
            for T in R.TEMPERATURES:
                ref = R.cached_ref(spec, False, True, T, variant)
                r = R.ratios(R.restate_f32(case, True, T, variant, "paired", defect=defect), ref, True)
                worst = max(worst, max(r.values()))
    assert worst > 1.0, (defect, worst)


def test_constructor_validation_and_old_pickles():
    from tensorrec_amd.loss_graphs import SampledSoftmaxLossGraph
    assert SampledSoftmaxLossGraph().shared_negatives is False and SampledSoftmaxLossGraph.shared_negatives is False
    g = SampledSoftmaxLossGraph(temperature=0.5, shared_negatives=True)
    assert g.shared_negatives is True and g.wants_sample_items is False and g.is_sample_based
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError, match="shared_negatives must be a bool"):
            SampledSoftmaxLossGraph(shared_negatives=bad)
    old = SampledSoftmaxLossGraph(temperature=0.5, log_q_correction=True)
    del old.__dict__["shared_negatives"]                            # a model pickled before the option existed
    back = pickle.loads(pickle.dumps(old))
    assert "shared_negatives" not in back.__dict__ and back.shared_negatives is False and back.log_q_correction is True


def test_coverage_mirror_and_abi_argument_checks():
    from tensorrec_amd import _native
    lib = _native.load()
    for S in (0, 1, 65, 4096):
        for d in (0, 2, 4, 6, 36, 64, 128, 132, 256):
            assert bool(lib.trec_softmax_shared_supported(S, d)) == R.supported(S, d), (S, d)
    for S, d in R.UNCOVERED:
        assert not R.supported(S, d)
    lib.trec_clear_tuning(b"softmax_shared_slices")
    for nu, S, d in ((300, 65, 128), (1, 1, 4), (1000000, 4096, 128), (100000, 1024, 128), (129, 257, 36)):
        assert lib.trec_softmax_shared_slices(nu, S, d) == R.slices(nu, S, d), (nu, S, d)
    try:
        for n in (1, 2, 3):
            lib.trec_set_tuning(b"softmax_shared_slices", n)
            assert lib.trec_softmax_shared_slices(300, 65, 128) == R.slices(300, 65, 128, forced=n) == n
    finally:
        lib.trec_clear_tuning(b"softmax_shared_slices")
    assert lib.trec_softmax_shared_slices(300, 65, 132) == -1
    p, f = ctypes.c_void_p(8), ctypes.c_float
    stats = lambda *a: lib.trec_softmax_shared_stats(*a, None)
    assert stats(None, p, None, None, None, 10, 5, 64, f(1.0), p, p) == 1 and b"null pointer" in lib.trec_last_error()
    assert stats(p, p, None, None, None, 10, 0, 64, f(1.0), p, p) == 1 and b"n_sampled" in lib.trec_last_error()
    assert stats(p, p, None, None, None, 10, 5, 132, f(1.0), p, p) == 1 and b"4 <= d <= 128" in lib.trec_last_error()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert stats(p, p, None, None, None, 10, 5, 64, f(bad), p, p) == 1 and b"inv_temperature" in lib.trec_last_error()
        assert lib.trec_softmax_shared_positives(p, p, p, p, p, 10, f(bad), p, p, p, None, None) == 1
        assert lib.trec_softmax_shared_grads(p, p, None, None, None, p, p, 10, 5, 64, f(bad), 1, None, p, p, None, None) == 1
    grads = lambda *a: lib.trec_softmax_shared_grads(*a, None)
    assert grads(p, p, None, None, None, p, None, 10, 5, 64, f(1.0), 1, None, p, p, None) == 1 and b"null pointer" in lib.trec_last_error()
    assert grads(p, p, None, None, None, p, p, 10, 0, 64, f(1.0), 1, None, p, p, None) == 1
    assert grads(p, p, None, None, None, p, p, 10, 5, 6, f(1.0), 1, None, p, p, None) == 1
    assert grads(p, p, None, None, None, p, p, 10, 5, 64, f(1.0), 7, None, p, p, None) == 1 and b"n_slices" in lib.trec_last_error()
    assert lib.trec_softmax_shared_positives(None, p, p, p, p, 10, f(1.0), p, p, p, None, None) == 1
    assert lib.trec_softmax_shared_scatter(None, p, p, None, 5, 64, 10, p, None, None) == 1
    assert lib.trec_softmax_shared_scatter(p, p, p, None, 0, 64, 10, p, None, None) == 1
