"""tests/softmax_full_reference.py checked on the CPU: the float64 gradients are central differences of the loss, a row shift moves
nothing beyond the bars, the float32 restatements (natural order and the kernels' orders) lie inside the bars on every GPU case,
seeded defects land outside; the loss class's constructor and the argument checks of the new entry points."""
import ctypes

import numpy as np
import pytest

import softmax_full_reference as R
from pair_reference import f64

TREC_ERR_INVALID = 1          # include/tensorrec_hip.h
SMALL = (33, 33, 36)


def small_case():
    return R.full_case(*SMALL)


# ------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("temperature", R.TEMPERATURES)
def test_step_gradients_are_central_differences(temperature):
    case = small_case()
    ref = R.ref_step(case, True, temperature)
    rng = np.random.default_rng(1)
    h = 1e-6
    for name, table, grad in (("U", case.U, ref.dU), ("V", case.V, ref.dV), ("ub", case.ub, ref.d_ub), ("ib", case.ib, ref.d_ib)):
        for _ in range(6):
            at = tuple(int(rng.integers(0, s)) for s in table.shape)
            up, dn = f64(table).copy(), f64(table).copy()
            up[at] += h
            dn[at] -= h
            fd = (R.loss_sum(case, True, temperature, **{name: up}) - R.loss_sum(case, True, temperature, **{name: dn})) / (2 * h)
            assert abs(fd - grad[at]) <= 1e-6 * max(1.0, abs(grad[at])) + 1e-5, (name, at, fd, grad[at])
    assert not ref.d_ub.any()                                        # the loss does not move with a shift of the row


def test_dense_gradients_are_central_differences():
    case = R.dense_case(9, 65)
    ref = R.ref_dense(case.pred, case, case.go, 0.25)
    rng = np.random.default_rng(2)
    h = 1e-6
    cells = [(int(rng.integers(0, 9)), int(rng.integers(0, 65))) for _ in range(12)]
    cells += [(int(u), int(i)) for u, i in zip(case.xu[::3], case.x_item[::3])][:20]        # cells that hold positives, duplicates
    for at in cells:
        up, dn = f64(case.pred).copy(), f64(case.pred).copy()
        up[at] += h
        dn[at] -= h
        fd = (R.dense_loss_sum(up, case, case.go, 0.25) - R.dense_loss_sum(dn, case, case.go, 0.25)) / (2 * h)
        assert abs(fd - ref.d_pred[at]) <= 1e-6 * max(1.0, abs(ref.d_pred[at])) + 1e-5, (at, fd, ref.d_pred[at])
    want = R.dense_loss_sum(f64(case.pred), case, case.go, 0.25)
    assert abs(float((f64(case.go) * ref.loss).sum()) - want) <= 1e-9 * max(1.0, abs(want))


def test_row_shift_changes_nothing_within_the_bars():
    case = R.dense_case(9, 257)
    ref = R.ref_dense(case.pred, case, case.go, 1.0)
    shifted = R.ref_dense(f64(case.pred) + 3.0, case, case.go, 1.0)
    assert (np.abs(shifted.loss - ref.loss) <= ref.b_loss).all() and (np.abs(shifted.d_pred - ref.d_pred) <= ref.b_d_pred).all()
    step = small_case()
    a = R.ref_step(step, True, 0.25)
    moved = R.full_case(*SMALL)
    moved.ub = (moved.ub + np.float32(2.0)).astype(np.float32)
    b = R.ref_step(moved, True, 0.25)
    for name in ("loss", "dU", "dV", "d_ib"):
        assert (np.abs(getattr(a, name) - getattr(b, name)) <= getattr(a, "b_" + name) + getattr(b, "b_" + name)).all(), name


def test_planted_rows_hold_what_they_are_meant_to():
    for spec in ((300, 1000, 36), (33, 33, 128)):
        for exact in (False, True):
            p = R.case_properties(R.cached_case(spec, exact))
            assert p["no_interaction"] and p["nonpositive"] and p["every_item"] and p["duplicates"] and p["all_equal"]
            assert p["far_biased"] > 90.0 and p["far_plain"] > 90.0 and p["span"] >= 2 * R.SPAN - 0.25
    c = R.cached_dense_case((300, 257))
    row = f64(c.pred)
    assert (row[R.U_EQUAL] == row[R.U_EQUAL, 0]).all() and row[R.U_SPAN].max() - row[R.U_SPAN].min() == 2 * R.SPAN
    assert np.sort(row[R.U_FAR])[-1] - np.sort(row[R.U_FAR])[-2] >= R.FAR - 1e-3
    assert (c.go > 0).any() and (c.go < 0).any()


# ------------------------------------------------------------------------------------------------ restatements inside the bars
@pytest.mark.parametrize("spec", R.GPU_CASES, ids=str)
def test_step_restatements_lie_inside_the_bars(spec):
    k = R.GPU_CASES.index(spec)
    biased, T = R.options_of(k)
    for exact in (False, True):
        case, ref = R.cached_case(spec, exact), R.cached_ref(spec, exact, biased, T)
        for order in ("natural", "paired"):
            got = R.restate_step_f32(case, biased, T, order=order)
            rat = R.ratios(got, ref, biased)
            assert max(rat.values()) <= 1.0, (spec, exact, order, rat)
            if exact:
                assert np.array_equal(got.pred_serial.astype(np.float64), ref.pred_serial)


@pytest.mark.parametrize("spec", R.LONG_CASES, ids=str)
def test_long_rows_and_columns(spec):
    """the cases that send the positives through the chunked gathers are what they say, and their restatement lies inside the bars"""
    case, ref = R.cached_case(spec, False), R.cached_ref(spec, False, True, 0.25)
    longest_row, longest_col = int(np.diff(case.indptr).max()), int(np.bincount(case.x_item).max())
    assert (longest_col if spec[3] == "popular" else longest_row) > R.SPLIT_T
    rat = R.ratios(R.restate_step_f32(case, True, 0.25, order="paired"), ref, True)
    assert max(rat.values()) <= 1.0, rat


@pytest.mark.parametrize("n_slices", [2, 3])
def test_sliced_restatement_lies_inside_the_bars(n_slices):
    case, ref = R.cached_case(R.SLICED, False), R.cached_ref(R.SLICED, False, True, 0.25)
    rat = R.ratios(R.restate_step_f32(case, True, 0.25, order="paired", n_slices=n_slices), ref, True)
    assert max(rat.values()) <= 1.0, rat


@pytest.mark.parametrize("spec", R.DENSE_CASES, ids=str)
def test_dense_restatements_lie_inside_the_bars(spec):
    case = R.cached_dense_case(spec)
    for T in R.TEMPERATURES:
        ref = R.cached_dense_ref(spec, T)
        for order in ("natural", "threads"):
            got = R.restate_dense_f32(case.pred, case, case.go, T, order=order)
            for name in ("loss", "d_pred"):
                err = np.abs(f64(getattr(got, name)) - getattr(ref, name))
                assert (err <= getattr(ref, "b_" + name)).all(), (spec, T, order, name)
            no = [u for u in range(case.n_users) if not (case.values[case.indptr[u]:case.indptr[u + 1]] > 0).any()]
            assert not got.d_pred[no].any() and not ref.d_pred[no].any() and not ref.b_d_pred[no].any()


# ------------------------------------------------------------------------------------------------ seeded defects outside the bars
@pytest.mark.parametrize("defect", R.DEFECTS)
def test_seeded_defects_land_outside_the_step_bars(defect):
    spec = (33, 33, 36)                                              # 33 items: one ragged tile; planted rows; T = 0.25, biases
    case, ref = R.cached_case(spec, False), R.cached_ref(spec, False, True, 0.25)
    clean = R.ratios(R.restate_step_f32(case, True, 0.25, order="paired"), ref, True)
    assert max(clean.values()) <= 1.0
    rat = R.ratios(R.restate_step_f32(case, True, 0.25, order="paired", defect=defect), ref, True)
    assert max(rat.values()) > 1.0, (defect, rat)


@pytest.mark.parametrize("defect", ["positives_dropped", "count_ignored", "no_t", "no_rescale", "duplicates_once"])
def test_seeded_defects_land_outside_the_dense_bars(defect):
    spec = (300, 257)
    case, ref = R.cached_dense_case(spec), R.cached_dense_ref(spec, 0.25)
    got = R.restate_dense_f32(case.pred, case, case.go, 0.25, order="threads", defect=defect)
    with np.errstate(invalid="ignore"):
        outside = (~(np.abs(f64(got.d_pred) - ref.d_pred) <= ref.b_d_pred)).any() or (~(np.abs(f64(got.loss) - ref.loss) <= ref.b_loss)).any()
    assert outside, defect


# ------------------------------------------------------------------------------------------------ the class and the ABI
def test_constructor_checks():
    from tensorrec_amd.loss_graphs import SoftmaxDenseLossGraph, SampledSoftmaxLossGraph
    g = SoftmaxDenseLossGraph()
    assert g.is_dense and not g.is_sample_based and g.temperature == 1.0
    assert SoftmaxDenseLossGraph(temperature="0.5").temperature == 0.5
    for bad in (0, 0.0, -1.0, float("inf"), float("nan"), None, "x", [1.0]):
        with pytest.raises(ValueError, match="temperature"):
            SoftmaxDenseLossGraph(temperature=bad)
        with pytest.raises(ValueError, match="temperature"):
            SampledSoftmaxLossGraph(temperature=bad)                 # validated exactly alike


def test_abi_argument_checks():
    from tensorrec_amd import _native
    lib = _native.load()
    p = ctypes.c_void_p(64)
    inf = float("inf")
    ok_f = (p, 8, p, p, p, 1, 8, 1.0, p, p, p, None)
    assert lib.trec_softmax_dense_fwd(None, 8, p, p, p, 1, 8, 1.0, p, p, p, None) == TREC_ERR_INVALID
    assert b"null pointer" in lib.trec_last_error()
    for k in (2, 3, 4, 8, 9, 10):
        args = list(ok_f)
        args[k] = None
        assert lib.trec_softmax_dense_fwd(*args) == TREC_ERR_INVALID, k
    for t in (0.0, -1.0, inf, float("nan")):
        assert lib.trec_softmax_dense_fwd(p, 8, p, p, p, 1, 8, t, p, p, p, None) == TREC_ERR_INVALID
        assert b"inv_temperature" in lib.trec_last_error()
        assert lib.trec_softmax_dense_bwd(p, 8, p, p, p, p, p, p, 1, 8, t, p, None) == TREC_ERR_INVALID
        assert lib.trec_softmax_full_positives(p, p, p, p, p, 1, t, p, p, p, p, None) == TREC_ERR_INVALID
    assert lib.trec_softmax_dense_fwd(p, 7, p, p, p, 1, 8, 1.0, p, p, p, None) == TREC_ERR_INVALID           # ld < n_items
    assert lib.trec_softmax_dense_fwd(p, 8, p, p, p, 1, 0, 1.0, p, p, p, None) == TREC_ERR_INVALID           # no items
    assert lib.trec_softmax_dense_bwd(p, 7, p, p, p, p, p, p, 1, 8, 1.0, p, None) == TREC_ERR_INVALID
    for k in (0, 2, 3, 4, 5, 6, 7, 11):
        args = [p, 8, p, p, p, p, p, p, 1, 8, 1.0, p, None]
        args[k] = None
        assert lib.trec_softmax_dense_bwd(*args) == TREC_ERR_INVALID, k
    for k in (0, 3, 4, 9):
        args = [p, p, p, p, p, 1, 1.0, p, p, p, p, None]
        args[k] = None
        assert lib.trec_softmax_full_positives(*args) == TREC_ERR_INVALID, k
    assert lib.trec_softmax_full_positives(p, p, p, p, p, -1, 1.0, p, p, p, p, None) == TREC_ERR_INVALID
    # nothing to do: no launch, no error
    assert lib.trec_softmax_dense_fwd(p, 8, p, p, p, 0, 8, 1.0, p, p, p, None) == 0
    assert lib.trec_softmax_dense_bwd(p, 8, p, p, p, p, p, p, 0, 8, 1.0, p, None) == 0
    assert lib.trec_softmax_full_positives(p, p, p, p, p, 0, 1.0, p, p, p, p, None) == 0
