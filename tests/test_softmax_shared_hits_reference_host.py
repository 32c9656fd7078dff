"""tests/softmax_shared_hits_reference.py on the CPU: the float64 step's gradients are central differences of its loss; the reference IS
the per-user reference with hits removed on the repeated table; a float32 restatement of the masked kernels' arithmetic
(csrc/softmax_shared.hip, sorted column order) lies inside the bars on every case the GPU test runs; each seeded defect leaves them;
the host mirrors of the hit ranges and of the transposed positives; step_plan.softmax_shared_hits_kernel's table with every fallback,
step_plan.kernel unchanged beside it; the ABI's argument checks."""
import ctypes

import numpy as np
import pytest

import softmax_shared_hits_reference as H
import softmax_step_reference as SR
from pair_reference import f64

SMALL = [(31, 31, 36, ""), (33, 33, 128, ""), (129, 65, 36, "")]      # the cases the seeded defects run on
IDS = lambda s: "U%d-S%d-d%d%s" % (s[0], s[1], s[2], "-" + s[3] if s[3] else "")


def test_cases_cover_every_edge():
    assert {s[0] for s in H.GPU_CASES} == {1, 31, 33, 129, 300}
    assert {s[1] for s in H.GPU_CASES} == {1, 31, 32, 33, 65, 1000}
    assert {s[2] for s in H.GPU_CASES} == {4, 36, 64, 128}
    assert all(c in H.GPU_CASES for c in (H.CORE, H.SLICED, H.NOHITS, H.EVERYONE))
    assert [H.slices(300, 65, 128, forced=n) for n in (1, 2, 3)] == [1, 2, 3]
    # 300 users: 2 slices of 160, 3 slices of 128 -- the planted users sit on both sides of every boundary
    assert set(H.BOUNDARY_USERS) == {127, 128, 159, 160, 255, 256}
    assert {H.options_of(i) for i in range(len(H.GPU_CASES))} >= {(True, 1.0, "plain"), (False, 1.0, "logq")}


@pytest.mark.parametrize("spec", H.GPU_CASES, ids=IDS)
@pytest.mark.parametrize("exact", [False, True], ids=["real", "dyadic"])
def test_case_properties(spec, exact):
    nu, S, d, kind = spec
    case = H.cached_case(spec, exact)
    p = H.case_properties(case)
    assert (case.n_users, case.S, case.d) == (nu, S, d) and (case.samples == case.row[None, :]).all() and H.supported(S, d)
    assert (case.row >= 0).all() and (case.row < case.n_items).all() and (case.x_item < case.n_items).all()
    for u in range(nu):                                              # CSR rows ascending without repeats: the ranges' premise
        assert (np.diff(case.x_item[case.indptr[u]:case.indptr[u + 1]]) > 0).all()
    assert p["run"] == (S >= 33)
    if kind == "nohits":
        assert not p["any_hit"] and H.hit_mask(case, True).any()     # matches of value <= 0 remain: nothing is masked for them
        return
    assert p["any_hit"]
    if nu == 1:
        assert p["all_hit_users"] == ([0] if S == 1 else [])
    if nu >= 31:
        assert p["col0"] and p["last"] and p["partial"] and p["run_hit"] and p["all"] and p["nonpos_match"]
        assert (H.U_ALL in p["all_hit_users"]) == (S <= 65) and p["users_without_positives"] >= (0 if kind == "everyone" else 1)
    if nu >= 300:
        assert p["boundaries"]
    if kind == "everyone":
        assert len(p["everyone"]) >= 1 and p["users_without_positives"] == 0
    if exact:
        assert H.scores_exact(case)
    assert spec != (33, 33, 128, "") or H.U_ALL in p["all_hit_users"]     # all hits at S = 33; at S = 1 above (one user)


@pytest.mark.parametrize("variant", H.VARIANTS)
@pytest.mark.parametrize("biased", [False, True], ids=["nobias", "bias"])
def test_reference_gradients_are_central_differences(variant, biased):
    spec, T = (31, 31, 36, ""), 0.5
    case = H.cached_case(spec, False)
    ref = H.ref_step(case, biased, T, variant)
    h = 1e-6
    rng = np.random.default_rng(3)
    U, V, ub, ib = f64(case.U), f64(case.V), f64(case.ub), f64(case.ib)

    def diff(name, index):
        out = []
        for sign in (1.0, -1.0):
            t = dict(U=U.copy(), V=V.copy(), ub=ub.copy(), ib=ib.copy())
            t[name][index] += sign * h
            out.append(H.loss_sum(case, biased, T, variant, **t))
        return (out[0] - out[1]) / (2.0 * h)

    touched = np.unique(np.concatenate([case.x_item, case.row]))
    for u in list(range(0, case.n_users, 3)) + [H.U_ALL, H.U_COL0, H.U_NONPOS_MATCH]:
        c = int(rng.integers(case.d))
        assert abs(diff("U", (u, c)) - ref.dU[u, c]) <= 1e-6 * (1.0 + abs(ref.dU[u, c])), ("dU", u, c)
        if biased:
            assert abs(diff("ub", u) - ref.d_ub[u]) <= 1e-6 * (1.0 + np.abs(ref.g).max()), ("d_ub", u)
    for i in list(rng.choice(touched, size=8, replace=False)) + [int(np.sort(case.row)[0]), int(np.sort(case.row)[-1])]:
        c = int(rng.integers(case.d))
        assert abs(diff("V", (int(i), c)) - ref.dV[i, c]) <= 1e-6 * (1.0 + abs(ref.dV[i, c])), ("dV", i, c)
        if biased:
            assert abs(diff("ib", int(i)) - ref.d_ib[i]) <= 1e-6 * (1.0 + abs(ref.d_ib[i])), ("d_ib", i)
    # the user whose samples are all hits: loss 0, no gradient at all, bars of 0
    b, e = case.indptr[H.U_ALL], case.indptr[H.U_ALL + 1]
    slots = (np.cumsum(case.values > 0) - 1)[b:e][case.values[b:e] > 0]
    assert not ref.loss[slots].any() and not ref.b_loss[slots].any()
    assert not ref.dU[H.U_ALL].any() and not ref.b_dU[H.U_ALL].any() and not ref.d_ub[H.U_ALL] and not ref.b_d_ub[H.U_ALL]


@pytest.mark.parametrize("variant", H.VARIANTS)
def test_reference_equals_the_per_user_reference_on_the_repeated_table(variant):
    """the definition: the values are softmax_step_reference.ref_step's, hits removed, on a table whose rows all equal the shared row"""
    case = H.cached_case(H.CORE, False)
    assert (case.samples == case.row[None, :]).all()
    mine, theirs = H.ref_step(case, True, 0.25, variant), SR.ref_step(case, True, 0.25, H.STEP_VARIANT[variant])
    for name in H.OUTPUTS:
        assert np.array_equal(getattr(mine, name), getattr(theirs, name)), name
    assert mine.hits.any() and not mine.g[case.x_item.size:][mine.hits.reshape(-1)].any()
    assert not mine.b_g[case.x_item.size:][mine.hits.reshape(-1)].any()


@pytest.mark.parametrize("spec", H.GPU_CASES, ids=IDS)
def test_float32_restatement_lies_inside_the_bars(spec):
    """both families, the options the GPU test runs on the case, one slice and several"""
    k = H.GPU_CASES.index(spec)
    combos = H.ALL_OPTIONS if spec == H.CORE else [H.options_of(k)]
    big = spec[0] * spec[1] > 50000
    for exact in ((False,) if big else (False, True)):
        case = H.cached_case(spec, exact)
        for biased, T, variant in combos:
            ref = H.cached_ref(spec, exact, biased, T, variant)
            for n_slices in ((3,) if big or spec == H.CORE else (1, 3 if spec == H.SLICED else 2)):
                got = H.restate_f32(case, biased, T, variant, n_slices=n_slices)
                r = H.ratios(got, ref, biased)
                assert max(r.values()) <= 1.0, (spec, exact, biased, T, variant, n_slices, r)
                assert np.isfinite(got.loss).all() and np.isfinite(got.dU).all() and np.isfinite(got.dV).all()
                assert not got.dVs[got.hit.all(0)].any() and not got.dbs[got.hit.all(0)].any()
                if exact:
                    assert np.array_equal(got.pred_serial.astype(np.float64), ref.pred_serial)


@pytest.mark.parametrize("defect", H.DEFECTS)
def test_seeded_defects_leave_the_bars(defect):
    worst = 0.0
    for spec in SMALL:
        case = H.cached_case(spec, False)
        for variant in ("plain", "logq"):
            for T in H.TEMPERATURES:
                ref = H.cached_ref(spec, False, True, T, variant)
                r = H.ratios(H.restate_f32(case, True, T, variant, n_slices=2, defect=defect), ref, True)
                worst = max(worst, max(r.values()))
    assert worst > 1.0, (defect, worst)


@pytest.mark.parametrize("spec", H.GPU_CASES, ids=IDS)
def test_host_mirrors(spec):
    """the ranges are ascending, disjoint, and OR to the hit mask in sorted column order; the transposed lists are ascending and hold
    exactly the pairs of value > 0"""
    case = H.cached_case(spec, False)
    order = np.argsort(case.row, kind="stable")
    hs = H.hit_mask(case)[:, order]
    rng, cnt = H.hit_ranges(case)
    for u in range(case.n_users):
        mask = np.zeros(case.S, bool)
        assert rng[u].shape == (cnt[u], 2) and (rng[u][:, 0] < rng[u][:, 1]).all() and (rng[u][1:, 0] >= rng[u][:-1, 1]).all()
        for lo, hi in rng[u]:
            mask[lo:hi] = True
        assert np.array_equal(mask, hs[u]), u
    indptr_tp, users_tp = H.transposed_positive(case)
    assert indptr_tp[-1] == int((case.values > 0).sum()) and indptr_tp.size == case.n_items + 1
    dense = np.zeros((case.n_users, case.n_items), bool)
    xu = np.repeat(np.arange(case.n_users), np.diff(case.indptr))
    dense[xu[case.values > 0], case.x_item[case.values > 0]] = True
    for i in range(case.n_items):
        mine = users_tp[indptr_tp[i]:indptr_tp[i + 1]]
        assert (np.diff(mine) > 0).all() and np.array_equal(mine, np.flatnonzero(dense[:, i])), i


# ------------------------------------------------------------------------------------------------ the route table
def test_hits_kernel_table_with_every_fallback():
    from tensorrec_amd import ops, step_plan, _native
    _native.clear_tuning("softmax_shared_hits")
    _native.clear_tuning("softmax_shared")
    assert ops.SOFTMAX_SHARED_HITS_DEFAULT == 0 and not ops.step_switch("softmax_shared_hits")
    base = dict(loss="sampled_softmax", engine=True, engine_mode=ops.MODE_DOT, multi=False, same_width=True, n_sampled=1024, d=128,
                shared_negatives=True, remove_accidental_hits=True)
    ask = lambda switch=True, **kw: step_plan.softmax_shared_hits_kernel(**dict(base, **kw), switch=switch)
    assert ask() == "softmax_shared_hits"
    assert ask(switch=None) is None and ask(switch=False) is None              # the default is off
    for change in (dict(loss=None), dict(loss="wmrb"), dict(loss="warp"), dict(engine=False), dict(engine_mode=ops.MODE_EUCLIDEAN),
                   dict(engine_mode=None), dict(multi=True), dict(same_width=False), dict(n_sampled=None), dict(shared_negatives=False),
                   dict(remove_accidental_hits=False), dict(d=132), dict(d=6), dict(d=256), dict(n_sampled=0)):
        assert ask(**change) is None, change
    for d in (4, 36, 64, 128):
        for S in (1, 65, 4096):
            assert ask(d=d, n_sampled=S) == "softmax_shared_hits" and ops.step_covers("softmax_shared_hits", S, 0, d)
    try:
        _native.set_tuning("softmax_shared_hits", 1)
        assert ask(switch=None) == "softmax_shared_hits"
        _native.set_tuning("softmax_shared", 0)                                # the MFMA route as such switched off
        assert ask(switch=None) is None and ask() is None
    finally:
        _native.clear_tuning("softmax_shared_hits")
        _native.clear_tuning("softmax_shared")

    from tensorrec_amd.loss_graphs import SampledSoftmaxLossGraph

    class Sub(SampledSoftmaxLossGraph):
        pass
    assert step_plan.loss_kind(Sub()) is None and step_plan.loss_kind(SampledSoftmaxLossGraph()) == "sampled_softmax"


def test_step_plan_kernel_answers_as_before():
    """hits removed on a shared row: ``kernel`` says None whatever the new tuning says; hits kept: "softmax_shared" as ever"""
    from tensorrec_amd import ops, step_plan, _native
    sw = step_plan.Switches(True, True, True, True, True)
    assert step_plan.Switches._fields == ("wmrb_fused", "wmrb_tiled", "softmax_fused", "softmax_shared", "fit_step_coop")
    args = ("sampled_softmax", True, ops.MODE_DOT, False, True, 1024, 8, 128)
    try:
        for tuning in (None, 0, 1):
            if tuning is not None:
                _native.set_tuning("softmax_shared_hits", tuning)
            assert step_plan.kernel(*args, True, True, switches=sw) is None
            assert step_plan.kernel(*args, True, False, switches=sw) == "softmax_shared"
            assert step_plan.kernel(*args[:5], 20, 8, 64, False, True, switches=sw) == "softmax_fused"
            assert step_plan.kernel(*args, True, True) is None
    finally:
        _native.clear_tuning("softmax_shared_hits")


def test_abi_argument_checks():
    from tensorrec_amd import _native
    lib = _native.load()
    p, f = ctypes.c_void_p(8), ctypes.c_float
    rng = lambda *a: lib.trec_softmax_shared_hit_ranges(*a, None)
    assert rng(None, p, p, p, 10, 5, p, p) == 1 and b"null pointer" in lib.trec_last_error()
    assert rng(p, p, p, p, 10, 5, None, p) == 1 and rng(p, p, p, p, 10, 0, p, p) == 1
    assert rng(p, p, p, p, 0, 5, p, p) == 0                                    # no users: nothing launched
    stats = lambda *a: lib.trec_softmax_shared_hits_stats(*a, None)
    ok = (p, p, None, None, None, p, p, p)
    assert stats(None, p, None, None, None, p, p, p, 10, 5, 64, f(1.0), p, p) == 1 and b"null pointer" in lib.trec_last_error()
    assert stats(p, p, None, None, None, p, None, p, 10, 5, 64, f(1.0), p, p) == 1 and b"null pointer" in lib.trec_last_error()
    assert stats(*ok, 10, 0, 64, f(1.0), p, p) == 1 and b"n_sampled" in lib.trec_last_error()
    for d in (132, 6, 2, 256):
        assert stats(*ok, 10, 5, d, f(1.0), p, p) == 1 and b"4 <= d <= 128" in lib.trec_last_error()
    assert stats(*ok, 0, 5, 64, f(1.0), p, p) == 0
    grads = lambda *a: lib.trec_softmax_shared_hits_grads(*a, None)
    head, lists = (p, p, None, None, None, p, p), (p, p, p, p, p, p)
    assert grads(*head, *lists, 20, 10, 5, 64, f(1.0), 1, None, p, None, None) == 1 and b"null pointer" in lib.trec_last_error()
    for k in range(6):
        broken = tuple(None if j == k else p for j in range(6))
        assert grads(*head, *broken, 20, 10, 5, 64, f(1.0), 1, None, p, p, None) == 1 and b"null pointer" in lib.trec_last_error()
    assert grads(*head, *lists, 20, 10, 5, 132, f(1.0), 1, None, p, p, None) == 1
    assert grads(*head, *lists, 20, 10, 5, 64, f(1.0), 7, None, p, p, None) == 1 and b"n_slices" in lib.trec_last_error()
    assert grads(*head, *lists, 20, 0, 5, 64, f(1.0), 1, None, p, p, None) == 0
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert stats(*ok, 10, 5, 64, f(bad), p, p) == 1 and b"inv_temperature" in lib.trec_last_error()
        assert grads(*head, *lists, 20, 10, 5, 64, f(bad), 1, None, p, p, None) == 1 and b"inv_temperature" in lib.trec_last_error()
