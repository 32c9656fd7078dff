"""The float64 references and the bars of tests/pair_reference.py, checked without the code under test: every chain is restated in
np.float32 in two orders -- sequential, and a 64-way split followed by a tree -- and each restatement has to lie within its bar of the
float64 reference at every shape tests/test_gpu_pair_kernels.py uses.  A bar that a legitimate float32 evaluation order misses is too
tight; the inputs are also checked to hold the cases they are meant to hold (clamped pairs, hinges of exactly 0, long items, ...), so
that a case cannot vanish silently."""
import numpy as np
import pytest

import pair_reference as R
from pair_reference import MODE_DOT, MODE_EUCLID, f64

F = np.float32


def fma32(a, b, c):
    """fmaf: the product of two float32 is exact in float64; one rounding of the sum (to float64 first: a restatement, not the bits)"""
    return (f64(a) * f64(b) + f64(c)).astype(F)


def tree64(lanes):
    """[n, 64, ...] lane sums -> [n, ...]: the xor butterfly's additions"""
    off = 32
    while off:
        lanes = lanes[:, :off] + lanes[:, off:2 * off]
        off >>= 1
    return lanes[:, 0]


def chain32(x, y, mode, order):
    """sum_c x_c y_c or sum_c (x_c - y_c)^2 over float32 rows, one fmaf per term"""
    n, d = x.shape
    if mode == MODE_EUCLID:
        x = y = (x - y).astype(F)
    if order == "seq":
        acc = np.zeros(n, F)
        for c in range(d):
            acc = fma32(x[:, c], y[:, c], acc)
        return acc
    lanes = np.zeros((n, 64), F)
    for c in range(d):
        lanes[:, c % 64] = fma32(x[:, c], y[:, c], lanes[:, c % 64])
    return tree64(lanes)


def check_forward_case(case, d):
    """the restatements run on the first and the last 4,096 pairs and on every clamped one (the chains do not depend on the pair count)"""
    assert case.U.dtype == F and case.V.dtype == F
    clamped = R.clamped_pairs(case)
    assert clamped.sum() >= 2 and clamped[-1], "the clamped pairs are gone (one of them sits in the last pair)"
    n = case.xi.size
    sel = np.unique(np.concatenate([np.arange(4096), np.arange(n - 4096, n), np.nonzero(clamped)[0]]))
    xu, xi, clamped = case.xu[sel], case.xi[sel], clamped[sel]
    for mode in (MODE_DOT, MODE_EUCLID):
        accs = {order: chain32(case.U[xu], case.V[xi], mode, order) for order in ("seq", "split64")}
        for with_bias in (False, True):
            ref = R.ref_pair_scores(case.U, case.V, xu, xi, mode, case.ub if with_bias else None, case.ib if with_bias else None)
            if mode == MODE_EUCLID:
                assert (ref.mag[clamped] < R.EPS).all() and (ref.raw[clamped] == -1e-8).all()
                assert (ref.mag[~clamped] > 1e-3).all()                        # nothing near the threshold: the clamp is decided alike
            bar, cbar = R.score_bar(ref, d), R.chain_bar(ref, d)
            for order, acc in accs.items():
                s = acc if mode == MODE_DOT else -np.sqrt(np.maximum(acc, F(1e-16)))
                if with_bias:
                    s = (s + case.ub[xu]).astype(F)
                    s = (s + case.ib[xi]).astype(F)
                assert (np.abs(f64(acc) - (ref.mag if mode == MODE_EUCLID else ref.raw)) <= cbar).all(), (d, mode, order)
                err = np.abs(f64(s) - ref.scores)
                assert (err <= bar).all(), "d %d mode %d bias %d %s: worst ratio %.2f" % (d, mode, with_bias, order, (err / bar).max())


@pytest.mark.parametrize("d", R.FWD_D)
def test_forward_bars_hold_for_float32_restatements(d):
    for n_pairs in R.FWD_N_PAIRS:
        check_forward_case(R.fwd_explicit_case(d, n_pairs), d)
    for ppu in R.FWD_PPU:
        check_forward_case(R.fwd_implicit_case(d, ppu), d)


def test_forward_cases_reach_every_instantiation():
    """the dispatcher of trec_pair_score_fwd restated (pair_reference.fwd_instantiation): the grid of the GPU test launches all seven
    <VEC, PP, UG> -- <1, 2> included: d = 5 or 67 with 65,536 pairs or more"""
    reached = {}
    for d in R.FWD_D:
        for pp, ug in [(None, 1)] + R.FWD_TUNINGS:
            for n in R.FWD_N_PAIRS:
                reached.setdefault(R.fwd_instantiation(d, n, 0, pp, ug), ("explicit", d, n, pp, ug))
            for ppu in R.FWD_PPU:
                reached.setdefault(R.fwd_instantiation(d, R.FWD_IMPLICIT_USERS * ppu, ppu, pp, ug), ("implicit", d, ppu, pp, ug))
    assert set(reached) == R.ALL_FWD_INSTANTIATIONS, reached
    # the defaults (no tuning set) the issue names
    assert [R.fwd_instantiation(128, R.FWD_IMPLICIT_USERS * p, p) for p in R.FWD_PPU] == [(4, 4, 4), (4, 2, 2), (4, 2, 0)]
    assert R.fwd_instantiation(128, 65535) == (4, 1, 0) and R.fwd_instantiation(128, 65536) == (4, 2, 0)
    assert R.fwd_instantiation(5, 65535) == (1, 1, 0) and R.fwd_instantiation(5, 65536) == (1, 2, 0)


# ------------------------------------------------------------------------------------------------ backward
def segment_sums32(terms, seg, n_seg, order):
    """per-segment float32 sums of the rows of terms, in pair order (seq) or 64 interleaved chains joined by a tree (split64)"""
    out = np.zeros((n_seg,) + terms.shape[1:], F)
    idx = np.argsort(seg, kind="stable")
    bounds = np.searchsorted(seg[idx], np.arange(n_seg + 1))
    for r in range(n_seg):
        t = terms[idx[bounds[r]:bounds[r + 1]]]
        if not t.shape[0]:
            continue
        if order == "seq":
            out[r] = np.cumsum(t, axis=0, dtype=F)[-1]
        else:
            pad = (-t.shape[0]) % 64
            t = np.concatenate([t, np.zeros((pad,) + t.shape[1:], F)]).reshape((-1, 64) + t.shape[1:])
            out[r] = tree64(np.cumsum(t, axis=0, dtype=F)[-1][None])[0]
    return out


def grads32(case, mode, order):
    x, y, g = case.U[case.xu], case.V[case.xi], case.g
    if mode == MODE_DOT:
        tu, tv = (g[:, None] * y).astype(F), (g[:, None] * x).astype(F)
    else:
        D = chain32(x, y, mode, order)
        with np.errstate(divide="ignore", invalid="ignore"):
            c = np.where(D >= F(1e-16), (-g / np.sqrt(D)).astype(F), F(0.0)).astype(F)
        tu = (c[:, None] * (x - y).astype(F)).astype(F)
        tv = -tu
    nu, ni = case.U.shape[0], case.V.shape[0]
    return (segment_sums32(tu, case.xu, nu, order), segment_sums32(tv, case.xi, ni, order),
            segment_sums32(g, case.xu, nu, order), segment_sums32(g, case.xi, ni, order))


def within(got, want, bar):
    return bool((np.abs(f64(got) - want) <= bar).all())


@pytest.mark.parametrize("d", R.BWD_D)
@pytest.mark.parametrize("form", R.BWD_FORMS)
def test_backward_bars_hold_for_float32_restatements(form, d):
    case = R.bwd_case(form, d)
    p = R.bwd_case_properties(case)
    assert p["n_pairs"] >= 65536 and p["max_item"] > R.SPLIT_T and p["max_user"] <= R.SPLIT_T and p["empty_item"]
    assert p["clamped"] >= len(R.BWD_CLAMPED)
    assert p["empty_user"] == (form != "implicit")
    assert (p["repeated"] > 0) == (form != "inter")
    for mode in (MODE_DOT, MODE_EUCLID):
        ref = R.ref_pair_grads(case.U, case.V, case.xu, case.xi, case.g, mode)
        if mode == MODE_EUCLID:
            clamped = R.clamped_pairs(case)
            assert (ref.coef[clamped] == 0.0).all() and (ref.coef[~clamped] != 0.0).all() and (ref.D[~clamped] > 1e-3).all()
        bars = R.grad_bars(ref, d)
        for order in ("seq", "split64"):
            got = grads32(case, mode, order)
            for name, a, b, bar in zip(("dU", "dV", "dub", "dib"), got, (ref.dU, ref.dV, ref.dub, ref.dib), bars):
                assert within(a, b, bar), "%s d %d mode %d %s %s: worst ratio %.2f" % (
                    form, d, mode, order, name, (np.abs(f64(a) - b) / np.maximum(bar, 1e-300)).max())
        # rows nobody touches have a bar of 0: the gradient there is exactly 0
        assert (bars[1][R.BWD_EMPTY_ITEM] == 0).all() and (ref.dV[R.BWD_EMPTY_ITEM] == 0).all()


def test_backward_routes_cover_every_entry_point():
    """ops_base._PairScore.backward's routing restated (pair_reference.bwd_routes): over the GPU test's grid every one of the four entry
    points is the named route of some case, both gathers meet in one case, and d = 261 sends Euclidean pairs to the atomic kernel"""
    seen = set()
    for form in R.BWD_FORMS:
        for d in R.BWD_D:
            p = R.bwd_case_properties(R.bwd_case(form, d)) if d == R.BWD_D[0] else p
            long_i = p["max_item"] > R.SPLIT_T if form == "inter" else p["n_pairs"] > R.BWD_ITEMS * 1700
            for mode in (MODE_DOT, MODE_EUCLID):
                seen |= R.bwd_routes(form, mode, d, p["n_pairs"], False, long_i)
    assert seen == set(R.BWD_ENTRY_POINTS)
    n = 66000
    assert R.bwd_routes("inter", MODE_DOT, 8, n, False, True) == {"trec_spmm_csr", "trec_spmm_csr_split"}
    assert R.bwd_routes("implicit", MODE_DOT, 8, n, False, False) == {"trec_spmm_csr"}
    assert R.bwd_routes("implicit", MODE_DOT, 5, n, False, False) == {"trec_spmm_csr_split"}
    assert R.bwd_routes("inter", MODE_DOT, 261, n, False, True) == {"trec_spmm_csr"}
    assert R.bwd_routes("inter", MODE_EUCLID, 261, n, False, True) == {"trec_pair_score_bwd"}
    assert R.bwd_routes("inter", MODE_EUCLID, 260, n, False, True) == {"trec_pair_euclid_coef", "trec_spmm_csr_split"}


# ------------------------------------------------------------------------------------------------ WMRB
def wmrb32(case, weight, order):
    """loss, d pred, d samp in np.float32, the kernels' operation order: (1 - p) + s, ratio * sum, * weight, log(smr + 1)"""
    S, nu = case.S, case.n_users
    ratio = F(F(case.n_items) / F(S))
    pos = case.values > 0
    slot = np.cumsum(pos) - 1
    loss, d_pred, d_samp = np.zeros(int(pos.sum()), F), np.zeros(case.pred.size, F), np.zeros((nu, S), F)

    def sums(t, axis):                                                     # t: [m, S]
        t = np.moveaxis(t, axis, 0)
        if order == "seq":
            return np.cumsum(t, axis=0, dtype=F)[-1]
        pad = (-t.shape[0]) % 64
        t = np.concatenate([t, np.zeros((pad,) + t.shape[1:], F)]).reshape((-1, 64) + t.shape[1:])
        return tree64(np.cumsum(t, axis=0, dtype=F)[-1][None])[0]

    for u in range(nu):
        idx = np.arange(case.indptr[u], case.indptr[u + 1])
        idx = idx[pos[idx]]
        if not idx.size:
            continue
        H = ((F(1.0) - case.pred[idx]).astype(F)[:, None] + case.samp[u][None, :]).astype(F)
        act = H >= 0
        smr = (ratio * sums(np.maximum(H, F(0.0)), 1)).astype(F)
        w = weight[idx].astype(F) if weight is not None else None
        if w is not None:
            smr = (smr * w).astype(F)
        loss[slot[idx]] = np.log(f64((smr + F(1.0)).astype(F))).astype(F)
        c = ((case.go[slot[idx]] * ratio).astype(F) / (F(1.0) + smr).astype(F)).astype(F)
        if w is not None:
            c = (c * w).astype(F)
        d_pred[idx] = (-c * act.sum(1).astype(F)).astype(F)
        d_samp[u] = sums(np.where(act, c[:, None], F(0.0)).astype(F), 0)
    return loss, d_pred, d_samp


def check_wmrb_case(case):
    assert R.wmrb_inputs_exact(case.pred, case.samp)
    w64, cnt = R.balanced_weights(case)
    assert (w64[case.values > 0] > 0).all() and (w64[case.values > 0] != 1.0).any() and (w64[case.values <= 0] == 0).all()
    n_pos = np.array([int((case.values[case.indptr[u]:case.indptr[u + 1]] > 0).sum()) for u in range(case.n_users)])
    assert list(n_pos) == R.WMRB_POSITIVES
    assert (case.values < 0).any() and (case.values == 0).any()
    for weight in (None, w64.astype(F)):
        ref = R.ref_wmrb(case.indptr, case.values, weight, case.pred, case.samp, case.n_items, case.go)
        # the hinge-at-zero and the all-inactive cases are there
        for u in range(case.n_users):
            if n_pos[u] and u != R.WMRB_INACTIVE_USER:
                assert ref.zero_hinges[u] >= 1, "user %d lost its hinge of exactly 0" % u
        assert ((1.0 - f64(case.pred)[ref.pos][:, None] + f64(case.samp)[np.repeat(np.arange(case.n_users), n_pos)]) == 0).sum() > 0
        assert ref.inactive_users == [R.WMRB_INACTIVE_USER]
        lo, hi = case.indptr[R.WMRB_INACTIVE_USER], case.indptr[R.WMRB_INACTIVE_USER + 1]
        sl = ref.slot[lo:hi][ref.pos[lo:hi]]
        assert (ref.loss[sl] == 0).all() and (ref.d_pred[lo:hi] == 0).all() and (ref.d_samp[R.WMRB_INACTIVE_USER] == 0).all()
        assert (ref.d_pred[~ref.pos] == 0).all() and (ref.d_samp[:2] == 0).all()           # non-positives / users without positives
        assert ref.max_sum * R.GRID < 2.0 ** 24
        bars = R.wmrb_bars(ref)
        for order in ("seq", "split64"):
            got = wmrb32(case, weight, order)
            for name, a, b, bar in zip(("loss", "d_pred", "d_samp"), got, (ref.loss, ref.d_pred, ref.d_samp), bars):
                err = np.abs(f64(a) - b)
                assert (err <= bar).all(), "S %d %s %s balanced %d: worst ratio %.2f" % (
                    case.S, order, name, weight is not None, (err / np.maximum(bar, 1e-300)).max())


@pytest.mark.parametrize("S", sorted(set(R.WMRB_S + R.WMRB_S_MANY)))
def test_wmrb_bars_hold_for_float32_restatements(S):
    check_wmrb_case(R.wmrb_case(S))


# ------------------------------------------------------------------------------------------------ the knob the GPU file restores with
def test_clear_tuning_returns_a_knob_to_its_callers_default():
    from tensorrec_amd import _native
    lib = _native.load()
    _native.set_tuning("a_knob_no_kernel_reads", 3)
    assert lib.trec_get_tuning(b"a_knob_no_kernel_reads", 7) == 3
    _native.clear_tuning("a_knob_no_kernel_reads")
    assert lib.trec_get_tuning(b"a_knob_no_kernel_reads", 7) == 7 and lib.trec_get_tuning(b"a_knob_no_kernel_reads", -5) == -5
    _native.clear_tuning("a_knob_no_kernel_reads")                          # clearing what is not set is not an error
