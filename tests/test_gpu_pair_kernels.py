"""K3 (csrc/pair_score.hip) and K6's WMRB kernels (csrc/loss.hip) against the float64 references of tests/pair_reference.py, within the
bars derived there from the number formats (tests/test_pair_reference_host.py shows on the CPU that the bars are not too tight).

* forward      every instantiation pair_score_fwd_kernel<VEC, PP, UG> that trec_pair_score_fwd launches, selected through the tunings
               pair_fwd_pp / pair_fwd_user_group: all of them give the bits of PP = 1, and those lie within the bar of float64;
* backward     every host route of ops_base._PairScore.backward, recorded at _native.call and asserted per case;
* clamp        D < 1e-16: score -1e-8, coefficient exactly 0, no gradient to either row, the biases still receive g;
* WMRB         hinges of exactly 0, S on both sides of the wave-per-user limit, more than 1,024 positives per user with S > 256,
               balanced weights, a user whose hinges are all inactive."""
import functools

import numpy as np
import pytest
import torch

import pair_reference as R
from pair_reference import MODE_DOT, MODE_EUCLID, f64

pytestmark = pytest.mark.gpu

UNSET = -(2 ** 31) + 12345                                    # no tuning holds this value


@pytest.fixture(scope="module")
def ops():
    from tensorrec_amd import ops as _ops, _native
    _native.require_gpu()
    _native.load()
    return _ops


@pytest.fixture(scope="module")
def N(ops):
    from tensorrec_amd import _native
    return _native


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class tunings(object):
    """``with tunings(N, pair_fwd_pp=2):`` -- set through _native.set_tuning, put back on exit: a knob that was not set is cleared again
    (pair_fwd_pp's default depends on the call, so no value would restore it)"""

    def __init__(self, N, **values):
        self.N, self.values = N, values

    def __enter__(self):
        lib = self.N.load()
        self.before = {k: lib.trec_get_tuning(k.encode(), UNSET) for k in self.values}
        for k, v in self.values.items():
            if v is not None:
                self.N.set_tuning(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.before.items():
            if v == UNSET:
                self.N.clear_tuning(k)
            else:
                self.N.set_tuning(k, v)
        return False


def check(got, want, bar, what):
    got, want, bar = f64(got).reshape(-1), f64(want).reshape(-1), f64(bar).reshape(-1)
    assert got.shape == want.shape, what
    assert np.isfinite(got).all(), "%s: %d entries not written or not finite" % (what, int((~np.isfinite(got)).sum()))
    err = np.abs(got - want)
    bad = err > bar
    if bad.any():
        k = int(np.argmax(err - bar))
        raise AssertionError("%s: %d of %d outside the bar; worst at %d: got %r, float64 %r, bar %.3e (ratio %.2f)"
                             % (what, int(bad.sum()), got.size, k, got[k], want[k], bar[k], err[k] / max(bar[k], 1e-300)))


# ------------------------------------------------------------------------------------------------ forward
def fwd_call(N, t, mode, with_bias, want_sqdist):
    n = t["xi"].numel()
    out = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    sq = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda") if want_sqdist else None
    N.call("trec_pair_score_fwd", N.ptr(t["U"]), N.ptr(t["V"]), N.ptr(t["xu"]), N.ptr(t["xi"]), n, t["ppu"], t["U"].shape[1], mode,
           N.ptr(t["ub"]) if with_bias else None, N.ptr(t["ib"]) if with_bias else None, N.ptr(out), N.ptr(sq))
    return out, sq


def check_forward(N, case, d, mode):
    implicit = case.ppu > 0
    t = dict(U=dev(case.U), V=dev(case.V), xu=None if implicit else dev(case.xu), xi=dev(case.xi), ub=dev(case.ub), ib=dev(case.ib),
             ppu=case.ppu)
    n = case.xi.size
    clamped = R.clamped_pairs(case)
    assert clamped.sum() >= 2 and clamped[-1]
    xu_l, xi_l = dev(case.xu.astype(np.int64)), dev(case.xi.astype(np.int64))
    for with_bias in (False, True):
        ref = R.ref_pair_scores(case.U, case.V, case.xu, case.xi, mode, case.ub if with_bias else None, case.ib if with_bias else None)
        what = "d %d n %d ppu %d mode %d bias %d" % (d, n, case.ppu, mode, with_bias)
        base = None
        for pp, ug in [(None, None)] + R.FWD_TUNINGS:               # first the shipped choice, then every forced one
            with tunings(N, pair_fwd_pp=pp, pair_fwd_user_group=ug):
                out, sq = fwd_call(N, t, mode, with_bias, mode == MODE_EUCLID)
            torch.cuda.synchronize()
            which = "%s, %s" % (what, R.fwd_instantiation(d, n, case.ppu, pp, 1 if ug is None else ug))
            if base is None:
                base = (out, sq)
                check(out.cpu().numpy(), ref.scores, R.score_bar(ref, d), which)
                if mode == MODE_EUCLID:
                    check(sq.cpu().numpy(), ref.mag, R.chain_bar(ref, d), which + " sqdist")
                    assert (sq.cpu().numpy()[clamped] == 0).all()
                    want = -torch.sqrt(torch.clamp(sq, min=1e-16))
                    if with_bias:
                        want = want + t["ub"][xu_l] + t["ib"][xi_l]
                    assert torch.equal(out, want), which + ": out != -sqrt(max(sqdist, 1e-16)) + biases bit for bit"
                    raw = out.cpu().numpy()[clamped] if not with_bias else None
                    assert raw is None or (raw == -np.sqrt(np.float32(1e-16))).all(), which + ": a clamped pair is not -1e-8"
            else:
                assert torch.equal(out, base[0]), which + ": not the bits of the shipped choice"
                assert sq is None or torch.equal(sq, base[1]), which + ": sqdist differs"


@pytest.mark.parametrize("mode", [MODE_DOT, MODE_EUCLID], ids=["dot", "euclid"])
@pytest.mark.parametrize("n_pairs", R.FWD_N_PAIRS)
@pytest.mark.parametrize("d", R.FWD_D)
def test_pair_fwd_explicit_users(N, d, n_pairs, mode):
    """<4,1> / <1,1> (65,535 pairs, or pair_fwd_pp = 1), <4,2> (the default from 65,536), <4,4> (pair_fwd_pp = 4), <1,2> (d = 5, 67 from
    65,536 pairs); 65,539 pairs leave a ragged tail under PP = 2 and 4, and the last pair is a clamped one"""
    check_forward(N, R.fwd_explicit_case(d, n_pairs), d, mode)


@pytest.mark.parametrize("mode", [MODE_DOT, MODE_EUCLID], ids=["dot", "euclid"])
@pytest.mark.parametrize("ppu", R.FWD_PPU)
@pytest.mark.parametrize("d", R.FWD_D)
def test_pair_fwd_implicit_users(N, d, ppu, mode):
    """16,385 users, user of pair p = p // ppu: by default ppu = 4 -> <4,4,4>, 6 -> <4,2,2>, 7 -> <4,2>; pair_fwd_user_group = 0 gives the
    same PP without the shared user row, pair_fwd_pp = 2 at ppu = 4 <4,2,2>, pair_fwd_pp = 4 at ppu = 6 <4,4>"""
    check_forward(N, R.fwd_implicit_case(d, ppu), d, mode)


def test_tunings_are_put_back(N):
    lib = N.load()
    names = ("pair_fwd_pp", "pair_fwd_user_group", "wmrb_wave")
    before = [lib.trec_get_tuning(k.encode(), UNSET) for k in names]
    with tunings(N, pair_fwd_pp=4, pair_fwd_user_group=None, wmrb_wave=0):
        assert lib.trec_get_tuning(b"pair_fwd_pp", UNSET) == 4 and lib.trec_get_tuning(b"wmrb_wave", 1) == 0
        assert lib.trec_get_tuning(b"pair_fwd_user_group", UNSET) == before[1]
    assert [lib.trec_get_tuning(k.encode(), UNSET) for k in names] == before


# ------------------------------------------------------------------------------------------------ Euclidean coefficient
@pytest.mark.parametrize("d", [4, 20, 260, 5, 67])
def test_euclid_coef_both_forms(N, d):
    """trec_pair_euclid_coef from the rows (pair_euclid_coef_kernel) and from the kept squared distances: -g / sqrt(D) within the bar,
    exactly 0 at the clamped pairs"""
    case = R.fwd_explicit_case(d, 65539)
    rng = np.random.default_rng(d)
    g = rng.standard_normal(case.xi.size).astype(np.float32)
    ref = R.ref_pair_grads(case.U, case.V, case.xu, case.xi, g, MODE_EUCLID)
    clamped = R.clamped_pairs(case)
    assert clamped.sum() >= 2 and (g[clamped] != 0).all() and (ref.coef[clamped] == 0).all()
    t = dict(U=dev(case.U), V=dev(case.V), xu=dev(case.xu), xi=dev(case.xi), ub=None, ib=None, ppu=0)
    gd = dev(g)
    n = g.size
    _, sq = fwd_call(N, t, MODE_EUCLID, False, True)
    for form, args in (("rows", (N.ptr(t["U"]), N.ptr(t["V"]), N.ptr(t["xu"]), N.ptr(t["xi"]), N.ptr(gd), None)),
                       ("sqdist", (None, None, None, None, N.ptr(gd), N.ptr(sq)))):
        coef = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
        N.call("trec_pair_euclid_coef", *args, n, 0, d, N.ptr(coef))
        torch.cuda.synchronize()
        got = coef.cpu().numpy()
        check(got, ref.coef, R.coef_bar(ref, d), "coef from %s, d %d" % (form, d))
        assert (got[clamped] == 0).all(), "coef from %s: a clamped pair has a coefficient" % form


# ------------------------------------------------------------------------------------------------ backward
@functools.lru_cache(maxsize=1)
def bwd_inputs(form, d):
    case = R.bwd_case(form, d)
    return case, {m: R.ref_pair_grads(case.U, case.V, case.xu, case.xi, case.g, m) for m in (MODE_DOT, MODE_EUCLID)}


def bwd_expected_routes(form, mode, d, case):
    p = R.bwd_case_properties(case)
    long_i = p["max_item"] > R.SPLIT_T if form == "inter" else p["n_pairs"] > R.BWD_ITEMS * 1700
    return R.bwd_routes(form, mode, d, p["n_pairs"], p["max_user"] > R.SPLIT_T, long_i)


BWD_CASES = []
for _form in R.BWD_FORMS:
    for _d in R.BWD_D:
        for _mode, _mname in ((MODE_DOT, "dot"), (MODE_EUCLID, "euclid")):
            _long_i = _form == "inter"                          # (asserted against the data in the test: item 0 of inter is long)
            _routes = R.bwd_routes(_form, _mode, _d, 66000, False, _long_i)
            _name = "+".join(sorted(r.replace("trec_", "") for r in _routes))
            for _bias in (False, True):
                BWD_CASES.append(pytest.param(_form, _mode, _d, _bias, frozenset(_routes),
                                              id="%s-%s-d%d-%s-%s" % (_form, _mname, _d, "bias" if _bias else "nobias", _name)))


@pytest.mark.parametrize("form,mode,d,with_bias,routes", BWD_CASES)
def test_pair_bwd_routes(ops, N, monkeypatch, form, mode, d, with_bias, routes):
    """dU, dV, dub, dib of sum_p g_p s_p on 66,000 pairs or more: a user and an item without pairs, repeated pairs, clamped Euclidean pairs
    and an item above SPLIT_T pairs; the entry points recorded at _native.call are those the id names; the structured routes give the
    same bits twice (sampled pairs: under ops.deterministic_grouping, which fixes the order inside an item's bucket)"""
    from tensorrec_amd.sparse import Interactions, PairIndex
    case, refs = bwd_inputs(form, d)
    ref = refs[mode]
    assert bwd_expected_routes(form, mode, d, case) == set(routes)
    if form == "inter":
        inter = Interactions(case.matrix, R.BWD_USERS, R.BWD_ITEMS, "cuda")
        assert np.array_equal(inter.x_user.cpu().numpy(), case.xu) and np.array_equal(inter.x_item.cpu().numpy(), case.xi)
        xu = PairIndex.make(inter.x_user, inter.x_user32, 0, inter)
        xi = PairIndex.make(inter.x_item, inter.x_item32, 0, inter)
    elif form == "implicit":
        flat = dev(case.xi)
        xu = xi = PairIndex.make(flat.long(), flat, case.ppu)
    else:
        xu, xi = dev(case.xu.astype(np.int64)), dev(case.xi.astype(np.int64))
    g = dev(case.g)
    calls = []
    real_call = N.call
    monkeypatch.setattr(N, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])

    def run():
        leaves = [dev(case.U).requires_grad_(), dev(case.V).requires_grad_()]
        leaves += [dev(case.ub).requires_grad_(), dev(case.ib).requires_grad_()] if with_bias else [None, None]
        s = ops.pair_score(leaves[0], leaves[1], xu, xi, mode, leaves[2], leaves[3])
        s.backward(g)
        torch.cuda.synchronize()
        return s.detach(), [t.grad if t is not None else None for t in leaves]

    s, grads = run()
    took = set(calls) & set(R.BWD_ENTRY_POINTS)
    assert took == set(routes), "took %s, the case names %s" % (sorted(took), sorted(routes))
    what = "%s mode %d d %d bias %d" % (form, mode, d, with_bias)
    fref = R.ref_pair_scores(case.U, case.V, case.xu, case.xi, mode, case.ub if with_bias else None, case.ib if with_bias else None)
    check(s.cpu().numpy(), fref.scores, R.score_bar(fref, d), what + " scores")
    bars = R.grad_bars(ref, d)
    wants = (ref.dU, ref.dV, ref.dub, ref.dib)
    for name, got, want, bar in zip(("dU", "dV", "dub", "dib"), grads, wants, bars):
        if got is not None:
            check(got.cpu().numpy(), want, bar, what + " " + name)
    if mode == MODE_EUCLID:
        # rows that hold clamped pairs only through them: user 10 / 11 get no gradient from (10, 3) / (11, 4); checked by the bar, whose
        # terms leave those pairs out (coefficient 0) -- and the biases still receive their g
        clamped = R.clamped_pairs(case)
        assert clamped.sum() >= len(R.BWD_CLAMPED) and (ref.coef[clamped] == 0).all()
    assert (f64(grads[1].cpu().numpy())[R.BWD_EMPTY_ITEM] == 0).all()
    if form != "implicit":
        assert (f64(grads[0].cpu().numpy())[R.BWD_EMPTY_USER] == 0).all()
    if "trec_pair_score_bwd" in routes:
        return                                                    # atomics: the order of the additions is not fixed
    if form == "implicit":
        with ops.deterministic_grouping(True):
            _, a = run()
            _, b = run()
        for name, x, want, bar in zip(("dU", "dV", "dub", "dib"), a, wants, bars):
            if x is not None:
                check(x.cpu().numpy(), want, bar, what + " (stable grouping) " + name)
    else:
        a, (_, b) = grads, run()
    for name, x, y in zip(("dU", "dV", "dub", "dib"), a, b):
        assert x is None or torch.equal(x, y), what + ": two calls differ in " + name


@pytest.mark.parametrize("d", [8, 5])
def test_clamped_pair_alone_gives_no_row_gradient(ops, d):
    """one user, one item, identical rows, three copies of the pair: score -1e-8 + biases, dU = dV = 0 exactly, dub = dib = sum g --
    on the atomic route and on the structured one"""
    from tensorrec_amd.sparse import PairIndex
    row = np.random.default_rng(d).standard_normal((1, d)).astype(np.float32)
    g = np.array([0.5, -2.0, 4.0], np.float32)
    idx = dev(np.zeros(3, np.int32))
    for x in (idx.long(), PairIndex.make(idx.long(), idx, 3)):
        u, v = dev(row).requires_grad_(), dev(row.copy()).requires_grad_()
        ub, ib = dev(np.array([0.25], np.float32)).requires_grad_(), dev(np.array([-1.0], np.float32)).requires_grad_()
        s = ops.pair_score(u, v, x, x, MODE_EUCLID, ub, ib)
        s.backward(dev(g))
        torch.cuda.synchronize()
        assert np.array_equal(s.detach().cpu().numpy(), np.full(3, (-np.sqrt(np.float32(1e-16)) + np.float32(0.25)) + np.float32(-1.0), np.float32))
        assert not u.grad.any() and not v.grad.any()
        assert float(ub.grad) == 2.5 and float(ib.grad) == 2.5


# ------------------------------------------------------------------------------------------------ WMRB
def run_wmrb(ops, case, inter, balanced):
    pt, st = dev(case.pred).requires_grad_(), dev(case.samp).requires_grad_()
    loss = ops.wmrb_loss(pt, st, inter, balanced=balanced)
    loss.backward(dev(case.go))
    torch.cuda.synchronize()
    return loss.detach().cpu().numpy(), pt.grad.cpu().numpy(), st.grad.cpu().numpy()


def check_wmrb(ops, N, S, balanced):
    from tensorrec_amd.sparse import Interactions
    case = R.wmrb_case(S)
    assert R.wmrb_inputs_exact(case.pred, case.samp)
    inter = Interactions(case.matrix, case.n_users, case.n_items, "cuda")
    assert np.array_equal(inter.indptr.cpu().numpy(), case.indptr) and np.array_equal(inter.values.cpu().numpy(), case.values)
    weight = None
    if balanced:
        # the weights are an input of the kernels: the reference takes the float32 values the kernels are handed; those are
        # value / item sum with the sum exact (multiples of 1/4) and one rounding for the division
        weight = inter.balanced_weight().cpu().numpy()
        w64, _ = R.balanced_weights(case)
        assert (np.abs(f64(weight) - w64) <= R.U32 * w64).all() and (weight[case.values > 0] != 1).any()
    ref = R.ref_wmrb(case.indptr, case.values, weight, case.pred, case.samp, case.n_items, case.go)
    n_pos = np.diff(case.indptr)
    assert ref.zero_hinges.sum() >= 7 and ref.inactive_users == [R.WMRB_INACTIVE_USER]
    bars = R.wmrb_bars(ref)
    results = {}
    for wave in ((1, 0) if S <= 256 else (1,)):                   # (above 256 samples the knob has no effect: the workgroup kernels run)
        with tunings(N, wmrb_wave=wave):
            results[wave] = run_wmrb(ops, case, inter, balanced)
        for name, got, want, bar in zip(("loss", "d_pred", "d_samp"), results[wave], (ref.loss, ref.d_pred, ref.d_samp), bars):
            check(got, want, bar, "S %d balanced %d wave %d %s" % (S, balanced, wave, name))
        loss, d_pred, d_samp = results[wave]
        lo, hi = case.indptr[R.WMRB_INACTIVE_USER], case.indptr[R.WMRB_INACTIVE_USER + 1]
        sl = ref.slot[lo:hi][ref.pos[lo:hi]]
        assert sl.size and (loss[sl] == 0).all() and (d_pred[lo:hi] == 0).all() and (d_samp[R.WMRB_INACTIVE_USER] == 0).all()
        assert (d_pred[~ref.pos] == 0).all() and (d_samp[:2] == 0).all() and n_pos[1] > 0
    if len(results) == 2:
        for name, a, b in zip(("loss", "d_pred", "d_samp"), results[1], results[0]):
            assert np.array_equal(a, b), "S %d balanced %d: wave and workgroup kernels differ in %s" % (S, balanced, name)


@pytest.mark.parametrize("balanced", [False, True], ids=["wmrb", "balanced"])
@pytest.mark.parametrize("S", R.WMRB_S)
def test_wmrb_sample_counts(ops, N, S, balanced):
    """S = 1 .. 256: the wave-per-user kernels and (wmrb_wave = 0) the workgroup kernels, bit-equal; 257, 300: the workgroup kernels.
    Users with 0, 65, 1,025 and 2,600 positives ride along at every S (1,025 and 2,600: the multi-pass backward)."""
    check_wmrb(ops, N, S, balanced)


@pytest.mark.parametrize("balanced", [False, True], ids=["wmrb", "balanced"])
@pytest.mark.parametrize("S", R.WMRB_S_MANY)
def test_wmrb_many_positives(ops, N, S, balanced):
    """0 / 65 / 1,025 / 2,600 positives per user at S = 40 (wave kernels: 64 positives per pass; workgroup kernels: 1,024 per pass) and
    S = 300 (workgroup kernels only)"""
    check_wmrb(ops, N, S, balanced)
