"""tests/score_reference.py held to the committed oracle on the CPU, its acceptance rules shown to reject planted errors, and its case table
counted against the dispatch code of csrc/score_gemm.hip / csrc/score_blockmax.hip.  No GPU."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import score_reference as R
from oracle import oracle as O
from score_reference import F32, f64

N_U, N_I = 37, 300


def oracle_scores(P, mode, bias):
    ub, ib = P.select(bias)
    if mode == R.MODE_EUCLID:
        return O.score_dense_euclid_exact(P.u_val, P.v_val, P.usq, P.vsq, ub, ib)
    return O.score_dense_exact(P.u_val, P.v_val, ub, ib)


# ------------------------------------------------------------------------------------------------ reference against the oracle
@pytest.mark.parametrize("bias", R.BIASES)
@pytest.mark.parametrize("mode", [R.MODE_DOT, R.MODE_EUCLID])
@pytest.mark.parametrize("kpad", R.KPADS)
def test_dyadic_restatement_equals_the_oracle_bit_for_bit(kpad, mode, bias):
    P = R.problem("dyadic", R.DT_F32, kpad, N_U, N_I)
    R.same_bits(P.restated(mode, bias), oracle_scores(P, mode, bias), "restate32")
    # ... and the float64 reference rounds to it wherever nothing but the last operation rounds (dot mode: nothing rounds at all)
    if mode == R.MODE_DOT:
        assert np.array_equal(f64(P.restated(mode, bias)), P.reference(mode, bias)[0])


def test_dyadic_euclid_hits_the_clamp_and_holds_ties():
    P = R.problem("dyadic", R.DT_F32, 64, N_U, N_I)
    s = P.restated(R.MODE_EUCLID, "none")
    assert np.all(s[R.DUP_USER, P.dups] == -np.sqrt(R.CLAMP32)) and len(P.dups) == 4
    d = P.restated(R.MODE_DOT, "both")
    assert len(set(d[R.DUP_USER, P.dups].tolist())) == 1 and np.all(np.argsort(-d[R.DUP_USER], kind="stable")[:4] == P.dups)
    ties = sum(int((np.diff(np.sort(row)) == 0).sum()) for row in d)
    assert ties > 1000, ties


@pytest.mark.parametrize("mode", [R.MODE_DOT, R.MODE_EUCLID])
@pytest.mark.parametrize("kpad", R.KPADS)
def test_real_reference_equals_the_oracle_within_the_bound(kpad, mode):
    P = R.problem("real", R.DT_F32, kpad, N_U, N_I)
    s, b = P.reference(mode, "both")
    r = R.within(oracle_scores(P, mode, "both"), s, b, "oracle against float64")
    assert 0 < r < 1
    assert b.min() > 0 and b.max() < 2e-3 * s.std()                               # a bound, not a blank cheque


def test_bf16_dot_restatement_uses_the_item_bias_first():
    """(b_i + s) + b_u and (s + b_u) + b_i are the same numbers on dyadic dot data (exact); behind the square root they are not"""
    Pb = R.problem("dyadic", R.DT_BF16, 64, N_U, N_I)
    Pf = R.problem("dyadic", R.DT_F32, 64, N_U, N_I)
    assert np.array_equal(bf := R.bf16_value(Pb.u_op), Pb.u_val) and bf.dtype == F32
    R.same_bits(Pb.restated(R.MODE_DOT, "both"), Pf.restated(R.MODE_DOT, "both"), "dot")
    R.same_bits(Pb.restated(R.MODE_EUCLID, "both"), Pf.restated(R.MODE_EUCLID, "both"), "euclid: both dtypes use (s + b_u) + b_i")


# ------------------------------------------------------------------------------------------------ bf16 rounding
def test_bf16_rounding_equals_torch():
    rng = np.random.default_rng(0)
    x = np.concatenate([
        rng.standard_normal(4096).astype(F32) * F32(10.0) ** rng.integers(-20, 20, 4096).astype(F32),
        np.array([0.0, -0.0, 1.0, -1.0, 3.0, 1e-40, -1e-40, 3.3895314e38], F32),
        # exact halves between two bf16 neighbours: ties go to the even one (bit 16 clear / set)
        np.array([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x00008000, 0x00018000], np.uint32).view(F32),
        # just above / below a half
        np.array([0x3F808001, 0x3F807FFF, 0x3F818001, 0x3F817FFF], np.uint32).view(F32),
        # rounds up into the next exponent (mantissa all ones)
        np.array([0x3FFFFFFF, 0x3FFF8000, 0x3FFF7FFF, 0xC07FC000, 0x007FFFFF], np.uint32).view(F32),
    ])
    want = torch.from_numpy(x).bfloat16().view(torch.int16).numpy().view(np.uint16)
    got = R.bf16_bits(x)
    assert np.array_equal(got, want)
    assert np.array_equal(R.bf16_value(got), torch.from_numpy(x).bfloat16().float().numpy())
    assert got[-5] == 0x4000 and got[-4] == 0x4000 and got[-3] == 0x3FFF          # 1.99999988 -> 2.0; the half rounds to even (up)


def test_operand_pads_with_zeros():
    x = np.arange(1, 11, dtype=F32).reshape(2, 5)
    op, val = R.operand(x, 32, R.DT_BF16)
    assert op.dtype == np.uint16 and op.shape == (2, 32) and np.all(op[:, 5:] == 0) and np.array_equal(val[:, :5], x)
    op, val = R.operand(x, 32, R.DT_F32)
    assert op.dtype == F32 and np.all(op[:, 5:] == 0) and np.array_equal(op, val)


# ------------------------------------------------------------------------------------------------ the dyadic claim
def test_dyadic_sums_are_exact_in_any_order():
    """the largest case (K = 256, both biases, Euclidean): products summed in three orders in float32 all equal the float64 result"""
    P = R.problem("dyadic", R.DT_F32, 256, N_U, N_I)
    prod = P.u_val[:, None, :] * P.v_val[None, :, :]                       # float32 products [n_u, n_i, K]
    assert prod.dtype == F32
    exact = f64(P.u_val) @ f64(P.v_val).T
    fwd = np.zeros(exact.shape, F32)
    bwd = np.zeros(exact.shape, F32)
    for k in range(256):
        fwd = fwd + prod[:, :, k]
        bwd = bwd + prod[:, :, 255 - k]
    tree = prod
    while tree.shape[2] > 1:                                               # pairwise: the order of a butterfly / of split accumulators
        tree = tree[:, :, 0::2] + tree[:, :, 1::2]
    for name, s in (("forward", fwd), ("backward", bwd), ("pairwise", tree[:, :, 0])):
        assert s.dtype == F32 and np.array_equal(f64(s), exact), name
    # the squared distance and the bias adds of the dot score are exact as well
    dist32 = (P.usq[:, None] - F32(2) * fwd) + P.vsq[None, :]
    assert np.array_equal(f64(dist32), f64(P.usq)[:, None] - 2 * exact + f64(P.vsq)[None, :])
    both32 = (fwd + P.ub[:, None]) + P.ib[None, :]
    assert np.array_equal(f64(both32), P.reference(R.MODE_DOT, "both")[0]) and np.array_equal((P.ib[None, :] + fwd) + P.ub[:, None], both32)
    assert np.abs(P.ub).max() <= 8 and np.all(P.ub * 4 == np.round(P.ub * 4)) and np.abs(P.u_val).max() == 3


# ------------------------------------------------------------------------------------------------ the rules can fail
K = 10


@pytest.fixture(scope="module")
def real():
    P = R.problem("real", R.DT_BF16, 64, N_U, N_I)
    s, b = P.reference(R.MODE_DOT, "both")
    v, i = R.topk(s, K, base=1000)
    return SimpleNamespace(P=P, s=s, b=b, v=v, i=i)


def test_rules_accept_the_reference(real):
    assert R.check_topk_bounded(real.v, real.i, real.s, real.b, K, base=1000) == 0.0
    assert R.check_store(real.s, real.s, real.b) == 0.0
    assert R.check_blockmax(R.blockmax(real.s, 128), real.s, real.b, 128) == 0.0
    d = R.problem("dyadic", R.DT_F32, 64, N_U, N_I).restated(R.MODE_DOT, "both")
    R.check_topk_exact(*R.topk(d, K, 1000), d, K, 1000)
    # fewer items than k
    v, i = R.topk(real.s[:, :7], K, base=1000)
    assert np.all(i[:, 7:] == -1) and np.all(v[:, 7:] == -np.inf)
    R.check_topk_bounded(v, i, real.s[:, :7], real.b[:, :7], K, base=1000)
    # a result that errs by less than the bound passes, and its ratio is reported
    assert 0.49 < R.check_store(real.s + 0.5 * real.b, real.s, real.b) < 0.51


def test_rules_reject_an_id_swapped_with_the_next_best(real):
    nxt = R.topk(real.s, K + 1, base=1000)[1][:, K]
    for place in (0, K - 1):
        i = real.i.copy()
        i[5, place] = nxt[5]
        with pytest.raises(AssertionError):
            R.check_topk_bounded(real.v, i, real.s, real.b, K, base=1000)
    # ... value and id swapped together: the order of the values is intact, an unlisted item is better than the k-th
    v, i = real.v.copy(), real.i.copy()
    v[5, K - 1], i[5, K - 1] = R.topk(real.s, K + 1, base=1000)[0][5, K], nxt[5]
    assert real.s[5, real.i[5, K - 1] - 1000] - v[5, K - 1] > 4 * real.b[5].max()          # (the gap the rule needs to see)
    with pytest.raises(AssertionError, match="unlisted"):
        R.check_topk_bounded(v, i, real.s, real.b, K, base=1000)


def test_rules_reject_a_value_moved_by_three_bounds(real):
    for sign in (1.0, -1.0):
        v = real.v.copy()
        v[3, 4] += sign * 3.0 * real.b[3, real.i[3, 4] - 1000]
        with pytest.raises(AssertionError):
            R.check_topk_bounded(v, real.i, real.s, real.b, K, base=1000)
        s = real.s.copy()
        s[3, 4] += sign * 3.0 * real.b[3, 4]
        with pytest.raises(AssertionError, match="beyond the bound"):
            R.check_store(s, real.s, real.b)


def test_rules_reject_ties_in_descending_index_order():
    P = R.problem("dyadic", R.DT_F32, 64, N_U, N_I)
    d = P.restated(R.MODE_DOT, "both")
    v, i = R.topk(d, K, 1000)
    assert v[R.DUP_USER, 0] == v[R.DUP_USER, 1] and i[R.DUP_USER, 0] < i[R.DUP_USER, 1]
    i2 = i.copy()
    i2[R.DUP_USER, [0, 1]] = i[R.DUP_USER, [1, 0]]
    with pytest.raises(AssertionError):
        R.check_topk_exact(v, i2, d, K, 1000)
    s, b = P.reference(R.MODE_DOT, "both")
    R.check_topk_bounded(v, i, s, b, K, 1000)
    with pytest.raises(AssertionError, match="ascending index"):
        R.check_topk_bounded(v, i2, s, b, K, 1000)
    # ... and an id listed twice, an id outside the catalogue, a filled place past the end
    for bad in ((1, i[2, 0]), (1, 1000 + N_I), (1, 999)):
        i3 = i.copy()
        i3[2, bad[0]] = bad[1]
        with pytest.raises(AssertionError):
            R.check_topk_bounded(v, i3, s, b, K, 1000)


def test_rules_reject_a_lowered_block_maximum(real):
    sb = 128
    table = R.blockmax(real.s, sb)
    cell = (1, 6)
    second = np.sort(real.s[cell[1], sb:2 * sb])[-2]
    assert table[cell] - second > 2 * real.b[cell[1], sb:2 * sb].max()
    low = table.copy()
    low[cell] = second
    with pytest.raises(AssertionError, match="beyond the bound"):
        R.check_blockmax(low, real.s, real.b, sb)
    d = R.problem("dyadic", R.DT_F32, 64, N_U, N_I).restated(R.MODE_DOT, "both")
    t32 = R.blockmax(d, sb)
    assert t32.dtype == F32 and t32.shape == (3, N_U)                     # 300 items: 128 + 128 + 44
    low = t32.copy()
    low[2, 0] = np.sort(np.unique(d[0, 2 * sb:]))[-2]
    with pytest.raises(AssertionError):
        R.same_bits(low, t32, "table")


def test_rules_reject_an_overwritten_padding_cell():
    buf = np.full((5, 9), -777.25, F32)
    written = np.zeros((5, 9), bool)
    written[:4, :6] = True
    buf[written] = 1.0
    R.check_padding(buf, written, F32(-777.25), "out")
    for cell in ((0, 6), (4, 0), (4, 8)):
        b2 = buf.copy()
        b2[cell] = 1.0
        with pytest.raises(AssertionError, match="overwritten"):
            R.check_padding(b2, written, F32(-777.25), "out")
    nanbuf = np.full((2, 2), np.nan, F32)
    R.check_padding(nanbuf, np.zeros((2, 2), bool), F32(np.nan), "nan sentinel")       # compared on the bits


# ------------------------------------------------------------------------------------------------ the case table
def test_grid_has_the_size_the_dispatch_code_implies():
    g = R.grid()
    n_cases = 8                       # TREC_SCORE_CASE lines of dispatch_score: 2 dtypes x kpad 32 / 64 / 128 / 256
    forms = (4 * 2 + 4 * 3)           # per (dtype, kpad): fp32 {dot, euclid}, bf16 {dot, glds, euclid} -> 20
    biases = 4                        # none, both, user only, item only
    epilogues = 1 + 3 + 1             # STORE, TOPK x capacity 8 / 12 / 16, BLOCKMAX
    tilings = 6 * 2                   # variant >> 1 in 1..6, glds bit: variants 2..13
    hand = 3 * 2 * biases             # pipelined bf16, pipelined fp32, filter16 x K 64 / 128 x bias option
    assert len(R.SCORE_CASES) == n_cases and sum(len(R.FORMS[dt]) for dt, _ in R.SCORE_CASES) == forms
    assert len(g) == forms * biases * epilogues + tilings + hand == 400 + 12 + 24
    assert len({c.id for c in g}) == len(g)
    assert sum(not c.testable for c in g) == 4 and all(c.variant >> 1 in (4, 5) for c in g if not c.testable)
    assert len(R.cases("store")) == 80 and len(R.cases("topk")) == 240 + 8 and len(R.cases("blockmax")) == 80 + 24
    assert all(c.variant & 1 for c in g if c.form == "glds") and all(c.dtype == R.DT_BF16 for c in g if c.form == "glds")


def test_geometry_restates_score_cfg():
    assert [R.rows_per_workgroup(dt, kp) for dt, kp in R.SCORE_CASES] == [128] * 4 + [256, 256, 256, 128]
    assert [R.tile_rows(dt, kp) for dt, kp in R.SCORE_CASES] == [32] * 4 + [64] * 4
    assert R.topk_parts(300, 1) == 2 and R.topk_parts(300, 3) == 6 and R.topk_parts(257, 2) == 4 and R.topk_parts(1, 1) == 2
