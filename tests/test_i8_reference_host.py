"""tests/i8_reference.py held to second formulations on the CPU, its acceptance helpers shown to reject planted errors on the operands the
GPU tests use (tests/test_gpu_i8_stage.py), the bound i8_pair_err shown to hold for the reference pipeline alone on the GPU bound test's
populations, and the case table counted against the dispatch code of csrc/score_blockmax_i8.hip.  No GPU."""
import os
import re

import numpy as np
import pytest

import i8_reference as R
from i8_reference import F32, f64

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tensorrec_amd", "csrc", "score_blockmax_i8.hip")
SENT = F32(-12345.5)


def case(cid):
    return next(c for c in R.grid() if c.id == cid)


# ------------------------------------------------------------------------------------------------ second formulations
def test_integer_matmul_equals_an_int64_einsum():
    P = R.pool(128)
    uq, iq = P.uq[:23], P.iq[:57]
    want = np.einsum("uk,ik->ui", uq.astype(np.int64), iq.astype(np.int64))
    assert np.array_equal(R.int_dots(uq, iq), want.astype(np.float64)) and np.array_equal(P.dots[:23, :57], want)
    assert P.dots[0, 0] == 127 * 127 * 128 and P.dots[1, 0] == -127 * 127 * 128              # the extreme accumulators
    # with the largest integer biases the sum still is an exact float64 and fits the int32 accumulator
    assert float(P.dots.max()) + R.BQ_MAX < 2 ** 31 and float(P.dots.min()) - R.BQ_MAX > -2 ** 31
    for kt in R.KTS:
        p = R.pool(kt)
        assert np.abs(p.uq).max() == 127 and np.abs(p.iq).max() == 127 and p.uq.min() == -127
        for q in (p.uq, p.iq):                                                                # no all-zero k-step anywhere
            assert np.all(np.abs(q.reshape(len(q), kt // 64, 64)).max(2) > 0)


def test_tags():
    rng = np.random.default_rng(3)
    lb = np.concatenate([rng.standard_normal(4000).astype(F32) * F32(10.0) ** rng.integers(-20, 20, 4000).astype(F32),
                         np.array([0.0, -0.0, 1.0, -1.0, 9.9e36, -9.9e36, 1e-45, -1e-45], F32)])
    idx = rng.integers(0, 4096, len(lb))
    t = R.lb_tag(lb, idx)
    assert np.all(t <= lb) and np.all(f64(lb) - f64(t) <= np.abs(f64(lb)) * 2.0 ** -10 + 1e-30)
    assert np.array_equal(R.lb_tag_index(t), idx)
    # monotone: a larger bound with any index stays above a smaller bound with any index once they are well apart (each tag moves a value by less than 2^13 units of its last place)
    a, b = np.sort(lb)[:-1], np.sort(lb)[1:]
    far = f64(b) - f64(a) > (np.abs(f64(b)) + np.abs(f64(a))) * 2.0 ** -8 + 1e-30
    assert np.all(R.lb_tag(b, 0)[far] > R.lb_tag(a, 4095)[far])
    dead = np.array([-np.inf, np.nan, np.inf, 1e37, -1e37, 3e38], F32)
    assert np.all(np.isneginf(R.lb_tag(dead, 5)))
    # the key is the monotone integer image of the float order
    s = np.sort(lb)
    assert np.all(np.diff(R.lb_key(s)) >= 0) and R.lb_key(F32(-0.0)) == 0 == R.lb_key(F32(0.0))


def test_chunk_arithmetic_equals_ops():
    from tensorrec_amd import ops
    for n_items in (1, 70, 128, 129, 717, 2637, 30005, 1_000_000):
        for n_chunks in (1, 2, 3, 7, 23, 128, 9999):
            for sb in (128, 512):
                assert R.chunks(n_items, n_chunks, sb) == tuple(ops.blockmax_i8_chunks(n_items, n_chunks, sb))
    assert R.chunks(717, 8, 128) == (128, 6)                                 # more chunks than superblocks: one superblock each


def test_quantisation_restated():
    x = np.array([[0.5, -0.5, 1.5, 2.5, 1000.0, -1000.0, np.nan, np.inf, -np.inf, 0.0]], F32)
    q = R.quantise(x, F32(1.0), 12)
    assert q.dtype == np.int8 and q.shape == (1, 12)
    assert q[0].tolist() == [0, 0, 2, 2, 127, -127, 0, 127, -127, 0, 0, 0]            # ties to even, clipped, NaN -> 0, zero padded
    # per-row and per-superblock scales
    y = np.arange(1, 13, dtype=F32).reshape(6, 2)
    b = R.item_scales(y, 4)
    assert np.array_equal(b, np.array([F32(8) / F32(127), F32(12) / F32(127)], F32))
    iq = R.quantise(y, R.rows_of_superblocks(b, 6, 4), 4)
    assert iq[3, 1] == 127 and iq[5, 1] == 127 and np.all(iq[:, 2:] == 0)
    st = R.row_stats(y, iq, R.rows_of_superblocks(b, 6, 4))
    assert np.allclose(st[:, 0], np.linalg.norm(y, axis=1)) and np.all(st[:, 1] < 0.5 * 2 ** 0.5 * b.max())
    assert R.item_scales(np.zeros((3, 2), F32), 4)[0] == 1 and R.item_scales(np.array([[np.nan, 1]], F32), 4)[0] == 1
    assert R.item_scales(np.array([[np.inf, 1]], F32), 4)[0] == 1
    # the users' one scale
    u = np.ones((8, 8), F32)
    u[0, 0] = 100
    assert R.user_scale(u, 0.0) == F32(100) / F32(127)
    rms = np.sqrt((f64(u) ** 2).mean())
    assert R.user_scale(u, 4.0) == F32(F32(4.0 * rms) / F32(127)) and R.user_scale(u, 1000.0) == F32(100) / F32(127)
    assert R.user_scale(np.zeros((2, 2), F32), 4.0) == 1
    # statistics of a superblock: float32 addition, NaN -> inf
    sb = R.sb_reduce(np.array([[1, 0.5], [3, 0.25], [np.nan, 1], [2, 2]], F32), 2)
    assert sb.tolist() == [[3.25, 0.5], [np.inf, 2.0]]


def test_row_scale_and_layout():
    rng = np.random.default_rng(5)
    x = R.rows("outliers", 600, 40, rng)
    x[::7] = 0
    nat, decided, gmax = R.row_scale(x)
    am = np.abs(x).max(1) / F32(127)
    assert np.all(nat[::7] == 0) and np.all(decided[::7]) and gmax == nat.max()
    ratio = nat[am > 0] / am[am > 0]
    assert set(np.unique(ratio).tolist()) <= {1.0, 0.5, 0.25} and (ratio == 1).any()
    src, wg_scale, wg_class, ladder, used = R.user_layout(nat, 512)
    assert np.array_equal(np.sort(src[src >= 0]), np.arange(600)) and len(src) % 512 == 0 and len(src) == 512 * len(wg_scale)
    assert np.array_equal(wg_scale, ladder[wg_class]) and set(np.flatnonzero(used)) == set(wg_class.tolist())
    # every row is quantised with a scale at least its own class's, within the band's factor 2^(1/2): nothing clips beyond what it chose
    a_u = R.rows_of_workgroups(wg_scale, len(src), 512)[src >= 0]
    want = nat[src[src >= 0]]
    assert np.all(a_u[want > 0] >= want[want > 0] * F32(0.9999)) and np.all((a_u <= want * F32(2 ** 0.5 * 1.0001))[want > ladder[63] * 2])


def test_bias_classes_restated():
    b = np.array([1.0, -1.0, 0.3, 0.0, 5.0], F32)
    ladder = np.array([2.0 ** -3, 1e-5, 1e-7], F32)
    bq, sb3, g2 = R.bias_classes(b, np.array([2.0 ** -4, 1e-3], F32), 4, ladder, np.array([1, 0, 1]))
    assert sorted(bq) == [0, 2] and g2 == 5
    assert bq[0].tolist() == [128, -128, 38, 0, 40000]
    assert bq[2][4] == R.BQ_MAX and abs(int(bq[2][0]) - 160_000_000) < 100               # 5 / 1e-10 clamps, 1 / 6.25e-9 does not
    assert sb3[1] >= F32((5 - R.BQ_MAX * 1e-10) / 1e-7) * F32(0.999)                       # the clamped class decides the superblock's error
    one, sb3_one, _ = R.bias_classes(b, np.array([2.0 ** -4, 1e-3], F32), 4, ladder[:1])
    assert np.array_equal(one[0], bq[0]) and np.all(sb3_one <= sb3)


# ------------------------------------------------------------------------------------------------ the rules can fail
@pytest.fixture(scope="module")
def prob():
    c = case("k64-tk10-both-classes")
    W = R.rows_per_workgroup(c.tk)
    p = R.stage_problem(c, W + W // 4 + 5, 5 * 128 + 77, 128)
    p.table = R.stage_table(p)
    p.lb = R.lower_bounds(p.table, R.stage_bound(p))
    p.n_chunks = 3
    p.lists = R.lists(p.lb, p.n_items, p.n_chunks, p.sb_rows, p.tk)
    return p


def as_buffer(want2d, stride, rows=None):
    buf = np.full((rows or want2d.shape[0], stride), SENT, F32)
    buf[:want2d.shape[0], :want2d.shape[1]] = want2d
    return buf


def test_helpers_accept_the_reference(prob):
    p = prob
    R.check_table(as_buffer(p.table, p.n_users + 4), p.table, p.written, SENT, "table")
    n_ch = p.lists.shape[0]
    R.check_lists(as_buffer(p.lists.reshape(n_ch * p.tk, -1), p.n_users + 4, (n_ch + 2) * p.tk), p.lists, p.written, SENT, "lists")
    tg = R.lists(p.lb, p.n_items, p.n_chunks, p.sb_rows, p.tk, tagged=True)
    assert R.chunks(p.n_items, p.n_chunks, p.sb_rows)[0] // p.sb_rows == 2           # chunks of more than one superblock
    R.check_tagged(tg, p.lists, p.lb, p.n_items, p.n_chunks, p.sb_rows, "tagged")
    # the maxima of the superblocks that hold the largest integer biases are beyond 2^24: the conversion rounds
    assert np.abs(p.table[0] / (p.a_u * p.sb_stats[0, 0])).max() > 2 ** 29
    # an overwritten padding cell, and a written column of an idle workgroup
    buf = as_buffer(p.table, p.n_users + 4)
    buf[2, p.n_users + 1] = 0
    with pytest.raises(AssertionError, match="overwritten"):
        R.check_table(buf, p.table, p.written, SENT, "table")
    written = p.written.copy()
    written[p.wg_rows + 3] = False
    with pytest.raises(AssertionError, match="overwritten"):
        R.check_table(as_buffer(p.table, p.n_users + 4), p.table, written, SENT, "table")


def test_helpers_reject_a_cell_off_by_one_unit(prob):
    p = prob
    for s, u in ((0, 0), (3, 700), (p.n_sb - 1, p.n_users - 1)):
        for sign in (1, -1):
            bad = p.table.copy()
            unit = p.a_u[u] * p.sb_stats[s, 0]
            bad[s, u] = F32(bad[s, u] + sign * unit)
            if bad[s, u] == p.table[s, u]:                  # a maximum beyond 2^24 units: one unit is below the rounding of the conversion
                assert abs(p.table[s, u] / unit) > 2 ** 24
                continue
            with pytest.raises(AssertionError, match="differ"):
                R.check_table(as_buffer(bad, p.n_users + 4), p.table, p.written, SENT, "table")
    assert p.table[3, 700] + p.a_u[700] * p.sb_stats[3, 0] != p.table[3, 700]


def test_helpers_reject_the_bias_row_of_the_wrong_class(prob):
    p = prob
    assert sorted(set(p.wg_class.tolist())) == [5, 63]
    swapped = np.where(p.class_u == 5, 63, 5)
    with pytest.raises(AssertionError, match="differ"):
        R.check_table(as_buffer(R.stage_table(p, class_u=swapped), p.n_users + 4), p.table, p.written, SENT, "table")
    # ... and a row nobody prepared (class 0: always class 0 is what a kernel that ignores wg_class reads)
    t0 = R.stage_table(p, class_u=np.zeros_like(p.class_u))
    assert np.abs(t0 - p.table).min() > 1.0
    with pytest.raises(AssertionError, match="differ"):
        R.check_table(as_buffer(t0, p.n_users + 4), p.table, p.written, SENT, "table")


def test_helpers_reject_db_without_the_user_scale(prob):
    p = prob
    lb = R.lower_bounds(p.table, R.stage_bound(p, db_with_scale=False))
    bad = R.lists(lb, p.n_items, p.n_chunks, p.sb_rows, p.tk)
    n_ch = bad.shape[0]
    with pytest.raises(AssertionError, match="differ"):
        R.check_lists(as_buffer(bad.reshape(n_ch * p.tk, -1), p.n_users + 4), p.lists, p.written, SENT, "lists")


def test_helpers_reject_swapped_and_missing_list_entries(prob):
    p = prob
    n_ch = p.lists.shape[0]
    bad = p.lists.copy()
    bad[1, [0, 1], 9] = bad[1, [1, 0], 9]
    assert bad[1, 0, 9] != bad[1, 1, 9]
    with pytest.raises(AssertionError, match="differ"):
        R.check_lists(as_buffer(bad.reshape(n_ch * p.tk, -1), p.n_users + 4), p.lists, p.written, SENT, "lists")
    # the last superblock is a partial one (77 of 128 items): a list made without it
    assert p.n_items % p.sb_rows == 77 and np.all(p.lb[-1] > -np.inf)
    lb = p.lb.copy()
    lb[-1] = -np.inf
    short = R.lists(lb, p.n_items, p.n_chunks, p.sb_rows, p.tk)
    with pytest.raises(AssertionError, match="differ"):
        R.check_lists(as_buffer(short.reshape(n_ch * p.tk, -1), p.n_users + 4), p.lists, p.written, SENT, "lists")
    # a tagged list that names the wrong superblock
    tg = R.lists(p.lb, p.n_items, p.n_chunks, p.sb_rows, p.tk, tagged=True)
    wrong = tg.copy()
    wrong[0, 0, 4] = R.lb_tag(p.lists[0, 0, 4:5], 1 - R.lb_tag_index(tg[0, 0, 4:5]))[0]
    with pytest.raises(AssertionError):
        R.check_tagged(wrong, p.lists, p.lb, p.n_items, p.n_chunks, p.sb_rows, "tagged")


@pytest.mark.parametrize("cid", ["k64-tk10-both-classes", "k128-tk16-none-one_scale", "k64-tk0-user-one_scale"])
def test_helpers_reject_a_dropped_last_k_step(cid):
    c = case(cid)
    W = R.rows_per_workgroup(c.tk)
    for n_users, n_items, sb in ((3, 70, 128), (W + W // 4 + 5, 5 * 512 + 77, 512)):
        p = R.stage_problem(c, n_users, n_items, sb)
        want = R.stage_table(p)
        short = R.stage_table(p, dots=R.int_dots(p.uq[:, :c.kt - 64], p.iq[:, :c.kt - 64]))
        assert (bits_differ := (R.bits(short) != R.bits(want))).mean() > 0.9, bits_differ.mean()
        with pytest.raises(AssertionError, match="differ"):
            R.check_table(as_buffer(short, n_users + 4), want, p.written, SENT, "table")


def test_non_finite_bound_inputs_empty_the_lists(prob):
    p = prob
    r_err = p.r_err.copy()
    r_err[11, 1] = np.nan
    sbs = p.sb_stats.copy()
    sbs[2, 2] = np.inf
    lb = R.lower_bounds(p.table, R.stage_bound(p, r_err=r_err, sb_stats=sbs))
    li = R.lists(lb, p.n_items, 1, p.sb_rows, p.tk)
    assert np.all(np.isneginf(li[:, :, 11])) and np.all(np.isneginf(lb[2]))
    assert np.all(np.isneginf(li[0, p.n_sb - 1:, :])) and np.all(li[0, :p.n_sb - 1, 12] > -np.inf)      # one superblock short for everybody


# ------------------------------------------------------------------------------------------------ the bound holds for the reference alone
BOUND_CASES = [(128, 10, False), (128, 10, True), (40, 16, False), (40, 16, True)]


@pytest.mark.parametrize("d,k,big_bias", BOUND_CASES)
def test_bound_dominates_on_the_reference_pipeline(d, k, big_bias):
    x, y, ub, ib = R.bound_population(d, big_bias, seed=d + k + big_bias)
    P = R.reference_pipeline(x, y, ub, ib, k)
    assert P.n_classes >= 12 and P.real.sum() == len(x)
    r = P.real
    diff, exact_max, m_int = R.observed_error(P.uq[r], P.iq, R.real_groups(P.groups, r), P.a_u[r], P.b_row, P.xs[r], y, P.ubs[r], ib, 512)
    e = f64(P.e)[:, r]
    assert e.shape == diff.shape and np.all(np.isfinite(e))
    assert np.all(diff <= e), float((diff / e).max())
    assert np.median(e / np.maximum(diff, 1e-300)) > 1.0
    # ... so every lower bound the stage would list lies below the exact maximum of its superblock
    table = m_int.astype(F32) * (P.a_u[r][None, :] * P.sbs[:, 0][:, None]) + P.ubs[r][None, :]
    assert table.dtype == F32 and np.all(f64(R.lower_bounds(table, P.e[:, r])) <= exact_max)


# ------------------------------------------------------------------------------------------------ the case table
def test_grid_has_the_size_the_dispatch_code_implies():
    text = open(SRC).read()
    lists_fn = text[text.index("int launch_i8x16_lists("):text.index("// fp32 rows -> int8 rows")]
    forms = re.findall(r"launch_i8x16<KT, BIAS, (\d+), (\d+)>", lists_fn)
    assert sorted((int(a), int(b)) for a, b in forms) == sorted(R.LISTS)
    tops = sorted(int(v) for v in re.findall(r"p\.top_k == (\d+)", lists_fn)) + [16]               # the last form takes what is left: 16
    assert tops == sorted(tk for tk, _ in R.LISTS)
    entry = text[text.index('extern "C" int trec_score_gemm_blockmax_i8('):]
    kb = re.findall(r"launch_i8x16_lists<(\d+), (true|false)>", entry)
    assert sorted(kb) == sorted((str(kt), b) for kt in R.KTS for b in ("true", "false"))
    assert "top_k == 10 || top_k == 16" in entry and "kpad == 64 || kpad == 128" in entry
    n_inst = len(forms) * len(kb)
    g = R.grid()
    assert n_inst == 12 and len({c.instantiation for c in g}) == n_inst
    # bias forms: BIAS = false has one (none), BIAS = true three (user, item, both); two user layouts each
    assert len(g) == len(forms) * len(R.KTS) * (1 + 3) * len(R.LAYOUTS) == 48 and len({c.id for c in g}) == 48
    assert all((c.bias != "none") == c.instantiation[1] for c in g)
    # the workgroup height the layouts are made for
    m = re.search(r"return top_k <= 10 \? NWQ \* (\d+) \* 16 : NWQ \* (\d+) \* 16;", text)
    assert m and [R.rows_per_workgroup(0), R.rows_per_workgroup(10), R.rows_per_workgroup(16)] == [4 * int(m.group(1)) * 16] * 2 + [4 * int(m.group(2)) * 16]
    assert {nub for tk, nub in R.LISTS if tk <= 10} == {int(m.group(1))} and {nub for tk, nub in R.LISTS if tk > 10} == {int(m.group(2))}


def test_prep_grid_names_every_row_kernel_form():
    text = open(SRC).read()
    g = R.prep_grid()
    for kernel, macro in (("prep_i8_kernel", "TREC_PQ"), ("row_natscale_kernel", "row_natscale_kernel<")):
        lanes = {c.lanes for c in g if c.kernel == kernel}
        assert lanes == {8, 16, 32}
    assert set(int(v) for v in re.findall(r"TREC_PQ\((\d+)\);", text)) == {8, 16, 32}
    assert set(int(v) for v in re.findall(r"TREC_PQU\((\d+)\);", text)) == {8, 16, 32}
    assert set(int(v) for v in re.findall(r"hipLaunchKernelGGL\(row_natscale_kernel<(\d+)>", text)) == {8, 16, 32}
    assert len({c.id for c in g}) == len(g) == len(R.PREP_SHAPES) + len(R.NATSCALE_D)
    # the kpad the entry points take is what the dispatch covers: G lanes x 2 x 4 columns
    for kp in range(4, 132, 4):
        if kp <= 64 or kp == 128:
            assert 8 * R.prep_lanes(kp) >= kp
        else:
            with pytest.raises(AssertionError):
                R.prep_lanes(kp)
    assert text.count("kpad <= 64 || kpad == 128") == 2
