"""The float64 references, the bars and the case list of tests/k1_reference.py, checked without the code under test.

* every chain is restated in np.float32 in the kernels' shapes (a lane's chain and a butterfly over the row's lanes; 64 strided lanes) and
  has to lie within its bar of the float64 reference on the inputs of tests/test_gpu_k1.py: a bar that a legitimate float32 order misses
  is too tight;
* the NumPy chain (chain32) equals the C oracle bit for bit;
* the inputs hold what the bars presuppose and the rows they are meant to hold (empty, zero weights, clamped, just not clamped, a ReLU
  pre-activation of exactly 0);
* the case list reaches every instantiation the entry points can launch (ALL_KERNELS), and what each case expects is what pick_kernel says;
* nine seeded defects each push a restatement over its bar (or break equality where the bar is 0)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import k1_reference as R
from k1_reference import F32, U32, f64
from oracle import oracle as O


def tree(lanes):
    """[n, L] lane sums (L a power of two) -> [n]: the xor butterfly's additions"""
    off = lanes.shape[1] >> 1
    while off:
        lanes = lanes[:, :off] + lanes[:, off:2 * off]
        off >>= 1
    return lanes[:, 0]


def lane_dot32(a, b, order):
    """sum_c a_c b_c in float32.  vec4: spmm_csr_vec4_kernel's epilogue (a lane owns four consecutive columns per iteration, rounded products
    added in turn, butterfly over the row's lanes); wave: the row kernels (64 strided lanes, one fmaf per term, butterfly)"""
    n, d = a.shape
    if order == "vec4" and d % 4 == 0 and d <= 1024:
        lpr, iters = R.vec4_lanes(d)
        pad = iters * lpr * 4 - d
        a, b = np.pad(a, ((0, 0), (0, pad))), np.pad(b, ((0, 0), (0, pad)))
        a = a.reshape(n, iters, lpr, 4).transpose(0, 2, 1, 3).reshape(n, lpr, iters * 4)
        b = b.reshape(n, iters, lpr, 4).transpose(0, 2, 1, 3).reshape(n, lpr, iters * 4)
        acc = np.zeros((n, lpr), F32)
        for k in range(iters * 4):
            acc = acc + a[:, :, k] * b[:, :, k]
        return tree(acc)
    pad = -d % 64
    a, b = np.pad(a, ((0, 0), (0, pad))), np.pad(b, ((0, 0), (0, pad)))
    a, b = a.reshape(n, -1, 64), b.reshape(n, -1, 64)
    acc = np.zeros((n, 64), F32)
    for k in range(a.shape[1]):
        acc = R.fmaf32(a[:, k], b[:, k], acc)
    return tree(acc)


def norm32(r, order, defect=None):
    ss = lane_dot32(r, r, order)
    if defect == "stray":                                   # the sum runs over a neighbour's column as well
        ss = ss + np.roll(r[:, 0], -1) ** 2
    if defect == "clamp_norm":
        inv = F32(1.0) / np.maximum(np.sqrt(ss), R.EPS32)
    else:
        inv = F32(1.0) / np.sqrt(np.maximum(ss, R.EPS32))
    return r * inv[:, None], inv


def bwd32(y, inv, dy, order):
    t = lane_dot32(y, dy, order)
    t = np.where(inv >= R.INV_EPS32, F32(0), t)
    return (dy - y * t[:, None]) * inv[:, None]


def rowsum32(indptr, values, order, base=None, skip_first=False):
    """seq: the gather's own chain; lanes16: segsum_csr_kernel"""
    n = indptr.size - 1
    lens = np.diff(indptr)
    lanes = np.zeros((n, 16 if order == "lanes16" else 1), F32)
    for k in range(1 if skip_first else 0, int(lens.max())):
        rows = np.nonzero(lens > k)[0]
        lanes[rows, k % lanes.shape[1]] += values[indptr[rows] + k]
    s = tree(lanes)
    return s if base is None else base + s


def colsum32(x):
    acc = np.zeros((4, x.shape[1]), F32)
    for r in range(x.shape[0]):
        acc[r % 4] += x[r]
    return (acc[0] + acc[1]) + (acc[2] + acc[3])


def stats32(chain, err, order):
    return np.stack([np.sqrt(lane_dot32(chain, chain, order)), np.sqrt(lane_dot32(err, err, order))], 1)


def within(got, want, bar, what):
    err = np.abs(f64(got) - f64(want))
    bar = np.broadcast_to(f64(bar), err.shape)
    bad = err > bar
    assert not bad.any(), "%s: worst ratio %.2f" % (what, float((err[bad] / np.maximum(bar[bad], 1e-300)).max()))
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(err == 0, 0.0, err / bar).max())


def outside(got, want, bar):
    return bool((np.abs(f64(got) - f64(want)) > bar).any())


@functools.lru_cache(maxsize=None)
def exact(case_id):
    case = CASE_BY_ID[case_id]
    m = case.matrix()
    _, _, vals = R.case_values(case)
    return O.spmm_exact(sp.csr_matrix((vals, m.indices, m.indptr), shape=m.shape), R.weights(m.shape[1], case.d))


CASE_BY_ID = {c.id: c for c in R.CASES}


# ------------------------------------------------------------------------------------------------ the case list
def test_case_ids_are_unique():
    assert len(CASE_BY_ID) == len(R.CASES)


def test_cases_reach_every_instantiation():
    reached = set()
    for case in R.CASES:
        m = case.matrix()
        for l in case.launches:
            got = R.pick_kernel(m.shape[0], m.nnz, case.d, l.epi, l.accumulate, l.tuning, l.entry)
            assert got == l.expect, "%s epilogue %d: the table says %r, the dispatch rule %r" % (case.id, l.epi, l.expect, got)
            reached.add(got)
    assert reached == R.ALL_KERNELS, (sorted(R.ALL_KERNELS - reached), sorted(reached - R.ALL_KERNELS))
    assert len(R.ALL_KERNELS) == 42 + 4 + 3


def test_short_csr_shapes():
    """0..4 non-zeros per row, rows 1 and n - 1 empty; mean 2 keeps the weight loads cached (4 nnz > 5 n), mean 1 does not"""
    for n in (4096, 4097, 4099):
        for mean in (2, 1):
            m = R.short_csr(n, R.F_BIG, R.SEED, mean)
            lens = np.diff(m.indptr)
            assert lens.max() == 4 and lens[1] == 0 and lens[n - 1] == 0 and set(lens) == {0, 1, 2, 3, 4}
            assert m.nnz <= 4 * n and (4 * m.nnz > 5 * n) == (mean == 2), (n, mean, m.nnz)
            assert m.indices.min() >= 0 and m.indices.max() < R.F_BIG
    # the seeded draw itself, so that a change of the builder shows: short rows with cached weight loads / with non-temporal ones
    assert (R.short_csr(4099, 977, R.SEED, 2).nnz, R.short_csr(4099, 977, R.SEED, 1).nnz) == (8304, 4073)
    p = R.prefix_csr(R.short_csr(4099, R.F_BIG, R.SEED, 2), 4095)
    assert p.shape[0] == 4095 and np.array_equal(p.toarray(), R.short_csr(4099, R.F_BIG, R.SEED, 2)[:4095].toarray())
    lens = np.diff(R.long_rows_csr().indptr)
    assert list(lens) == [0, 1, 64, 65, 200]


def test_input_conditions():
    """every matrix / width of the case list (one_per_row has no planted rows: it is the plain chain)"""
    seen = set()
    for case in R.CASES:
        m = case.matrix()
        key = (m.shape, m.nnz, case.d)
        if case.group == "one_per_row" or key in seen:
            continue
        seen.add(key)
        cond = R.input_conditions(m, R.weights(m.shape[1], case.d), R.bias(case.d))
        assert cond["values_in_range"] and cond["weights_in_range"] and cond["clamp_band_clear"], (case.id, cond)
        assert cond["empty_rows"] >= 2 and cond["zero_row"] and cond["clamped_row"] and cond["small_row"], (case.id, cond)
        assert cond["relu_zero_rows"] == [R.ROW_RELU0] and cond["relu_zero_elsewhere"] == 0, (case.id, cond)
    # the ReLU margin is what the backward mask needs: asserted where a mask is taken, the towers (the forward is the chain bit for bit)
    for name, d in R.TOWER_CASES:
        m = R.tower_matrix(name)
        cond = R.input_conditions(m, R.weights(m.shape[1], d, R.TOWER_SEED), R.bias(d, R.TOWER_SEED))
        assert cond["clamp_band_clear"] and cond["relu_margin"] >= 8.0 and cond["relu_zero_rows"] == [R.ROW_RELU0], (name, d, cond)


# ------------------------------------------------------------------------------------------------ restatements within the bars
@pytest.mark.parametrize("case", [c for c in R.CASES if c.group in ("r4", "r4wide", "r1", "scalar", "r4perm", "r4plain")
                                  and not c.id.startswith(("r4-n4096", "r4-n4097"))], ids=lambda c: c.id)
def test_gather_epilogues_within_bars(case):
    m = case.matrix()
    n, d = m.shape[0], case.d
    W, b = R.weights(m.shape[1], d), R.bias(d)
    _, _, vals = R.case_values(case)
    mv = sp.csr_matrix((vals, m.indices, m.indptr), shape=m.shape)
    chain = exact(case.id)
    assert np.array_equal(R.chain32(m.indptr, m.indices, vals, W), chain), "the NumPy chain is not the C oracle's"
    ref, bar = R.gather_ref(mv, W)
    within(chain, ref, bar, case.id + " gather")
    epis = {l.epi for l in case.launches}
    if any(l.accumulate for l in case.launches):
        base, rs_base = R.accumulate_base(n, d)
        ref, bar = R.gather_ref(mv, W, base)
        within(R.chain32(m.indptr, m.indices, vals, W, base), ref, bar, case.id + " accumulate")
        s, sbar = R.segsum_ref(m.indptr, vals, rs_base)
        for order in ("seq", "lanes16"):
            within(rowsum32(m.indptr, vals, order, rs_base), s, sbar, case.id + " row sums on a base, " + order)
    if 1 in epis:
        nr = R.normalize_ref(chain)
        for order in ("vec4", "wave"):
            y, inv = norm32(chain, order)
            within(y, nr.y, nr.bar_y, "%s normalise %s" % (case.id, order))
            within(inv, nr.inv, nr.bar_inv, "%s inv %s" % (case.id, order))
            zero = nr.ss == 0
            assert zero.sum() >= 3 and (y[zero] == 0).all() and (inv[zero] == R.INV_EPS32).all()
    if 2 in epis:
        t = R.relu_tower_ref(mv, W, b, np.zeros(chain.shape))
        within(np.maximum(chain + b, F32(0)), t.out, t.bar_out, case.id + " bias + ReLU")
    if 3 in epis:
        s, sbar = R.segsum_ref(m.indptr, vals)
        for order in ("seq", "lanes16"):
            within(rowsum32(m.indptr, vals, order), s, sbar, "%s row sums %s" % (case.id, order))


@pytest.mark.parametrize("case", [c for c in R.CASES if c.group == "filter" and "n4096" not in c.id], ids=lambda c: c.id)
def test_filter_stats_within_bars(case):
    chain = exact(case.id)
    fr = R.filter_ref(chain)
    assert np.array_equal(R.bf16_back(fr.bits).view(np.uint32) & 0xFFFF, np.zeros(chain.shape, np.uint32))
    assert (np.abs(f64(fr.err)) <= 2.0 ** -8 * np.abs(f64(chain))).all()               # half a bf16 ulp at most
    for order in ("vec4", "wave"):
        within(stats32(chain, fr.err, order), fr.stats, fr.bar, "%s stats %s" % (case.id, order))
    empty = np.diff(case.matrix().indptr) == 0
    assert (fr.stats[empty] == 0).all()


def test_bf16_rounding_is_to_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -23, -1.0 - 2.0 ** -8, 1.0 + 2.0 ** -8 - 2.0 ** -23], F32)
    assert list(R.bf16_bits(x)) == [0x3F80, 0x3F80, 0x3F82, 0x3F81, 0xBF80, 0x3F80]     # ties go to even; just above and below a tie


def test_fmaf32_is_correctly_rounded():
    """(1 + 2^-23) * 2^-24 (1 - 2^-23) = 2^-24 (1 - 2^-46): added to 1 + 2^-23 it lies just below the tie and rounds down; the float64 sum
    is the tie itself, and rounding that to float32 goes to even, one ulp up"""
    a, b, c = F32(1.0 + 2.0 ** -23), F32(2.0 ** -24) * F32(1.0 - 2.0 ** -23), F32(1.0 + 2.0 ** -23)
    assert (f64(a) * f64(b) + f64(c)).astype(F32) == F32(1.0 + 2.0 ** -22)
    assert R.fmaf32(a, b, c)[0] == c and R.fmaf32(-a, b, -c)[0] == -c
    assert R.fmaf32(a, F32(2.0 ** -24) * F32(1.0 + 2.0 ** -23), F32(1.0))[0] == F32(1.0 + 2.0 ** -23)      # just above the tie: up
    rng = np.random.default_rng(0)
    v, w, acc = (rng.standard_normal(100000).astype(F32) for _ in range(3))
    assert (R.fmaf32(v, w, acc) == (f64(v) * f64(w) + f64(acc)).astype(F32)).mean() > 0.9999


@pytest.mark.parametrize("n,d", R.ROWNORM_CASES)
def test_row_normalise_within_bars(n, d):
    x, dy = R.dense_rows(n, d, R.SEED), R.gradient(n, d, 3)
    nr = R.normalize_ref(x)
    if n >= 16:
        assert nr.clamped[R.ROW_CLAMPED] and not nr.clamped[R.ROW_SMALL] and (nr.ss[[1, n - 1]] == 0).all()
        ordinary = np.ones(n, bool)
        ordinary[[1, n - 1, R.ROW_CLAMPED, R.ROW_SMALL]] = False
        assert (nr.ss[ordinary] > 4e-12).all()
    y32, inv32 = R.l2norm_bwd_inputs(nr)
    dx, bar = R.l2norm_bwd_ref(nr, dy)
    for order in ("wave", "vec4"):
        y, inv = norm32(x, order)
        within(y, nr.y, nr.bar_y, "normalise " + order)
        within(inv, nr.inv, nr.bar_inv, "inv " + order)
        assert (inv[nr.clamped] == R.INV_EPS32).all()
        within(bwd32(y32, inv32, dy, order), dx, bar, "backward " + order)


@pytest.mark.parametrize("name,d", R.TOWER_CASES)
def test_towers_within_bars(name, d):
    m = R.tower_matrix(name)
    n, F = m.shape
    W, b, g = R.weights(F, d, R.TOWER_SEED), R.bias(d, R.TOWER_SEED), R.gradient(n, d, 5)
    t = sp.csr_matrix(m.T)
    t.sort_indices()
    chain = R.chain32(m.indptr, m.indices, m.data, W)
    nt = R.norm_tower_ref(m, W, g)
    for order in ("vec4", "wave"):
        y, inv = norm32(chain, order)
        within(y, nt.y, nt.bar_y, "normalise tower y " + order)
        dx = bwd32(y, inv, g, order)
        within(dx, nt.dx, nt.bar_dx, "normalise tower dx " + order)
        within(R.chain32(t.indptr, t.indices, t.data, dx), nt.dW, nt.bar_dW, "normalise tower dW " + order)
    rt = R.relu_tower_ref(m, W, b, g)
    out = np.maximum(chain + b, F32(0))
    within(out, rt.out, rt.bar_out, "ReLU tower out")
    dpre = np.where(out > 0, g, F32(0))
    assert np.array_equal(f64(dpre), rt.dpre) and (dpre[R.ROW_RELU0] == 0).all()
    within(R.chain32(t.indptr, t.indices, t.data, dpre), rt.dW, rt.bar_dW, "ReLU tower dW")
    within(colsum32(dpre), rt.db, rt.bar_db, "ReLU tower db")
    cs, cbar = R.colsum_ref(dpre)
    within(colsum32(dpre), cs, cbar, "column sums")


def test_long_row_sums_within_bars():
    m = R.long_rows_csr()
    s, bar = R.segsum_ref(m.indptr, m.data)
    for order in ("seq", "lanes16"):
        within(rowsum32(m.indptr.astype(np.int64), m.data, order), s, bar, order)


# ------------------------------------------------------------------------------------------------ seeded defects
def _defect_inputs(d=128, mean=2):
    m = R.short_csr(4099, R.F_BIG, R.SEED, mean)
    return m, R.weights(R.F_BIG, d), O.spmm_exact(m, R.weights(R.F_BIG, d))


def test_defect_odd_last_nonzero_dropped():
    """the pairwise loop's tail: a row of 2 or 4 entries loses its last one"""
    m, W, chain = _defect_inputs()
    lens = np.diff(m.indptr)
    keep = np.ones(m.nnz, bool)
    hit = (lens >= 2) & (lens % 2 == 0)
    keep[m.indptr[1:][hit] - 1] = False
    indptr = np.concatenate([[0], np.cumsum(lens - hit)]).astype(np.int64)
    assert hit.sum() > 100 and not np.array_equal(R.chain32(indptr, m.indices[keep], m.data[keep], W), chain)


def test_defect_column_tail_left_zero():
    for d in (100, 260, 768):
        m, W, chain = _defect_inputs(d)
        bad = chain.copy()
        bad[:, d - 4:] = 0
        assert not np.array_equal(bad, chain)


def test_defect_neighbour_rows_value_in_a_batch():
    m, W, chain = _defect_inputs()
    lens = np.diff(m.indptr)
    r = np.nonzero((lens[:-1] > 0) & (lens[1:] > 0) & (np.arange(m.shape[0] - 1) % 4 != 3))[0]
    vals = m.data.copy()
    vals[m.indptr[r]] = m.data[m.indptr[r + 1]]
    assert not np.array_equal(R.chain32(m.indptr, m.indices, vals, W), chain)


def test_defect_row_sum_misses_first_entry():
    m, _, _ = _defect_inputs()
    s, bar = R.segsum_ref(m.indptr, m.data)
    assert outside(rowsum32(m.indptr.astype(np.int64), m.data, "seq", skip_first=True), s, bar)


def test_defect_stray_term_in_the_norm():
    for d in (4, 100, 128, 1024):
        _, _, chain = _defect_inputs(d)
        nr = R.normalize_ref(chain)
        y, inv = norm32(chain, "vec4", defect="stray")
        assert outside(y, nr.y, nr.bar_y) and outside(inv, nr.inv, nr.bar_inv)


def test_defect_clamp_on_the_norm():
    _, _, chain = _defect_inputs()
    nr = R.normalize_ref(chain)
    y, inv = norm32(chain, "vec4", defect="clamp_norm")
    err = np.abs(f64(y) - nr.y) > nr.bar_y
    assert err[R.ROW_CLAMPED].any() and not err[R.ROW_SMALL].any() and outside(inv, nr.inv, nr.bar_inv)


def test_defect_relu_gradient_passes_at_zero():
    for name in ("4099x977", "150x40"):
        m = R.tower_matrix(name)
        n, F = m.shape
        W, b, g = R.weights(F, 12, R.TOWER_SEED), R.bias(12, R.TOWER_SEED), R.gradient(n, 12, 5)
        rt = R.relu_tower_ref(m, W, b, g)
        pre = R.chain32(m.indptr, m.indices, m.data, W) + b
        dpre = np.where(pre >= 0, g, F32(0))                                     # >= instead of >
        t = sp.csr_matrix(m.T)
        t.sort_indices()
        assert outside(R.chain32(t.indptr, t.indices, t.data, dpre), rt.dW, rt.bar_dW)
        assert (rt.bar_dW[F - R.N_SPECIAL] == 0).all()                           # the planted row's feature: exactly 0 is asked for


def test_defect_accumulate_ignores_the_base():
    m, W, chain = _defect_inputs(64)
    base, rs_base = R.accumulate_base(4099, 64)
    assert not np.array_equal(R.chain32(m.indptr, m.indices, m.data, W, base), chain)
    s, bar = R.segsum_ref(m.indptr, m.data, rs_base)
    assert outside(rowsum32(m.indptr.astype(np.int64), m.data, "seq"), s, bar)


def test_defect_val_perm_ignored():
    case = next(c for c in R.CASES if c.group == "r4perm")
    m = case.matrix()
    store, perm, vals = R.case_values(case)
    W = R.weights(m.shape[1], case.d)
    assert not np.array_equal(R.chain32(m.indptr, m.indices, store[:m.nnz], W), exact(case.id))
    s, bar = R.segsum_ref(m.indptr, vals)
    assert outside(rowsum32(m.indptr.astype(np.int64), store[:m.nnz], "seq"), s, bar)
