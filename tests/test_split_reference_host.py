"""tests/split_reference.py checked on the CPU, without the kernels of csrc/spmm_split.hip:

* hand-worked cases in which the chunked order, the whole-row chain and the reversed order round differently;
* rows at or below the threshold are k1_reference.chain32 and the C oracle (oracle.spmm_exact) bit for bit;
* the reference lies within (m + 1) u sum |terms| of float64 on every case: it is itself a correct sum;
* the case list reaches all 18 rows / chunks forms and all 6 reduce forms (through pick_split), each of them with `own`, with accumulate +
  rowsum and on a matrix that holds every chunk tail 1 .. 8; the stride cases exceed the caps of the restated launch arithmetic, and no case
  lists more chunks or long rows than the workspace is sized for;
* every seeded defect (`bug=`) changes the result on the case inputs;
* the host query trec_csr_split_workspace_bytes equals the restated layout and refuses a threshold below 2."""
import numpy as np
import pytest

import split_reference as R
from k1_reference import F32, chain32, f64
from oracle import oracle as O

E = F32(2.0 ** -24)            # half an ulp of 1


def one_row(vals, d=1):
    n = len(vals)
    return np.array([0, n], np.int64), np.arange(n, dtype=np.int32), np.array(vals, F32), np.ones((n, d), F32)


# ------------------------------------------------------------------------------------------------ the launch rule
def test_pick_split_restates_the_launch_rule():
    want = {4: (1, 4), 12: (1, 4), 256: (1, 4), 260: (2, 4), 512: (2, 4), 516: (4, 4), 768: (4, 4), 772: (4, 4), 1024: (4, 4),
            1: (1, 1), 5: (1, 1), 63: (1, 1), 64: (1, 4), 65: (2, 1), 126: (2, 1), 129: (4, 1), 190: (4, 1), 193: (4, 1), 255: (4, 1)}
    for d, (iters, vec) in want.items():
        assert R.pick_split(d) == (iters, False, vec, False), d
        assert R.pick_split(d, perm=True) == (iters, False, vec, True) and R.pick_split(d, packed=True) == (iters, True, vec, False)
        assert R.pick_split(d, packed=True, perm=True) == (iters, True, vec, False)            # packed entries carry their values
    assert [R.lanes_of(d)[0] for d in (4, 12, 256, 1024, 1, 5, 63, 65, 255)] == [1, 4, 64, 64, 1, 8, 64, 64, 64]
    assert all(R.accepts(d) for d in (1, 3, 255, 256, 260, 1024)) and not any(R.accepts(d) for d in (0, -4, 257, 258, 1025, 1028, 2048))
    assert len(R.ALL_SPLIT_KERNELS) == 18 and len(R.ALL_REDUCE_KERNELS) == 6


def test_cases_reach_every_instantiation():
    assert len(R.CASE_BY_ID) == len(R.CASES)
    reached, with_own, with_acc_rs, with_tails, reduce = set(), set(), set(), set(), set()
    for case in R.CASES:
        assert R.accepts(case.d)
        for l in case.launches:
            packed, perm = R.SOURCES[l.source]
            form = R.pick_split(case.d, packed, perm)
            reached.add(form)
            reduce.add((form[0], form[2]))
            if l.own:
                with_own.add(form)
            if l.accumulate and l.rowsum:
                with_acc_rs.add(form)
            if case.group == "widths":
                with_tails.add(form)
    assert reached == with_own == with_acc_rs == with_tails == R.ALL_SPLIT_KERNELS
    assert reduce == R.ALL_REDUCE_KERNELS
    # 3 runs as 4: widths whose fourth iteration is dead, in both lane types
    assert R.lanes_of(516)[1] == R.lanes_of(768)[1] == R.lanes_of(129)[1] == R.lanes_of(190)[1] == 4
    for case in R.CASES:
        if case.group == "widths":
            names = {l.name for l in case.launches}
            assert set(R.PRODUCTION) <= names, case.id
    # the route of ops._prefer_split: single-column lanes, two iterations, values through val_perm
    assert R.pick_split(70, perm=True) == (2, False, 1, True)
    # every pair of options in all four combinations
    for a, b in ((1, 2), (1, 3), (2, 3)):
        assert {(o[a], o[b]) for o in R.OPTIONS} == {(False, False), (False, True), (True, False), (True, True)}


def test_row_lengths_reach_every_tail_and_edge():
    m = R.lens_csr(R.LENS16, R.N_COLS16, 16)
    lens = np.diff(m.indptr)
    assert tuple(lens) == R.LENS16 and m.shape == (25, 1500)
    assert set(R.LENS16) >= {0, 1, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 100, 1000}
    st = R.chunks_of(m.indptr, 16)
    assert st.chunk == 8 and list(np.nonzero(st.long)[0]) == [0] + list(range(5, 14)) + [16, 24]
    tails = {int((st.end - st.start)[st.first[r] + st.nch[r] - 1]) for r in np.nonzero(st.long)[0]}
    assert tails == {1, 2, 3, 4, 5, 6, 7, 8}                       # scalar only (1 .. 3), a pipelined block (4), a block and 1 .. 3 (5 .. 7), two
    assert st.long[0] and st.long[-1] and any(st.long[r] and lens[r + 1] == 0 for r in range(24))
    assert (lens[~st.long] <= 16).all() and (lens == 16).sum() >= 2 and not st.long[lens == 16].any()
    for t, chunk, n_long in ((2, 1, 19), (3, 1, 18), (5, 2, 18), (16, 8, 12), (17, 8, 10)):
        st = R.chunks_of(m.indptr, t)
        assert st.chunk == chunk and st.long.sum() == n_long, t
        assert np.array_equal(np.bincount(st.row, weights=st.end - st.start, minlength=25), lens)      # the chunks tile the rows
    d = np.diff(R.lens_csr(R.LENS_DEFAULT, R.N_COLS_DEFAULT, 2048).indptr)
    st = R.chunks_of(np.concatenate([[0], np.cumsum(d)]), R.SPLIT_T_DEFAULT)
    assert list(st.long) == [True, False, False, False, True] and list(st.nch) == [3, 1, 1, 1, 5] and st.chunk == 1024


def test_plan_bounds_hold_and_stride_cases_exceed_the_caps():
    """no case lists more chunks / long rows than plan_layout sizes the workspace for (the kernels write these lists unchecked); the stride
    cases exceed the fixed grids, so that the grid-stride loops take a second step"""
    seen = [(c.matrix(), c.split_t) for c in R.CASES] + [(c.matrix(), c.split_t) for c in R.SPMV_CASES]
    for m, t in seen:
        st = R.chunks_of(m.indptr, t)
        max_long, max_chunks = R.plan_bounds(m.nnz, t)
        assert int(st.nch[st.long].sum()) <= max_chunks and int(st.long.sum()) <= max_long, (m.shape, t)
        assert m.indices.min() >= 0 and m.indices.max() < m.shape[1]
    m = R.CASE_BY_ID["stride-t4-d256"].matrix()
    st = R.chunks_of(m.indptr, R.STRIDE_T)
    n_chunks, n_long = int(st.nch[st.long].sum()), int(st.long.sum())
    g = R.gather_grid(m.nnz, R.STRIDE_D, R.STRIDE_T)
    assert (n_chunks, n_long) == (24600, 8200) and (g.chunk_subgroups, g.reduce_subgroups) == (16384, 8192)
    assert g.chunk_subgroups < n_chunks < 2 * g.chunk_subgroups and g.reduce_subgroups < n_long
    assert set(st.nch) == {3} and set(st.end - st.start) == {1, 2}                                  # three chunks per five non-zeros
    s = R.spmv_grid(m.nnz, R.STRIDE_T)
    assert s.chunk_waves == 16384 < n_chunks
    big = R.SPMV_CASE_BY_ID["stride-reduce"].matrix()
    s = R.spmv_grid(big.nnz, R.STRIDE_T)
    assert s.reduce_threads == 262144 < big.shape[0] == 262200 and s.chunk_waves == 16384
    # the ordinary cases stay under the caps: one step
    m16 = R.lens_csr(R.LENS16, R.N_COLS16, 16)
    assert R.gather_grid(m16.nnz, 256, 16).chunk_subgroups >= R.plan_bounds(m16.nnz, 16)[1]


# ------------------------------------------------------------------------------------------------ by hand
def test_hand_worked_gather():
    """split_t = 4, a row of 1, e, e, e, e (e = 2^-24) against weights of 1: the whole chain stays at 1 (every add is a tie that goes to
    even); the chunks are 1 + e = 1, e + e = 2^-23 and e; (0 + 1) + 2^-23 = 1 + 2^-23, + e is a tie that goes to 1 + 2^-22 -- the float64 sum"""
    indptr, idx, v, W = one_row([1, E, E, E, E], d=3)
    out, rs = R.split_gather_ref(indptr, idx, v, W, 4)
    assert (out == F32(1 + 2.0 ** -22)).all() and rs[0] == F32(1 + 2.0 ** -22)
    whole, _ = R.split_gather_ref(indptr, idx, v, W, 4, bug="whole")
    assert (whole == 1).all() and np.array_equal(whole, chain32(indptr, idx, v, W))
    assert np.array_equal(R.split_gather_ref(indptr, idx, v, W, 5)[0], whole)                       # five non-zeros are short at split_t = 5
    # reversed: e + 2^-23 = 3 e, + 1 rounds to 1 + 2^-22 as well; with split_t = 2 (chunks of 1): ((1 + e) + e) ... = 1, reversed 1 + 2^-22
    assert (R.split_gather_ref(indptr, idx, v, W, 2)[0] == 1).all()
    assert (R.split_gather_ref(indptr, idx, v, W, 2, bug="reverse")[0] == F32(1 + 2.0 ** -22)).all()
    # a base: a short row chains from it, a long row adds its partials onto it
    base = np.full((1, 3), 2.0, F32)
    out, rs = R.split_gather_ref(indptr, idx, v, W, 4, base=base, base_rowsum=np.array([4.0], F32))
    assert (out == F32(3)).all() and rs[0] == F32(5)                                                 # 2 + 1 = 3, + 2^-23 and + e are lost
    out, _ = R.split_gather_ref(indptr, idx, np.array([1, 2, 3, 4, 5], F32), W, 5, base=base)
    assert (out == 17).all()
    # own: v (own - w), the difference rounded once: 1 - 3 * 2^-26 rounds to 1 - 2^-24
    indptr, idx, v, _ = one_row([2, 4, 8])
    W = np.array([[1], [2], [F32(3 * 2.0 ** -26)]], F32)
    own = np.array([[3.0]], F32)
    out, rs = R.split_gather_ref(indptr, idx, v, W, 2, own=own)
    assert out[0, 0] == 2 * 2 + 4 * 1 + 8 * 3 and rs[0] == 14
    out, _ = R.split_gather_ref(indptr, idx, v, W, 2, own=np.array([[1.0]], F32))
    assert out[0, 0] == F32(0 - 4 + 8 * (1 - 2.0 ** -24))
    # an empty row is zero, or its base
    out, rs = R.split_gather_ref(np.array([0, 0, 0], np.int64), np.zeros(0, np.int32), np.zeros(0, F32), np.ones((2, 2), F32), 2,
                                 base=np.full((2, 2), 7.0, F32), base_rowsum=np.array([1.0, 2.0], F32))
    assert (out == 7).all() and list(rs) == [1, 2]


def test_hand_worked_spmv():
    """16 lanes and the butterfly 8, 4, 2, 1 on a short row: lane 0 = 1, lanes 4, 8, 12 = e: (1 + e) = 1 meets (e + e) = 2^-23: 1 + 2^-23 -- a
    chain in entry order stays at 1.  A chunk of 8 in 64 lanes: the butterfly 32, 16, 8 adds zeros, then the same picture at 4, 2, 1."""
    v = np.zeros(13, F32)
    v[[0, 4, 8, 12]] = [1, E, E, E]
    indptr, idx, v, _ = one_row(list(v))
    assert R.split_spmv_ref(indptr, idx, v, 16)[0] == F32(1 + 2.0 ** -23)
    ones = np.ones(13, F32)
    assert R.split_spmv_ref(indptr, idx, v, 16, beta=ones)[0] == 1                                   # with beta: one fmaf chain
    v = np.zeros(17, F32)
    v[[0, 2, 4, 6, 16]] = [1, E, E, E, E]
    indptr, idx, v, _ = one_row(list(v))
    for beta in (None, np.ones(17, F32)):
        # chunk 0: (1 + e) + (e + e) = 1 + 2^-23; chunk 1: 0; chunk 2: e; 0 + (1 + 2^-23) + 0 + e: a tie that goes to 1 + 2^-22
        assert R.split_spmv_ref(indptr, idx, v, 16, beta=beta)[0] == F32(1 + 2.0 ** -22)
    assert R.split_spmv_ref(indptr, idx, v, 16, bug="whole")[0] == F32(1 + 2.0 ** -23)                # 16 lanes: lane 0 = (1 + e), 2, 4, 6 = e
    # strided lanes: entry 16 of a short row returns to lane 0
    v = np.zeros(17, F32)
    v[[0, 16, 8]] = [1, E, 2 * E]
    indptr, idx, v, _ = one_row(list(v))
    assert R.split_spmv_ref(indptr, idx, v, 17)[0] == F32(1 + 2.0 ** -23)                            # (1 + e) = 1, + 2 e
    # perm: values are read through it
    assert R.split_spmv_ref(indptr, idx, v[::-1].copy(), 17, val_perm=np.arange(16, -1, -1))[0] == F32(1 + 2.0 ** -23)


# ------------------------------------------------------------------------------------------------ short rows, the float64 bar
@pytest.mark.parametrize("d", [4, 12, 65, 260])
def test_short_rows_are_the_chain_and_the_oracle(d):
    m = R.lens_csr(R.LENS16, R.N_COLS16, 16)
    W = R.weights(R.N_COLS16, d)
    exact = O.spmm_exact(m, W)
    assert np.array_equal(exact, chain32(m.indptr, m.indices, m.data, W))
    out, rs = R.split_gather_ref(m.indptr, m.indices, m.data, W, 16)
    short = np.diff(m.indptr) <= 16
    assert short.sum() == 13 and np.array_equal(out[short], exact[short]) and (out[np.diff(m.indptr) == 0] == 0).all()
    assert not np.array_equal(out[~short], exact[~short])
    whole, rs_whole = R.split_gather_ref(m.indptr, m.indices, m.data, W, 1000)                       # nothing is long: the oracle's chain
    assert np.array_equal(whole, exact) and np.array_equal(rs[short], rs_whole[short])
    base = R.rows_f32(25, d, 7)
    acc, _ = R.split_gather_ref(m.indptr, m.indices, m.data, W, 16, base=base)
    assert np.array_equal(acc[short], chain32(m.indptr, m.indices, m.data, W, base)[short])
    store, perm = R.perm_values(m)
    assert np.array_equal(store[perm], m.data) and not np.array_equal(store[:m.nnz], m.data)
    assert np.array_equal(R.split_gather_ref(m.indptr, m.indices, store, W, 16, val_perm=perm)[0], out)


def within(got, want, bar, what):
    err = np.abs(f64(got) - f64(want))
    bad = err > bar
    assert not bad.any(), "%s: worst ratio %.2f" % (what, float((err[bad] / np.maximum(bar[bad], 1e-300)).max()))


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_reference_within_the_float64_bar(case):
    x = R.case_inputs(case)
    for own, acc in sorted({(l.own, l.accumulate) for l in case.launches}):
        out, rs = R.expected(case.id, own, acc)
        ref = R.split_gather_f64(x.m.indptr, x.m.indices, x.m.data, x.W, own=x.own if own else None, base=x.base if acc else None,
                                 base_rowsum=x.base_rowsum if acc else None)
        within(out, ref.out, ref.bar, "%s own %d accumulate %d" % (case.id, own, acc))
        within(rs, ref.rowsum, ref.bar_rowsum, "%s row sums" % case.id)
        empty = np.diff(x.m.indptr) == 0
        assert np.array_equal(out[empty], x.base[empty] if acc else np.zeros_like(out[empty]))


@pytest.mark.parametrize("case", R.SPMV_CASES, ids=lambda c: c.id)
def test_spmv_reference_within_the_float64_bar(case):
    m = case.matrix()
    beta = R.beta_of(m.shape[1])
    store, perm = R.perm_values(m)
    for with_beta in (True, False):
        out = R.expected_spmv(case.id, with_beta)
        s, bar = R.spmv_f64(m.indptr, m.indices, m.data, beta=beta if with_beta else None)
        within(out, s, bar, "%s beta %d" % (case.id, with_beta))
    if m.shape[0] < 100:
        assert np.array_equal(R.split_spmv_ref(m.indptr, m.indices, store, case.split_t, val_perm=perm, beta=beta), R.expected_spmv(case.id, True))


# ------------------------------------------------------------------------------------------------ seeded defects
SHARE_FLOOR = 0.2


def test_every_seeded_defect_changes_the_result():
    """Share of the long rows' elements whose bits differ from the reference's, LENS16 at split_t = 16 (measured with this file):

        d       whole   chunk_t  reverse
        12      0.715   0.576    0.444
        65      0.726   0.579    0.432
        130     0.719   0.562    0.417
        260     0.712   0.576    0.406
        516     0.707   0.560    0.409

    The floor is half of the smallest (0.406), rounded down: 0.2.  The other defects touch few rows (the rows of exactly 16, the rows with a partial
    tail, the long rows' sums) and have to change at least one element of each of them."""
    m = R.lens_csr(R.LENS16, R.N_COLS16, 16)
    lens = np.diff(m.indptr)
    long = lens > 16
    base_rs = R.base_rowsum(25)
    for d in (12, 65, 130, 260, 516):
        W, own, base = R.weights(R.N_COLS16, d), R.rows_f32(25, d, 3), R.rows_f32(25, d, 7)
        args = (m.indptr, m.indices, m.data, W, 16)
        out, rs = R.split_gather_ref(*args)
        shares = {}
        for bug in ("whole", "chunk_t", "reverse"):
            bad, bad_rs = R.split_gather_ref(*args, bug=bug)
            assert np.array_equal(bad[~long], out[~long]) and np.array_equal(bad_rs[~long], rs[~long])
            shares[bug] = float((bad[long] != out[long]).mean())
            assert shares[bug] >= SHARE_FLOOR, (d, bug, shares[bug])
            assert not np.array_equal(bad_rs[long], rs[long]), (d, bug)
        print("d %d: shares of differing long-row elements %r" % (d, {k: round(v, 3) for k, v in shares.items()}))
        bad, bad_rs = R.split_gather_ref(*args, bug="ge")
        hit = lens == 16
        assert (bad[hit] != out[hit]).any(1).all() and np.array_equal(bad[~hit], out[~hit])
        bad, bad_rs = R.split_gather_ref(*args, bug="drop_tail")
        hit = long & (lens % 8 != 0)
        assert hit.sum() == 10 and (bad[hit] != out[hit]).any(1).all() and (bad_rs[hit] != rs[hit]).all() and np.array_equal(bad[~hit], out[~hit])
        bad, bad_rs = R.split_gather_ref(*args, bug="rowsum_short_only")
        assert np.array_equal(bad, out) and (bad_rs[long] == 0).all() and (rs[long] != 0).all() and np.array_equal(bad_rs[~long], rs[~long])
        good = R.split_gather_ref(*args, own=own, base=base, base_rowsum=base_rs)
        late = R.split_gather_ref(*args, own=own, base=base, base_rowsum=base_rs, bug="own_late")
        assert np.array_equal(late[1], good[1]) and float((late[0][lens > 0] != good[0][lens > 0]).mean()) >= SHARE_FLOOR
        # accumulate: ignoring the base, or chaining a long row from it instead of adding the partials onto it, shows as well
        assert not np.array_equal(good[0], R.split_gather_ref(*args, own=own)[0])
        assert float((R.split_gather_ref(*args, base=base, bug="whole")[0][long] != R.split_gather_ref(*args, base=base)[0][long]).mean()) >= SHARE_FLOOR
    # the other thresholds of the case list tell the chunk length apart as well
    W = R.weights(R.N_COLS16, 12)
    for t in R.THRESHOLDS:
        out, _ = R.split_gather_ref(m.indptr, m.indices, m.data, W, t)
        for bug in ("whole", "chunk_t", "reverse") + (("drop_tail",) if t >> 1 > 1 else ()):          # (chunks of 1 have no partial tail)
            assert not np.array_equal(R.split_gather_ref(m.indptr, m.indices, m.data, W, t, bug=bug)[0], out), (t, bug)
        if (lens == t).any():
            assert not np.array_equal(R.split_gather_ref(m.indptr, m.indices, m.data, W, t, bug="ge")[0], out), t
    # 16 and 17 differ in the row of 17 alone
    a, b = (R.split_gather_ref(m.indptr, m.indices, m.data, W, t)[0] for t in (16, 17))
    assert np.array_equal(a[lens != 17], b[lens != 17]) and (a[lens == 17] != b[lens == 17]).any(1).all()


def test_every_seeded_spmv_defect_changes_the_result():
    m = R.lens_csr(R.LENS16, R.N_COLS16, 16)
    lens = np.diff(m.indptr)
    for beta in (R.beta_of(R.N_COLS16), None):
        out = R.split_spmv_ref(m.indptr, m.indices, m.data, 16, beta=beta)
        for bug in R.SPMV_BUGS:
            bad = R.split_spmv_ref(m.indptr, m.indices, m.data, 16, beta=beta, bug=bug)
            touched = lens == 16 if bug == "ge" else lens > 16
            assert np.array_equal(bad[~touched], out[~touched]) and not np.array_equal(bad[touched], out[touched]), (bug, beta is None)
    # the stride matrix: three chunks of 2, 2, 1 against the whole row, with and without beta
    s = R.SPMV_CASE_BY_ID["stride"].matrix()
    for with_beta in (True, False):
        beta = R.beta_of(s.shape[1]) if with_beta else None
        whole = R.split_spmv_ref(s.indptr, s.indices, s.data, R.STRIDE_T, beta=beta, bug="whole")
        assert float((whole != R.expected_spmv("stride", with_beta)).mean()) >= 0.1


def test_stride_case_tells_the_order_apart():
    case = R.CASE_BY_ID["stride-t4-d256"]
    x = R.case_inputs(case)
    out, rs = R.expected(case.id, False, False)
    whole, rs_whole = R.split_gather_ref(x.m.indptr, x.m.indices, x.m.data, x.W, case.split_t, bug="whole")
    assert float((whole != out).mean()) >= SHARE_FLOOR and float((rs_whole != rs).mean()) >= 0.1
    assert np.array_equal(whole, O.spmm_exact(x.m, x.W))


# ------------------------------------------------------------------------------------------------ the host query
def test_workspace_query_equals_the_restated_layout_and_refuses_a_threshold_below_two():
    from tensorrec_amd import _native as N
    lib = N.load()
    unset = -(2 ** 31) + 12345
    before = lib.trec_get_tuning(b"split_t", unset)
    q = lambda nnz, d: N.query("trec_csr_split_workspace_bytes", nnz, d)
    try:
        N.clear_tuning("split_t")
        for nnz, d in ((0, 1), (1, 4), (41000, 256), (1311000, 1), (2396, 1024), (20000263, 100)):
            assert q(nnz, d) == R.workspace_bytes(nnz, d, R.SPLIT_T_DEFAULT), (nnz, d)
        for t in (0, 1, -5):
            N.set_tuning("split_t", t)
            assert q(1000, 4) == -1 and q(0, 1) == -1, t
        for t in (2, 3, 4, 5, 16, 17):
            N.set_tuning("split_t", t)
            for nnz, d in ((0, 1), (2396, 1024), (41000, 256), (1311000, 1)):
                assert q(nnz, d) == R.workspace_bytes(nnz, d, t) > 0, (t, nnz, d)
        assert q(-1, 4) == -1 and q(10, 0) == -1
    finally:
        if before == unset:
            N.clear_tuning("split_t")
        else:
            N.set_tuning("split_t", before)
    assert lib.trec_get_tuning(b"split_t", R.SPLIT_T_DEFAULT) == R.SPLIT_T_DEFAULT
    assert q(1000, 4) == R.workspace_bytes(1000, 4, R.SPLIT_T_DEFAULT)
