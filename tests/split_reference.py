"""Bit-exact references, the float64 bar, the launch rule and the case list for the chunked gathers of csrc/spmm_split.hip:
split_rows_kernel / split_chunks_kernel<ITERS, PACKED, VEC> (with the val_perm fork of gather_range), split_reduce_kernel<ITERS, VEC> and the
SpMV / segment-sum kernels that share the plan.  NumPy / SciPy only: no torch, nothing of the code under test.  tests/test_split_reference_host.py
checks the references on the CPU (hand-worked cases, the C oracle on short rows, the float64 bar, coverage of every instantiation, seeded
defects); tests/test_gpu_split_gather.py holds the kernels to them with np.array_equal.

The order (the header of csrc/spmm_split.hip and include/tensorrec_hip.h), T = the tuning split_t:
* a row of n <= T non-zeros is the CSR-order fmaf chain of K1 (k1_reference.chain32), started from `out` when accumulating;
* a row of n > T non-zeros is cut into chunks of T >> 1 (the last one may be shorter); every chunk is an fmaf chain from zero, and the
  partials are added in chunk order, with float32 adds, onto `out` (accumulate) or onto zero;
* with `own` the operand of the fmaf is the float32 difference own[row] - W[col], rounded once;
* rowsum: per chunk (a short row is one chunk) the values are added in entry order from zero; the chunk sums are added in chunk order onto
  the base (accumulate) or onto zero;
* SpMV: short rows with beta are one fmaf chain in CSR order; without beta 16 strided lanes (lane l adds entries l, l + 16, ...) and the xor
  butterfly 8, 4, 2, 1; a chunk of a long row is 64 strided lanes (fmaf with beta, plain adds without) and the butterfly 32 .. 1; the chunk
  sums are added in chunk order from zero.

Bar against float64 (k1_reference's gather bar): a sum of m terms passes every term through at most m + 1 roundings -- a chunk of c entries
and then ceil(m / c) additions, c + ceil(m / c) <= m + 1 for m > 2 c -- so (m + 1) u sum |terms|, u = 2^-24, a base counting as one more term.
With `own` the terms are those of the rounded differences (the rounding of the difference is part of the stated operation).

`bug=`: seeded defects for the host test's discrimination checks alone (see BUGS)."""
import functools
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

from k1_reference import F32, U32, chain32, f64, fmaf32, packed_entries  # noqa: F401  (packed_entries: re-exported for the GPU test)

SPLIT_T_DEFAULT = 2048
BUGS = ("whole",                # no splitting: every row is one chain
        "chunk_t",              # chunks of split_t instead of split_t >> 1
        "ge",                   # rows of exactly split_t non-zeros are split as well
        "reverse",              # partials added last to first
        "drop_tail",            # the last, partial chunk of a long row is lost
        "own_late",             # rowsum * own - gather instead of per-entry differences
        "rowsum_short_only")    # the row sums of long rows are never written
SPMV_BUGS = ("whole", "chunk_t", "ge", "reverse", "drop_tail")


# ------------------------------------------------------------------------------------------------ which kernel a call takes
def accepts(d):
    """the entry point's width rule: a multiple of 4 up to 1,024 (float4 lanes), or any width up to 256 (single-column lanes)"""
    return d >= 1 and ((d % 4 == 0 and d <= 1024) or d <= 256)


def _pow2ceil_log2(x):
    l = 0
    while (1 << l) < x:
        l += 1
    return l


def lanes_of(d):
    """(lanes per row, ITERS as launched, VEC): per = d / 4 column groups of float4, or d single columns; lpr = min(64, pow2ceil(per));
    ceil(per / lpr) is mapped to 1 / 2 / 4 (3 runs as 4)"""
    assert accepts(d), d
    vec = 4 if d % 4 == 0 else 1
    per = d // 4 if vec == 4 else d
    lpr = 1 << min(_pow2ceil_log2(per), 6)
    iters = -(-per // lpr)
    assert 1 <= iters <= 4
    return lpr, (1 if iters == 1 else 2 if iters == 2 else 4), vec


def pick_split(d, packed=False, perm=False):
    """(ITERS, PACKED, VEC, PERM) of split_rows_kernel / split_chunks_kernel for this call; gather_range reads val_perm only where the
    entries are not packed.  The reduce kernel of the same call is (ITERS, VEC)."""
    _, iters, vec = lanes_of(d)
    return (iters, bool(packed), vec, bool(perm) and not packed)


SOURCES = {"plain": (False, False), "perm": (False, True), "packed": (True, False)}           # name -> (PACKED, PERM)
ALL_SPLIT_KERNELS = {(it, pk, vec, pm) for it in (1, 2, 4) for vec in (4, 1) for pk, pm in SOURCES.values()}
ALL_REDUCE_KERNELS = {(it, vec) for it in (1, 2, 4) for vec in (4, 1)}


def plan_bounds(nnz, split_t):
    """(max_long, max_chunks) of plan_layout: what the workspace is sized for and the grids are derived from"""
    assert split_t >= 2
    return nnz // split_t + 1, 3 * nnz // split_t + 2


def workspace_bytes(nnz, d, split_t):
    """plan_layout restated: header, three lists per long row, three per chunk and the partials, each rounded up to 16 bytes"""
    max_long, max_chunks = plan_bounds(nnz, split_t)
    up16 = lambda x: (x + 15) & ~15
    return sum(up16(b) for b in (16, 8 * max_long, 4 * max_long, 4 * max_long, 8 * max_chunks, 4 * max_chunks, 4 * max_chunks,
                                 4 * max_chunks * d))


def gather_grid(nnz, d, split_t):
    """subgroups of the fixed grids of split_chunks_kernel (at most 4,096 workgroups) and split_reduce_kernel (2,048): a chunk list / long
    row list longer than that makes the grid-stride loop take a second step"""
    max_long, max_chunks = plan_bounds(nnz, split_t)
    lpr = lanes_of(d)[0]
    chunk_blocks = min(-(-max_chunks * lpr // 256), 4096)
    reduce_blocks = min(-(-max_long * lpr // 256), 2048)
    return SimpleNamespace(chunk_subgroups=chunk_blocks * 256 // lpr, reduce_subgroups=reduce_blocks * 256 // lpr)


def spmv_grid(nnz, split_t):
    """waves of split_spmv_chunks_kernel (4,096 workgroups of four) and threads of split_spmv_reduce_kernel (1,024 workgroups of 256)"""
    max_long, max_chunks = plan_bounds(nnz, split_t)
    return SimpleNamespace(chunk_waves=min(-(-max_chunks * 64 // 256), 4096) * 4, reduce_threads=min(-(-max_long // 256), 1024) * 256)


# ------------------------------------------------------------------------------------------------ the chunk structure
def chunks_of(indptr, split_t, bug=None):
    """one entry per chunk (a short row is one chunk, an empty row an empty one), rows in order, a row's chunks in order:
    row, k, start / end in the CSR arrays, `long` per row, first chunk and chunk count per row"""
    assert split_t >= 2 and bug in (None,) + BUGS
    indptr = np.asarray(indptr, dtype=np.int64)
    n = indptr.size - 1
    lens = np.diff(indptr)
    chunk = split_t if bug == "chunk_t" else split_t >> 1
    long = lens >= split_t if bug == "ge" else lens > split_t
    if bug == "whole":
        long = np.zeros(n, bool)
    nch = np.where(long, -(-lens // chunk), 1)
    if bug == "drop_tail":
        nch = nch - (long & (lens % chunk != 0))
    first = np.concatenate([[0], np.cumsum(nch)])[:-1]
    row = np.repeat(np.arange(n), nch)
    k = np.arange(int(nch.sum())) - first[row]
    start = indptr[row] + np.where(long[row], k * chunk, 0)
    end = np.where(long[row], np.minimum(start + chunk, indptr[row + 1]), indptr[row + 1])
    return SimpleNamespace(row=row, k=k, start=start, end=end, long=long, first=first, nch=nch, lens=lens, chunk=chunk)


def _flatten(st):
    """(pointer over the chunks, CSR positions of their entries in order, chunk of every entry)"""
    clen = st.end - st.start
    cptr = np.concatenate([[0], np.cumsum(clen)]).astype(np.int64)
    sel = np.repeat(st.start - cptr[:-1], clen) + np.arange(int(cptr[-1]))
    return cptr, sel, np.repeat(np.arange(clen.size), clen)


def _sum32(cptr, v):
    """per chunk: the values added in entry order from zero, float32"""
    clen = np.diff(cptr)
    s = np.zeros(clen.size, F32)
    for k in range(int(clen.max()) if clen.size else 0):
        rows = np.nonzero(clen > k)[0]
        s[rows] = s[rows] + v[cptr[rows] + k]
    return s


def _add_in_chunk_order(acc, st, part, reverse=False):
    """acc[row] += part[first chunk of the row + k] for k = 0, 1, ... over the long rows, one float32 add each"""
    rows_long = np.nonzero(st.long)[0]
    for k in range(int(st.nch[rows_long].max()) if rows_long.size else 0):
        rows = rows_long[st.nch[rows_long] > k]
        c = st.first[rows] + (st.nch[rows] - 1 - k if reverse else k)
        acc[rows] = acc[rows] + part[c]
    return acc


# ------------------------------------------------------------------------------------------------ the gather
def split_gather_ref(indptr, indices, values, W, split_t, val_perm=None, own=None, base=None, base_rowsum=None, bug=None):
    """(out [n, d], rowsum [n]) of trec_spmm_csr_split in float32, bit for bit (module docstring).  values[val_perm] are the values in CSR
    order; base / base_rowsum: what an accumulating call finds in out / out_rowsum."""
    indptr = np.asarray(indptr, dtype=np.int64)
    n, d = indptr.size - 1, W.shape[1]
    W = np.asarray(W, dtype=F32)
    vals = np.asarray(values, dtype=F32)
    if val_perm is not None:
        vals = vals[np.asarray(val_perm, dtype=np.int64)]
    if bug == "own_late":
        assert own is not None
        g, rs = split_gather_ref(indptr, indices, vals, W, split_t)
        res = rs[:, None] * np.asarray(own, dtype=F32) - g
        _, rowsum = split_gather_ref(indptr, indices, vals, W, split_t, base_rowsum=base_rowsum)
        return (res if base is None else np.asarray(base, dtype=F32) + res), rowsum
    st = chunks_of(indptr, split_t, bug)
    cptr, sel, cof = _flatten(st)
    cols, v = np.asarray(indices)[sel].astype(np.int64), vals[sel]
    if own is None:
        operand, opidx = W, cols
    else:
        operand, opidx = np.asarray(own, dtype=F32)[st.row[cof]] - W[cols], np.arange(sel.size)       # rounded once, then fed to the fmaf
        assert operand.dtype == F32
    short = ~st.long[st.row]                                                                        # per chunk
    cbase = np.zeros((st.row.size, d), F32)
    if base is not None:
        cbase[short] = np.asarray(base, dtype=F32).reshape(n, d)[st.row[short]]
    part = chain32(cptr, opidx, v, operand, cbase)
    psum = _sum32(cptr, v)
    out = np.zeros((n, d), F32) if base is None else np.array(base, dtype=F32).reshape(n, d)
    rowsum = np.zeros(n, F32) if base_rowsum is None else np.array(base_rowsum, dtype=F32).reshape(n)
    out[st.row[short]] = part[short]
    rowsum[st.row[short]] = rowsum[st.row[short]] + psum[short]
    _add_in_chunk_order(out, st, part, reverse=bug == "reverse")
    if bug != "rowsum_short_only":
        _add_in_chunk_order(rowsum, st, psum, reverse=bug == "reverse")
    return out, rowsum


def split_gather_f64(indptr, indices, values, W, val_perm=None, own=None, base=None, base_rowsum=None):
    """the float64 result and the bar (m + 1) u sum |terms| for out and rowsum (m: the row's non-zeros, a base one more term)"""
    indptr = np.asarray(indptr, dtype=np.int64)
    n = indptr.size - 1
    vals = np.asarray(values, dtype=F32)
    if val_perm is not None:
        vals = vals[np.asarray(val_perm, dtype=np.int64)]
    row = np.repeat(np.arange(n), np.diff(indptr))
    operand = np.asarray(W, dtype=F32)[np.asarray(indices)]
    if own is not None:
        operand = np.asarray(own, dtype=F32)[row] - operand
    pick = sp.csr_matrix((f64(vals), np.arange(vals.size), indptr), shape=(n, vals.size))
    out, mag = pick @ f64(operand), abs(pick) @ np.abs(f64(operand))
    rs, rmag = np.asarray(pick.sum(1)).reshape(-1), np.asarray(abs(pick).sum(1)).reshape(-1)
    cnt = np.diff(indptr).astype(np.float64)
    co, cr = cnt.copy(), cnt.copy()
    if base is not None:
        out, mag, co = out + f64(base), mag + np.abs(f64(base)), co + 1
    if base_rowsum is not None:
        rs, rmag, cr = rs + f64(base_rowsum), rmag + np.abs(f64(base_rowsum)), cr + 1
    return SimpleNamespace(out=out, bar=(co[:, None] + 1) * U32 * mag, rowsum=rs, bar_rowsum=(cr + 1) * U32 * rmag)


# ------------------------------------------------------------------------------------------------ SpMV / segment sums
def _butterfly(lanes):
    """every lane: acc += acc of lane ^ off, off = L / 2 .. 1 (the xor shuffles of the kernels); lane 0 is what is stored"""
    L = lanes.shape[1]
    idx = np.arange(L)
    off = L >> 1
    while off:
        lanes = lanes + lanes[:, idx ^ off]
        off >>= 1
    return lanes[:, 0]


def _lane_sums(start, clen, v, b, L, block=32768):
    """per chunk: L strided lanes (lane l takes entries l, l + L, ... in order: fmaf with b, plain add without), then the butterfly"""
    out = np.zeros(clen.size, F32)
    for lo in range(0, clen.size, block):
        s, c = start[lo:lo + block], clen[lo:lo + block]
        lanes = np.zeros((c.size, L), F32)
        for k in range(int(c.max()) if c.size else 0):
            rows = np.nonzero(c > k)[0]
            j = s[rows] + k
            if b is None:
                lanes[rows, k % L] = lanes[rows, k % L] + v[j]
            else:
                lanes[rows, k % L] = fmaf32(v[j], b[j], lanes[rows, k % L])
        out[lo:lo + block] = _butterfly(lanes) if L > 1 else lanes[:, 0]
    return out


def split_spmv_ref(indptr, indices, values, split_t, val_perm=None, beta=None, bug=None):
    """out [n] of trec_spmv_csr_split in float32, bit for bit (module docstring); beta None: the segment sums of the values"""
    assert bug in (None,) + SPMV_BUGS
    indptr = np.asarray(indptr, dtype=np.int64)
    n = indptr.size - 1
    vals = np.asarray(values, dtype=F32)
    if val_perm is not None:
        vals = vals[np.asarray(val_perm, dtype=np.int64)]
    b = None if beta is None else np.asarray(beta, dtype=F32)[np.asarray(indices)]
    st = chunks_of(indptr, split_t, bug)
    clen = st.end - st.start
    short = ~st.long[st.row]
    psum = np.zeros(st.row.size, F32)
    psum[short] = _lane_sums(st.start[short], clen[short], vals, b, 1 if beta is not None else 16)
    psum[~short] = _lane_sums(st.start[~short], clen[~short], vals, b, 64)
    out = np.zeros(n, F32)
    out[st.row[short]] = psum[short]
    return _add_in_chunk_order(out, st, psum, reverse=bug == "reverse")


def spmv_f64(indptr, indices, values, val_perm=None, beta=None):
    indptr = np.asarray(indptr, dtype=np.int64)
    n = indptr.size - 1
    vals = f64(values if val_perm is None else np.asarray(values)[np.asarray(val_perm, dtype=np.int64)])
    terms = vals if beta is None else vals * f64(beta)[np.asarray(indices)]
    row = np.repeat(np.arange(n), np.diff(indptr))
    s = np.bincount(row, weights=terms, minlength=n)
    a = np.bincount(row, weights=np.abs(terms), minlength=n)
    return s, (np.diff(indptr) + 1.0) * U32 * a


# ------------------------------------------------------------------------------------------------ inputs
def _signed(rng, shape, lo):
    """standard normal pushed away from 0: magnitudes in [lo, lo + ~6]"""
    x = rng.standard_normal(shape)
    return (np.sign(x) * (lo + np.abs(x))).astype(F32)


@functools.lru_cache(maxsize=None)
def lens_csr(lens, n_cols, seed):
    """CSR with exactly these row lengths, sorted distinct columns"""
    rng = np.random.default_rng(seed)
    lens = np.array(lens, dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    indices = np.concatenate([np.sort(rng.choice(n_cols, size=c, replace=False)) for c in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    m = sp.csr_matrix((_signed(rng, indptr[-1], 0.05), indices, indptr), shape=(lens.size, n_cols))
    assert m.has_sorted_indices and m.nnz == indptr[-1]
    return m


@functools.lru_cache(maxsize=None)
def uniform_csr(n_rows, per, n_cols, seed):
    """every row holds `per` non-zeros: columns start, start + step, ... with a random start and step"""
    rng = np.random.default_rng(seed)
    step = rng.integers(1, (n_cols - 1) // (per - 1) + 1, n_rows)
    start = rng.integers(0, n_cols - (per - 1) * step)
    indices = (start[:, None] + step[:, None] * np.arange(per)[None, :]).reshape(-1).astype(np.int32)
    assert indices.min() >= 0 and indices.max() < n_cols
    return sp.csr_matrix((_signed(rng, n_rows * per, 0.05), indices, np.arange(0, (n_rows + 1) * per, per, dtype=np.int64)),
                         shape=(n_rows, n_cols))


@functools.lru_cache(maxsize=None)
def weights(n_cols, d, seed=0):
    w = _signed(np.random.default_rng(15485863 * seed + 1000 * n_cols + d), (n_cols, d), 0.01)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def rows_f32(n, d, seed):
    """[n, d] dense rows: `own` (seed 3), the base of an accumulating call (seed 7)"""
    x = _signed(np.random.default_rng(282917 * seed + 17 * n + d), (n, d), 0.01)
    x.setflags(write=False)
    return x


def base_rowsum(n):
    return np.ascontiguousarray(rows_f32(n, 1, 9)[:, 0])


def beta_of(n_cols):
    return np.ascontiguousarray(rows_f32(n_cols, 1, 11)[:, 0])


@functools.lru_cache(maxsize=None)
def _perm_values(nnz, seed):
    rng = np.random.default_rng(seed)
    return _signed(rng, nnz + 13, 0.05), rng.permutation(nnz + 13)[:nnz].astype(np.int32)


def perm_values(m):
    """(store, val_perm) with store[val_perm] == m.data: a separate, larger value array read through the permutation, so that the plain,
    permuted and packed sources carry the same values in CSR order"""
    store, perm = _perm_values(m.nnz, m.nnz + m.shape[0])
    store = store.copy()
    store[perm] = m.data
    return store, perm


# ------------------------------------------------------------------------------------------------ the cases
VEC4_WIDTHS = (4, 12, 256, 260, 512, 516, 768, 772, 1024)      # ITERS 1 1 1 | 2 2 | 3->4 3->4 | 4 4
VEC1_WIDTHS = (1, 5, 63, 65, 126, 129, 190, 193, 255)          # ITERS 1 1 1 | 2 2 | 3->4 3->4 | 4 4
# split_t = 16 (chunks of 8): every tail 1 .. 8 (17 .. 24 non-zeros; 25, 100, 1000: 1, 4, 8), the threshold itself (16) and one below,
# a long row first, a long row last, an empty row right after a long one (rows 1, 14, 17)
LENS16 = (1000, 0, 1, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 0, 16, 100, 0, 3, 16, 15, 1, 12, 0, 17)
N_COLS16 = 1500
THRESHOLDS = (2, 3, 5, 16, 17)
LENS_DEFAULT = (2049, 0, 2048, 7, 5000)                         # split_t = 2,048: 2,048 is short (the whole chain), 2,049 and 5,000 are cut
N_COLS_DEFAULT = 5200
STRIDE_ROWS, STRIDE_T, STRIDE_COLS, STRIDE_D = 8200, 4, 512, 256  # rows of split_t + 1 = 5: three chunks per five non-zeros, the densest
SPMV_STRIDE_ROWS = 262200

# (name, own, accumulate, rowsum): every pair of options meets in all four combinations
OPTIONS = (("rowsum", False, False, True), ("own", True, False, False), ("accumulate+rowsum", False, True, True),
           ("own+accumulate+rowsum", True, True, True), ("accumulate", False, True, False))
PRODUCTION = ("perm+own",                     # the Euclidean item-side pair gradient
              "perm+accumulate+rowsum",       # the item-side gradient and bias gradient of the fused steps
              "packed+accumulate+rowsum")     # the sampled pairs grouped by item on the device


def _launches(sources, options):
    return [SimpleNamespace(name="%s+%s" % (s, o[0]), source=s, own=o[1], accumulate=o[2], rowsum=o[3]) for s in sources for o in OPTIONS
            if o[0] in options]


def _case(group, name, matrix, d, split_t, launches):
    return SimpleNamespace(group=group, id="%s-%s-d%d" % (group, name, d), matrix=matrix, d=d, split_t=split_t, launches=launches)


def _build_cases():
    cases = []
    m16 = functools.partial(lens_csr, LENS16, N_COLS16, 16)
    every = tuple(o[0] for o in OPTIONS)
    for d in VEC4_WIDTHS + VEC1_WIDTHS:
        cases.append(_case("widths", "t16", m16, d, 16, _launches(SOURCES, every)))
    for t in THRESHOLDS:
        for d in (12, 65):
            cases.append(_case("thresholds", "t%d" % t, m16, d, t, _launches(SOURCES, ("rowsum", "own+accumulate+rowsum"))))
    for d in (12, 65):
        cases.append(_case("default", "t2048", functools.partial(lens_csr, LENS_DEFAULT, N_COLS_DEFAULT, 2048), d, SPLIT_T_DEFAULT,
                           _launches(SOURCES, ("rowsum", "own+accumulate+rowsum"))))
    cases.append(_case("stride", "t4", functools.partial(uniform_csr, STRIDE_ROWS, STRIDE_T + 1, STRIDE_COLS, 4), STRIDE_D, STRIDE_T,
                       _launches(("plain",), ("rowsum",)) + _launches(("perm",), ("own+accumulate+rowsum",)) +
                       _launches(("packed",), ("accumulate+rowsum",))))
    return cases


CASES = _build_cases()
CASE_BY_ID = {c.id: c for c in CASES}

SPMV_CASES = [SimpleNamespace(id="t%d" % t, matrix=functools.partial(lens_csr, LENS16, N_COLS16, 16), split_t=t) for t in THRESHOLDS] + [
    SimpleNamespace(id="default", matrix=functools.partial(lens_csr, LENS_DEFAULT, N_COLS_DEFAULT, 2048), split_t=SPLIT_T_DEFAULT),
    SimpleNamespace(id="stride", matrix=functools.partial(uniform_csr, STRIDE_ROWS, STRIDE_T + 1, STRIDE_COLS, 4), split_t=STRIDE_T),
    SimpleNamespace(id="stride-reduce", matrix=functools.partial(uniform_csr, SPMV_STRIDE_ROWS, STRIDE_T + 1, STRIDE_COLS, 5), split_t=STRIDE_T)]
SPMV_CASE_BY_ID = {c.id: c for c in SPMV_CASES}


def case_inputs(case):
    """the host arrays of a gather case: matrix, weights, own rows, base and base of the row sums (shared by all of its launches)"""
    m = case.matrix()
    n = m.shape[0]
    return SimpleNamespace(m=m, W=weights(m.shape[1], case.d), own=rows_f32(n, case.d, 3), base=rows_f32(n, case.d, 7), base_rowsum=base_rowsum(n))


@functools.lru_cache(maxsize=None)
def expected(case_id, own, accumulate):
    """(out, rowsum) of a launch of the case with these options, computed once; the source does not enter: all three carry the same values
    in CSR order"""
    case = CASE_BY_ID[case_id]
    x = case_inputs(case)
    out, rs = split_gather_ref(x.m.indptr, x.m.indices, x.m.data, x.W, case.split_t, own=x.own if own else None,
                               base=x.base if accumulate else None, base_rowsum=x.base_rowsum if accumulate else None)
    out.setflags(write=False)
    rs.setflags(write=False)
    return out, rs


@functools.lru_cache(maxsize=None)
def expected_spmv(case_id, with_beta):
    case = SPMV_CASE_BY_ID[case_id]
    m = case.matrix()
    out = split_spmv_ref(m.indptr, m.indices, m.data, case.split_t, beta=beta_of(m.shape[1]) if with_beta else None)
    out.setflags(write=False)
    return out
