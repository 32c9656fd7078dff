"""Float64 references, error bars, inputs and the kernel-selection rule for K1 (csrc/spmm.hip): the CSR gather spmm_csr_vec4_kernel<ITERS, R,
EPI, NT, NTL, PACKED>, its scalar fallback, spmm_one_per_row_kernel<ITERS> and the tower kernels (row normalise forward / backward, bias +
ReLU, ReLU backward, column sums, segment sums, CSR -> dense).  NumPy / SciPy only: no torch, nothing of the code under test.
tests/test_k1_reference_host.py holds the references and the bars to float32 restatements on the CPU and shows that the case list reaches
every instantiation; tests/test_gpu_k1.py holds the kernels to the references.

The gather itself is exact: one fmaf per element in CSR order, which oracle.spmm_exact (C) computes independently; chain32 below restates
it in NumPy (fmaf32 is a correctly rounded fmaf, not an approximation of one) for the calls that start from a base (accumulate).

Bars.  u = 2^-24 is the unit roundoff of float32.

* normalise               y = r / sqrt(max(S, 1e-12)), S = sum r^2, taken on the float32 chain result r.  The float32 S passes a term through at
  (epilogue 1,            most d + 6 roundings (a lane's chain, six butterfly levels) plus the square's own: (d + 8) u relative on S, half of that
  row_l2norm_fwd)         on the root; two ulps cover sqrtf, two the division, one the product: ((d + 8) / 2 + 4) u |y|, and the same, relative,
                          on inv = 1 / sqrt(max(S, 1e-12)).  A row with S = 0 is exact zeros with inv == 1 / sqrtf(1e-12f) (bar 0).
* row_l2norm_bwd          dx_c = (dy_c - y_c t) inv, t = sum y dy; the kernel is fed the float32 roundings of the float64 y and inv.
                          t: d + 6 roundings and the rounding of every y, (d + 9) u A with A = sum |y dy|; the product y_c t carries its own
                          rounding and that of y_c, 2 u |y_c t| (|t| <= A); the difference one rounding of at most |dy_c| + |y_c t|; the product
                          with inv its own rounding and that of inv, 2 u |dx_c|:
                          u inv (|y_c| ((d + 9) A + 3 |t|) + |dy_c|) + 2 u |dx_c|.
                          A clamped row (inv >= 1 / sqrtf(1e-12f), fed as that float32 constant) is dy_c inv, one rounding: u |dx_c|.
* row sums, column sums   m terms in any order (a chain, 16 lanes and a butterfly, slices and a finish pass): m u sum |terms|; a base that is
                          accumulated into counts as one more term.
* filter operand          (epilogue 4) the fp32 row is the exact chain, the bf16 image its round-to-nearest-even bit for bit, the error terms
                          row - bf16(row) exact float32 differences.  The two norms are d fmaf terms, a butterfly (or the DPP reduction) and
                          sqrtf: (d + 8) u relative on the sum, half of it on the root, two ulps for sqrtf less the two spare units:
                          ((d + 8) / 2 + 2) u relative.  gstats[0..1] are the maxima of the stats the kernel wrote, bit for bit.
* gather against float64  a sum of m fmaf terms: (m + 1) u sum |terms| (pair_reference.py's gradient-entry bar with k = 1).
* towers                  first-order propagation of the bars above through the closed forms.
                          E_r = m_i u sum_j |x_ij w_jc|                                                     (the forward gather, m_i non-zeros)
                          E_y,c = inv (E_r,c + |y_c| sum_k |y_k| E_r,k) + ((d + 8) / 2 + 4) u |y_c|          (d y = (dr - y (y . dr)) / |r|)
                          E_inv / inv = inv sum_k |y_k| E_r,k + ((d + 8) / 2 + 4) u
                          E_dx,c = inv (E_y,c |t| + |y_c| sum_k |g_k| E_y,k) + |dx_c| E_inv / inv + bar of row_l2norm_bwd
                          E_dW = |X|^T E_dx + (m_f + 1) u |X|^T |dx|                                         (m_f non-zeros of the feature)
                          ReLU tower: out = max(r + b, 0) is the chain, one rounding of the sum and a maximum: E_r + u |r + b|.  The mask
                          out > 0 agrees with float64 because no pre-activation lies within 8 u of 0 relative to its sum of absolute terms
                          (asserted on the inputs; the planted exact zero is 0 on both sides), so d pre = g * mask is exact and
                          E_dW = (m_f + 1) u |X|^T |d pre|, E_db = n u sum_i |d pre_ic|.

Which kernel.  pick_kernel restates launch_vec4 and the five entry points; ALL_KERNELS is every instantiation they can launch:
* trec_spmm_csr, epilogues 0..3: the non-temporal forms <1, 4, E, NT, NTL> (NTL 0 / 1) and the plain forms <ITERS, R, E> for ITERS 1 / 2 / 4
  and R 1 / 4.  accumulate never meets epilogue 1 / 2 (rejected by the entry point), and with epilogues 0 / 3 it only moves <1, 4> from the
  non-temporal to the plain form, so it adds nothing.
* trec_spmm_csr_filter (epilogue 4): d <= 256, so ITERS is always 1: <1, 4, 4, NT, NTL>, <1, 4, 4> and <1, 1, 4>.
* trec_spmm_csr_packed: <ITERS, 1, E, PACKED> for E 0 / 3: always one row per subgroup, never non-temporal.
* the scalar fallback (d % 4 != 0 or d > 1024) with the pass that follows it under each epilogue, and spmm_one_per_row_kernel<1 / 2 / 4>.
The kernels without template parameters (row normalise, ReLU backward, column sums, segment sums, CSR -> dense) are not listed: a call
either runs them or does not."""
import functools
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

U32 = 2.0 ** -24
F32 = np.float32
EPS32 = np.float32(1e-12)                                   # L2NORM_EPS
INV_EPS32 = np.float32(1.0) / np.sqrt(EPS32)                # 1 / sqrtf(1e-12f): inv of a clamped row
NORM_CLAMPED, NORM_SMALL = 5e-7, 2e-6                       # planted row norms: squared 2.5e-13 (clamped) and 4e-12 (not)
N_SPECIAL = 4                                               # features F-1 .. F-4 belong to the planted rows
ROW_ZERO_W, ROW_CLAMPED, ROW_SMALL, ROW_RELU0 = 5, 6, 7, 8  # planted rows (matrices of 16 rows and more); rows 1 and n - 1 are empty


def f64(a):
    return np.asarray(a, dtype=np.float64)


# ------------------------------------------------------------------------------------------------ the exact chain
def fmaf32(a, b, c):
    """fmaf, correctly rounded: the product of two float32 is exact in float64; the float64 sum is rounded to odd (TwoSum gives the error
    of the addition), after which the rounding to float32 is that of the exact value"""
    p = np.atleast_1d(f64(a) * f64(b))
    c = np.atleast_1d(f64(c))
    p, c = np.broadcast_arrays(p, c)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    fix = (e != 0) & ((s.view(np.int64) & 1) == 0)
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def chain32(indptr, indices, values, W, base=None):
    """out[r] = base[r] (or 0), then fmaf(values[j], W[indices[j]], out[r]) for j in CSR order: what every K1 kernel computes"""
    indptr = np.asarray(indptr, dtype=np.int64)
    n, d = indptr.size - 1, W.shape[1]
    out = np.zeros((n, d), F32) if base is None else np.array(base, dtype=F32).reshape(n, d)
    lens = np.diff(indptr)
    for k in range(int(lens.max()) if n else 0):
        rows = np.nonzero(lens > k)[0]
        j = indptr[rows] + k
        out[rows] = fmaf32(values[j][:, None], W[indices[j]], out[rows])
    return out


def bf16_bits(x):
    """round-to-nearest-even bf16 image of finite float32 values, as uint16"""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_back(bits):
    return (bits.astype(np.uint32) << 16).view(F32)


# ------------------------------------------------------------------------------------------------ references and bars
def gather_ref(m, W, base=None):
    """float64 X . W (+ base) and its bar (m_i + 1) u sum |terms|"""
    ax = abs(m).astype(np.float64)
    ref, mag = m.astype(np.float64) @ f64(W), ax @ np.abs(f64(W))
    cnt = np.diff(m.indptr).astype(np.float64)
    if base is not None:
        ref, mag, cnt = ref + f64(base), mag + np.abs(f64(base)), cnt + 1
    return ref, (cnt[:, None] + 1) * U32 * mag


def normalize_ref(r):
    """y, inv of the float64 row normalise of r and their bars; rows with S = 0 carry inv = 1 / sqrtf(1e-12f) exactly (bar 0)"""
    r = f64(r)
    d = r.shape[1]
    ss = (r * r).sum(1)
    inv = 1.0 / np.sqrt(np.maximum(ss, float(EPS32)))
    inv[ss == 0] = float(INV_EPS32)
    y = r * inv[:, None]
    k = ((d + 8) / 2.0 + 4.0) * U32
    bar_inv = np.where(ss == 0, 0.0, k * inv)
    return SimpleNamespace(y=y, inv=inv, ss=ss, bar_y=k * np.abs(y), bar_inv=bar_inv, clamped=ss < float(EPS32))


def l2norm_bwd_inputs(nr):
    """the float32 y and inv the backward kernel is fed: roundings of the float64 ones; a clamped row carries the kernel's own constant"""
    inv32 = nr.inv.astype(F32)
    inv32[nr.clamped] = INV_EPS32
    return nr.y.astype(F32), inv32


def l2norm_bwd_ref(nr, dy):
    """dx and its bar for dy through the normalise whose forward reference is nr (normalize_ref)"""
    y, dy = nr.y, f64(dy)
    d = y.shape[1]
    inv = np.where(nr.clamped, float(INV_EPS32), nr.inv)[:, None]
    t = (y * dy).sum(1)[:, None]
    A = np.abs(y * dy).sum(1)[:, None]
    dx = np.where(nr.clamped[:, None], dy * inv, (dy - y * t) * inv)
    bar = U32 * inv * (np.abs(y) * ((d + 9) * A + 3 * np.abs(t)) + np.abs(dy)) + 2 * U32 * np.abs(dx)
    return dx, np.where(nr.clamped[:, None], U32 * np.abs(dx), bar)


def segsum_ref(indptr, values, base=None):
    """row sums of the values and the bar m u sum |terms| (a base counts as a term)"""
    indptr = np.asarray(indptr, dtype=np.int64)
    row = np.repeat(np.arange(indptr.size - 1), np.diff(indptr))
    n = indptr.size - 1
    s = np.bincount(row, weights=f64(values), minlength=n)
    a = np.bincount(row, weights=np.abs(f64(values)), minlength=n)
    m = np.diff(indptr).astype(np.float64)
    if base is not None:
        s, a, m = s + f64(base), a + np.abs(f64(base)), m + 1
    return s, m * U32 * a


def colsum_ref(x):
    x = f64(x)
    return x.sum(0), x.shape[0] * U32 * np.abs(x).sum(0)


def filter_ref(chain):
    """bf16 bits, {|row|, |row - bf16(row)|} in float64 and the relative bar of the two norms, from the float32 chain result"""
    bits = bf16_bits(chain)
    err = chain - bf16_back(bits)                                       # exact in float32: the discarded low bits
    assert np.array_equal(f64(err), f64(chain) - f64(bf16_back(bits)))
    d = chain.shape[1]
    stats = np.stack([np.sqrt((f64(chain) ** 2).sum(1)), np.sqrt((f64(err) ** 2).sum(1))], 1)
    return SimpleNamespace(bits=bits, err=err, stats=stats, bar=((d + 8) / 2.0 + 2.0) * U32 * stats)


def norm_tower_ref(m, W, g):
    """y = normalise(X W), dW of sum g * y, and their bars (module docstring)"""
    X, ax = m.astype(np.float64), abs(m).astype(np.float64)
    W, g = f64(W), f64(g)
    d = W.shape[1]
    r = X @ W
    cnt_r = np.diff(m.indptr).astype(np.float64)[:, None]
    cnt_f = np.bincount(m.indices, minlength=m.shape[1]).astype(np.float64)[:, None]
    nr = normalize_ref(r)
    E_r = cnt_r * U32 * (ax @ np.abs(W))
    k = ((d + 8) / 2.0 + 4.0) * U32
    inv = nr.inv[:, None]
    yE = (np.abs(nr.y) * E_r).sum(1)[:, None]
    E_y = inv * (E_r + np.abs(nr.y) * yE) + k * np.abs(nr.y)
    E_y = np.where(nr.clamped[:, None], inv * E_r + 2 * U32 * np.abs(nr.y), E_y)      # a clamped row is r * constant
    E_inv_rel = np.where(nr.clamped[:, None], 0.0, inv * yE + k)
    dx, bar_bwd = l2norm_bwd_ref(nr, g)
    t = (nr.y * g).sum(1)[:, None]
    E_dx = inv * (E_y * np.abs(t) + np.abs(nr.y) * (np.abs(g) * E_y).sum(1)[:, None]) + np.abs(dx) * E_inv_rel + bar_bwd
    E_dx = np.where(nr.clamped[:, None], bar_bwd, E_dx)                                # dy * constant: y does not enter
    dW = X.T @ dx
    E_dW = ax.T @ E_dx + (cnt_f + 1) * U32 * (ax.T @ np.abs(dx))
    return SimpleNamespace(y=nr.y, bar_y=E_y, dW=dW, bar_dW=E_dW, nr=nr, r=r, dx=dx, bar_dx=E_dx)


def relu_tower_ref(m, W, b, g):
    """out = relu(X W + b), dW and db of sum g * out, their bars, and margin = |pre| / (u sum |terms|) (inf where pre is an exact planted 0)"""
    X, ax = m.astype(np.float64), abs(m).astype(np.float64)
    W, b, g = f64(W), f64(b), f64(g)
    pre = X @ W + b
    mag = ax @ np.abs(W) + np.abs(b)
    cnt_r = np.diff(m.indptr).astype(np.float64)[:, None]
    cnt_f = np.bincount(m.indices, minlength=m.shape[1]).astype(np.float64)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        margin = np.where(pre == 0, np.inf, np.abs(pre) / (U32 * mag))
    out = np.maximum(pre, 0.0)
    dpre = np.where(pre > 0, g, 0.0)
    return SimpleNamespace(out=out, bar_out=cnt_r * U32 * (ax @ np.abs(W)) + U32 * np.abs(pre), pre=pre, margin=margin, dpre=dpre,
                           dW=X.T @ dpre, bar_dW=(cnt_f + 1) * U32 * (ax.T @ np.abs(dpre)),
                           db=dpre.sum(0), bar_db=m.shape[0] * U32 * np.abs(dpre).sum(0))


# ------------------------------------------------------------------------------------------------ which kernel a call takes
def _vec4_shape(d):
    n4 = d // 4
    lpr_log2 = 0
    while (1 << lpr_log2) < n4:
        lpr_log2 += 1
    lpr = 1 << min(lpr_log2, 6)
    iters = (n4 + lpr - 1) // lpr
    return lpr, (1 if iters == 1 else 2 if iters == 2 else 4)


def vec4_lanes(d):
    """(lanes per row, ITERS) of the float4 kernels at this width"""
    return _vec4_shape(d)


def pick_kernel(n_rows, nnz, d, epilogue, accumulate=0, tuning=None, entry="csr"):
    """the instantiation a call launches.  entry: csr (trec_spmm_csr; epilogue 4: trec_spmm_csr_filter), packed (trec_spmm_csr_packed) or
    one_per_row (trec_spmm_one_per_row); tuning: {"spmm_nt": 0 / 1, "spmm_ntload": -1 / 0 / 1}, defaults 1 and -1 (the data decides).
    ("vec4", ITERS, R, EPI, NT, NTL, PACKED) | ("scalar", EPI) | ("one_per_row", ITERS)"""
    tuning = tuning or {}
    if entry == "one_per_row":
        assert d % 4 == 0 and 4 <= d <= 1024 and epilogue == 0 and not accumulate
        return ("one_per_row", _vec4_shape(d)[1])
    if entry == "packed":
        assert d % 4 == 0 and 4 <= d <= 1024 and epilogue in (0, 3)
        return ("vec4", _vec4_shape(d)[1], 1, epilogue, False, False, True)
    assert entry == "csr"
    if epilogue == 4:
        assert d in (32, 64, 128, 256) and not accumulate
    else:
        assert epilogue in (0, 1, 2, 3) and not (accumulate and epilogue in (1, 2))
        if d % 4 != 0 or d > 1024:
            return ("scalar", epilogue)
    _, iters = _vec4_shape(d)
    R = 4 if (0 <= nnz <= 4 * n_rows and n_rows >= 4096) else 1
    ntl = tuning.get("spmm_ntload", -1)
    if ntl < 0:
        ntl = 1 if (nnz >= 0 and 4 * nnz <= 5 * n_rows) else 0
    nt = tuning.get("spmm_nt", 1)
    if R == 4 and iters == 1 and nt and not accumulate:
        return ("vec4", 1, 4, epilogue, True, bool(ntl), False)
    return ("vec4", iters, R, epilogue, False, False, False)


ALL_KERNELS = (
    {("vec4", 1, 4, e, True, ntl, False) for e in (0, 1, 2, 3, 4) for ntl in (False, True)}
    | {("vec4", it, r, e, False, False, False) for it in (1, 2, 4) for r in (1, 4) for e in (0, 1, 2, 3)}
    | {("vec4", 1, r, 4, False, False, False) for r in (1, 4)}
    | {("vec4", it, 1, e, False, False, True) for it in (1, 2, 4) for e in (0, 3)}
    | {("scalar", e) for e in (0, 1, 2, 3)}
    | {("one_per_row", it) for it in (1, 2, 4)})


# ------------------------------------------------------------------------------------------------ inputs
def _signed(rng, shape, lo):
    """standard normal pushed away from 0: magnitudes in [lo, lo + ~6]"""
    x = rng.standard_normal(shape)
    return (np.sign(x) * (lo + np.abs(x))).astype(F32)


def _from_counts(n, F, counts, rng):
    """CSR with the given row lengths, sorted distinct columns below F - N_SPECIAL, rows 1 and n - 1 empty and the planted rows (one entry
    each, value 1, in a feature of their own; value 1.5 for the all-zero weight row)"""
    counts = np.array(counts, dtype=np.int64)
    planted = n >= 16
    if n > 3:
        counts[[1, n - 1]] = 0
    if planted:
        counts[ROW_ZERO_W:ROW_RELU0 + 1] = 1
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    indices = np.empty(indptr[-1], np.int32)
    for r in np.nonzero(counts)[0]:
        indices[indptr[r]:indptr[r + 1]] = np.sort(rng.choice(F - N_SPECIAL, size=counts[r], replace=False))
    values = _signed(rng, indptr[-1], 0.05)
    if planted:
        for row, feat, v in ((ROW_ZERO_W, F - 1, 1.5), (ROW_CLAMPED, F - 2, 1.0), (ROW_SMALL, F - 3, 1.0), (ROW_RELU0, F - 4, 1.0)):
            indices[indptr[row]], values[indptr[row]] = feat, v
    m = sp.csr_matrix((values, indices, indptr), shape=(n, F))
    assert m.has_sorted_indices and m.nnz == indptr[-1]
    return m


@functools.lru_cache(maxsize=None)
def short_csr(n, F, seed, mean):
    """0..4 non-zeros per row: uniformly 0..4 (mean 2) or mostly one (mean 1: about one non-zero per row, the embedding shape)"""
    rng = np.random.default_rng(1000003 * seed + 10 * n + mean)
    p = {2: [0.2] * 5, 1: [0.15, 0.75, 0.06, 0.03, 0.01]}[mean]
    return _from_counts(n, F, rng.choice(5, size=n, p=p), rng)


@functools.lru_cache(maxsize=None)
def dense_csr(n, F, density, seed):
    """every cell of the ordinary features kept with probability `density`"""
    rng = np.random.default_rng(7919 * seed + n)
    return _from_counts(n, F, rng.binomial(F - N_SPECIAL, density, size=n), rng)


def prefix_csr(m, n):
    """the first n rows of m, entry for entry"""
    return sp.csr_matrix((m.data[:m.indptr[n]], m.indices[:m.indptr[n]], m.indptr[:n + 1]), shape=(n, m.shape[1]))


@functools.lru_cache(maxsize=None)
def one_per_row_csr(n, F, seed):
    rng = np.random.default_rng(31 * seed + n)
    return sp.csr_matrix((_signed(rng, n, 0.05), rng.integers(0, F, n).astype(np.int32), np.arange(n + 1, dtype=np.int64)), shape=(n, F))


@functools.lru_cache(maxsize=None)
def long_rows_csr():
    """5 x 300 with rows of 0, 1, 64, 65 and 200 entries: rows longer than a wave (CSR -> dense) and than 16 lanes (segment sums)"""
    rng = np.random.default_rng(5300)
    counts = [0, 1, 64, 65, 200]
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    indices = np.concatenate([np.sort(rng.choice(300, size=c, replace=False)) for c in counts]).astype(np.int32)
    return sp.csr_matrix((_signed(rng, indptr[-1], 0.05), indices, indptr), shape=(5, 300))


@functools.lru_cache(maxsize=None)
def bias(d, seed=0):
    return _signed(np.random.default_rng(104729 * seed + d), d, 0.01)


@functools.lru_cache(maxsize=None)
def weights(F, d, seed=0):
    """[F, d] weights of magnitude 0.01 .. ~6; the last four rows serve the planted rows: all zero, norm 5e-7, norm 2e-6, -bias(d)"""
    rng = np.random.default_rng(15485863 * seed + 1000 * F + d)
    W = _signed(rng, (F, d), 0.01)
    W[F - 1] = 0
    for row, norm in ((F - 2, NORM_CLAMPED), (F - 3, NORM_SMALL)):
        t = f64(W[row])
        W[row] = (t * (norm / np.sqrt((t * t).sum()))).astype(F32)
    W[F - 4] = -bias(d, seed)
    W.setflags(write=False)
    return W


def dense_rows(n, d, seed):
    """[n, d] input of the row normalise: ordinary rows of magnitude 0.01 .. ~6 and (16 rows and more) the planted ones: rows 1 and n - 1
    zero, row 6 of norm 5e-7, row 7 of norm 2e-6"""
    rng = np.random.default_rng(611953 * seed + 1031 * n + d)
    x = _signed(rng, (n, d), 0.01)
    if n >= 16:
        x[[1, n - 1]] = 0
        for row, norm in ((ROW_CLAMPED, NORM_CLAMPED), (ROW_SMALL, NORM_SMALL)):
            t = f64(x[row])
            x[row] = (t * (norm / np.sqrt((t * t).sum()))).astype(F32)
    return x


def gradient(n, d, seed):
    return _signed(np.random.default_rng(282917 * seed + 17 * n + d), (n, d), 0.01)


def packed_entries(m):
    """int2 {column, value bits} per non-zero, as an [nnz, 2] int32 array"""
    return np.ascontiguousarray(np.stack([m.indices.astype(np.int32), m.data.astype(F32).view(np.int32)], 1))


def input_conditions(m, W, b=None):
    """what the bars presuppose, as a dict the host test asserts: magnitudes, nothing but the planted rows near the clamp, no ReLU
    pre-activation near 0 but the planted exact zeros"""
    planted = m.shape[0] >= 16
    ordinary_w = np.abs(W[:W.shape[0] - N_SPECIAL]) if planted else np.abs(W)
    r = m.astype(np.float64) @ f64(W)
    ss = (r * r).sum(1)
    special = np.zeros(m.shape[0], bool)
    lens = np.diff(m.indptr)
    special[lens == 0] = True
    if planted:
        special[ROW_ZERO_W:ROW_RELU0] = True                                    # zero weights, clamped, small; not the ReLU row
    out = dict(values_in_range=bool(m.nnz == 0 or (np.abs(m.data).min() >= 1e-3 and np.abs(m.data).max() <= 1e3)),
               weights_in_range=bool(ordinary_w.min() >= 1e-3 and ordinary_w.max() <= 1e3),
               clamp_band_clear=bool(((ss[~special] < 0.25e-12) | (ss[~special] > 4e-12)).all()),
               empty_rows=int((lens == 0).sum()))
    if planted:
        out.update(zero_row=bool(ss[ROW_ZERO_W] == 0 and lens[ROW_ZERO_W] == 1), clamped_row=bool(0 < ss[ROW_CLAMPED] < 0.5e-12),
                   small_row=bool(2e-12 < ss[ROW_SMALL] < 8e-12))
    if b is not None:
        t = relu_tower_ref(m, W, b, np.zeros(r.shape))
        zero = t.pre == 0
        out.update(relu_margin=float(t.margin[~zero].min()), relu_zero_rows=sorted(set(np.nonzero(zero.all(1))[0].tolist())),
                   relu_zero_elsewhere=int(zero[~zero.all(1)].sum()))
    return out


# ------------------------------------------------------------------------------------------------ the GPU cases
F_BIG, F_SMALL = 977, 57
SEED = 1
TOWER_SEED = 5                   # weights / bias of the towers: a seed under which every ReLU pre-activation keeps its margin (asserted)


def _launch(epi, expect, accumulate=0, tuning=None, entry="csr"):
    return SimpleNamespace(epi=epi, expect=expect, accumulate=accumulate, tuning=tuning or {}, entry=entry)


def _case(group, name, matrix, d, launches, **kw):
    return SimpleNamespace(group=group, id="%s-%s-d%d" % (group, name, d), matrix=matrix, d=d, launches=launches, **kw)


def _plain(it, R, e):
    return ("vec4", it, R, e, False, False, False)


def _iters(d):
    return {4: 1, 12: 1, 32: 1, 64: 1, 100: 1, 128: 1, 256: 1, 260: 2, 512: 2, 768: 4, 1024: 4}[d]


def _build_cases():
    cases = []
    short = lambda n, mean: functools.partial(short_csr, n, F_BIG, SEED, mean)
    small = functools.partial(dense_csr, 203, F_SMALL, 0.15, SEED)
    r1big = lambda: prefix_csr(short_csr(4099, F_BIG, SEED, 2), 4095)
    # 4 rows per subgroup, every epilogue: the non-temporal forms; mean 1 also loads the weights non-temporally
    for n in (4096, 4097, 4099):
        for mean in (2, 1):
            for d in (4, 12, 64, 100, 128, 256):
                cases.append(_case("r4", "n%d-mean%d" % (n, mean), short(n, mean), d,
                                   [_launch(e, ("vec4", 1, 4, e, True, mean == 1, False)) for e in (0, 1, 2, 3)]))
    # 4 rows, two and four float4 per lane (768: a dead fourth iteration)
    for mean in (2, 1):
        for d in (260, 512, 768, 1024):
            cases.append(_case("r4wide", "mean%d" % mean, short(4099, mean), d, [_launch(e, _plain(_iters(d), 4, e)) for e in (0, 1, 2, 3)]))
    # 4 rows without the non-temporal stores: accumulate, spmm_nt = 0; spmm_ntload forced against the data
    for d in (64, 128):
        cases.append(_case("r4plain", "accumulate", short(4099, 2), d, [_launch(e, _plain(1, 4, e), accumulate=1) for e in (0, 3)]))
        cases.append(_case("r4plain", "nt0", short(4099, 2), d, [_launch(e, _plain(1, 4, e), tuning={"spmm_nt": 0}) for e in (0, 1, 2, 3)]))
        cases.append(_case("r4plain", "ntload0", short(4099, 1), d,
                           [_launch(e, ("vec4", 1, 4, e, True, False, False), tuning={"spmm_ntload": 0}) for e in (0, 1, 2, 3)]))
        cases.append(_case("r4plain", "ntload1", short(4099, 2), d,
                           [_launch(e, ("vec4", 1, 4, e, True, True, False), tuning={"spmm_ntload": 1}) for e in (0, 1, 2, 3)]))
    # 4 rows, values through val_perm
    for d, mean in ((128, 2), (128, 1), (512, 2), (512, 1)):
        exp = (lambda e: ("vec4", 1, 4, e, True, mean == 1, False)) if d == 128 else (lambda e: _plain(2, 4, e))
        cases.append(_case("r4perm", "mean%d" % mean, short(4099, mean), d, [_launch(e, exp(e)) for e in (0, 3)], perm=True))
    # one row per subgroup; the 4,095 rows are the first 4,095 of the 4,099-row matrix: R = 1 against R = 4, bit for bit
    for d in (4, 12, 100, 260, 768, 1024):
        cases.append(_case("r1", "203x57", small, d, [_launch(e, _plain(_iters(d), 1, e)) for e in (0, 1, 2, 3)]))
        cases.append(_case("r1", "4095", r1big, d, [_launch(e, _plain(_iters(d), 1, e)) for e in (0, 1, 2, 3)], same_as_r4=True))
    # scalar fallback
    for d in (1, 6, 1028):
        for name, mk in (("203x57", small), ("4099", short(4099, 2))):
            cases.append(_case("scalar", name, mk, d, [_launch(e, ("scalar", e)) for e in (0, 1, 2, 3)] +
                               [_launch(e, ("scalar", e), accumulate=1) for e in (0, 3)]))
    # filter operand
    for d in (32, 64, 128, 256):
        for n in (4096, 4099):
            for mean in (2, 1):
                cases.append(_case("filter", "n%d-mean%d" % (n, mean), short(n, mean), d, [_launch(4, ("vec4", 1, 4, 4, True, mean == 1, False))]))
        cases.append(_case("filter", "203x57", small, d, [_launch(4, _plain(1, 1, 4))]))
    cases.append(_case("filter", "nt0", short(4099, 2), 128, [_launch(4, _plain(1, 4, 4), tuning={"spmm_nt": 0})]))
    # packed entries
    for d in (4, 128, 260, 1024):
        cases.append(_case("packed", "300x90", functools.partial(dense_csr, 300, 90, 0.2, SEED), d,
                           [_launch(e, ("vec4", _iters(d), 1, e, False, False, True), accumulate=a, entry="packed") for e in (0, 3) for a in (0, 1)]))
    # one non-zero per row (128: <1>, which the other widths leave out)
    for n in (7, 4099):
        for d in (128, 260, 512, 768):
            cases.append(_case("one_per_row", "n%d" % n, functools.partial(one_per_row_csr, n, F_BIG, SEED), d,
                               [_launch(0, ("one_per_row", _iters(d)), entry="one_per_row")]))
    return cases


CASES = _build_cases()
ROWNORM_CASES = [(n, d) for n in (1, 77, 4099) for d in (1, 63, 64, 65, 100, 1024)]
TOWER_CASES = [(name, d) for name in ("4099x977", "150x40") for d in (12, 128, 260)]


def tower_matrix(name):
    return short_csr(4099, F_BIG, SEED, 2) if name == "4099x977" else dense_csr(150, 40, 0.2, SEED)


def case_values(case):
    """(values array handed to the kernel, val_perm or None, the CSR-order values the chain sees)"""
    m = case.matrix()
    if not getattr(case, "perm", False):
        return m.data, None, m.data
    rng = np.random.default_rng(m.nnz + case.d)
    store = _signed(rng, m.nnz + 13, 0.05)                              # a separate, larger value array
    perm = rng.permutation(m.nnz + 13)[:m.nnz].astype(np.int32)
    return store, perm, store[perm]


def accumulate_base(n, d):
    """the random base an accumulating call starts from, and the base of its row sums"""
    return gradient(n, d, 7), np.ascontiguousarray(gradient(n, 1, 9)[:, 0])
