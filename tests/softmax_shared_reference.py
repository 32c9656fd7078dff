"""Float64 reference, error bars, inputs, a float32 restatement and the coverage mirror for the sampled-softmax step with SHARED
negatives (csrc/softmax_shared.hip, ops.softmax_shared_step).  NumPy / SciPy only, nothing of the code under test.
tests/test_softmax_shared_reference_host.py holds the reference to central differences and the bars to the restatement on the CPU
(and shows that seeded defects fall outside); tests/test_gpu_softmax_shared.py holds the kernels to the reference.

The step.  By definition the step of softmax_step_reference.ref_step on a case whose [n_users, S] sample table repeats ONE row of S
ids: the values below ARE that function's (imported, not edited).  Hits are kept; the variants are plain / logq / logq-uniform.

The kernels' form.  t = float32(1 / temperature), c_s = -(log S + log q(item_s)) or 0,
    w_us = ((u . v_s + b_u) + b_s) t + c_s,  M = max_s w,  Z = sum_s exp(w - M)  (online: a running (m, z) per half-wave over tiles of
    32 samples, rescaled by exp(m_old - m_new) when the maximum moves, the two halves combined at the end),
    w_p = y_p t,  m = max(M, w_p),  a = exp(w_p - m),  b = exp(M - m),  D = a + b Z,  loss_p = (m - w_p) + log D,
    d y_p = -t b Z / D,  K = sum_p b_p / D_p,  P_us = (t K) exp(w_us - M),  d b_u = sum_p d y_p + (t K) Z.

Bars.  The derivation of sampled_loss_reference / sampled_adjust_reference (u = 2^-24, counts in units of u, LIB = 4 per library
function, DIV = 2, TINY absolute per exponential), with these changes; nothing is tuned.
    w_s     formed WITHOUT a shift by the row maximum: t is rounded and the product is rounded (2 |y_s| t), the addition of c rounds
            (|w_s|; the kernel fuses the two, the count takes them apart), c itself carries (LIB + 1) |c_s| as in the adjusted
            loss                                                                                              -> absolute dw_s
    E_s     in P: exp(w_s - M) with the final M: dw_s + |w_s - M| + LIB                                       =: e_rel_s (relative)
    Z       online.  With span = M - min_s w and T = ceil(S / 32) tiles, an element enters as exp(w_s - m_tile) (argument rounded:
            at most span; LIB) and is then multiplied by at most T factors exp(m_old - m_new) (the rescales of its half-wave and
            the final combination), each an exponential of a rounded difference and a rounded product; the differences telescope
            to at most span:  dw_s + 2 span + LIB + T (LIB + 1)                                                =: e_on_s
            the sum in any order, the two halves, the rescaled partial: S + 2.   rz = (sum E e_on + (S + 2) Z) / Z, + S TINY
    w_p     2 |y_p| t absolute =: dp;  a, b: dp + |w_p - m| + LIB resp. dp + |M - m| + LIB.  As in the adjusted loss, every output
            (loss, b Z / D, E b / D, t K Z) is invariant under the shift M, so the float32 M the kernel finds is taken as the
            reference's shift and adds nothing.
    D, loss, d y_p, K, P: as there.  (m - w_p): |m - w_p| + dp.
    scores  the loss phase is handed float32 scores off by at most delta (pair_reference.score_bar: the MFMA chain and K3's chain
            are both d fused multiply-adds): softmax_step_reference's argument -- loss_p moves by 2 t delta_u, every gradient
            coefficient by a relative expm1(2 t delta_u).
    dU, dV, d b_u, d b_i   pair_reference.grad_bars on the pair list of the repeated table (a term passes through at most as many
            additions as the entry has terms, whatever the tiles, slices and the duplicate fold do), plus the coefficients' bars
            carried through.  d b_u's analytic t K Z is the sum of the user's P: its error -- rz on Z, dK on K, two products -- is
            below what the carried bars of the S coefficients plus grad_bars' S + n roundings give.
The dyadic family (tables and biases multiples of 1/8, scores_exact) has delta = 0: pred_serial is held bit for bit and the loss
phase stands alone.  Entries whose terms are all 0 have a bar of 0."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

import softmax_step_reference as SR
from pair_reference import MODE_DOT, f64, grad_bars, ref_pair_grads
from sampled_loss_reference import U32, TINY, LIB, DIV, _users
from softmax_step_reference import scores_exact, ratios, OUTPUTS, OP_RESULTS  # noqa: F401  (re-exported)

F = np.float32
VARIANTS = ("plain", "logq", "logq-uniform")
TEMPERATURES = [1.0, 0.25]
FAR = 100.0
SPAN = 30.0
MAX_D = 128


def supported(n_sampled, d):
    """mirror of trec_softmax_shared_supported / ops.softmax_shared_supported (tuning aside)"""
    return bool(1 <= n_sampled < 2 ** 31 and d % 4 == 0 and 4 <= d <= MAX_D)


def slices(n_users, n_sampled, d, forced=0):
    """mirror of trec_softmax_shared_slices: how many user slices the dV role runs"""
    tiles = -(-n_users // 32)
    n = forced if forced >= 1 else -(-1024 // -(-n_sampled // 128))
    n = max(1, min(n, (256 << 20) // (n_sampled * (d + 1) * 4), tiles))
    return -(-n_users // (-(-tiles // n) * 32))


# ------------------------------------------------------------------------------------------------ inputs
# (users, S, d, kind): every user count (wave and workgroup edges), every S (tile edges, many tiles) and every d at least once; kinds: "" nothing special,
# "alleq" all samples the same item, "span" samples on reserved items with zero rows and biases spanning +-SPAN
GPU_CASES = [(1, 1, 4, ""), (31, 31, 36, ""), (32, 32, 64, ""), (33, 33, 128, ""), (127, 64, 36, ""), (128, 65, 64, ""),
             (129, 257, 128, ""), (300, 1000, 36, ""), (300, 65, 128, ""), (33, 1000, 4, ""), (129, 1, 128, ""), (1, 257, 36, ""),
             (129, 65, 36, ""), (129, 65, 36, "alleq"), (129, 65, 36, "span"), (33, 31, 64, "span")]
CORE = (129, 65, 36, "")               # every option crossed on this one; the model-level shape
SLICED = (300, 65, 128, "")            # forced slice counts 1, 2, 3
UNCOVERED = [(65, 132), (65, 256), (65, 6), (65, 2), (0, 64)]
U_NONE, U_NONPOS, U_ABOVE, U_BELOW, U_SHARED_POS = 1, 2, 3, 4, 5      # planted users (cases with >= 8 users)


def shared_case(n_users, S, d, kind="", exact=False, seed=0):
    """A softmax_step_reference-shaped case whose sample table repeats one row.  Planted (>= 8 users): user 1 has no interaction,
    user 2 interactions of value <= 0 beside a positive (pos_slot < 0), user 3 a positive FAR above and user 4 one FAR below every
    sample (through item biases: what they mean in the runs WITH biases), user 5 a positive on an item that is ALSO sampled (it stays
    a negative).  S >= 2: slot 1 repeats the id of slot 0.  With one user: three interactions, one of value 0."""
    rng = np.random.default_rng(9001 * n_users + 101 * S + 13 * d + (5 if exact else 0) + 3 * len(kind) + seed)
    n_reg = 200
    span0 = n_reg
    n_span = S if kind == "span" else 0
    far_above, far_below = n_reg + n_span, n_reg + n_span + 1
    n_items = n_reg + n_span + 2
    if exact:
        U = (rng.integers(-8, 9, size=(n_users, d)) / 8.0 * (rng.random((n_users, d)) < min(1.0, 16.0 / d))).astype(F)
        V = (rng.integers(-8, 9, size=(n_items, d)) / 8.0 * (rng.random((n_items, d)) < min(1.0, 16.0 / d))).astype(F)
        ub = (rng.integers(-8, 9, n_users) / 8.0).astype(F)
        ib = (rng.integers(-8, 9, n_items) / 8.0).astype(F)
    else:
        U = (rng.standard_normal((n_users, d)) / np.sqrt(d)).astype(F)
        V = (2.0 * rng.standard_normal((n_items, d))).astype(F)
        ub = (0.5 * rng.standard_normal(n_users)).astype(F)
        ib = (0.5 * rng.standard_normal(n_items)).astype(F)
    row = rng.integers(0, n_reg, size=S).astype(np.int32)
    if kind == "alleq":
        row[:] = row[0]
    elif kind == "span":
        row = (span0 + rng.permutation(S)).astype(np.int32)
        V[span0:span0 + S] = 0.0
        span = np.linspace(-SPAN, SPAN, S) if S > 1 else np.array([SPAN])
        ib[span0:span0 + S] = (np.round(span * 8.0) / 8.0).astype(F)
    if S >= 2:
        row[1] = row[0]
    planted = n_users >= 8
    lens = rng.integers(1, 6, size=n_users)
    if planted:
        lens[U_NONE], lens[U_NONPOS] = 0, 4
    else:
        lens[0] = 3
    r_idx, c_idx, vals = [], [], []
    for u in range(n_users):
        n = int(lens[u])
        cols = np.sort(rng.choice(n_reg, size=n, replace=False))
        v = rng.integers(1, 13, size=n) / 4.0
        if planted and u == U_NONPOS:
            v[:] = [1.0, -1.0, 0.0, 2.0]
        if planted and u == U_SHARED_POS and kind != "span":
            cols[0] = row[-1]
            cols = np.unique(cols)
            v = v[:cols.size]
            v[:] = 1.0
        if not planted and u == 0:
            v[1] = 0.0
        r_idx += [u] * cols.size
        c_idx += list(cols)
        vals += list(v)
    m = sp.csr_matrix((np.array(vals, F), (np.array(r_idx, np.int64), np.array(c_idx, np.int64))), shape=(n_users, n_items))
    assert m.nnz == len(vals) and m.has_sorted_indices
    indptr, x_item, values = m.indptr.astype(np.int64), m.indices.astype(np.int32).copy(), m.data.astype(F)
    above = below = -1
    if planted:
        # the LAST interaction of the user is moved onto a reserved item beyond every other column: the row stays sorted
        for u, item, up in ((U_ABOVE, far_above, True), (U_BELOW, far_below, False)):
            q = int(indptr[u + 1] - 1)
            x_item[q], values[q] = item, 1.0
            V[item] = 0.0
            s = f64(V)[row] @ f64(U)[u] + float(ub[u]) + f64(ib)[row]
            target = (s.max() + FAR if up else s.min() - FAR) - float(ub[u])
            ib[item] = F(np.ceil(target * 8.0) / 8.0 if up else np.floor(target * 8.0) / 8.0)
        above, below = int(indptr[U_ABOVE + 1] - 1), int(indptr[U_BELOW + 1] - 1)
    log_q = rng.permutation(np.linspace(-2.0, -14.0, n_items)).astype(F)
    m = sp.csr_matrix((values, x_item, indptr), shape=(n_users, n_items))
    assert m.has_sorted_indices
    samples = np.ascontiguousarray(np.broadcast_to(row, (n_users, S)))
    return SimpleNamespace(U=U, V=V, ub=ub, ib=ib, matrix=m, indptr=indptr, x_item=x_item, cols=x_item, values=values, samples=samples,
                           items=samples, row=row, log_q=log_q, S=S, d=d, n_users=n_users, n_items=n_items, kind=kind,
                           max_pos=int(np.diff(indptr).max()), exact=exact, planted=planted, above=above, below=below)


def case_properties(case):
    """what the cases are meant to hold (scores with biases), as a dict the host test asserts"""
    xu, xi = SR.pair_lists(case)
    sc = SR.ref_pair_scores(case.U, case.V, xu, xi, MODE_DOT, case.ub, case.ib).scores
    nnz = case.x_item.size
    yp, ys = sc[:nnz], sc[nnz:].reshape(case.n_users, case.S)
    lens = np.diff(case.indptr)
    out = dict(repeated=bool((case.samples == case.row[None, :]).all()), duplicate=bool(case.S < 2 or case.row[0] == case.row[1]),
               all_equal=bool((case.row == case.row[0]).all()), span=float(ys[0].max() - ys[0].min()))
    if case.planted:
        r = lambda u: slice(case.indptr[u], case.indptr[u + 1])
        out.update(no_interaction=bool(lens[U_NONE] == 0), nonpositive=bool((case.values[r(U_NONPOS)] <= 0).any()
                                                                            and (case.values[r(U_NONPOS)] > 0).any()),
                   far_above=float(yp[case.above] - ys[U_ABOVE].max()), far_below=float(ys[U_BELOW].min() - yp[case.below]),
                   sampled_positive=bool(np.isin(case.x_item[r(U_SHARED_POS)][case.values[r(U_SHARED_POS)] > 0], case.row).any()))
    return out


# ------------------------------------------------------------------------------------------------ reference
def corrections(case, variant):
    """c [S] float64"""
    if variant == "plain":
        return np.zeros(case.S)
    lq = f64(case.log_q)[case.row] if variant == "logq" else np.full(case.S, -np.log(float(case.n_items)))
    return -(np.log(float(case.S)) + lq)


def loss_bars(case, yp, ys, cs, temperature):
    """(bar_loss [P+], bar_d_pred [P], bar_d_samp [U, S]) of the kernels' form, per the module docstring"""
    t = 1.0 / float(temperature)
    S, T = case.S, math.ceil(case.S / 32.0)
    bar_loss = np.zeros(int((case.values > 0).sum()))
    bar_d_pred, bar_d_samp = np.zeros(yp.size), np.zeros(ys.shape)
    for u, idx, n, slot, pos in _users(case.indptr, case.values):
        if not idx.size:
            continue
        y = ys[u]
        w = y * t + cs
        dw = U32 * (2.0 * np.abs(y) * t + np.abs(w) + (LIB + 1.0) * np.abs(cs))
        M = w.max()
        span = M - w.min()
        E = np.exp(w - M)
        Z = E.sum()
        e_rel = dw + (np.abs(w - M) + LIB) * U32
        e_on = dw + (2.0 * span + LIB + T * (LIB + 1.0)) * U32
        rz = ((E * e_on).sum() + (S + 2.0) * U32 * Z + S * TINY) / Z
        wp = yp[idx] * t
        dp = 2.0 * U32 * np.abs(yp[idx]) * t
        m = np.maximum(M, wp)
        a, b = np.exp(wp - m), np.exp(M - m)
        ea, eb = dp + (np.abs(wp - m) + LIB) * U32, dp + (np.abs(M - m) + LIB) * U32
        bz = b * Z
        D = a + bz
        rD = (a * ea + bz * (eb + rz + U32) + (1.0 + Z) * TINY) / D + U32
        logD = np.where(wp >= M, np.log1p(bz), np.log(D))
        lo = (m - wp) + logD
        bar_loss[slot[idx]] = rD + LIB * U32 * logD + U32 * (m - wp) + dp + U32 * lo
        r = bz / D
        rr = eb + rz + U32 + rD + DIV * U32
        bar_d_pred[idx] = t * r * (rr + 3.0 * U32) + t * (Z + 2.0) * TINY + TINY
        term = b / D
        rt = eb + U32 + rD + DIV * U32
        aK = term.sum()
        dK = (term * rt).sum() + n * U32 * aK + n * 2.0 * TINY
        bar_d_samp[u] = t * E * (aK * (e_rel + 3.0 * U32) + dK) + (t * aK + 1.0) * TINY
    return bar_loss, bar_d_pred, bar_d_samp


def ref_step(case, biased, temperature, variant="plain"):
    """the float64 step (softmax_step_reference.ref_step on the repeated table) with the bars of the shared-negatives kernels"""
    assert variant in VARIANTS
    r = SR.ref_step(case, biased, temperature, variant)
    assert not r.hits.any()
    d, nu, S, nnz = case.d, case.n_users, case.S, case.x_item.size
    t = 1.0 / float(temperature)
    xu, xi = SR.pair_lists(case)
    yp, ys = r.scores.scores[:nnz], r.scores.scores[nnz:].reshape(nu, S)
    bl, bp, bs = loss_bars(case, yp, ys, corrections(case, variant), temperature)
    du = np.zeros(nu)
    np.maximum.at(du, xu, r.delta)
    f = np.expm1(2.0 * t * du)
    pos = case.values > 0
    r.b_pred_serial = r.delta[:nnz]
    r.b_loss = bl + 2.0 * t * du[xu[:nnz]][pos]
    r.b_g = np.concatenate([bp, bs.reshape(-1)]) + np.abs(r.g) * f[xu]
    inh = ref_pair_grads(np.abs(f64(case.U)), np.abs(f64(case.V)), xu, xi, r.b_g, MODE_DOT)
    bU, bV, bub, bib = grad_bars(r.pg, d)
    r.b_dU, r.b_dV, r.b_d_ub, r.b_d_ib = bU + inh.dU, bV + inh.dV, bub + inh.dub, bib + inh.dib
    return r


@functools.lru_cache(maxsize=None)
def cached_case(spec, exact):
    return shared_case(*spec, exact=exact)


@functools.lru_cache(maxsize=None)
def cached_ref(spec, exact, biased, temperature, variant):
    """computed once and shared by the host and the GPU tests; nobody writes into it"""
    return ref_step(cached_case(spec, exact), biased, temperature, variant)


def options_of(i):
    """(biased, temperature, variant) of GPU case number i: the options cycle over the cases, CORE crosses them all"""
    return (i % 2 == 0, TEMPERATURES[(i // 2) % 2], VARIANTS[i % 3])


ALL_OPTIONS = [(b, t, v) for b in (True, False) for t in TEMPERATURES for v in VARIANTS]


def loss_sum(case, biased, temperature, variant, U=None, V=None, ub=None, ib=None):
    """sum of the reference loss at perturbed tables (central differences)"""
    return SR.loss_sum(case, biased, temperature, variant, U=U, V=V, ub=ub, ib=ib)


# ------------------------------------------------------------------------------------------------ float32 restatement
DEFECTS = ("ragged_zero", "k_without_b", "p_without_t", "duplicates_once", "positive_corrected", "dub_without_z")


def _cd_row(r, half):
    return (r & 3) + 8 * (r >> 2) + 4 * half


def _tile_order(n):
    """the streamed rows of n in the order the chained MFMA adds them: tile by tile, k-step r pairs the half-waves' r-th columns"""
    out = []
    for t0 in range(0, n, 32):
        for r in range(16):
            for half in (0, 1):
                s = t0 + _cd_row(r, half)
                if s < n:
                    out.append(s)
    return np.array(out, np.int64)


def _fma(a, b, c):
    return (f64(a) * f64(b) + f64(c)).astype(F)            # (one rounding; the double product of two floats is exact)


def restate_f32(case, biased, temperature, variant, order="natural", defect=None, n_slices=1):
    """the kernels' arithmetic in float32 NumPy.  order: 'natural' (row maximum first, every sum in index order) or 'paired' (the online
    (m, z) per half-wave and the half-wave-paired k-steps of the chained MFMA, the users of dV in n_slices slices).  `defect`: one of
    DEFECTS seeded into it.  Returns a namespace with the six outputs."""
    t = F(1.0 / temperature)
    S, nu, d, ni = case.S, case.n_users, case.d, case.n_items
    U, V, row = case.U.astype(F), case.V.astype(F), case.row.astype(np.int64)
    Vs = V[row]
    cs = np.zeros(S, F)
    if variant == "logq":
        cs = (-(case.log_q[row] + F(np.log(float(S))))).astype(F)
    elif variant == "logq-uniform":
        cs = np.full(S, -F(F(np.log(float(S))) + F(-np.log(float(ni)))), F)
    # ---- scores: the k-ordered chain of fused multiply-adds, then (dot + b_u) + b_s, then one fma with t and c
    dot = np.zeros((nu, S), F)
    for k in range(d):
        dot = _fma(U[:, k][:, None], Vs[:, k][None, :], dot)
    y = dot
    if biased:
        y = ((dot + case.ub[:, None]).astype(F) + case.ib[row][None, :]).astype(F)
    w = _fma(y, t, cs[None, :])
    # ---- row statistics
    if order == "natural":
        M = w.max(1)
        Z = np.zeros(nu, F)
        for s in range(S):
            Z = (Z + np.exp((w[:, s] - M).astype(F)).astype(F)).astype(F)
    else:
        Sp = -(-S // 32) * 32
        wp_ = np.full((nu, Sp), F(0.0) if defect == "ragged_zero" else F(-np.inf), F)
        wp_[:, :S] = w
        hm, hz = [], []
        with np.errstate(invalid="ignore", over="ignore"):
            for half in (0, 1):
                rm, rz = np.full(nu, -np.inf, F), np.zeros(nu, F)
                for t0 in range(0, Sp, 32):
                    cols = [t0 + _cd_row(r, half) for r in range(16)]
                    tm = wp_[:, cols].max(1)
                    live = tm > -np.inf
                    up = live & (tm > rm)
                    sc = np.where(up, np.exp((rm - tm).astype(F)).astype(F), F(1.0)).astype(F)
                    rz = np.where(up, (rz * sc).astype(F), rz)
                    rm = np.where(up, tm, rm)
                    for c in cols:
                        e = np.exp((wp_[:, c] - rm).astype(F)).astype(F)
                        rz = np.where(live, (rz + e).astype(F), rz)
                hm.append(rm)
                hz.append(rz)
            M = np.maximum(hm[0], hm[1])
            parts = [np.where(hm[h] > -np.inf, (hz[h] * np.exp((hm[h] - M).astype(F)).astype(F)).astype(F), F(0.0)) for h in (0, 1)]
        Z = (parts[0] + parts[1]).astype(F)
    # ---- positives
    pos = case.values > 0
    slot = np.cumsum(pos) - 1
    nnz = case.x_item.size
    xu = np.repeat(np.arange(nu), np.diff(case.indptr))
    xi = case.x_item.astype(np.int64)
    pdot = np.zeros(nnz, F)
    for k in range(d):
        pdot = _fma(U[xu, k], V[xi, k], pdot)
    pred = pdot
    if biased:
        pred = ((pdot + case.ub[xu]).astype(F) + case.ib[xi]).astype(F)
    loss = np.zeros(int(pos.sum()), F)
    d_pred = np.zeros(nnz, F)
    tK, d_ub = np.zeros(nu, F), np.zeros(nu, F)
    for u in range(nu):
        K, sdy = F(0.0), F(0.0)
        for q in range(case.indptr[u], case.indptr[u + 1]):
            if not pos[q]:
                continue
            wq = F(pred[q] * t)
            if defect == "positive_corrected" and variant != "plain":
                cq = -(F(np.log(float(S))) + (case.log_q[xi[q]] if variant == "logq" else F(-np.log(float(ni)))))
                wq = F(wq + F(cq))
            m = max(M[u], wq)
            a, b = np.exp(F(wq - m)).astype(F), np.exp(F(M[u] - m)).astype(F)
            bz = F(b * Z[u])
            D = F(a + bz)
            loss[slot[q]] = F(F(m - wq) + np.log(D).astype(F))
            dy = F(-t * F(bz / D))
            d_pred[q] = dy
            sdy = F(sdy + dy)
            K = F(K + (F(F(1.0) / D) if defect == "k_without_b" else F(b / D)))
        tK[u] = K if defect == "p_without_t" else F(t * K)
        d_ub[u] = F(sdy + (tK[u] if defect == "dub_without_z" else F(tK[u] * Z[u])))
    # ---- the samples' gradients
    P = (tK[:, None] * np.exp((w - M[:, None]).astype(F)).astype(F)).astype(F)
    dU, dV = np.zeros((nu, d), F), np.zeros((ni, d), F)
    d_ib = np.zeros(ni, F)
    for q in range(nnz):                                            # the positives' parts, in interaction order
        dU[xu[q]] = _fma(d_pred[q], V[xi[q]], dU[xu[q]])
    for i in np.unique(xi):
        for q in np.flatnonzero(xi == i):
            dV[i] = _fma(d_pred[q], U[xu[q]], dV[i])
            d_ib[i] = F(d_ib[i] + d_pred[q])
    s_order = np.arange(S) if order == "natural" else _tile_order(S)
    acc = np.zeros((nu, d), F)
    for s in s_order:
        acc = _fma(P[:, s][:, None], Vs[s][None, :], acc)
    dU = (dU + acc).astype(F)
    dVs, dbs = np.zeros((S, d), F), np.zeros(S, F)
    if order == "natural":
        bounds = [(0, nu)]
    else:
        ln = -(-(-(-nu // 32)) // n_slices) * 32
        bounds = [(a0, min(a0 + ln, nu)) for a0 in range(0, nu, ln)]
    for a0, a1 in bounds:
        part, psum = np.zeros((S, d), F), [np.zeros(S, F), np.zeros(S, F)]
        users = np.arange(a0, a1) if order == "natural" else a0 + _tile_order(a1 - a0)
        for u in users:
            part = _fma(P[u][:, None], U[u][None, :], part)
            h = 0 if order == "natural" else (((u - a0) % 32) >> 2) & 1
            psum[h] = (psum[h] + P[u]).astype(F)
        dVs = (dVs + part).astype(F)
        dbs = (dbs + (psum[0] + psum[1]).astype(F)).astype(F)
    for i in np.unique(row):                                        # duplicates: added in slot order, then onto the positives' part
        slots = np.flatnonzero(row == i)
        if defect == "duplicates_once":
            slots = slots[:1]
        a_v, a_b = np.zeros(d, F), F(0.0)
        for s in slots:
            a_v = (a_v + dVs[s]).astype(F)
            a_b = F(a_b + dbs[s])
        dV[i] = (dV[i] + a_v).astype(F)
        d_ib[i] = F(d_ib[i] + a_b)
    return SimpleNamespace(loss=loss, pred_serial=pred, dU=dU, dV=dV, d_ub=d_ub, d_ib=d_ib, M=M, Z=Z, tK=tK)
