"""Float64 references, error bars and inputs for the sampled softmax and BPR kernels (csrc/loss_sampled.hip).  NumPy only: no torch,
nothing of the code under test.  tests/test_sampled_loss_reference_host.py holds the references to central differences and the bars to
float32 restatements on the CPU; tests/test_gpu_sampled_losses.py holds the kernels to the references.

Notation.  t = 1 / temperature; y_p a positive's prediction, y_s a sample's prediction of the same user, go_p the upstream gradient.
    sampled softmax   loss_p = log(1 + sum_s exp((y_s - y_p) t));  with M = max_s y_s, E_s = exp((y_s - M) t), Z = sum_s E_s,
                      m = max(M, y_p), a = exp((y_p - m) t), b = exp((M - m) t), D = a + b Z:   loss_p = (m - y_p) t + log D,
                      d y_p = -go_p t b Z / D,   d y_us = t E_s K_u,   K_u = sum_p go_p b_p / D_p
    BPR               loss_p = (1/S) sum_s softplus(x_ps), x_ps = y_s - y_p, softplus(x) = max(x, 0) + log1p(e), e = exp(-|x|),
                      sigma(x) = (x >= 0 ? 1 : e) / (1 + e),   d y_p = -(go_p / S) sum_s sigma(x_ps),   d y_us = sum_p (go_p / S) sigma(x_ps)

Bars.  u = 2^-24 is the unit roundoff of float32, every count below is in units of u and relative unless it says otherwise.  The inputs
(predictions, samples, go) are float32 numbers and exact.  Building blocks:

* library functions    expf, logf, log1pf within two ulps, LIB = 4 (an ulp of x is at most 2 u |x|): the figure pair_reference.py already
                       takes for logf; the ROCm installation ships no document that gives another.
* a division           DIV = 2, as in pair_reference.py (within an ulp).
* an exponential       exp((x - y) t): the difference is rounded (u |x - y| absolute), t = float32(1 / temperature) is rounded, the product
                       is rounded: the argument is off by 3 u |x - y| t, which is a RELATIVE 3 |x - y| t on the exponential; with the
                       function itself (3 |x - y| t + LIB).  BPR has no t and no product: (|x| + LIB).  A result below 2^-126 may be
                       flushed or lose bits: TINY = 2^-126 absolute on every exponential, carried through as an absolute part.
* a sum of n terms     every sum in these formulas has terms of one sign (go may be signed: then the bar takes sum |terms|); in any order a
                       term passes through at most n - 1 additions: n relative on the sum of the absolute terms, no condition number.
                       Adding the exact 0 of a padded lane, of a non-positive interaction or of an idle thread rounds nothing.
* a fused multiply-add rounds once where the separate operations round twice: the counts below take the separate operations.

Sampled softmax.
    Z       sum_s E_s (3 |y_s - M| t + LIB) + S Z, + S TINY absolute                                    -> relative rz, Z >= 1
    D       a (3 |y_p - m| t + LIB) + b Z (3 |M - m| t + LIB + rz + 1) + 1 D (the sum), + (1 + Z) TINY    -> relative rD, D >= 1
    loss    (m - y_p) t: difference, t, product = 3 (m - y_p) t;  log D: rD absolute (d log D = dD / D) + LIB log D;  the last sum
            1 loss.  rD >= u, so the bar has an absolute part: a loss that underflows to 0 against a reference of 1e-40 passes.
    d y_p   b Z / D: (3 |M - m| t + LIB + rz + 1) + rD + DIV =: rr;  -(go t) (.): t, two products = 3:  (rr + 3) |d y_p|,
            + |go| t (Z + 2) TINY + TINY absolute
    K       term_p = (go_p b_p) / D_p: (3 |M - m| t + LIB) + 1 + rD + DIV =: rt_p;  K: sum_p |term_p| rt_p + n sum |term_p|,
            + n (max |go| + 1) TINY absolute, n the number of the user's interactions                     -> absolute dK
    d y_us  (t E_s) K: (3 |y_s - M| t + LIB) + t, two products = 3:  t E_s (sum |term_p| (3 |y_s - M| t + LIB + 3) + dK),
            + (t sum |term_p| + 1) TINY absolute
BPR.
    softplus   x = y_s - y_p rounded: 1 max(x, 0);  e: (|x| + LIB) e, through log1p (slope 1 / (1 + e)): e (|x| + LIB) / (1 + e);
               log1pf: LIB log1p(e);  the sum of the two parts: 1 softplus;  + TINY absolute                -> absolute dsp
    loss       sum_s dsp / S + (S + 2) loss (the sum; 1 / S rounded; the product), + TINY absolute
    sigma      numerator (x < 0 only): (|x| + LIB);  1 + e: e (|x| + LIB) / (1 + e) + 1;  DIV                -> relative rs, + 2 TINY
    d y_p      c = go / S: 2;  c sum_s sigma: sum_s sigma rs |c| + (S + 3) |d y_p|, + |c| 2 S TINY + TINY absolute
    d y_us     sum_p c_p sigma_ps: sum_p |c_p| sigma_ps (rs + 3) + n sum_p |c_p| sigma_ps, + (2 sum |c_p| + n) TINY absolute

Entries that must be exactly 0 (d pred of a non-positive interaction, the d samp row of a user without positives) have a bar of 0.
"""
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

U32 = 2.0 ** -24
TINY = 2.0 ** -126
LIB = 4.0
DIV = 2.0


def f64(a):
    return np.asarray(a, dtype=np.float64)


def _users(indptr, values):
    pos = np.asarray(values) > 0.0
    slot = np.cumsum(pos) - 1
    for u in range(len(indptr) - 1):
        idx = np.arange(indptr[u], indptr[u + 1])
        yield u, idx[pos[idx]], idx.size, slot, pos


def ref_sampled_softmax(indptr, values, pred, samp, go, temperature):
    """loss [P+], d_pred [P], d_samp [U, S] of sum_p go_p loss_p, their bars (bar_loss, bar_d_pred, bar_d_samp), and M, Z per user"""
    indptr, pred, samp, go = np.asarray(indptr), f64(pred), f64(samp), f64(go)
    n_users, S = samp.shape
    t = 1.0 / float(temperature)
    n_pos = int((np.asarray(values) > 0.0).sum())
    loss, bar_loss = np.zeros(n_pos), np.zeros(n_pos)
    d_pred, bar_d_pred = np.zeros(pred.size), np.zeros(pred.size)
    d_samp, bar_d_samp = np.zeros(samp.shape), np.zeros(samp.shape)
    Ms, Zs = np.zeros(n_users), np.zeros(n_users)
    for u, idx, n, slot, pos in _users(indptr, values):
        if not idx.size:
            continue
        ys = samp[u]
        M = ys.max()
        E = np.exp((ys - M) * t)
        Z = E.sum()
        e_rel = (3.0 * np.abs(ys - M) * t + LIB) * U32
        rz = ((E * e_rel).sum() + S * U32 * Z + S * TINY) / Z
        yp, g = pred[idx], go[slot[idx]]
        m = np.maximum(M, yp)
        a, b = np.exp((yp - m) * t), np.exp((M - m) * t)
        ea, eb = (3.0 * np.abs(yp - m) * t + LIB) * U32, (3.0 * np.abs(M - m) * t + LIB) * U32
        bz = b * Z
        D = a + bz
        rD = (a * ea + bz * (eb + rz + U32) + (1.0 + Z) * TINY) / D + U32
        logD = np.where(yp >= M, np.log1p(bz), np.log(D))         # (y_p >= M: a = 1 exactly)
        lo = (m - yp) * t + logD
        loss[slot[idx]] = lo
        bar_loss[slot[idx]] = rD + LIB * U32 * logD + 3.0 * U32 * (m - yp) * t + U32 * lo
        r = bz / D
        rr = eb + rz + U32 + rD + DIV * U32
        d_pred[idx] = -g * t * r
        bar_d_pred[idx] = np.abs(g) * t * r * (rr + 3.0 * U32) + np.abs(g) * t * (Z + 2.0) * TINY + TINY
        term = g * b / D
        rt = eb + U32 + rD + DIV * U32
        K, aK = term.sum(), np.abs(term).sum()
        dK = (np.abs(term) * rt).sum() + n * U32 * aK + n * (np.abs(g).max() + 1.0) * TINY
        d_samp[u] = t * E * K
        bar_d_samp[u] = t * E * (aK * (e_rel + 3.0 * U32) + dK) + (t * aK + 1.0) * TINY
        Ms[u], Zs[u] = M, Z
    return SimpleNamespace(loss=loss, d_pred=d_pred, d_samp=d_samp, bar_loss=bar_loss, bar_d_pred=bar_d_pred, bar_d_samp=bar_d_samp,
                           M=Ms, Z=Zs)


def ref_bpr(indptr, values, pred, samp, go):
    """loss [P+], d_pred [P], d_samp [U, S] of sum_p go_p loss_p and their bars"""
    indptr, pred, samp, go = np.asarray(indptr), f64(pred), f64(samp), f64(go)
    n_users, S = samp.shape
    n_pos = int((np.asarray(values) > 0.0).sum())
    loss, bar_loss = np.zeros(n_pos), np.zeros(n_pos)
    d_pred, bar_d_pred = np.zeros(pred.size), np.zeros(pred.size)
    d_samp, bar_d_samp = np.zeros(samp.shape), np.zeros(samp.shape)
    for u, idx, n, slot, pos in _users(indptr, values):
        if not idx.size:
            continue
        yp, g = pred[idx], go[slot[idx]]
        X = samp[u][None, :] - yp[:, None]
        A = np.abs(X)
        e = np.exp(-A)
        l1 = np.log1p(e)
        spl = np.maximum(X, 0.0) + l1
        lo = spl.sum(1) / S
        dsp = U32 * (np.maximum(X, 0.0) + e * (A + LIB) / (1.0 + e) + LIB * l1 + spl) + TINY
        loss[slot[idx]] = lo
        bar_loss[slot[idx]] = dsp.sum(1) / S + (S + 2.0) * U32 * lo + TINY
        sig = np.where(X >= 0.0, 1.0, e) / (1.0 + e)
        rs = ((X < 0.0) * (A + LIB) + e * (A + LIB) / (1.0 + e) + 1.0 + DIV) * U32
        c = g / S
        dp = -c * sig.sum(1)
        d_pred[idx] = dp
        bar_d_pred[idx] = np.abs(c) * ((sig * rs).sum(1) + 2.0 * S * TINY) + (S + 3.0) * U32 * np.abs(dp) + TINY
        T = np.abs(c)[:, None] * sig
        d_samp[u] = (c[:, None] * sig).sum(0)
        bar_d_samp[u] = (T * (rs + 3.0 * U32)).sum(0) + n * U32 * T.sum(0) + (2.0 * np.abs(c).sum() + n) * TINY
    return SimpleNamespace(loss=loss, d_pred=d_pred, d_samp=d_samp, bar_loss=bar_loss, bar_d_pred=bar_d_pred, bar_d_samp=bar_d_samp)


def bars(ref):
    """(bar loss, bar d pred, bar d samp)"""
    return ref.bar_loss, ref.bar_d_pred, ref.bar_d_samp


# ------------------------------------------------------------------------------------------------ inputs
SAMPLE_COUNTS = [1, 63, 64, 65, 256, 257, 300]           # both forms below 257, the workgroup form above
SAMPLE_COUNTS_MANY = [40, 300]                          # the staging passes of the users above 1,024 positives
TEMPERATURES = [1.0, 0.25]
N_ITEMS = 2700
POSITIVES = [0, 0, 65, 1025, 2600, 4, 17, 1, 30, 64, 3]  # per user; user 0 has no interaction, user 1 non-positives only
U_PLANTED_M, U_EQUAL, U_SPAN, U_FAR = 2, 5, 6, 8


def loss_case(S, seed=0):
    """11 users x 2,700 items with the geometry of pair_reference.wmrb_case: users with 0 (no interaction / non-positives only), 65, 1,025
    and 2,600 positives and a few small ones, negative and explicit-zero interactions mixed in.  Real-valued float32 predictions.
    Planted: user 2 holds a positive above its samples' maximum M (M + 0.75), one equal to M bit for bit, the others mostly below; user
    5's samples are all equal; user 6's samples span +-30 (temperature 0.25: exponents down to -240, which underflow); user 8 holds a
    positive 100 above every sample (its loss underflows) and one 100 below (loss about 100 / temperature); go is non-uniform and every
    seventh entry is exactly 0."""
    rng = np.random.default_rng(4241 * S + seed)
    nu, ni = len(POSITIVES), N_ITEMS
    rows, cols, vals = [], [], []
    for u, n_pos in enumerate(POSITIVES):
        n_neg = 0 if u == 0 else (3 if n_pos < 100 else 40)
        c = np.sort(rng.choice(ni, size=n_pos + n_neg, replace=False))
        v = rng.uniform(0.25, 3.0, size=c.size)
        neg = rng.choice(c.size, size=n_neg, replace=False)
        v[neg] = np.where(np.arange(n_neg) % 2 == 0, -1.0, 0.0)
        rows += [u] * c.size
        cols += list(c)
        vals += list(v)
    m = sp.csr_matrix((np.array(vals, np.float32), (np.array(rows), np.array(cols))), shape=(nu, ni))
    assert m.nnz == len(vals)                                       # explicit zeros stay stored
    indptr, values = m.indptr.astype(np.int64), m.data.astype(np.float32)
    pred = rng.standard_normal(m.nnz).astype(np.float32)
    samp = rng.standard_normal((nu, S)).astype(np.float32)
    samp[U_EQUAL] = np.float32(0.3)
    samp[U_SPAN] = rng.permutation(np.linspace(-30.0, 30.0, S)).astype(np.float32)

    def positives(u):
        idx = np.arange(indptr[u], indptr[u + 1])
        return idx[values[idx] > 0]
    p2, p8 = positives(U_PLANTED_M), positives(U_FAR)
    pred[p2[3]] = samp[U_PLANTED_M].max() + np.float32(0.75)
    pred[p2[40]] = samp[U_PLANTED_M].max()
    pred[p8[5]] = samp[U_FAR].max() + np.float32(100.0)
    pred[p8[20]] = samp[U_FAR].min() - np.float32(100.0)
    n_pos = int((values > 0).sum())
    go = rng.uniform(0.5, 1.5, n_pos).astype(np.float32)
    go[::7] = 0.0
    planted = SimpleNamespace(above=p2[3], equal=p2[40], far_above=p8[5], far_below=p8[20])
    return SimpleNamespace(matrix=m, indptr=indptr, values=values, pred=pred, samp=samp, go=go, n_users=nu, n_items=ni, S=S,
                           planted=planted)


def case_properties(case):
    """what the issue asks the data to hold, as a dict the host test asserts"""
    pos = case.values > 0
    per_user = np.array([int(pos[case.indptr[u]:case.indptr[u + 1]].sum()) for u in range(case.n_users)])
    M2, p = case.samp[U_PLANTED_M].max(), case.planted
    idx2 = np.arange(case.indptr[U_PLANTED_M], case.indptr[U_PLANTED_M + 1])
    idx2 = idx2[pos[idx2]]
    return dict(positives=list(per_user), interactions_user1=int(case.indptr[2] - case.indptr[1]),
                negatives=int((case.values < 0).sum()), zeros=int((case.values == 0).sum()),
                above=bool(case.pred[p.above] > M2), equal=bool(case.pred[p.equal] == M2), below=bool((case.pred[idx2] < M2).any()),
                all_equal=bool((case.samp[U_EQUAL] == case.samp[U_EQUAL, 0]).all()),
                span=float(case.samp[U_SPAN].max() - case.samp[U_SPAN].min()),
                far_above=float(case.pred[p.far_above] - case.samp[U_FAR].max()),
                far_below=float(case.samp[U_FAR].min() - case.pred[p.far_below]),
                go_zeros=int((case.go == 0).sum()), go_distinct=int(np.unique(case.go).size))
