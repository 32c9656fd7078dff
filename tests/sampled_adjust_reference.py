"""Float64 references, error bars and inputs for the adjusted sampled softmax and BPR kernels (csrc/loss_sampled.hip:
trec_sampled_softmax_adj_* / trec_bpr_adj_*): accidental hits removed and / or the logQ correction.  NumPy only, nothing of the code
under test; constants and conventions are those of tests/sampled_loss_reference.py, which this module imports and extends.

Definitions.  t = 1 / temperature; sample s of user u is a HIT (h_us = 1) when its item is the column of an interaction of u with a
value > 0 -- a value <= 0 is no hit, the mask is per user; kept = not a hit (or every sample when hits are not removed).
    c_us    = -log(S q(item_us)) with the correction, else 0; q from log_q [n_items] (float32, taken as exact) or 1 / n_items
    softmax   loss_p = log(1 + sum_{kept} exp((y_s - y_p) t + c_s));  no kept sample: loss_p = 0 and every gradient of the user is 0
    BPR       loss_p = (1 / S) sum_{kept} softplus(y_s - y_p)      -- divided by S, not by the number kept; no c
The kernels' form of the softmax:  R = max_kept y_s,  w_s = (y_s - R) t + c_s,  M = max_kept w_s,  E_s = exp(w_s - M),  Z = sum E_s,
w_p = (y_p - R) t,  m = max(M, w_p),  a = exp(w_p - m),  b = exp(M - m),  D = a + b Z,  loss_p = (m - w_p) + log D,
d y_p = -go_p t b Z / D,  d y_us = t E_s K_u (kept) or 0 (hit),  K_u = sum_p go_p b_p / D_p.

Bars: the derivation of sampled_loss_reference (u = 2^-24, counts in units of u, LIB = 4 per library function, DIV = 2) with these
changes.  R is a maximum of inputs and exact.  The loss and the gradients do not depend on the shift M (b Z, E_s b_p / D_p and
(m - w_p) + log D are invariant), so the M the kernel finds -- a float32 maximum of rounded w -- is taken as the shift of the
reference too and contributes nothing; only |w_s - M| below moves by the error of M, a second-order term.
    c_s     log S (rounded once on the host) plus log q (float32 input), one addition: held to (LIB + 1) |c_s| absolute -- "logf's two
            ulps inside c as stored in float32" and the one extra addition; 0 without the correction
    w_s     difference, t, product: 3 |y_s - R| t;  the addition of c: |w_s|;  the error of c           -> absolute dw_s
    E_s     the argument w_s - M is rounded (|w_s - M|) and carries dw_s; expf LIB: relative dw_s + |w_s - M| + LIB =: e_rel_s
    Z       sum E_s e_rel_s + S Z, + S TINY                                                              -> relative rz
    w_p     3 |y_p - R| t absolute =: dp;   a, b: relative dp + |w_p - m| + LIB resp. dp + |M - m| + LIB  (either may be the branch
            taken when w_p and M are within dp of each other; both are continuous there)
    D, loss, d y_p, K, d y_us: as in sampled_loss_reference with these ea, eb, rz, and (m - w_p): |m - w_p| + dp instead of 3 (m - y_p) t.
BPR: a hit adds an exact 0 to every sum (softplus(-inf) = 0, sigma(-inf) = 0), which rounds nothing: the bars of sampled_loss_reference
over the kept samples, with S -- the divisor and the number of slots a sum may pass through -- unchanged.
Entries that must be exactly 0 (sampled_loss_reference's, d y_us of a hit, everything of a user without a kept sample) have a bar of 0."""
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

from sampled_loss_reference import U32, TINY, LIB, DIV, f64, _users, bars  # noqa: F401  (bars: re-exported)


def hit_mask(indptr, cols, values, items, count_non_positives=False):
    """[U, S] bool: the sample's item is the column of one of the user's interactions with a value > 0"""
    items = np.asarray(items)
    out = np.zeros(items.shape, bool)
    for u in range(items.shape[0]):
        idx = np.arange(indptr[u], indptr[u + 1])
        if not count_non_positives:
            idx = idx[np.asarray(values)[idx] > 0]
        out[u] = np.isin(items[u], np.asarray(cols)[idx])
    return out


def corrections(items, log_q, n_items, S):
    """c [U, S] float64 = -(log S + log q(item)); log_q float32 [n_items] or None (uniform)"""
    lq = f64(log_q)[np.asarray(items)] if log_q is not None else np.full(np.shape(items), -np.log(float(n_items)))
    return -(np.log(float(S)) + lq)


def ref_sampled_softmax_adj(case, temperature, log_q_correction, remove_hits, log_q="case"):
    """loss [P+], d_pred [P], d_samp [U, S] of sum_p go_p loss_p with the options, and their bars"""
    indptr, values, pred, samp, go = case.indptr, case.values, f64(case.pred), f64(case.samp), f64(case.go)
    n_users, S = samp.shape
    t = 1.0 / float(temperature)
    hits = hit_mask(indptr, case.cols, values, case.items) if remove_hits else np.zeros(samp.shape, bool)
    log_q = case.log_q if isinstance(log_q, str) else log_q
    cs = corrections(case.items, log_q, case.n_items, S) if log_q_correction else np.zeros(samp.shape)
    n_pos = int((np.asarray(values) > 0.0).sum())
    loss, bar_loss = np.zeros(n_pos), np.zeros(n_pos)
    d_pred, bar_d_pred = np.zeros(pred.size), np.zeros(pred.size)
    d_samp, bar_d_samp = np.zeros(samp.shape), np.zeros(samp.shape)
    for u, idx, n, slot, pos in _users(indptr, values):
        kept = ~hits[u]
        if not idx.size or not kept.any():
            continue
        ys, c = samp[u][kept], cs[u][kept]
        R = ys.max()
        w = (ys - R) * t + c
        dw = U32 * (3.0 * np.abs(ys - R) * t + np.abs(w) + (LIB + 1.0) * np.abs(c))
        M = w.max()
        E = np.exp(w - M)
        Z = E.sum()
        e_rel = dw + (np.abs(w - M) + LIB) * U32
        rz = ((E * e_rel).sum() + S * U32 * Z + S * TINY) / Z
        yp, g = pred[idx], go[slot[idx]]
        wp = (yp - R) * t
        dp = 3.0 * U32 * np.abs(yp - R) * t
        m = np.maximum(M, wp)
        a, b = np.exp(wp - m), np.exp(M - m)
        ea, eb = dp + (np.abs(wp - m) + LIB) * U32, dp + (np.abs(M - m) + LIB) * U32
        bz = b * Z
        D = a + bz
        rD = (a * ea + bz * (eb + rz + U32) + (1.0 + Z) * TINY) / D + U32
        logD = np.where(wp >= M, np.log1p(bz), np.log(D))
        lo = (m - wp) + logD
        loss[slot[idx]] = lo
        bar_loss[slot[idx]] = rD + LIB * U32 * logD + U32 * (m - wp) + dp + U32 * lo
        r = bz / D
        rr = eb + rz + U32 + rD + DIV * U32
        d_pred[idx] = -g * t * r
        bar_d_pred[idx] = np.abs(g) * t * r * (rr + 3.0 * U32) + np.abs(g) * t * (Z + 2.0) * TINY + TINY
        term = g * b / D
        rt = eb + U32 + rD + DIV * U32
        K, aK = term.sum(), np.abs(term).sum()
        dK = (np.abs(term) * rt).sum() + n * U32 * aK + n * (np.abs(g).max() + 1.0) * TINY
        d_samp[u, kept] = t * E * K
        bar_d_samp[u, kept] = t * E * (aK * (e_rel + 3.0 * U32) + dK) + (t * aK + 1.0) * TINY
    return SimpleNamespace(loss=loss, d_pred=d_pred, d_samp=d_samp, bar_loss=bar_loss, bar_d_pred=bar_d_pred, bar_d_samp=bar_d_samp,
                           hits=hits, c=cs)


def ref_bpr_adj(case, remove_hits=True):
    indptr, values, pred, samp, go = case.indptr, case.values, f64(case.pred), f64(case.samp), f64(case.go)
    n_users, S = samp.shape
    hits = hit_mask(indptr, case.cols, values, case.items) if remove_hits else np.zeros(samp.shape, bool)
    n_pos = int((np.asarray(values) > 0.0).sum())
    loss, bar_loss = np.zeros(n_pos), np.zeros(n_pos)
    d_pred, bar_d_pred = np.zeros(pred.size), np.zeros(pred.size)
    d_samp, bar_d_samp = np.zeros(samp.shape), np.zeros(samp.shape)
    for u, idx, n, slot, pos in _users(indptr, values):
        kept = ~hits[u]
        if not idx.size or not kept.any():
            continue
        yp, g = pred[idx], go[slot[idx]]
        X = samp[u][kept][None, :] - yp[:, None]
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
        dpv = -c * sig.sum(1)
        d_pred[idx] = dpv
        bar_d_pred[idx] = np.abs(c) * ((sig * rs).sum(1) + 2.0 * S * TINY) + (S + 3.0) * U32 * np.abs(dpv) + TINY
        T = np.abs(c)[:, None] * sig
        d_samp[u, kept] = (c[:, None] * sig).sum(0)
        bar_d_samp[u, kept] = (T * (rs + 3.0 * U32)).sum(0) + n * U32 * T.sum(0) + (2.0 * np.abs(c).sum() + n) * TINY
    return SimpleNamespace(loss=loss, d_pred=d_pred, d_samp=d_samp, bar_loss=bar_loss, bar_d_pred=bar_d_pred, bar_d_samp=bar_d_samp,
                           hits=hits)


# ------------------------------------------------------------------------------------------------ inputs
SAMPLE_COUNTS = [1, 63, 64, 65, 256, 257, 300]           # both forms below 257, the workgroup form above
TEMPERATURES = [1.0, 0.25]
N_ITEMS = 2700
# (positives, non-positives) per user
USERS = [(0, 0), (0, 3), (65, 3), (1025, 40), (1, 0), (4, 3), (17, 3), (30, 3), (64, 3), (3, 0), (300, 40)]
U_NONE, U_NONPOS, U_MAX_HIT, U_TRIPLE, U_ROW1, U_NO_HIT, U_NONPOS_ITEM, U_ALL_HITS, U_ENDS = 0, 1, 2, 3, 4, 6, 7, 8, 9
MAX_HIT_MARGIN = 200.0
# softmax configurations: (log_q_correction, remove_hits, log_q "case" | None); BPR has the hit removal only
CONFIGS = {"logq": (True, False, "case"), "logq-uniform": (True, False, None), "hits": (False, True, "case"),
           "both": (True, True, "case"), "both-uniform": (True, True, None)}


def adjust_case(S, seed=0):
    """11 users x 2,700 items: users with 0 (no interaction / non-positives only), 1, 65 and 1,025 positives and a few more, negative
    and explicit-zero interactions mixed in; random sampled ids (so hits occur by chance: user 3 holds 38 %, user 10 11 % of the
    catalogue) with these rows planted:
      user 2  the sample with the largest prediction is a hit, 200 above the others (a maximum taken over masked samples underflows
              every kept term at temperature 0.25);     user 3  the same hit item in slots 0, 1, 2;
      user 4  a row of length 1, its item in slot 0;    user 6  no hit (ids from outside the row);
      user 7  slot 0 holds the item of an interaction of value <= 0: no hit;
      user 8  every sample a hit;                       user 9  slot 0 / the last slot hold the first / last entry of the CSR row.
    log_q spans -2 ... -14 over the items (any table will do: the kernels do not ask for a distribution); go is non-uniform with
    every seventh entry exactly 0.  For S < 3 the planted slots overlap: later plants win, the references take the ids as they are."""
    rng = np.random.default_rng(977 * S + seed)
    nu, ni = len(USERS), N_ITEMS
    rows, cols, vals = [], [], []
    for u, (n_pos, n_neg) in enumerate(USERS):
        c = np.sort(rng.choice(ni, size=n_pos + n_neg, replace=False))
        v = rng.uniform(0.25, 3.0, size=c.size)
        neg = rng.choice(c.size, size=n_neg, replace=False)
        v[neg] = np.where(np.arange(n_neg) % 2 == 0, -1.0, 0.0)
        rows += [u] * c.size
        cols += list(c)
        vals += list(v)
    m = sp.csr_matrix((np.array(vals, np.float32), (np.array(rows), np.array(cols))), shape=(nu, ni))
    assert m.nnz == len(vals) and m.has_sorted_indices
    indptr, values, xcols = m.indptr.astype(np.int64), m.data.astype(np.float32), m.indices.astype(np.int32)
    pred = rng.standard_normal(m.nnz).astype(np.float32)
    samp = rng.standard_normal((nu, S)).astype(np.float32)
    items = rng.integers(0, ni, size=(nu, S)).astype(np.int32)

    def row(u, positive=None):
        idx = np.arange(indptr[u], indptr[u + 1])
        if positive is not None:
            idx = idx[(values[idx] > 0) == positive]
        return xcols[idx]
    k = int(np.argmax(samp[U_MAX_HIT]))
    items[U_MAX_HIT, k] = row(U_MAX_HIT, True)[7]
    samp[U_MAX_HIT, k] += np.float32(MAX_HIT_MARGIN)
    items[U_TRIPLE, :3] = row(U_TRIPLE, True)[500]
    items[U_ROW1, 0] = row(U_ROW1)[0]
    outside = np.setdiff1d(np.arange(ni), row(U_NO_HIT))
    items[U_NO_HIT] = rng.choice(outside, size=S).astype(np.int32)
    items[U_NONPOS_ITEM, 0] = row(U_NONPOS_ITEM, False)[0]
    items[U_ALL_HITS] = rng.choice(row(U_ALL_HITS, True), size=S).astype(np.int32)
    items[U_ENDS, 0], items[U_ENDS, -1] = row(U_ENDS)[0], row(U_ENDS)[-1]
    log_q = rng.permutation(np.linspace(-2.0, -14.0, ni)).astype(np.float32)
    n_pos = int((values > 0).sum())
    go = rng.uniform(0.5, 1.5, n_pos).astype(np.float32)
    go[::7] = 0.0
    return SimpleNamespace(matrix=m, indptr=indptr, values=values, cols=xcols, pred=pred, samp=samp, go=go, items=items, log_q=log_q,
                           n_users=nu, n_items=ni, S=S, max_hit_slot=k)
