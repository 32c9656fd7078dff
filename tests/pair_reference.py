"""Float64 references, error bars and inputs for the pair-score kernels (csrc/pair_score.hip) and the WMRB kernels (csrc/loss.hip).
NumPy / SciPy only: no torch, nothing of the code under test.  tests/test_pair_reference_host.py holds the references and the bars to
float32 restatements of the same chains on the CPU; tests/test_gpu_pair_kernels.py holds the kernels to the references.

Bars.  u = 2^-24 is the unit roundoff of float32; a float32 ulp of x is at most 2 u |x|.

* one pair, dot            the kernel adds the d products with one fmaf each (one rounding per term) and joins up to 64 lanes with a
                           six-level butterfly; a term passes through at most d + 6 roundings, so |s^ - s| <= (d + 8) u A_p with
                           A_p = sum_c |u_c v_c| (the issue's chain bar; the two spare units cover the second-order terms).
* one pair, Euclidean      D = sum_c (u_c - v_c)^2: the difference is rounded before it is squared (2 u relative on the term), then the
                           same chain: (d + 6 + 2) u D = (d + 8) u D.  s = -sqrt(max(D, 1e-16)): a relative error e on D is e / 2 on
                           the root, the root itself is within two ulps (4 u): ((d + 8) / 2 + 4) u sqrt(D), sqrt(D) taken as 1e-8 at
                           least (a clamped pair is the constant -1e-8 on both sides).
* a bias add               one more rounding of the running value: u |s + b_u|, then u |s + b_u + b_i|.
* a gradient entry         a float32 sum of m terms in any order (chain, chunks of chains, atomics): every term passes through at most
                           m - 1 additions: m u sum |terms|.  The terms carry their own roundings, k per term:
                           dot        the product g_p v_c (rounded on the atomic route, fused on the others): k = 1;
                           Euclidean  c_p (x_c - y_c) with c_p = -g_p / sqrt(D_p): (d + 8) / 2 from D, 4 for the root, 2 for the division
                                      (within an ulp), 1 for the difference, 1 for the product: k = (d + 8) / 2 + 8.
                           Bar: (m + k) u sum |terms|.  Bias gradients are plain sums of g_p: m u sum |g_p|.
* Euclidean coefficient    ((d + 8) / 2 + 6) u |c_p|, and exactly 0 where D_p < 1e-16.
* WMRB                     predictions and samples are multiples of 2^-10 of magnitude 4 at most, so every hinge term 1 - p + s (9 at
                           most) and every partial sum of up to 1,024 of them is a multiple of 2^-10 below 2^14 -- fewer than 24 bits:
                           exact in float32 in ANY order (asserted by wmrb_inputs_exact).  What is left is ratio = n_items / S (u), ratio * sum (u), * weight (u): smr within
                           3 u; smr + 1 (u): x = 1 + smr within 4 u relative, i.e. 4 u absolute on log x; logf within two ulps:
                           loss bar u (4 + 4 |loss|).
                           c_p = go ratio w / (1 + smr): 2 + 4 + 2 (division) + 1 = 9 u; d pred_p = -c_p * count (count exact): 10 u |d pred|;
                           d samp[u, s] = sum of the n active c_p (adding an inactive 0 is exact): (n + 9) u sum |c_p|.
"""
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

U32 = 2.0 ** -24
EPS = 1e-16
MODE_DOT, MODE_EUCLID = 0, 1
SPLIT_T = 2048
GRID = 1024.0                    # WMRB inputs are multiples of 1 / GRID


def f64(a):
    return np.asarray(a, dtype=np.float64)


# ------------------------------------------------------------------------------------------------ pair scores
def ref_pair_scores(U, V, xu, xi, mode, ub=None, ib=None, chunk=16384):
    """scores: the float64 scores; raw: before the biases; with_ub: after the user bias; mag: A_p (dot) or D_p (Euclidean)"""
    U, V = f64(U), f64(V)
    xu, xi = np.asarray(xu, dtype=np.int64), np.asarray(xi, dtype=np.int64)
    n = xi.size
    raw, mag = np.empty(n), np.empty(n)
    for a in range(0, n, chunk):
        x, y = U[xu[a:a + chunk]], V[xi[a:a + chunk]]
        if mode == MODE_DOT:
            t = x * y
            raw[a:a + chunk], mag[a:a + chunk] = t.sum(1), np.abs(t).sum(1)
        else:
            D = ((x - y) ** 2).sum(1)
            raw[a:a + chunk], mag[a:a + chunk] = -np.sqrt(np.maximum(D, EPS)), D
    with_ub = raw + f64(ub)[xu] if ub is not None else raw
    scores = with_ub + f64(ib)[xi] if ib is not None else with_ub
    return SimpleNamespace(scores=scores, raw=raw, with_ub=with_ub, mag=mag, mode=mode, has_ub=ub is not None, has_ib=ib is not None)


def chain_bar(ref, d):
    """the accumulated A_p / D_p itself (out_sqdist): (d + 8) u mag"""
    return (d + 8) * U32 * ref.mag


def score_bar(ref, d):
    if ref.mode == MODE_DOT:
        b = chain_bar(ref, d)
    else:
        b = ((d + 8) / 2.0 + 4.0) * U32 * np.maximum(np.sqrt(ref.mag), 1e-8)
    if ref.has_ub:
        b = b + U32 * np.abs(ref.with_ub)
    if ref.has_ib:
        b = b + U32 * np.abs(ref.scores)
    return b


def ref_pair_grads(U, V, xu, xi, g, mode, chunk=16384):
    """closed-form dU, dV, dub, dib of sum_p g_p s_p, the per-entry sums of absolute terms (aU, aV, aub, aib), the number of terms per
    user / item (cnt_u, cnt_i) and, Euclidean, the coefficients c_p (0 where D_p < 1e-16: tf.maximum sends the gradient to the constant)"""
    U, V, g = f64(U), f64(V), f64(g)
    xu, xi = np.asarray(xu, dtype=np.int64), np.asarray(xi, dtype=np.int64)
    nu, ni, n = U.shape[0], V.shape[0], xi.size
    dU, dV, aU, aV = np.zeros_like(U), np.zeros_like(V), np.zeros_like(U), np.zeros_like(V)
    coef, D = g.copy(), np.zeros(n)
    for a in range(0, n, chunk):
        ku, ki, gc = xu[a:a + chunk], xi[a:a + chunk], g[a:a + chunk]
        x, y = U[ku], V[ki]
        m = ku.size
        su = sp.csr_matrix((np.ones(m), (ku, np.arange(m))), shape=(nu, m))
        si = sp.csr_matrix((np.ones(m), (ki, np.arange(m))), shape=(ni, m))
        if mode == MODE_DOT:
            tu, tv = gc[:, None] * y, gc[:, None] * x
        else:
            Dc = ((x - y) ** 2).sum(1)
            c = np.where(Dc >= EPS, -gc / np.sqrt(np.maximum(Dc, 1e-300)), 0.0)
            coef[a:a + chunk], D[a:a + chunk] = c, Dc
            tu = c[:, None] * (x - y)
            tv = -tu
        dU += su @ tu
        dV += si @ tv
        aU += su @ np.abs(tu)
        aV += si @ np.abs(tv)
    return SimpleNamespace(dU=dU, dV=dV, aU=aU, aV=aV, coef=coef, D=D, mode=mode,
                           dub=np.bincount(xu, weights=g, minlength=nu), dib=np.bincount(xi, weights=g, minlength=ni),
                           aub=np.bincount(xu, weights=np.abs(g), minlength=nu), aib=np.bincount(xi, weights=np.abs(g), minlength=ni),
                           cnt_u=np.bincount(xu, minlength=nu).astype(np.float64), cnt_i=np.bincount(xi, minlength=ni).astype(np.float64))


def term_roundings(d, mode):
    return 1.0 if mode == MODE_DOT else (d + 8) / 2.0 + 8.0


def grad_bars(ref, d):
    """(bar dU, bar dV, bar dub, bar dib)"""
    k = term_roundings(d, ref.mode)
    return ((ref.cnt_u[:, None] + k) * U32 * ref.aU, (ref.cnt_i[:, None] + k) * U32 * ref.aV,
            ref.cnt_u * U32 * ref.aub, ref.cnt_i * U32 * ref.aib)


def coef_bar(ref, d):
    return ((d + 8) / 2.0 + 6.0) * U32 * np.abs(ref.coef)


# ------------------------------------------------------------------------------------------------ which kernel a call takes
ALL_FWD_INSTANTIATIONS = {(4, 1, 0), (1, 1, 0), (4, 2, 0), (4, 4, 0), (1, 2, 0), (4, 2, 2), (4, 4, 4)}


def fwd_instantiation(d, n_pairs, pairs_per_user=0, pp_tuning=None, ug_tuning=1):
    """<VEC, PP, UG> of pair_score_fwd_kernel that trec_pair_score_fwd launches (pairs_per_user > 0: implicit users)"""
    implicit = pairs_per_user > 0
    vec = 4 if d % 4 == 0 else 1
    pp = 1
    if n_pairs >= 65536:
        pp = pp_tuning if pp_tuning is not None else (4 if implicit and pairs_per_user % 4 == 0 else 2)
    pp = 4 if (pp >= 4 and vec == 4) else (2 if pp >= 2 else 1)
    if implicit and vec == 4 and ug_tuning and pp >= 2 and pairs_per_user % pp == 0:
        return (4, pp, pp)
    return (vec, pp, 0)


def split_ok(d):
    return (d % 4 == 0 and d <= 1024) or d <= 256


def prefer_split(d, nnz):
    return d % 4 != 0 and d <= 256 and nnz >= 65536


BWD_ENTRY_POINTS = ("trec_pair_score_bwd", "trec_spmm_csr", "trec_spmm_csr_split", "trec_pair_euclid_coef")


def bwd_routes(form, mode, d, n_pairs, long_u, long_i):
    """the entry points of BWD_ENTRY_POINTS that _PairScore.backward calls (ops_base.py); form: plain / implicit / inter"""
    if form == "plain" or (mode == MODE_EUCLID and not split_ok(d)):
        return {"trec_pair_score_bwd"}
    if mode == MODE_EUCLID:
        return {"trec_pair_euclid_coef", "trec_spmm_csr_split"}
    out = set()
    for long_side in (long_u, long_i):
        out.add("trec_spmm_csr_split" if (long_side or prefer_split(d, n_pairs)) and split_ok(d) else "trec_spmm_csr")
    return out


# ------------------------------------------------------------------------------------------------ inputs: forward
FWD_D = [4, 8, 20, 128, 260, 5, 67]
FWD_N_PAIRS = [65535, 65536, 65539]
FWD_PPU = [4, 6, 7]
FWD_IMPLICIT_USERS = 16385
FWD_TUNINGS = [(pp, ug) for pp in (1, 2, 4) for ug in (0, 1)]


def _tables(nu, ni, d, rng):
    return rng.standard_normal((nu, d)).astype(np.float32), rng.standard_normal((ni, d)).astype(np.float32)


def fwd_explicit_case(d, n_pairs):
    """50 users x 70 items, explicit indices.  Items 5 and 6 carry the rows of users 7 and 8: the pairs (7, 5) and (8, 6) are clamped;
    they sit at the front, at the very end (inside the ragged tail of PP = 2 / 4) and a few hundred times in between."""
    rng = np.random.default_rng(1000 * d + n_pairs % 1000)
    U, V = _tables(50, 70, d, rng)
    V[5], V[6] = U[7], U[8]
    xu, xi = rng.integers(0, 50, n_pairs), rng.integers(0, 70, n_pairs)
    xu[[0, 1, -1]], xi[[0, 1, -1]] = [7, 8, 7], [5, 6, 5]
    ub, ib = rng.standard_normal(50).astype(np.float32), rng.standard_normal(70).astype(np.float32)
    return SimpleNamespace(U=U, V=V, xu=xu.astype(np.int32), xi=xi.astype(np.int32), ub=ub, ib=ib, ppu=0)


def fwd_implicit_case(d, ppu):
    """16,385 users x 70 items, user of pair p = p // ppu.  Users 7 and 16,384 (the last group) carry the rows of items 5 and 6 and
    hold them as their first / last pair."""
    rng = np.random.default_rng(77 * d + ppu)
    nu = FWD_IMPLICIT_USERS
    U, V = _tables(nu, 70, d, rng)
    U[7], U[nu - 1] = V[5], V[6]
    items = rng.integers(0, 70, (nu, ppu))
    items[7, 0], items[nu - 1, ppu - 1] = 5, 6
    ub, ib = rng.standard_normal(nu).astype(np.float32), rng.standard_normal(70).astype(np.float32)
    return SimpleNamespace(U=U, V=V, xu=np.repeat(np.arange(nu), ppu).astype(np.int32), xi=items.reshape(-1).astype(np.int32),
                           ub=ub, ib=ib, ppu=ppu)


def clamped_pairs(case):
    """pairs whose two rows are identical (D_p = 0 < 1e-16)"""
    return (case.U[case.xu] == case.V[case.xi]).all(1)


# ------------------------------------------------------------------------------------------------ inputs: backward
BWD_USERS, BWD_ITEMS, BWD_PPU = 2200, 50, 30
BWD_D = [8, 5, 260, 261]            # 5: _prefer_split; 8, 260: _split_ok only; 261: neither
BWD_FORMS = ["plain", "implicit", "inter"]
BWD_EMPTY_USER, BWD_EMPTY_ITEM, BWD_LONG_ITEM = 7, 5, 0
BWD_CLAMPED = [(10, 3), (11, 4)]


def bwd_case(form, d):
    """2,200 users x 50 items, more than 65,536 pairs.  Item 0 holds the pairs of 2,099 or more users (> SPLIT_T), item 5 none, user 7
    none (plain and inter: implicit users all hold BWD_PPU pairs); users 10 and 11 carry the rows of items 3 and 4 and hold them;
    plain and implicit lists repeat pairs (an Interactions matrix holds a cell once)."""
    rng = np.random.default_rng(31 * d + len(form))
    nu, ni = BWD_USERS, BWD_ITEMS
    U, V = _tables(nu, ni, d, rng)
    for a, b in BWD_CLAMPED:
        U[a] = V[b]
    ub, ib = rng.standard_normal(nu).astype(np.float32), rng.standard_normal(ni).astype(np.float32)
    matrix = None
    if form == "inter":
        dense = rng.random((nu, ni)) < 0.62
        dense[:2100, BWD_LONG_ITEM] = True
        for a, b in BWD_CLAMPED:
            dense[a, b] = True
        dense[BWD_EMPTY_USER, :] = False
        dense[:, BWD_EMPTY_ITEM] = False
        matrix = sp.csr_matrix(dense.astype(np.float32))
        coo = matrix.tocoo()                                  # row-major, the serial order of Interactions
        xu, xi = coo.row.astype(np.int64), coo.col.astype(np.int64)
        ppu = 0
    else:
        items = rng.integers(0, ni, (nu, BWD_PPU))
        items[items == BWD_EMPTY_ITEM] = BWD_EMPTY_ITEM + 1
        items[:2100, 2] = BWD_LONG_ITEM
        items[::3, 1] = items[::3, 0]                         # repeated pairs
        for a, b in BWD_CLAMPED:
            items[a, 3] = b
        xu, xi = np.repeat(np.arange(nu), BWD_PPU), items.reshape(-1)
        ppu = BWD_PPU
        if form == "plain":
            xu = xu.copy()
            moved = xu == BWD_EMPTY_USER
            xu[moved] = BWD_EMPTY_USER + 1                    # user 7 gives its pairs to user 8 (more repeats)
            order = rng.permutation(xu.size)
            xu, xi, ppu = xu[order], xi[order], 0
    g = rng.standard_normal(xi.size).astype(np.float32)
    return SimpleNamespace(U=U, V=V, xu=xu.astype(np.int32), xi=xi.astype(np.int32), g=g, ub=ub, ib=ib, ppu=ppu, matrix=matrix,
                           form=form, d=d)


def bwd_case_properties(case):
    """what the issue asks the data to hold, as a dict of booleans / counts the host test asserts"""
    cu, ci = np.bincount(case.xu, minlength=BWD_USERS), np.bincount(case.xi, minlength=BWD_ITEMS)
    key = case.xu.astype(np.int64) * BWD_ITEMS + case.xi
    return dict(n_pairs=int(case.xi.size), empty_user=bool((cu == 0).any()), empty_item=bool((ci == 0).any()),
                repeated=int(key.size - np.unique(key).size), clamped=int(clamped_pairs(case).sum()),
                max_item=int(ci.max()), max_user=int(cu.max()))


# ------------------------------------------------------------------------------------------------ WMRB
def ref_wmrb(indptr, values, weight, pred, samp, n_items, go):
    """loss [P+], d pred [P], d samp [U, S] of sum_p go_p loss_p (loss_graphs.py:153-227): positives only, the hinge passes the gradient
    at >= 0 (tf.maximum), weight: value_p / item sum for BalancedWMRB (None: WMRB).  Also a_samp / n_samp (sum |c_p| and number of the
    active c_p of every sample), the number of hinges that are exactly 0 and the users whose hinges are all inactive."""
    indptr, values, pred, samp, go = np.asarray(indptr), f64(values), f64(pred), f64(samp), f64(go)
    n_users, S = samp.shape
    ratio = float(n_items) / float(S)
    pos = values > 0.0
    slot = np.cumsum(pos) - 1
    loss, d_pred = np.zeros(int(pos.sum())), np.zeros(pred.size)
    d_samp, a_samp, n_samp = np.zeros(samp.shape), np.zeros(samp.shape), np.zeros(samp.shape)
    zero_hinges, inactive_users, max_sum = np.zeros(n_users, dtype=np.int64), [], 0.0
    for u in range(n_users):
        idx = np.arange(indptr[u], indptr[u + 1])
        idx = idx[pos[idx]]
        if not idx.size:
            continue
        H = 1.0 - pred[idx][:, None] + samp[u][None, :]
        act = H >= 0.0
        w = f64(weight)[idx] if weight is not None else 1.0
        hs = np.maximum(H, 0.0).sum(1)
        smr = ratio * hs * w
        loss[slot[idx]] = np.log(smr + 1.0)
        c = go[slot[idx]] * ratio * w / (1.0 + smr)
        d_pred[idx] = -c * act.sum(1)
        d_samp[u] = (c[:, None] * act).sum(0)
        a_samp[u] = (np.abs(c)[:, None] * act).sum(0)
        n_samp[u] = act.sum(0)
        zero_hinges[u] = int((H == 0.0).sum())
        max_sum = max(max_sum, float(hs.max()))
        if not act.any():
            inactive_users.append(u)
    return SimpleNamespace(loss=loss, d_pred=d_pred, d_samp=d_samp, a_samp=a_samp, n_samp=n_samp, zero_hinges=zero_hinges,
                           inactive_users=inactive_users, max_sum=max_sum, slot=slot, pos=pos)


def wmrb_bars(ref):
    """(bar loss, bar d pred, bar d samp)"""
    return (U32 * (4.0 + 4.0 * np.abs(ref.loss)), 10.0 * U32 * np.abs(ref.d_pred), (ref.n_samp + 9.0) * U32 * ref.a_samp)


def wmrb_inputs_exact(pred, samp):
    """the premise of the WMRB bars: multiples of 2^-10 of magnitude 4 at most, at most 1,024 samples"""
    p, s = f64(pred) * GRID, f64(samp) * GRID
    return bool((p == np.round(p)).all() and (s == np.round(s)).all() and np.abs(f64(pred)).max() <= 4.0 and np.abs(f64(samp)).max() <= 4.0
                and samp.shape[1] <= 1024)


WMRB_S = [1, 63, 64, 65, 256, 257, 300]
WMRB_S_MANY = [40, 300]
WMRB_ITEMS = 2700
WMRB_POSITIVES = [0, 0, 65, 1025, 2600, 4, 17, 1, 30, 64, 3]        # per user; user 0 has no interaction, user 1 non-positives only
WMRB_INACTIVE_USER = 5


def wmrb_case(S, seed=0):
    """11 users x 2,700 items: users with 0 (no interaction at all / non-positive interactions only), 65, 1,025 and 2,600 positives and a few
    small ones; non-positive interactions (negative and explicit 0) are mixed in.  Values are multiples of 1/4 (so BalancedWMRB's weights are
    not 1).  pred / samp are multiples of 2^-10; every user with positives has one hinge set to exactly 0, except user 5, whose hinges are
    all inactive (predictions 4, samples 2 at most)."""
    rng = np.random.default_rng(977 * S + seed)
    nu, ni = len(WMRB_POSITIVES), WMRB_ITEMS
    rows, cols, vals = [], [], []
    for u, n_pos in enumerate(WMRB_POSITIVES):
        n_neg = 0 if u == 0 else (3 if n_pos < 100 else 40)
        c = np.sort(rng.choice(ni, size=n_pos + n_neg, replace=False))
        v = rng.integers(1, 13, size=c.size) / 4.0
        neg = rng.choice(c.size, size=n_neg, replace=False)
        v[neg] = np.where(np.arange(n_neg) % 2 == 0, -1.0, 0.0)
        rows += [u] * c.size
        cols += list(c)
        vals += list(v)
    m = sp.csr_matrix((np.array(vals, np.float32), (np.array(rows), np.array(cols))), shape=(nu, ni))
    assert m.nnz == len(vals)                                       # explicit zeros stay stored
    indptr, values = m.indptr.astype(np.int64), m.data.astype(np.float32)
    grid = lambda a: (np.round(np.clip(a, -3.0, 3.0) * GRID) / GRID).astype(np.float32)
    pred, samp = grid(rng.standard_normal(m.nnz)), grid(rng.standard_normal((nu, S)))
    for u in range(nu):
        idx = np.arange(indptr[u], indptr[u + 1])
        idx = idx[values[idx] > 0]
        if not idx.size:
            continue
        if u == WMRB_INACTIVE_USER:
            pred[idx] = 4.0
            samp[u] = np.minimum(samp[u], np.float32(2.0))
            continue
        samp[u, (7 * u) % S] = pred[idx[idx.size // 2]] - np.float32(1.0)       # 1 - p + s == 0
    n_pos = int((values > 0).sum())
    go = (np.round(rng.uniform(0.5, 1.5, n_pos) * 64) / 64).astype(np.float32)
    return SimpleNamespace(matrix=m, indptr=indptr, values=values, pred=pred, samp=samp, go=go, n_users=nu, n_items=ni, S=S)


def balanced_weights(case):
    """value_p / (sum of the positive values of p's item), 0 for non-positives, in float64; cnt: positives per item"""
    m = case.matrix
    vals, pos = f64(m.data), m.data > 0
    per_item = np.bincount(m.indices[pos], weights=vals[pos], minlength=m.shape[1])
    cnt = np.bincount(m.indices[pos], minlength=m.shape[1])
    w = np.zeros(m.nnz)
    w[pos] = vals[pos] / per_item[m.indices[pos]]
    return w, cnt[m.indices]
