"""Float64 reference, error bars, inputs and dispatch mirrors for the one-pass WMRB step kernels: csrc/wmrb_fused.hip
(trec_wmrb_fused_step), csrc/wmrb_tiled.hip + csrc/wmrb_tiled_body.hpp (trec_wmrb_tiled_step) and csrc/step_coop.hip
(trec_fit_step_coop).  NumPy / SciPy only, nothing of the code under test.  tests/test_step_reference_host.py holds the reference and
the bars to float32 restatements on the CPU (and shows that seeded defects fall outside); tests/test_gpu_wmrb_steps.py holds the
kernels to the reference.

Inputs.  Rows of U and V are multiples of 1/8 of magnitude 2 at most (item rows of the cooperative step: sums of up to nine such rows):
every product is a multiple of 2^-6, every partial sum of a dot product or of a squared distance is a multiple of 2^-6 below 2^13 --
fewer than 24 bits, exact in float32 in ANY order (inputs_exact asserts the premise).  Biases are multiples of 1/8.  (The planted
user entries of the cooperative cases are multiples of 1/64 of magnitude 128 at most, against item entries 0 / 1: the same holds, and
the tests assert that every hinge sum of a dot case is a multiple of 2^-6 below 2^18.)  Dot cases: every score, hinge 1 - y_q + y_s and hinge sum is exact and the active sets are unambiguous; hinges
of exactly 0 are planted.  Euclidean cases: only the square root rounds; step_bars asserts that the float64 reference holds no hinge
with |H| below the sum of the bars of its two scores (zero included), so the active sets are unambiguous there too.

Bars.  u = 2^-24; every bar is (roundings on the path) * u * (sum of |terms|), per element, plus what the element inherits.

* score           dot: exact (0).  Euclidean: D exact, sqrtf within 2 ulp (wmrb_tiled_body.hpp:145; 4 u), then one rounding per
                  bias add (:146-147): 4 u sqrt(D) + u |s + b_u| + u |s + b_u + b_i|.  Dot with biases: the adds are exact too.
* hinge sum hs_q  Euclidean only: every active hinge inherits sb_q + sb_s and is rounded twice (base = 1 - y_q, base + y_s:
                  :164, :175), the sum of S terms in 8 partials + 3 shuffles passes S roundings at most:
                  hb_q = sum_active (sb_q + sb_s + u (|1 - y_q| + |H|)) + S u hs_q.
* loss            ratio (1), ratio * hs (1), * w (1), + 1 (1): x = 1 + smr within 4 u relative = 4 u on log x, logf within 2 ulp
                  (4 u |loss|), and d loss / d hs = c:  u (4 + 4 |loss|) + c hb_q            (:192-196, wmrb_fused.hip:280-284)
* c_q             ratio / (1 + smr) * w: 1 + 4 + 2 (division) + 1 = 8, kept at pair_reference's 9;  d c / d hs = -c^2:
                  cb_q = 9 u c + c^2 hb_q
* g of a pair     -c * cnt (cnt exact: no ambiguous hinge), one product: 10 u |g| + cnt c^2 hb_q         (:197)
* g of a sample   sum of the n active c_q, a chain of n additions (:222-226; inactive ones add an exact 0):
                  (n + 9) u sum c + sum_active c_q^2 hb_q
* val             dot: g.  Euclidean: -g / sqrtf(D), 0 where D < 1e-16 (:201, :232): root 4 u, division 2 u:
                  vb = gb / sqrt(D) + 6 u |val|
* dU[u, c]        sum over the user's R rows of val_j * t_jc, t = V_jc (dot) or U_uc - V_jc (Euclidean, exact here): one fmaf per
                  term and at most R - 1 further additions (chain per subgroup, then the subgroups' partials, :278-303;
                  wmrb_fused.hip:315-331):  (R + 1) u sum |val_j t_jc| + sum vb_j |t_jc|
* d b_u           sum of the R values g_j (exactly 0 in exact arithmetic): per-thread chains, six shuffles, three adds
                  (:290-306; wmrb_fused.hip:333-337): (R + 9) u sum |g_j| + sum gb_j.  val_rowsum: the same on val.
* G[u, i]         the m values of the cell added by float atomics: m u sum |val| + sum vb        (:205, :236)
* dV[i, c]        sum over the n_i pairs of item i of val_p * U_uc (dot) / val_p * (V_ic - U_uc): one fmaf per term, n_i - 1
                  additions in any grouping (LDS tiles + atomics, step_coop.hip:176-187; K1 gathers; fp32 GEMM):
                  (n_i + 1) u sum |terms| + sum vb_p |t|;  through G the cell sums come first: + m_cell u on their terms,
                  bounded by using (n_i + 1 + m_max) u.
* d b_i           sum of the n_i values g_p: (n_i + 1) u sum |g_p| + sum gb_p.
* split-bf16 GEMM route (dense_g_split_bf16 = 1): d item_in and d user_in take 1e-4 * sum |terms| (include/tensorrec_hip.h:115-117),
                  Euclidean: of the products centred at the mean item row (ops_base.py:923-929, tests/test_gpu_fit_euclid.py).
* fp32 dense-G route of distances (dense_g_split_bf16 = 0): d user_in = rowsum(G) (U - c) - G . (V - c), d item_in = colsum(G) (V - c) -
                  G^T . (U - c) with c the float32 mean item row (ops_base.py:923-941).  In exact arithmetic c cancels; in float32 every
                  term val (U_uc - c_c) and val (V_jc - c_c) is formed on its own: the centring rounds once (1), the product (1), the
                  chain of R (n_i) terms of the GEMM plus the outer product and the subtraction (R + 2), the cells of G were summed
                  first (m_max): (R + 4 + m_max) u sum |val| (|U_uc - c_c| + |V_jc - c_c|) + sum vb (|U_uc - c_c| + |V_jc - c_c|)
                  (dense_fp32_euclid_bars; restated in float32 by tests/test_step_reference_host.py).
* item tower      V = X . W_i: fmaf in CSR order (step_coop.hip:91-99), k_i terms: k_i u sum |x w| -- exact (0) for the indicator
                  features (x = 1) and dyadic weights used here.  d W_i[f] = sum over the column's n_f items of x * dV[i]: n_f u sum |terms| +
                  sum dVb (:210-245); d beta_i alike.  L2: gg = g + l2 * w, two roundings (:31): + u (|l2 w| + |gg|).
"""
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

from pair_reference import EPS, MODE_DOT, MODE_EUCLID, U32, f64

GRID8 = 8.0


# ------------------------------------------------------------------------------------------------ reference
def ref_step(U, V, ub, ib, indptr, x_item, values, weight, samples, n_items, mode):
    """One WMRB / BalancedWMRB step with upstream gradient 1 in float64 (loss_graphs.py:153-227 of the reference project on the serial
    prediction graphs).  Hinges are active at >= 0; duplicate samples and samples that are also positives of the user each count as a
    pair of their own.  Returns the outputs, per output the sum of the absolute values of its terms (a*), and what step_bars needs."""
    U, V, values = f64(U), f64(V), f64(values)
    indptr, x_item, samples = np.asarray(indptr, np.int64), np.asarray(x_item, np.int64), np.asarray(samples, np.int64)
    n_users, d = U.shape
    S = samples.shape[1]
    nnz = x_item.size
    ratio = float(n_items) / float(S)
    pos = values > 0.0
    slot = np.cumsum(pos) - 1
    r = SimpleNamespace(mode=mode, S=S, d=d, n_users=n_users, n_items=n_items, pos=pos, slot=slot, ratio=ratio,
                        has_ub=ub is not None, has_ib=ib is not None)
    r.y_s, r.y_p = np.zeros((n_users, S)), np.zeros(nnz)                 # scores
    r.D_s, r.D_p = np.zeros((n_users, S)), np.zeros(nnz)                 # squared distances (Euclidean)
    r.wub_s, r.wub_p = np.zeros((n_users, S)), np.zeros(nnz)             # scores before the item bias
    r.loss, r.c, r.hs, r.cnt = (np.zeros(int(pos.sum())) for _ in range(4))
    r.g_s, r.g_p, r.val_s, r.val_p = np.zeros((n_users, S)), np.zeros(nnz), np.zeros((n_users, S)), np.zeros(nnz)
    r.dU, r.aU, r.dV, r.aV = np.zeros((n_users, d)), np.zeros((n_users, d)), np.zeros((n_items, d)), np.zeros((n_items, d))
    r.d_ub, r.a_ub, r.d_ib, r.a_ib = np.zeros(n_users), np.zeros(n_users), np.zeros(n_items), np.zeros(n_items)
    r.G, r.aG, r.mG = np.zeros((n_users, n_items)), np.zeros((n_users, n_items)), np.zeros((n_users, n_items))
    r.rowsum, r.a_rowsum = np.zeros(n_users), np.zeros(n_users)
    r.n_item = np.zeros(n_items)                                         # pairs per item
    r.act, r.zero_hinges, r.inactive_users, r.n_hinges, r.n_active = {}, np.zeros(n_users, np.int64), [], 0, 0
    for u in range(n_users):
        idx = np.arange(indptr[u], indptr[u + 1])
        items = np.concatenate([samples[u], x_item[idx]])
        rows = V[items]
        if mode == MODE_DOT:
            raw, D = (U[u] * rows).sum(1), np.zeros(items.size)
        else:
            D = ((U[u] - rows) ** 2).sum(1)
            raw = -np.sqrt(np.maximum(D, EPS))
        wub = raw + f64(ub)[u] if ub is not None else raw
        y = wub + f64(ib)[items] if ib is not None else wub
        r.y_s[u], r.y_p[idx], r.D_s[u], r.D_p[idx], r.wub_s[u], r.wub_p[idx] = y[:S], y[S:], D[:S], D[S:], wub[:S], wub[S:]
        np.add.at(r.n_item, items, 1.0)
        q = np.flatnonzero(pos[idx])
        if not q.size:
            continue
        H = 1.0 - y[S + q][:, None] + y[:S][None, :]
        act = H >= 0.0
        w = f64(weight)[idx[q]] if weight is not None else np.ones(q.size)
        hs = np.maximum(H, 0.0).sum(1)
        smr = ratio * hs * w
        c = ratio * w / (1.0 + smr)
        sl = slot[idx[q]]
        r.loss[sl], r.c[sl], r.hs[sl], r.cnt[sl] = np.log(smr + 1.0), c, hs, act.sum(1)
        r.act[u] = act
        r.zero_hinges[u] = int((H == 0.0).sum())
        r.n_hinges += H.size
        r.n_active += int(act.sum())
        if not act.any():
            r.inactive_users.append(u)
        g = np.zeros(items.size)
        g[:S] = (c[:, None] * act).sum(0)
        g[S + q] = -c * act.sum(1)
        val = g if mode == MODE_DOT else np.where(D >= EPS, -g / np.sqrt(np.maximum(D, 1e-300)), 0.0)
        r.g_s[u], r.g_p[idx], r.val_s[u], r.val_p[idx] = g[:S], g[S:], val[:S], val[S:]
        tu = rows if mode == MODE_DOT else U[u] - rows
        tv = np.broadcast_to(U[u], rows.shape) if mode == MODE_DOT else rows - U[u]
        r.dU[u], r.aU[u] = val @ tu, np.abs(val) @ np.abs(tu)
        np.add.at(r.dV, items, val[:, None] * tv)
        np.add.at(r.aV, items, np.abs(val[:, None] * tv))
        r.d_ub[u], r.a_ub[u] = g.sum(), np.abs(g).sum()
        np.add.at(r.d_ib, items, g)
        np.add.at(r.a_ib, items, np.abs(g))
        np.add.at(r.G[u], items, val)
        np.add.at(r.aG[u], items, np.abs(val))
        np.add.at(r.mG[u], items, 1.0)
        r.rowsum[u], r.a_rowsum[u] = val.sum(), np.abs(val).sum()
    r.pred_serial = r.y_p
    return r


def step_bars(ref, U, V, indptr, x_item, samples):
    """the bars of the module docstring for every output of ref_step, as a namespace with the outputs' names.  Asserts the Euclidean
    condition: no hinge of the reference lies within the sum of the bars of its two scores."""
    U, V = f64(U), f64(V)
    indptr, x_item, samples = np.asarray(indptr, np.int64), np.asarray(x_item, np.int64), np.asarray(samples, np.int64)
    euclid = ref.mode == MODE_EUCLID
    S, n_users = ref.S, ref.n_users
    b = SimpleNamespace()

    def sbar(D, wub, y):
        if not euclid:
            return np.zeros_like(y)
        out = 4.0 * U32 * np.maximum(np.sqrt(D), 1e-8)
        if ref.has_ub:
            out = out + U32 * np.abs(wub)
        if ref.has_ib:
            out = out + U32 * np.abs(y)
        return out

    b.y_s, b.y_p = sbar(ref.D_s, ref.wub_s, ref.y_s), sbar(ref.D_p, ref.wub_p, ref.y_p)
    b.pred_serial = b.y_p
    hb = np.zeros_like(ref.hs)
    b.g_s, b.g_p = np.zeros_like(ref.g_s), np.zeros_like(ref.g_p)
    b.min_abs_hinge = np.inf
    for u, act in ref.act.items():
        idx = np.arange(indptr[u], indptr[u + 1])
        q = np.flatnonzero(ref.pos[idx])
        sl = ref.slot[idx[q]]
        c = ref.c[sl]
        if euclid:
            H = 1.0 - ref.y_p[idx[q]][:, None] + ref.y_s[u][None, :]
            pair = b.y_p[idx[q]][:, None] + b.y_s[u][None, :]
            assert (np.abs(H) > pair).all(), "user %d: a hinge within the bars of its scores (|H| %.3e): choose another seed" \
                % (u, np.abs(H).min())
            b.min_abs_hinge = min(b.min_abs_hinge, float(np.abs(H).min()))
            per = pair + U32 * (np.abs(1.0 - ref.y_p[idx[q]])[:, None] + np.abs(H))
            hb[sl] = (per * act).sum(1) + S * U32 * ref.hs[sl]
        b.g_p[idx[q]] = 10.0 * U32 * np.abs(ref.g_p[idx[q]]) + ref.cnt[sl] * c * c * hb[sl]
        b.g_s[u] = (act.sum(0) + 9.0) * U32 * ref.g_s[u] + ((c * c * hb[sl])[:, None] * act).sum(0)
    b.loss = U32 * (4.0 + 4.0 * np.abs(ref.loss)) + ref.c * hb
    if euclid:
        inv = lambda D: np.where(D >= EPS, 1.0 / np.sqrt(np.maximum(D, 1e-300)), 0.0)
        b.val_s = b.g_s * inv(ref.D_s) + 6.0 * U32 * np.abs(ref.val_s)
        b.val_p = b.g_p * inv(ref.D_p) + 6.0 * U32 * np.abs(ref.val_p)
    else:
        b.val_s, b.val_p = b.g_s, b.g_p
    n_rows = S + np.diff(indptr)
    inh_U, inh_V = np.zeros_like(ref.dU), np.zeros_like(ref.dV)
    inh_ub, inh_ib, inh_rs = np.zeros(n_users), np.zeros(ref.n_items), np.zeros(n_users)
    inh_G = np.zeros_like(ref.G)
    for u in ref.act:
        idx = np.arange(indptr[u], indptr[u + 1])
        items = np.concatenate([samples[u], x_item[idx]])
        vb = np.concatenate([b.val_s[u], b.val_p[idx]])
        gb = np.concatenate([b.g_s[u], b.g_p[idx]])
        t = np.abs(V[items] if not euclid else U[u] - V[items])
        tv = np.abs(np.broadcast_to(U[u], t.shape) if not euclid else t)
        inh_U[u] = vb @ t
        np.add.at(inh_V, items, vb[:, None] * tv)
        inh_ub[u], inh_rs[u] = gb.sum(), vb.sum()
        np.add.at(inh_ib, items, gb)
        np.add.at(inh_G[u], items, vb)
    b.dU = (n_rows[:, None] + 1.0) * U32 * ref.aU + inh_U
    b.d_ub = (n_rows + 9.0) * U32 * ref.a_ub + inh_ub
    b.rowsum = (n_rows + 9.0) * U32 * ref.a_rowsum + inh_rs
    b.G = ref.mG * U32 * ref.aG + inh_G
    b.dV = (ref.n_item[:, None] + 1.0 + ref.mG.max()) * U32 * ref.aV + inh_V
    b.d_ib = (ref.n_item + 1.0) * U32 * ref.a_ib + inh_ib
    b.inh_U, b.inh_V = inh_U, inh_V
    return b


def split_bf16_bars(ref, U, V, indptr, x_item, samples):
    """(bar d user_in, bar d item_in) of the dense-G route on split-bf16 operands: 1e-4 * sum |terms| of the products the GEMMs form --
    Euclidean: G . (V - c), rowsum(G) (U - c), G^T . (U - c), colsum(G) (V - c) with c the mean item row (ops_base.py:923-941)"""
    U, V = f64(U), f64(V)
    if ref.mode == MODE_DOT:
        return 1e-4 * ref.aU, 1e-4 * ref.aV
    a_u, a_v = centred_abs(ref, U, V, indptr, x_item, samples)
    return 1e-4 * a_u, 1e-4 * a_v


def centred_abs(ref, U, V, indptr, x_item, samples, val_bars=None):
    """per entry of d user_in / d item_in the sum of |val| (|U_uc - c_c| + |V_jc - c_c|) over its pairs, c = the mean item row; with
    val_bars = (bar val_s, bar val_p) the same sums over the values' bars instead"""
    U, V = f64(U), f64(V)
    indptr, x_item, samples = np.asarray(indptr, np.int64), np.asarray(x_item, np.int64), np.asarray(samples, np.int64)
    c = V.mean(0)
    a_u, a_v = np.zeros_like(ref.dU), np.zeros_like(ref.dV)
    for u in ref.act:
        idx = np.arange(indptr[u], indptr[u + 1])
        items = np.concatenate([samples[u], x_item[idx]])
        if val_bars is None:
            av = np.abs(np.concatenate([ref.val_s[u], ref.val_p[idx]]))
        else:
            av = np.concatenate([val_bars[0][u], val_bars[1][idx]])
        both = np.abs(U[u] - c)[None, :] + np.abs(V[items] - c)
        a_u[u] = av @ both
        np.add.at(a_v, items, av[:, None] * both)
    return a_u, a_v


def dense_fp32_euclid_bars(ref, bars, U, V, indptr, x_item, samples):
    """(bar d user_in, bar d item_in) of the dense-G route of distances on fp32 GEMMs: the module docstring's centred bar"""
    args = (ref, U, V, indptr, x_item, samples)
    a_u, a_v = centred_abs(*args)
    i_u, i_v = centred_abs(*args, val_bars=(bars.val_s, bars.val_p))
    rows = (ref.S + np.diff(np.asarray(indptr, np.int64)))[:, None]
    m_max = ref.mG.max()
    return (rows + 4.0 + m_max) * U32 * a_u + i_u, (ref.n_item[:, None] + 4.0 + m_max) * U32 * a_v + i_v


def ref_coop_step(Wu, Wi, bu, bi, X, indptr, x_item, values, weight, samples, n_items, l2):
    """ref_step behind the item tower of csrc/step_coop.hip (identity user features, X: scipy CSR [n_items, n_features]):
    V = X . W_i, b_i = X . beta_i, d W_i = X^T . dV, d beta_i = X^T . d b_i, and gg = g + l2 * w on all four variables
    (tensorrec.py:313, :487 of the reference project regularise the bias variables too).  Adam itself is replayed in float32."""
    X = sp.csr_matrix(X).astype(np.float64)
    Wu, Wi = f64(Wu), f64(Wi)
    V = X @ Wi
    ib = X @ f64(bi) if bi is not None else None
    r = ref_step(Wu, V, f64(bu) if bu is not None else None, ib, indptr, x_item, values, weight, samples, n_items, MODE_DOT)
    r.V, r.ib = V, ib
    aX = abs(X)
    r.dWi, r.aWi = X.T @ r.dV, aX.T @ r.aV
    r.n_feat = np.asarray((X != 0).sum(0)).reshape(-1).astype(np.float64)
    r.gg = dict(Wu=r.dU + l2 * Wu, Wi=r.dWi + l2 * Wi)
    r.l2w = dict(Wu=np.abs(l2 * Wu), Wi=np.abs(l2 * Wi))
    if bi is not None:
        r.dbi, r.abi = X.T @ r.d_ib, aX.T @ r.a_ib
        r.gg.update(bu=r.d_ub + l2 * f64(bu), bi=r.dbi + l2 * f64(bi))
        r.l2w.update(bu=np.abs(l2 * f64(bu)), bi=np.abs(l2 * f64(bi)))
    r.X = X
    return r


def coop_bars(ref, Wu, indptr, x_item, samples):
    """step_bars plus the tower's: d W_i, d beta_i, and gg of the four variables"""
    b = step_bars(ref, Wu, ref.V, indptr, x_item, samples)
    aX = abs(ref.X)
    b.dWi = ref.n_feat[:, None] * U32 * ref.aWi + aX.T @ b.dV
    b.gg = dict(Wu=b.dU + U32 * (ref.l2w["Wu"] + np.abs(ref.gg["Wu"])), Wi=b.dWi + U32 * (ref.l2w["Wi"] + np.abs(ref.gg["Wi"])))
    if ref.has_ib:
        b.dbi = ref.n_feat * U32 * ref.abi + aX.T @ b.d_ib
        b.gg.update(bu=b.d_ub + U32 * (ref.l2w["bu"] + np.abs(ref.gg["bu"])), bi=b.dbi + U32 * (ref.l2w["bi"] + np.abs(ref.gg["bi"])))
    return b


def osum(terms, order):
    """float32 sum over axis 0: 'seq' one accumulator; an integer P: P interleaved partials (term k goes to partial k % P), added in turn"""
    terms = np.asarray(terms, np.float32)
    if order == "seq":
        acc = np.zeros(terms.shape[1:], np.float32)
        for t in terms:
            acc = acc + t
        return acc
    parts = [osum(terms[k::order], "seq") for k in range(order)]
    return osum(np.stack(parts), "seq")


# ------------------------------------------------------------------------------------------------ which kernel a call takes
ALL_FUSED_INSTANTIATIONS = {(1, 16, 0), (1, 16, 4), (1, 16, 8), (1, 16, 12), (1, 32, 0), (1, 32, 16), (2, 16, 0), (2, 16, 8)}
ALL_TILED_INSTANTIATIONS = {(it, rb, mode, lpr) for (it, rb, lpr) in ((1, 12, 16), (1, 12, 32), (2, 8, 32), (4, 4, 32)) for mode in (0, 1)}


def fused_rows_capacity(d):
    return 256 if d <= 128 else 128                          # wmrb_fused.hip:348


def fused_instantiation(S, max_pos, d):
    """<ITERS, RMAX, SURE> of wmrb_user_fused_kernel (wmrb_fused.hip:397-410), None where trec_wmrb_fused_lds_bytes (:357-359) is -1"""
    if S < 1 or S > 256 or d < 4 or d % 4 or d > 256 or max_pos < 0 or S + max_pos > fused_rows_capacity(d):
        return None
    sure = S // 8
    if d <= 128 and S + max_pos <= 128:
        return (1, 16, 12 if sure >= 12 else 8 if sure >= 8 else 4 if sure >= 4 else 0)
    if d <= 128:
        return (1, 32, 16 if sure >= 16 else 0)
    return (2, 16, 8 if sure >= 8 else 0)


def tiled_instantiation(d, mode):
    """<ITERS, RB, MODE, LPR> of wmrb_user_tiled_kernel (wmrb_tiled.hip:123-133)"""
    return ((1, 12, mode, 16) if d <= 64 else (1, 12, mode, 32) if d <= 128 else (2, 8, mode, 32) if d <= 256 else (4, 4, mode, 32))


def tiled_tile_rows(d):
    it, rb, _, lpr = tiled_instantiation(d, 0)
    return 256 // lpr * rb                                   # wmrb_tiled_body.hpp:94: a pass takes NSG * RB rows


def tiled_lds_bytes(S, max_pos, d):
    """trec_wmrb_tiled_lds_bytes (wmrb_tiled.hip:81-86 on wmrb_tiled_body.hpp:40-46)"""
    if S < 1 or d < 4 or d % 4 or d > 512 or max_pos < 0:
        return -1
    mr4, mp4 = (S + max_pos + 3) // 4 * 4, (max_pos + 3) // 4 * 4
    n = (2 * mr4 + 2 * mp4 + (16 if d <= 64 else 8) * d + 8) * 4
    return n if n <= 128 * 1024 else -1


COOP_IB, COOP_P3_LDS = 16, 32 * 1024                         # step_coop.hip:37-38


def coop_seg_len(n_users, d):
    """step_coop.hip:42-49"""
    s = min((n_users + 7) // 8, COOP_P3_LDS // (4 * (COOP_IB + d)), 128)
    return max(s, 16)


def coop_lds_bytes(S, max_pos, d, n_users):
    """step_coop.hip:279-286"""
    p2 = (tiled_lds_bytes(S, max_pos, d) // 4 + S + 4) * 4 if tiled_lds_bytes(S, max_pos, d) >= 0 else 1 << 30
    return max(p2, coop_seg_len(n_users, d) * (COOP_IB + d) * 4, 16 * (d + 4) * 4)


def coop_layout(n_users, n_items, d):
    """float offsets of the workspace arrays (step_coop.hip:298-312)"""
    ni4, nu4 = (n_items + 3) // 4 * 4, (n_users + 3) // 4 * 4
    l = SimpleNamespace(V=0, ldg=ni4)
    l.ib = l.V + n_items * d
    l.G = l.ib + ni4
    l.dU = l.G + n_users * ni4
    l.dub = l.dU + n_users * d
    l.dV = l.dub + nu4
    l.dib = l.dV + n_items * d
    l.clk = l.dib + ni4
    l.total = l.clk + 16
    return l


def coop_workspace_floats(n_users, n_items, d, S, max_pos):
    """trec_fit_step_coop_workspace_floats (step_coop.hip:317-326)"""
    if n_users < 1 or n_items < 1 or d < 4 or d % 4 or d > 128 or S < 1 or S > n_items or max_pos < 0:
        return -1
    if coop_lds_bytes(S, max_pos, d, n_users) > 64 * 1024 or n_users * ((n_items + 3) // 4 * 4) > 1 << 26:
        return -1
    return coop_layout(n_users, n_items, d).total


# ------------------------------------------------------------------------------------------------ inputs
def dyadic_rows(n, d, rng, nnz=16):
    """multiples of 1/8 in [-1, 1], thinned to about `nnz` non-zero columns"""
    a = rng.integers(-8, 9, size=(n, d)) / GRID8
    if d > nnz:
        keep = rng.random((n, d)) < float(nnz) / d
        a = a * keep
    return a.astype(np.float32)


def spread_columns(U, V, mode, rng):
    """the thinned rows alone give scores that differ by less than the margin 1 (nearly every hinge active, above all for distances):
    the first min(4, d / 2) columns hold one value t_i per item (a multiple of 1/8 in [-2, 2]) against a constant of the users (1 for
    dot scores, 2 for distances), which spreads an item's scores over all users alike: 20 % - 80 % of the hinges come out active"""
    ns = min(4, U.shape[1] // 2)
    V[:, :ns] = (rng.integers(-16, 17, V.shape[0]) / GRID8).astype(np.float32)[:, None]
    U[:, :ns] = 1.0 if mode == MODE_DOT else 2.0
    if mode == MODE_EUCLID:
        # 64 D = sum of the squared differences in units of 1/8; a square is 0 or 1 mod 4.  Users hold even entries, items even ones but
        # for exactly two odd ones: 64 D = 2 mod 4 is no perfect square, every distance is irrational, and 1 + sqrt(a) - sqrt(b) + (a
        # rational bias difference) is 0 only for a = b with a difference of -1 -- no hinge of a distance case is exactly 0 by accident
        U[:] = np.floor(U * 4.0) / 4.0
        V[:] = np.floor(V * 4.0) / 4.0
        for i in range(V.shape[0]):
            V[i, ns + rng.choice(V.shape[1] - ns, size=2, replace=False)] += 1.0 / GRID8


def inputs_exact(case):
    """the premise of the bars: U, V, biases multiples of 1/8, |.| <= 2, so that every partial sum of a score is a multiple of 2^-6
    below 2^10 (d <= 512: 512 * 4 = 2^11 at the very most, 17 bits): exact in float32 in any order"""
    ok = True
    for a in (case.U, case.V, case.ub, case.ib):
        t = f64(a) * GRID8
        ok = ok and bool((t == np.round(t)).all() and np.abs(f64(a)).max() <= 2.0)
    return ok and case.U.shape[1] <= 512


U_NONE, U_NONPOS, U_ONE, U_LONG, U_INACTIVE, U_CLAMP = 0, 1, 2, 3, 4, 5       # the user mix of pair_reference.wmrb_case
N_FIXED_USERS = 6


def step_case(S, longest, d, mode, n_items=300, rows=(7, 5, 3, 9, 4, 6), seed=0):
    """6 + len(rows) users.  User 0 has no interaction, user 1 non-positive ones only, user 2 one positive, user 3 the longest row
    (`longest` interactions), user 4 hinges that are all inactive, user 5 (Euclidean: clamped) one interaction and one sampled item
    that carry its own row; the others `rows` interactions each (cut to `longest`).  Values are multiples of 1/4 with negatives and
    explicit zeros mixed into the longer rows.  Dot: every user with positives but user 4 holds a hinge of exactly 0 (a sampled item
    whose row is its first positive's with one column, where the user holds 1, lowered by 1).  Where S >= 2 user 3 samples one item
    twice; where S >= 3 it also samples one of its positives (S = 1: user 5's only sample is its clamped positive)."""
    rng = np.random.default_rng(100003 * S + 1009 * longest + 17 * d + 5 * mode + seed)
    lens = [0, min(2, longest), 1, longest, min(3, longest), min(4, longest)] + [min(int(x), longest) for x in rows]
    nu = len(lens)
    n_special = 8 + nu                                            # near [4] | far [4] | one zero-hinge item per user
    n_reg = n_items - n_special
    assert n_reg >= longest + 2 and n_reg >= 8, "n_items too small for the longest row"
    near, far, zh = n_reg + np.arange(4), n_reg + 4 + np.arange(4), n_reg + 8 + np.arange(nu)
    U, V = dyadic_rows(nu, d, rng), dyadic_rows(n_items, d, rng)
    spread_columns(U, V, mode, rng)
    ub = (rng.integers(-8, 9, nu) / GRID8).astype(np.float32)
    ib = (rng.integers(-8, 9, n_items) / GRID8).astype(np.float32)
    if mode == MODE_EUCLID:
        ib = (rng.integers(-3, 4, n_items) / GRID8).astype(np.float32)       # |b_i - b_j| < 1: equal distances never give a hinge of 0
    r_idx, c_idx, vals = [], [], []
    for u, n in enumerate(lens):
        cols = np.sort(rng.choice(n_reg, size=n, replace=False))
        if u == U_INACTIVE:
            cols = near[:n]
        if u == N_FIXED_USERS and n and c_idx[lens[U_NONPOS]] not in cols:
            cols = np.sort(np.concatenate([cols[1:], [c_idx[lens[U_NONPOS]]]]))      # shares user 2's item: a balanced weight below 1
        v = rng.integers(1, 13, size=n) / 4.0
        if u == U_NONPOS:
            v[:] = [-1.0, 0.0][:n]
        elif n >= 5:
            v[1], v[n - 2] = -1.0, 0.0                            # non-positive interactions inside the longer rows
        r_idx += [u] * n
        c_idx += list(cols)
        vals += list(v)
    m = sp.csr_matrix((np.array(vals, np.float32), (np.array(r_idx), np.array(c_idx))), shape=(nu, n_items))
    assert m.nnz == len(vals)                                     # explicit zeros stay stored
    indptr, x_item, values = m.indptr.astype(np.int64), m.indices.astype(np.int32), m.data.astype(np.float32)
    samples = rng.integers(0, n_reg, size=(nu, S)).astype(np.int32)
    # user 4: U = +-1 on (up to) 16 columns; near rows = 2 U (dot) / U + a small step (Euclidean), far rows = -U; its samples are far
    k = min(d, 16)
    U[U_INACTIVE] = 0
    U[U_INACTIVE, :k] = np.where(np.arange(k) % 2 == 0, 1.0, -1.0)
    for j in range(4):
        V[near[j]] = 2.0 * U[U_INACTIVE] if mode == MODE_DOT else U[U_INACTIVE]
        if mode == MODE_EUCLID:
            V[near[j], j % k] += (1 + j) / GRID8
        V[far[j]] = -U[U_INACTIVE]
    ib[near], ib[far] = 1.0, -1.0
    samples[U_INACTIVE] = far[np.arange(S) % 4]
    # user 5: an interaction and a sampled item with the user's own row
    b5 = indptr[U_CLAMP]
    clamp_pos, clamp_samp = int(x_item[b5]), int(x_item[b5]) if S == 1 else int((x_item[b5] + 1) % n_reg)
    while clamp_samp != clamp_pos and clamp_samp in set(x_item[b5:indptr[U_CLAMP + 1]]):
        clamp_samp = (clamp_samp + 1) % n_reg
    V[clamp_pos], V[clamp_samp] = U[U_CLAMP], U[U_CLAMP]
    samples[U_CLAMP, S - 1] = clamp_samp
    values[b5] = 1.5
    # duplicates and a sample that is a positive of its user
    if S >= 2:
        samples[U_LONG, 1] = samples[U_LONG, 0]
    if S >= 3:
        samples[U_LONG, 2] = x_item[indptr[U_LONG]]
        values[indptr[U_LONG]] = 2.0
    # hinges of exactly 0 (dot): sample zh[u] against the user's first positive
    if mode == MODE_DOT:
        for u in range(nu):
            if u in (U_INACTIVE, U_NONE, U_NONPOS) or (u == U_CLAMP and S == 1):
                continue
            idx = np.arange(indptr[u], indptr[u + 1])
            idx = idx[values[idx] > 0]
            if not idx.size:
                continue
            qi = int(x_item[idx[-1]])
            col = d - 1 - (u % 2)
            U[u, col] = 1.0
            V[zh[u]] = V[qi]
            V[zh[u], col] = V[qi, col] - 1.0
            ib[zh[u]] = ib[qi]
            samples[u, (5 * u) % S if u != U_LONG else S - 1] = zh[u]
        # (U[u, col] is written before V[zh[u]] is taken from V[qi], and every user owns its item zh[u]: each planted hinge stands;
        # the host test asserts it through zero_hinges)
    m = sp.csr_matrix((values, x_item, indptr), shape=(nu, n_items))
    return SimpleNamespace(U=U, V=V, ub=ub, ib=ib, matrix=m, indptr=indptr, x_item=x_item, values=values, samples=samples, S=S, d=d,
                           mode=mode, n_users=nu, n_items=n_items, longest=longest, max_pos=int(np.diff(indptr).max()),
                           clamp=(clamp_pos, clamp_samp))


def case_weights(case):
    """float32 BalancedWMRB weights as sparse.Interactions.balanced_weight computes them (value / item sum, one rounding)"""
    m = case.matrix
    vals, pos = m.data.astype(np.float32), m.data > 0
    per_item = np.zeros(m.shape[1], np.float32)
    np.add.at(per_item, m.indices[pos], vals[pos])
    w = np.zeros(m.nnz, np.float32)
    w[pos] = vals[pos] / per_item[m.indices[pos]]
    return w


def case_ref(case, biased, balanced):
    w = case_weights(case) if balanced else None
    ref = ref_step(case.U, case.V, case.ub if biased else None, case.ib if biased else None, case.indptr, case.x_item, case.values, w,
                   case.samples, case.n_items, case.mode)
    return ref, step_bars(ref, case.U, case.V, case.indptr, case.x_item, case.samples)


def case_properties(case, ref):
    """what every case is meant to hold, as a dict the host test asserts"""
    lens = np.diff(case.indptr)
    s = case.samples
    dup = any(np.unique(s[u]).size < s.shape[1] for u in range(case.n_users))
    also_pos = any(np.intersect1d(s[u], case.x_item[case.indptr[u]:case.indptr[u + 1]][case.values[case.indptr[u]:case.indptr[u + 1]] > 0]).size
                   for u in range(case.n_users))
    cl_p = (case.V[case.x_item[case.indptr[U_CLAMP]]] == case.U[U_CLAMP]).all()
    cl_s = (case.V[s[U_CLAMP, -1]] == case.U[U_CLAMP]).all()
    wts = case_weights(case)
    return dict(active_share=ref.n_active / float(max(ref.n_hinges, 1)), n_hinges=ref.n_hinges, zero_hinges=ref.zero_hinges.copy(),
                inactive_users=list(ref.inactive_users), duplicate_sample=bool(dup), sample_is_positive=bool(also_pos),
                clamped=bool(cl_p and cl_s), no_interaction=bool(lens[U_NONE] == 0),
                nonpositive_only=bool(lens[U_NONPOS] > 0 and not ref.pos[case.indptr[U_NONPOS]:case.indptr[U_NONPOS + 1]].any()),
                one_positive=bool(lens[U_ONE] == 1), longest=int(lens.max()), weights_not_one=bool((wts[case.values > 0] != 1).any()),
                values_quarter=bool((f64(case.values) * 4 == np.round(f64(case.values) * 4)).all()))


# (S, longest row, d) of the fused cases: the smallest that reach each edge of wmrb_fused.hip:397-410; ~300 items, 12 users
FUSED_CASES = [(1, 3, 4), (31, 97, 128), (32, 20, 20), (63, 20, 20), (64, 33, 64), (95, 33, 64), (96, 32, 100), (127, 1, 128),
               (100, 156, 128), (97, 32, 64), (128, 1, 4), (255, 1, 128), (63, 65, 132), (127, 1, 256), (64, 31, 200)]


def fused_case(S, longest, d):
    return step_case(S, longest, d, MODE_DOT, n_items=300 if longest < 150 else 360)


# (S, d, rows of the users past the fixed six, n_items): tiles of 192 / 96 / 64 / 32 rows (tiled_tile_rows); R = S + rows at tile - 1,
# tile, tile + 1, 2 tile + 1; rows of 31, 32, 33, 65 interactions; S = 1, 1023, 1024, 1025
TILED_CASES = [
    (1, 4, (190, 191, 192, 384, 31), 460),
    (127, 64, (64, 65, 66, 258, 31, 32, 33), 340),
    (30, 68, (65, 66, 67, 163, 31, 32, 33), 300),
    (1023, 128, (31, 32, 33, 65), 300),
    (20, 132, (43, 44, 45, 109, 31, 32, 33, 65), 300),
    (1024, 256, (5, 20), 300),
    (20, 260, (11, 12, 13, 45, 31, 32, 33, 65), 300),
    (1025, 512, (3, 12), 300),
]
TILED_BIG = (3000, 512, (), 4000)                               # dot only: LDS above 64 KB, longest row 1,700


def tiled_case(S, d, rows, n_items, mode):
    longest = 1700 if (S, d, rows, n_items) == TILED_BIG else max(rows)
    return step_case(S, longest, d, mode, n_items=n_items, rows=rows)


# ------------------------------------------------------------------------------------------------ cooperative step
# (n_users, n_items, d, S, features): step_coop.hip's edges -- fewer users than a 16-user segment, fewer items than a 16-item tile,
# S = n_items, d = 68 (17 float4 columns: 32 lanes per row), segments of 128 users, feature columns of 0, 1, 31, 32, 33, 64, 65 and
# >= 200 items (a phase-4 round is 64 entries at 16 groups, 32 at 8); the last case gives the 16-group kernel (d <= 64) columns of
# 65 and 99 entries, i.e. a second round
COOP_CASES = [(1, 1, 4, 1, "identity"), (9, 15, 20, 7, "columns"), (130, 33, 64, 33, "columns"), (150, 333, 68, 40, "columns"),
              (1100, 40, 16, 8, "columns"), (257, 100, 128, 25, "columns"), (64, 100, 64, 20, "columns")]
COOP_COLUMN_SIZES = [0, 1, 31, 32, 33, 64, 65, 200]


def coop_features(n_items, kind):
    """identity, or [identity | indicator columns]: column f holds the first COOP_COLUMN_SIZES[f] items (cut to n_items - 1), so that an
    item row is the sum of up to nine weight rows (exact for dyadic weights: multiples of 1/8 below 2^5); the last item holds no
    feature at all, not even its own.  Returns scipy CSR [n_items, n_features]."""
    if kind == "identity":
        return sp.identity(n_items, dtype=np.float32, format="csr")
    r_idx, c_idx = list(range(n_items - 1)), list(range(n_items - 1))
    for f, n in enumerate(COOP_COLUMN_SIZES):
        n = min(n, n_items - 1)
        r_idx += list(range(n))
        c_idx += [n_items + f] * n
    return sp.csr_matrix((np.ones(len(r_idx), np.float32), (np.array(r_idx, np.int64), np.array(c_idx, np.int64))),
                         shape=(n_items, n_items + len(COOP_COLUMN_SIZES)))


def coop_case(n_users, n_items, d, S, kind, seed=0):
    """Dyadic weight tables behind coop_features.  The item rows V = X . W_i are chosen first and the identity block of W_i solved from
    them (V_i minus the rows of the item's columns), so the cases carry what step_case's do: user 0 has no interaction, user 1
    non-positive ones only, user 2 one positive, user 3 the longest row (12, or what the items allow), a duplicated sample and a sample
    that is one of its positives, user 4 hinges that are all inactive (column d - 3 holds 128 for this user alone and 1 for its
    positives, which it never samples); the others 1 - 12 interactions with non-positives mixed in.  Every other user with positives
    holds a hinge of exactly 0 with AND without biases: columns d - 1 / d - 2 hold bit 0 / bit 1 of the item number, samples 0 and 1
    of the user are its first positive q with bit 0 / bit 1 flipped (interactions stay below the last full block of four items), and
    the user's entries in the two columns solve 1 - y_q + y_s = 0 for the first sample without biases and for the second with them
    (multiples of 1/64 against integers: every score stays a multiple of 1/64).
    The identity case (1 user, 1 item, d = 4) can carry none of this: its one hinge is 1 - y + y = 1, active."""
    rng = np.random.default_rng(7919 * n_users + 31 * n_items + d + seed)
    X = coop_features(n_items, kind)
    nf = X.shape[1]
    bu = (rng.integers(-8, 9, n_users) / GRID8).astype(np.float32)
    if kind == "identity":
        Wu, Wi = dyadic_rows(n_users, d, rng), dyadic_rows(nf, d, rng)
        spread_columns(Wu, Wi, MODE_DOT, rng)
        bi = (rng.integers(-8, 9, nf) / GRID8).astype(np.float32)
        m = sp.csr_matrix((np.full(n_users, 1.5, np.float32), (np.arange(n_users), np.arange(n_users) % n_items)), shape=(n_users, n_items))
        samples = rng.integers(0, n_items, size=(n_users, S)).astype(np.int32)
    else:
        assert n_users >= 6 and d >= 16 and S >= 5 and n_items >= 13
        usable = (n_items - 1) // 4 * 4
        c0, c1, c2 = d - 1, d - 2, d - 3
        U, Vt = dyadic_rows(n_users, d, rng), dyadic_rows(n_items, d, rng)
        spread_columns(U, Vt, MODE_DOT, rng)
        ar = np.arange(n_items)
        U[:, [c0, c1, c2]] = 0.0
        Vt[:, c0], Vt[:, c1], Vt[:, c2] = ar % 2, (ar // 2) % 2, 0.0
        ibt = (rng.integers(-8, 9, n_items) / GRID8).astype(np.float32)
        Vt[-1], ibt[-1] = 0.0, 0.0                                  # the item without features
        r_idx, c_idx, vals = [], [], []
        longest = min(12, usable)
        for u in range(n_users):
            n = [0, 2, 1, longest, min(3, usable)][u] if u < 5 else int(rng.integers(1, longest + 1))
            cols = np.sort(rng.choice(usable, size=n, replace=False))
            v = rng.integers(1, 13, size=n) / 4.0
            if u == U_NONPOS:
                v[:] = [-1.0, 0.0]
            elif n >= 3 and u != U_INACTIVE:
                v[1] = -1.0 if u % 2 else 0.0
            r_idx += [u] * n
            c_idx += list(cols)
            vals += list(v)
        m = sp.csr_matrix((np.array(vals, np.float32), (np.array(r_idx, np.int64), np.array(c_idx, np.int64))), shape=(n_users, n_items))
        assert m.nnz == len(vals)
        samples = rng.integers(0, n_items, size=(n_users, S)).astype(np.int32)
        own = m.indices[m.indptr[U_INACTIVE]:m.indptr[U_INACTIVE + 1]]
        U[U_INACTIVE, c2] = 128.0
        Vt[own, c2] = 1.0
        samples[U_INACTIVE] = np.setdiff1d(ar, own)[np.arange(S) % (n_items - own.size)]
        U64, V64, ib64 = f64(U), f64(Vt), f64(ibt)
        for u in range(n_users):
            idx = np.arange(m.indptr[u], m.indptr[u + 1])
            idx = idx[m.data[idx] > 0]
            if u == U_INACTIVE or not idx.size:
                continue
            q = int(m.indices[idx[0]])
            s1, s2 = q ^ 1, q ^ 2
            samples[u, 0], samples[u, 1] = s1, s2
            U64[u, c0] = (-1.0 - U64[u] @ (V64[s1] - V64[q])) / (V64[s1, c0] - V64[q, c0])
            U64[u, c1] = (-1.0 - U64[u] @ (V64[s2] - V64[q]) - (ib64[s2] - ib64[q])) / (V64[s2, c1] - V64[q, c1])      # (c1 still 0)
            if u == U_LONG:
                samples[u, 3], samples[u, 4] = samples[u, 2], int(m.indices[idx[-1]])
        Wu = U64.astype(np.float32)
        assert (f64(Wu) == U64).all() and (U64 * 64.0 == np.round(U64 * 64.0)).all()
        Wi, bi = dyadic_rows(nf, d, rng), (rng.integers(-8, 9, nf) / GRID8).astype(np.float32)
        cols_part = X[:, n_items:].astype(np.float64)
        Wi[:n_items] = (V64 - cols_part @ f64(Wi[n_items:])).astype(np.float32)
        bi[:n_items] = (ib64 - cols_part @ f64(bi[n_items:])).astype(np.float32)
    return SimpleNamespace(Wu=Wu, Wi=Wi, bu=bu, bi=bi, X=X, matrix=m, indptr=m.indptr.astype(np.int64), x_item=m.indices.astype(np.int32),
                           values=m.data.astype(np.float32), samples=samples, S=S, d=d, n_users=n_users, n_items=n_items,
                           n_features=nf, max_pos=int(np.diff(m.indptr).max()), kind=kind)


def coop_case_properties(case, ref):
    """the conditions of coop_case's docstring, as a dict the host test asserts (ref: with or without biases)"""
    s, ip, xi = case.samples, case.indptr, case.x_item
    has_pos = np.array([u in ref.act for u in range(case.n_users)])
    planted = has_pos.copy()
    planted[U_INACTIVE] = False
    positives = lambda u: xi[ip[u]:ip[u + 1]][case.values[ip[u]:ip[u + 1]] > 0]
    return dict(active_share=ref.n_active / float(ref.n_hinges), zero_hinge_everywhere=bool((ref.zero_hinges[planted] >= 1).all()),
                inactive_users=list(ref.inactive_users), no_interaction=bool(ip[1] == ip[0]),
                nonpositive_only=bool(ip[2] - ip[1] == 2 and not has_pos[U_NONPOS]), one_positive=bool(ip[3] - ip[2] == 1 and has_pos[U_ONE]),
                duplicate_sample=bool(np.unique(s[U_LONG]).size < case.S), sample_is_positive=bool(np.intersect1d(s[U_LONG], positives(U_LONG)).size),
                values_quarter=bool((f64(case.values) * 4 == np.round(f64(case.values) * 4)).all()),
                weights_not_one=bool((case_weights(case)[case.values > 0] != 1).any()))
