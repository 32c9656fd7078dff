"""Float64 reference, error bars, inputs, float32 restatements and the dispatch mirrors for the tiled one-pass sampled-softmax step
(csrc/softmax_tiled.hip, trec_softmax_tiled_step, ops.softmax_tiled_step).  NumPy / SciPy only, nothing of the code under test.
tests/test_softmax_tiled_reference_host.py holds the reference to central differences and the bars to the restatements on the CPU (and
shows that seeded defects fall outside); tests/test_gpu_softmax_tiled.py holds the kernel to the reference.

The step.  Scores of the interactions and of the [U, S] samples (pair_reference.ref_pair_scores, dot or Euclidean), the loss on them
with upstream gradient 1 (sampled_loss_reference.ref_sampled_softmax, or sampled_adjust_reference.ref_sampled_softmax_adj when an
option is on), the gradients of the tables and biases through pair_reference.ref_pair_grads fed with the reference d_pred / d_samp.

Bars.  u = 2^-24.  Nothing is tuned; every bar is one of
* pred_serial        pair_reference.score_bar =: delta_p (dot: (d + 8) u sum |u_c v_c|; Euclidean: ((d + 8) / 2 + 4) u sqrt(D); one u per
                     bias add).  The kernel's chain is shorter (d / LPR fmafs per lane and four or five DPP adds).
* loss, g            the loss references' own bars (unit roundoffs per operation, 2 ulp per expf / logf, the argument error of every
                     exponential), plus what the scores' error does to them, as tests/softmax_step_reference.py derives it: with
                     delta_u the largest delta among a user's interactions and samples, every logit moves by at most t delta_u and every
                     exponential ratio by a factor within exp(+-2 t delta_u): loss_p moves by at most 2 t delta_u, g by a relative
                     expm1(2 t delta_u).  (The corrections c_s are constants and the hit mask depends on ids only.)  =: bar_g.
* val                dot: g itself.  Euclidean: c = -g / sqrt(D), 0 where D < 1e-16: bar_g / sqrt(D) + pair_reference.coef_bar
                     (((d + 8) / 2 + 6) u |c|: D's chain halved by the root, sqrtf 2 ulp, the division 1 ulp).
* dU, dV, d b_u, d b_i   pair_reference.grad_bars for the sums themselves ((m + k) u sum |terms|, k = 1 dot, (d + 8) / 2 + 8 Euclidean;
                     biases m u sum |g|), plus bar_g carried through: sum_p bar_g_p |d score_p / d entry| (dot |v_c| resp. |u_c|,
                     Euclidean |u_c - v_c| / sqrt(D); biases 1).  val_rowsum: m u sum |val| + sum bar_val.
* G[u, i]            the m values of the cell added by float atomics: m u sum |val| + sum bar_val.
* dense-G route      (ops.softmax_tiled_step with G, fp32 GEMMs: tuning dense_g_split_bf16 = 0).  Dot: dU = G . V, dV = G^T . U: the
                     same terms with the cells of G summed first: (m + k + m_cell) u sum |terms| + inherited.  Euclidean: the centred
                     form of ops_base._tiled_item_side, dU = rowsum(G) (U - c) - G . (V - c), dV = colsum(G) (V - c) - G^T . (U - c):
                     (m + 4 + m_cell) u sum |val| (|U_uc - c_c| + |V_jc - c_c|) + sum bar_val (the same factor), the bar
                     tests/step_reference.py derives for the WMRB step on this route.
The dyadic family (dot; tables and biases multiples of 1/8: every partial sum of a score is a multiple of 2^-6 far below 2^24, exact in
float32 in any order -- scores_exact asserts it) has delta = 0: pred_serial is held bit for bit and the loss phase stands alone.
An entry whose terms are all 0 (dU / d b_u of a user without positives, the value of a hit) has a bar of 0."""
import functools
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

import sampled_adjust_reference as AR
import sampled_loss_reference as LR
from pair_reference import EPS, MODE_DOT, MODE_EUCLID, U32, coef_bar, f64, grad_bars, ref_pair_grads, ref_pair_scores, score_bar

F = np.float32

# (log_q_correction, remove_hits, log q: "case" = the case's table | None = the null table, -log(n_items))
VARIANTS = {"plain": (False, False, None), "hits": (False, True, None), "logq": (True, False, "case"),
            "logq-uniform": (True, False, None), "both": (True, True, "case")}


# ------------------------------------------------------------------------------------------------ which kernel a call takes
LADDER = ((64, 1, 12, 16), (128, 1, 12, 32), (256, 2, 8, 32), (512, 4, 4, 32))       # (d up to, ITERS, RB, LPR)
ALL_INSTANTIATIONS = {(it, rb, mode, lpr, adj) for (_, it, rb, lpr) in LADDER for mode in (0, 1) for adj in (False, True)}


def instantiation(d, mode, variant):
    """<ITERS, RB, MODE, LPR, ADJ> of softmax_user_tiled_kernel that trec_softmax_tiled_step launches"""
    use_q, no_hits, _ = VARIANTS[variant]
    for top, it, rb, lpr in LADDER:
        if d <= top:
            return (it, rb, mode, lpr, bool(use_q or no_hits))
    return None


def lds_bytes(S, max_pos, d):
    """trec_softmax_tiled_lds_bytes: y [mr4] | cf [mr4] | w [ms4] | partial dU [subgroups][d] | red [24], -1 outside the coverage"""
    if S < 1 or d < 4 or d % 4 or d > 512 or max_pos < 0:
        return -1
    mr4, ms4 = (S + max_pos + 3) // 4 * 4, (S + 3) // 4 * 4
    n = (2 * mr4 + ms4 + (16 if d <= 64 else 8) * d + 24) * 4
    return n if n <= 128 * 1024 else -1


UNCOVERED = [(7, 5, 6), (7, 5, 516), (0, 5, 8), (7, 5, 2), (20000, 5, 8), (100, 16000, 128)]       # (S, longest row, d)


# ------------------------------------------------------------------------------------------------ inputs
U_NONE, U_NONPOS, U_ONE, U_ABOVE, U_BELOW, U_ALLEQ, U_SPAN, U_ALLHITS, U_HITMAX, U_DUP, U_CLAMP = range(11)
N_FIXED = 11
FIXED_ROWS = [0, 2, 1, 3, 3, 3, 2, 6, 5, 4, 3]
FAR = 100.0
SPAN = 30.0
HITMAX_LIFT = 64.0


def tiled_case(S, d, mode, rows=(), exact=False, seed=0):
    """11 + len(rows) users.  0: no interaction; 1: interactions of value <= 0 only; 2: one positive; 3 / 4: a positive FAR above / below
    every sample (its last interaction sits on a reserved item); 5: all samples the same item (equal scores); 6: samples on reserved
    items with zero rows and biases spanning +-SPAN in logit at t = 1; 7: every sample one of its positives (all hits); 8: columns of
    its own -- slot 0 samples one of its positives whose item bias is HITMAX_LIFT above the others (a hit that is the maximum), slot 1
    (S >= 2) the item of its interaction of value <= 0 (no hit); 9: a duplicated sample id (S >= 2); 10: its last interaction and its
    last sample sit on two reserved items that carry the user's own row (Euclidean: D = 0 as a positive and as a sample); then one user
    per entry of `rows` with that many interactions (value <= 0 mixed in from five on).  The planted scores go through item biases, so
    they are what they mean in the runs WITH biases.  exact (dot): tables and biases multiples of 1/8.  log_q: a table spanning
    -2 ... -14."""
    rng = np.random.default_rng(9001 * S + 13 * d + 5 * mode + 101 * len(rows) + sum(rows) + (3 if exact else 0) + seed)
    lens = FIXED_ROWS + [int(r) for r in rows]
    nu, longest = len(lens), max(lens)
    n_reg = max(160, longest + 45)
    own0 = n_reg - 5                                              # five columns only U_HITMAX interacts with and samples
    span0 = n_reg
    far_above, far_below, clamp_pos, clamp_samp = n_reg + S, n_reg + S + 1, n_reg + S + 2, n_reg + S + 3
    n_items = n_reg + S + 4
    if exact:
        assert mode == MODE_DOT
        U = (rng.integers(-8, 9, size=(nu, d)) / 8.0 * (rng.random((nu, d)) < min(1.0, 16.0 / d))).astype(F)
        V = (rng.integers(-8, 9, size=(n_items, d)) / 8.0 * (rng.random((n_items, d)) < min(1.0, 16.0 / d))).astype(F)
        ub = (rng.integers(-8, 9, nu) / 8.0).astype(F)
        ib = (rng.integers(-8, 9, n_items) / 8.0).astype(F)
    else:
        U = (rng.standard_normal((nu, d)) / np.sqrt(d)).astype(F)
        V = ((2.0 if mode == MODE_DOT else 1.0) * rng.standard_normal((n_items, d)) / (1.0 if mode == MODE_DOT else np.sqrt(d))).astype(F)
        ub = (0.5 * rng.standard_normal(nu)).astype(F)
        ib = (0.5 * rng.standard_normal(n_items)).astype(F)
    r_idx, c_idx, vals = [], [], []
    for u, n in enumerate(lens):
        cols = np.sort(rng.choice(own0, size=n, replace=False))
        if u == U_HITMAX:
            cols = own0 + np.arange(n)
        v = rng.integers(1, 13, size=n) / 4.0
        if u == U_NONPOS:
            v[:] = [-1.0, 0.0][:n]
        elif u == U_HITMAX:
            v[0] = -1.0
        elif n >= 5:
            v[1], v[n - 2] = -1.0, 0.0
        r_idx += [u] * n
        c_idx += list(cols)
        vals += list(v)
    m = sp.csr_matrix((np.array(vals, F), (np.array(r_idx), np.array(c_idx))), shape=(nu, n_items))
    assert m.nnz == len(vals) and m.has_sorted_indices            # explicit zeros stay stored
    indptr, x_item, values = m.indptr.astype(np.int64), m.indices.astype(np.int32).copy(), m.data.astype(F)
    samples = rng.integers(0, own0, size=(nu, S)).astype(np.int32)

    def row(u, positive=None):
        idx = np.arange(indptr[u], indptr[u + 1])
        if positive is not None:
            idx = idx[(values[idx] > 0) == positive]
        return idx
    if S >= 2:
        samples[U_DUP, 1] = samples[U_DUP, 0]
    samples[U_ALLEQ] = samples[U_ALLEQ, 0]
    samples[U_SPAN] = span0 + rng.permutation(S)
    V[span0:span0 + S] = 0.0
    span = np.linspace(-SPAN, SPAN, S) if S > 1 else np.array([SPAN])
    ib[span0:span0 + S] = (np.round(span * 8.0) / 8.0).astype(F)
    samples[U_ALLHITS] = x_item[rng.choice(row(U_ALLHITS, True), size=S)]
    hit_max = int(x_item[row(U_HITMAX, True)[0]])
    samples[U_HITMAX, 0] = hit_max
    ib[own0:n_reg] = 0.0
    ib[hit_max] = HITMAX_LIFT
    if S >= 2:
        samples[U_HITMAX, 1] = x_item[row(U_HITMAX, False)[0]]
    # the rows equal to a user's own: the last interaction and the last sample of U_CLAMP
    x_item[indptr[U_CLAMP + 1] - 1] = clamp_pos
    values[indptr[U_CLAMP + 1] - 1] = 1.5
    V[clamp_pos], V[clamp_samp] = U[U_CLAMP], U[U_CLAMP]
    ib[clamp_pos], ib[clamp_samp] = 0.25, -0.25
    samples[U_CLAMP, S - 1] = clamp_samp
    # the planted positives: the LAST interaction of the user is moved onto a reserved item (beyond every regular column: the row
    # stays sorted) with a zero row; its score in float64 with biases is set through the item's bias
    for u, item, up in ((U_ABOVE, far_above, True), (U_BELOW, far_below, False)):
        x_item[indptr[u + 1] - 1] = item
        values[indptr[u + 1] - 1] = 1.0
        V[item], ib[item] = 0.0, 0.0
        s = ref_pair_scores(U, V, np.full(S, u), samples[u], mode, ub, ib).scores
        base = float(ref_pair_scores(U, V, [u], [item], mode, ub, ib).scores[0])
        target = (s.max() + FAR if up else s.min() - FAR) - base
        ib[item] = F(np.ceil(target * 8.0) / 8.0 if up else np.floor(target * 8.0) / 8.0)
    log_q = rng.permutation(np.linspace(-2.0, -14.0, n_items)).astype(F)
    m = sp.csr_matrix((values, x_item, indptr), shape=(nu, n_items))
    assert m.has_sorted_indices
    return SimpleNamespace(U=U, V=V, ub=ub, ib=ib, matrix=m, indptr=indptr, x_item=x_item, values=values, samples=samples, log_q=log_q,
                           S=S, d=d, mode=mode, n_users=nu, n_items=n_items, rows=tuple(rows), max_pos=int(np.diff(indptr).max()),
                           exact=exact, hit_max=hit_max, clamp=(clamp_pos, clamp_samp),
                           planted=SimpleNamespace(above=int(indptr[U_ABOVE + 1] - 1), below=int(indptr[U_BELOW + 1] - 1)))


def scores_exact(case):
    """the premise of delta = 0: dot scores, tables and biases multiples of 1/8, every sum of |terms| of a score below 2^17"""
    if case.mode != MODE_DOT:
        return False
    for a in (case.U, case.V, case.ub, case.ib):
        t = f64(a) * 8.0
        if not (t == np.round(t)).all():
            return False
    big = np.abs(f64(case.U)).max(initial=0) * np.abs(f64(case.V)).sum(1).max() + np.abs(case.ub).max() + np.abs(case.ib).max()
    return bool(big < 2.0 ** 17)


def pair_lists(case):
    """(xu, xi) of the interactions followed by the sampled pairs"""
    S, nu = case.S, case.n_users
    xu = np.concatenate([np.repeat(np.arange(nu), np.diff(case.indptr)), np.repeat(np.arange(nu), S)])
    xi = np.concatenate([case.x_item.astype(np.int64), case.samples.reshape(-1).astype(np.int64)])
    return xu, xi


def case_properties(case):
    """what the cases are meant to hold, as a dict the host test asserts (scores with biases)"""
    xu, xi = pair_lists(case)
    sc = ref_pair_scores(case.U, case.V, xu, xi, case.mode, case.ub, case.ib)
    nnz = case.x_item.size
    yp, ys = sc.scores[:nnz], sc.scores[nnz:].reshape(case.n_users, case.S)
    D_p, D_s = sc.mag[:nnz], sc.mag[nnz:].reshape(case.n_users, case.S)
    lens = np.diff(case.indptr)
    pos = case.values > 0
    row_pos = lambda u: pos[case.indptr[u]:case.indptr[u + 1]]
    hits = AR.hit_mask(case.indptr, case.x_item, case.values, case.samples)
    p = case.planted
    kept = ~hits[U_HITMAX]
    return dict(rows=sorted(int(x) for x in lens[N_FIXED:]), no_interaction=bool(lens[U_NONE] == 0),
                nonpositive_only=bool(lens[U_NONPOS] > 0 and not row_pos(U_NONPOS).any()), one_positive=bool(lens[U_ONE] == 1 and row_pos(U_ONE).all()),
                far_above=float(yp[p.above] - ys[U_ABOVE].max()), far_below=float(ys[U_BELOW].min() - yp[p.below]),
                all_equal=bool((case.samples[U_ALLEQ] == case.samples[U_ALLEQ, 0]).all()), span=float(ys[U_SPAN].max() - ys[U_SPAN].min()),
                all_hits=bool(hits[U_ALLHITS].all()),
                hit_is_max=bool(hits[U_HITMAX, 0] and (case.S < 2 or ys[U_HITMAX, 0] > ys[U_HITMAX][kept].max() + 30.0)),
                nonpos_item_no_hit=bool(case.S < 2 or not hits[U_HITMAX, 1]),
                duplicate=bool(case.S < 2 or case.samples[U_DUP, 0] == case.samples[U_DUP, 1]),
                clamp_pos=float(D_p[case.indptr[U_CLAMP + 1] - 1]), clamp_samp=float(D_s[U_CLAMP, case.S - 1]),
                mixed_long=bool(all((~row_pos(u)).any() and row_pos(u).any() for u in range(N_FIXED, case.n_users) if lens[u] >= 5)))


# ------------------------------------------------------------------------------------------------ reference
def _loss_ref(case, yp, ys, temperature, variant, log_q_table="case"):
    use_q, no_hits, lq = VARIANTS[variant]
    if lq == "case":
        lq = case.log_q if isinstance(log_q_table, str) else log_q_table
    go = np.ones(int((case.values > 0).sum()))
    if variant == "plain":
        lr = LR.ref_sampled_softmax(case.indptr, case.values, yp, ys, go, temperature)
        lr.hits = np.zeros(ys.shape, bool)
        return lr
    lc = SimpleNamespace(indptr=case.indptr, values=case.values, cols=case.x_item, pred=yp, samp=ys, go=go, items=case.samples,
                         log_q=lq, n_items=case.n_items)
    return AR.ref_sampled_softmax_adj(lc, temperature, use_q, no_hits, log_q=lq)


def _sums(rows, n, terms):
    """[n, k] = the terms [m, k] (or [m]) summed by row index"""
    m = rows.size
    return sp.csr_matrix((np.ones(m), (rows, np.arange(m))), shape=(n, m)) @ terms


def ref_step(case, biased, temperature, variant="plain", log_q_table="case"):
    """the float64 step and its bars: a namespace with loss, pred_serial, dU, dV, d_ub, d_ib, g / val (interactions | samples, flat),
    rowsum and b_<name> for each, the hit mask, D per pair and what dense_bars needs"""
    mode = getattr(case, "mode", MODE_DOT)
    d, S, nu, ni, nnz = case.d, case.S, case.n_users, case.n_items, case.x_item.size
    ub, ib = (case.ub, case.ib) if biased else (None, None)
    xu, xi = pair_lists(case)
    sc = ref_pair_scores(case.U, case.V, xu, xi, mode, ub, ib)
    exact = getattr(case, "exact", False)
    if exact:
        assert scores_exact(case)
    delta = np.zeros(xu.size) if exact else score_bar(sc, d)
    yp, ys = sc.scores[:nnz], sc.scores[nnz:].reshape(nu, S)
    lr = _loss_ref(case, yp, ys, temperature, variant, log_q_table)
    t = 1.0 / float(temperature)
    du = np.zeros(nu)                                             # delta_u
    np.maximum.at(du, xu, delta)
    pos = case.values > 0
    f = np.expm1(2.0 * t * du)
    r = SimpleNamespace(loss=lr.loss, pred_serial=yp, hits=lr.hits, scores=sc, delta=delta, mode=mode, xu=xu, xi=xi)
    r.b_pred_serial = delta[:nnz]
    r.b_loss = lr.bar_loss + 2.0 * t * du[xu[:nnz]][pos]                  # (slots follow the CSR order of the positives)
    r.g = np.concatenate([lr.d_pred, lr.d_samp.reshape(-1)])
    r.b_g = np.concatenate([lr.bar_d_pred, lr.bar_d_samp.reshape(-1)]) + np.abs(r.g) * f[xu]
    pg = ref_pair_grads(case.U, case.V, xu, xi, r.g, mode)
    r.pg = pg
    bU, bV, bub, bib = grad_bars(pg, d)
    Uf, Vf = f64(case.U), f64(case.V)
    if mode == MODE_DOT:
        r.val, r.b_val, r.D = r.g, r.b_g, np.zeros(xu.size)
        tu, tv = np.abs(Vf[xi]), np.abs(Uf[xu])
    else:
        inv = np.where(pg.D >= EPS, 1.0 / np.sqrt(np.maximum(pg.D, 1e-300)), 0.0)
        r.val, r.D = pg.coef, pg.D
        r.b_val = r.b_g * inv + coef_bar(pg, d)
        tu = np.abs(Uf[xu] - Vf[xi]) * inv[:, None]
        tv = tu
    inh_U, inh_V = _sums(xu, nu, r.b_g[:, None] * tu), _sums(xi, ni, r.b_g[:, None] * tv)
    inh_ub, inh_ib = np.bincount(xu, weights=r.b_g, minlength=nu), np.bincount(xi, weights=r.b_g, minlength=ni)
    r.dU, r.dV, r.d_ub, r.d_ib = pg.dU, pg.dV, pg.dub, pg.dib
    r.b_dU, r.b_dV, r.b_d_ub, r.b_d_ib = bU + inh_U, bV + inh_V, bub + inh_ub, bib + inh_ib
    r.rowsum = np.bincount(xu, weights=r.val, minlength=nu)
    r.b_rowsum = pg.cnt_u * U32 * np.bincount(xu, weights=np.abs(r.val), minlength=nu) + np.bincount(xu, weights=r.b_val, minlength=nu)
    return r


def dense_G(case, ref):
    """(G, bar) [n_users, n_items]: the values added at (user, item), duplicates included; m u sum |val| + sum bar_val per cell"""
    shape = (case.n_users, case.n_items)
    cell = lambda w: np.asarray(sp.coo_matrix((w, (ref.xu, ref.xi)), shape=shape).todense())
    return cell(ref.val), cell(np.ones(ref.xu.size)) * U32 * cell(np.abs(ref.val)) + cell(ref.b_val)


def dense_bars(case, ref):
    """(bar dU, bar dV, bar d_ib) of ops.softmax_tiled_step on the dense-G route with fp32 GEMMs (the module docstring's last bar)"""
    xu, xi, nu, ni, d = ref.xu, ref.xi, case.n_users, case.n_items, case.d
    m_cell = float(np.asarray(sp.coo_matrix((np.ones(xu.size), (xu, xi)), shape=(nu, ni)).tocsr().max()))
    pg = ref.pg
    if ref.mode == MODE_DOT:
        return (ref.b_dU + m_cell * U32 * pg.aU, ref.b_dV + m_cell * U32 * pg.aV, ref.b_d_ib + m_cell * U32 * pg.aib)
    Uf, Vf = f64(case.U), f64(case.V)
    c = f64(case.V.astype(F).mean(0, dtype=F))
    both = np.abs(Uf[xu] - c) + np.abs(Vf[xi] - c)
    a_u, a_v = _sums(xu, nu, np.abs(ref.val)[:, None] * both), _sums(xi, ni, np.abs(ref.val)[:, None] * both)
    i_u, i_v = _sums(xu, nu, ref.b_val[:, None] * both), _sums(xi, ni, ref.b_val[:, None] * both)
    return ((pg.cnt_u[:, None] + 4.0 + m_cell) * U32 * a_u + i_u, (pg.cnt_i[:, None] + 4.0 + m_cell) * U32 * a_v + i_v, ref.b_d_ib)


# (S, d, rows): the GPU cases.  Every instantiation: d in {4, 36, 64, 128, 256, 512}, rows that leave the last tile ragged (tiles of
# 192 / 96 / 64 / 32 rows) and take more than one pass of 256 interactions in the loss phase
D_CASES = [(37, 4, (193, 70)), (37, 36, (157, 70)), (41, 64, (300, 33)), (37, 128, (60, 257)), (37, 256, (28, 90)), (37, 512, (1, 33))]
# S at the edges of the 256-sample stride, S = 1, S in the thousands
S_CASES = [(1, 36, (5,)), (255, 36, (5,)), (256, 36, (5,)), (257, 36, (5,)), (1023, 132, (5,)), (1025, 36, (300,))]
BIG_LDS = (9000, 64, (40,))                                       # 112 KB of dynamic LDS
LONG_ROWS = (100, 128, (255, 256, 257, 1025, 2600))               # rows of 0, non-positives only, 1, 255, 256, 257, 1,025, 2,600
ALL_CASES = D_CASES + S_CASES + [BIG_LDS, LONG_ROWS]
TEMPERATURE = 0.5
# (S, longest row, d) that the per-user fused step covers too: the two steps against each other
SHARED_WITH_FUSED = [(7, 20, 36), (100, 28, 128), (64, 64, 256)]


@functools.lru_cache(maxsize=None)
def cached_case(spec, mode, exact=False):
    S, d, rows = spec
    return tiled_case(S, d, mode, rows, exact=exact)


@functools.lru_cache(maxsize=None)
def cached_ref(spec, mode, exact, biased, temperature, variant):
    """computed once and shared by the host and the GPU tests; nobody writes into it"""
    return ref_step(cached_case(spec, mode, exact), biased, temperature, variant)


OUTPUTS = ("loss", "pred_serial", "dU", "d_ub", "dV", "d_ib")
OP_RESULTS = ("loss", "pred_serial", "dU", "dV", "d_ub", "d_ib")          # the order ops.softmax_tiled_step returns them in


def loss_sum(case, biased, temperature, variant, U=None, V=None, ub=None, ib=None):
    """sum of the reference loss at perturbed tables (central differences)"""
    c = SimpleNamespace(**vars(case))
    c.U, c.V = (case.U if U is None else U), (case.V if V is None else V)
    c.ub, c.ib = (case.ub if ub is None else ub), (case.ib if ib is None else ib)
    nu, S, nnz = c.n_users, c.S, c.x_item.size
    xu, xi = pair_lists(c)
    sc = ref_pair_scores(c.U, c.V, xu, xi, c.mode, c.ub if biased else None, c.ib if biased else None).scores
    return float(_loss_ref(c, sc[:nnz], sc[nnz:].reshape(nu, S), temperature, variant).loss.sum())


# ------------------------------------------------------------------------------------------------ float32 restatements
def _seq32(terms):
    """float32 sum over axis 0 with one accumulator"""
    terms = np.asarray(terms, F)
    acc = np.zeros(terms.shape[1:], F)
    for x in terms:
        acc = (acc + x).astype(F)
    return acc


def _tree32(v):
    """the xor butterfly over the leading axis (a power of two): pairwise, lane i with lane i ^ off, off = n/2 ... 1"""
    v = np.asarray(v, F)
    off = v.shape[0] // 2
    while off:
        idx = np.arange(v.shape[0]) ^ off
        v = (v + v[idx]).astype(F)
        off //= 2
    return v[0]


def _wg32(terms, order, op="sum"):
    """the kernel's workgroup reduction of a 1-d list: thread k takes the slots k, k + 256, ... in ascending order, a butterfly inside
    each wave of 64, the four waves as (0 + 1) + (2 + 3); order 'seq': one accumulator over the list"""
    terms = np.asarray(terms, F)
    if op == "max":
        return F(terms.max()) if terms.size else F(-np.inf)
    if order == "seq":
        return F(_seq32(terms))
    part = np.zeros(256, F)
    for k in range(min(256, terms.size)):
        part[k] = _seq32(terms[k::256])
    w = [_tree32(part[64 * i:64 * i + 64]) for i in range(4)]
    return F(F(w[0] + w[1]) + F(w[2] + w[3]))


def _rows32(x, rows, mode, lpr, order):
    """float32 scores' raw part (dot product / squared distance) of the user row x against `rows` [n, d]: 'strided' -- lane `sub` of
    lpr takes the float4 chunks sub, sub + lpr, ... in a chain of rounded multiply-adds, the lanes join as a tree; 'seq' -- one chain"""
    x, rows = np.asarray(x, F), np.asarray(rows, F)
    t = (rows * x[None, :]).astype(F) if mode == MODE_DOT else ((x[None, :] - rows).astype(F) ** 2).astype(F)
    n, d = t.shape
    if order == "seq":
        return _seq32(t.T)
    pad = np.zeros((n, (d + 4 * lpr - 1) // (4 * lpr) * 4 * lpr), F)
    pad[:, :d] = t
    chunks = pad.reshape(n, -1, lpr, 4)                            # [row, it, lane, 4]
    lanes = _seq32(chunks.transpose(1, 3, 2, 0).reshape(-1, lpr, n))      # per lane: its it x 4 entries in turn -> [lane, row]
    return _tree32(lanes)


DEFECTS = ("mask_ignored", "positive_corrected", "max_over_hits", "euclid_unguarded", "k_over_nonpositives", "positive_without_t")


def restate_f32(case, biased, temperature, variant, order="strided", defect=None):
    """the kernel's arithmetic in float32 NumPy (fmaf chains become rounded multiply-adds): order 'strided' -- the kernel's summation
    orders (samples and interactions strided by 256 and joined by the butterfly, the row sweeps strided by subgroup); 'seq' -- every
    sum in plain order.  `defect`: one of DEFECTS seeded into it.  Returns a namespace with the six outputs, val and g."""
    use_q, no_hits, lq = VARIANTS[variant]
    lq = case.log_q if lq == "case" else None
    mode = case.mode
    t = F(1.0 / temperature)
    S, nu, d, ni = case.S, case.n_users, case.d, case.n_items
    inst = instantiation(d, mode, variant)
    lpr, nsg = inst[3], 256 // inst[3]
    U, V = case.U.astype(F), case.V.astype(F)
    log_s, log_uni = F(np.log(float(S))), F(-np.log(float(ni)))
    pos = case.values > 0
    slot = np.cumsum(pos) - 1
    nnz = case.x_item.size
    loss, pred = np.zeros(int(pos.sum()), F), np.zeros(nnz, F)
    dU, d_ub = np.zeros((nu, d), F), np.zeros(nu, F)
    g_all, val_all = np.zeros(nnz + nu * S, F), np.zeros(nnz + nu * S, F)
    with np.errstate(all="ignore"):
        for u in range(nu):
            idx = np.arange(case.indptr[u], case.indptr[u + 1])
            if not idx.size:
                continue
            items = np.concatenate([case.samples[u], case.x_item[idx]]).astype(np.int64)
            raw = _rows32(U[u], V[items], mode, lpr, order)
            y = raw if mode == MODE_DOT else (-np.sqrt(np.maximum(raw, F(EPS)))).astype(F)
            if biased:
                y = ((y + case.ub[u]).astype(F) + case.ib[items]).astype(F)
            ys, yp = y[:S], y[S:]
            pred[idx] = yp
            g = np.zeros(items.size, F)
            q = np.flatnonzero(pos[idx])
            if defect == "mask_ignored":
                hit = np.zeros(S, bool)
            else:
                hit = np.isin(case.samples[u], case.x_item[idx[q]]) if no_hits else np.zeros(S, bool)
            kept = ~hit
            dead = False
            if variant == "plain":
                M = _wg32(ys, order, "max")
                E = np.exp(((ys - M).astype(F) * t).astype(F)).astype(F)
                Z = _wg32(E, order)
                wp, tt = yp, t
            else:
                c = (-(log_s + (lq[case.samples[u]] if lq is not None else log_uni))).astype(F) if use_q else np.zeros(S, F)
                over = np.ones(S, bool) if defect == "max_over_hits" else kept
                dead = not over.any()
                if not dead:
                    Rm = _wg32(ys[over], order, "max")
                    w = (((ys - Rm).astype(F) * t).astype(F) + c).astype(F)
                    M = _wg32(w[over], order, "max")
                    E = np.where(kept, np.exp((w - M).astype(F)).astype(F), F(0)).astype(F)
                    Z = _wg32(E, order)
                    wp, tt = ((yp - Rm).astype(F) * t).astype(F), F(1.0)
                    if defect == "positive_corrected" and use_q:
                        cp = (-(log_s + (lq[case.x_item[idx]] if lq is not None else log_uni))).astype(F)
                        wp = (wp + cp).astype(F)
            terms = np.zeros(idx.size, F)
            if dead:
                loss[slot[idx[q]]] = 0.0
            else:
                over_q = np.arange(idx.size) if defect == "k_over_nonpositives" else q
                for k in over_q:
                    m = max(M, wp[k])
                    a = np.exp(F(F(wp[k] - m) * tt)).astype(F)
                    b = np.exp(F(F(M - m) * tt)).astype(F)
                    bz = F(b * Z)
                    D = F(a + bz)
                    terms[k] = F(b / D)
                    if pos[idx[k]]:
                        loss[slot[idx[k]]] = F(F(F(m - wp[k]) * tt) + np.log(D).astype(F))
                        g[S + k] = F(-F(bz / D)) if defect == "positive_without_t" else F(-t * F(bz / D))
                K = _wg32(terms, order)
                g[:S] = ((t * E).astype(F) * K).astype(F)
            if mode == MODE_DOT:
                val = g
                tu = V[items]
            else:
                root = np.sqrt(raw).astype(F)
                if defect == "euclid_unguarded":
                    val = (-g / root).astype(F)
                else:
                    val = np.where(raw >= F(EPS), (-g / np.where(root > 0, root, F(1))).astype(F), F(0)).astype(F)
                tu = (U[u][None, :] - V[items]).astype(F)
            prod = (val[:, None] * tu).astype(F)
            if order == "seq":
                dU[u] = _seq32(prod)
            else:
                dU[u] = _seq32(np.stack([_seq32(prod[k::nsg]) if k < prod.shape[0] else np.zeros(d, F) for k in range(nsg)]))
            own = np.concatenate([g[S:], g[:S]])                   # a thread adds its interactions first, then its samples
            d_ub[u] = _wg32(own, "seq") if order == "seq" else _wg_two(g[S:], g[:S])
            g_all[idx], val_all[idx] = g[S:], val[S:]
            g_all[nnz + u * S:nnz + (u + 1) * S], val_all[nnz + u * S:nnz + (u + 1) * S] = g[:S], val[:S]
        xu, xi = pair_lists(case)
        dV, d_ib = np.zeros((ni, d), F), np.zeros(ni, F)
        tv = U[xu] if mode == MODE_DOT else (V[xi] - U[xu]).astype(F)
        prod = (val_all[:, None] * tv).astype(F)
        walk = np.arange(xu.size) if order == "seq" else np.arange(xu.size)[::-1]
        np.add.at(dV, xi[walk], prod[walk])
        np.add.at(d_ib, xi[walk], g_all[walk])
    return SimpleNamespace(loss=loss, pred_serial=pred, dU=dU, dV=dV, d_ub=d_ub, d_ib=d_ib, g=g_all, val=val_all)


def _wg_two(first, second):
    """d b_u in the kernel's order: thread k adds its interactions k, k + 256, ... and then its samples k, k + 256, ... into one
    accumulator; butterfly; (0 + 1) + (2 + 3)"""
    part = np.zeros(256, F)
    for k in range(256):
        part[k] = _seq32(np.concatenate([np.asarray(first, F)[k::256], np.asarray(second, F)[k::256]]))
    w = [_tree32(part[64 * i:64 * i + 64]) for i in range(4)]
    return F(F(w[0] + w[1]) + F(w[2] + w[3]))


def ratios(got, ref, biased, names=OUTPUTS):
    """{output: largest |got - reference| / bar}; a bar of 0 asks for equality (ratio 0 when equal, inf otherwise)"""
    out = {}
    for name in names:
        if name in ("d_ub", "d_ib") and not biased:
            continue
        g, w, b = f64(getattr(got, name)).reshape(-1), f64(getattr(ref, name)).reshape(-1), f64(getattr(ref, "b_" + name)).reshape(-1)
        assert g.shape == w.shape, name
        if not np.isfinite(g).all():                              # (an overflow of a seeded defect: outside every bar)
            out[name] = float("inf")
            continue
        err = np.abs(g - w)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[name] = float(np.where(err == 0, 0.0, err / b).max()) if g.size else 0.0
    return out
