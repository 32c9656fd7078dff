"""Float64 reference, error bars, inputs, a float32 restatement and the dispatch mirror for the one-pass sampled-softmax step
(csrc/softmax_fused.hip, trec_softmax_fused_step, ops.softmax_fused_step).  NumPy / SciPy only, nothing of the code under test.
tests/test_softmax_step_reference_host.py holds the reference to central differences and the bars to the restatement on the CPU (and
shows that seeded defects fall outside); tests/test_gpu_softmax_fused.py holds the kernel to the reference.

The step.  Scores of the interactions and of the [U, S] samples (pair_reference.ref_pair_scores, dot), the loss on them with
upstream gradient 1 (sampled_loss_reference.ref_sampled_softmax, or sampled_adjust_reference.ref_sampled_softmax_adj when an option
is on), the gradients of the tables and biases through pair_reference.ref_pair_grads fed with the reference d_pred / d_samp.

Bars.  Nothing is tuned; every bar is one of
* pred_serial        pair_reference.score_bar =: delta_p.
* the loss kernels'  own bars (the two loss reference modules), plus what the scores' error does to them, as the docstring of
                     tests/test_gpu_sampled_losses.py::test_one_fit_step_against_float64 derives it: the loss phase is handed float32
                     scores off by at most delta; with delta_u the largest delta among a user's interactions and samples, moving every
                     logit by at most t delta_u multiplies each exponential ratio by a factor within exp(+-2 t delta_u): loss_p moves by
                     at most 2 t delta_u, d y_p and d y_us by a relative expm1(2 t delta_u).  (The corrections c_s are constants and the
                     hit mask depends on ids only: the same holds for the adjusted loss.)  This gives bar_g per pair.
* dU, dV, d b_u, d b_i   pair_reference.grad_bars for the sums themselves (m + 1 roundings on sum |terms|), plus bar_g carried through:
                     sum_p bar_g_p |d score_p / d entry| (|v_c| resp. |u_c|; biases: 1).
The dyadic family (tables and biases multiples of 1/8: every partial sum of a score is a multiple of 2^-6 far below 2^24, exact in
float32 in any order -- scores_exact asserts it) has delta = 0: pred_serial is held bit for bit and the loss phase stands alone.
An entry whose terms are all 0 (dU / d b_u of a user without positives, the dV row of an item that only hits touch) has a bar of 0."""
import functools
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

import sampled_adjust_reference as AR
import sampled_loss_reference as LR
from pair_reference import MODE_DOT, U32, f64, grad_bars, ref_pair_grads, ref_pair_scores, score_bar

F = np.float32

# (log_q_correction, remove_hits, log q: "case" = the case's table | None = uniform)
VARIANTS = {"plain": (False, False, None), "logq": (True, False, "case"), "logq-uniform": (True, False, None),
            "hits": (False, True, None), "both": (True, True, "case"), "both-uniform": (True, True, None)}
TEMPERATURES = [1.0, 0.25]


# ------------------------------------------------------------------------------------------------ which kernel a call takes
ALL_INSTANTIATIONS = {(1, 16, 0), (1, 16, 4), (1, 16, 8), (1, 16, 12), (1, 32, 0), (1, 32, 16), (2, 16, 0), (2, 16, 8)}


def rows_capacity(d):
    return 256 if d <= 128 else 128


def instantiation(S, max_pos, d):
    """<ITERS, RMAX, SURE> of softmax_user_fused_kernel (the dispatch USER_FUSED_LAUNCH of csrc/user_fused_body.hpp), None where
    trec_softmax_fused_lds_bytes is -1"""
    if S < 1 or S > 256 or d < 4 or d % 4 or d > 256 or max_pos < 0 or S + max_pos > rows_capacity(d):
        return None
    sure = S // 8
    if d <= 128 and S + max_pos <= 128:
        return (1, 16, 12 if sure >= 12 else 8 if sure >= 8 else 4 if sure >= 4 else 0)
    if d <= 128:
        return (1, 32, 16 if sure >= 16 else 0)
    return (2, 16, 8 if sure >= 8 else 0)


def lds_bytes(S, max_pos, d):
    if instantiation(S, max_pos, d) is None:
        return -1
    return (4 * ((S + max_pos + 3) // 4 * 4) + 16 + 8 * d) * 4


# ------------------------------------------------------------------------------------------------ inputs
# the users of every case; rows are cut to the case's longest row
U_NONE, U_NONPOS, U_ONE, U_LONG, U_MIXED, U_ABOVE, U_BELOW, U_EQUAL, U_ALLEQ, U_SPAN, U_ALLHITS, U_NONPOS_ITEM, U_PLAIN = range(13)
N_USERS = 13
FAR = 100.0
SPAN = 30.0

# (S, longest row, d): every instantiation, rows at the register capacity, d with zeroed columns past it (36) -- 13 users each
GPU_CASES = [(1, 3, 4), (7, 20, 36), (33, 20, 128), (64, 33, 64), (100, 28, 128),
             (40, 100, 128), (128, 128, 64), (255, 1, 36),
             (7, 30, 132), (64, 64, 256), (7, 121, 256), (64, 20, 132)]
UNCOVERED = [(3, 126, 132), (1, 256, 128), (257, 1, 128), (7, 5, 6)]       # rows 129 at d 132; rows 257 at d 128; S 257; d 6


def softmax_case(S, longest, d, exact=False, seed=0):
    """13 users.  0: no interaction; 1: interactions of value <= 0 only; 2: one positive; 3: the longest row (`longest` interactions, a
    few of value <= 0 mixed in where it has five or more) with a duplicated sample (S >= 2); 4: mixed signs (values 1, -1, 0, 2, 0.5);
    5: a positive FAR above every sample; 6: a positive FAR below every sample; 7: a positive whose score equals its samples' maximum
    bit for bit (its item carries the row and the bias of the sampled item with the largest score); 8: all samples the same item
    (equal scores); 9: samples on reserved items with zero rows and biases spanning +-SPAN; 10: every sample one of its positives
    (all hits); 11: slot 0 holds the item of an interaction of value <= 0 (no hit) and slot 1 (S >= 2) one of its positives (a hit);
    12: nothing planted.  The planted scores go through item biases, so they are what they mean in the runs WITH biases.
    exact: tables and biases multiples of 1/8 (delta = 0).  log_q: a table spanning -2 ... -14 (any table will do)."""
    rng = np.random.default_rng(7001 * S + 101 * longest + 13 * d + (5 if exact else 0) + seed)
    want = [0, 2, 1, longest, 5, 3, 3, 4, 3, 2, 6, 5, 4]
    lens = [min(n, longest) for n in want]
    n_reg = max(160, longest + 45)
    span0 = n_reg                                                 # S reserved items: the samples of U_SPAN
    far_above, far_below, equal_item = n_reg + S, n_reg + S + 1, n_reg + S + 2
    n_items = n_reg + S + 3
    if exact:
        U = (rng.integers(-8, 9, size=(N_USERS, d)) / 8.0 * (rng.random((N_USERS, d)) < min(1.0, 16.0 / d))).astype(F)
        V = (rng.integers(-8, 9, size=(n_items, d)) / 8.0 * (rng.random((n_items, d)) < min(1.0, 16.0 / d))).astype(F)
        ub = (rng.integers(-8, 9, N_USERS) / 8.0).astype(F)
        ib = (rng.integers(-8, 9, n_items) / 8.0).astype(F)
    else:
        U = (rng.standard_normal((N_USERS, d)) / np.sqrt(d)).astype(F)
        V = (2.0 * rng.standard_normal((n_items, d))).astype(F)
        ub = (0.5 * rng.standard_normal(N_USERS)).astype(F)
        ib = (0.5 * rng.standard_normal(n_items)).astype(F)
    r_idx, c_idx, vals = [], [], []
    for u, n in enumerate(lens):
        cols = np.sort(rng.choice(n_reg - 5, size=n, replace=False))
        if u == U_NONPOS_ITEM:
            cols = n_reg - 5 + np.arange(n)                       # columns of its own: nobody else interacts with them
        v = (rng.integers(1, 13, size=n) / 4.0)
        if u == U_NONPOS:
            v[:] = [-1.0, 0.0][:n]
        elif u == U_MIXED:
            v[:] = [1.0, -1.0, 0.0, 2.0, 0.5][:n]
        elif u == U_NONPOS_ITEM and n >= 2:
            v[0] = -1.0
        elif u == U_LONG and n >= 5:
            v[1], v[n - 2] = -1.0, 0.0
        r_idx += [u] * n
        c_idx += list(cols)
        vals += list(v)
    m = sp.csr_matrix((np.array(vals, F), (np.array(r_idx), np.array(c_idx))), shape=(N_USERS, n_items))
    assert m.nnz == len(vals) and m.has_sorted_indices
    indptr, x_item, values = m.indptr.astype(np.int64), m.indices.astype(np.int32).copy(), m.data.astype(F)
    samples = rng.integers(0, n_reg, size=(N_USERS, S)).astype(np.int32)

    def row(u, positive=None):
        idx = np.arange(indptr[u], indptr[u + 1])
        if positive is not None:
            idx = idx[(values[idx] > 0) == positive]
        return idx
    if S >= 2:
        samples[U_LONG, 1] = samples[U_LONG, 0]
    samples[U_ALLEQ] = samples[U_ALLEQ, 0]
    samples[U_SPAN] = span0 + rng.permutation(S)
    V[span0:span0 + S] = 0.0
    span = np.linspace(-SPAN, SPAN, S) if S > 1 else np.array([SPAN])
    ib[span0:span0 + S] = (np.round(span * 8.0) / 8.0).astype(F)
    samples[U_ALLHITS] = x_item[rng.choice(row(U_ALLHITS, True), size=S)]
    if row(U_NONPOS_ITEM, False).size:
        samples[U_NONPOS_ITEM, 0] = x_item[row(U_NONPOS_ITEM, False)[0]]
    hit_item = -1
    if S >= 2 and row(U_NONPOS_ITEM, True).size:
        # a positive of this user (whose columns are nobody else's), sampled here and nowhere else: with hits removed only the
        # interaction's own term reaches the item's gradient row
        hit_item = int(x_item[row(U_NONPOS_ITEM, True)[0]])
        samples[samples == hit_item] = 0
        samples[U_NONPOS_ITEM, 1] = hit_item
    # the planted positives: the LAST interaction of the user is moved onto a reserved item (beyond every regular column: the row
    # stays sorted); scores of the samples in float64 with biases
    def sample_scores(u):
        return f64(V)[samples[u]] @ f64(U)[u] + float(ub[u]) + f64(ib)[samples[u]]
    for u, item, off in ((U_ABOVE, far_above, FAR), (U_BELOW, far_below, -FAR)):
        x_item[indptr[u + 1] - 1] = item
        values[indptr[u + 1] - 1] = 1.0
        V[item] = 0.0
        s = sample_scores(u)
        target = (s.max() + FAR if off > 0 else s.min() - FAR) - float(ub[u])
        ib[item] = F(np.ceil(target * 8.0) / 8.0 if off > 0 else np.floor(target * 8.0) / 8.0)
    top = int(samples[U_EQUAL, int(np.argmax(sample_scores(U_EQUAL)))])
    x_item[indptr[U_EQUAL + 1] - 1] = equal_item
    values[indptr[U_EQUAL + 1] - 1] = 1.0
    V[equal_item], ib[equal_item] = V[top], ib[top]
    log_q = rng.permutation(np.linspace(-2.0, -14.0, n_items)).astype(F)
    m = sp.csr_matrix((values, x_item, indptr), shape=(N_USERS, n_items))
    assert m.has_sorted_indices
    return SimpleNamespace(U=U, V=V, ub=ub, ib=ib, matrix=m, indptr=indptr, x_item=x_item, cols=x_item, values=values, samples=samples,
                           items=samples, log_q=log_q, S=S, d=d, n_users=N_USERS, n_items=n_items, longest=longest,
                           max_pos=int(np.diff(indptr).max()), exact=exact, equal_top=top, hit_item=hit_item,
                           planted=SimpleNamespace(above=int(indptr[U_ABOVE + 1] - 1), below=int(indptr[U_BELOW + 1] - 1),
                                                   equal=int(indptr[U_EQUAL + 1] - 1)))


def scores_exact(case):
    """the premise of delta = 0: tables and biases multiples of 1/8, every sum of |terms| of a score below 2^17 (a multiple of 2^-6
    with fewer than 24 bits: exact in float32 in any order)"""
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


def case_properties(case, biased=True):
    """what the cases are meant to hold, as a dict the host test asserts (scores with biases)"""
    xu, xi = pair_lists(case)
    sc = ref_pair_scores(case.U, case.V, xu, xi, MODE_DOT, case.ub, case.ib).scores
    nnz = case.x_item.size
    yp, ys = sc[:nnz], sc[nnz:].reshape(case.n_users, case.S)
    lens = np.diff(case.indptr)
    pos = case.values > 0
    row_pos = lambda u: pos[case.indptr[u]:case.indptr[u + 1]]
    hits = AR.hit_mask(case.indptr, case.x_item, case.values, case.samples)
    p = case.planted
    return dict(longest=int(lens.max()), no_interaction=bool(lens[U_NONE] == 0),
                nonpositive_only=bool(lens[U_NONPOS] > 0 and not row_pos(U_NONPOS).any()), one_positive=bool(lens[U_ONE] == 1 and row_pos(U_ONE).all()),
                mixed=bool(row_pos(U_MIXED).any() and not row_pos(U_MIXED).all()),
                far_above=float(yp[p.above] - ys[U_ABOVE].max()), far_below=float(ys[U_BELOW].min() - yp[p.below]),
                equal=bool(F(yp[p.equal]) == F(ys[U_EQUAL].max())) and bool(case.samples[U_EQUAL, int(np.argmax(ys[U_EQUAL]))] == case.equal_top),
                all_equal=bool((case.samples[U_ALLEQ] == case.samples[U_ALLEQ, 0]).all()), span=float(ys[U_SPAN].max() - ys[U_SPAN].min()),
                all_hits=bool(hits[U_ALLHITS].all()), nonpos_item_no_hit=bool(not hits[U_NONPOS_ITEM, 0]),
                a_hit=bool(case.S < 2 or lens[U_NONPOS_ITEM] < 2 or hits[U_NONPOS_ITEM, 1]),
                duplicate=bool(case.S < 2 or case.samples[U_LONG, 0] == case.samples[U_LONG, 1]), rows=int(case.S + lens.max()))


# ------------------------------------------------------------------------------------------------ reference
def ref_step(case, biased, temperature, variant="plain", log_q_table="case"):
    """the float64 step and its bars: a namespace with loss, pred_serial, dU, dV, d_ub, d_ib and b_<name> for each, g (d_pred | d_samp
    flat) with b_g, and the hit mask"""
    use_q, no_hits, lq = VARIANTS[variant]
    if lq == "case":
        lq = case.log_q if isinstance(log_q_table, str) else log_q_table
    d, S, nu, nnz = case.d, case.S, case.n_users, case.x_item.size
    ub, ib = (case.ub, case.ib) if biased else (None, None)
    xu, xi = pair_lists(case)
    sc = ref_pair_scores(case.U, case.V, xu, xi, MODE_DOT, ub, ib)
    delta = np.zeros(xu.size) if case.exact else score_bar(sc, d)
    if case.exact:
        assert scores_exact(case)
    yp, ys = sc.scores[:nnz], sc.scores[nnz:].reshape(nu, S)
    n_pos = int((case.values > 0).sum())
    go = np.ones(n_pos)
    if variant == "plain":
        lr = LR.ref_sampled_softmax(case.indptr, case.values, yp, ys, go, temperature)
        hits = np.zeros((nu, S), bool)
    else:
        lc = SimpleNamespace(indptr=case.indptr, values=case.values, cols=case.x_item, pred=yp, samp=ys, go=go, items=case.samples,
                             log_q=lq, n_items=case.n_items)
        lr = AR.ref_sampled_softmax_adj(lc, temperature, use_q, no_hits, log_q=lq)
        hits = lr.hits
    t = 1.0 / float(temperature)
    du = np.zeros(nu)                                             # delta_u
    np.maximum.at(du, xu, delta)
    pos = case.values > 0
    f = np.expm1(2.0 * t * du)
    r = SimpleNamespace(loss=lr.loss, pred_serial=yp, hits=hits, scores=sc, delta=delta)
    r.b_pred_serial = delta[:nnz]
    r.b_loss = lr.bar_loss + 2.0 * t * du[xu[:nnz]][pos]                  # (slots follow the CSR order of the positives)
    r.g = np.concatenate([lr.d_pred, lr.d_samp.reshape(-1)])
    r.b_g = np.concatenate([lr.bar_d_pred, lr.bar_d_samp.reshape(-1)]) + np.abs(r.g) * f[xu]
    pg = ref_pair_grads(case.U, case.V, xu, xi, r.g, MODE_DOT)
    inh = ref_pair_grads(np.abs(f64(case.U)), np.abs(f64(case.V)), xu, xi, r.b_g, MODE_DOT)
    bU, bV, bub, bib = grad_bars(pg, d)
    r.dU, r.dV, r.d_ub, r.d_ib = pg.dU, pg.dV, pg.dub, pg.dib
    r.b_dU, r.b_dV, r.b_d_ub, r.b_d_ib = bU + inh.dU, bV + inh.dV, bub + inh.dub, bib + inh.dib
    r.pg = pg
    return r


@functools.lru_cache(maxsize=None)
def cached_case(spec, exact):
    return softmax_case(*spec, exact=exact)


@functools.lru_cache(maxsize=None)
def cached_ref(spec, exact, biased, temperature, variant):
    """computed once and shared by the host and the GPU tests; nobody writes into it"""
    return ref_step(cached_case(spec, exact), biased, temperature, variant)


OUTPUTS = ("loss", "pred_serial", "dU", "d_ub", "dV", "d_ib")
OP_RESULTS = ("loss", "pred_serial", "dU", "dV", "d_ub", "d_ib")          # the order ops.softmax_fused_step returns them in


def loss_sum(case, biased, temperature, variant, U=None, V=None, ub=None, ib=None):
    """sum of the reference loss at perturbed tables (central differences)"""
    c = SimpleNamespace(**vars(case))
    c.U, c.V = (case.U if U is None else U), (case.V if V is None else V)
    c.ub, c.ib = (case.ub if ub is None else ub), (case.ib if ib is None else ib)
    c.exact = False
    return float(ref_step_loss_only(c, biased, temperature, variant).sum())


def ref_step_loss_only(case, biased, temperature, variant):
    use_q, no_hits, lq = VARIANTS[variant]
    lq = case.log_q if lq == "case" else None
    nu, S, nnz = case.n_users, case.S, case.x_item.size
    xu, xi = pair_lists(case)
    sc = ref_pair_scores(case.U, case.V, xu, xi, MODE_DOT, case.ub if biased else None, case.ib if biased else None).scores
    yp, ys = sc[:nnz], sc[nnz:].reshape(nu, S)
    go = np.ones(int((case.values > 0).sum()))
    if variant == "plain":
        return LR.ref_sampled_softmax(case.indptr, case.values, yp, ys, go, temperature).loss
    lc = SimpleNamespace(indptr=case.indptr, values=case.values, cols=case.x_item, pred=yp, samp=ys, go=go, items=case.samples,
                         log_q=lq, n_items=case.n_items)
    return AR.ref_sampled_softmax_adj(lc, temperature, use_q, no_hits, log_q=lq).loss


# ------------------------------------------------------------------------------------------------ float32 restatement
def _sum32(terms, order):
    """float32 sum of a 1-d or [n, k] array over axis 0: 'seq' one accumulator, an integer P: P interleaved partials added in turn"""
    terms = np.asarray(terms, F)
    if order == "seq":
        acc = np.zeros(terms.shape[1:], F)
        for x in terms:
            acc = F(acc + x) if acc.ndim == 0 else (acc + x).astype(F)
        return acc
    parts = [_sum32(terms[k::order], "seq") for k in range(order)]
    return _sum32(np.stack(parts), "seq")


DEFECTS = ("k_without_b", "samples_without_t", "z_without_shift", "positive_corrected", "mask_per_positive", "nonpositive_is_hit",
           "dub_without_samples")


def restate_f32(case, biased, temperature, variant, order="seq", defect=None):
    """the kernel's arithmetic in float32 NumPy: fmaf chains become rounded multiply-adds, the reductions run in `order` ('seq', or
    P interleaved partials); `defect`: one of DEFECTS seeded into it.  Returns a namespace with the six outputs."""
    use_q, no_hits, lq = VARIANTS[variant]
    lq = case.log_q if lq == "case" else None
    t = F(1.0 / temperature)
    S, nu, d, ni = case.S, case.n_users, case.d, case.n_items
    U, V = case.U.astype(F), case.V.astype(F)
    log_s, log_uni = F(np.log(float(S))), F(-np.log(float(ni)))
    pos = case.values > 0
    slot = np.cumsum(pos) - 1
    loss = np.zeros(int(pos.sum()), F)
    pred = np.zeros(case.x_item.size, F)
    dU, dV = np.zeros((nu, d), F), np.zeros((ni, d), F)
    d_ub, d_ib = np.zeros(nu, F), np.zeros(ni, F)
    pair_u, pair_i, pair_g = [], [], []
    for u in range(nu):
        idx = np.arange(case.indptr[u], case.indptr[u + 1])
        items = np.concatenate([case.samples[u], case.x_item[idx]]).astype(np.int64)
        y = _sum32((V[items] * U[u][None, :]).T, order if order == "seq" else min(order, d))
        if biased:
            y = ((y + case.ub[u]).astype(F) + case.ib[items]).astype(F)
        ys, yp = y[:S], y[S:]
        pred[idx] = yp
        coef = np.zeros(items.size, F)
        q = np.flatnonzero(pos[idx])
        if idx.size:
            if defect == "nonpositive_is_hit":
                hit = np.isin(case.samples[u], case.x_item[idx])
            else:
                hit = np.isin(case.samples[u], case.x_item[idx[q]])
            kept = ~hit if no_hits else np.ones(S, bool)
            c = np.zeros(S, F)
            if use_q:
                c = (-(log_s + (lq[case.samples[u]] if lq is not None else log_uni))).astype(F)
            if variant == "plain":
                M = ys.max()
                E = np.exp(((ys - M).astype(F) * t).astype(F)).astype(F)
                if defect == "z_without_shift":
                    with np.errstate(over="ignore", invalid="ignore"):
                        Z = F(_sum32(np.exp((ys * t).astype(F)).astype(F), order) / np.exp(F(M * t)).astype(F))
                else:
                    Z = _sum32(E, order)
                wp, tt, Mx = yp, t, M
            elif kept.any():
                Rm = ys[kept].max()
                w = np.where(kept, (((ys - Rm).astype(F) * t).astype(F) + c).astype(F), F(-np.inf)).astype(F)
                Mx = w.max()
                E = np.exp((w - Mx).astype(F)).astype(F)
                if defect == "z_without_shift":
                    with np.errstate(over="ignore", invalid="ignore"):
                        Z = F(_sum32(np.exp(w).astype(F), order) / np.exp(Mx).astype(F))
                else:
                    Z = _sum32(E, order)
                wp, tt = ((yp - Rm).astype(F) * t).astype(F), F(1.0)
                if defect == "positive_corrected" and use_q:
                    cp = (-(log_s + (lq[case.x_item[idx]] if lq is not None else log_uni))).astype(F)
                    wp = (wp + cp).astype(F)
            else:
                loss[slot[idx[q]]] = 0.0
                E = None
            if E is not None and q.size:
                terms = np.zeros(idx.size, F)
                for k in q:
                    if defect == "mask_per_positive" and no_hits:            # only the positive's own item is masked, for it alone
                        own = case.samples[u] != case.x_item[idx[k]]
                        wk = (((ys - Rm).astype(F) * t).astype(F) + c).astype(F)
                        Zk = _sum32(np.where(own, np.exp((wk - Mx).astype(F)).astype(F), F(0)), order)
                    else:
                        Zk = Z
                    m = max(Mx, wp[k])
                    a = np.exp(F(F(wp[k] - m) * tt)).astype(F)
                    b = np.exp(F(F(Mx - m) * tt)).astype(F)
                    bz = F(b * Zk)
                    D = F(a + bz)
                    loss[slot[idx[k]]] = F(F(F(m - wp[k]) * tt) + np.log(D).astype(F))
                    coef[S + k] = F(-t * F(bz / D))
                    terms[k] = F(1.0 / D) if defect == "k_without_b" else F(b / D)
                K = _sum32(terms, order)
                cs = (E * K).astype(F) if defect == "samples_without_t" else ((t * E).astype(F) * K).astype(F)
                coef[:S] = np.where(kept, cs, F(0)) if variant != "plain" else cs
        dU[u] = _sum32(coef[:, None] * V[items], order) if items.size else 0
        d_ub[u] = _sum32(coef[S:], order) if defect == "dub_without_samples" else _sum32(coef, order)
        pair_u += [u] * items.size
        pair_i += list(items)
        pair_g += list(coef)
    pair_u, pair_i, pair_g = np.array(pair_u), np.array(pair_i), np.array(pair_g, F)
    for i in np.unique(pair_i):
        k = np.flatnonzero(pair_i == i)
        dV[i] = _sum32(pair_g[k][:, None] * U[pair_u[k]], order)
        d_ib[i] = _sum32(pair_g[k], order)
    return SimpleNamespace(loss=loss, pred_serial=pred, dU=dU, dV=dV, d_ub=d_ub, d_ib=d_ib)


def ratios(got, ref, biased):
    """{output: largest |got - reference| / bar}; a bar of 0 asks for equality (ratio 0 when equal, inf otherwise)"""
    out = {}
    for name in OUTPUTS:
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
