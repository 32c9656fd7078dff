"""Float64 reference, error bars, inputs and a float32 restatement for the one-pass BPR step (csrc/bpr_fused.hip,
trec_bpr_fused_step, ops.bpr_fused_step).  NumPy / SciPy only, nothing of the code under test.
tests/test_bpr_step_reference_host.py holds the reference to central differences and the bars to the restatement on the CPU (and
shows that seeded defects fall outside); tests/test_gpu_bpr_fused.py holds the kernel to the reference.

The step.  Scores of the interactions and of the [U, S] samples (pair_reference.ref_pair_scores, dot), the BPR loss on them with
upstream gradient 1 (sampled_loss_reference.ref_bpr, or sampled_adjust_reference.ref_bpr_adj with hits removed: loss,
d_pred = coef_pairs, d_samp = coef_samples), the gradients of the tables and biases through pair_reference.ref_pair_grads fed with
those coefficients.  The instantiation ladder of the kernel is the sampled-softmax step's: its mirror (instantiation, GPU_CASES,
UNCOVERED) and its inputs (softmax_case) are imported from tests/softmax_step_reference.py and only read; lds_bytes is this
kernel's own (the wave sums and the sample partials of its loss phase need room).

Bars.  Nothing is tuned; every bar is one of
* pred_serial        pair_reference.score_bar =: delta (per pair); 0 on the dyadic family (scores_exact).
* loss, coef_pairs, coef_samples   ref_bpr's own bars (they take the float32 scores as exact inputs), plus what the scores' error
                     does: the loss phase is handed float32 scores off by at most delta, so x_ps = y_s - y_p is off by at most
                     delta_p + delta_s.  softplus has slope sigma <= 1 and sigma has slope sigma (1 - sigma) <= 1/4, hence
                         loss_p   moves by at most (1/S) sum_{s kept} (delta_p + delta_s)           (<= delta_p + mean_s delta_s)
                         coef_p   by at most (1/S) sum_{s kept} (delta_p + delta_s) / 4
                         coef_s   by at most (1/S) sum_{p of u, positive} (delta_p + delta_s) / 4   (s kept; a hit stays an exact 0)
                     times (1 + 8 u) for the bars of ref_bpr being taken at the float64 scores and not at the rounded ones.
* dU, dV, d b_u, d b_i   pair_reference.grad_bars for the sums (m + 1 roundings on sum |terms|), plus the coefficients' bars carried
                     through |d score / d entry| (|v_c| resp. |u_c|; biases: 1).
An entry whose terms are all 0 (coef_p of an interaction of value <= 0, coef_s of a hit or of a user without a positive, dU / d b_u of
such a user, the dV row of an item that only such pairs touch) has a bar of 0: it must be an exact 0.

Which shapes (SPECS).  GPU_CASES reach all eight <ITERS, RMAX, SURE>.  The loss phase of csrc/bpr_fused.hip adds edges of its own:
W = 1, 2, 4 waves hold the samples (S <= 64, <= 128, above), G = 4 / W groups share a user's interactions q = g (mod G), a wave
whose 64 sample slots are all past S is skipped (S = 129 .. 192).  The rule: every W; S one past a multiple of 64 on both sides of
a change of W (65, 129) and at the top of the skipped wave's range (192); at every G > 1 rows whose length is no multiple of G
(softmax_case's users have 1, 2, 3, 5 and 6 interactions wherever the longest row allows: (40, 5, 32) for G = 4 with the longest
row itself 5, (65, 5, 64) for G = 2) and rows shorter than G (groups without an interaction)."""
import functools
from types import SimpleNamespace

import numpy as np

import sampled_adjust_reference as AR
import sampled_loss_reference as LR
from pair_reference import MODE_DOT, U32, f64, grad_bars, ref_pair_grads, ref_pair_scores, score_bar
from softmax_step_reference import (ALL_INSTANTIATIONS, GPU_CASES, UNCOVERED, N_USERS, U_NONE, U_NONPOS, U_ONE, U_LONG,  # noqa: F401
                                    U_MIXED, U_ABOVE, U_BELOW, U_EQUAL, U_ALLEQ, U_SPAN, U_ALLHITS, U_NONPOS_ITEM, U_PLAIN,
                                    _sum32, case_properties, instantiation, pair_lists, rows_capacity, scores_exact, softmax_case)

F = np.float32

LOSS_PHASE_EDGES = [(65, 5, 64), (129, 3, 64), (192, 20, 64), (40, 5, 32)]
SPECS = list(GPU_CASES) + LOSS_PHASE_EDGES


def sample_waves(S):
    """W of csrc/bpr_fused.hip: the waves that hold a user's samples, a power of two"""
    return 1 if S <= 64 else 2 if S <= 128 else 4


def lds_bytes(S, max_pos, d):
    """trec_bpr_fused_lds_bytes: y | coef | slots | hit ids [rows4 each] | the wave sums, 2 W max_pos rounded up to 4 | the sample
    partials [256] | partial dU [8][d], in 4-byte words"""
    if instantiation(S, max_pos, d) is None:
        return -1
    r4 = (S + max_pos + 3) // 4 * 4
    sums = (2 * sample_waves(S) * max_pos + 3) // 4 * 4
    return (4 * r4 + sums + 256 + 8 * d) * 4


# ------------------------------------------------------------------------------------------------ reference
def _loss_phase(case, yp, ys, remove_hits):
    go = np.ones(int((case.values > 0).sum()))
    if not remove_hits:
        return LR.ref_bpr(case.indptr, case.values, yp, ys, go), np.zeros(ys.shape, bool)
    lc = SimpleNamespace(indptr=case.indptr, values=case.values, cols=case.x_item, pred=yp, samp=ys, go=go, items=case.samples)
    lr = AR.ref_bpr_adj(lc, True)
    return lr, lr.hits


def ref_step(case, biased, remove_hits):
    """the float64 step and its bars: a namespace with loss, pred_serial, coef_pairs, coef_samples, dU, dV, d_ub, d_ib and b_<name>
    for each; hits (the [U, S] mask, all False without hit removal); scores (ref_pair_scores' answer)"""
    d, S, nu, nnz = case.d, case.S, case.n_users, case.x_item.size
    ub, ib = (case.ub, case.ib) if biased else (None, None)
    xu, xi = pair_lists(case)
    sc = ref_pair_scores(case.U, case.V, xu, xi, MODE_DOT, ub, ib)
    exact = getattr(case, "exact", False)
    delta = np.zeros(xu.size) if exact else score_bar(sc, d)
    if exact:
        assert scores_exact(case)
    yp, ys = sc.scores[:nnz], sc.scores[nnz:].reshape(nu, S)
    pos = case.values > 0
    lr, hits = _loss_phase(case, yp, ys, remove_hits)
    delta_p, delta_s = delta[:nnz], delta[nnz:].reshape(nu, S)
    c_loss, c_ds = np.zeros(nnz), np.zeros((nu, S))              # the scores' error carried through the loss phase
    for u in range(nu):
        idx = np.arange(case.indptr[u], case.indptr[u + 1])
        idx = idx[pos[idx]]
        kept = ~hits[u]
        if not idx.size or not kept.any():
            continue
        c_loss[idx] = (kept.sum() * delta_p[idx] + delta_s[u, kept].sum()) / S
        c_ds[u, kept] = (delta_p[idx].sum() + idx.size * delta_s[u, kept]) / (4.0 * S)
    more = 1.0 + 8.0 * U32
    r = SimpleNamespace(bpr=lr, hits=hits, scores=sc, delta=delta, pred_serial=yp, b_pred_serial=delta_p)
    r.loss, r.b_loss = lr.loss, lr.bar_loss + more * c_loss[pos]
    r.coef_pairs, r.b_coef_pairs = lr.d_pred, lr.bar_d_pred + more * c_loss / 4.0
    r.coef_samples, r.b_coef_samples = lr.d_samp, lr.bar_d_samp + more * c_ds
    g = np.concatenate([r.coef_pairs, r.coef_samples.reshape(-1)])
    b_g = np.concatenate([r.b_coef_pairs, r.b_coef_samples.reshape(-1)])
    pg = ref_pair_grads(case.U, case.V, xu, xi, g, MODE_DOT)
    inh = ref_pair_grads(np.abs(f64(case.U)), np.abs(f64(case.V)), xu, xi, b_g, MODE_DOT)       # b_g through |d score / d entry|
    bU, bV, bub, bib = grad_bars(pg, d)
    r.dU, r.dV, r.d_ub, r.d_ib = pg.dU, pg.dV, pg.dub, pg.dib
    r.b_dU, r.b_dV, r.b_d_ub, r.b_d_ib = bU + inh.dU, bV + inh.dV, bub + inh.dub, bib + inh.dib
    return r


@functools.lru_cache(maxsize=None)
def cached_case(spec, exact):
    return softmax_case(*spec, exact=exact)


@functools.lru_cache(maxsize=None)
def cached_ref(spec, exact, biased, remove_hits):
    """computed once and shared by the host and the GPU tests; nobody writes into it"""
    return ref_step(cached_case(spec, exact), biased, remove_hits)


OUTPUTS = ("pred_serial", "loss", "coef_pairs", "coef_samples", "dU", "d_ub", "dV", "d_ib")


def loss_sum(case, biased, remove_hits, U=None, V=None, ub=None, ib=None):
    """sum of the reference loss at perturbed tables (central differences)"""
    c = SimpleNamespace(**vars(case))
    c.U, c.V = (case.U if U is None else U), (case.V if V is None else V)
    c.ub, c.ib = (case.ub if ub is None else ub), (case.ib if ib is None else ib)
    nnz = case.x_item.size
    xu, xi = pair_lists(c)
    sc = ref_pair_scores(c.U, c.V, xu, xi, MODE_DOT, c.ub if biased else None, c.ib if biased else None).scores
    return float(_loss_phase(case, sc[:nnz], sc[nnz:].reshape(case.n_users, case.S), remove_hits)[0].loss.sum())


# ------------------------------------------------------------------------------------------------ float32 restatement
# the divisor is the number of kept samples instead of S; a hit stays in the sums; sigma(-x) for sigma(x); an interaction of
# value <= 0 counted as a positive; the partial of the last group left out of coef_s
DEFECTS = ("kept_divisor", "hit_kept", "sigma_sign", "nonpositive_counted", "group_dropped")


def _butterfly64(v):
    """the xor butterfly of wave_sum over 64 lanes (v zero-padded to 64), float32; the value every lane ends with"""
    a = np.zeros(64, F)
    a[:v.size] = v
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        a = (a + a[lanes ^ off]).astype(F)
    assert (a == a[0]).all()
    return a[0]


def cell_f32(x):
    """(softplus, sigma) of float32 x, each operation rounded to float32: e = exp(-|x|) shared, as softplus_sigmoid_f"""
    x = np.asarray(x, F)
    e = np.exp(-np.abs(x)).astype(F)
    sp = (np.maximum(x, F(0)) + np.log1p(e).astype(F)).astype(F)
    sg = (np.where(x >= 0, F(1), e).astype(F) / (F(1) + e).astype(F)).astype(F)
    return sp, sg


def restate_f32(case, biased, remove_hits, order="shipped", defect=None):
    """the kernel's arithmetic in float32 NumPy: scores as rounded multiply-adds, the loss phase of csrc/bpr_fused.hip operation by
    operation, dU / d b_u per user and dV / d b_i per item as float32 sums.  order "shipped": the wave butterflies, the W wave sums
    in turn, the G group partials in turn (the other sums sequential); "seq": every sum of the loss phase with one accumulator, in
    sample resp. interaction order (another order of the same terms).  `defect`: one of DEFECTS seeded into the loss phase.
    Returns a namespace with the eight OUTPUTS and sample_scores, the [U, S] float32 scores of the samples."""
    S, nu, d, ni = case.S, case.n_users, case.d, case.n_items
    U, V = case.U.astype(F), case.V.astype(F)
    W = sample_waves(S)
    G = 4 // W
    pos = case.values > 0
    slot = np.cumsum(pos) - 1
    loss, pred = np.zeros(int(pos.sum()), F), np.zeros(case.x_item.size, F)
    coef_p, coef_s, samp = np.zeros(case.x_item.size, F), np.zeros((nu, S), F), np.zeros((nu, S), F)
    dU, dV, d_ub, d_ib = np.zeros((nu, d), F), np.zeros((ni, d), F), np.zeros(nu, F), np.zeros(ni, F)
    pair_u, pair_i, pair_g = [], [], []
    for u in range(nu):
        idx = np.arange(case.indptr[u], case.indptr[u + 1])
        items = np.concatenate([case.samples[u], case.x_item[idx]]).astype(np.int64)
        y = _sum32((V[items] * U[u][None, :]).T, "seq")
        if biased:
            y = ((y + case.ub[u]).astype(F) + case.ib[items]).astype(F)
        ys, yp = y[:S], y[S:]
        pred[idx] = yp
        samp[u] = ys
        kept = np.ones(S, bool)
        if remove_hits and defect != "hit_kept":
            kept = ~np.isin(case.samples[u], case.x_item[idx[pos[idx]]])
        inv_s = F(F(1) / F(S))
        if defect == "kept_divisor" and kept.any():
            inv_s = F(F(1) / F(kept.sum()))
        groups = [[] for _ in range(G)]                           # the sigma rows of each group's interactions, in interaction order
        for k in range(idx.size):
            if not pos[idx[k]] and defect != "nonpositive_counted":
                continue
            x = (ys - yp[k]).astype(F)
            sp, sg = cell_f32(-x if defect == "sigma_sign" else x)
            if defect == "sigma_sign":
                sp = cell_f32(x)[0]
            sp, sg = np.where(kept, sp, F(0)).astype(F), np.where(kept, sg, F(0)).astype(F)
            if order == "shipped":
                tp = _sum32([_butterfly64(sp[64 * w:64 * w + 64]) for w in range((S + 63) // 64)], "seq")
                tg = _sum32([_butterfly64(sg[64 * w:64 * w + 64]) for w in range((S + 63) // 64)], "seq")
            else:
                tp, tg = _sum32(sp, "seq"), _sum32(sg, "seq")
            if pos[idx[k]]:
                loss[slot[idx[k]]] = F(tp * inv_s)
            coef_p[idx[k]] = -F(tg * inv_s)
            groups[k % G if order == "shipped" else 0].append(sg)
        if defect == "group_dropped" and G > 1:
            groups = groups[:-1]
        parts = [_sum32(np.stack(g), "seq") if g else np.zeros(S, F) for g in groups]
        coef_s[u] = (_sum32(np.stack(parts), "seq") * inv_s).astype(F)
        coef = np.concatenate([coef_s[u], coef_p[idx]])
        if idx.size:
            dU[u] = _sum32(coef[:, None] * V[items], 8)
            d_ub[u] = _sum32(coef, "seq")
        pair_u += [u] * items.size
        pair_i += list(items)
        pair_g += list(coef)
    pair_u, pair_i, pair_g = np.array(pair_u), np.array(pair_i), np.array(pair_g, F)
    live = pair_g != 0                                            # (a term of exactly 0 changes no float32 sum)
    pair_u, pair_i, pair_g = pair_u[live], pair_i[live], pair_g[live]
    for i in np.unique(pair_i):
        k = np.flatnonzero(pair_i == i)
        dV[i] = _sum32(pair_g[k][:, None] * U[pair_u[k]], "seq")
        d_ib[i] = _sum32(pair_g[k], "seq")
    return SimpleNamespace(loss=loss, pred_serial=pred, coef_pairs=coef_p, coef_samples=coef_s, dU=dU, dV=dV, d_ub=d_ub, d_ib=d_ib,
                           sample_scores=samp)


def ratios(got, ref, biased):
    """{output: largest |got - reference| / bar}; a bar of 0 asks for equality (ratio 0 when equal, inf otherwise)"""
    out = {}
    for name in OUTPUTS:
        if name in ("d_ub", "d_ib") and not biased:
            continue
        g, w, b = f64(getattr(got, name)).reshape(-1), f64(getattr(ref, name)).reshape(-1), f64(getattr(ref, "b_" + name)).reshape(-1)
        assert g.shape == w.shape, name
        if not np.isfinite(g).all():
            out[name] = float("inf")
            continue
        err = np.abs(g - w)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[name] = float(np.where(err == 0, 0.0, err / b).max()) if g.size else 0.0
    return out
