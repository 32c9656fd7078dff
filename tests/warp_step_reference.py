"""Float64 reference, error bars, inputs and a float32 restatement for the one-pass WARP step (csrc/warp_fused.hip,
trec_warp_fused_step, ops.warp_fused_step).  NumPy / SciPy only, nothing of the code under test.
tests/test_warp_step_reference_host.py holds the reference to central differences and the bars to the restatement on the CPU (and
shows which seeded defects fall outside); tests/test_gpu_warp_fused.py holds the kernel to the reference.

The step.  Scores of the interactions and of the [U, S] samples (pair_reference.ref_pair_scores, dot), the WARP loss on them with
upstream gradient 1 (warp_reference.ref_warp: loss, first, d_pred = coef_pairs, d_samp = coef_samples), the gradients of the tables
and biases through pair_reference.ref_pair_grads fed with those coefficients.  The dispatch of the kernel is the sampled-softmax
step's: its mirror (instantiation, lds_bytes, GPU_CASES, UNCOVERED) is imported from tests/softmax_step_reference.py and only read.

Bars, as tests/test_gpu_warp_loss.py::float64_step builds them; nothing is tuned:
* pred_serial        pair_reference.score_bar =: delta (per pair).
* loss               warp_reference's own bar plus L_p (delta_p + delta_f) (1 + 8 u): the loss phase is handed float32 scores off by
                     at most delta, and where the float32 scores decide f_p as the float64 ones do (below), N_p and L_p are the
                     reference's and loss_p = L_p v_f moves by L_p times the error of v_f.
* coef_pairs, coef_samples   warp_reference's own bars: they are functions of L alone.
* dU, dV, d b_u, d b_i   pair_reference.grad_bars for the sums, plus the coefficients' bars carried through |d score / d entry|
                     (|v_c| resp. |u_c|; biases: 1).
An entry whose terms are all 0 has a bar of 0: it must be an exact 0.

Two families.
* dyadic   tables and biases multiples of 1/8: every score, and every v = (1 - y_p) + y_s, is exact in float32 in any order
           (scores_exact asserts the premise), so delta = 0, pred_serial is held bit for bit, and ``first`` and every zero pattern
           must equal the reference EVERYWHERE, positives with v == 0 exactly included.  The ``near`` band of warp_reference is a
           statement about ROUNDED v; it does not apply when v is exact and is not consulted for this family.
* real     a positive is AMBIGUOUS if a kept sample at or before the reference's f_p (every kept sample when f_p = -1) has
           |v| <= delta_p + delta_s + 2^-23 (1 + |y_p| + |y_s|): then float32 scores might pick another first violator.  This is a
           condition on the data, not a tolerance: the seeds are chosen so that NO positive of any case is ambiguous (ref.ambiguous
           is empty; the host test asserts it), so the GPU test compares every output of every user.

Planted users (warp_case): their items are reserved ones with zero rows, so their scores are b_u + b_i with b_u a multiple of 1/8 --
exact in both families and what the plants mean in the runs WITH biases (without biases every planted score is 0, every v is 1 and
every positive stops at its first kept sample: still a case, just not the planted one).  The strictness plant (v_0 == 0 exactly) is
by construction ambiguous in the sense above, so the real-valued family moves that positive half a unit up (v_0 = -0.5, f = 1 all
the same) and only the dyadic family holds v_0 == 0."""
import functools
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

import warp_reference as W
from pair_reference import MODE_DOT, U32, f64, grad_bars, ref_pair_grads, ref_pair_scores, score_bar
from softmax_step_reference import ALL_INSTANTIATIONS, GPU_CASES, UNCOVERED, instantiation, lds_bytes, rows_capacity  # noqa: F401

F = np.float32

# ------------------------------------------------------------------------------------------------ inputs
(U_NONE, U_NONPOS, U_ONE, U_LONG, U_PLAIN, U_PLAIN2, U_ABOVE, U_BELOW, U_STRICT, U_LAST, U_B63, U_B64, U_B127, U_B128, U_B191, U_B192,
 U_TWO, U_DUP, U_HIT_BEFORE, U_ONLY_HIT, U_ALLHITS, U_NONPOS_ITEM, U_HIT63) = range(23)
N_USERS = 23
BOUNDARY = {U_B63: 63, U_B64: 64, U_B127: 127, U_B128: 128, U_B191: 191, U_B192: 192}
N_REGULAR = 6                                                    # users 0 .. 5 live on the regular items, the others on reserved ones
# reserved items behind the regular ones: zero rows, the score is b_u + the level
R_LOW, R_HIGH, R_MID, R_POS0, R_POS1, R_POS2, R_ABOVE, R_BELOW, R_NEG = range(9)
LEVELS = [-64.0, 64.0, 0.0, 0.0, 1.0, 0.5, 200.0, -200.0, 64.0]
SEEDS = {(7, 121, 256): 1}                                       # spec -> seed of the real-valued case, where 0 gives an ambiguous positive


def warp_case(S, longest, d, exact=False, seed=0):
    """23 users, rows cut to `longest`.  Regular items: 0 no interaction; 1 interactions of value <= 0 only; 2 one positive; 3 the
    longest row (values <= 0 mixed in where it has five or more) with a duplicated sample; 4, 5 nothing planted (5: mixed signs).
    Reserved items (y = b_u + level; LOW -64, HIGH 64, MID 0, the positives POS0 0, POS1 1 (real family: 1.5), POS2 0.5, ABOVE 200,
    BELOW -200, NEG 64 with a value of -1); every sample not named is LOW, which no positive but BELOW is violated by:
      ABOVE       positive ABOVE, samples HIGH: no violator, f = -1            BELOW   positive BELOW: f = 0
      STRICT      positive POS1, slot 0 MID (v = 0 exactly, dyadic family; -0.5 real), slot 1 HIGH: f = 1
      LAST        positive POS0, HIGH at slot S - 1; with S = 255 and n_items = 500 N_p = 255 > 499 / 2: L = 0 with f >= 0 (late)
      B63 .. B192 positive POS0, HIGH at that slot (f = -1 where S does not reach it): the word boundaries of the kept mask
      TWO         positives POS0 and POS2, HIGH at slot min(2, S - 1): two terms on one slot
      DUP         positive POS0, HIGH at slots min(1, S - 1) and min(2, S - 1): only the first is stopped at
      HIT_BEFORE  positive POS0, slot 0 POS0 itself (v = 1: a violator and a hit), slot 1 HIGH: f = 0, with hits removed f = 1, N = 1
      ONLY_HIT    positive POS0, slot min(2, S - 1) POS0: the only violator is a hit, f = -1 with hits removed
      ALLHITS     positives POS0, POS2, every sample one of the two
      NONPOS_ITEM positive POS0 and NEG (value -1), slot 0 NEG: a violator and no hit, f = 0 either way
      HIT63       positive POS0, slots 63 and 64 POS0, slot 65 HIGH: f = 63, with hits removed f = 65 and N = 64
    n_items = 500 in the S = 255 case (so that the late row exists), 1,109 otherwise (L > 0 for every N <= 256)."""
    rng = np.random.default_rng(9001 * S + 131 * longest + 17 * d + (5 if exact else 0) + seed)
    n_reg = 491 if S == 255 else 1100
    n_items = n_reg + len(LEVELS)
    res = lambda k: n_reg + k
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
    V[n_reg:] = 0.0
    ib[n_reg:] = np.array(LEVELS, F)
    if not exact:
        ib[res(R_POS1)] = 1.5
    ub[N_REGULAR:] = ((np.arange(N_REGULAR, N_USERS) % 5) - 2) / 8.0
    rows = {u: [] for u in range(N_USERS)}
    want = {U_NONPOS: 2, U_ONE: 1, U_LONG: longest, U_PLAIN: 4, U_PLAIN2: 6}
    for u, n in want.items():
        n = min(n, longest)
        cols = np.sort(rng.choice(n_reg, size=n, replace=False))
        v = rng.integers(1, 13, size=n) / 4.0
        if u == U_NONPOS:
            v[:] = [-1.0, 0.0][:n]
        elif u == U_PLAIN2:
            v[:] = [1.0, -1.0, 0.0, 2.0, 0.5, 1.0][:n]
        elif u == U_LONG and n >= 5:
            v[1], v[n - 2] = -1.0, 0.0
        rows[u] = list(zip(cols.tolist(), v.tolist()))
    samples = rng.integers(0, n_reg, size=(N_USERS, S)).astype(np.int32)
    if S >= 2:
        samples[U_LONG, 1] = samples[U_LONG, 0]
    samples[N_REGULAR:] = res(R_LOW)

    def plant(u, inter, at):
        rows[u] = [(res(k), val) for k, val in inter[:max(longest, 1)]]
        for slot, k in at:
            if 0 <= slot < S:
                samples[u, slot] = res(k)
    plant(U_ABOVE, [(R_ABOVE, 1.0)], [(s, R_HIGH) for s in range(S)])
    plant(U_BELOW, [(R_BELOW, 1.0)], [])
    plant(U_STRICT, [(R_POS1, 1.0)], [(1, R_HIGH), (0, R_MID)])
    plant(U_LAST, [(R_POS0, 1.0)], [(S - 1, R_HIGH)])
    for u, k in BOUNDARY.items():
        plant(u, [(R_POS0, 1.0)], [(k, R_HIGH)])
    plant(U_TWO, [(R_POS0, 1.0), (R_POS2, 2.0)], [(min(2, S - 1), R_HIGH)])
    plant(U_DUP, [(R_POS0, 1.0)], [(min(1, S - 1), R_HIGH), (min(2, S - 1), R_HIGH)])
    plant(U_HIT_BEFORE, [(R_POS0, 1.0)], [(1, R_HIGH), (0, R_POS0)])
    plant(U_ONLY_HIT, [(R_POS0, 1.0)], [(min(2, S - 1), R_POS0)])
    plant(U_ALLHITS, [(R_POS0, 1.0), (R_POS2, 1.0)], [(s, R_POS0 if (s % 2 == 0 or longest < 2) else R_POS2) for s in range(S)])
    plant(U_NONPOS_ITEM, [(R_POS0, 1.0), (R_NEG, -1.0)], [(0, R_NEG if longest >= 2 else R_HIGH)])
    plant(U_HIT63, [(R_POS0, 1.0)], [(65, R_HIGH), (63, R_POS0), (64, R_POS0)])
    r_idx = [u for u in range(N_USERS) for _ in rows[u]]
    c_idx = [c for u in range(N_USERS) for c, _ in rows[u]]
    vals = [v for u in range(N_USERS) for _, v in rows[u]]
    m = sp.csr_matrix((np.array(vals, F), (np.array(r_idx), np.array(c_idx))), shape=(N_USERS, n_items))
    assert m.nnz == len(vals) and m.has_sorted_indices
    indptr, x_item, values = m.indptr.astype(np.int64), m.indices.astype(np.int32).copy(), m.data.astype(F)
    return SimpleNamespace(U=U, V=V, ub=ub, ib=ib, matrix=m, indptr=indptr, x_item=x_item, values=values, samples=samples, S=S, d=d,
                           n_users=N_USERS, n_items=n_items, n_reg=n_reg, longest=longest, max_pos=int(np.diff(indptr).max()),
                           exact=exact)


def scores_exact(case):
    """the premise of delta = 0: tables and biases multiples of 1/8, every sum of |terms| of a score below 2^17 (a multiple of 2^-6
    with fewer than 24 bits: exact in float32 in any order), and so is v = (1 - y_p) + y_s"""
    for a in (case.U, case.V, case.ub, case.ib):
        t = f64(a) * 8.0
        if not (t == np.round(t)).all():
            return False
    big = np.abs(f64(case.U)).max(initial=0) * np.abs(f64(case.V)).sum(1).max() + np.abs(case.ub).max() + np.abs(case.ib).max()
    return bool(big < 2.0 ** 16)


def pair_lists(case):
    """(xu, xi) of the interactions followed by the sampled pairs"""
    S, nu = case.S, case.n_users
    xu = np.concatenate([np.repeat(np.arange(nu), np.diff(case.indptr)), np.repeat(np.arange(nu), S)])
    xi = np.concatenate([case.x_item.astype(np.int64), case.samples.reshape(-1).astype(np.int64)])
    return xu, xi


def expected_first(case, remove_hits):
    """{user: [f of its interactions]} for the planted users, in the runs WITH biases, from the plants' definitions alone"""
    S, two = case.S, case.longest >= 2
    at = lambda k: k if k < S else -1
    out = {U_ABOVE: [-1], U_BELOW: [0], U_STRICT: [at(1)], U_LAST: [S - 1], U_TWO: [min(2, S - 1)] * (2 if two else 1),
           U_DUP: [min(1, S - 1)]}
    for u, k in BOUNDARY.items():
        out[u] = [at(k)]
    out[U_HIT_BEFORE] = [at(1)] if remove_hits else [0]
    out[U_ONLY_HIT] = [-1] if remove_hits else [min(2, S - 1)]
    out[U_ALLHITS] = [-1 if remove_hits else 0] * (2 if two else 1)
    out[U_NONPOS_ITEM] = [0, -1] if two else [0]                  # (columns are sorted: POS0 before NEG; NEG is no positive)
    out[U_HIT63] = [at(65) if remove_hits else at(63)]
    return out


# ------------------------------------------------------------------------------------------------ reference
def ref_step(case, biased, remove_hits):
    """the float64 step and its bars: a namespace with loss, pred_serial, first, coef_pairs, coef_samples, dU, dV, d_ub, d_ib and
    b_<name> for each but first; warp (ref_warp's answer); ambiguous (interaction indices, see the module docstring)"""
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
    w = W.ref_warp(case.indptr, case.values, yp, ys, np.ones(int(pos.sum())), case.n_items, case.samples, case.x_item, remove_hits)
    delta_p, delta_s = delta[:nnz], delta[nnz:].reshape(nu, S)
    at_first, ambiguous = np.zeros(nnz), []
    for p in np.flatnonzero(pos):
        u, f = xu[p], w.first[p]
        upto = S if f < 0 else f + 1
        kept = W.kept_mask(case.indptr, case.values, case.x_item, case.samples, u, remove_hits)
        kept = np.ones(S, bool)[:upto] if kept is None else kept[:upto]
        v = (1.0 - yp[p]) + ys[u, :upto]
        band = delta_p[p] + delta_s[u, :upto] + W.NEAR * (1.0 + abs(yp[p]) + np.abs(ys[u, :upto]))
        if not exact and ((np.abs(v) <= band) & kept).any():
            ambiguous.append(int(p))
        if f >= 0:
            at_first[p] = delta_p[p] + delta_s[u, f]
    r = SimpleNamespace(warp=w, scores=sc, ambiguous=ambiguous, first=w.first, pred_serial=yp, b_pred_serial=delta_p)
    r.loss, r.b_loss = w.loss, w.bar_loss + (w.weight * at_first * (1.0 + 8.0 * U32))[pos]
    r.coef_pairs, r.b_coef_pairs = w.d_pred, w.bar_d_pred
    r.coef_samples, r.b_coef_samples = w.d_samp, w.bar_d_samp
    g = np.concatenate([w.d_pred, w.d_samp.reshape(-1)])
    b_g = np.concatenate([w.bar_d_pred, w.bar_d_samp.reshape(-1)])
    pg = ref_pair_grads(case.U, case.V, xu, xi, g, MODE_DOT)
    inh = ref_pair_grads(np.abs(f64(case.U)), np.abs(f64(case.V)), xu, xi, b_g, MODE_DOT)       # b_g through |d score / d entry|
    bU, bV, bub, bib = grad_bars(pg, d)
    r.dU, r.dV, r.d_ub, r.d_ib = pg.dU, pg.dV, pg.dub, pg.dib
    r.b_dU, r.b_dV, r.b_d_ub, r.b_d_ib = bU + inh.dU, bV + inh.dV, bub + inh.dub, bib + inh.dib
    return r


@functools.lru_cache(maxsize=None)
def cached_case(spec, exact):
    return warp_case(*spec, exact=exact, seed=0 if exact else SEEDS.get(spec, 0))


@functools.lru_cache(maxsize=None)
def cached_ref(spec, exact, biased, remove_hits):
    """computed once and shared by the host and the GPU tests; nobody writes into it"""
    return ref_step(cached_case(spec, exact), biased, remove_hits)


OUTPUTS = ("pred_serial", "loss", "coef_pairs", "coef_samples", "dU", "d_ub", "dV", "d_ib")


def loss_sum_fixed_weight(case, biased, ref, U=None, V=None, ub=None, ib=None):
    """sum_p L_p v_{f_p} at perturbed tables with f and L HELD at the reference's: what the gradients are the derivative of (L is
    piecewise constant and not differentiated, and away from a discontinuity f does not move)"""
    c = SimpleNamespace(**vars(case))
    c.U, c.V = (case.U if U is None else U), (case.V if V is None else V)
    c.ub, c.ib = (case.ub if ub is None else ub), (case.ib if ib is None else ib)
    nnz = case.x_item.size
    xu, xi = pair_lists(c)
    sc = ref_pair_scores(c.U, c.V, xu, xi, MODE_DOT, c.ub if biased else None, c.ib if biased else None).scores
    yp, ys = sc[:nnz], sc[nnz:].reshape(case.n_users, case.S)
    total = 0.0
    for p in np.flatnonzero(ref.first >= 0):
        total += ref.warp.weight[p] * ((1.0 - yp[p]) + ys[xu[p], ref.first[p]])
    return total


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


# >= for >, N = f, n_items for n_items - 1, the last violator, a hit counted as a trial, coef_s spread over all kept violators, coef_s
# added in reverse interaction order, no -L on the positive
DEFECTS = ("ge", "n_is_f", "n_items", "last", "hit_is_trial", "spread", "reverse", "no_minus")
# "reverse" cannot show at upstream gradient 1: N_p is a function of f_p and the user's mask, so every term of a slot is the same L
# and a sum of equal float32 terms has one value in any order (the host test asserts exactly that)
INVISIBLE_DEFECTS = ("reverse",)


def restate_f32(case, biased, remove_hits, order="seq", defect=None):
    """the kernel's arithmetic in float32 NumPy: scores as rounded multiply-adds in `order`, the loss phase of csrc/warp_fused.hip
    operation by operation, dU / d b_u per user and dV / d b_i per item as float32 sums.  `defect`: one of DEFECTS seeded into the
    loss phase.  Returns a namespace with `first`, the eight OUTPUTS and sample_scores, the [U, S] float32 scores of the samples."""
    S, nu, d, ni = case.S, case.n_users, case.d, case.n_items
    U, V = case.U.astype(F), case.V.astype(F)
    pos = case.values > 0
    slot = np.cumsum(pos) - 1
    top = ni if defect == "n_items" else ni - 1
    loss, pred = np.zeros(int(pos.sum()), F), np.zeros(case.x_item.size, F)
    first = np.full(case.x_item.size, -1, np.int64)
    coef_p, coef_s, samp = np.zeros(case.x_item.size, F), np.zeros((nu, S), F), np.zeros((nu, S), F)
    dU, dV, d_ub, d_ib = np.zeros((nu, d), F), np.zeros((ni, d), F), np.zeros(nu, F), np.zeros(ni, F)
    pair_u, pair_i, pair_g = [], [], []
    for u in range(nu):
        idx = np.arange(case.indptr[u], case.indptr[u + 1])
        items = np.concatenate([case.samples[u], case.x_item[idx]]).astype(np.int64)
        y = _sum32((V[items] * U[u][None, :]).T, order if order == "seq" else min(order, d))
        if biased:
            y = ((y + case.ub[u]).astype(F) + case.ib[items]).astype(F)
        ys, yp = y[:S], y[S:]
        pred[idx] = yp
        samp[u] = ys
        kept = np.ones(S, bool)
        if remove_hits:
            kept = ~np.isin(case.samples[u], case.x_item[idx[pos[idx]]])
        ckept = np.arange(1, S + 1) if defect == "hit_is_trial" else np.cumsum(kept)
        stops = []                                                # (f, L) in interaction order
        for k in np.flatnonzero(pos[idx]):
            v = (F(1.0) - yp[k]) + ys
            assert v.dtype == F
            viol = ((v >= 0) if defect == "ge" else (v > 0)) & kept
            if not viol.any():
                continue
            f = int(np.flatnonzero(viol)[-1 if defect == "last" else 0])
            n = int(ckept[f]) - (1 if defect == "n_is_f" else 0)
            r = top // n if n > 0 else 2 ** 31 - 1                # (a division by 0 gives anything; take the largest)
            L = np.log(F(r)).astype(F) if r > 1 else F(0)
            first[idx[k]] = f
            loss[slot[idx[k]]] = F(L * v[f])
            coef_p[idx[k]] = F(0) if defect == "no_minus" else -L
            stops.append((np.flatnonzero(viol) if defect == "spread" else [f], L))
        for f, L in (stops[::-1] if defect == "reverse" else stops):
            for s in f:
                coef_s[u, s] = F(coef_s[u, s] + L)
        coef = np.concatenate([coef_s[u], coef_p[idx]])
        if idx.size:
            dU[u] = _sum32(coef[:, None] * V[items], order)
            d_ub[u] = _sum32(coef, order)
        pair_u += [u] * items.size
        pair_i += list(items)
        pair_g += list(coef)
    pair_u, pair_i, pair_g = np.array(pair_u), np.array(pair_i), np.array(pair_g, F)
    live = pair_g != 0                                            # (a term of exactly 0 changes no float32 sum)
    pair_u, pair_i, pair_g = pair_u[live], pair_i[live], pair_g[live]
    for i in np.unique(pair_i):
        k = np.flatnonzero(pair_i == i)
        dV[i] = _sum32(pair_g[k][:, None] * U[pair_u[k]], order)
        d_ib[i] = _sum32(pair_g[k], order)
    return SimpleNamespace(loss=loss, pred_serial=pred, first=first, coef_pairs=coef_p, coef_samples=coef_s, dU=dU, dV=dV, d_ub=d_ub,
                           d_ib=d_ib, sample_scores=samp)


def ratios(got, ref, biased):
    """{output: largest |got - reference| / bar}; a bar of 0 asks for equality (ratio 0 when equal, inf otherwise); "first": 0 where it
    equals the reference's everywhere, inf otherwise"""
    out = {"first": 0.0 if np.array_equal(np.asarray(got.first, np.int64), ref.first) else float("inf")}
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
