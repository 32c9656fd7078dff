"""Float64 reference, error bars, a float32 restatement and inputs for the WARP kernels (csrc/loss_warp.hip).  NumPy only: no torch,
nothing of the code under test.  tests/test_warp_reference_host.py holds the reference to central differences and the bars to the
float32 restatement on the CPU; tests/test_gpu_warp_loss.py holds the kernels to the reference.

Definition (include/tensorrec_hip.h restates it).  y_p a positive's prediction, y_s the prediction of sample s of the same user, the
samples tried in table order, go_p the upstream gradient.
    v_s = (1 - y_p) + y_s;  s violates iff v_s > 0;  kept: every sample, or (remove_hits) those whose item is not the column of an
    interaction of the user with a value > 0;  f_p = the smallest kept s that violates (-1: none);  N_p = the kept samples with index
    <= f_p;  r_p = (n_items - 1) div N_p;  L_p = log(max(r_p, 1));  loss_p = L_p v_f;   d y_p = -go_p L_p,
    d y_us = sum_{p of u, f_p = s} go_p L_p   (L is piecewise constant and not differentiated).

Bars.  u = 2^-24, the unit roundoff of float32; the inputs are float32 numbers and exact.  They hold for a positive whose f_p the
float32 arithmetic decides as the float64 arithmetic does (see ``near`` below); N_p, r_p are then the same integers.
    v        two roundings, 1 - y_p and the sum:   dv = u |1 - y_p| (1 + u) + u |v|
    L        the library's logf, LIB = 4 units as in sampled_loss_reference;  (float) r_p is exact below 2^24, one rounding of r_p above,
             which moves log r_p by u:   dL = LIB u L  (+ u);   r_p <= 1 gives an exact 0
    loss     one multiply:   e = L dv + |v| dL + dv dL,   bar = e + u (|loss| + e) + TINY;   an exact 0 where L_p = 0 or f_p = -1
    d y_p    c_p = go_p L_p, one multiply:   bc = |go| dL + u |go| (L + dL) + TINY;   an exact 0 where go_p L_p = 0
    d y_us   n terms c_p added in interaction order, one rounding per term added:   sum bc + n u sum (|c_p| + bc)
Entries that must be exactly 0 (d pred of a non-positive interaction or of a positive without a violator, the d samp row of a user
without positives, every slot no positive stopped at) have a bar of 0.

``near``.  In float32 v_s is off by at most 2^-23 (1 + |y_p| + |y_s|), so the sign test can only differ from the float64 one for a
sample inside that band.  near[p] says that some kept sample at or before the reference's f_p (every kept sample when f_p = -1) lies
in it: only such a positive may be left out of a comparison, and only a d samp row that holds one.
"""
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

import sampled_loss_reference as SR
from sampled_loss_reference import U32, TINY, LIB, f64

F = np.float32
NEAR = 2.0 ** -23
MAX_LEFT_OUT = 0.005            # the share of a case's positives that may be left out as ``near``


def kept_mask(indptr, values, x_item, samples, u, remove_hits):
    """[S] bools: the samples of user u that are no hits; None without hit removal (every sample is kept)"""
    if not remove_hits:
        return None
    b, e = indptr[u], indptr[u + 1]
    cols = np.asarray(x_item[b:e])[np.asarray(values[b:e]) > 0]
    return ~np.isin(samples[u], cols)


def ref_warp(indptr, values, pred, samp, go, n_items, samples=None, x_item=None, remove_hits=False):
    """loss [P+], first / trials (int64) / weight [P], d_pred [P], d_samp [U, S] of sum_p go_p loss_p, their bars, near [P] and the
    number of (positive, kept sample) cells the scans looked at"""
    indptr, values, pred, samp, go = np.asarray(indptr), np.asarray(values), f64(pred), f64(samp), f64(go)
    n_users, S = samp.shape
    pos = values > 0
    slot = np.cumsum(pos) - 1
    n_pos = int(pos.sum())
    loss, bar_loss = np.zeros(n_pos), np.zeros(n_pos)
    first, trials = np.full(pred.size, -1, np.int64), np.zeros(pred.size, np.int64)
    weight, d_pred, bar_d_pred = np.zeros(pred.size), np.zeros(pred.size), np.zeros(pred.size)
    d_samp, bar_d_samp = np.zeros(samp.shape), np.zeros(samp.shape)
    near = np.zeros(pred.size, bool)
    scanned = 0
    for u in range(n_users):
        idx = np.arange(indptr[u], indptr[u + 1])
        idx = idx[pos[idx]]
        if not idx.size:
            continue
        kept = kept_mask(indptr, values, x_item, samples, u, remove_hits)
        kept = np.ones(S, bool) if kept is None else kept
        ckept = np.cumsum(kept)
        yp, ys, g = pred[idx], samp[u], go[slot[idx]]
        V = (1.0 - yp)[:, None] + ys[None, :]
        viol = (V > 0) & kept[None, :]
        has = viol.any(1)
        f = np.where(has, viol.argmax(1), -1)
        upto = np.where(has, f + 1, S)
        looked = (np.arange(S)[None, :] < upto[:, None]) & kept[None, :]
        band = NEAR * (1.0 + np.abs(yp)[:, None] + np.abs(ys)[None, :])
        near[idx] = ((np.abs(V) <= band) & looked).any(1)
        scanned += int(looked.sum())
        fc = np.maximum(f, 0)
        N = np.where(has, ckept[fc], 1)
        r = (int(n_items) - 1) // np.maximum(N, 1)
        L = np.where(has, np.log(np.maximum(r, 1).astype(np.float64)), 0.0)
        vf = np.where(has, V[np.arange(idx.size), fc], 0.0)
        lo = L * vf
        dv = U32 * np.abs(1.0 - yp) * (1.0 + U32) + U32 * np.abs(vf)
        dL = np.where(L > 0, LIB * U32 * L + np.where(r >= 2 ** 24, U32, 0.0), 0.0)
        e = L * dv + np.abs(vf) * dL + dv * dL
        first[idx], trials[idx], weight[idx] = f, np.where(has, N, 0), L
        loss[slot[idx]] = lo
        bar_loss[slot[idx]] = np.where(L > 0, e + U32 * (np.abs(lo) + e) + TINY, 0.0)
        c = g * L
        bc = np.where(c != 0, np.abs(g) * dL + U32 * np.abs(g) * (L + dL) + TINY, 0.0)
        d_pred[idx] = -c
        bar_d_pred[idx] = bc
        live = has
        np.add.at(d_samp[u], f[live], c[live])
        terms, mass = np.zeros(S), np.zeros(S)
        np.add.at(terms, f[live], 1.0)
        np.add.at(mass, f[live], (np.abs(c) + bc)[live])
        np.add.at(bar_d_samp[u], f[live], bc[live])
        bar_d_samp[u] += terms * U32 * mass
    return SimpleNamespace(loss=loss, first=first, trials=trials, weight=weight, d_pred=d_pred, d_samp=d_samp, bar_loss=bar_loss,
                           bar_d_pred=bar_d_pred, bar_d_samp=bar_d_samp, near=near, scanned=scanned)


def bars(ref):
    """(bar loss, bar d pred, bar d samp)"""
    return ref.bar_loss, ref.bar_d_pred, ref.bar_d_samp


def comparable(case, ref):
    """(positives [P+] to compare, interactions [P] to compare, d samp rows [U] to compare, the share of positives left out): a
    positive is left out only when it is ``near``, a row only when it holds such a positive"""
    pos = case.values > 0
    keep_p = ~ref.near
    rows = np.ones(case.n_users, bool)
    for u in range(case.n_users):
        rows[u] = not ref.near[case.indptr[u]:case.indptr[u + 1]].any()
    left_out = float(ref.near[pos].sum()) / max(int(pos.sum()), 1)
    return keep_p[pos], keep_p, rows, left_out


# ------------------------------------------------------------------------------------------------ the kernels' arithmetic in float32
DEFECTS = ["ge", "n_is_f", "n_items", "last", "hit_is_trial", "spread"]


def f32_warp(case, remove_hits=False, defect=None):
    """csrc/loss_warp.hip, every operation in float32: (loss, first, d_pred, d_samp).  ``defect``: one of DEFECTS --
    >= in place of >, N = f in place of f + 1, n_items in place of n_items - 1, the LAST violator, a hit counted as a trial, d samp
    spread over all kept violators."""
    pos = case.values > 0
    slot = np.cumsum(pos) - 1
    S = case.S
    loss, d_pred, d_samp = np.zeros(int(pos.sum()), F), np.zeros(case.pred.size, F), np.zeros(case.samp.shape, F)
    first = np.full(case.pred.size, -1, np.int64)
    pred, samp, go = case.pred.astype(F), case.samp.astype(F), case.go.astype(F)
    top = case.n_items if defect == "n_items" else case.n_items - 1
    for u in range(case.n_users):
        idx = np.arange(case.indptr[u], case.indptr[u + 1])
        idx = idx[pos[idx]]
        if not idx.size:
            continue
        kept = kept_mask(case.indptr, case.values, getattr(case, "x_item", None), getattr(case, "samples", None), u, remove_hits)
        kept = np.ones(S, bool) if kept is None else kept
        ckept = np.cumsum(kept) if defect != "hit_is_trial" else np.arange(1, S + 1)
        yp, ys, g = pred[idx], samp[u], go[slot[idx]]
        V = (F(1.0) - yp)[:, None] + ys[None, :]
        assert V.dtype == F
        viol = ((V >= 0) if defect == "ge" else (V > 0)) & kept[None, :]
        has = viol.any(1)
        f = (S - 1 - viol[:, ::-1].argmax(1)) if defect == "last" else viol.argmax(1)
        f = np.where(has, f, -1)
        fc = np.maximum(f, 0)
        N = ckept[fc] - (1 if defect == "n_is_f" else 0)
        r = np.where(N > 0, top // np.maximum(N, 1), 2 ** 31 - 1)            # (a division by 0 gives anything; take the largest)
        L = np.where(has & (r > 1), np.log(np.maximum(r, 1).astype(F)), F(0)).astype(F)
        vf = np.where(has, V[np.arange(idx.size), fc], F(0)).astype(F)
        first[idx] = f
        loss[slot[idx]] = L * vf
        c = (g * L).astype(F)
        d_pred[idx] = np.where(has, -c, F(0))
        for j in np.flatnonzero(has):                                         # interaction order, one float32 addition per term
            if defect == "spread":
                d_samp[u, viol[j]] += c[j]
            else:
                d_samp[u, f[j]] = F(d_samp[u, f[j]] + c[j])
    return loss, first, d_pred, d_samp


# ------------------------------------------------------------------------------------------------ inputs
SAMPLE_COUNTS = SR.SAMPLE_COUNTS                        # [1, 63, 64, 65, 256, 257, 300]: both forms below 257, the workgroup form above
SAMPLE_COUNTS_MANY = SR.SAMPLE_COUNTS_MANY              # [40, 300]: the multi-pass rows (1,025 and 2,600 positives) in both forms
N_ITEMS = SR.N_ITEMS                                    # 2,700
U_ALL_HITS, U_ONLY_HIT, U_HIT_FIRST, U_NON_POSITIVE, U_LONG = 4, 7, 10, 5, 2      # users of hits_case (SR.POSITIVES: 2600, 1, 3, 4, 65)


def signed(go):
    """non-constant and signed: every third entry changes sign (SR.loss_case already zeroes every seventh)"""
    return (go * np.where(np.arange(go.size) % 3 == 1, -1.0, 1.0)).astype(F)


def real_case(S):
    """the real-valued family: SR.loss_case -- N(0, 1) predictions, users with 0 / non-positives only / 1 / 64 / 65 / 1,025 / 2,600
    positives, equal samples (user 5), a positive 100 above and one 100 below every sample (user 8) -- with a signed go"""
    case = SR.loss_case(S)
    case.go = signed(case.go)
    return case


def dyadic(x):
    return np.clip(np.round(np.asarray(x, np.float64) * 64.0) / 64.0, -4.0, 4.0).astype(F)


def dyadic_case(S):
    """the dyadic family: the same geometry, every prediction a multiple of 2^-6 in [-4, 4]: v is exact in float32 and in float64, so
    ``first`` is unambiguous"""
    case = real_case(S)
    case.pred, case.samp = dyadic(case.pred), dyadic(case.samp)
    return case


def values_exact(case):
    return bool((np.abs(case.pred) <= 4).all() and (np.abs(case.samp) <= 4).all() and (case.pred * 64 == np.round(case.pred * 64)).all()
                and (case.samp * 64 == np.round(case.samp * 64)).all())


PLANTED = [(S, N_ITEMS, sorted(k for k in {0, 63, 64, 255, 256, S - 1} if k < S)) for S in SAMPLE_COUNTS] + [
    (2000, N_ITEMS, [0, 1348, 1349, 1999]),             # N = 1349: r = 2, L = log 2;  N >= 1350: r = 1, L = 0 with a violator
    (64, 50, [0, 48, 49, 63]),                          # N = 49: r = 1;  N = 50, 64: n_items - 1 < N, r = 0 -- in the wave form
    (300, 50, [0, 48, 49, 60, 299]),                    # the same in the workgroup form
    (16384, N_ITEMS, [0, 1348, 16383])]                 # the largest S: 64 KB of samples in LDS, more with the kept mask


def planted_case(S, n_items, firsts, seed=0):
    """Planted rows, one user each, two positives (and a negative and an explicit-zero interaction, predictions 0) per user:
      first k      samples -4 before slot k, 2 at k, 3 behind: positives 1.0 and 1.5 stop at k with v = 2 and 1.5
      none         samples -4, positives 1.0 and 0.0: no violator
      zero / eps   samples 0.5, 0.5 + 2^-20, 2, ...: positive 1.5 sees v = 0 (no violation) then 2^-20 (first = 1), positive 1.0 stops at 0
      equal        samples all 0.5: positive 1.0 stops at the lowest index, positive 2.0 has no violator
      far          dyadic samples in [-4, 4]: a positive at 100 (no violator) and one at -100 (stops at 0)
    in front of them a user without interactions and one with non-positive interactions only.  Every v is exact in float32.
    ``expected``: interaction index -> first.  ``samples``: ids for a run with hit removal -- an item the user has no interaction with
    everywhere, except that a "first k" row, k >= 1, holds its first positive's item at slot k - 1 (no violator there): the hit changes
    no ``first`` and takes one trial off N."""
    rng = np.random.default_rng(977 * S + n_items + seed)
    specs = [("empty", None, np.full(S, 3.0)), ("non-positive", [], np.full(S, 3.0))]
    for k in firsts:
        row = np.full(S, -4.0)
        row[k] = 2.0
        row[k + 1:] = 3.0
        specs.append(("first %d" % k, [(1.0, k), (1.5, k)], row))
    specs.append(("none", [(1.0, -1), (0.0, -1)], np.full(S, -4.0)))
    row = np.full(S, 2.0)
    row[0] = 0.5
    if S > 1:
        row[1] = 0.5 + 2.0 ** -20
    specs.append(("zero / eps", [(1.5, 1 if S > 1 else -1), (1.0, 0)], row))
    specs.append(("equal", [(1.0, 0), (2.0, -1)], np.full(S, 0.5)))
    specs.append(("far", [(100.0, -1), (-100.0, 0)], dyadic(rng.uniform(-4, 4, S)).astype(np.float64)))
    indptr, cols, vals, pred, expected = [0], [], [], [], {}
    for name, positives, row in specs:
        if positives is not None:
            m = len(positives) + 2
            c = np.sort(rng.choice(n_items, size=m, replace=False))
            order = list(positives[:1]) + [None] + list(positives[1:]) + [None]           # a positive first (if any), non-positives between
            for j, p in enumerate(order):
                cols.append(int(c[j]))
                if p is None:
                    vals.append(-1.0 if j == 1 else 0.0)
                    pred.append(0.0)
                else:
                    expected[len(pred)] = p[1]
                    vals.append(1.0 + 0.25 * j)
                    pred.append(p[0])
        indptr.append(len(cols))
    nu = len(specs)
    indptr = np.array(indptr, np.int64)
    m = sp.csr_matrix((np.array(vals, F), np.array(cols, np.int32), indptr), shape=(nu, n_items))
    assert m.nnz == len(vals)
    values = m.data.astype(F)
    n_pos = int((values > 0).sum())
    go = rng.uniform(0.5, 1.5, n_pos).astype(F)
    go[1::2] *= F(-1.0)
    samp = np.stack([s[2] for s in specs]).astype(F)
    assert (samp.astype(np.float64) == np.stack([s[2] for s in specs])).all()
    x_item = m.indices.astype(np.int32)
    ids = np.zeros((nu, S), np.int32)
    for u, (name, _, _) in enumerate(specs):
        own = set(x_item[indptr[u]:indptr[u + 1]].tolist())
        ids[u] = next(i for i in range(n_items) if i not in own)
        if name.startswith("first ") and int(name[6:]) >= 1:
            ids[u, int(name[6:]) - 1] = x_item[indptr[u]]
    return SimpleNamespace(matrix=m, indptr=indptr, values=values, pred=np.array(pred, F), samp=samp, go=go, n_users=nu,
                           n_items=n_items, S=S, expected=expected, names=[s[0] for s in specs], samples=ids, x_item=x_item)


def hits_case(S, seed=0):
    """dyadic_case with a sample-id table: three in ten ids are columns of the user's own interactions (positive or not), the others
    any item, drawn with replacement (so ids repeat).  Planted, every v exact:
      user 4 (2,600 positives)   every sample is one of its positives: no trial at all
      user 7 (1 positive)        the only violator (slot min(2, S - 1)) is the positive itself: first = -1, where the plain loss stops there
      user 10 (3 positives)      slot 0 violates and is a hit, slot 1 violates and is none: first = 1 with N = 1
      user 5 (4 positives)       slot 0 violates and is the column of an interaction of value <= 0: no hit, first = 0; slots 1, 2 repeat
                                 one positive's id, slot 3 repeats slot 0's
      user 2 (65 positives, a row the wave form searches in memory)  as user 10, for its first five positives"""
    rng = np.random.default_rng(8161 * S + seed)
    case = dyadic_case(S)
    indptr, values = case.indptr, case.values
    x_item = case.matrix.indices.astype(np.int32)
    ids = rng.integers(0, case.n_items, size=(case.n_users, S))
    for u in range(case.n_users):
        own = x_item[indptr[u]:indptr[u + 1]]
        if own.size:
            take = rng.random(S) < 0.3
            ids[u, take] = rng.choice(own, size=int(take.sum()))

    def cols(u, positive):
        idx = np.arange(indptr[u], indptr[u + 1])
        return idx[(values[idx] > 0) == positive]

    def stranger(u):                                                   # an item the user has no interaction with
        own = set(x_item[indptr[u]:indptr[u + 1]].tolist())
        return next(i for i in range(case.n_items) if i not in own)

    ids[U_ALL_HITS] = x_item[cols(U_ALL_HITS, True)[:S]]
    p7 = cols(U_ONLY_HIT, True)
    k7 = min(2, S - 1)
    case.pred[p7] = 1.0
    case.samp[U_ONLY_HIT] = -4.0
    case.samp[U_ONLY_HIT, k7] = 3.0
    ids[U_ONLY_HIT] = stranger(U_ONLY_HIT)
    ids[U_ONLY_HIT, k7] = x_item[p7[0]]
    for u, n_planted in ((U_HIT_FIRST, 3), (U_LONG, 5)):
        p = cols(u, True)[:n_planted]
        case.pred[p] = 1.0
        case.samp[u, 0] = 3.0
        ids[u, 0] = x_item[p[0]]
        if S > 1:
            case.samp[u, 1] = 2.0
            ids[u, 1] = stranger(u)
    p5 = cols(U_NON_POSITIVE, True)
    case.pred[p5] = 1.0
    case.samp[U_NON_POSITIVE, 0] = 3.0
    ids[U_NON_POSITIVE, 0] = x_item[cols(U_NON_POSITIVE, False)[0]]
    if S >= 4:
        case.samp[U_NON_POSITIVE, 1:4] = 3.0
        ids[U_NON_POSITIVE, 1:3] = x_item[p5[1]]
        ids[U_NON_POSITIVE, 3] = ids[U_NON_POSITIVE, 0]
    case.samples, case.x_item = ids.astype(np.int32), x_item
    case.k7 = k7
    return case


def run_ref(case, remove_hits=False):
    return ref_warp(case.indptr, case.values, case.pred, case.samp, case.go, case.n_items, getattr(case, "samples", None),
                    getattr(case, "x_item", None), remove_hits)
