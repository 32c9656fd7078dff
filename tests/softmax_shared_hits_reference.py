"""Float64 reference, error bars, inputs, host mirrors and a float32 restatement for the sampled-softmax step with SHARED negatives
and ACCIDENTAL HITS REMOVED (csrc/softmax_shared.hip's masked instantiations, ops.softmax_shared_hits_step).  NumPy / SciPy only,
nothing of the code under test.  tests/test_softmax_shared_hits_reference_host.py holds the reference to central differences and the
bars to the restatement on the CPU (and shows that seeded defects fall outside); tests/test_gpu_softmax_shared_hits.py holds the
kernels to the reference.

The step.  By definition the step of softmax_step_reference.ref_step on a case whose [n_users, S] sample table repeats ONE row of S
ids, with hits removed: the values below ARE that function's (imported, not edited) under its variants "hits" / "both" /
"both-uniform" -- here named by the logQ variant alone: plain / logq / logq-uniform.  Column s is a hit for user u when row[s] is the
column of an interaction of u with a value > 0; a hit leaves M_u and Z_u and its coefficient is exactly 0; a user without a kept
column has loss 0 and zero gradients; duplicate ids are separate terms, all hits when one is; c_s = -(log S + log q) keeps the
full S.

Bars.  softmax_shared_reference.loss_bars -- the shared route's own -- evaluated per user on the KEPT columns, with S itself
unchanged.  Why they still apply: a masked column enters the kernels as -inf (statistics) or as a literal 0 (gradients); max(m, -inf)
= m and z + exp(-inf - m) = z + 0 are exact, a product with 0 and a sum with 0 are exact, so a masked column rounds nothing and the
kept columns pass through the operations the derivation counts.  What the derivation counts per ROW stays as it is: T = ceil(S / 32)
tiles may still rescale a kept element (a tile whose kept part moves the maximum rescales whatever came before it) and a sum still
passes through at most S + 2 additions -- so S, not the kept count, stays in both; the kept set only selects the terms.  The order of
the columns (the kernels work in sorted id order) does not enter the derivation: it bounds any order.  The empty kept set: the
kernels find M = -inf, Z = 0, and then m = w_p, a = exp(0) = 1, b = exp(-inf) = 0, D = 1 + 0, loss = 0 + log 1 = 0, d y_p = -t (0 / 1),
K = 0: every operation is exact, the bars are 0 (equality).  The score error delta_u that the loss phase inherits is taken over the
user's interactions and KEPT sampled pairs only: a masked score reaches no output.
dU, dV, d b_u, d b_i: pair_reference.grad_bars on the pair list of the repeated table plus the coefficients' bars carried through, as
in softmax_shared_reference.ref_step; a masked pair has coefficient 0 and bar 0 and adds nothing to either."""
import functools
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

import sampled_adjust_reference as AR
import softmax_shared_reference as R
import softmax_step_reference as SR
from pair_reference import MODE_DOT, f64, grad_bars, ref_pair_grads
from softmax_shared_reference import (supported, slices, scores_exact, ratios, OUTPUTS, OP_RESULTS, TEMPERATURES, ALL_OPTIONS,  # noqa: F401
                                      VARIANTS, options_of, corrections, _cd_row, _fma, _tile_order)

F = np.float32
STEP_VARIANT = {"plain": "hits", "logq": "both", "logq-uniform": "both-uniform"}      # softmax_step_reference's names

# ------------------------------------------------------------------------------------------------ inputs
# (users, S, d, kind): users 1 / 31 / 33 / 129 / 300, S 1 / 31 / 32 / 33 / 65 / 1000, d 4 / 36 / 64 / 128 at least once each.
# kinds: "" the planted hits below; "nohits" no positive of anybody is sampled; "everyone" one sampled item is a positive of EVERY user
GPU_CASES = [(1, 1, 4, ""), (31, 31, 36, ""), (33, 32, 64, ""), (33, 33, 128, ""), (129, 65, 36, ""), (300, 65, 128, ""),
             (300, 1000, 64, ""), (31, 1000, 4, ""), (129, 1, 128, ""), (129, 65, 36, "nohits"), (33, 33, 64, "everyone")]
CORE = (129, 65, 36, "")               # every option crossed on this one
SLICED = (300, 65, 128, "")            # forced slice counts 1, 2, 3
NOHITS = (129, 65, 36, "nohits")
EVERYONE = (33, 33, 64, "everyone")
# planted users (cases with >= 31 users; users 1 ... 5 are softmax_shared_reference.shared_case's): a hit at sorted column 0, at
# column S - 1, in the last (partial) tile, on the run of three equal ids over the columns 30 .. 32 (S >= 33), on every column
# (S <= 65), and a user whose only match with the row is an interaction of value <= 0
U_COL0, U_LAST, U_PARTIAL, U_RUN, U_ALL, U_NONPOS_MATCH = 6, 7, 8, 9, 10, 11
BOUNDARY_USERS = (127, 128, 159, 160, 255, 256)     # 300 users: both sides of the slice boundaries 128, 256 (3 slices) and 160 (2)


def hits_case(n_users, S, d, kind="", exact=False):
    """softmax_shared_reference.shared_case with hits planted (module comment above); with one user: a positive on the id of sorted
    column 0 -- at S = 1 every sample of that user is a hit.  The row gets, from S = 33 on, one id on the sorted columns 30 .. 32:
    a run of three duplicates across a tile edge."""
    base = R.shared_case(n_users, S, d, "", exact=exact, seed=17)
    row = base.row.copy()
    if S >= 33:
        order = np.argsort(row, kind="stable")
        row[order[30]] = row[order[32]] = row[order[31]]
    srt = np.sort(row)
    sampled = set(int(i) for i in row)
    cells = {}
    for u in range(n_users):
        for q in range(base.indptr[u], base.indptr[u + 1]):
            cells[(u, int(base.x_item[q]))] = float(base.values[q])

    def drop_sampled_positives(users):
        for key in [k for k, v in cells.items() if k[0] in users and k[1] in sampled and v > 0]:
            del cells[key]
    if kind == "nohits":
        drop_sampled_positives(set(range(n_users)))
    else:
        if n_users == 1:
            cells[(0, int(srt[0]))] = 1.0
        if n_users >= 31:
            cells[(U_COL0, int(srt[0]))] = 1.0
            cells[(U_LAST, int(srt[-1]))] = 1.0
            cells[(U_PARTIAL, int(srt[32 * ((S - 1) // 32)]))] = 1.0
            if S >= 33:
                cells[(U_RUN, int(srt[31]))] = 1.0
            if S <= 65:
                for i in sampled:
                    cells[(U_ALL, i)] = 1.0
            if kind != "everyone":
                drop_sampled_positives({U_NONPOS_MATCH})
                cells[(U_NONPOS_MATCH, int(srt[S // 3]))] = -1.0
                free = [i for i in range(200) if i not in sampled]
                if free:
                    cells[(U_NONPOS_MATCH, free[0])] = 1.0
        if n_users >= 300:
            for u in BOUNDARY_USERS:
                cells[(u, int(srt[S // 2]))] = 1.0
    if kind == "everyone":
        for u in range(n_users):
            cells[(u, int(srt[S // 2]))] = 1.0
    keys = sorted(cells)
    indptr = np.zeros(n_users + 1, np.int64)
    for u, _ in keys:
        indptr[u + 1] += 1
    indptr = np.cumsum(indptr)
    x_item = np.array([i for _, i in keys], np.int32)
    values = np.array([cells[k] for k in keys], F)
    m = sp.csr_matrix((values, x_item, indptr), shape=(n_users, base.n_items))
    assert m.has_sorted_indices and m.nnz == values.size
    case = SimpleNamespace(**vars(base))
    samples = np.ascontiguousarray(np.broadcast_to(row, (n_users, S)))
    case.__dict__.update(matrix=m, indptr=indptr, x_item=x_item, cols=x_item, values=values, row=row, samples=samples, items=samples,
                         kind=kind, max_pos=int(np.diff(indptr).max()), above=-1, below=-1)
    return case


def hit_mask(case, count_non_positives=False):
    """[U, S] bool in the row's own column order"""
    return AR.hit_mask(case.indptr, case.x_item, case.values, case.samples, count_non_positives)


def case_properties(case):
    """what the cases are meant to hold, as a dict the host test asserts (columns in SORTED order)"""
    order = np.argsort(case.row, kind="stable")
    hs = hit_mask(case)[:, order]
    S = case.S
    pos = case.values > 0
    has_pos = np.array([pos[case.indptr[u]:case.indptr[u + 1]].any() for u in range(case.n_users)])
    out = dict(any_hit=bool(hs.any()), all_hit_users=[int(u) for u in np.flatnonzero(hs.all(1) & has_pos)],
               run=bool(S >= 33 and np.sort(case.row)[30] == np.sort(case.row)[32]),
               everyone=[int(s) for s in np.flatnonzero(hs.all(0))], users_without_positives=int((~has_pos).sum()))
    if case.n_users >= 31 and case.kind != "nohits":
        out.update(col0=bool(hs[U_COL0, 0]), last=bool(hs[U_LAST, S - 1]), partial=bool(hs[U_PARTIAL, 32 * ((S - 1) // 32)]),
                   run_hit=bool(S < 33 or hs[U_RUN, 30:33].all()), all=bool(S > 65 or hs[U_ALL].all()),
                   nonpos_match=bool(case.kind == "everyone" or
                                     (not hs[U_NONPOS_MATCH].any() and hit_mask(case, True)[U_NONPOS_MATCH].any())))
    if case.n_users >= 300 and case.kind != "nohits":
        out["boundaries"] = bool(hs[list(BOUNDARY_USERS)].any(1).all())
    return out


# ------------------------------------------------------------------------------------------------ host mirrors
def hit_ranges(case):
    """mirror of trec_softmax_shared_hit_ranges: (ranges, counts) -- per user the list of [lo, hi) ranges of SORTED columns, in
    interaction order, one per interaction of value > 0 whose item is sampled"""
    srt = np.sort(case.row)
    out, cnt = [], np.zeros(case.n_users, np.int32)
    for u in range(case.n_users):
        mine = []
        for q in range(case.indptr[u], case.indptr[u + 1]):
            if case.values[q] > 0:
                lo, hi = int(np.searchsorted(srt, case.x_item[q], "left")), int(np.searchsorted(srt, case.x_item[q], "right"))
                if hi > lo:
                    mine.append((lo, hi))
        out.append(np.array(mine, np.int32).reshape(-1, 2))
        cnt[u] = len(mine)
    return out, cnt


def transposed_positive(case):
    """mirror of Interactions.transposed_positive: (indptr_tp [n_items + 1], users_tp): per item the users, ascending, with a value
    > 0 on it (one padding entry when there is none at all)"""
    xu = np.repeat(np.arange(case.n_users), np.diff(case.indptr))
    lists = [[] for _ in range(case.n_items)]
    for q in range(case.x_item.size):
        if case.values[q] > 0:
            lists[case.x_item[q]].append(int(xu[q]))
    indptr_tp = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    users_tp = np.array([u for x in lists for u in sorted(x)], np.int32)
    return indptr_tp, (users_tp if users_tp.size else np.zeros(1, np.int32))


# ------------------------------------------------------------------------------------------------ reference
def loss_bars_kept(case, yp, ys, cs, temperature, hits):
    """softmax_shared_reference.loss_bars per user on the kept columns (S unchanged); zeros for a user without a kept column"""
    bar_loss = np.zeros(int((case.values > 0).sum()))
    bar_d_pred, bar_d_samp = np.zeros(yp.size), np.zeros(ys.shape)
    slot = np.cumsum(case.values > 0) - 1
    for u in range(case.n_users):
        b, e = int(case.indptr[u]), int(case.indptr[u + 1])
        kept = ~hits[u]
        pos = case.values[b:e] > 0
        if not pos.any() or not kept.any():
            continue
        sub = SimpleNamespace(S=case.S, indptr=np.array([0, e - b], np.int64), values=case.values[b:e])
        bl, bp, bs = R.loss_bars(sub, yp[b:e], ys[u][kept][None, :], cs[kept], temperature)
        bar_loss[slot[b:e][pos]] = bl
        bar_d_pred[b:e] = bp
        bar_d_samp[u, kept] = bs[0]
    return bar_loss, bar_d_pred, bar_d_samp


def ref_step(case, biased, temperature, variant="plain"):
    """the float64 step (softmax_step_reference.ref_step on the repeated table, hits removed) with the shared route's bars on the
    kept set"""
    assert variant in VARIANTS
    r = SR.ref_step(case, biased, temperature, STEP_VARIANT[variant])
    assert np.array_equal(r.hits, hit_mask(case))
    d, nu, S, nnz = case.d, case.n_users, case.S, case.x_item.size
    t = 1.0 / float(temperature)
    xu, xi = SR.pair_lists(case)
    yp, ys = r.scores.scores[:nnz], r.scores.scores[nnz:].reshape(nu, S)
    bl, bp, bs = loss_bars_kept(case, yp, ys, corrections(case, variant), temperature, r.hits)
    delta = r.delta.copy()
    delta[nnz:][r.hits.reshape(-1)] = 0.0
    du = np.zeros(nu)
    np.maximum.at(du, xu, delta)
    f = np.expm1(2.0 * t * du)
    pos = case.values > 0
    r.b_pred_serial = r.delta[:nnz]
    r.b_loss = bl + 2.0 * t * du[xu[:nnz]][pos]
    empty = np.array([not (~r.hits[u]).any() for u in range(nu)])
    r.b_loss[empty[xu[:nnz]][pos]] = 0.0                            # no kept column: the loss is an exact 0 whatever the scores
    r.b_g = np.concatenate([bp, bs.reshape(-1)]) + np.abs(r.g) * f[xu]
    inh = ref_pair_grads(np.abs(f64(case.U)), np.abs(f64(case.V)), xu, xi, r.b_g, MODE_DOT)
    bU, bV, bub, bib = grad_bars(r.pg, d)
    r.b_dU, r.b_dV, r.b_d_ub, r.b_d_ib = bU + inh.dU, bV + inh.dV, bub + inh.dub, bib + inh.dib
    return r


@functools.lru_cache(maxsize=None)
def cached_case(spec, exact):
    return hits_case(*spec, exact=exact)


@functools.lru_cache(maxsize=None)
def cached_ref(spec, exact, biased, temperature, variant):
    """computed once and shared by the host and the GPU tests; nobody writes into it"""
    return ref_step(cached_case(spec, exact), biased, temperature, variant)


def loss_sum(case, biased, temperature, variant, U=None, V=None, ub=None, ib=None):
    """sum of the reference loss at perturbed tables (central differences)"""
    return SR.loss_sum(case, biased, temperature, STEP_VARIANT[variant], U=U, V=V, ub=ub, ib=ib)


# ------------------------------------------------------------------------------------------------ float32 restatement
DEFECTS = ("mask_ignored_in_z", "mask_ignored_in_dv", "mask_off_by_one", "nonpositive_is_hit", "first_duplicate_only",
           "slice_start_hits_dropped")


def restate_f32(case, biased, temperature, variant, n_slices=1, defect=None):
    """the kernels' arithmetic in float32 NumPy, in SORTED column order: the online (m, z) per half-wave over tiles of 32 sorted
    columns with the masked ones at -inf, the positives on (M, Z) -- M = -inf, Z = 0 included --, P with the masked entries a literal
    0, the half-wave-paired k-steps of the chained MFMA, the users of dV in n_slices slices, duplicates folded over the sorted runs.
    `defect`: one of DEFECTS seeded into it.  Returns a namespace with the six outputs and M, Z, tK."""
    t = F(1.0 / temperature)
    S, nu, d, ni = case.S, case.n_users, case.d, case.n_items
    U, V = case.U.astype(F), case.V.astype(F)
    row = np.sort(case.row).astype(np.int64)
    hit = AR.hit_mask(case.indptr, case.x_item, case.values, np.broadcast_to(row, (nu, S)), defect == "nonpositive_is_hit")
    if defect == "first_duplicate_only":
        first = np.concatenate([[True], row[1:] != row[:-1]])
        hit = hit & first[None, :]
    if defect == "mask_off_by_one":
        hit = np.concatenate([np.zeros((nu, 1), bool), hit[:, :-1]], axis=1)
    Vs = V[row]
    cs = np.zeros(S, F)
    if variant == "logq":
        cs = (-(case.log_q[row] + F(np.log(float(S))))).astype(F)
    elif variant == "logq-uniform":
        cs = np.full(S, -F(F(np.log(float(S))) + F(-np.log(float(ni)))), F)
    dot = np.zeros((nu, S), F)
    for k in range(d):
        dot = _fma(U[:, k][:, None], Vs[:, k][None, :], dot)
    y = dot
    if biased:
        y = ((dot + case.ub[:, None]).astype(F) + case.ib[row][None, :]).astype(F)
    w = _fma(y, t, cs[None, :])
    # ---- row statistics over the kept columns
    Sp = -(-S // 32) * 32
    wm = np.full((nu, Sp), F(-np.inf), F)
    wm[:, :S] = np.where(hit, F(-np.inf), w)
    wz = wm.copy()
    if defect == "mask_ignored_in_z":
        wz[:, :S] = w
    hm, hz = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for half in (0, 1):
            rm, rz = np.full(nu, -np.inf, F), np.zeros(nu, F)
            for t0 in range(0, Sp, 32):
                cols = [t0 + _cd_row(r, half) for r in range(16)]
                tm = wm[:, cols].max(1)
                live = tm > -np.inf
                up = live & (tm > rm)
                sc = np.where(up, np.exp((rm - tm).astype(F)).astype(F), F(1.0)).astype(F)
                rz = np.where(up, (rz * sc).astype(F), rz)
                rm = np.where(up, tm, rm)
                for c in cols:
                    e = np.exp((wz[:, c] - rm).astype(F)).astype(F)
                    rz = np.where(live, (rz + e).astype(F), rz)
            hm.append(rm)
            hz.append(rz)
        M = np.maximum(hm[0], hm[1])
        parts = [np.where(hm[h] > -np.inf, (hz[h] * np.exp((hm[h] - M).astype(F)).astype(F)).astype(F), F(0.0)) for h in (0, 1)]
    Z = (parts[0] + parts[1]).astype(F)
    # ---- positives (shared_positives_kernel as it stands: M = -inf gives m = w_p, a = 1, b = 0, D = 1)
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
    with np.errstate(invalid="ignore", over="ignore"):
        for u in range(nu):
            K, sdy = F(0.0), F(0.0)
            for q in range(case.indptr[u], case.indptr[u + 1]):
                if not pos[q]:
                    continue
                wq = F(pred[q] * t)
                m = max(M[u], wq)
                a, b = np.exp(F(wq - m)).astype(F), np.exp(F(M[u] - m)).astype(F)
                bz = F(b * Z[u])
                D = F(a + bz)
                loss[slot[q]] = F(F(m - wq) + np.log(D).astype(F))
                dy = F(-t * F(bz / D))
                d_pred[q] = dy
                sdy = F(sdy + dy)
                K = F(K + F(b / D))
            tK[u] = F(t * K)
            d_ub[u] = F(sdy + F(tK[u] * Z[u]))
        # ---- the samples' gradients: a masked entry is a literal 0
        Pfull = (tK[:, None] * np.exp((w - M[:, None]).astype(F)).astype(F)).astype(F)
    P = np.where(hit, F(0.0), Pfull).astype(F)
    dU, dV = np.zeros((nu, d), F), np.zeros((ni, d), F)
    d_ib = np.zeros(ni, F)
    for q in range(nnz):
        dU[xu[q]] = _fma(d_pred[q], V[xi[q]], dU[xu[q]])
    for i in np.unique(xi):
        for q in np.flatnonzero(xi == i):
            dV[i] = _fma(d_pred[q], U[xu[q]], dV[i])
            d_ib[i] = F(d_ib[i] + d_pred[q])
    acc = np.zeros((nu, d), F)
    for s in _tile_order(S):
        acc = _fma(P[:, s][:, None], Vs[s][None, :], acc)
    dU = (dU + acc).astype(F)
    dVs, dbs = np.zeros((S, d), F), np.zeros(S, F)
    ln = -(-(-(-nu // 32)) // n_slices) * 32
    for k, a0 in enumerate(range(0, nu, ln)):
        a1 = min(a0 + ln, nu)
        Pv = P
        if defect == "mask_ignored_in_dv":
            Pv = np.where(np.isfinite(Pfull), Pfull, F(0.0)).astype(F)
        elif defect == "slice_start_hits_dropped" and k > 0:       # the cursor of a later slice starts one tile late
            Pv = P.copy()
            first = slice(a0, min(a0 + 32, a1))
            Pv[first] = np.where(np.isfinite(Pfull[first]), Pfull[first], F(0.0))
        part, psum = np.zeros((S, d), F), [np.zeros(S, F), np.zeros(S, F)]
        for u in a0 + _tile_order(a1 - a0):
            part = _fma(Pv[u][:, None], U[u][None, :], part)
            h = (((u - a0) % 32) >> 2) & 1
            psum[h] = (psum[h] + Pv[u]).astype(F)
        dVs = (dVs + part).astype(F)
        dbs = (dbs + (psum[0] + psum[1]).astype(F)).astype(F)
    for i in np.unique(row):                                        # the runs of the sorted row, added in column order
        a_v, a_b = np.zeros(d, F), F(0.0)
        for s in np.flatnonzero(row == i):
            a_v = (a_v + dVs[s]).astype(F)
            a_b = F(a_b + dbs[s])
        dV[i] = (dV[i] + a_v).astype(F)
        d_ib[i] = F(d_ib[i] + a_b)
    return SimpleNamespace(loss=loss, pred_serial=pred, dU=dU, dV=dV, d_ub=d_ub, d_ib=d_ib, M=M, Z=Z, tK=tK, dVs=dVs, dbs=dbs, hit=hit)
