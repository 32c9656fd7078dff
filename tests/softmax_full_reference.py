"""Float64 references, error bars, inputs, float32 restatements and the route mirror for the FULL softmax over the catalogue
(SoftmaxDenseLossGraph): the generic kernels on a dense prediction (csrc/loss_dense.hip, ops.softmax_dense_loss) and the streamed step
(csrc/softmax_shared.hip with the item representation as the streamed matrix, ops.softmax_full_step).  NumPy / SciPy only, nothing of
the code under test.  tests/test_softmax_full_reference_host.py holds the references to central differences and the bars to the
restatements on the CPU (and shows that seeded defects fall outside); tests/test_gpu_softmax_full.py holds the kernels to the references.

The loss.  t = 1 / temperature, w_ui = y_ui t, M_u = max_i w_ui, Z_u = sum_i exp(w_ui - M_u) >= 1.  For every interaction p = (u, i)
of value > 0 (duplicates each their own; a value <= 0 is no positive, its item stays in the sums):
    loss_p = (M_u - w_up) + log Z_u,     G_u = sum_p go_p,     d y_ui = t G_u exp(w_ui - M_u) / Z_u - t sum_{p of u on i} go_p.
The streamed step has go = 1 (G_u = n_u), y = (u . v + b_u) + b_i, d b_u = 0 (the loss does not move with a shift of the row).

Bars.  The derivation of sampled_loss_reference / softmax_shared_reference (u = 2^-24, counts in units of u, LIB = 4 per library
function, DIV = 2, TINY absolute per exponential; a sum of n terms of one sign in ANY order: n relative on the sum of absolute terms);
nothing is tuned.  Every output is invariant under the shift M, so the float32 M a kernel finds is taken as the reference's shift.
    w_i     t is rounded, the product is rounded: 2 |w_i| absolute; scores that are themselves computed (the streamed step, a model's
            dense predictions) are off by delta_ui (pair_reference.score_bar: a chain of d fused multiply-adds, the biases), t delta_ui
            more                                                                                                -> absolute dw_i
    E_i     exp(w_i - M) with the final M: expm1(dw_i + (|w_i - M| + LIB) u)                                    =: e_rel_i (relative)
    Z       online.  An element enters as exp(w_i - m) under the running maximum of its thread (argument rounded: at most span =
            M - min_i w; LIB) and is then multiplied by at most R factors exp(m_old - m_new), each an exponential of a rounded
            difference and a rounded product; the differences telescope to at most span:
            expm1(dw_i + (2 span + LIB + R (LIB + 1)) u) =: e_on_i.  It passes through at most A additions.
            rz = (sum E e_on + A u Z) / Z + n_items TINY.
              generic kernel, T threads per row (64 up to 512 items, else 256), chunks of 4: R = ceil(n_items / 4T) + 6 (+ 3: the
              four waves), A = 4 ceil(n_items / 4T) + 6 (+ 3)
              streamed tiles (softmax_shared_reference): R = ceil(n_items / 32) tiles, A = n_items + 2
    loss    w_p: dw_p absolute (the streamed step: K3's score, its own delta, against the tile's rounding of the same score -- both
            within delta);  (M - w_p): |M - w_p| u;  log Z: rz absolute + LIB |log Z| u;  the sum: |loss| u.
    coef    c = (t G) / Z: G in interaction order, n (sum |go|) u absolute -- relative n u sum |go| / |G| is NOT taken: the bar stays
            absolute, t dG / Z;  t, the product, DIV: (2 + DIV) u;  rz.  Streamed: n_u is exact, dG = 0.
    soft_i  c E_i: |c| E_i ((2 + DIV) u + rz + e_rel_i + u) + E_i t dG / Z, + (|c| + 1) TINY.  A row with sum |go| = 0 is an exact 0: bar 0.
    cell    generic: the positives of a cell are subtracted one by one: t go_p has two roundings, each subtraction rounds at most
            (|soft| + t sum |go|) u.  streamed: d y_p = -float32(t): t u; it reaches dU, dV, d b_i through the K1 gathers.
    dU, dV, d b_i   sums over n terms in any order (tiles, slices, the gathers added before or after): (n + 1) u on the sum of the
            absolute terms (one rounding per product) plus the coefficients' bars carried through |V| resp. |U|.
    d b_u   streamed: 0.f exactly, bar 0.  Generic route of a model: the row sum of d y, (n_items + n_u) u on sum |terms| + carried.
The dyadic family (tables and biases multiples of 1/8, scores_exact) has delta = 0: pred_serial is held bit for bit.  Entries whose
terms are all 0 have a bar of 0."""
import functools
import math
from types import SimpleNamespace

import numpy as np

from pair_reference import MODE_DOT, U32, f64, score_bar
from sampled_loss_reference import TINY, LIB, DIV
from softmax_shared_reference import _cd_row, _tile_order, _fma, slices, MAX_D      # noqa: F401  (slices re-exported)
from softmax_step_reference import scores_exact, ratios, OUTPUTS, OP_RESULTS         # noqa: F401  (re-exported)

F = np.float32
TEMPERATURES = [1.0, 0.25]
FAR = 100.0
SPAN = 30.0
WAVE_MAX_ITEMS = 512                   # csrc/loss_dense.hip: SD_WAVE_MAX_ITEMS


# ------------------------------------------------------------------------------------------------ the route
def tile_supported(n_items, d):
    """mirror of trec_softmax_shared_supported(n_items, d)"""
    return bool(1 <= n_items < 2 ** 31 and d % 4 == 0 and 4 <= d <= MAX_D)


def dense_kernel(exact_class, engine, dot_mode, multi, same_width, n_items, d, switch):
    """mirror of step_plan.dense_kernel"""
    if not (exact_class and engine and dot_mode) or multi or not same_width or not tile_supported(n_items, d) or not switch:
        return None
    return "softmax_full"


# ------------------------------------------------------------------------------------------------ interactions
def _finish_csr(n_users, n_items, rows):
    """rows: per user a list of (column, value), columns sorted, duplicates allowed -> indptr, x_item, values, pos_slot, xu"""
    indptr = np.zeros(n_users + 1, np.int64)
    cols, vals = [], []
    for u, r in enumerate(rows):
        assert [c for c, _ in r] == sorted(c for c, _ in r)
        cols += [c for c, _ in r]
        vals += [v for _, v in r]
        indptr[u + 1] = len(cols)
    x_item, values = np.array(cols, np.int32).reshape(-1), np.array(vals, F).reshape(-1)
    pos = values > 0
    pos_slot = np.where(pos, np.cumsum(pos) - 1, -1).astype(np.int32)
    xu = np.repeat(np.arange(n_users), np.diff(indptr)).astype(np.int64)
    assert x_item.size == 0 or (0 <= x_item.min() and x_item.max() < n_items)
    return SimpleNamespace(indptr=indptr, x_item=x_item, values=values, pos_slot=pos_slot, xu=xu, n_users=n_users, n_items=n_items,
                           n_positive=int(pos.sum()))


U_NONE, U_NONPOS, U_ALL, U_DUP, U_FAR, U_EQUAL, U_SPAN = 1, 2, 3, 4, 5, 6, 7          # planted users (>= 8 users and >= 8 items)


def _rows(rng, n_users, n_items, planted):
    rows = []
    for u in range(n_users):
        n = int(min(n_items, rng.integers(1, 6)))
        cols = np.sort(rng.choice(n_items, size=n, replace=False))
        vals = rng.integers(1, 13, size=n) / 4.0
        r = [(int(c), float(v)) for c, v in zip(cols, vals)]
        if planted and u == U_NONE:
            r = []
        elif planted and u == U_NONPOS:
            r = [(int(c), v) for c, v in zip(np.sort(rng.choice(n_items, size=4, replace=False)), (-1.0, 0.0, -2.5, 0.0))]
        elif planted and u == U_ALL:
            r = [(i, 1.0) for i in range(n_items)]
        elif planted and u == U_DUP:
            a, b, c = (int(x) for x in np.sort(rng.choice(n_items, size=3, replace=False)))
            r = [(a, 1.0), (a, 2.0), (b, 1.0), (b, -1.0), (b, 3.0), (c, 0.0), (c, 0.0)]
        elif not planted and u == 0 and len(r) >= 2:
            r[1] = (r[1][0], 0.0)
        rows.append(r)
    return rows


# ------------------------------------------------------------------------------------------------ the generic kernels: inputs
DENSE_ITEMS = [1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000]        # 512 | 513: the wave / workgroup boundary
DENSE_USERS = [1, 3, 300]
# every n_items with 300 users (the planted rows), the small user counts on both sides of the boundary
DENSE_CASES = [(300, i) for i in DENSE_ITEMS] + [(1, 1), (1, 65), (1, 1000), (3, 1), (3, 257), (3, 512), (3, 513)]
DENSE_PADDED = (300, 257)              # also run as a view of a wider tensor (row stride 257 + 7)


def dense_case(n_users, n_items, seed=0):
    """a float32 prediction and interactions with the planted rows: user 1 no interaction, 2 values <= 0 only, 3 every item positive,
    4 duplicate pairs (and duplicates of value <= 0), 5 one item FAR above the rest, 6 all scores equal, 7 scores spanning +-SPAN"""
    rng = np.random.default_rng(7001 * n_users + 11 * n_items + seed)
    planted = n_users >= 8 and n_items >= 8
    pred = (2.0 * rng.standard_normal((n_users, n_items))).astype(F)
    inter = _finish_csr(n_users, n_items, _rows(rng, n_users, n_items, planted))
    if planted:
        far_item = int(inter.x_item[inter.indptr[U_FAR]])
        pred[U_FAR, far_item] = F(pred[U_FAR].max() + FAR)
        pred[U_EQUAL] = F(0.625)
        pred[U_SPAN] = rng.permutation(np.linspace(-SPAN, SPAN, n_items)).astype(F)
    go = (rng.integers(-8, 17, size=inter.n_positive) / 8.0).astype(F)          # non-constant, both signs
    return SimpleNamespace(pred=pred, go=go, planted=planted, **vars(inter))


# ------------------------------------------------------------------------------------------------ the generic kernels: reference
def _online_counts(n_items, form):
    """(R, A): rescale factors an element may meet and additions it may pass through, per the module docstring"""
    if form == "tiles":
        return float(math.ceil(n_items / 32.0)), n_items + 2.0
    T = 64 if n_items <= WAVE_MAX_ITEMS else 256
    nc = math.ceil(n_items / (4.0 * T))
    lv = 6.0 if T == 64 else 9.0
    return nc + lv, 4.0 * nc + lv


def softmax_rows(W, dw, form):
    """M, E, Z, log-sum bars of the rows of W [U, I] whose entries carry the absolute error dw: (M, E, Z, e_rel, rz)"""
    n_items = W.shape[1]
    R, A = _online_counts(n_items, form)
    M = W.max(1)
    span = M - W.min(1)
    E = np.exp(W - M[:, None])
    Z = E.sum(1)
    e_rel = np.expm1(dw + (np.abs(W - M[:, None]) + LIB) * U32)
    e_on = np.expm1(dw + (2.0 * span[:, None] + LIB + R * (LIB + 1.0)) * U32)
    rz = ((E * e_on).sum(1) + A * U32 * Z) / Z + n_items * TINY
    return M, E, Z, e_rel, rz


def ref_dense(pred, inter, go, temperature, delta=None):
    """loss [P+], d_pred [U, I], M, Z of sum_p go_p loss_p on the dense prediction, and the bars b_loss, b_d_pred of the generic kernels.
    `delta`: the absolute error of the prediction itself (a model's computed scores), None: the prediction is exact input."""
    t = 1.0 / float(temperature)
    Y = f64(pred)
    nu, ni = Y.shape
    W = Y * t
    dw = 2.0 * U32 * np.abs(W) + (t * delta if delta is not None else 0.0)
    M, E, Z, e_rel, rz = softmax_rows(W, dw, "generic")
    pos = inter.values > 0
    xu, xi = inter.xu, inter.x_item.astype(np.int64)
    go = f64(go)
    gp = np.zeros(xu.size)
    gp[pos] = go[inter.pos_slot[pos]]
    G = np.bincount(xu, weights=gp, minlength=nu)
    aG = np.bincount(xu, weights=np.abs(gp), minlength=nu)
    n = np.bincount(xu, weights=pos.astype(np.float64), minlength=nu)
    wp = W[xu, xi]
    lo = (M[xu] - wp) + np.log(Z[xu])
    b_lo = dw[xu, xi] + U32 * np.abs(M[xu] - wp) + rz[xu] + LIB * U32 * np.abs(np.log(Z[xu])) + U32 * np.abs(lo)
    coef = t * G / Z
    dG = n * U32 * aG
    soft = coef[:, None] * E
    b_soft = np.abs(soft) * ((3.0 + DIV) * U32 + rz[:, None] + e_rel) + E * (t * dG / Z)[:, None] + (np.abs(coef)[:, None] + 1.0) * TINY
    b_soft[aG == 0] = 0.0
    C = np.zeros((nu, ni))
    Ca = np.zeros((nu, ni))
    cnt = np.zeros((nu, ni))
    np.add.at(C, (xu, xi), gp)
    np.add.at(Ca, (xu, xi), np.abs(gp))
    np.add.at(cnt, (xu, xi), pos.astype(np.float64))
    d_pred = soft - t * C
    b_d = b_soft + 2.0 * U32 * t * Ca + cnt * U32 * (np.abs(soft) + t * Ca)
    return SimpleNamespace(loss=lo[pos], b_loss=b_lo[pos], d_pred=d_pred, b_d_pred=b_d, M=M, Z=Z, rz=rz, n=n, G=G)


@functools.lru_cache(maxsize=None)
def cached_dense_case(spec):
    return dense_case(*spec)


@functools.lru_cache(maxsize=None)
def cached_dense_ref(spec, temperature):
    c = cached_dense_case(spec)
    return ref_dense(c.pred, c, c.go, temperature)


def dense_loss_sum(pred64, inter, go, temperature):
    """sum_p go_p loss_p in float64 straight from the definition (central differences)"""
    t = 1.0 / float(temperature)
    W = f64(pred64) * t
    M = W.max(1)
    lse = M + np.log(np.exp(W - M[:, None]).sum(1))
    pos = inter.values > 0
    return float((f64(go)[inter.pos_slot[pos]] * (lse[inter.xu[pos]] - W[inter.xu[pos], inter.x_item[pos]])).sum())


# ------------------------------------------------------------------------------------------------ the streamed step: inputs
# (users, items, d): every edge of the 32-row tiles and the 128-row workgroups on both axes, many tiles, every d
GPU_CASES = [(1, 1, 4), (31, 31, 36), (32, 32, 64), (33, 33, 128), (127, 128, 36), (128, 129, 64), (129, 127, 128), (300, 1000, 36),
             (1000, 300, 4), (1, 300, 64), (300, 1, 36), (33, 129, 4)]
SLICED = (300, 129, 128)               # forced slice counts 1, 2, 3
# the chunked K1 gathers of the positives (rows / columns of more than 2,048 entries): the planted user with every item positive on
# 2,100 items; 2,100 users who all hold item 0 (kind "popular")
LONG_CASES = [(9, 2100, 4, ""), (2100, 40, 4, "popular")]
SPLIT_T = 2048
MODEL = (129, 200, 36)


def full_case(n_users, n_items, d, kind="", exact=False, seed=0):
    """tables, biases and interactions of a streamed step.  Planted (>= 8 users and items; embedding columns 0 and 1 are reserved:
    zero everywhere else): user 1 no interaction, 2 values <= 0 only, 3 every item positive, 4 duplicate pairs, 5 one item FAR above
    the rest (column 1), 6 a zero row: all scores equal without biases, 7 scores spanning +-SPAN (column 0)."""
    rng = np.random.default_rng(9101 * n_users + 103 * n_items + 17 * d + (5 if exact else 0) + seed)
    planted = n_users >= 8 and n_items >= 8
    if exact:
        U = (rng.integers(-8, 9, size=(n_users, d)) / 8.0 * (rng.random((n_users, d)) < min(1.0, 16.0 / d))).astype(F)
        V = (rng.integers(-8, 9, size=(n_items, d)) / 8.0 * (rng.random((n_items, d)) < min(1.0, 16.0 / d))).astype(F)
        ub = (rng.integers(-8, 9, n_users) / 8.0).astype(F)
        ib = (rng.integers(-8, 9, n_items) / 8.0).astype(F)
    else:
        U = (rng.standard_normal((n_users, d)) / np.sqrt(d)).astype(F)
        V = (2.0 * rng.standard_normal((n_items, d))).astype(F)
        ub = (0.5 * rng.standard_normal(n_users)).astype(F)
        ib = (0.5 * rng.standard_normal(n_items)).astype(F)
    rows = _rows(rng, n_users, n_items, planted)
    if kind == "popular":                                             # item 0 in every row that has a positive
        rows = [r if not any(v > 0 for _, v in r) or r[0][0] == 0 else [(0, 1.0)] + r for r in rows]
    inter = _finish_csr(n_users, n_items, rows)
    far_item = -1
    if planted:
        U[:, :2] = 0.0
        V[:, :2] = 0.0
        U[U_EQUAL] = 0.0
        U[U_SPAN] = 0.0
        U[U_SPAN, 0] = 1.0
        V[:, 0] = (np.round(rng.permutation(np.linspace(-SPAN, SPAN, n_items)) * 8.0) / 8.0).astype(F)
        far_item = int(inter.x_item[inter.indptr[U_FAR]])
        rest = f64(V) @ f64(U[U_FAR]) + f64(ib)
        U[U_FAR, 1] = 1.0
        V[far_item, 1] = F(np.ceil((np.delete(rest, far_item).max() - rest[far_item] + FAR) * 8.0) / 8.0)
    return SimpleNamespace(U=U, V=V, ub=ub, ib=ib, d=d, exact=exact, planted=planted, far_item=far_item, S=n_items, **vars(inter))


def case_properties(case):
    """what the planted rows are meant to hold, as a dict the host test asserts"""
    Yb = f64(case.U) @ f64(case.V).T + f64(case.ub)[:, None] + f64(case.ib)[None, :]
    Yn = f64(case.U) @ f64(case.V).T
    r = lambda u: slice(case.indptr[u], case.indptr[u + 1])
    out = {}
    if case.planted:
        far = lambda Y: float(Y[U_FAR, case.far_item] - np.delete(Y[U_FAR], case.far_item).max())
        cols = case.x_item[r(U_DUP)]
        out = dict(no_interaction=bool(case.indptr[U_NONE + 1] == case.indptr[U_NONE]),
                   nonpositive=bool(case.values[r(U_NONPOS)].size > 0 and (case.values[r(U_NONPOS)] <= 0).all()),
                   every_item=bool(np.array_equal(case.x_item[r(U_ALL)], np.arange(case.n_items)) and (case.values[r(U_ALL)] > 0).all()),
                   duplicates=bool((np.diff(cols) == 0).sum() >= 3), far_biased=far(Yb), far_plain=far(Yn),
                   all_equal=bool((Yn[U_EQUAL] == Yn[U_EQUAL, 0]).all()), span=float(Yn[U_SPAN].max() - Yn[U_SPAN].min()))
    return out


# ------------------------------------------------------------------------------------------------ the streamed step: reference
def _scores(case, biased):
    U, V = f64(case.U), f64(case.V)
    raw, mag = U @ V.T, np.abs(U) @ np.abs(V).T
    with_ub = raw + f64(case.ub)[:, None] if biased else raw
    Y = with_ub + f64(case.ib)[None, :] if biased else with_ub
    sc = SimpleNamespace(mode=MODE_DOT, mag=mag, with_ub=with_ub, scores=Y, has_ub=biased, has_ib=biased)
    if case.exact:
        assert scores_exact(case)
    return Y, (np.zeros_like(Y) if case.exact else score_bar(sc, case.d))


def ref_step(case, biased, temperature, route="streamed"):
    """the float64 step with upstream gradient 1 and its bars: loss, pred_serial, dU, dV, d_ub, d_ib and b_<name> for each.
    route "streamed": ops.softmax_full_step;  "generic": dense scores -> the generic kernels -> GEMMs and bias sums (a model's step)."""
    t = 1.0 / float(temperature)
    nu, ni, d = case.n_users, case.n_items, case.d
    Y, delta = _scores(case, biased)
    xu, xi = case.xu, case.x_item.astype(np.int64)
    pos = case.values > 0
    aU, aV = np.abs(f64(case.U)), np.abs(f64(case.V))
    r = SimpleNamespace(pred_serial=Y[xu, xi], b_pred_serial=delta[xu, xi], scores=Y, delta=delta)
    cnt = np.zeros((nu, ni))
    np.add.at(cnt, (xu, xi), pos.astype(np.float64))
    n = cnt.sum(1)
    if route == "generic":
        inter = SimpleNamespace(values=case.values, xu=xu, x_item=case.x_item, pos_slot=case.pos_slot)
        dr = ref_dense(Y, inter, np.ones(int(pos.sum())), temperature, delta=delta)
        r.loss, r.b_loss, g, b_g = dr.loss, dr.b_loss, dr.d_pred, dr.b_d_pred
        r.M, r.Z = dr.M, dr.Z
        a_g = np.abs(dr.d_pred + t * cnt) + t * cnt
        r.d_ub, r.b_d_ub = g.sum(1), (ni + n) * U32 * a_g.sum(1) + b_g.sum(1)
        extra_u, extra_i = 0.0, 0.0
    else:
        W = Y * t
        dw = 2.0 * U32 * np.abs(W) + t * delta
        M, E, Z, e_rel, rz = softmax_rows(W, dw, "tiles")
        wp = W[xu, xi]
        lo = (M[xu] - wp) + np.log(Z[xu])
        b_lo = dw[xu, xi] + U32 * np.abs(M[xu] - wp) + rz[xu] + LIB * U32 * np.abs(np.log(Z[xu])) + U32 * np.abs(lo)
        r.loss, r.b_loss = lo[pos], b_lo[pos]
        tk = t * n / Z
        P = tk[:, None] * E
        b_P = P * ((3.0 + DIV) * U32 + rz[:, None] + e_rel) + (tk[:, None] + 1.0) * TINY
        b_P[n == 0] = 0.0
        g, b_g = P - t * cnt, b_P + U32 * t * cnt
        a_g = P + t * cnt
        r.M, r.Z, r.tK = M, Z, tk
        r.d_ub, r.b_d_ub = np.zeros(nu), np.zeros(nu)
        extra_u, extra_i = n[:, None], cnt.sum(0)
    r.g, r.b_g = g, b_g
    r.dU, r.dV, r.d_ib = g @ f64(case.V), g.T @ f64(case.U), g.sum(0)
    r.b_dU = (ni + extra_u + 1.0) * U32 * (a_g @ aV) + b_g @ aV
    r.b_dV = (nu + (extra_i[:, None] if route == "streamed" else 0.0) + 1.0) * U32 * (a_g.T @ aU) + b_g.T @ aU
    r.b_d_ib = (nu + extra_i) * U32 * a_g.sum(0) + b_g.sum(0)
    return r


@functools.lru_cache(maxsize=None)
def cached_case(spec, exact):
    return full_case(*spec[:3], kind=spec[3] if len(spec) > 3 else "", exact=exact)


@functools.lru_cache(maxsize=None)
def cached_ref(spec, exact, biased, temperature, route="streamed"):
    """computed once and shared by the host and the GPU tests; nobody writes into it"""
    return ref_step(cached_case(spec, exact), biased, temperature, route)


def options_of(i):
    """(biased, temperature) of GPU case number i"""
    return (i % 2 == 0, TEMPERATURES[(i // 2) % 2])


def loss_sum(case, biased, temperature, U=None, V=None, ub=None, ib=None):
    """sum of the loss in float64 straight from the definition, at perturbed tables (central differences)"""
    U, V = f64(case.U if U is None else U), f64(case.V if V is None else V)
    Y = U @ V.T
    if biased:
        Y = Y + f64(case.ub if ub is None else ub)[:, None] + f64(case.ib if ib is None else ib)[None, :]
    return dense_loss_sum(Y, case, np.ones(case.n_positive), temperature)


# ------------------------------------------------------------------------------------------------ float32 restatements
DEFECTS = ("padding_zero", "positives_dropped", "count_ignored", "no_t", "no_rescale", "no_item_bias", "duplicates_once")


def _stats_tiles(w, defect):
    """the online (m, z) per half-wave over 32-column tiles and their combination, in float32 (softmax_shared_reference's)"""
    nu, S = w.shape
    Sp = -(-S // 32) * 32
    wp_ = np.full((nu, Sp), F(0.0) if defect == "padding_zero" else F(-np.inf), F)
    wp_[:, :S] = w
    hm, hz = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for half in (0, 1):
            rm, rz = np.full(nu, -np.inf, F), np.zeros(nu, F)
            for t0 in range(0, Sp, 32):
                cols = [t0 + _cd_row(r, half) for r in range(16)]
                tm = wp_[:, cols].max(1)
                live = tm > -np.inf
                up = live & (tm > rm)
                sc = np.where(up, np.exp((rm - tm).astype(F)).astype(F), F(1.0)).astype(F)
                if defect != "no_rescale":
                    rz = np.where(up, (rz * sc).astype(F), rz)
                rm = np.where(up, tm, rm)
                for c in cols:
                    e = np.exp((wp_[:, c] - rm).astype(F)).astype(F)
                    rz = np.where(live, (rz + e).astype(F), rz)
            hm.append(rm)
            hz.append(rz)
        M = np.maximum(hm[0], hm[1])
        parts = [np.where(hm[h] > -np.inf, (hz[h] * np.exp((hm[h] - M).astype(F)).astype(F)).astype(F), F(0.0)) for h in (0, 1)]
    return M, (parts[0] + parts[1]).astype(F)


def restate_step_f32(case, biased, temperature, order="natural", defect=None, n_slices=1):
    """ops.softmax_full_step's arithmetic in float32 NumPy.  order 'natural': row maximum first, every sum in index order; 'paired': the
    online (m, z) per half-wave and the half-wave-paired k-steps of the chained MFMA, the users of dV in n_slices slices.  `defect`: one
    of DEFECTS seeded into it."""
    t = F(1.0 / temperature)
    nu, ni, d = case.n_users, case.n_items, case.d
    U, V = case.U.astype(F), case.V.astype(F)
    dot = np.zeros((nu, ni), F)
    for k in range(d):
        dot = _fma(U[:, k][:, None], V[:, k][None, :], dot)
    y = dot
    if biased:
        y = (dot + case.ub[:, None]).astype(F)
        if defect != "no_item_bias":
            y = (y + case.ib[None, :]).astype(F)
    w = (y * t).astype(F)
    if order == "natural":
        M = w.max(1)
        Z = np.zeros(nu, F)
        for s in range(ni):
            Z = (Z + np.exp((w[:, s] - M).astype(F)).astype(F)).astype(F)
    else:
        M, Z = _stats_tiles(w, defect)
    # ---- positives
    pos = case.values > 0
    nnz = case.x_item.size
    xu, xi = case.xu, case.x_item.astype(np.int64)
    keep = np.ones(nnz, bool)
    if defect == "duplicates_once":
        keep[1:] = ~((xu[1:] == xu[:-1]) & (xi[1:] == xi[:-1]))
    pdot = np.zeros(nnz, F)
    for k in range(d):
        pdot = _fma(U[xu, k], V[xi, k], pdot)
    pred = pdot
    if biased:
        pred = ((pdot + case.ub[xu]).astype(F) + case.ib[xi]).astype(F)
    lz = np.log(Z).astype(F)
    lo = ((M[xu] - (pred * t).astype(F)).astype(F) + lz[xu]).astype(F)
    d_pred = np.where(pos & keep, -(F(1.0) if defect == "no_t" else t), F(0.0)).astype(F)
    if defect == "positives_dropped":
        d_pred[:] = 0.0
    counted = (np.ones(nnz, bool) if defect == "count_ignored" else pos) & keep
    n = np.bincount(xu, weights=counted.astype(np.float64), minlength=nu).astype(F)
    tn = n if defect == "no_t" else (t * n).astype(F)
    with np.errstate(invalid="ignore", divide="ignore"):
        tK = np.where(n > 0, (tn / Z).astype(F), F(0.0)).astype(F)
    # ---- gradients: the positives' K1 gather over the users first, the tiles add onto it; over the items the tiles first
    P = (tK[:, None] * np.exp((w - M[:, None]).astype(F)).astype(F)).astype(F)
    dU = np.zeros((nu, d), F)
    for q in range(nnz):
        dU[xu[q]] = _fma(d_pred[q], V[xi[q]], dU[xu[q]])
    s_order = np.arange(ni) if order == "natural" else _tile_order(ni)
    acc = np.zeros((nu, d), F)
    for s in s_order:
        acc = _fma(P[:, s][:, None], V[s][None, :], acc)
    dU = (dU + acc).astype(F)
    dV, d_ib = np.zeros((ni, d), F), np.zeros(ni, F)
    if order == "natural":
        bounds = [(0, nu)]
    else:
        ln = -(-(-(-nu // 32)) // n_slices) * 32
        bounds = [(a0, min(a0 + ln, nu)) for a0 in range(0, nu, ln)]
    for a0, a1 in bounds:
        part, psum = np.zeros((ni, d), F), [np.zeros(ni, F), np.zeros(ni, F)]
        users = np.arange(a0, a1) if order == "natural" else a0 + _tile_order(a1 - a0)
        for u in users:
            part = _fma(P[u][:, None], U[u][None, :], part)
            h = 0 if order == "natural" else (((u - a0) % 32) >> 2) & 1
            psum[h] = (psum[h] + P[u]).astype(F)
        dV = (dV + part).astype(F)
        d_ib = (d_ib + (psum[0] + psum[1]).astype(F)).astype(F)
    for q in np.argsort(xi, kind="stable"):
        dV[xi[q]] = _fma(d_pred[q], U[xu[q]], dV[xi[q]])
        d_ib[xi[q]] = F(d_ib[xi[q]] + d_pred[q])
    return SimpleNamespace(loss=lo[pos], pred_serial=pred, dU=dU, dV=dV, d_ub=np.zeros(nu, F), d_ib=d_ib, M=M, Z=Z, tK=tK)


def _stats_threads(w, T, defect):
    """the generic kernel's order in float32: T threads stride over the row four elements at a time, xor butterflies, the four waves"""
    nu, n = w.shape
    tm, tz = np.full((nu, T), -np.inf, F), np.zeros((nu, T), F)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(T):
            for i0 in range(r, n, 4 * T):
                idx = [i for i in range(i0, i0 + 4 * T, T) if i < n]
                cm = w[:, idx].max(1)
                up = cm > tm[:, r]
                sc = np.where(up, np.exp((tm[:, r] - cm).astype(F)).astype(F), F(1.0)).astype(F)
                if defect != "no_rescale":
                    tz[:, r] = np.where(up, (tz[:, r] * sc).astype(F), tz[:, r])
                tm[:, r] = np.where(up, cm, tm[:, r])
                for i in idx:
                    tz[:, r] = (tz[:, r] + np.exp((w[:, i] - tm[:, r]).astype(F)).astype(F)).astype(F)

        def merge(m, z, om, oz):
            mx = np.maximum(m, om)
            a = np.where(m > -np.inf, (z * np.exp((m - mx).astype(F)).astype(F)).astype(F), F(0.0))
            b = np.where(om > -np.inf, (oz * np.exp((om - mx).astype(F)).astype(F)).astype(F), F(0.0))
            return mx, (a + b).astype(F)
        lanes = np.arange(T)
        off = 1
        while off < 64:
            tm, tz = merge(tm, tz, tm[:, lanes ^ off], tz[:, lanes ^ off])
            off <<= 1
        m, z = tm[:, 0], tz[:, 0]
        for k in range(1, T // 64):
            m, z = merge(m, z, tm[:, 64 * k], tz[:, 64 * k])
    return m, z


def restate_dense_f32(pred, inter, go, temperature, order="natural", defect=None):
    """the generic kernels' arithmetic in float32 NumPy: order 'natural' (row maximum first, Z in index order) or 'threads' (the
    kernel's online order); `defect` as in DEFECTS where it applies to this form"""
    t = F(1.0 / temperature)
    Y = np.asarray(pred, F)
    nu, ni = Y.shape
    w = (Y * t).astype(F)
    if order == "natural":
        M = w.max(1)
        Z = np.zeros(nu, F)
        for s in range(ni):
            Z = (Z + np.exp((w[:, s] - M).astype(F)).astype(F)).astype(F)
    else:
        M, Z = _stats_threads(w, 64 if ni <= WAVE_MAX_ITEMS else 256, defect)
    pos = inter.values > 0
    xu, xi = inter.xu, inter.x_item.astype(np.int64)
    nnz = xi.size
    keep = np.ones(nnz, bool)
    if defect == "duplicates_once":
        keep[1:] = ~((xu[1:] == xu[:-1]) & (xi[1:] == xi[:-1]))
    lz = np.log(Z).astype(F)
    lo = ((M[xu] - w[xu, xi]).astype(F) + lz[xu]).astype(F)
    gp = np.zeros(nnz, F)
    gp[pos] = np.asarray(go, F)[inter.pos_slot[pos]]
    counted = (np.ones(nnz, bool) if defect == "count_ignored" else pos) & keep
    if defect == "count_ignored":
        gp_all = np.where(pos, gp, F(1.0)).astype(F)
    else:
        gp_all = gp
    G = np.zeros(nu, F)
    for q in range(nnz):
        if counted[q]:
            G[xu[q]] = F(G[xu[q]] + gp_all[q])
    tt = F(1.0) if defect == "no_t" else t
    coef = ((tt * G).astype(F) / Z).astype(F)
    d = (coef[:, None] * np.exp((w - M[:, None]).astype(F)).astype(F)).astype(F)
    if defect != "positives_dropped":
        for q in range(nnz):
            if pos[q] and keep[q]:
                d[xu[q], xi[q]] = F(d[xu[q], xi[q]] - F(tt * gp[q]))
    return SimpleNamespace(loss=lo[pos], d_pred=d, M=M, Z=Z)
