"""Host references for the selection and glue kernels of the exact top-k (csrc/topk2.hip, the floor / pre-refinement kernels of
csrc/topk_filter.hip, trec_topk_dense_users / trec_topk_rows_wg_map of csrc/topk_cascade.hip, trec_exclusive_scan_i32 of csrc/segment.hip and
the list kernels of csrc/exclude.hip).  NumPy only: no torch, nothing of the code under test.  Every function restates the CONTRACT of an
entry point as include/tensorrec_hip.h and the kernel headers give it, not the kernel's code; tests/test_topk_glue_reference_host.py checks
the references on hand-worked cases, shows that the case lists reach every instantiation and that they tell a subtly wrong kernel from a
right one; tests/test_gpu_topk_glue.py holds the kernels to the references.

Tables are [n_sb][stride] float32 (superblock-major, one column per user); only the first n_users columns of a row mean anything.

A ``bug`` keyword selects a deliberately WRONG variant of a reference.  It exists for the discrimination checks of the host test alone.

The floor bracket (filter_floor, filter_floor_ex, cascade_floor, prerefine_tau_listed).  E = the bound in the header of filter_eps, in
float64 and WITHOUT its last inflation:

    E = |dx| (|y| (1 + 2^-8)) + |x| |dy| + (K + 2) (2^-24 + 2^-22) (|x| |y| (1 + 2^-7) + |b_u| + |b_i|)

with {|x|, |dx|} the user's statistics and {|y|, |dy|, |b_i|} the item side's maxima.  The kernels evaluate eps = E (1 + 2^-9) + 1e-30 in
float32 and return floor = tau - mult eps, rounded to nearest and then taken down two floats.
* soundness  floor <= tau - mult E.  The float32 evaluation of E is a sum of non-negative terms with at most 12 roundings on the way of any
  term ((1 +- 2^-24)^12, whether or not the compiler contracts a product and a sum into an fma), so eps >= E (1 + 2^-9) (1 - 12 * 2^-24)
  > E; mult is a power of two; the subtraction errs by half a float and the floor is then moved down two.
* tightness  floor >= tau - mult E (1 + 2^-9) - 1e-29 - w,  w = 12 * 2^-23 max(|tau|, mult E).  eps <= (E (1 + 2^-9) + 1e-30) (1 + 12 *
  2^-24): 6 * 2^-23 mult E (1 + 2^-9); the difference d = tau - mult eps has |d| <= 2 max(|tau|, mult eps), it is rounded once (half a
  float) and taken down twice, 2.5 floats of at most 2^-23 |d| each: 5 * 2^-23 max(|tau|, mult eps).  Together below 12 * 2^-23 max(|tau|,
  mult E); 1e-29 covers mult * 1e-30.
floor_position() is where a floor sits in that bracket (0 = the sound end, 1 = the tight end); the host test evaluates the kernels'
formula in NumPy float32 (floor_f32) and shows that it stays inside."""
import functools
from types import SimpleNamespace

import numpy as np

F32 = np.float32
I32 = np.int32
NINF = F32(-np.inf)
PINF = F32(np.inf)

N_USERS = (1, 255, 256, 257, 700)
N_SB = (1, 7, 31, 32, 33, 70)
LAYOUTS = ("aligned", "odd", "offset")         # stride = n_users rounded up to 4 / n_users + 1 / rounded up, base 4 bytes off 16
KINDS = ("cont", "ties", "short", "inf")       # continuous / integers 0..3 / columns with at most 3 finite entries / with -inf and +inf
SEL_TS = 8                                     # rows per tile of the tiled kernels: the tiled selection wants n_sb >= 4 * SEL_TS


# ------------------------------------------------------------------------------------------------------------------ dispatch rules
def select_ksel(k):
    """list length (registers) of the selection kernels: exact up to 16, then 20 / 24 / 32 / 40 / 48 / 64"""
    assert 1 <= k <= 64
    if k <= 16:
        return k
    for ks in (20, 24, 32, 40, 48, 64):
        if k <= ks:
            return ks


def pick_select(k, n_sb, stride, base_aligned16, select_tiled=1):
    """(KSEL, form) of trec_topk_select_blocks(_ex): the tiled form needs 16-byte loads and at least four tiles"""
    tiled = stride % 4 == 0 and base_aligned16 and n_sb >= 4 * SEL_TS and bool(select_tiled)
    return select_ksel(k), ("tiled" if tiled else "lane")


def pick_scan(k):
    assert 1 <= k <= 16
    return 4 if k <= 4 else 8 if k <= 8 else 10 if k <= 10 else 12 if k <= 12 else 16


def pick_certify(kc):
    assert 1 <= kc <= 64
    return 16 if kc <= 16 else 32 if kc <= 32 else 64


def pick_prerefine(k):
    """(KS, users per workgroup): four users per thread up to k = 16, one above"""
    assert 1 <= k <= 64
    return (16, 1024) if k <= 16 else (64, 256)


def pick_fill(n_sb):
    """where trec_topk_fill_groups(_index) keeps the group starts while it searches them"""
    return "lds" if n_sb <= 2048 else "global"


# ------------------------------------------------------------------------------------------------------------------ tables
def layout_of(n_users, layout):
    """(stride, offset in floats of the table inside its flat buffer)"""
    if layout == "aligned":
        return (n_users + 3) // 4 * 4, 0
    if layout == "odd":
        return n_users + 1, 0
    assert layout == "offset"
    return (n_users + 3) // 4 * 4, 1


def wide_loads(n_users, layout):
    """whether a table of this layout can be read with 16-byte loads: every aligned one, and the n_users + 1 stride where that is a multiple
    of 4 (n_users = 255)"""
    stride, offset = layout_of(n_users, layout)
    return offset == 0 and stride % 4 == 0


@functools.lru_cache(maxsize=None)
def make_table(n_sb, n_users, layout, kind, seed):
    """SimpleNamespace(flat, offset, stride, table): flat is the float32 buffer to upload, table = flat[offset:] as [n_sb][stride].
    Columns beyond n_users hold NaN (a kernel that used them would show).  Read-only."""
    stride, offset = layout_of(n_users, layout)
    rng = np.random.default_rng(1000003 * seed + 7919 * n_sb + n_users)
    if kind == "ties":
        t = rng.integers(0, 4, size=(n_sb, n_users)).astype(F32)
    else:
        t = rng.standard_normal((n_sb, n_users)).astype(F32)
    if kind == "short":
        keep = rng.integers(0, 4, size=n_users)                    # finite entries per column: 0..3
        rank = np.argsort(np.argsort(rng.random((n_sb, n_users)), axis=0), axis=0)
        t[rank >= keep[None, :]] = NINF
    elif kind in ("inf", "nan"):
        r = rng.random((n_sb, n_users))
        t[r < 0.15] = NINF
        t[r > 0.90] = PINF
        if kind == "nan":
            t[(r > 0.40) & (r < 0.50)] = F32(np.nan)
    flat = np.full(n_sb * stride + offset, np.nan, dtype=F32)
    table = flat[offset:].reshape(n_sb, stride)
    table[:, :n_users] = t
    flat.setflags(write=False)
    return SimpleNamespace(flat=flat, offset=offset, stride=stride, table=table, n_sb=n_sb, n_users=n_users, layout=layout, kind=kind)


def shapes(salt, kinds=KINDS):
    """the 30 (n_users, n_sb) shapes, each with a layout and a value kind that rotate with ``salt`` (twelve salts: every combination)"""
    out = []
    for iu, nu in enumerate(N_USERS):
        for isb, nsb in enumerate(N_SB):
            i = iu * len(N_SB) + isb
            out.append(SimpleNamespace(n_users=nu, n_sb=nsb, layout=LAYOUTS[(i + salt) % 3], kind=kinds[(i + salt // 3) % len(kinds)],
                                       seed=salt, index=i))
    return out


def bits(a):
    """float32 array -> its bit patterns (what 'equal' means for floats here)"""
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------ 1. select
SELECT_KS = (1, 2, 3, 5, 8, 10, 12, 16, 17, 20, 21, 24, 25, 32, 33, 40, 41, 48, 49, 64)


def select_cases(k):
    """the cases of one k: all 30 shapes; k_tau rotates over {1, k // 2 + 1, k}; every fifth case passes sel_max and tau as NULL"""
    salt = SELECT_KS.index(k)
    out = []
    for sh in shapes(salt):
        k_tau = (1, k // 2 + 1, k)[(sh.index // 2 + salt) % 3]
        out.append(SimpleNamespace(k=k, k_tau=k_tau, nulls=(sh.index + salt) % 5 == 0, **vars(sh)))
    return out


def select_blocks(table, n_users, k, k_tau=None, bug=None):
    """sel [n_users][k] = the k superblocks with the largest entries of each column, ordered (value desc, superblock asc); -inf entries
    and missing superblocks give slot -1; sel_max [k][n_users] their values (-inf in empty slots); tau = entry k_tau - 1 (-inf if empty).
    No NaN in the table."""
    k_tau = k if k_tau is None else k_tau
    col = np.asarray(table)[:, :n_users].T                             # [n_users][n_sb]
    assert not np.isnan(col).any()
    n_sb = col.shape[1]
    if bug == "tie_reversed":                                          # (value desc, superblock DESC)
        order = (n_sb - 1 - np.argsort(-col[:, ::-1], axis=1, kind="stable"))
    else:
        order = np.argsort(-col, axis=1, kind="stable")                # stable: equal values keep ascending superblocks
    sel = np.full((n_users, k), -1, dtype=I32)
    val = np.full((n_users, k), NINF, dtype=F32)
    m = min(k, n_sb)
    sel[:, :m] = order[:, :m]
    val[:, :m] = np.take_along_axis(col, order[:, :m], axis=1)
    if bug != "neg_inf_selected":
        sel[val == NINF] = -1
    tau = np.where(sel[:, k_tau - 1] >= 0, val[:, k_tau - 1], NINF).astype(F32)
    return SimpleNamespace(sel=sel, sel_max=np.ascontiguousarray(val.T), tau=tau)


# ------------------------------------------------------------------------------------------------------------------ 2. collect
COLLECT_KSEL = (1, 6, 48)
COLLECT_KINDS = KINDS + ("nan",)


def collect_inputs(table, n_users, ksel, seed):
    """floor / flag_in / redo for a collect case: floors at an entry of the column (so entries EQUAL to the floor occur), about a third of
    the users with more than ksel qualifying superblocks, +inf and -inf floors, a third of the users flagged before; redo leaves users
    256..511 (a whole workgroup) unmarked"""
    rng = np.random.default_rng(77 + seed)
    col = np.asarray(table)[:, :n_users]
    n_sb = col.shape[0]
    srt = -np.sort(-np.where(np.isnan(col), PINF, col), axis=0)        # descending, NaN counted as qualifying
    q = rng.integers(0, min(n_sb, ksel + 2), size=n_users)
    floor = srt[q, np.arange(n_users)].astype(F32)
    floor[np.isinf(floor) & (floor < 0)] = F32(-1.0)
    pick = rng.random(n_users)
    floor[pick < 0.06] = PINF
    floor[pick > 0.94] = NINF
    flag_in = (rng.random(n_users) < 0.33).astype(I32)
    redo = (rng.random(n_users) < 0.4).astype(I32)
    redo[256:512] = 0
    return SimpleNamespace(floor=floor, flag_in=flag_in, redo=redo, n_flagged_in=5)


def collect_blocks(table, n_users, floor, ksel, flag_in, n_flagged_in, redo=None, keys_in=None, count_in=None, bug=None):
    """keys [n_users][ksel] = the superblocks with !(v < floor) ascending, -1 in unused slots, count their number; more than ksel of them:
    keys all -1, count 0, flag 1, and n_flagged rises if the user was not flagged before.  redo given: users with redo == 0 keep keys_in /
    count_in / flag_in."""
    col = np.asarray(table)[:, :n_users]
    keys = np.full((n_users, ksel), -1, dtype=I32)
    count = np.zeros(n_users, dtype=I32)
    flag = np.array(flag_in, dtype=I32)
    n_flagged = int(n_flagged_in)
    for u in range(n_users):
        if redo is not None and not redo[u]:
            keys[u] = keys_in[u]
            count[u] = count_in[u]
            continue
        q = np.nonzero(~(col[:, u] < floor[u]))[0]
        if len(q) > ksel:
            if bug == "over_not_emptied":
                keys[u] = q[:ksel]
                count[u] = ksel
            if bug == "count_reflagged" or flag[u] == 0:
                n_flagged += 1
            flag[u] = 1
        else:
            keys[u, :len(q)] = q
            count[u] = len(q)
    return SimpleNamespace(keys=keys, count=count, flag=flag, n_flagged=n_flagged)


# ------------------------------------------------------------------------------------------------------------------ 3. scan + prune
SCAN_KS = (1, 4, 5, 8, 9, 10, 11, 12, 13, 16)
SCAN_CAPS = (1, 6, 128)
SENT_I = -7                                                            # what an output buffer holds before a call (int32)
SENT_F = F32(-12345.5)                                                 # ... (float32)


def scan_blocks(table, n_users, k, floor0, cand_cap, bug=None):
    """tau / sel_max as select_blocks(k, k); cand_s / cand_v [cand_cap][n_users] (slot-major) = the first min(c, cand_cap) entries with
    !(v < floor0) in superblock order (the other slots keep SENT_I / SENT_F); cand_n = c, uncapped.  The table may hold NaN (a NaN entry
    is a candidate; the k largest are taken over the non-NaN entries)."""
    col = np.asarray(table)[:, :n_users]
    sel = select_blocks(np.where(np.isnan(col), NINF, col), n_users, k)
    cs = np.full((cand_cap, n_users), SENT_I, dtype=I32)
    cv = np.full((cand_cap, n_users), SENT_F, dtype=F32)
    cn = np.zeros(n_users, dtype=I32)
    for u in range(n_users):
        q = np.nonzero(~(col[:, u] < floor0[u]))[0]
        cn[u] = len(q)
        m = min(len(q), cand_cap)
        cs[:m, u] = q[:m]
        cv[:m, u] = col[q[:m], u]
    if bug == "user_major":                                            # the same lists written [n_users][cand_cap]
        cs = np.ascontiguousarray(cs.T).reshape(cand_cap, n_users)
        cv = np.ascontiguousarray(cv.T).reshape(cand_cap, n_users)
    return SimpleNamespace(sel_max=sel.sel_max, tau=sel.tau, cand_s=cs, cand_v=cv, cand_n=cn)


def prune_candidates(cand_s, cand_v, cand_n, cand_cap, floor, ksel, flag_in, n_flagged_in):
    """collect_blocks over the listed candidates instead of the table, except for the users with an incomplete list and a floor below
    +inf (cand_n > cand_cap): redo = 1, keys -1, count 0, no flag"""
    n_users = len(cand_n)
    keys = np.full((n_users, ksel), -1, dtype=I32)
    count = np.zeros(n_users, dtype=I32)
    flag = np.array(flag_in, dtype=I32)
    redo = np.zeros(n_users, dtype=I32)
    n_flagged = int(n_flagged_in)
    for u in range(n_users):
        if cand_n[u] > cand_cap and floor[u] < PINF:
            redo[u] = 1
            continue
        m = min(int(cand_n[u]), cand_cap)
        q = cand_s[:m, u][~(cand_v[:m, u] < floor[u])]
        if len(q) > ksel:
            if flag[u] == 0:
                n_flagged += 1
            flag[u] = 1
        else:
            keys[u, :len(q)] = q
            count[u] = len(q)
    return SimpleNamespace(keys=keys, count=count, flag=flag, n_flagged=n_flagged, redo=redo)


# ------------------------------------------------------------------------------------------------------------------ 4. floors
FLOOR_MULTS = (1.0, 2.0, 4.0)
FLOOR_KDIMS = (5, 64, 128, 256)
U23 = 2.0 ** -23


def eps_bound(ustats, bu_abs, gstats, kdim):
    """E of the module docstring, float64, per user"""
    st = np.asarray(ustats, dtype=np.float64)
    ni, ai, bi = (float(x) for x in np.asarray(gstats, dtype=np.float64)[:3])
    ck = (kdim + 2) * (2.0 ** -24 + 2.0 ** -22)
    with np.errstate(invalid="ignore", over="ignore"):
        return st[:, 1] * (ni * (1 + 2.0 ** -8)) + st[:, 0] * ai + ck * (st[:, 0] * ni * (1 + 2.0 ** -7) + np.asarray(bu_abs, np.float64) + bi)


def floor_bracket(tau, E, mult):
    """(lo, hi) float64: lo <= floor <= hi for finite tau and E"""
    tau = np.asarray(tau, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        hi = tau - mult * E
        w = 12 * U23 * np.maximum(np.abs(tau), mult * E)
        lo = tau - mult * E * (1 + 2.0 ** -9) - 1e-29 - w
    return lo, hi


def floor_position(floor, lo, hi):
    """0 at the sound end (tau - mult E), 1 at the tight end"""
    return (hi - np.asarray(floor, dtype=np.float64)) / (hi - lo)


def floor_f32(tau, ustats, bu_abs, gstats, kdim, mult, bug=None):
    """the kernels' formula in NumPy float32 (no fused multiply-add): eps and tau - mult eps taken down two floats"""
    st = np.asarray(ustats, dtype=F32)
    ni, ai, bi = (F32(x) for x in gstats[:3])
    ck = F32(kdim + 2) * F32(2.98023224e-07)
    with np.errstate(invalid="ignore", over="ignore"):
        eps = st[:, 1] * (ni * F32(1.00390625)) + st[:, 0] * ai + ck * (st[:, 0] * ni * F32(1.0078125) + np.asarray(bu_abs, F32) + bi)
        eps = eps * F32(1.001953125) + F32(1e-30)
        d = (np.asarray(tau, F32) - F32(mult) * eps).astype(F32)
    f = np.nextafter(np.nextafter(d, NINF), NINF)
    if bug == "one_above":                                             # the first float ABOVE tau - mult E
        hi = np.asarray(tau, np.float64) - mult * eps_bound(ustats, bu_abs, gstats, kdim)
        f = hi.astype(F32)
        f = np.where(f.astype(np.float64) <= hi, np.nextafter(f, PINF), f)
    return f.astype(F32)


def floor_inputs(n_users, kdim, with_bias, seed):
    """statistics of plausible size (normalised rows: |x| ~ 1, |dx| ~ 2^-9 |x|), taus of both signs, small and large; the first users carry
    the exact cases: 0 tau = -inf; 1 |x| = +inf; 2 |dx| = NaN; 3 tau = NaN; 4 tau = -inf AND |x| = NaN"""
    rng = np.random.default_rng(4242 + 13 * seed + kdim)
    x = np.exp(rng.uniform(-2, 2, n_users))
    st = np.stack([x, x * rng.uniform(0.2, 1.0, n_users) * 2.0 ** -9], axis=1).astype(F32)
    tau = (rng.standard_normal(n_users) * np.exp(rng.uniform(-6, 4, n_users))).astype(F32)
    bias = (rng.standard_normal(n_users) * 0.3).astype(F32) if with_bias else None
    gstats = np.array([rng.uniform(0.5, 3.0), rng.uniform(0.5, 3.0) * 2.0 ** -9, rng.uniform(0, 0.5) if with_bias else 0.0], dtype=F32)
    special = {}
    if n_users >= 5:
        tau[0] = NINF
        st[1, 0] = PINF
        st[2, 1] = F32(np.nan)
        tau[3] = F32(np.nan)
        tau[4] = NINF
        st[4, 0] = F32(np.nan)
        special = {"keep_all": [0], "bad": [1, 2, 3, 4]}
    return SimpleNamespace(tau=tau, ustats=st, bias=bias, gstats=gstats, special=special, kdim=kdim, n_users=n_users)


def floor_expect(inp, mult, cascade=False, src=None):
    """what is exact about the floor kernels: flags, the floors of the special users, and (lo, hi) for everybody else.
    cascade: a bad bound gives floor +inf instead of -inf; src[u] < 0 gives tau = floor = +inf and flag 0."""
    n = inp.n_users
    bu = np.abs(inp.bias) if inp.bias is not None else np.zeros(n, F32)
    E = eps_bound(inp.ustats, bu, inp.gstats, inp.kdim)
    lo, hi = floor_bracket(inp.tau, E, mult)
    bad = ~np.isfinite(E) | np.isnan(inp.tau)
    keep_all = ~bad & (inp.tau == NINF)
    exact = np.full(n, np.nan, dtype=F32)                              # NaN = "held to the bracket"
    exact[bad] = PINF if cascade else NINF
    exact[keep_all] = NINF
    flag = bad.astype(I32)
    tau_out = np.array(inp.tau, dtype=F32)
    if src is not None:
        dead = np.asarray(src) < 0
        exact[dead] = PINF
        flag[dead] = 0
        tau_out[dead] = PINF
    return SimpleNamespace(lo=lo, hi=hi, exact=exact, flag=flag, n_flagged=int(flag.sum()), tau_out=tau_out,
                           bracketed=np.isnan(exact))


def check_floor(floor, exp):
    """assert a float32 floor array against floor_expect; returns the largest position inside the bracket"""
    floor = np.asarray(floor, dtype=F32)
    ex = ~exp.bracketed
    assert np.array_equal(bits(floor[ex]), bits(exp.exact[ex])), "exact floors differ"
    f = floor[exp.bracketed].astype(np.float64)
    lo, hi = exp.lo[exp.bracketed], exp.hi[exp.bracketed]
    assert np.all(np.isfinite(f))
    assert np.all(f <= hi), "unsound floor: above tau - mult E by %g" % float(np.max(f - hi))
    assert np.all(f >= lo), "floor below the bracket by %g" % float(np.max(lo - f))
    return float(np.max(floor_position(f, lo, hi))) if len(f) else 0.0


# ------------------------------------------------------------------------------------------------------------------ 5. prerefine_rows_pos
LB_TAG_BITS = 12


def lb_key(x):
    """monotone signed integer key of a float32 (negative floats -> negative keys)"""
    b = np.asarray(x, dtype=F32).view(np.int32).astype(np.int64)
    return np.where(b >= 0, b, 0x80000000 - (b & 0xFFFFFFFF))


def lb_untag_key(k2):
    k2 = np.asarray(k2, dtype=np.int64)
    b = np.where(k2 >= 0, k2, (0x80000000 - k2) & 0xFFFFFFFF)
    return b.astype(np.uint32).view(F32)


def lb_tag(lb, idx):
    """the tagged lower bound: the key floored to the multiple of 4096 strictly below it, plus the index (score_common.hpp's format);
    -inf, NaN and |lb| >= 1e37 give -inf"""
    lb = np.asarray(lb, dtype=F32)
    k2 = ((lb_key(lb) >> LB_TAG_BITS) - 1) * (1 << LB_TAG_BITS) + np.asarray(idx, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        ok = np.abs(lb) < F32(1e37)
    return np.where(ok, lb_untag_key(np.where(ok, k2, 0)), NINF).astype(F32)


def lb_tag_index(tagged):
    return (lb_key(tagged) & ((1 << LB_TAG_BITS) - 1)).astype(np.int64)


PREREFINE_CASES = tuple(SimpleNamespace(k=k, n_users=nu, n_sb=n_sb, hot=hot, rcap=512, top_k=16, sb_per_chunk=(64 if n_sb == 300 else 2))
                        for k, nu, n_sb, hot in ((1, 1061, 3, False), (10, 1061, 300, True), (16, 1061, 300, False), (10, 1061, 3, False),
                                                 (17, 293, 300, False), (40, 293, 3, False), (64, 293, 300, False), (17, 1061, 300, True)))


@functools.lru_cache(maxsize=None)
def prerefine_inputs(ci):
    """sel [n_users][k] (rows of the chunk lists), val [k][n_users] (tagged lower bounds), src.  Every user wants distinct superblocks;
    hot: slot 0 of everybody is superblock 0 (more users than rcap).  Empty slots come as row -1 or as a -inf value; every ninth user has
    no source."""
    c = PREREFINE_CASES[ci]
    rng = np.random.default_rng(900 + ci)
    sel = np.full((c.n_users, c.k), -1, dtype=I32)
    val = np.full((c.k, c.n_users), NINF, dtype=F32)
    for u in range(c.n_users):
        m = min(c.k, c.n_sb)
        if u % 5 == 3:
            m = int(rng.integers(0, m + 1))
        s = rng.permutation(c.n_sb)[:m]
        if c.hot and m:
            s = np.concatenate([[0], s[s != 0]])[:m]
        lbv = rng.standard_normal(m).astype(F32) * F32(3.0)
        sel[u, :m] = (s // c.sb_per_chunk) * c.top_k + rng.integers(0, c.top_k, size=m)
        val[:m, u] = lb_tag(lbv, s % c.sb_per_chunk)
        if u % 7 == 2 and m > 1:
            val[m - 1, u] = NINF                                       # a listed row that certifies nothing
    src = np.arange(c.n_users, dtype=I32)
    src[8::9] = -1
    for a in (sel, val, src):
        a.setflags(write=False)
    return SimpleNamespace(sel=sel, val=val, src=src)


def prerefine_want(sel, val, k, top_k, sb_per_chunk, n_sb, src):
    """want [n_users][k] = the superblock a live user's slot asks for ((row // top_k) * sb_per_chunk + tag index) or -1; row_count [n_sb]"""
    n_users = sel.shape[0]
    s = (sel.astype(np.int64) // top_k) * sb_per_chunk + lb_tag_index(val.T)
    live = (np.asarray(src) >= 0)[:, None] if src is not None else np.ones((n_users, 1), bool)
    want = np.where(live & (sel >= 0) & (val.T > NINF), s, -1)
    assert want.max(initial=-1) < n_sb
    return want, np.bincount(want[want >= 0], minlength=n_sb).astype(I32)


def check_prerefine(want, row_count_ref, rcap, sel_sb, row_count, row_user, ok, sel_pos):
    """the invariants of trec_topk_prerefine_rows_pos (which users an over-full list drops is not determined).  row_user [n_sb][rcap] was -1
    everywhere before the call."""
    n_users, k = want.shape
    n_sb = len(row_count_ref)
    assert np.array_equal(row_count, row_count_ref), "row_count"
    placed = sel_sb >= 0
    assert np.array_equal(sel_sb[placed], want[placed]), "a placed slot names another superblock than it asked for"
    assert not placed[want < 0].any(), "an empty slot was placed"
    pos = sel_pos[placed]
    assert (pos >= 0).all() and (pos < rcap).all(), "sel_pos out of range"
    uu = np.nonzero(placed)[0]
    assert np.array_equal(row_user[sel_sb[placed], pos], uu), "row_user[sel_sb][sel_pos] is not the user"
    n_placed = np.bincount(sel_sb[placed], minlength=n_sb)
    assert np.array_equal(n_placed, np.minimum(row_count_ref, rcap)), "min(count, rcap) pairs must be placed"
    filled = row_user >= 0
    assert np.array_equal(filled.sum(axis=1), n_placed), "entries in row_user that no (user, slot) owns"
    assert np.array_equal(filled, np.arange(rcap)[None, :] < n_placed[:, None]), "a list with holes"
    for s in np.nonzero(n_placed)[0]:
        us = row_user[s, :n_placed[s]]
        assert len(np.unique(us)) == len(us), "a user twice in the list of superblock %d" % s
    assert np.array_equal(ok, (placed.all(axis=1)).astype(I32)), "ok"


def prerefine_simulate(want, n_sb, rcap, bug=None):
    """a sequential model of the kernel (users in order) for the host test; bug 'dup': an over-full list's last slot is handed out twice"""
    n_users, k = want.shape
    sel_sb = np.full((n_users, k), -1, dtype=I32)
    sel_pos = np.zeros((n_users, k), dtype=I32)
    row_user = np.full((n_sb, rcap), -1, dtype=I32)
    cnt = np.zeros(n_sb, dtype=I32)
    for u in range(n_users):
        for j in range(k):
            s = want[u, j]
            if s < 0:
                continue
            p = cnt[s]
            cnt[s] += 1
            if bug == "dup" and p >= rcap:
                p = rcap - 1
            sel_pos[u, j] = p
            if p < rcap:
                sel_sb[u, j] = s
                row_user[s, p] = u
    ok = (sel_sb >= 0).all(axis=1).astype(I32)
    return SimpleNamespace(sel_sb=sel_sb, row_count=cnt, row_user=row_user, ok=ok, sel_pos=sel_pos)


# ------------------------------------------------------------------------------------------------------------------ 6. prerefine_tau_listed
TAU_LISTED_KS = (10, 16, 17, 40)


@functools.lru_cache(maxsize=None)
def tau_listed_inputs(k, n_users=293, n_sb=40, rcap=512):
    """placed lists (from prerefine_simulate over random wants), maxima pre_max [n_sb * rcap], statistics, tau and cand_floor.  tau before
    the call lies either far below or far above min maxima - eps, so that whether it rises is decided; user classes by u % 8:
    0 tau far above (stays); 1 a NaN maximum; 2 not ok (an empty slot); 3 no source; 4 cand_floor +inf; 5 cand_floor already above;
    6 |x| = +inf (unusable bound); 7 plain.  Every other user is plain."""
    rng = np.random.default_rng(600 + k)
    want = np.stack([rng.permutation(n_sb)[:k] if k <= n_sb else np.resize(rng.permutation(n_sb), k) for _ in range(n_users)]).astype(np.int64)
    if k > n_sb:                                                       # more slots than superblocks: the surplus slots are empty
        want[:, n_sb:] = -1
    cls = np.arange(n_users) % 16
    cls[cls >= 8] = 7
    for u in np.nonzero(cls == 2)[0]:
        want[u, rng.integers(0, min(k, n_sb))] = -1
    src = np.arange(n_users, dtype=I32)
    src[cls == 3] = -1
    sim = prerefine_simulate(np.where((src >= 0)[:, None], want, -1), n_sb, rcap)
    pre_max = (rng.standard_normal(n_sb * rcap) * 2.0).astype(F32)
    for u in np.nonzero(cls == 1)[0]:
        pre_max[sim.sel_sb[u, 0] * rcap + sim.sel_pos[u, 0]] = F32(np.nan)
    x = np.exp(rng.uniform(-1, 1, n_users))
    st = np.stack([x, x * 2.0 ** -9 * rng.uniform(0.3, 1, n_users)], axis=1).astype(F32)
    st[cls == 6, 0] = PINF
    gstats = np.array([1.5, 1.5 * 2.0 ** -9, 0.2], dtype=F32)
    bias = (rng.standard_normal(n_users) * 0.2).astype(F32)
    tau = np.full(n_users, -50.0, dtype=F32) + rng.standard_normal(n_users).astype(F32)
    tau[cls == 0] = F32(50.0)
    tau[3::32] = NINF
    cand_floor = np.where(np.isinf(tau), F32(-60.0), tau - F32(1.0)).astype(F32)
    cand_floor[cls == 4] = PINF
    cand_floor[cls == 5] = F32(40.0)
    ok = sim.ok.copy()
    if k > n_sb:                                                       # (every user has empty slots: nobody is ok)
        assert not ok.any()
    return SimpleNamespace(k=k, n_users=n_users, n_sb=n_sb, rcap=rcap, sel_sb=sim.sel_sb, sel_pos=sim.sel_pos, ok=ok, pre_max=pre_max,
                           src=src, ustats=st, bias=bias, gstats=gstats, kdim=64, tau=tau, cand_floor=cand_floor, cls=cls)


def tau_listed_expect(inp):
    """vals exact; per user: 'same' (tau and cand_floor keep their bits) or the bracket the new tau must lie in"""
    n, k = inp.n_users, inp.k
    live = inp.src >= 0
    vals = np.full((n, k), PINF, dtype=F32)
    pl = (inp.sel_sb >= 0) & live[:, None]
    vals[pl] = inp.pre_max[inp.sel_sb[pl].astype(np.int64) * inp.rcap + inp.sel_pos[pl]]
    with np.errstate(invalid="ignore"):
        m = np.min(np.where(np.isnan(vals), NINF, vals), axis=1).astype(np.float64)
    E = eps_bound(inp.ustats, np.abs(inp.bias), inp.gstats, inp.kdim)
    lo, hi = floor_bracket(m, E, 1.0)
    usable = live & (inp.ok != 0) & np.isfinite(E) & np.isfinite(m)
    rises = usable & (lo > inp.tau)
    stays = ~usable | (hi <= inp.tau)
    assert np.all(rises | stays), "an input whose outcome the bracket does not decide"
    return SimpleNamespace(vals=vals, rises=rises, lo=lo, hi=hi, E=E)


def check_tau_listed(inp, exp, tau, vals, cand_floor):
    """returns the largest position of a raised tau / cand_floor inside its bracket"""
    assert np.array_equal(bits(vals), bits(exp.vals)), "vals"
    st = ~exp.rises
    assert np.array_equal(bits(tau[st]), bits(inp.tau[st])), "tau of a user that must keep it"
    assert np.array_equal(bits(cand_floor[st]), bits(inp.cand_floor[st])), "cand_floor of a user that must keep it"
    r = exp.rises
    t = tau[r].astype(np.float64)
    assert np.all(t <= exp.hi[r]) and np.all(t >= exp.lo[r]), "raised tau outside its bracket"
    worst = float(np.max(floor_position(t, exp.lo[r], exp.hi[r]))) if r.any() else 0.0
    lo2, hi2 = floor_bracket(tau[r], exp.E[r], 1.0)                    # cand_floor: F(the float32 tau the kernel wrote)
    old = inp.cand_floor[r]
    new = cand_floor[r]
    keep = np.isinf(old) | (hi2 <= old)
    assert np.array_equal(bits(new[keep]), bits(old[keep])), "cand_floor must only rise, and only where it was finite"
    up = ~np.isinf(old) & (lo2 > old)
    assert np.all(keep | up), "an input whose cand_floor outcome the bracket does not decide"
    f = new[up].astype(np.float64)
    assert np.all(f <= hi2[up]) and np.all(f >= lo2[up]), "raised cand_floor outside its bracket"
    if up.any():
        worst = max(worst, float(np.max(floor_position(f, lo2[up], hi2[up]))))
    return worst


# ------------------------------------------------------------------------------------------------------------------ 7. rows_wg_map
WG_MAP_N_SB = (1, 255, 256, 257, 700)
GROUP_ROWS = 512


def wg_map_inputs(n_sb, wgs_per_row, seed=0):
    rng = np.random.default_rng(31 + n_sb + seed)
    pool = np.array([0, 1, 512, 513, wgs_per_row * 512, wgs_per_row * 512 + 1, wgs_per_row * 512 + 5000, 1024, 1025, 0, 0], dtype=I32)
    rc = pool[rng.integers(0, len(pool), size=n_sb)]
    rc[:min(n_sb, 7)] = pool[:min(n_sb, 7)]
    return rc


def rows_wg_map(row_count, wgs_per_row, map_cap, guard=64, bug=None):
    """wg_start [n_sb + 1]; wg_map [map_cap + guard] with SENT_I wherever nothing may be written"""
    c = np.minimum(-(-row_count.astype(np.int64) // GROUP_ROWS), wgs_per_row)
    start = np.concatenate([[0], np.cumsum(c)]).astype(I32)
    wm = np.full(map_cap + guard, SENT_I, dtype=I32)
    for s in range(len(row_count)):
        for j in range(int(c[s])):
            p = start[s] + j
            if p < map_cap or bug == "no_cap":
                wm[p] = s * wgs_per_row + j
    return SimpleNamespace(wg_start=start, wg_map=wm)


# ------------------------------------------------------------------------------------------------------------------ 8. dense_users
DENSE_N_SB = (32, 33, 70)
DENSE_ROWS = 8                                                          # rows per sampled group; four groups


def dense_sampled_rows(n_sb):
    """the 32 sampled superblocks: four groups of eight rows, evenly spaced over the n_sb // 8 whole groups"""
    groups = n_sb // DENSE_ROWS
    return np.concatenate([np.arange(DENSE_ROWS) + (groups * j // 4) * DENSE_ROWS for j in range(4)])


def dense_inputs(n_sb, n_users, layout, limit, seed):
    """A table whose sampled entries sit 0.5 above or below thr - e(u, s): ten error widths are below 1e-3 here (every quantity is O(1) and
    e is inflated by at most 0.3 %), so the kept count is decided in float64.  Unsampled entries are +inf (they would count as kept)."""
    rng = np.random.default_rng(5150 + seed + n_sb)
    stride, offset = layout_of(n_users, layout)
    user_err = np.stack([np.exp(rng.uniform(-1, 1, n_users)), rng.uniform(0.001, 0.02, n_users), rng.uniform(0, 0.01, n_users),
                         rng.uniform(0.001, 0.01, n_users)], axis=1).astype(F32)          # {|x|, |x - a q|, cu, a}
    sb_stats = np.stack([rng.uniform(0.001, 0.01, n_sb), rng.uniform(0.5, 2, n_sb), rng.uniform(0.001, 0.02, n_sb),
                         rng.uniform(0, 0.5, n_sb)], axis=1).astype(F32)                  # {b_s, |yh|, |dy|, db}
    thr = rng.standard_normal(n_users).astype(F32)
    kdim = 64
    ck = (kdim + 6) * (2.0 ** -24 + 2.0 ** -22)
    ue, ss = user_err.astype(np.float64), sb_stats.astype(np.float64)
    e = ue[None, :, 0] * (ss[:, None, 2] + ck * ss[:, None, 1]) + ue[None, :, 1] * ss[:, None, 1] + ue[None, :, 3] * ss[:, None, 3] + ue[None, :, 2]
    rows = dense_sampled_rows(n_sb)
    n_keep = rng.integers(0, 33, size=n_users)
    n_keep[::5] = limit
    n_keep[1::5] = limit - 1
    keep = np.zeros((n_sb, n_users), dtype=bool)
    for u in range(n_users):
        keep[rows[rng.permutation(32)[:n_keep[u]]], u] = True
    flat = np.full(n_sb * stride + offset, np.nan, dtype=F32)
    table = flat[offset:].reshape(n_sb, stride)
    table[:, :n_users] = (thr[None, :].astype(np.float64) - e + np.where(keep, 0.5, -0.5)).astype(F32)
    unsampled = np.setdiff1d(np.arange(n_sb), rows)
    table[unsampled, :n_users] = PINF
    cand_floor = rng.standard_normal(n_users).astype(F32)
    cand_floor[2::7] = PINF
    thr = thr.copy()
    thr[3::11] = PINF                                                  # a +inf threshold keeps nothing
    n_keep = np.where(np.isinf(thr), 0, n_keep)
    flag_in = (rng.random(n_users) < 0.3).astype(I32)
    return SimpleNamespace(flat=flat, offset=offset, stride=stride, table=table, thr=thr, user_err=user_err, sb_stats=sb_stats, kdim=kdim,
                           n_keep=n_keep, cand_floor=cand_floor, flag_in=flag_in, n_flagged_in=3, limit=limit, n_sb=n_sb, n_users=n_users)


def dense_users(inp, bug=None):
    limit = inp.limit + (1 if bug == "limit_off_by_one" else 0)
    hit = (inp.n_keep >= limit) & (inp.cand_floor < PINF)
    cf = np.where(hit, PINF, inp.cand_floor).astype(F32)
    flag = np.where(hit, 1, inp.flag_in).astype(I32)
    return SimpleNamespace(cand_floor=cf, flag=flag, n_flagged=inp.n_flagged_in + int((hit & (inp.flag_in == 0)).sum()))


# ------------------------------------------------------------------------------------------------------------------ 9. grouping glue
SCAN_NS = (1, 1023, 1024, 1025, 262144 + 1025)
FILL_CASES = tuple(SimpleNamespace(n_sb=n_sb, rows_wg=rw, row_bytes=rb, extras=ex)
                   for n_sb, rw, rb, ex in ((5, 4, 16, True), (5, 256, 512, False), (2048, 4, 512, True), (2048, 256, 16, False),
                                            (2049, 4, 16, False), (2049, 256, 512, True)))


def group_keys(sel, sel_max, floor, k):
    """keys[i] = sel[i], or -1 for empty slots and (floor given) for superblocks with sel_max < floor[i // k]; sel_max is [k][n / k]"""
    sel = np.asarray(sel).reshape(-1)
    keep = sel >= 0
    if floor is not None:
        keep &= ~(np.asarray(sel_max).T.reshape(-1) < np.repeat(floor, k))
    return np.where(keep, sel, -1).astype(I32)


def pad_counts(indptr_t, n_sb, rows_wg):
    """cnt_pad [n_sb + 1]: every group rounded up to whole workgroups; the dummy bucket n_sb is 0"""
    c = np.diff(np.asarray(indptr_t, dtype=np.int64)[:n_sb + 1])
    return np.concatenate([(c + rows_wg - 1) // rows_wg * rows_wg, [0]]).astype(I32)


def exclusive_scan(counts):
    """out [n + 1] int64"""
    return np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=np.int64))]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def fill_inputs(ci):
    """about 40 non-empty groups with empty ones at the start, in the middle and at the end; group sizes around rows_wg (below, equal,
    above); users_op [n_users][row_bytes] random bytes"""
    c = FILL_CASES[ci]
    rng = np.random.default_rng(80 + ci)
    n_users = 97
    cnt = np.zeros(c.n_sb + 1, dtype=np.int64)                          # (the dummy bucket n_sb stays empty here)
    if c.n_sb == 5:
        cnt[[1, 3]] = [c.rows_wg + 1, 3]                               # empty: 0, 2, 4
    else:
        live = np.unique(np.concatenate([rng.integers(3, c.n_sb - 3, size=40), [c.n_sb - 4, 3, 1030 if c.n_sb > 1040 else 5]]))
        cnt[live] = rng.choice([1, c.rows_wg - 1, c.rows_wg, c.rows_wg + 1, 2 * c.rows_wg], size=len(live))
    indptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)     # [n_sb + 2]
    n_e = int(indptr[-1])
    users_t = rng.integers(0, n_users, size=n_e).astype(I32)
    perm_t = rng.permutation(n_e).astype(I32)
    cp = pad_counts(indptr, c.n_sb, c.rows_wg)
    pstart = exclusive_scan(cp)
    max_rows = int(pstart[-1]) + 3 * c.rows_wg                          # beyond the padded total
    users_op = rng.integers(0, 256, size=(n_users, c.row_bytes), dtype=np.uint8)
    users_op[0] = 0xAB                                                  # user 0's row: what padding rows copy
    ub, usq, ut = (rng.standard_normal(n_users).astype(F32) for _ in range(3))
    return SimpleNamespace(case=c, n_users=n_users, indptr=indptr, users_t=users_t, perm_t=perm_t, cnt_pad=cp, pstart=pstart,
                           max_rows=max_rows, users_op=users_op, user_bias=ub, user_sq=usq, user_tau=ut)


def fill_groups(inp, bug=None):
    """row v of the grouped layout: its superblock sb (the group whose padded range holds v), entry o = v - pstart[sb]; o < the group's
    count: user users_t[e], pair perm_t[e]; else a padding row: a copy of user 0, pair -1, g_tau +inf.  Rows at or beyond the padded total
    are padding rows too.  rblock_chunk[w] = the superblock of workgroup w's rows, -1 beyond the padded total.
    row_user is the index form's output (-1 for padding rows)."""
    c = inp.case
    total = int(inp.pstart[c.n_sb])
    v = np.arange(inp.max_rows, dtype=np.int64)
    sb = np.searchsorted(inp.pstart[:c.n_sb], v, side="right") - 1
    o = v - inp.pstart[sb]
    real = (v < total) & (o < (inp.indptr[sb + 1] - inp.indptr[sb]))
    e = np.where(real, inp.indptr[sb] + o, 0)
    user = np.where(real, inp.users_t[e], 0)
    pair = np.where(real, inp.perm_t[e], -1).astype(I32)
    g_tau = np.where(real, inp.user_tau[user], PINF).astype(F32)
    if bug == "finite_pad_tau":
        g_tau = inp.user_tau[user]
    rb = np.where(v[::c.rows_wg] < total, sb[::c.rows_wg], -1).astype(I32)
    if bug == "chunk_beyond_total":
        rb = sb[::c.rows_wg].astype(I32)
    return SimpleNamespace(G=inp.users_op[user], g_bias=inp.user_bias[user], g_sq=inp.user_sq[user], g_tau=g_tau, row_pair=pair,
                           rblock_chunk=rb, row_user=np.where(real, user, -1).astype(I32))


# ------------------------------------------------------------------------------------------------------------------ 11. exclusion lists
EXCLUDE_KF = (1, 64, 65, 130)


@functools.lru_cache(maxsize=None)
def exclude_inputs(kf, n_users=37, n_items=400):
    """exact top-kf lists (value desc, index asc; ties present) ending in -1 places for some users, an exclusion CSR with empty rows, rows
    that exclude the whole list, and a `rows` indirection (a permutation)"""
    rng = np.random.default_rng(1100 + kf)
    vals = np.full((n_users, kf), NINF, dtype=F32)
    idx = np.full((n_users, kf), -1, dtype=I32)
    ex = []
    for u in range(n_users):
        m = kf if u % 3 else int(rng.integers(0, kf + 1))              # entries before the -1 places
        ids = rng.permutation(n_items)[:m]
        v = np.round(rng.standard_normal(m) * 2).astype(F32) / F32(2)
        o = np.lexsort((ids, -v))
        vals[u, :m], idx[u, :m] = v[o], ids[o]
        if u % 5 == 0:
            e = np.array([], dtype=np.int64)
        elif u % 5 == 1:
            e = np.unique(np.concatenate([ids, rng.integers(0, n_items, 5)]))          # the whole list excluded
        else:
            e = np.unique(np.concatenate([ids[rng.random(m) < 0.4], rng.integers(0, n_items, 7)]))
        ex.append(e.astype(I32))
    perm = rng.permutation(n_users)                                     # CSR row rows[u] = perm[u] holds user u's exclusions
    by_row = [None] * n_users
    for u in range(n_users):
        by_row[perm[u]] = ex[u]
    ptr_rows = np.concatenate([[0], np.cumsum([len(e) for e in by_row])]).astype(np.int64)
    ptr_id = np.concatenate([[0], np.cumsum([len(e) for e in ex])]).astype(np.int64)
    return SimpleNamespace(vals=vals, idx=idx, ex=ex, rows=perm.astype(I32), ex_ptr_rows=ptr_rows, ex_idx_rows=np.concatenate(by_row).astype(I32),
                           ex_ptr=ptr_id, ex_idx=np.concatenate(ex).astype(I32), kf=kf, n_users=n_users)


def exclude_filter_topk(vals, idx, ex, k, bug=None):
    """the first k non-excluded entries of every list in order, (-inf, -1) behind them; flag = fewer than k survivors AND a real last entry"""
    n, kf = idx.shape
    ov = np.full((n, k), NINF, dtype=F32)
    oi = np.full((n, k), -1, dtype=I32)
    flag = np.zeros(n, dtype=I32)
    for u in range(n):
        keep = (idx[u] >= 0) & ~np.isin(idx[u], ex[u])
        s = np.nonzero(keep)[0][:k]
        ov[u, :len(s)], oi[u, :len(s)] = vals[u, s], idx[u, s]
        flag[u] = int(keep.sum() < k and (idx[u, kf - 1] >= 0 or bug == "flag_short_lists"))
    return SimpleNamespace(vals=ov, idx=oi, flag=flag, n_flagged=int(flag.sum()))


@functools.lru_cache(maxsize=None)
def rank_adjust_inputs(n_users=41, n_items=300):
    """pairs grouped by user, exclusion rows with scores; half-integer scores, so ties on both sides of the target's index abound;
    users without pairs, users without exclusions"""
    rng = np.random.default_rng(1212)
    score = (np.round(rng.standard_normal((n_users, n_items)) * 2) / 2).astype(F32)
    pp, t_idx, ee, e_idx = [0], [], [0], []
    for u in range(n_users):
        npair = 0 if u % 6 == 1 else int(rng.integers(1, 80))
        nex = 0 if u % 6 == 2 else int(rng.integers(1, 90))
        t_idx.append(rng.integers(0, n_items, npair))
        e_idx.append(np.sort(rng.permutation(n_items)[:nex]))
        pp.append(pp[-1] + npair)
        ee.append(ee[-1] + nex)
    t_idx, e_idx = np.concatenate(t_idx).astype(I32), np.concatenate(e_idx).astype(I32)
    pu = np.repeat(np.arange(n_users), np.diff(pp))
    eu = np.repeat(np.arange(n_users), np.diff(ee))
    counts = rng.integers(100, 400, size=len(t_idx)).astype(I32)
    return SimpleNamespace(pair_ptr=np.array(pp, np.int64), t_idx=t_idx, t_score=score[pu, t_idx], ex_ptr=np.array(ee, np.int64),
                           ex_idx=e_idx, ex_score=score[eu, e_idx], counts=counts, n_users=n_users)


def exclude_rank_adjust(inp, bug=None):
    """counts[p] -= #{x in E_u : s_x > s_t or (s_x == s_t and x < t)}"""
    out = inp.counts.copy()
    for u in range(inp.n_users):
        e0, e1 = inp.ex_ptr[u], inp.ex_ptr[u + 1]
        xs, xi = inp.ex_score[e0:e1], inp.ex_idx[e0:e1]
        for p in range(inp.pair_ptr[u], inp.pair_ptr[u + 1]):
            t, s = inp.t_idx[p], inp.t_score[p]
            tie = (xi > t) if bug == "tie_reversed" else (xi < t)
            out[p] -= int(((xs > s) | ((xs == s) & tie)).sum())
    return out


# ------------------------------------------------------------------------------------------------------------------ 10. euclid_certify
EUCLID_USERS, EUCLID_ITEMS = 600, 400
EUCLID_DS = (5, 64)
EUCLID_KC_K = ((16, 10), (16, 12), (32, 24), (64, 48))
EUCLID_DATA = ("separated", "near_ties", "ties")


@functools.lru_cache(maxsize=None)
def euclid_data(kind, d):
    """users, items, biases of a catalogue small enough to score whole.  separated: item radii 1, 1.05, 1.10, ... around users near the origin, so the distances of a
    user's nearest items differ by per cents; near_ties: items in a ball of 1e-3 around one point, biases of the size of the distance gaps;
    ties: small integer rows and biases that are multiples of 1 / 4"""
    rng = np.random.default_rng({"separated": 1, "near_ties": 2, "ties": 3}[kind] * 100 + d)
    nu, ni = EUCLID_USERS, EUCLID_ITEMS
    if kind == "separated":
        u = rng.standard_normal((nu, d)) * 0.05
        dirs = rng.standard_normal((ni, d))
        v = dirs / np.linalg.norm(dirs, axis=1, keepdims=True) * (1.0 + 0.05 * np.arange(ni))[rng.permutation(ni), None]
        ub, ib = rng.standard_normal(nu) * 0.1, rng.standard_normal(ni) * 0.002
    elif kind == "near_ties":
        u = rng.standard_normal((nu, d))
        v = rng.standard_normal((1, d)) + rng.standard_normal((ni, d)) * 1e-3
        ub, ib = rng.standard_normal(nu) * 0.1, rng.standard_normal(ni) * 1e-3
    else:
        u = rng.integers(-2, 3, size=(nu, d)).astype(np.float64)
        v = rng.integers(-2, 3, size=(ni, d)).astype(np.float64)
        ub, ib = rng.integers(-2, 3, size=nu) / 4.0, rng.integers(-2, 3, size=ni) / 4.0
    u, v, ub, ib = (np.ascontiguousarray(a, dtype=F32) for a in (u, v, ub, ib))
    r_u = np.sum(u * u, axis=1, dtype=F32)
    r_i = np.sum(v * v, axis=1, dtype=F32)
    for a in (u, v, ub, ib, r_u, r_i):
        a.setflags(write=False)
    return SimpleNamespace(u=u, v=v, ub=ub, ib=ib, r_u=r_u, r_i=r_i, d=d, kind=kind)


def euclid_lambda(data, positive):
    """0, or a measured-style weight: the median distance from a user to its items"""
    if not positive:
        return F32(0.0)
    dist = np.sqrt(np.maximum(data.r_u[:, None].astype(np.float64) - 2 * data.u.astype(np.float64) @ data.v.astype(np.float64).T + data.r_i[None, :], 0))
    return F32(np.median(dist))


def euclid_candidates(data, kc, lam):
    """the kc largest h = u.i - r_i / 2 + lambda b_i per user (float64, ties by id), as the cascade would hand them over: ids, float32
    values descending, and the item side's maxima {max |v|, -, max |-r_i / 2 + lambda b_i|}"""
    term = -0.5 * data.r_i.astype(np.float64) + float(lam) * data.ib.astype(np.float64)
    h = data.u.astype(np.float64) @ data.v.astype(np.float64).T + term[None, :]
    order = np.argsort(-h, axis=1, kind="stable")[:, :kc]
    g = np.take_along_axis(h, order, axis=1).astype(F32)
    gstats = np.array([np.sqrt(data.r_i.astype(np.float64).max()) * (1 + 1e-6), 0.0, np.abs(term).max() * (1 + 1e-6)], dtype=F32)
    return order.astype(I32), g, gstats


def order_by_score(scores, ids, k):
    """the first k of every row by (score desc, id asc); entries with id < 0 last, written (-inf, -1)"""
    n = scores.shape[0]
    ov = np.full((n, k), NINF, dtype=F32)
    oi = np.full((n, k), -1, dtype=I32)
    for u in range(n):
        real = np.nonzero(ids[u] >= 0)[0]
        o = real[np.lexsort((ids[u, real], -scores[u, real].astype(np.float64)))][:k]
        ov[u, :len(o)], oi[u, :len(o)] = scores[u, o], ids[u, o]
    return ov, oi


def euclid_upper_bound(data, g_last, lam):
    """the header's bound on the score of an item outside the candidates, in float64 and without any slack:
    b_u + max(phi(b_min), phi(b_max), the kink if inside), phi(b) = b - sqrt(max(r_u - 2 H + 2 lambda b, 0))"""
    c = data.r_u.astype(np.float64) - 2.0 * g_last.astype(np.float64)
    lam = float(lam)
    bmin, bmax = float(data.ib.min()), float(data.ib.max())
    phi = lambda b: b - np.sqrt(np.maximum(c + 2 * lam * b, 0))
    best = np.maximum(phi(bmin), phi(bmax))
    if lam > 0:
        bk = -c / (2 * lam)
        best = np.where((bk > bmin) & (bk < bmax), np.maximum(best, bk), best)
    return best + data.ub.astype(np.float64), np.sqrt(np.maximum(c, 0))


def euclid_must_certify(data, exact_kth, g_last, lam):
    """users whose k-th best candidate score exceeds the bound by 1e-3 of its magnitude (the bias, the distance term and the user bias):
    the kernel's slack is orders of magnitude smaller, so these must not be flagged"""
    ub, root = euclid_upper_bound(data, g_last, lam)
    mag = np.abs(ub) + root + np.abs(data.ub) + float(np.abs(data.ib).max())
    return exact_kth.astype(np.float64) > ub + 1e-3 * mag
