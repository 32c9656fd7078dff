"""NumPy reference of the int8 pre-filter: csrc/score_blockmax_i8.hip, the int8 image of csrc/user_prep.hip and the bound i8_pair_err of
csrc/score_common.hpp, restated from the kernels' comments and include/tensorrec_hip.h.  Nothing of the code under test is imported.
tests/test_i8_reference_host.py holds this module to second formulations and shows its acceptance helpers rejecting planted errors;
tests/test_gpu_i8_stage.py holds every kernel instantiation to it.

What is exact and what is not
-----------------------------
Everything the stage computes from its int8 operands is held to bit-for-bit equality:
* quantisation q = clip(rint(x * (1 / scale)), +-127): three float32 operations, each correctly rounded on both sides (NaN -> 0);
* the scales: max |y| / 127, min(clip_sigmas * rms, max |x|) / 127 (one float32 division of a maximum, which is order independent;
  the rms is a float64 sum whose rounding cannot move the float32 result except by a 1e-8 coincidence);
* integer biases rint(b / (a_c * b_s)) and their error maxima (float32 operation for operation; a maximum has no order);
* the table: the integer maximum is exact (|q . q| <= 127^2 * 128 < 2^21, |bias_q| <= 2^30: the float64 matmul holds every partial sum
  exactly), then float32(m) * float32(a_u * b_s) and + b_u are single roundings;
* i8_pair_err, the lower bounds and the sorted lists (the file is built with -ffp-contract=off: every operation rounds on its own);
* lb_tag: integer arithmetic on the float's bits.

The row norms are the exception.  The device accumulates sum x^2 and sum (x - scale q)^2 as float32 fmaf chains (at most 8 per lane) followed by
log2(G) <= 5 butterfly additions and one square root; the reference computes both in float64 from the same float32 inputs.  With
u = 2^-24 every term of the device's sum passes through at most 13 roundings of non-negative partial sums, so the sum is within
13 u relative, the root within 7.5 u: below (kpad + 4) u for every kpad >= 8, which is the tolerance used for ||x|| (it grows with K like
the chain does; the issue that introduced this file fixes the form).  For ||x - scale q|| the device also rounds the product q * scale
before it subtracts: every element of the error vector moves by at most u |q scale| (+ u |err| for the subtraction, inside the relative
term), the vector's norm by at most u ||q scale|| <= u (||x|| + ||err||) -- charged as an absolute 2^-23 ||x|| (twice the worst case, since
||err|| <= ||x|| whenever the scale is sane).  Non-finite rows must be non-finite in the same way (NaN as NaN, inf as inf).
"""
import zlib
from types import SimpleNamespace

import numpy as np

F32 = np.float32
U24 = 2.0 ** -24
BNQ = 128                                   # item rows per tile
NWQ = 4                                     # waves per workgroup
KTS = (64, 128)
LISTS = ((0, 12), (10, 12), (16, 8))        # (list slots TK, 16-user blocks per wave NUB)
BIASES = ("none", "user", "item", "both")
LAYOUTS = ("one_scale", "classes")
N_CLASSES = 64
BQ_MAX = 1 << 30
TAG_BITS = 12
GARBAGE_BQ = 999_999_999                    # rows of bias_q nobody may read (a maximum that saw one is off by ~1e9 units)


def f64(a):
    return np.asarray(a, np.float64)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    bad = bits(got) != bits(want) if got.dtype == F32 else got != want
    if bad.any():
        at = tuple(int(i) for i in np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d entries differ, first at %s: got %r, expected %r"
                             % (what, int(bad.sum()), bad.size, at, got[at], want[at]))


# ------------------------------------------------------------------------------------------------ geometry
def rows_per_workgroup(tk):
    """users of one int8 workgroup: 4 waves x NUB blocks x 16"""
    return NWQ * (12 if tk <= 10 else 8) * 16


def chunks(n_items, n_chunks, sb_rows):
    """(chunk length in items, chunks the launch really has): chunks are whole superblocks"""
    per = -(-n_items // n_chunks)
    chunk_len = -(-per // sb_rows) * sb_rows
    return chunk_len, -(-n_items // chunk_len)


def n_superblocks(n, sb_rows):
    return -(-n // sb_rows)


def kpad_of(d):
    """trec_score_kpad"""
    for kp in (32, 64, 128, 256):
        if d <= kp:
            return kp
    raise ValueError(d)


def prep_lanes(kpad):
    """G of prep_i8_kernel<G> for a kpad the entry points accept"""
    assert kpad % 4 == 0 and (kpad <= 64 or kpad == 128)
    return 32 if kpad == 128 else (16 if kpad == 64 else 8)


def natscale_lanes(d):
    kp = (d + 3) // 4 * 4
    return 32 if kp > 64 else (16 if kp > 32 else 8)


# ------------------------------------------------------------------------------------------------ quantisation
def rows_of_superblocks(per_sb, n, sb_rows):
    return np.repeat(np.asarray(per_sb), sb_rows)[:n]


def rows_of_workgroups(per_wg, n, wg_rows):
    return np.repeat(np.asarray(per_wg), wg_rows)[:n]


def quantise(x, scale_rows, kpad):
    """int8 [n, kpad] = clip(rint(x * (1 / scale)), +-127), zero padded, NaN -> 0; scale_rows: a scalar or one float32 per row"""
    x = np.asarray(x, F32)
    n, d = x.shape
    scale_rows = np.broadcast_to(np.asarray(scale_rows, F32).reshape(-1), (n,)) if np.ndim(scale_rows) else np.full((n,), scale_rows, F32)
    with np.errstate(all="ignore"):
        inv = F32(1) / scale_rows
        q = np.rint(x * inv[:, None])
    assert q.dtype == F32
    q = np.where(np.isnan(q), F32(0), q)
    q = np.clip(q, F32(-127), F32(127))
    out = np.zeros((n, kpad), np.int8)
    out[:, :d] = q.astype(np.int8)
    return out


def row_stats(x, q, scale_rows):
    """float64 [n, 2] = {||x||, ||x - scale q||} from the float32 inputs"""
    x = np.asarray(x, F32)
    n, d = x.shape
    s = np.broadcast_to(f64(np.asarray(scale_rows, F32)).reshape(-1), (n,)) if np.ndim(scale_rows) else np.full((n,), float(F32(scale_rows)))
    with np.errstate(all="ignore"):
        xd = f64(x)
        r = xd - s[:, None] * f64(q[:, :d])
        return np.stack([np.sqrt((xd * xd).sum(1)), np.sqrt((r * r).sum(1))], 1)


def norm_tolerances(stats64, kpad):
    """[n, 2] absolute tolerances of the device's float32 norms against row_stats (derivation: module docstring)"""
    rel = (kpad + 4) * U24
    with np.errstate(all="ignore"):
        return np.stack([rel * stats64[:, 0], rel * stats64[:, 1] + 2.0 ** -23 * stats64[:, 0]], 1)


def check_norms(got, stats64, kpad, what):
    """device row statistics [n, 2] float32 against the float64 norms; returns the largest error / tolerance"""
    got = np.asarray(got)
    assert got.dtype == F32 and got.shape == stats64.shape, what
    fin = np.isfinite(stats64)
    assert np.array_equal(np.isnan(got), np.isnan(stats64)), "%s: NaN rows differ" % what
    assert np.array_equal(np.isinf(got), np.isinf(stats64)), "%s: inf rows differ" % what
    tol = norm_tolerances(stats64, kpad)
    err = np.abs(f64(got)[fin] - stats64[fin])
    t = tol[fin]
    bad = err > t
    if bad.any():
        raise AssertionError("%s: %d norms beyond the tolerance, worst error / tolerance %.3g"
                             % (what, int(bad.sum()), float((err[bad] / np.maximum(t[bad], 1e-300)).max())))
    nz = t > 0
    return float((err[nz] / t[nz]).max()) if nz.any() else 0.0


# ------------------------------------------------------------------------------------------------ scales
def _absmax(a):
    """max |a| with 'NaN sticks, then turns inf'"""
    a = np.abs(np.asarray(a, F32))
    if a.size == 0:
        return F32(0)
    return F32(np.inf) if np.isnan(a).any() else a.max()


def _sane(s):
    return s if (s > 0 and s < np.inf) else F32(1)


def item_scales(y, sb_rows):
    """b_s = max |y| / 127 per superblock in float32; 1.0 for an all-zero or non-finite superblock"""
    y = np.asarray(y, F32)
    n_sb = n_superblocks(len(y), sb_rows)
    return np.array([_sane(_absmax(y[s * sb_rows:(s + 1) * sb_rows]) / F32(127)) for s in range(n_sb)], F32)


def sb_reduce(stats32, sb_rows):
    """[n_sb, 2] float32 = {max (||y|| + ||dy||), max ||dy||} over a superblock's rows (float32 addition, NaN -> inf)"""
    st = np.asarray(stats32, F32)
    with np.errstate(all="ignore"):
        a, b = st[:, 0] + st[:, 1], st[:, 1].copy()
    a[np.isnan(a)] = np.inf
    b[np.isnan(b)] = np.inf
    at = np.arange(0, len(st), sb_rows)
    return np.stack([np.maximum(np.maximum.reduceat(a, at), F32(0)), np.maximum(np.maximum.reduceat(b, at), F32(0))], 1).astype(F32)


def user_scale(x, clip_sigmas):
    """the users' one scale: min(clip_sigmas * rms, max |x|) / 127; rms in float64; clip_sigmas <= 0: nothing clips"""
    x = np.asarray(x, F32)
    with np.errstate(all="ignore"):
        xd = f64(x)
        rms = np.sqrt((xd * xd).sum() / float(x.size))
        top = _absmax(x)
        if clip_sigmas > 0:
            c = F32(float(F32(clip_sigmas)) * rms)
            if c < top:
                top = c
        return F32(_sane(F32(top) / F32(127)))


def row_scale(x):
    """trec_score_row_scale_i8: (nat [n] float32, decided [n] bool, gmax).  nat = the best of max |x| / 127, half and a quarter of it by the
    quantisation error each leaves (the first wins ties, the half wins a tie with the quarter); decided: the choice is not a near-tie (the
    kernel sums the errors in float32 in lane order, the reference in float64).  (Read from the arithmetic, not asserted anywhere: at the
    unclipped scale s every element errs by at most s / 2, d s^2 / 4 in all, while a halved scale clips the largest element by 127 s / 2 --
    for d <= 256 the first candidate always wins and nat = max |x| / 127; the tests hold the kernel to the three-way rule as written.)"""
    x = np.asarray(x, F32)
    am = np.abs(x).max(axis=1)
    best = am / F32(127)
    errs = []
    with np.errstate(all="ignore"):
        for f in (F32(1), F32(0.5), F32(0.25)):
            sc = (best * f)[:, None]
            q = np.clip(np.rint(x * (F32(1) / sc)), F32(-127), F32(127))
            r = x - q * sc
            assert r.dtype == F32
            errs.append((f64(r) ** 2).sum(axis=1))
    e0, e1, e2 = errs
    half = (e1 < e0) & (e1 <= e2)
    quarter = ~half & (e2 < e0) & (e2 < e1)
    nat = np.where(half, best * F32(0.5), np.where(quarter, best * F32(0.25), best)).astype(F32)
    nat = np.where(am > 0, nat, F32(0)).astype(F32)

    def far(a, b):
        return np.abs(a - b) > 1e-3 * np.maximum(np.maximum(a, b), 1e-30)
    decided = (far(e0, e1) & far(e0, e2) & far(e1, e2)) | (am == 0)
    return nat, decided, (nat.max() if len(nat) else F32(0))


def user_layout(nat, wg_rows):
    """The class layout of csrc/user_prep.hip restated (host tests only: float32 log2 / exp2 may differ from the device's in the last bit):
    classes clamp(floor(4 log2(gmax / nat)), 0, 63), a stable sort by class, bands of two classes padded to whole workgroups, every workgroup
    with the scale of the class of its first row.  Returns src [n_pad] (-1: padding), wg_scale, wg_class, ladder, class_used."""
    nat = np.asarray(nat, F32)
    g = F32(nat.max()) if nat.max() > 0 else F32(1)
    with np.errstate(all="ignore"):
        cls = np.floor(F32(4) * np.log2(g / nat))
    cls = np.nan_to_num(np.clip(cls, 0, N_CLASSES - 1), nan=0.0).astype(np.int64)
    ladder = (g * np.exp2(-np.arange(N_CLASSES, dtype=F32) / F32(4))).astype(F32)
    src, wg_scale, wg_class = [], [], []
    for b in range(N_CLASSES // 2):
        first = np.flatnonzero(cls == 2 * b)
        rows = np.concatenate([first, np.flatnonzero(cls == 2 * b + 1)])
        if not len(rows):
            continue
        pad = -(-len(rows) // wg_rows) * wg_rows
        src.append(np.concatenate([rows, np.full(pad - len(rows), -1, np.int64)]))
        for w in range(pad // wg_rows):
            c = 2 * b if w * wg_rows < len(first) else 2 * b + 1
            wg_class.append(c)
            wg_scale.append(ladder[c])
    wg_class = np.array(wg_class, np.int32)
    used = np.zeros(N_CLASSES, np.int32)
    used[wg_class] = 1
    return np.concatenate(src), np.array(wg_scale, F32), wg_class, ladder, used


# ------------------------------------------------------------------------------------------------ integer biases
def bias_classes(bias, sb_scales, sb_rows, ladder, class_used=None):
    """(bias_q {class: int32 [n]}, sb3 [n_sb] float32, gmax |b|): bias_q[c][i] = clip(rint(b / (a_c * b_s)), +-2^30) with the product formed in
    float32; sb3[s] = max over the classes in use of (max |b - sp bq| / a_c) * 1.0000005; one class without class_used (ladder = [a])."""
    b = np.asarray(bias, F32)
    n = len(b)
    ladder = np.asarray(ladder, F32).reshape(-1)
    used = range(len(ladder)) if class_used is None else [int(c) for c in np.flatnonzero(np.asarray(class_used))]
    b_row = rows_of_superblocks(np.asarray(sb_scales, F32), n, sb_rows)
    at = np.arange(0, n, sb_rows)
    sb3 = np.zeros(len(at), F32)
    out = {}
    with np.errstate(all="ignore"):
        for c in used:
            sp = ladder[c] * b_row
            t = np.rint(b / sp)
            assert sp.dtype == F32 and t.dtype == F32
            t = np.where(np.isnan(t), F32(0), t)
            t = np.clip(t, F32(-BQ_MAX), F32(BQ_MAX))
            out[c] = t.astype(np.int64).astype(np.int32)
            a3 = np.abs(b - t * sp)
            a3[np.isnan(a3)] = np.inf
            rel = (np.maximum(np.maximum.reduceat(a3, at), F32(0)) / ladder[c]) * F32(1.0000005)
            rel = np.where(np.isnan(rel), F32(np.inf), rel).astype(F32)
            sb3 = np.maximum(sb3, rel)
    return out, sb3, _absmax(b)


def ck_of(kdim):
    return F32(kdim + 6) * F32(2.98023224e-07)


def user_err(ustats32, user_bias, g2, kdim, a_u):
    """r_err [n, 4] float32 = {nx, ex, ck (|b_u| + gstats[2]), a_u}"""
    st = np.asarray(ustats32, F32)
    n = len(st)
    bu = np.abs(np.asarray(user_bias, F32)) if user_bias is not None else np.zeros(n, F32)
    out = np.empty((n, 4), F32)
    out[:, 0], out[:, 1] = st[:, 0], st[:, 1]
    with np.errstate(all="ignore"):
        out[:, 2] = ck_of(kdim) * (bu + F32(g2))
    out[:, 3] = np.broadcast_to(np.asarray(a_u, F32), (n,))
    return out


# ------------------------------------------------------------------------------------------------ the bound, the lists, the tags
def pair_err(nx, ex, cu, yh, dy, db, kdim):
    """i8_pair_err (csrc/score_common.hpp) in float32, operation for operation"""
    args = [np.asarray(a, F32) for a in (nx, ex, cu, yh, dy, db)]
    nx, ex, cu, yh, dy, db = args
    ck = ck_of(kdim)
    with np.errstate(all="ignore"):
        e = nx * (dy + ck * yh) + ex * yh + db + cu
        e = e * F32(1.001953125) + F32(1e-30)
    assert e.dtype == F32
    return e


def lower_bounds(table, e):
    with np.errstate(all="ignore"):
        lb = (np.asarray(table, F32) - np.asarray(e, F32)).astype(F32)
    lb[np.isnan(lb)] = -np.inf
    return lb


def lb_key(x):
    b = bits(x).astype(np.int64)
    return np.where(b >= 0, b, -(b & 0x7FFFFFFF))


def lb_tag(lb, idx):
    lb = np.asarray(lb, F32)
    idx = np.broadcast_to(np.asarray(idx, np.int64), lb.shape)
    k2 = ((lb_key(lb) >> TAG_BITS) - 1) * (1 << TAG_BITS) + idx
    b2 = np.where(k2 >= 0, k2, 0x80000000 + (-k2)).astype(np.uint32)
    out = b2.view(F32).copy()
    with np.errstate(all="ignore"):
        out[~(np.abs(lb) < F32(1e37))] = -np.inf
    return out


def lb_tag_index(tagged):
    return lb_key(tagged) & ((1 << TAG_BITS) - 1)


def lists(lb, n_items, n_chunks, sb_rows, tk, tagged=False):
    """[n_ch, tk, n_users] float32: per chunk and user the tk largest lower bounds, descending, -inf padded"""
    lb = np.asarray(lb, F32)
    chunk_len, n_ch = chunks(n_items, n_chunks, sb_rows)
    spc = chunk_len // sb_rows
    out = np.full((n_ch, tk, lb.shape[1]), -np.inf, F32)
    for c in range(n_ch):
        blk = lb[c * spc:(c + 1) * spc]
        if tagged:
            blk = lb_tag(blk, np.arange(len(blk))[:, None])
        top = -np.sort(-blk, axis=0)[:tk]
        out[c, :len(top)] = top
    return out


def check_tagged(tg, ut, lb, n_items, n_chunks, sb_rows, what):
    """the tagged lists tg against the untagged ones ut (both [n_ch, tk, n_users]) and the lower bounds lb [n_sb, n_users]"""
    chunk_len, n_ch = chunks(n_items, n_chunks, sb_rows)
    spc = chunk_len // sb_rows
    tk, n_u = tg.shape[1], tg.shape[2]
    tag = lb_tag_index(tg)
    for c in range(n_ch):
        blk = lb[c * spc:(c + 1) * spc]
        live = np.sort(blk > -np.inf, axis=0)[::-1][:tk]                           # per user: how many entries certify something
        t, r = f64(tg[c][:len(live)]), f64(ut[c][:len(live)])
        assert np.all(np.isneginf(tg[c][len(live):])) and np.all(np.isneginf(tg[c][:len(live)][~live])), "%s: chunk %d padding" % (what, c)
        assert np.all(t[live] <= r[live]) and np.all((r - t)[live] <= np.abs(r[live]) * 2.0 ** -10 + 1e-30), "%s: chunk %d gap" % (what, c)
        src = f64(np.take_along_axis(blk, np.minimum(tag[c][:len(live)], len(blk) - 1), axis=0))
        assert np.all(tag[c][:len(live)][live] < len(blk)), "%s: chunk %d names a superblock outside the chunk" % (what, c)
        assert np.all(t[live] <= src[live]) and np.all((src - t)[live] <= np.abs(src[live]) * 2.0 ** -10 + 1e-30), "%s: chunk %d source" % (what, c)
        # lists sorted by tagged value may order two bounds within 2^-11 of each other differently: the smallest source is (nearly) the last entry
        last = np.where(live, r, np.inf).min(axis=0)
        has = live.any(axis=0)
        assert np.all(np.where(live, src, np.inf).min(axis=0)[has] >= (last - np.abs(last) * 2.0 ** -10 - 1e-30)[has]), "%s: chunk %d last" % (what, c)
        for j in range(n_u):
            tj = tag[c][:len(live), j][live[:, j]]
            assert len(np.unique(tj)) == len(tj), "%s: chunk %d user %d lists a superblock twice" % (what, c, j)


# ------------------------------------------------------------------------------------------------ acceptance of device buffers
def check_table(buf, want, written, sentinel, what):
    """buf [n_sb, bm_stride] as the kernel left it: the columns of `written` users equal `want` bit for bit, every other cell keeps the sentinel"""
    n_sb, n_u = want.shape
    assert buf.shape[0] == n_sb and buf.shape[1] >= n_u
    cols = np.flatnonzero(written)
    same_bits(buf[:, cols], want[:, cols], what)
    mask = np.ones(buf.shape, bool)
    mask[:, cols] = False
    assert np.all(bits(buf)[mask] == bits(np.full(1, sentinel, F32))[0]), "%s: a cell outside the result was overwritten" % what


def check_lists(buf, want, written, sentinel, what):
    """buf [rows, bm_stride]: rows 0 .. n_ch * tk of the `written` users equal `want` [n_ch, tk, n_users], everything else keeps the sentinel"""
    n_ch, tk, n_u = want.shape
    cols = np.flatnonzero(written)
    assert buf.shape[0] >= n_ch * tk and buf.shape[1] >= n_u
    same_bits(buf[:n_ch * tk][:, cols], want.reshape(n_ch * tk, n_u)[:, cols], what)
    mask = np.ones(buf.shape, bool)
    mask[:n_ch * tk, cols] = False
    assert np.all(bits(buf)[mask] == bits(np.full(1, sentinel, F32))[0]), "%s: a cell outside the lists was overwritten" % what


# ------------------------------------------------------------------------------------------------ the case table
def grid():
    """every instantiation blockmax_i8x16_kernel<KT, BIAS, TK, NUB> x the bias forms x the user layouts"""
    out = []
    for kt in KTS:
        for tk, nub in LISTS:
            for bias in BIASES:
                for layout in LAYOUTS:
                    out.append(SimpleNamespace(id="k%d-tk%d-%s-%s" % (kt, tk, bias, layout), kt=kt, tk=tk, nub=nub, bias=bias, layout=layout,
                                               instantiation=(kt, bias != "none", tk, nub)))
    return out


PREP_SHAPES = ((128, 128), (100, 128), (64, 64), (40, 64), (30, 32), (5, 8))          # (d, kpad) of prep_i8_kernel
NATSCALE_D = (5, 40, 64, 100, 128, 256)


def prep_grid():
    """the G = 8 / 16 / 32 forms of prep_i8_kernel (by kpad) and of row_natscale_kernel (by d)"""
    out = [SimpleNamespace(id="prep-g%d-d%d-k%d" % (prep_lanes(kp), d, kp), kernel="prep_i8_kernel", lanes=prep_lanes(kp), d=d, kpad=kp)
           for d, kp in PREP_SHAPES]
    out += [SimpleNamespace(id="natscale-g%d-d%d" % (natscale_lanes(d), d), kernel="row_natscale_kernel", lanes=natscale_lanes(d), d=d, kpad=None)
            for d in NATSCALE_D]
    return out


# ------------------------------------------------------------------------------------------------ populations of real rows
def rows(kind, n, d, rng):
    x = rng.standard_normal((n, d)).astype(F32)
    if kind == "scaled":                       # row scales over six orders of magnitude
        x *= np.exp(rng.uniform(-7, 7, size=(n, 1))).astype(F32)
    elif kind == "outliers":                   # a few huge elements: clipped under clip_sigmas 4, and rows that want to clip
        x[rng.random((n, d)) < 0.01] *= F32(60)
    elif kind == "zeros":                      # all-zero rows, and (for sb_rows 128) an all-zero superblock in front
        x[::5] = 0
        x[:min(n, 128)] = 0
    elif kind == "nonfinite":                  # one NaN and one inf element, in different rows
        x[n // 2, d // 2] = np.nan
        x[n - 1, 0] = np.inf
    else:
        assert kind == "gauss"
    return x


POPULATIONS = ("gauss", "scaled", "outliers", "zeros", "nonfinite")


# ------------------------------------------------------------------------------------------------ the stage's own operands
NU_MAX = 2 * 768 + 5
NI_MAX = 5 * 512 + 77
_POOLS = {}
WG_SCALES = (F32(2.0 ** -7), F32(1.3125 * 2.0 ** -9), F32(1.7 * 2.0 ** -11), F32(2.0 ** -12))
WG_CLASSES = (5, 63, 0, 17)


def pool(kt):
    """int8 operands over the full +-127 range shared by every case of one K, with their exact dot products.  User 0 and item 0 are all +127,
    user 1 is all -127; no 64-element k-step of any row is all zero."""
    if kt not in _POOLS:
        rng = np.random.default_rng(1000 + kt)
        uq = rng.integers(-127, 128, (NU_MAX, kt)).astype(np.int8)
        iq = rng.integers(-127, 128, (NI_MAX, kt)).astype(np.int8)
        uq[0], uq[1], iq[0] = 127, -127, 127
        _POOLS[kt] = SimpleNamespace(uq=uq, iq=iq, dots=int_dots(uq, iq))
    return _POOLS[kt]


def int_dots(uq, iq):
    """exact: |sum| < 2^21, float64 holds it"""
    return f64(uq) @ f64(iq).T


def stage_problem(case, n_users, n_items, sb_rows, idle=None):
    """Operands of one trec_score_gemm_blockmax_i8 call for a case of grid().  idle: index of a workgroup whose scale is 0 (layout classes)."""
    P = pool(case.kt)
    # (seeded without the list length: the TK = 0 and TK = 10 forms of a case get the same operands and must write the same table)
    rng = np.random.default_rng(zlib.crc32(("k%d-%s-%s/%d/%d/%d" % (case.kt, case.bias, case.layout, n_users, n_items, sb_rows)).encode()))
    W = rows_per_workgroup(case.tk)
    n_wg, n_sb = -(-n_users // W), n_superblocks(n_items, sb_rows)
    p = SimpleNamespace(case=case, kt=case.kt, tk=case.tk, n_users=n_users, n_items=n_items, sb_rows=sb_rows, n_sb=n_sb, wg_rows=W,
                        uq=P.uq[:n_users], iq=P.iq[:n_items], dots=P.dots[:n_users, :n_items])
    p.scales = np.array([1.37 * 2.0 ** -8, 0, 0], F32)
    if case.layout == "classes":
        assert n_wg <= len(WG_SCALES)
        p.wg_scale = np.array(WG_SCALES[:n_wg], F32)
        p.wg_class = np.array(WG_CLASSES[:n_wg], np.int32)
        if idle is not None:
            p.wg_scale[idle], p.wg_class[idle] = 0, -1
        p.a_u = rows_of_workgroups(p.wg_scale, n_users, W)
        p.class_u = rows_of_workgroups(p.wg_class, n_users, W).astype(np.int64)
    else:
        assert idle is None
        p.wg_scale = p.wg_class = None
        p.a_u = np.full(n_users, p.scales[0], F32)
        p.class_u = np.zeros(n_users, np.int64)
    p.written = p.a_u != 0
    p.sb_stats = np.stack([rng.uniform(0.5e-3, 2e-3, n_sb), rng.uniform(0.5, 2, n_sb), rng.uniform(1e-3, 2e-2, n_sb),
                           rng.uniform(0.01, 0.5, n_sb)], 1).astype(F32)
    p.r_err = np.stack([rng.uniform(0.5, 2, n_users), rng.uniform(1e-3, 2e-2, n_users), rng.uniform(0, 1e-3, n_users), p.a_u], 1).astype(F32)
    p.ub = (0.3 * rng.standard_normal(n_users)).astype(F32) if case.bias in ("user", "both") else None
    p.bias_q = None
    if case.bias in ("item", "both"):
        def one_row(c):
            r = rng.integers(-3000, 3001, n_items).astype(np.int32)
            r[7] = -BQ_MAX                                                   # never the maximum: the smallest accumulator
            if n_items > 100:
                r[100] = BQ_MAX - 12345 - 1000 * c                          # the maximum of its superblock is beyond 2^24: the conversion rounds
            if n_items > 1500:
                r[1500] = BQ_MAX
            return r
        if case.layout == "classes":
            p.bias_q = np.full((N_CLASSES, n_items), GARBAGE_BQ, np.int32)
            for c in sorted(set(int(c) for c in p.wg_class if c >= 0)):
                p.bias_q[c] = one_row(c)
        else:
            p.bias_q = one_row(0)
    return p


def stage_table(p, dots=None, class_u=None):
    """[n_sb, n_users] float32: float32(integer maximum) * float32(a_u * b_s) (+ b_u in the biased forms); columns of idle workgroups: no meaning"""
    dots = p.dots if dots is None else dots
    class_u = p.class_u if class_u is None else class_u
    pad = p.n_sb * p.sb_rows - p.n_items
    m = np.empty((p.n_sb, p.n_users))
    for c in np.unique(class_u):
        sel = np.flatnonzero(class_u == c)
        t = dots[sel]
        if p.bias_q is not None:
            t = t + f64(p.bias_q[max(c, 0)] if p.bias_q.ndim == 2 else p.bias_q)[None, :]
        t = np.concatenate([t, np.full((len(sel), pad), -np.inf)], 1).reshape(len(sel), p.n_sb, p.sb_rows).max(2)
        m[:, sel] = t.T
    assert np.all(np.abs(m) < 2.0 ** 31)
    sp = p.a_u[None, :] * p.sb_stats[:, 0][:, None]
    v = m.astype(F32) * sp
    assert sp.dtype == F32 and v.dtype == F32
    if p.case.bias != "none":
        v = v + (p.ub if p.ub is not None else np.zeros(p.n_users, F32))[None, :]
    return v


def stage_bound(p, r_err=None, sb_stats=None, db_with_scale=True):
    r_err = p.r_err if r_err is None else r_err
    sbs = p.sb_stats if sb_stats is None else sb_stats
    db = (p.a_u[None, :] * sbs[:, 3][:, None]) if db_with_scale else np.broadcast_to(sbs[:, 3][:, None], (p.n_sb, p.n_users))
    return pair_err(r_err[:, 0][None, :], r_err[:, 1][None, :], r_err[:, 2][None, :], sbs[:, 1][:, None], sbs[:, 2][:, None], db, p.kt)


# ------------------------------------------------------------------------------------------------ real-valued populations for the bound
def bound_population(d, big_bias, seed, n_users=2000, n_items=6 * 512 + 77):
    """users: scaled, outlier and partly zero rows (many scale classes); items: Gaussian rows of mixed size; both biases, the item biases either
    of the scores' size or 100 times it"""
    rng = np.random.default_rng(seed)
    third = n_users // 3
    x = np.concatenate([rows("scaled", third, d, rng), rows("outliers", third, d, rng), rows("zeros", n_users - 2 * third, d, rng)[::-1]])
    x = np.ascontiguousarray(x[rng.permutation(n_users)])
    y = rng.standard_normal((n_items, d)).astype(F32) * rng.uniform(0.3, 3, (n_items, 1)).astype(F32)
    ub = (0.3 * rng.standard_normal(n_users)).astype(F32)
    ib = (rng.standard_normal(n_items) * (100.0 * np.sqrt(d) if big_bias else 0.3)).astype(F32)
    return x, y, ub, ib


def observed_error(uq, iq, bias_q_of_user_rows, a_u, b_row, x, y, ub, ib, sb_rows):
    """Three [n_sb, n_users] float64 tables: the largest |a_u b_s (q_u . q_i + bq) + b_u - (x . y + b_u + b_i)| over the superblock's items (the
    right side in float64), the exact maximum, and the integer maximum.  bias_q_of_user_rows: (user rows, int [n_items]) per group of users
    of one class; a_u [n_users], b_row [n_items] float32."""
    n_u, n_i = len(uq), len(iq)
    n_sb = n_superblocks(n_i, sb_rows)
    pad = n_sb * sb_rows - n_i
    s_int = int_dots(uq, iq)
    for sel, bq in bias_q_of_user_rows:
        s_int[sel] += f64(bq)[None, :]
    s8 = s_int * f64(a_u)[:, None] * f64(b_row)[None, :] + f64(ub)[:, None]
    exact = f64(x) @ f64(y).T + f64(ub)[:, None] + f64(ib)[None, :]
    def per_sb(a, fill):
        return np.concatenate([a, np.full((n_u, pad), fill)], 1).reshape(n_u, n_sb, sb_rows).max(2).T
    return per_sb(np.abs(s8 - exact), 0.0), per_sb(exact, -np.inf), per_sb(s_int, -np.inf)


def reference_pipeline(x, y, ub, ib, k, sb_rows=512):
    """The stage's operands made by this module alone, end to end: user classes and layout, quantisation of both sides, integer biases per class,
    user error record, bound.  Returns a namespace with everything in LAYOUT order for the users (real: rows with a source)."""
    d = x.shape[1]
    kpad = kpad_of(d)
    W = rows_per_workgroup(10 if k <= 10 else 16)
    nat, _, _ = row_scale(x)
    src, wg_scale, wg_class, ladder, used = user_layout(nat, W)
    real = src >= 0
    xs = np.where(real[:, None], x[np.clip(src, 0, None)], F32(0)).astype(F32)
    ubs = np.where(real, ub[np.clip(src, 0, None)], F32(0)).astype(F32)
    a_u = rows_of_workgroups(wg_scale, len(src), W)
    uq = quantise(xs, a_u, kpad)
    ust = row_stats(xs, uq, a_u).astype(F32)
    b_s = item_scales(y, sb_rows)
    b_row = rows_of_superblocks(b_s, len(y), sb_rows)
    iq = quantise(y, b_row, kpad)
    ist = row_stats(y, iq, b_row).astype(F32)
    bq, sb3, g2 = bias_classes(ib, b_s, sb_rows, ladder, used)
    sbs = np.concatenate([b_s[:, None], sb_reduce(ist, sb_rows), sb3[:, None]], 1).astype(F32)
    r_err = user_err(ust, ubs, g2, kpad, a_u)
    e = pair_err(r_err[:, 0][None, :], r_err[:, 1][None, :], r_err[:, 2][None, :], sbs[:, 1][:, None], sbs[:, 2][:, None],
                 r_err[:, 3][None, :] * sbs[:, 3][:, None], kpad)
    class_u = rows_of_workgroups(wg_class, len(src), W)
    groups = [(np.flatnonzero(class_u == c), bq[int(c)]) for c in np.unique(class_u)]
    return SimpleNamespace(kpad=kpad, src=src, real=real, xs=xs, ubs=ubs, a_u=a_u, uq=uq, iq=iq, b_row=b_row, sbs=sbs, r_err=r_err, e=e,
                           groups=groups, wg_class=wg_class, wg_scale=wg_scale, n_classes=int(used.sum()))


def real_groups(groups, real):
    """(rows, bias_q) groups over layout rows -> the same over the real rows only, numbered in layout order"""
    inv = np.full(len(real), -1, np.int64)
    inv[np.flatnonzero(real)] = np.arange(int(real.sum()))
    return [(inv[sel][inv[sel] >= 0], bq) for sel, bq in groups]
