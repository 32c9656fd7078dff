"""Float64 reference, error bound, inputs, acceptance rules and the case table for the stage-1 score kernels (K2):
score_gemm_kernel<DT, KT, BN, NCB, EPI, GLDS, EUCLID, WPS, KTOP, BIAS> of csrc/score_gemm.hip with its STORE / TOPK / BLOCKMAX epilogues and
the hand-scheduled BLOCKMAX forms of csrc/score_blockmax.hip.  NumPy only: no torch, nothing of the code under test.
tests/test_score_reference_host.py holds the reference to the committed oracle on the CPU, shows that the acceptance rules reject planted
errors and that grid() has the size the dispatch code implies; tests/test_gpu_score_kernels.py holds the kernels to the reference.

Operands.  The tests write the padded operands themselves ([n, kpad] float32, or bf16 bit patterns as uint16 with zero padding columns), so
the kernels are judged independently of trec_score_prep.  bf16 is round-to-nearest-even on the bit pattern (bf16_bits).

Two kinds of data.
* dyadic   operands are integers in [-3, 3], biases multiples of 1/4 with |b| <= 8, squared norms the exact integers.  For K <= 256 every
           product, every partial sum in any order (|sum| <= 9 * 256 < 2^24), the squared distance and -- in dot mode -- both bias adds are
           exact in float32, and sqrtf is correctly rounded: restate32 (a float32 restatement of the documented order) is what EVERY
           instantiation, bf16 included, must return bit for bit.  The order of the bias adds:
               fp32, and every Euclidean form     (s + b_u) + b_i          (tensorrec/recommendation_graphs.py:41)
               bf16 dot                           (b_i + s) + b_u          (the item bias is the initial accumulator of the MFMA chain)
           which only matters behind the square root (everything else is exact).  User row 0 is a copy of item row DUPS[0] and the item
           rows DUPS are identical, so that user's list starts with exact ties that live in different half-wave lists, tiles and chunks; in
           Euclidean mode its distance to them is 0 and the 1e-16 clamp is hit.
* real     standard-normal rows with row scales in [0.3, 3], biases N(0, 1); distances stay far from 0 (asserted where the bound is built).
           fp32 kernels are held bit for bit to oracle.score_dense_exact / score_dense_euclid_exact (the project's bar); bf16 kernels to the
           float64 reference on the bf16-rounded operands within the bound B.

The bf16 bound (u = 2^-24, the unit roundoff of float32).  The K products of bf16 values are exact in float32; a score is K + 1 accumulator
additions (the item bias is the initial accumulator) and one more for b_u, each rounding a partial sum of magnitude at most
A = sum_k |u_k v_k| + |b_i| + |b_u|.  With 2^-23 = 2 u per addition -- twice the round-to-nearest unit, which covers the undocumented
rounding of the MFMA's internal adds --
    B = (K + 3) 2^-23 A.
Euclidean: s = -sqrt(max(dist, 1e-16)) + biases, dist = (usq - 2 dot) + vsq.  With B_dot = (K + 3) 2^-23 sum_k |u_k v_k|,
    d_dist = 2 B_dot + 3 u (usq + 2 |dot| + vsq)                     (the product by 2 is exact; two adds, one spare unit)
    d      = d_dist / (2 sqrt(dist - d_dist)) + 2^-23 |v|            (first order in the root, evaluated at the near end; sqrtf)
             + 2^-23 (|v| + |b_u| + |b_i|)                           (two bias adds of u each)
with v = -sqrt(dist); dist - d_dist > 0 is asserted (real data stays far from 0; dyadic data is held to equality, not to the bound).

Acceptance rules for results held to the bound (no user is left out of any of them): check_store, check_blockmax, check_topk_bounded."""
import functools
from types import SimpleNamespace

import numpy as np

U32 = 2.0 ** -24
F32 = np.float32
DT_F32, DT_BF16 = 0, 1
MODE_DOT, MODE_EUCLID = 0, 1
KPADS = (32, 64, 128, 256)
CAPACITIES = (8, 12, 16)
BIASES = ("none", "both", "user", "item")
CLAMP32 = np.float32(1e-16)
DUPS = (3, 40, 70)                      # identical item rows (and biases): another 32-row block, another tile; the last item joins them
DUP_USER = 0                            # ... and this user row equals them


def f64(a):
    return np.asarray(a, dtype=np.float64)


# ------------------------------------------------------------------------------------------------ launch geometry (score_cfg)
def tile_rows(dtype, kpad):
    """BN: item rows per tile (trec_score_tile_rows)"""
    return 64 if dtype == DT_BF16 else 32


def rows_per_workgroup(dtype, kpad):
    """4 waves * NCB * 32 (trec_score_rows_per_workgroup)"""
    return 256 if dtype == DT_BF16 and kpad <= 128 else 128


def topk_parts(n_items, n_chunks):
    """partial lists per user of trec_score_gemm_topk (trec_score_topk_parts): chunks are rounded to 128 rows, two half-wave lists each"""
    cl = -(-(-(-n_items // n_chunks)) // 128) * 128
    return 2 * -(-n_items // cl)


# ------------------------------------------------------------------------------------------------ bf16
def bf16_bits(x):
    """round-to-nearest-even of float32 to bfloat16, on the bit pattern (finite values)"""
    b = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(F32)


def operand(x, kpad, dtype):
    """x [n, d] -> (what the kernel reads: [n, kpad] float32 or uint16 bf16 bits, zero padding columns; its values as float32 [n, kpad])"""
    x = np.asarray(x, F32)
    n, d = x.shape
    assert d <= kpad
    val = np.zeros((n, kpad), F32)
    val[:, :d] = x
    if dtype == DT_BF16:
        bits = bf16_bits(val)
        return bits, bf16_value(bits)
    return val, val.copy()


# ------------------------------------------------------------------------------------------------ the reference
def scores(u, v, ub, ib, mode, dtype, usq=None, vsq=None):
    """(S, B): float64 scores [n_u, n_i] of the operand values u [n_u, K], v [n_i, K] and the per-element bound of the module docstring.
    usq / vsq are the arrays the test hands to the kernel (Euclidean mode): the kernel is judged, not the norm computation.
    dtype does not enter the value (the operands are already rounded); it is kept so that a call reads like the kernel's."""
    u, v = f64(u), f64(v)
    k = u.shape[1]
    dot = u @ v.T
    absdot = np.abs(u) @ np.abs(v.T)
    bu = np.zeros(u.shape[0]) if ub is None else f64(ub)
    bi = np.zeros(v.shape[0]) if ib is None else f64(ib)
    babs = np.abs(bu)[:, None] + np.abs(bi)[None, :]
    if mode == MODE_DOT:
        return dot + bu[:, None] + bi[None, :], (k + 3) * 2.0 ** -23 * (absdot + babs)
    uq, vq = f64(usq)[:, None], f64(vsq)[None, :]
    dist = uq - 2.0 * dot + vq
    val = -np.sqrt(np.maximum(dist, 1e-16))
    d_dist = 2.0 * (k + 3) * 2.0 ** -23 * absdot + 3.0 * U32 * (uq + 2.0 * np.abs(dot) + vq)
    with np.errstate(invalid="ignore", divide="ignore"):
        bound = d_dist / (2.0 * np.sqrt(dist - d_dist)) + 2.0 ** -23 * np.abs(val) + 2.0 ** -23 * (np.abs(val) + babs)
    return val + bu[:, None] + bi[None, :], bound


def restate32(u, v, ub, ib, mode, dtype, usq=None, vsq=None):
    """float32 restatement of the documented order on DYADIC data (asserted: the dot products are exact in float32)"""
    dot64 = f64(u) @ f64(v).T
    s = dot64.astype(F32)
    assert np.array_equal(f64(s), dot64) and np.abs(f64(u)).max() <= 3 and u.shape[1] <= 256, "not dyadic"
    if mode == MODE_EUCLID:
        dist = (np.asarray(usq, F32)[:, None] - F32(2.0) * s) + np.asarray(vsq, F32)[None, :]
        s = -np.sqrt(np.maximum(dist, CLAMP32))
        assert s.dtype == F32
    bu = None if ub is None else np.asarray(ub, F32)[:, None]
    bi = None if ib is None else np.asarray(ib, F32)[None, :]
    if dtype == DT_BF16 and mode == MODE_DOT:             # (b_i + s) + b_u
        if bi is not None:
            s = bi + s
        if bu is not None:
            s = s + bu
    else:                                                 # (s + b_u) + b_i
        if bu is not None:
            s = s + bu
        if bi is not None:
            s = s + bi
    return np.ascontiguousarray(np.broadcast_to(s, dot64.shape), F32)


def blockmax(s, sb_rows):
    """[n_sb, n_u]: the maximum of s [n_u, n_i] over each superblock of sb_rows items (the layout of the kernels' table)"""
    n_i = s.shape[1]
    n_sb = -(-n_i // sb_rows)
    return np.stack([s[:, b * sb_rows:min(n_i, (b + 1) * sb_rows)].max(axis=1) for b in range(n_sb)])


def topk(s, k, base=0):
    """(values [n_u, k], ids [n_u, k] int32) by value descending, index ascending; -inf / -1 where there are fewer than k items"""
    s = np.asarray(s)
    n_u, n_i = s.shape
    kk = min(k, n_i)
    order = np.argsort(-s, axis=1, kind="stable")[:, :kk]
    vals = np.full((n_u, k), -np.inf, s.dtype)
    ids = np.full((n_u, k), -1, np.int32)
    vals[:, :kk] = np.take_along_axis(s, order, axis=1)
    ids[:, :kk] = order + base
    return vals, ids


# ------------------------------------------------------------------------------------------------ inputs
class Problem(object):
    """Operands, biases and squared norms of one shape, with both biases present; select() drops one or both."""

    def __init__(self, kind, dtype, kpad, n_users, n_items, d, seed):
        rng = np.random.default_rng(seed)
        self.kind, self.dtype, self.kpad, self.n_users, self.n_items, self.d = kind, dtype, kpad, n_users, n_items, d
        self._cache = {}
        if kind == "dyadic":
            u = rng.integers(-3, 4, (n_users, d)).astype(F32)
            v = rng.integers(-3, 4, (n_items, d)).astype(F32)
            ub = (rng.integers(-32, 33, n_users) / 4.0).astype(F32)
            ib = (rng.integers(-32, 33, n_items) / 4.0).astype(F32)
            dups = [j for j in DUPS if j < n_items] + [n_items - 1]
            v[dups] = v[dups[0]]
            ib[dups] = ib[dups[0]]
            u[DUP_USER] = v[dups[0]]
            self.dups = sorted(set(dups))
        else:
            assert kind == "real"
            u = (rng.standard_normal((n_users, d)) * rng.uniform(0.3, 3.0, (n_users, 1))).astype(F32)
            v = (rng.standard_normal((n_items, d)) * rng.uniform(0.3, 3.0, (n_items, 1))).astype(F32)
            ub = rng.standard_normal(n_users).astype(F32)
            ib = rng.standard_normal(n_items).astype(F32)
        self.u_op, self.u_val = operand(u, kpad, dtype)
        self.v_op, self.v_val = operand(v, kpad, dtype)
        self.ub, self.ib = ub, ib
        self.usq = (f64(self.u_val) ** 2).sum(1).astype(F32)      # dyadic: exact integers
        self.vsq = (f64(self.v_val) ** 2).sum(1).astype(F32)
        for a in (self.u_op, self.v_op, self.u_val, self.v_val, self.ub, self.ib, self.usq, self.vsq):
            a.setflags(write=False)

    def select(self, bias):
        """(user bias, item bias) of a bias option of BIASES"""
        return (self.ub if bias in ("both", "user") else None), (self.ib if bias in ("both", "item") else None)

    def reference(self, mode, bias):
        """(S, B) float64, read-only (kept with the problem)"""
        key = ("reference", mode, bias)
        if key not in self._cache:
            ub, ib = self.select(bias)
            s, b = scores(self.u_val, self.v_val, ub, ib, mode, self.dtype, self.usq, self.vsq)
            if self.kind == "real":
                assert np.isfinite(b).all(), "a distance too close to 0 for the bound"
            s.setflags(write=False)
            b.setflags(write=False)
            self._cache[key] = (s, b)
        return self._cache[key]

    def restated(self, mode, bias):
        """float32 restatement (dyadic data), read-only (kept with the problem)"""
        key = ("restated", mode, bias)
        if key not in self._cache:
            ub, ib = self.select(bias)
            s = restate32(self.u_val, self.v_val, ub, ib, mode, self.dtype, self.usq, self.vsq)
            s.setflags(write=False)
            self._cache[key] = s
        return self._cache[key]


@functools.lru_cache(maxsize=12)
def problem(kind, dtype, kpad, n_users, n_items, d=None, seed=0):
    """the problem of a shape, computed once and shared (the last dozen are kept); the data does not depend on dtype"""
    return Problem(kind, dtype, kpad, n_users, n_items, kpad if d is None else d, 7919 * seed + 31 * kpad + n_users + n_items)


# ------------------------------------------------------------------------------------------------ acceptance rules
def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = got.view(np.int32) != want.view(np.int32) if got.dtype == F32 else got != want
    if bad.any():
        at = tuple(int(x) for x in np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d entries differ, first at %s: got %r, want %r" % (what, int(bad.sum()), bad.size, at, got[at], want[at]))


def check_padding(buf, written, sentinel, what):
    """every cell of buf outside the boolean mask `written` still holds the sentinel, bit for bit"""
    buf = np.asarray(buf)
    keep = buf[~written]
    bad = keep.view(np.int32) != np.asarray(sentinel, buf.dtype).view(np.int32)
    assert not bad.any(), "%s: %d cells outside the result were overwritten" % (what, int(bad.sum()))


def within(got, ref, bound, what):
    """|got - ref| <= bound elementwise; returns the largest error / bound"""
    got, ref, bound = f64(got), f64(ref), f64(bound)
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    assert np.isfinite(got).all(), "%s: %d entries not written or not finite" % (what, int((~np.isfinite(got)).sum()))
    err = np.abs(got - ref)
    bad = err > bound
    if bad.any():
        at = tuple(int(x) for x in np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d entries beyond the bound, first at %s: got %r, reference %r, bound %.3g (x %.2f)"
                             % (what, int(bad.sum()), bad.size, at, got[at], ref[at], bound[at], err[at] / bound[at]))
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(err == 0, 0.0, err / bound).max()) if err.size else 0.0


def check_store(got, ref, bound, what="store"):
    return within(got, ref, bound, what)


def check_blockmax(got, ref, bound, sb_rows, what="blockmax"):
    """|got[s, u] - max_ref[s, u]| <= the largest bound of the superblock, for every cell"""
    return within(got, blockmax(ref, sb_rows), blockmax(bound, sb_rows), what)


def check_topk_exact(got_v, got_i, ref32, k, base=0, what="topk"):
    want_v, want_i = topk(ref32, k, base)
    same_bits(np.asarray(got_i, np.int32), want_i, what + " ids")
    same_bits(np.asarray(got_v, F32), want_v, what + " values")


def check_topk_bounded(got_v, got_i, ref, bound, k, base=0, what="topk"):
    """the four rules of a top-k held to the bound; returns the largest |value - reference of its id| / bound"""
    got_v, got_i, ref, bound = f64(got_v), np.asarray(got_i, np.int64), f64(ref), f64(bound)
    n_u, n_i = ref.shape
    kk = min(k, n_i)
    assert got_v.shape == got_i.shape == (n_u, k), (what, got_v.shape, got_i.shape)
    assert np.all(got_i[:, kk:] == -1) and np.all(got_v[:, kk:] == -np.inf), what + ": unused places are not -1 / -inf"
    ids = got_i[:, :kk] - base
    vals = got_v[:, :kk]
    assert np.all((ids >= 0) & (ids < n_i)), what + ": an id outside the catalogue"
    srt = np.sort(ids, axis=1)
    assert np.all(srt[:, 1:] != srt[:, :-1]), what + ": an id listed twice"
    assert np.all(vals[:, 1:] <= vals[:, :-1]), what + ": values increase"
    tied = vals[:, 1:] == vals[:, :-1]
    assert np.all(ids[:, 1:][tied] > ids[:, :-1][tied]), what + ": equal values not in ascending index order"
    ratio = within(vals, np.take_along_axis(ref, ids, axis=1), np.take_along_axis(bound, ids, axis=1), what + " values")
    if kk < n_i:
        listed = np.zeros((n_u, n_i), bool)
        np.put_along_axis(listed, ids, True, axis=1)
        kth = vals[:, -1] + np.take_along_axis(bound, ids[:, -1:], axis=1)[:, 0]
        over = ~listed & (ref > kth[:, None] + bound)
        if over.any():
            at = tuple(int(x) for x in np.argwhere(over)[0])
            raise AssertionError("%s: user %d: unlisted item %d has reference score %r above the k-th listed value %r + bounds"
                                 % (what, at[0], at[1], ref[at], vals[at[0], -1]))
    return ratio


# ------------------------------------------------------------------------------------------------ the case table
# TREC_SCORE_CASE(DT, KT, BN, NCB) of dispatch_score: every (dtype, kpad)
SCORE_CASES = tuple((dt, kp) for dt in (DT_F32, DT_BF16) for kp in KPADS)
FORMS = {DT_F32: ("dot", "euclid"), DT_BF16: ("dot", "glds", "euclid")}      # glds (variant bit 0): bf16 dot only
TILING_VARIANTS = tuple(range(2, 14))        # variant >> 1 in 1..6 at bf16 / K = 128 / capacity 12 / dot
# variant >> 1 = 4, 5 are ablation builds (ABL 1: no epilogue; ABL 2: the rare path is never taken): they list nothing by construction and
# cannot be held to a reference; the case table names them so that the count below is the dispatch code's
TILING_ABLATIONS = (8, 9, 10, 11)
HAND_FORMS = (("pipelined", DT_BF16), ("pipelined_f32", DT_F32), ("filter16", DT_BF16))   # score_blockmax.hip: K 64 / 128, dot
DT_NAME = {DT_F32: "f32", DT_BF16: "bf16"}


def case_id(c):
    epi = c.epi + (str(c.capacity) if c.epi == "topk" else "")
    if c.kernel.startswith("tiling"):
        return "%s-%s-k%d-v%d-%s" % (epi, DT_NAME[c.dtype], c.kpad, c.variant, c.bias)
    if c.kernel != "generic":
        return "%s-%s-%s-k%d-%s" % (epi, c.kernel, DT_NAME[c.dtype], c.kpad, c.bias)
    return "%s-%s-k%d-%s-%s" % (epi, DT_NAME[c.dtype], c.kpad, c.form, c.bias)


def _case(**kw):
    c = SimpleNamespace(capacity=0, variant=0, kernel="generic", testable=True, **kw)
    c.mode = MODE_EUCLID if c.form == "euclid" else MODE_DOT
    if c.form == "glds":
        c.variant |= 1
    return c


@functools.lru_cache(maxsize=None)
def grid():
    """every instantiation the dispatch code can reach, with a readable id (c.id):
    dispatch_score x epilogue (STORE, TOPK with capacity 8 / 12 / 16, BLOCKMAX) x {dot, glds, euclid} x bias option; the experimental tilings
    of trec_score_gemm_topk; launch_blockmax_pipelined / _pipelined_f32 / _filter16.  A one-sided bias runs the BIAS = true instantiation with
    one NULL pointer: its own case, because the kernels branch on the pointers."""
    out = []
    for epi, caps in (("store", (0,)), ("topk", CAPACITIES), ("blockmax", (0,))):
        for cap in caps:
            for dt, kp in SCORE_CASES:
                for form in FORMS[dt]:
                    for bias in BIASES:
                        c = _case(epi=epi, dtype=dt, kpad=kp, form=form, bias=bias)
                        c.capacity = cap
                        out.append(c)
    for v in TILING_VARIANTS:
        c = _case(epi="topk", dtype=DT_BF16, kpad=128, form="dot", bias="both")
        c.capacity, c.variant, c.kernel, c.testable = 12, v, "tiling%d" % (v >> 1), v not in TILING_ABLATIONS
        out.append(c)
    for kernel, dt in HAND_FORMS:
        for kp in (64, 128):
            for bias in BIASES:
                c = _case(epi="blockmax", dtype=dt, kpad=kp, form="dot", bias=bias)
                c.kernel = kernel
                c.variant = 32 if kernel == "filter16" else 0
                out.append(c)
    for c in out:
        c.id = case_id(c)
    assert len({c.id for c in out}) == len(out)
    return tuple(out)


def cases(epi, kernel=None, testable=True):
    return [c for c in grid() if c.epi == epi and (kernel is None or (c.kernel == kernel if isinstance(kernel, str) else kernel(c.kernel)))
            and (c.testable or not testable)]
