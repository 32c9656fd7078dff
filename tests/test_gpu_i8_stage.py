"""Every kernel of the int8 pre-filter (csrc/score_blockmax_i8.hip, the int8 image of csrc/user_prep.hip) against tests/i8_reference.py, called
at the ABI (_native.call) on operands the tests build themselves.  tests/test_i8_reference_host.py shows on the CPU that the reference
agrees with second formulations, that its acceptance helpers reject planted errors on these very operands, that the bound holds for
the reference pipeline alone on the populations of test_bound_dominates_with_scale_classes, and that the case table has the size of the
dispatch code.

Bars (i8_reference.py derives them): the table, the lists (untagged and tagged), the int8 rows, every scale, the integer biases and their
error maxima, the user error record: bit for bit.  Row norms (float32 fmaf chains on the device): (kpad + 4) 2^-24 relative, the error
norm with 2^-23 ||x|| on top.  Everything outside a result (stride padding, columns of an idle workgroup, list rows of chunks that do not
exist, bias rows of classes nobody uses, outputs of a refused call) keeps its sentinel bit for bit.

Instantiation -> test.  c.id is the id of i8_reference.grid(): k<KT>-tk<TK>-<bias>-<layout>.
    blockmax_i8x16_kernel<64 | 128, false, 0, 12>      test_stage_table_and_lists[k<KT>-tk0-none-<one_scale | classes>]
    blockmax_i8x16_kernel<64 | 128, true, 0, 12>       test_stage_table_and_lists[k<KT>-tk0-<user | item | both>-<one_scale | classes>]
    blockmax_i8x16_kernel<64 | 128, false, 10, 12>     test_stage_table_and_lists[k<KT>-tk10-none-<one_scale | classes>]
    blockmax_i8x16_kernel<64 | 128, true, 10, 12>      test_stage_table_and_lists[k<KT>-tk10-<user | item | both>-<one_scale | classes>]
    blockmax_i8x16_kernel<64 | 128, false, 16, 8>      test_stage_table_and_lists[k<KT>-tk16-none-<one_scale | classes>]
    blockmax_i8x16_kernel<64 | 128, true, 16, 8>       test_stage_table_and_lists[k<KT>-tk16-<user | item | both>-<one_scale | classes>]
  bias forms: none = no bias pointer at all (BIAS = false); user = user_bias with item_bias_q NULL (the side[] = 0 branch); item =
  item_bias_q with user_bias NULL; both.  Layouts: one_scale = scales[0], one bias row; classes = wg_scale / wg_class per workgroup,
  bias_q [64][n_items] with garbage in the rows of unused classes, non-zero sb_stats[:, 3], and one run with an idle (scale 0) workgroup
  between two live ones.  Every case runs n_users 3 and W + W/4 + 5, n_items 70 and 5 sb + 77 at sb_rows 128 and 512, n_chunks 1, 3 and
  n_sb + 2, bm_stride n_users + 4; every TK > 0 case also with top_k | 0x100 and with a NaN in r_err / an inf in sb_stats.
  The product path (trec_user_prep_sorted + trec_score_bias_i8_classes + the stage): test_bound_dominates_with_scale_classes.
    prep_i8_kernel<8 | 16 | 32>         test_prep_i8[prep-g<G>-d<d>-k<kpad>]   (trec_score_prep_i8 sides 0, 1, 2; trec_score_prep_i8_users)
    sb_scale_kernel, sb_reduce_kernel, sumsq_absmax_kernel, scale_from_stats_kernel, bias_i8_kernel (one class)      test_prep_i8
    bias_i8_kernel (classes)            test_bias_classes
    row_natscale_kernel<8 | 16 | 32>    test_row_scale[natscale-g<G>-d<d>]
    user_err_i8_kernel                  test_user_err
    prep_sorted_kernel<16 | 32> (int8 image)    test_sorted_user_operand_against_the_reference, test_sorted_user_operand_with_a_nan_element
    refusals (nothing launched)         test_stage_refuses_a_layout_for_the_other_list_length, test_prep_refuses_a_kpad_no_kernel_covers

Measured on the MI355X (TREC_I8_RATIOS_OUT=<file> writes the figures of a run there):
  largest error / tolerance of the norm comparisons, per form of prep_i8_kernel (all populations, all entry points):
      g32-d128-k128 0.056   g32-d100-k128 0.063   g16-d64-k64 0.11   g16-d40-k64 0.12   g8-d30-k32 0.16   g8-d5-k8 0.33
    and of prep_sorted_kernel: 0.042 .. 0.057 at kpad 128, 0.096 .. 0.11 at kpad 64 (the tolerance charges every element a full chain).
  median e / observed of test_bound_dominates_with_scale_classes (largest observed / e in brackets):
      d 128 k 10: 6.3 (0.36), with item biases 100 x the scores 6.9 (0.28);   d 40 k 16: 3.8 (0.54), big biases 4.2 (0.45)
  The file takes 5 to 6 s of wall time (5.3 s measured for 74 of its 75 cases; 2,395 GPU tests of the whole suite: 702 s).

What the planted-error runs showed (scratch builds of score_blockmax_i8.hip, not committed):
arithmetic changes only, nothing that moves a global address.  Which tests failed:
    the LDS read offsets koff[] of the CH == 4 form without their swizzle (the writes keep it)
                                            every k64-* case of test_stage_table_and_lists (24), test_bound_dominates_with_scale_classes[40-16-*]
    the one k-step of KT = 64 dropped (acc = c0)         the same 24 + 2
    wg_class ignored (always the bias row of class 0)    every *-item-classes and *-both-classes case (12), test_bound_dominates_with_scale_classes[*] (4)
    db = ss_cur[3] without a_user                        every tk10 / tk16 case (32), test_bound_dominates_with_scale_classes[*] (4),
                                                         test_gpu_cascade.py::test_int8_table_is_exact_integer_arithmetic_and_bound_holds
    own_bias skipped when t_bias_q is NULL               every *-user-* case (12), nothing else
  Of the five, the suite before this file caught the fourth only.  (A swizzle made constant on BOTH sides is no error: writes and reads agree
  and only the bank conflicts change.)

What the tests found in the shipped code, fixed with them: trec_score_prep_i8 / trec_score_prep_i8_users sized their grid by kpad / 4 lanes per
row but launch the 8-lane form for every kpad below 64, so for kpad < 32 only about the first kpad / 32 of the rows were written (prep-g8-d5-k8,
n = 515: rows from 160 on kept the sentinel); 64 < kpad < 128 reached a form that covers 64 columns (now refused); a NaN element was
quantised to -127, not 0, because fmaxf(NaN, -127) is -127 and the NaN test came after the clamp (every *-nonfinite population)."""
import json
import os
import time

import numpy as np
import pytest
import torch

import i8_reference as R
from i8_reference import F32, f64

pytestmark = pytest.mark.gpu

SENT = F32(-12345.5)
SENT_Q = 0x55
RATIOS, LOOSE = {}, {}
T0 = time.time()
GRID = R.grid()
PREP = [c for c in R.prep_grid() if c.kernel == "prep_i8_kernel"]
NATSCALE = [c for c in R.prep_grid() if c.kernel == "row_natscale_kernel"]


@pytest.fixture(scope="module")
def N():
    from tensorrec_amd import _native
    _native.require_gpu()
    _native.load()
    yield _native
    out = os.environ.get("TREC_I8_RATIOS_OUT")
    if out:
        with open(out, "w") as f:
            json.dump({"norm_error_over_tolerance": {k: float("%.4g" % v) for k, v in sorted(RATIOS.items())},
                       "median_bound_over_observed": {k: float("%.4g" % v) for k, v in sorted(LOOSE.items())},
                       "seconds_since_import": round(time.time() - T0, 2)}, f, indent=1)
            f.write("\n")


@pytest.fixture(scope="module")
def ops(N):
    from tensorrec_amd import ops as _ops
    return _ops


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def filled(shape, value, dtype=torch.float32):
    return torch.full(shape, value, dtype=dtype, device="cuda")


def W_of(N, tk):
    return int(N.query("trec_score_blockmax_i8_rows_per_workgroup", tk))


# ------------------------------------------------------------------------------------------------ the stage
class Stage(object):
    """the device operands of an i8_reference.stage_problem and the call"""

    def __init__(self, N, p):
        self.N, self.p = N, p
        self.uq, self.iq, self.ub, self.bias_q = dev(p.uq), dev(p.iq), dev(p.ub), dev(p.bias_q)
        # with wg_scale the kernel must not look at scales[0]: garbage there
        self.scales = dev(p.scales if p.wg_scale is None else np.array([1e9, 0, 0], F32))
        self.sb_stats, self.r_err = dev(p.sb_stats), dev(p.r_err)
        self.wg_scale, self.wg_class = dev(p.wg_scale), dev(p.wg_class)
        self.stride = p.n_users + 4

    def run(self, n_chunks, top_k, r_err=None, sb_stats=None, kpad=None, wg_rows=None, wg_scale="own", wg_class="own", table=None, ctop=None):
        p, N = self.p, self.N
        tk = top_k & 0xff
        table = filled((p.n_sb, self.stride), float(SENT)) if table is None else table
        if tk and ctop is None:
            ctop = filled((n_chunks * tk, self.stride), float(SENT))
        wgs = self.wg_scale if wg_scale == "own" else wg_scale
        wgc = self.wg_class if wg_class == "own" else wg_class
        N.call("trec_score_gemm_blockmax_i8", N.ptr(self.uq), N.ptr(self.iq), p.kt if kpad is None else kpad, p.n_users, p.n_items,
               N.ptr(self.ub), N.ptr(self.bias_q), N.ptr(self.scales), N.ptr(self.sb_stats if sb_stats is None else sb_stats), p.sb_rows,
               n_chunks, N.ptr(table), self.stride, N.ptr((self.r_err if r_err is None else r_err) if tk else None), N.ptr(ctop), top_k,
               N.ptr(wgs), N.ptr(wgc), (p.wg_rows if wgs is not None else 0) if wg_rows is None else wg_rows)
        return host(table), (host(ctop) if tk else None)


def stage_shapes(W):
    for n_users in (3, W + W // 4 + 5):
        for n_items, sb in ((70, 128), (70, 512), (5 * 128 + 77, 128), (5 * 512 + 77, 512)):
            yield n_users, n_items, sb


@pytest.mark.parametrize("c", GRID, ids=[c.id for c in GRID])
def test_stage_table_and_lists(N, c):
    W = W_of(N, c.tk)
    assert W == R.rows_per_workgroup(c.tk) == 4 * c.nub * 16
    for n_users, n_items, sb in stage_shapes(W):
        p = R.stage_problem(c, n_users, n_items, sb)
        S = Stage(N, p)
        want = R.stage_table(p)
        lb = R.lower_bounds(want, R.stage_bound(p)) if c.tk else None
        for n_chunks in (1, 3, p.n_sb + 2):
            what = "%s users %d items %d sb %d chunks %d" % (c.id, n_users, n_items, sb, n_chunks)
            table, ctop = S.run(n_chunks, c.tk)
            R.check_table(table, want, p.written, SENT, what + ": table")
            if not c.tk:
                continue
            ut = R.lists(lb, n_items, n_chunks, sb, c.tk)
            R.check_lists(ctop, ut, p.written, SENT, what + ": lists")
            # ---- the tagged lists: the same table; every entry a slightly smaller lower bound that names its superblock inside the chunk
            table_t, ctop_t = S.run(n_chunks, c.tk | 0x100)
            R.check_table(table_t, want, p.written, SENT, what + ": table of the tagged run")
            tg = R.lists(lb, n_items, n_chunks, sb, c.tk, tagged=True)
            R.check_lists(ctop_t, tg, p.written, SENT, what + ": tagged lists")
            n_ch = ut.shape[0]
            R.check_tagged(ctop_t[:n_ch * c.tk, :n_users].reshape(n_ch, c.tk, n_users), ctop[:n_ch * c.tk, :n_users].reshape(n_ch, c.tk, n_users),
                           lb, n_items, n_chunks, sb, what + ": tagged")
        if n_users > 3 and n_items > 70 and not c.tk:
            # ---- the form without lists writes the table of the 10-slot form (same operands: the seed does not know the list length)
            sib = next(g for g in GRID if (g.kt, g.bias, g.layout, g.tk) == (c.kt, c.bias, c.layout, 10))
            p10 = R.stage_problem(sib, n_users, n_items, sb)
            assert np.array_equal(p10.uq, p.uq) and np.array_equal(p10.sb_stats, p.sb_stats) and p10.wg_rows == p.wg_rows
            table10, _ = Stage(N, p10).run(3, 10)
            R.same_bits(table10, S.run(3, 0)[0], what + ": TK = 0 against TK = 10")
        if n_users > 3 and (n_items, sb) == (5 * 128 + 77, 128) and c.tk:
            # ---- non-finite inputs to the lists: a NaN in one user's record empties that user's lists, an inf in a superblock's
            # statistics removes it from everybody's; the table does not change
            r_err, sbs = p.r_err.copy(), p.sb_stats.copy()
            r_err[W + 7, 1] = np.nan
            sbs[2, 2] = np.inf
            lb_nf = R.lower_bounds(want, R.stage_bound(p, r_err=r_err, sb_stats=sbs))
            assert np.all(np.isneginf(lb_nf[:, W + 7])) and np.all(np.isneginf(lb_nf[2])) and np.isfinite(lb_nf[3, 5])
            for n_chunks in (1, 3):
                table, ctop = S.run(n_chunks, c.tk, r_err=dev(r_err), sb_stats=dev(sbs))
                R.check_table(table, want, p.written, SENT, c.id + ": table with non-finite list inputs")
                li = R.lists(lb_nf, n_items, n_chunks, sb, c.tk)
                R.check_lists(ctop, li, p.written, SENT, c.id + ": lists with non-finite inputs")
                assert np.all(np.isneginf(ctop[:li.shape[0] * c.tk, W + 7]))
    if c.layout == "classes":
        # ---- an idle workgroup (scale 0) between two live ones: its columns keep the sentinel, the neighbours are exact
        n_users, n_items, sb = 2 * W + 5, 5 * 128 + 77, 128
        p = R.stage_problem(c, n_users, n_items, sb, idle=1)
        assert not p.written[W:2 * W].any() and p.written[:W].all() and p.written[2 * W:].all()
        want = R.stage_table(p)
        table, ctop = Stage(N, p).run(3, c.tk)
        R.check_table(table, want, p.written, SENT, c.id + ": table around an idle workgroup")
        assert np.all(R.bits(table[:, W:2 * W]) == R.bits(np.full(1, SENT, F32))[0])
        if c.tk:
            li = R.lists(R.lower_bounds(want, R.stage_bound(p)), n_items, 3, sb, c.tk)
            R.check_lists(ctop, li, p.written, SENT, c.id + ": lists around an idle workgroup")


def test_stage_refuses_a_layout_for_the_other_list_length(N):
    c = next(g for g in GRID if g.id == "k128-tk10-both-classes")
    p = R.stage_problem(c, 3, 70, 128)
    S = Stage(N, p)
    table, ctop = filled((p.n_sb, S.stride), float(SENT)), filled((10, S.stride), float(SENT))
    other = W_of(N, 16)
    assert other != p.wg_rows
    with pytest.raises(RuntimeError, match="another workgroup height"):
        S.run(1, 10, wg_rows=other, table=table, ctop=ctop)
    c16 = next(g for g in GRID if g.id == "k128-tk16-both-classes")
    S16 = Stage(N, R.stage_problem(c16, 3, 70, 128))
    ctop16 = filled((16, S.stride), float(SENT))
    with pytest.raises(RuntimeError, match="another workgroup height"):
        S16.run(1, 16 | 0x100, wg_rows=W_of(N, 10), table=table, ctop=ctop16)
    with pytest.raises(RuntimeError, match="wg_class comes with wg_scale"):
        S.run(1, 10, wg_scale=None, wg_rows=0, table=table, ctop=ctop)
    with pytest.raises(RuntimeError, match="kpad must be 64 or 128"):
        S.run(1, 10, kpad=32, table=table, ctop=ctop)
    torch.cuda.synchronize()
    for buf in (table, ctop, ctop16):
        assert np.all(R.bits(host(buf)) == R.bits(np.full(1, SENT, F32))[0])
    S.run(1, 10, table=table, ctop=ctop)                                    # the same buffers, the right arguments: written
    assert not np.any(R.bits(host(table))[:, :3] == R.bits(np.full(1, SENT, F32))[0])


# ------------------------------------------------------------------------------------------------ operand preparation
def prep_call(N, x, kpad, side, clip=0.0, sb_rows=0, bias=None, scales=None, sb_stats=None, gstats=None):
    """trec_score_prep_i8 on sentinel-filled outputs; returns the device tensors"""
    n = len(x) if x is not None else len(bias)
    d = x.shape[1] if x is not None else 1
    o = dict(q=filled((n, kpad), SENT_Q, torch.int8), st=filled((n, 2), float(SENT)),
             scales=filled((3,), 0.0) if scales is None else scales, ws=torch.empty((2,), dtype=torch.float64, device="cuda"),
             bq=filled((n,), -777, torch.int32) if bias is not None else None, sb=sb_stats, g=gstats)
    dx, dbias = dev(x), dev(bias)                          # (named: a temporary's memory may be handed out again before the launch)
    N.call("trec_score_prep_i8", N.ptr(dx), n, d, kpad, side, float(clip), sb_rows, N.ptr(dbias), N.ptr(o["scales"]),
           N.ptr(o["ws"]) if side == 0 else None, N.ptr(o["q"]) if side != 2 else None, N.ptr(o["st"]) if side != 2 else None,
           N.ptr(o["bq"]), N.ptr(o["sb"]), N.ptr(o["g"]))
    return o


@pytest.mark.parametrize("c", PREP, ids=[c.id for c in PREP])
def test_prep_i8(N, c):
    d, kpad = c.d, c.kpad
    worst = 0.0
    for n in (1, 515):
        for kind in R.POPULATIONS:
            rng = np.random.default_rng(1000 * d + n + len(kind))
            x = R.rows(kind, n, d, rng)
            what = "%s n %d %s" % (c.id, n, kind)
            # ---- side 0: the users' one scale, with and without clipping
            for clip in (4.0, 0.0):
                o = prep_call(N, x, kpad, 0, clip=clip)
                a = R.user_scale(x, clip)
                R.same_bits(host(o["scales"])[:1], np.array([a], F32), what + ": user scale, clip %g" % clip)
                q = R.quantise(x, a, kpad)
                R.same_bits(host(o["q"]), q, what + ": user rows")
                worst = max(worst, R.check_norms(host(o["st"]), R.row_stats(x, q, a), kpad, what + ": user norms"))
                if kind == "outliers" and clip > 0 and n > 1:
                    assert (np.abs(x) > 127.5 * a).any() and a < R.user_scale(x, 0.0)      # something clips
            # ---- side 1 with a bias (the users' scale is there), then side 2 for another user scale
            bias = (0.3 * rng.standard_normal(n)).astype(F32)
            for sb in (128, 512):
                n_sb = R.n_superblocks(n, sb)
                scales = dev(np.array([a, 0, 0], F32))
                o = prep_call(N, x, kpad, 1, sb_rows=sb, bias=bias, scales=scales, sb_stats=filled((n_sb, 4), 0.0), gstats=filled((4,), 0.0))
                sbs, st = host(o["sb"]), host(o["st"])
                b_s = R.item_scales(x, sb)
                R.same_bits(sbs[:, 0], b_s, what + ": item scales, sb %d" % sb)
                b_row = R.rows_of_superblocks(b_s, n, sb)
                q = R.quantise(x, b_row, kpad)
                R.same_bits(host(o["q"]), q, what + ": item rows")
                st64 = R.row_stats(x, q, b_row)
                worst = max(worst, R.check_norms(st, st64, kpad, what + ": item norms"))
                R.same_bits(sbs[:, 1:3], R.sb_reduce(st, sb), what + ": superblock maxima of the device's own norms")
                # ... and against the float64 norms: a maximum moves by at most the largest tolerance of its rows (+ the addition's rounding)
                want = f64(R.sb_reduce(st64.astype(F32), sb))
                tol = R.norm_tolerances(np.nan_to_num(st64, nan=0.0, posinf=0.0), kpad)
                slack = np.maximum.reduceat(tol.sum(1), np.arange(0, n, sb))[:, None] + 2.0 ** -22 * np.where(np.isfinite(want), want, 0)
                fin = np.isfinite(want)
                assert np.array_equal(np.isinf(sbs[:, 1:3]), ~fin), what
                assert np.all(np.abs(f64(sbs[:, 1:3])[fin] - want[fin]) <= np.broadcast_to(slack, want.shape)[fin]), what
                bq, sb3, g2 = R.bias_classes(bias, b_s, sb, np.array([a], F32))
                R.same_bits(host(o["bq"]), bq[0], what + ": integer biases")
                R.same_bits(sbs[:, 3], sb3, what + ": bias error maxima")
                R.same_bits(host(o["g"])[2:3], np.array([g2], F32), what + ": max |bias|")
                a2 = F32(a * F32(0.37))
                o["sb"][:, 3] = 0
                o2 = prep_call(N, None, kpad, 2, sb_rows=sb, bias=bias, scales=dev(np.array([a2, 0, 0], F32)), sb_stats=o["sb"], gstats=filled((4,), 0.0))
                bq2, sb3_2, _ = R.bias_classes(bias, b_s, sb, np.array([a2], F32))
                R.same_bits(host(o2["bq"]), bq2[0], what + ": integer biases, side 2")
                R.same_bits(host(o2["sb"])[:, 3], sb3_2, what + ": bias error maxima, side 2")
                R.same_bits(host(o2["sb"])[:, :3], sbs[:, :3], what + ": side 2 leaves the item statistics alone")
            # ---- users with a scale per workgroup (128 rows here: five workgroups, the last one partial)
            wg = 128
            n_wg = -(-n // wg)
            wg_scale = np.array([F32(2.0 ** -(2 * w)) * R._sane(R._absmax(x[w * wg:(w + 1) * wg]) / F32(127)) * F32(1.0 if w % 2 else 0.5)
                                 for w in range(n_wg)], F32)
            qd, std = filled((n, kpad), SENT_Q, torch.int8), filled((n, 2), float(SENT))
            dx, dwg = dev(x), dev(wg_scale)
            N.call("trec_score_prep_i8_users", N.ptr(dx), n, d, kpad, N.ptr(dwg), wg, N.ptr(qd), N.ptr(std))
            a_rows = R.rows_of_workgroups(wg_scale, n, wg)
            q = R.quantise(x, a_rows, kpad)
            R.same_bits(host(qd), q, what + ": rows under workgroup scales")
            worst = max(worst, R.check_norms(host(std), R.row_stats(x, q, a_rows), kpad, what + ": norms under workgroup scales"))
    RATIOS[c.id] = worst
    assert worst <= 1.0


def test_prep_refuses_a_kpad_no_kernel_covers(N):
    """64 < kpad < 128 has no prep_i8_kernel form (G = 8 covers 64 columns, G = 32 is dispatched for 128 only): refused, nothing written"""
    rng = np.random.default_rng(96)
    for d in (70, 96):
        x = dev(rng.standard_normal((40, d)).astype(F32))
        for kpad in (96, 68, 124):
            if kpad < d:
                continue
            q, st = filled((40, kpad), SENT_Q, torch.int8), filled((40, 2), float(SENT))
            scales, ws = filled((3,), float(SENT)), torch.empty((2,), dtype=torch.float64, device="cuda")
            sbs = filled((1, 4), 0.0)
            with pytest.raises(RuntimeError, match="kpad <= 64 or kpad == 128"):
                N.call("trec_score_prep_i8", N.ptr(x), 40, d, kpad, 0, 4.0, 0, None, N.ptr(scales), N.ptr(ws), N.ptr(q), N.ptr(st), None, None, None)
            with pytest.raises(RuntimeError, match="kpad <= 64 or kpad == 128"):
                N.call("trec_score_prep_i8", N.ptr(x), 40, d, kpad, 1, 0.0, 128, None, N.ptr(scales), None, N.ptr(q), N.ptr(st), None, N.ptr(sbs), None)
            with pytest.raises(RuntimeError, match="kpad <= 64 or kpad == 128"):
                wg_scale = filled((1,), 0.01)
                N.call("trec_score_prep_i8_users", N.ptr(x), 40, d, kpad, N.ptr(wg_scale), 128, N.ptr(q), N.ptr(st))
            torch.cuda.synchronize()
            assert np.all(host(q) == SENT_Q) and np.all(host(st) == SENT) and np.all(host(scales) == SENT) and not host(sbs).any()


def test_bias_classes(N):
    rng = np.random.default_rng(64)
    n, sb = 5 * 128 + 77, 128
    n_sb = R.n_superblocks(n, sb)
    b_s = rng.uniform(0.5e-3, 2e-3, n_sb).astype(F32)
    bias = rng.standard_normal(n).astype(F32)
    bias[3], bias[700] = 1.0, -1.0
    ladder = (F32(2.0 ** -3) * np.exp2(-np.arange(64, dtype=F32) / F32(4))).astype(F32)
    ladder[40], ladder[50] = 1e-5, 1e-7                   # products a_c b_s of 1e-8 (a bias of 1 is 1e8 units) and 1e-10 (it clamps at 2^30)
    for used_classes in ((0, 5, 40, 50, 63), (0, 5), (17,)):
        used = np.zeros(64, np.int32)
        used[list(used_classes)] = 1
        sbs = np.zeros((n_sb, 4), F32)
        sbs[:, 0] = b_s
        sbs[:, 1:3] = SENT
        d_sbs, d_bq, d_g = dev(sbs), filled((64, n), -777, torch.int32), filled((4,), 0.0)
        d_bias, d_ladder, d_used = dev(bias), dev(ladder), dev(used)
        N.call("trec_score_bias_i8_classes", N.ptr(d_bias), n, sb, N.ptr(d_ladder), N.ptr(d_used), 64, N.ptr(d_sbs), N.ptr(d_bq), N.ptr(d_g))
        bq, sb3, g2 = R.bias_classes(bias, b_s, sb, ladder, used)
        got = host(d_bq)
        for cl in range(64):
            if used[cl]:
                R.same_bits(got[cl], bq[cl], "bias_q of class %d" % cl)
            else:
                assert np.all(got[cl] == -777), cl
        if 50 in used_classes:
            assert got[50][3] == R.BQ_MAX and got[50][700] == -R.BQ_MAX and 5e7 < got[40][3] < 2e8
        out = host(d_sbs)
        R.same_bits(out[:, 3], sb3, "sb_stats[:, 3] over the classes %s" % (used_classes,))
        R.same_bits(out[:, :3], sbs[:, :3], "the other statistics")
        assert host(d_g)[2] == g2 and not host(d_g)[[0, 1, 3]].any()
    # the maximum is over the classes in use only: the clamped class is not in the last two runs
    assert sb3.max() < 1e-3 * R.bias_classes(bias, b_s, sb, ladder, np.ones(64, np.int32))[1].max()


@pytest.mark.parametrize("c", NATSCALE, ids=[c.id for c in NATSCALE])
def test_row_scale(N, c):
    d = c.d
    for n in (1, 515):
        rng = np.random.default_rng(7 * d + n)
        x = R.rows("outliers", n, d, rng) * np.exp(rng.uniform(-7, 7, size=(n, 1))).astype(F32)
        if n > 1:
            x[::9] = 0
        nat, gmax = filled((n,), float(SENT)), filled((1,), 0.0)
        dx = dev(x)
        N.call("trec_score_row_scale_i8", N.ptr(dx), n, d, N.ptr(nat), N.ptr(gmax))
        got = host(nat)
        ref, decided, _ = R.row_scale(x)
        R.same_bits(got[decided], ref[decided], "%s n %d: wanted scales" % (c.id, n))
        am = np.abs(x).max(1) / F32(127)
        live = am > 0
        assert np.all(np.isin(got[live] / am[live], (1.0, 0.5, 0.25))) and np.all(got[~live] == 0)
        assert host(gmax)[0] == got.max()


def test_user_err(N):
    rng = np.random.default_rng(12)
    n = 1000                                               # no multiple of 256, 512 or 768
    ust = np.abs(rng.standard_normal((n, 2))).astype(F32)
    ub = rng.standard_normal(n).astype(F32)
    g = np.array([SENT, SENT, 0.7, SENT], F32)
    scales = np.array([0.0123, SENT, SENT], F32)
    for kdim in (64, 128):
        for wg_rows, wg_scale in ((0, None), (W_of(N, 10), np.array([2.0 ** -7, 3e-4], F32)), (W_of(N, 16), np.array([0.5, 2.0 ** -9], F32))):
            for bias in (ub, None):
                out = filled((n + 1, 4), float(SENT))
                d_ust, d_bias, d_g, d_scales, d_wg = dev(ust), dev(bias), dev(g), dev(scales), dev(wg_scale)
                N.call("trec_score_user_err_i8", N.ptr(d_ust), N.ptr(d_bias), N.ptr(d_g), kdim, n,
                       N.ptr(d_scales) if wg_scale is None else None, N.ptr(d_wg), wg_rows, N.ptr(out))
                a_u = scales[0] if wg_scale is None else R.rows_of_workgroups(wg_scale, n, wg_rows)
                got = host(out)
                R.same_bits(got[:n], R.user_err(ust, bias, g[2], kdim, a_u), "user_err kdim %d wg_rows %d bias %s" % (kdim, wg_rows, bias is not None))
                assert np.all(got[n] == SENT)
    assert R.ck_of(128) == F32(134) * F32(2.98023224e-07)


SORTED = [("scaled", 128, 10, False), ("outliers", 40, 16, False), ("zeros", 128, 16, False), ("scaled", 40, 10, True),
          ("outliers", 128, 10, True), ("zeros", 40, 16, True)]


@pytest.mark.parametrize("kind,d,k,normalize", SORTED)
def test_sorted_user_operand_against_the_reference(N, ops, kind, d, k, normalize):
    """the int8 image the one gather pass writes (prep_sorted_kernel) against NumPy, not against the stand-alone kernel"""
    n = 2500
    rng = np.random.default_rng(n + d + k)
    x = R.rows(kind, n, d, rng)
    op = ops.score_prep_filter(dev(x), normalize=normalize, sort_users=True, k=k)
    wg = W_of(N, 10 if k <= 10 else 16)
    assert op.wg_rows == wg and op.kpad == R.kpad_of(d) and op.n % wg == 0
    src, f32, wg_scale = host(op.src), host(op.f32), host(op.wg_scale)
    keep = src >= 0
    assert np.array_equal(np.sort(src[keep]), np.arange(n))
    # the fp32 operand is the caller's row (zero padded), normalised for cosine
    want = np.zeros((int(keep.sum()), op.kpad), F32)
    want[:, :d] = x[src[keep]]
    if normalize:
        nrm = np.sqrt((f64(want) ** 2).sum(1, keepdims=True))
        np.testing.assert_allclose(f32[keep], f64(want) / np.maximum(nrm, 1e-6), rtol=2e-6, atol=1e-30)
    else:
        R.same_bits(f32[keep], want, "fp32 operand")
    a_rows = R.rows_of_workgroups(wg_scale, op.n, wg)
    assert np.all(a_rows[keep] > 0) and len(np.unique(a_rows[keep])) >= (4 if kind == "scaled" else 1)
    q = R.quantise(f32[keep], a_rows[keep], op.kpad)
    R.same_bits(host(op.i8)[keep], q, "int8 rows under wg_scale")
    assert np.abs(q).max() >= 64                                            # the scales fit the rows: the range is used
    RATIOS["sorted-%s-d%d-k%d-%s" % (kind, d, k, "cos" if normalize else "dot")] = \
        R.check_norms(host(op.stats8)[keep], R.row_stats(f32[keep], q, a_rows[keep]), op.kpad, "stats8")
    assert not host(op.i8)[~keep].any() and not host(op.stats8)[~keep].any()


def test_sorted_user_operand_with_a_nan_element(N, ops):
    """a NaN poisons gmax (every scale is inf: everybody is flagged downstream); the int8 rows are then all zero -- the NaN element too"""
    rng = np.random.default_rng(9)
    x = R.rows("gauss", 300, 40, rng)
    x[7, 3] = np.nan
    op = ops.score_prep_filter(dev(x), sort_users=True, k=10)
    assert np.isinf(host(op.gmax)[0])
    src, wg_scale = host(op.src), host(op.wg_scale)
    a_rows = R.rows_of_workgroups(wg_scale, op.n, op.wg_rows)
    keep = src >= 0
    assert np.all(np.isinf(a_rows[keep]))
    R.same_bits(host(op.i8)[keep], R.quantise(host(op.f32)[keep], a_rows[keep], op.kpad), "int8 rows under an infinite scale")
    assert not host(op.i8).any() and np.isnan(host(op.stats8)[host(op.pos)[7]]).all()


@pytest.mark.parametrize("d,k,big_bias", [(128, 10, False), (128, 10, True), (40, 16, False), (40, 16, True)])
def test_bound_dominates_with_scale_classes(N, ops, d, k, big_bias):
    """The product path: class-sorted users, integer biases per class, the stage's table; e from the reference formula on the device's
    user_err and sb_stats must dominate the observed |int8 score - exact score| of every (superblock, real user)."""
    sb, tk = 512, 10 if k <= 10 else 16
    x, y, ub, ib = R.bound_population(d, big_bias, seed=d + k + big_bias)
    dub, dib = dev(ub), dev(ib)
    uop = ops.score_prep_filter(dev(x), sort_users=True, k=k, user_bias=dub)
    iop = ops.score_prep_filter(dev(y), bias=dib, want_gstats=True)
    ops.score_prep_i8_pair(uop, iop, dib, sb, top_k=tk)
    kpad, n_u, n_i = uop.kpad, uop.n, len(y)
    n_sb = R.n_superblocks(n_i, sb)
    uerr = filled((n_u, 4), float(SENT))
    N.call("trec_score_user_err_i8", N.ptr(uop.stats8), N.ptr(uop.bias_sorted), N.ptr(iop.gstats8), kpad, n_u, None, N.ptr(uop.wg_scale),
           uop.wg_rows, N.ptr(uerr))
    n_chunks, stride = 3, n_u + 4
    table, ctop = filled((n_sb, stride), float(SENT)), filled((n_chunks * tk, stride), float(SENT))
    N.call("trec_score_gemm_blockmax_i8", N.ptr(uop.i8), N.ptr(iop.i8), kpad, n_u, n_i, N.ptr(uop.bias_sorted), N.ptr(iop.bias_q), None,
           N.ptr(iop.sb_stats), sb, n_chunks, N.ptr(table), stride, N.ptr(uerr), N.ptr(ctop), tk, N.ptr(uop.wg_scale), N.ptr(uop.wg_class),
           uop.wg_rows)
    src, wg_scale, wg_class = host(uop.src), host(uop.wg_scale), host(uop.wg_class)
    real = src >= 0
    r = np.flatnonzero(real)
    ue, sbs = host(uerr), host(iop.sb_stats)
    a_u = R.rows_of_workgroups(wg_scale, n_u, uop.wg_rows)
    assert np.array_equal(ue[:, 3], a_u) and len(np.unique(wg_class[wg_class >= 0])) >= 12 and real.sum() == len(x)
    e = R.pair_err(ue[:, 0][None, :], ue[:, 1][None, :], ue[:, 2][None, :], sbs[:, 1][:, None], sbs[:, 2][:, None],
                   ue[:, 3][None, :] * sbs[:, 3][:, None], kpad)
    class_u = R.rows_of_workgroups(wg_class, n_u, uop.wg_rows)
    bq = host(iop.bias_q)
    groups = R.real_groups([(np.flatnonzero(class_u == cl), bq[cl]) for cl in np.unique(class_u[real])], real)
    b_row = R.rows_of_superblocks(sbs[:, 0], n_i, sb)
    xs = np.zeros((len(r), kpad), F32)
    xs[:, :d] = x[src[r]]
    ys = np.zeros((n_i, kpad), F32)
    ys[:, :d] = y
    ubs = ub[src[r]]
    diff, exact_max, m_int = R.observed_error(host(uop.i8)[r], host(iop.i8), groups, a_u[r], b_row, xs, ys, ubs, ib, sb)
    # the table is the integer maximum of the device's own operands, converted once
    got = host(table)
    want = m_int.astype(F32) * (a_u[r][None, :] * sbs[:, 0][:, None]) + ubs[None, :]
    R.same_bits(got[:, r], want, "table of the product path")
    idle = np.flatnonzero(a_u == 0)
    assert np.all(R.bits(got[:, idle]) == R.bits(np.full(1, SENT, F32))[0]) and np.all(R.bits(got[:, n_u:]) == R.bits(np.full(1, SENT, F32))[0])
    er = f64(e[:, r])
    ratio = er / np.maximum(diff, 1e-300)
    print("bound d %d k %d big_bias %s: largest observed / e %.4g, median e / observed %.4g" % (d, k, big_bias, (diff / er).max(), np.median(ratio)))
    LOOSE["d%d-k%d-%s" % (d, k, "big" if big_bias else "small")] = float(np.median(ratio))
    assert np.all(np.isfinite(er)) and np.all(diff <= er)
    # every list entry is a lower bound of the table's own column, and every such bound lies below the exact maximum of its superblock
    lb = R.lower_bounds(got[:, :n_u], e)
    assert np.all(f64(lb[:, r]) <= exact_max)
    R.check_lists(host(ctop), R.lists(lb, n_i, n_chunks, sb, tk), a_u != 0, SENT, "lists of the product path")
