"""Every stage-1 score kernel instantiation (csrc/score_gemm.hip, csrc/score_blockmax.hip) against tests/score_reference.py, called at the
ABI (_native.call) on operands the tests pad and round themselves.  tests/test_score_reference_host.py shows on the CPU that the reference
equals the committed oracle, that the acceptance rules reject planted errors and that the case table has the size of the dispatch code.

Bars (score_reference.py derives them):
* dyadic data (integers in [-3, 3], quarter biases): values AND ids bit for bit against the float32 restatement, every instantiation, bf16
  included; thousands of exact ties hold the (value desc, index asc) rule across half-wave lists, tiles and chunks.
  The bias order is a documented property, encoded by restate32: (s + b_u) + b_i for fp32 and every Euclidean form, (b_i + s) + b_u for bf16
  dot (exact either way on this data; behind the Euclidean square root only the first order is used).
* real data, fp32: bit for bit against oracle.score_dense_exact / score_dense_euclid_exact; bf16: within the bound B of the float64
  reference on the bf16-rounded operands (STORE elementwise; BLOCKMAX per cell with the largest B of the superblock; TOPK by the four rules
  of check_topk_bounded).
* everything outside a result (ld_out / bm_stride padding, the row past the end, lists nobody owns) keeps its sentinel bit for bit.

Instantiation -> test.  c.id is the id of score_reference.grid():
    store-<dtype>-k<kpad>-<dot|glds|euclid>-<bias>                 test_store_dyadic[<id>]
    topk<8|12|16>-<dtype>-k<kpad>-<form>-<bias>                    test_topk_dyadic[<id>]           (n_chunks 1 and 3, k = capacity and 1)
    topk12-bf16-k128-v<2..7, 12, 13>-both                          test_topk_tilings[<id>]          (v8..v11 are ablation builds that list
                                                                                                     nothing: named by grid(), not run)
    blockmax-<dtype>-k<kpad>-<form>-<bias>                         test_blockmax_dyadic[<id>]       (both tunings 0: the generic kernel)
    blockmax-pipelined-bf16-k<64|128>-<bias>                       test_blockmax_dyadic[<id>]       (launch_blockmax_pipelined)
    blockmax-pipelined_f32-f32-k<64|128>-<bias>                    test_blockmax_dyadic[<id>]       (launch_blockmax_pipelined_f32)
    blockmax-filter16-bf16-k<64|128>-<bias>                        test_blockmax_dyadic[<id>]       (variant | 32)
  and by (dtype, kpad, mode) on real data: test_store_real, test_topk_real, test_blockmax_real; launch geometry: test_topk_edges,
  test_blockmax_shapes, test_store_d_below_kpad; blockmax_bf16x16_kernel<KT, BIAS, GRP>: test_blockmax_grouped (GRP, both layouts),
  test_blockmax_hot (dense over a list); the grouped TOPK launch: test_topk_grouped; score_prep_kernel / score_prep_vec4_kernel<8 / 16 / 32>:
  test_score_prep.

Largest error / bound measured on the MI355X over the bf16 real-data cases of this file, per (dtype, kpad, mode) (fp32 is held to equality):
    bf16 dot        kpad 32: 0.025   kpad 64: 0.013   kpad 128: 0.0071   kpad 256: 0.0031   (the bound charges every addition a full unit at the
                                                                                         sum of magnitudes; the errors of a chain mostly cancel)
    bf16 euclid     kpad 32: 0.33    kpad 64: 0.20    kpad 128: 0.098    kpad 256: 0.066    (the square root's own rounding dominates at small K)
  TREC_SCORE_RATIOS_OUT=<file> writes the ratios of a run there.  All 586 cases of the file take 8 s on the MI355X.

What the planted-error runs showed (scratch builds of score_gemm.hip, not committed): the last k-step of the bf16 main loop dropped fails
every bf16 case of the generic kernel (store, topk, blockmax, dyadic and real); r_bias read for a NULL t_bias fails the user-only bias cases of
test_store_dyadic, test_topk_dyadic, test_blockmax_dyadic, test_topk_tilings and test_topk_edges; `hit = v >= thr` is caught by
test_topk_grouped alone, through the rows whose floor is the float just above one of their scores (anywhere else the extra entry equals the
list's own last value and changes nothing); skipping the rows_left mask of the BLOCKMAX epilogue changes no result: rows past the end are
staged as copies of the last valid item (with an item bias of -inf where there is one), so a maximum cannot see them."""
import functools
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import score_reference as R
from oracle import oracle as O
from score_reference import DT_BF16, DT_F32, F32, MODE_DOT, MODE_EUCLID, f64

pytestmark = pytest.mark.gpu

RATIOS = {}
UNSET = -(2 ** 31) + 12345                                    # no tuning holds this value
TUNINGS = ("blockmax_pipelined", "blockmax_pipelined_f32")
SENT, SENT_I = F32(-12345.5), np.int32(-777)
BASE = 1000
MODE_NAME = {MODE_DOT: "dot", MODE_EUCLID: "euclid"}
DKM = [(dt, kp, mode) for dt, kp in R.SCORE_CASES for mode in (MODE_DOT, MODE_EUCLID)]
DKM_IDS = ["%s-k%d-%s" % (R.DT_NAME[dt], kp, MODE_NAME[mode]) for dt, kp, mode in DKM]
DK_IDS = ["%s-k%d" % (R.DT_NAME[dt], kp) for dt, kp in R.SCORE_CASES]


@pytest.fixture(scope="module")
def N():
    from tensorrec_amd import _native
    _native.require_gpu()
    lib = _native.load()
    before = [lib.trec_get_tuning(k.encode(), UNSET) for k in TUNINGS]
    yield _native
    assert [lib.trec_get_tuning(k.encode(), UNSET) for k in TUNINGS] == before, "a test left a tuning behind"
    out = os.environ.get("TREC_SCORE_RATIOS_OUT")
    if out:
        with open(out, "w") as f:
            json.dump({k: float("%.4g" % v) for k, v in sorted(RATIOS.items())}, f, indent=1)
            f.write("\n")


@pytest.fixture(scope="module")
def ops(N):
    from tensorrec_amd import ops as _ops
    return _ops


class tunings(object):
    """``with tunings(N, blockmax_pipelined=0):`` -- set through _native.set_tuning, put back on exit (a knob that was not set is cleared)"""

    def __init__(self, N, **values):
        self.N, self.values = N, values

    def __enter__(self):
        lib = self.N.load()
        self.before = {k: lib.trec_get_tuning(k.encode(), UNSET) for k in self.values}
        try:
            for k, v in self.values.items():
                self.N.set_tuning(k, v)
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        for k, v in self.before.items():
            if v == UNSET:
                self.N.clear_tuning(k)
            else:
                self.N.set_tuning(k, v)
        return False


def kernel_tunings(N, kernel):
    """the tunings that send trec_score_gemm_blockmax to a kernel form of the case table"""
    on = 0 if kernel == "generic" else 1
    return tunings(N, blockmax_pipelined=on, blockmax_pipelined_f32=on)


def dev(a):
    """a device copy (None -> None); bf16 bit patterns travel as int16"""
    if a is None:
        return None
    a = np.array(a, order="C")                                 # (a copy: the cached inputs of score_reference are read-only)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def full(shape, value):
    return torch.full(shape, value.item(), dtype=torch.int32 if isinstance(value, np.int32) else torch.float32, device="cuda")


@functools.lru_cache(maxsize=8)
def on_device(P):
    return SimpleNamespace(u=dev(P.u_op), v=dev(P.v_op), ub=dev(P.ub), ib=dev(P.ib), usq=dev(P.usq), vsq=dev(P.vsq))


def dev_bias(D, bias):
    return (D.ub if bias in ("both", "user") else None), (D.ib if bias in ("both", "item") else None)


def note(dtype, kpad, mode, ratio):
    key = "%s-k%d-%s" % (R.DT_NAME[dtype], kpad, MODE_NAME[mode])
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    print("%s: largest error / bound %.3f" % (key, ratio))


def oracle_scores(P, mode, bias):
    """the fp32 bar on real data: the committed oracle's k-ordered fmaf chain on the operand values"""
    ub, ib = P.select(bias)
    if mode == MODE_EUCLID:
        return O.score_dense_euclid_exact(P.u_val, P.v_val, P.usq, P.vsq, ub, ib)
    return O.score_dense_exact(P.u_val, P.v_val, ub, ib)


# ------------------------------------------------------------------------------------------------ the calls
def run_store(N, P, mode, bias, variant=0):
    """trec_score_gemm_store into a [n_users + 1, n_items + 3] buffer; the padding and the row past the end must keep the sentinel"""
    D = on_device(P)
    ub, ib = dev_bias(D, bias)
    ld = P.n_items + 3
    out = full((P.n_users + 1, ld), SENT)
    N.call("trec_score_gemm_store", N.ptr(D.u), N.ptr(D.v), P.dtype, P.kpad, P.n_users, P.n_items, N.ptr(ub), N.ptr(ib), mode,
           N.ptr(D.usq) if mode else None, N.ptr(D.vsq) if mode else None, N.ptr(out), ld, variant)
    out = out.cpu().numpy()
    written = np.zeros(out.shape, bool)
    written[:P.n_users, :P.n_items] = True
    R.check_padding(out, written, SENT, "store")
    return np.ascontiguousarray(out[:P.n_users, :P.n_items])


def run_topk_lists(N, P, mode, bias, capacity, n_chunks, variant=0):
    """trec_score_gemm_topk: the partial lists (device tensors [n_users + 1, parts * capacity]; the last row must keep the sentinel)"""
    D = on_device(P)
    ub, ib = dev_bias(D, bias)
    parts = N.query("trec_score_topk_parts", P.dtype, P.kpad, P.n_items, n_chunks)
    assert parts == R.topk_parts(P.n_items, n_chunks)
    pv = full((P.n_users + 1, parts * capacity), SENT)
    pi = full((P.n_users + 1, parts * capacity), SENT_I)
    N.call("trec_score_gemm_topk", N.ptr(D.u), N.ptr(D.v), P.dtype, P.kpad, P.n_users, P.n_items, BASE, N.ptr(ub), N.ptr(ib), mode,
           N.ptr(D.usq) if mode else None, N.ptr(D.vsq) if mode else None, n_chunks, capacity, N.ptr(pv), N.ptr(pi), variant)
    assert bool((pv[-1] == SENT.item()).all()) and bool((pi[-1] == SENT_I.item()).all()), "lists past the last user were written"
    return pv, pi


def run_merge(N, pv, pi, n_rows, k):
    """trec_topk_merge of the first n_rows rows of [*, n_cand] lists -> numpy (values, ids)"""
    ov, oi = full((n_rows + 1, k), SENT), full((n_rows + 1, k), SENT_I)
    N.call("trec_topk_merge", N.ptr(pv), N.ptr(pi), n_rows, pv.shape[1], k, N.ptr(ov), N.ptr(oi))
    ov, oi = ov.cpu().numpy(), oi.cpu().numpy()
    assert np.all(ov[-1] == SENT) and np.all(oi[-1] == SENT_I), "the merge wrote past the last row"
    return ov[:n_rows], oi[:n_rows]


def run_blockmax(N, P, mode, bias, sb_rows, n_chunks, variant=0):
    """trec_score_gemm_blockmax into a [n_sb + 1, n_users + 5] table; returns [n_sb, n_users]"""
    D = on_device(P)
    ub, ib = dev_bias(D, bias)
    n_sb = -(-P.n_items // sb_rows)
    stride = P.n_users + 5
    t = full((n_sb + 1, stride), SENT)
    N.call("trec_score_gemm_blockmax", N.ptr(D.u), N.ptr(D.v), P.dtype, P.kpad, P.n_users, P.n_items, N.ptr(ub), N.ptr(ib), mode,
           N.ptr(D.usq) if mode else None, N.ptr(D.vsq) if mode else None, sb_rows, n_chunks, N.ptr(t), stride, variant)
    t = t.cpu().numpy()
    written = np.zeros(t.shape, bool)
    written[:n_sb, :P.n_users] = True
    R.check_padding(t, written, SENT, "blockmax table")
    return np.ascontiguousarray(t[:n_sb, :P.n_users])


def check_topk(N, P, mode, bias, capacity, n_chunks, ks, variant=0, what=""):
    """lists + merge against the bar of the data's kind, for every k of ks (one kernel call, one merge per k)"""
    pv, pi = run_topk_lists(N, P, mode, bias, capacity, n_chunks, variant)
    for k in ks:
        gv, gi = run_merge(N, pv, pi, P.n_users, k)
        tag = "%s chunks %d k %d" % (what, n_chunks, k)
        if P.kind == "dyadic":
            R.check_topk_exact(gv, gi, P.restated(mode, bias), k, BASE, tag)
        elif P.dtype == DT_F32:
            R.check_topk_exact(gv, gi, oracle_scores(P, mode, bias), k, BASE, tag)
        else:
            s, b = P.reference(mode, bias)
            note(P.dtype, P.kpad, mode, R.check_topk_bounded(gv, gi, s, b, k, BASE, tag))


def test_geometry_queries_agree_with_the_reference(N):
    for dt, kp in R.SCORE_CASES:
        assert N.query("trec_score_rows_per_workgroup", dt, kp) == R.rows_per_workgroup(dt, kp)
        assert N.query("trec_score_tile_rows", dt, kp) == R.tile_rows(dt, kp)
    assert [N.query("trec_score_kpad", d) for d in (5, 33, 100, 129)] == [32, 64, 128, 256]
    assert [N.query("trec_score_topk_capacity", k) for k in (1, 8, 9, 12, 13, 16)] == [8, 8, 12, 12, 16, 16]


# ------------------------------------------------------------------------------------------------ STORE
def ragged(kind, dtype, kpad, d=None):
    """one workgroup and a row, two tiles and an item"""
    return R.problem(kind, dtype, kpad, R.rows_per_workgroup(dtype, kpad) + 1, 2 * R.tile_rows(dtype, kpad) + 1, d)


@pytest.mark.parametrize("c", R.cases("store"), ids=lambda c: c.id)
def test_store_dyadic(N, c):
    P = ragged("dyadic", c.dtype, c.kpad)
    R.same_bits(run_store(N, P, c.mode, c.bias, c.variant), P.restated(c.mode, c.bias), c.id)


@pytest.mark.parametrize("dtype,kpad,mode", DKM, ids=DKM_IDS)
def test_store_real(N, dtype, kpad, mode):
    P = ragged("real", dtype, kpad)
    for variant in ((0, 1) if dtype == DT_BF16 and mode == MODE_DOT else (0,)):
        got = run_store(N, P, mode, "both", variant)
        if dtype == DT_F32:
            R.same_bits(got, oracle_scores(P, mode, "both"), "store")
        else:
            s, b = P.reference(mode, "both")
            note(dtype, kpad, mode, R.check_store(got, s, b, "store variant %d" % variant))


@pytest.mark.parametrize("d", [5, 33, 100, 129])
@pytest.mark.parametrize("dtype", [DT_F32, DT_BF16], ids=["f32", "bf16"])
def test_store_d_below_kpad(N, dtype, d):
    kpad = N.query("trec_score_kpad", d)
    for mode in (MODE_DOT, MODE_EUCLID):
        P = ragged("dyadic", dtype, kpad, d)
        assert np.all(P.u_val[:, d:] == 0) and np.any(P.u_val[:, d - 1] != 0)
        R.same_bits(run_store(N, P, mode, "both"), P.restated(mode, "both"), "dyadic")
        P = ragged("real", dtype, kpad, d)
        got = run_store(N, P, mode, "both")
        if dtype == DT_F32:
            # the oracle on the UNPADDED operands: the zero columns add nothing to the chain
            ref = (O.score_dense_euclid_exact(P.u_val[:, :d], P.v_val[:, :d], P.usq, P.vsq, P.ub, P.ib) if mode else
                   O.score_dense_exact(P.u_val[:, :d], P.v_val[:, :d], P.ub, P.ib))
            R.same_bits(got, ref, "real")
        else:
            s, b = P.reference(mode, "both")
            note(dtype, kpad, mode, R.check_store(got, s, b, "real"))


# ------------------------------------------------------------------------------------------------ TOPK
def topk_problem(kind, dtype, kpad, n_users=None, n_items=300):
    return R.problem(kind, dtype, kpad, R.rows_per_workgroup(dtype, kpad) + 1 if n_users is None else n_users, n_items)


@pytest.mark.parametrize("c", R.cases("topk", "generic"), ids=lambda c: c.id)
def test_topk_dyadic(N, c):
    P = topk_problem("dyadic", c.dtype, c.kpad)
    for n_chunks in (1, 3):
        check_topk(N, P, c.mode, c.bias, c.capacity, n_chunks, (c.capacity, 1), c.variant, c.id)


@pytest.mark.parametrize("c", R.cases("topk", lambda k: k.startswith("tiling")), ids=lambda c: c.id)
def test_topk_tilings(N, c):
    """the experimental tilings of the hot configuration (variant >> 1 = 1, 2, 3 and 6), selected by trec_score_gemm_topk itself"""
    P = topk_problem("dyadic", c.dtype, c.kpad)
    for bias in ("both", "none", "user", "item"):
        for n_chunks in (1, 3):
            check_topk(N, P, c.mode, bias, c.capacity, n_chunks, (c.capacity, 1), c.variant, c.id + " bias " + bias)


@pytest.mark.parametrize("dtype,kpad,mode", DKM, ids=DKM_IDS)
def test_topk_real(N, dtype, kpad, mode):
    P = topk_problem("real", dtype, kpad)
    for capacity, n_chunks in ((8, 1), (12, 3), (16, 3)):
        for variant in ((0, 1) if dtype == DT_BF16 and mode == MODE_DOT else (0,)):
            check_topk(N, P, mode, "both", capacity, n_chunks, (capacity,), variant, "capacity %d variant %d" % (capacity, variant))


@pytest.mark.parametrize("dtype,kpad", R.SCORE_CASES, ids=DK_IDS)
def test_topk_edges(N, dtype, kpad):
    """fewer items than k (unused places -1 / -inf), a last chunk of one item, user counts around the rows of a workgroup; dot with both
    biases and Euclidean with a user bias only (no item bias: the padded rows of a partial tile are masked by the partial-tile mask alone)"""
    rows = R.rows_per_workgroup(dtype, kpad)
    for mode, bias in ((MODE_DOT, "both"), (MODE_EUCLID, "user"), (MODE_DOT, "user")):
        for n_items in (1, 7):
            check_topk(N, topk_problem("dyadic", dtype, kpad, 33, n_items), mode, bias, 8, 1, (8, 1), 0, "%d items" % n_items)
        for n_users in (1, rows - 1, rows, rows + 1):
            P = topk_problem("dyadic", dtype, kpad, n_users, 257)
            assert R.topk_parts(257, 2) == 4                            # chunks of 256 and 1
            check_topk(N, P, mode, bias, 12, 2, (12,), 0, "%d users" % n_users)


# ------------------------------------------------------------------------------------------------ BLOCKMAX
def accepts(c):
    return c.kernel == "generic" or (c.mode == MODE_DOT and c.kpad in (64, 128))


@pytest.mark.parametrize("c", R.cases("blockmax"), ids=lambda c: c.id)
def test_blockmax_dyadic(N, c):
    """the table itself, every cell, for the kernel form the case names"""
    assert accepts(c)
    big, small = R.problem("dyadic", c.dtype, c.kpad, 513, 1300), R.problem("dyadic", c.dtype, c.kpad, 5, 129)
    with kernel_tunings(N, c.kernel):
        for P, sb_rows, n_chunks in ((big, 128, 3), (big, 256, 1), (big, 512, 3), (small, 128, 1), (small, 128, 3)):
            got = run_blockmax(N, P, c.mode, c.bias, sb_rows, n_chunks, c.variant)
            R.same_bits(got, R.blockmax(P.restated(c.mode, c.bias), sb_rows), "%s sb_rows %d chunks %d" % (c.id, sb_rows, n_chunks))


SHAPE_FORMS = [("generic", DT_F32, 64, MODE_DOT), ("generic", DT_F32, 32, MODE_EUCLID), ("generic", DT_BF16, 128, MODE_DOT),
               ("generic", DT_BF16, 256, MODE_EUCLID), ("pipelined", DT_BF16, 64, MODE_DOT), ("pipelined", DT_BF16, 128, MODE_DOT),
               ("pipelined_f32", DT_F32, 64, MODE_DOT), ("pipelined_f32", DT_F32, 128, MODE_DOT), ("filter16", DT_BF16, 64, MODE_DOT),
               ("filter16", DT_BF16, 128, MODE_DOT)]


@pytest.mark.parametrize("kernel,dtype,kpad,mode", SHAPE_FORMS,
                         ids=["%s-%s-k%d-%s" % (k, R.DT_NAME[dt], kp, MODE_NAME[m]) for k, dt, kp, m in SHAPE_FORMS])
def test_blockmax_shapes(N, kernel, dtype, kpad, mode):
    """superblocks that end inside a tile (70 = 64 + 6, 1300 = 2 * 512 + 4 * 64 + 20) and inside a 32-row block, a superblock of one item
    (129, 1025), 5 and 513 users, every superblock height and chunk count.  Where the pipelined fp32 kernel runs, the generic one gives the
    same table."""
    variant = 32 if kernel == "filter16" else 0
    for n_users in (5, 513):
        for n_items in (70, 129, 1025, 1300):
            P = R.problem("dyadic", dtype, kpad, n_users, n_items)
            for sb_rows in (128, 256, 512):
                want = R.blockmax(P.restated(mode, "both"), sb_rows)
                for n_chunks in (1, 3):
                    what = "%d x %d sb_rows %d chunks %d" % (n_users, n_items, sb_rows, n_chunks)
                    with kernel_tunings(N, kernel):
                        got = run_blockmax(N, P, mode, "both", sb_rows, n_chunks, variant)
                    R.same_bits(got, want, what)
                    if kernel == "pipelined_f32":
                        with kernel_tunings(N, "generic"):
                            R.same_bits(run_blockmax(N, P, mode, "both", sb_rows, n_chunks, variant), got, what + " generic")


@pytest.mark.parametrize("dtype,kpad,mode", DKM, ids=DKM_IDS)
def test_blockmax_declined_configurations_fall_to_the_generic_kernel(N, dtype, kpad, mode):
    """with the hand-scheduled kernels switched on (the default), K = 32 / 256 and Euclidean launches are declined by them and must give
    the generic kernel's table; K = 64 / 128 dot launches are theirs and must give the same table too (dyadic data: every form is exact)"""
    P = R.problem("dyadic", dtype, kpad, 513, 1300)
    with kernel_tunings(N, "generic"):
        generic = run_blockmax(N, P, mode, "both", 256, 3)
    with kernel_tunings(N, "pipelined"):
        R.same_bits(run_blockmax(N, P, mode, "both", 256, 3), generic, "hand-scheduled kernels on")
    R.same_bits(generic, R.blockmax(P.restated(mode, "both"), 256), "generic")


REAL_FORMS = ([("pipelined", DT_BF16, kp, MODE_DOT) for kp in (64, 128)] + [("filter16", DT_BF16, kp, MODE_DOT) for kp in (64, 128)] +
              [("pipelined_f32", DT_F32, kp, MODE_DOT) for kp in (64, 128)] +
              [("generic", dt, kp, MODE_DOT) for dt in (DT_F32, DT_BF16) for kp in R.KPADS] +
              [("generic", dt, kp, MODE_EUCLID) for dt in (DT_F32, DT_BF16) for kp in R.KPADS])


@pytest.mark.parametrize("kernel,dtype,kpad,mode", REAL_FORMS,
                         ids=["%s-%s-k%d-%s" % (k, R.DT_NAME[dt], kp, MODE_NAME[m]) for k, dt, kp, m in REAL_FORMS])
def test_blockmax_real(N, kernel, dtype, kpad, mode):
    P = R.problem("real", dtype, kpad, 513, 1300)
    for sb_rows, n_chunks in ((256, 3), (512, 1)):
        with kernel_tunings(N, kernel):
            got = run_blockmax(N, P, mode, "both", sb_rows, n_chunks, 32 if kernel == "filter16" else 0)
        if dtype == DT_F32:
            R.same_bits(got, R.blockmax(oracle_scores(P, mode, "both"), sb_rows), kernel)
        else:
            s, b = P.reference(mode, "both")
            note(dtype, kpad, mode, R.check_blockmax(got, s, b, sb_rows, kernel))


# ------------------------------------------------------------------------------------------------ grouped / hot BLOCKMAX (bf16, 16x16x32)
G_USERS, G_ITEMS, G_SB = 1300, 3000, 512            # 6 superblocks, the last of 440 items (6 tiles and 56 rows)


def check_listed_cells(P, bias, table, keep, what):
    """the cells of `keep` [n_sb, n_users] equal the reference maxima (dyadic: bit for bit; real: within the bound), all others -- the
    bm_stride padding included -- keep the sentinel"""
    n_sb = keep.shape[0]
    written = np.zeros(table.shape, bool)
    written[:n_sb, :P.n_users] = keep
    R.check_padding(table, written, SENT, what)
    got = table[:n_sb, :P.n_users]
    if P.kind == "dyadic":
        want = R.blockmax(P.restated(MODE_DOT, bias), G_SB)
        R.same_bits(got[keep], want[keep], what)
    else:
        s, b = P.reference(MODE_DOT, bias)
        note(P.dtype, P.kpad, MODE_DOT, R.within(got[keep], R.blockmax(s, G_SB)[keep], R.blockmax(b, G_SB)[keep], what))


@pytest.mark.parametrize("kind", ["dyadic", "real"])
@pytest.mark.parametrize("kpad", [64, 128])
def test_blockmax_grouped(N, kpad, kind):
    """trec_score_gemm_blockmax_grouped: the list layout (wgs_per_row = 0: a superblock per workgroup, -1 rows pad every superblock's
    users to 512, one idle workgroup) and the fixed-capacity layout (rblock_chunk = the superblocks' row counts)"""
    P = R.problem(kind, DT_BF16, kpad, G_USERS, G_ITEMS)
    D = on_device(P)
    rng = np.random.default_rng(kpad)
    n_sb = -(-G_ITEMS // G_SB)
    stride = G_USERS + 5
    keep = rng.random((n_sb, G_USERS)) < 0.45
    keep[2] = rng.random(G_USERS) < 0.05                              # a superblock with a single, mostly empty workgroup
    for bias in (("both", "none", "user", "item") if kind == "dyadic" else ("both",)):
        ub, ib = dev_bias(D, bias)
        rows, chunks = [], []
        for s in range(n_sb):
            us = rng.permutation(np.nonzero(keep[s])[0])
            pad = (-len(us)) % 512
            rows.append(np.concatenate([us, np.full(pad, -1)]))
            chunks += [s] * ((len(us) + pad) // 512)
            if s == 1:                                                # an idle workgroup: whatever its rows say, it writes nothing
                rows.append(np.arange(512))
                chunks.append(-1)
        row_user, rblock_chunk = dev(np.concatenate(rows).astype(np.int32)), dev(np.asarray(chunks, np.int32))
        table = full((n_sb + 1, stride), SENT)
        N.call("trec_score_gemm_blockmax_grouped", N.ptr(D.u), N.ptr(D.v), kpad, row_user.numel(), G_ITEMS, N.ptr(ub), N.ptr(ib), G_SB,
               N.ptr(rblock_chunk), N.ptr(row_user), N.ptr(table), stride, 0)
        check_listed_cells(P, bias, table.cpu().numpy(), keep, "list layout, bias " + bias)
        rcap = 1024
        counts = keep.sum(1).astype(np.int32)
        assert 512 < counts.max() <= rcap and counts.min() < 512
        ru = np.full((n_sb, rcap), -1, np.int32)
        for s in range(n_sb):
            ru[s, :counts[s]] = rng.permutation(np.nonzero(keep[s])[0])
            ru[s, counts[s]:] = rng.integers(0, G_USERS, rcap - counts[s])       # rows past the count are not rows
        dcounts, dru = dev(counts), dev(ru.reshape(-1))
        table = full((n_sb + 1, stride), SENT)
        N.call("trec_score_gemm_blockmax_grouped", N.ptr(D.u), N.ptr(D.v), kpad, n_sb * rcap, G_ITEMS, N.ptr(ub), N.ptr(ib), G_SB,
               N.ptr(dcounts), N.ptr(dru), N.ptr(table), stride, rcap // 512)
        check_listed_cells(P, bias, table.cpu().numpy(), keep, "fixed-capacity layout, bias " + bias)


@pytest.mark.parametrize("kind", ["dyadic", "real"])
@pytest.mark.parametrize("kpad", [64, 128])
def test_blockmax_hot(N, kpad, kind):
    """trec_score_gemm_blockmax_hot: the listed superblocks for EVERY user, hot_list padded with -1"""
    P = R.problem(kind, DT_BF16, kpad, G_USERS, G_ITEMS)
    D = on_device(P)
    n_sb = -(-G_ITEMS // G_SB)
    stride = G_USERS + 5
    for bias in (("both", "none", "user", "item") if kind == "dyadic" else ("both",)):
        ub, ib = dev_bias(D, bias)
        for hot in ([1, 5, -1, -1], [0], [-1, -1]):
            keep = np.zeros((n_sb, G_USERS), bool)
            keep[[s for s in hot if s >= 0]] = True
            hot_list = dev(np.asarray(hot, np.int32))
            table = full((n_sb + 1, stride), SENT)
            N.call("trec_score_gemm_blockmax_hot", N.ptr(D.u), N.ptr(D.v), kpad, G_USERS, G_ITEMS, N.ptr(ub), N.ptr(ib), G_SB,
                   N.ptr(hot_list), len(hot), N.ptr(table), stride)
            check_listed_cells(P, bias, table.cpu().numpy(), keep, "hot %s, bias %s" % (hot, bias))


# ------------------------------------------------------------------------------------------------ grouped TOPK
T_USERS, T_ITEMS, T_SB = 700, 1300, 512             # 3 superblocks, the last of 276 items


def grouped_expected(s32, user, sb, floor, capacity, half=None):
    """the best `capacity` scores >= floor of user `user` among the items of superblock `sb` (of one half-wave's rows with `half`), ids
    global + BASE; (values [capacity], ids [capacity])"""
    lo, hi = sb * T_SB, min(T_ITEMS, (sb + 1) * T_SB)
    row = s32[user, lo:hi].copy()
    item = np.arange(lo, hi)
    mask = row >= floor
    if half is not None:
        # acc = mfma(items, users): register r of half-wave h holds the block's item row cd_row(r, h) = (r & 3) + 8 (r >> 2) + 4 h, so
        # half-wave h owns the items with bit 2 of (item % 32) equal to h (superblocks start on multiples of 32)
        mask &= ((item >> 2) & 1) == half
    row[~mask] = -np.inf
    v, i = R.topk(row[None, :], capacity, BASE + lo)
    i[v == -np.inf] = -1
    return v[0], i[0]


@pytest.mark.parametrize("mode", [MODE_DOT, MODE_EUCLID], ids=["dot", "euclid"])
@pytest.mark.parametrize("dtype,kpad", [(dt, kp) for dt in (DT_F32, DT_BF16) for kp in (64, 128)],
                         ids=["%s-k%d" % (R.DT_NAME[dt], kp) for dt in (DT_F32, DT_BF16) for kp in (64, 128)])
def test_topk_grouped(N, dtype, kpad, mode):
    """trec_score_gemm_topk_grouped on dyadic data: rows grouped by superblock and padded to the rows of a workgroup, one idle workgroup,
    row_pair scattering the lists; the gathered operand and the row_index form give the same lists; floors; independent lists"""
    P = R.problem("dyadic", dtype, kpad, T_USERS, T_ITEMS)
    D = on_device(P)
    s32 = P.restated(mode, "both")
    rows_wg = R.rows_per_workgroup(dtype, kpad)
    rng = np.random.default_rng(100 * dtype + kpad + mode)
    n_sb = -(-T_ITEMS // T_SB)
    rows, chunks = [], []
    for s in range(n_sb):
        us = rng.permutation(np.nonzero(rng.random(T_USERS) < 0.5)[0])
        us[0] = R.DUP_USER if R.DUP_USER not in us else us[0]      # (the user whose best scores tie)
        pad = (-len(us)) % rows_wg
        assert len(us) > rows_wg
        rows.append(np.concatenate([us, np.full(pad, -1)]))
        chunks += [s] * ((len(us) + pad) // rows_wg)
        if s == 0:
            rows.append(np.full(rows_wg, -1))
            chunks.append(-1)
    row_index = np.concatenate(rows).astype(np.int32)
    row_sb = np.repeat(np.asarray(chunks, np.int32), rows_wg)
    is_row = row_index >= 0
    n_pairs = int(is_row.sum())
    assert (~is_row).sum() > rows_wg                                  # -1 rows inside working workgroups, not only the idle one
    row_pair = np.full(len(row_index), -1, np.int32)
    row_pair[is_row] = rng.permutation(n_pairs)
    # floors per USER: its 1st .. 30th best score of the whole catalogue (so equality with the floor is met: listed), -inf, +inf
    order = np.sort(s32, axis=1)[:, ::-1]
    floor_u = order[np.arange(T_USERS), rng.integers(0, 30, T_USERS)].astype(F32)
    above = rng.random(T_USERS) < 0.25                               # ... or the float just above one: that score is BELOW the floor
    floor_u[above] = np.nextafter(floor_u[above], F32(np.inf))
    floor_u[rng.random(T_USERS) < 0.1] = -np.inf
    floor_u[rng.random(T_USERS) < 0.1] = np.inf
    floor_u[R.DUP_USER] = order[R.DUP_USER, 1]                       # the tied maximum itself
    src = np.maximum(row_index, 0)
    gathered = SimpleNamespace(
        u=dev(np.where(is_row[:, None], P.u_op[src], 0).astype(P.u_op.dtype)), ub=dev(np.where(is_row, P.ub[src], 0).astype(F32)),
        usq=dev(np.where(is_row, P.usq[src], 0).astype(F32)), floor=dev(np.where(is_row, floor_u[src], np.inf).astype(F32)), index=None)
    indexed = SimpleNamespace(u=D.u, ub=D.ub, usq=D.usq, floor=dev(floor_u), index=dev(row_index))
    d_chunk, d_pair = dev(np.asarray(chunks, np.int32)), dev(row_pair)
    pair_user, pair_sb = np.empty(n_pairs, np.int64), np.empty(n_pairs, np.int64)
    pair_user[row_pair[is_row]], pair_sb[row_pair[is_row]] = row_index[is_row], row_sb[is_row]

    def run(form, floor, capacity, variant):
        pv, pi = full(((n_pairs + 1) * 2, capacity), SENT), full(((n_pairs + 1) * 2, capacity), SENT_I)
        N.call("trec_score_gemm_topk_grouped", N.ptr(form.u), N.ptr(D.v), dtype, kpad, len(row_index), T_ITEMS, BASE, N.ptr(form.ub),
               N.ptr(D.ib), mode, N.ptr(form.usq) if mode else None, N.ptr(D.vsq) if mode else None, T_SB, N.ptr(d_chunk), N.ptr(d_pair),
               N.ptr(form.floor) if floor else None, capacity, N.ptr(pv), N.ptr(pi), variant, N.ptr(form.index))
        assert bool((pv[-2:] == SENT.item()).all()) and bool((pi[-2:] == SENT_I.item()).all()), "lists of no pair were written"
        return pv, pi

    for capacity, floor, variant in ((8, False, 0), (12, True, 0), (16, True, 1 if dtype == DT_BF16 else 0), (8, True, 16), (16, True, 16)):
        what = "capacity %d floor %s variant %d" % (capacity, floor, variant)
        pv, pi = run(gathered, floor, capacity, variant)
        pv2, pi2 = run(indexed, floor, capacity, variant)
        R.same_bits(pi2.cpu().numpy(), pi.cpu().numpy(), what + ": row_index form against gathered, ids")
        R.same_bits(pv2.cpu().numpy(), pv.cpu().numpy(), what + ": row_index form against gathered, values")
        fl = floor_u if floor else np.full(T_USERS, -np.inf, F32)
        if variant & 16:
            # independent lists: list 2 p + h on its own is the best `capacity` scores >= floor of half-wave h's rows
            lv, li = pv.cpu().numpy(), pi.cpu().numpy()
            want = [grouped_expected(s32, pair_user[p], pair_sb[p], fl[pair_user[p]], capacity, h) for p in range(n_pairs) for h in (0, 1)]
            R.same_bits(li[:2 * n_pairs], np.stack([w[1] for w in want]), what + " list ids")
            R.same_bits(lv[:2 * n_pairs], np.stack([w[0] for w in want]), what + " list values")
        gv, gi = run_merge(N, pv.view(n_pairs + 1, 2 * capacity), pi.view(n_pairs + 1, 2 * capacity), n_pairs, capacity)
        want = [grouped_expected(s32, pair_user[p], pair_sb[p], fl[pair_user[p]], capacity) for p in range(n_pairs)]
        R.same_bits(gi, np.stack([w[1] for w in want]), what + " merged ids")
        R.same_bits(gv, np.stack([w[0] for w in want]), what + " merged values")
        if floor:
            nothing = np.isin(pair_user, np.nonzero(floor_u == np.inf)[0])
            assert nothing.any() and np.all(gi[nothing] == -1) and np.all(gv[nothing] == -np.inf), "a floor of +inf lists nothing"


# ------------------------------------------------------------------------------------------------ trec_score_prep
@pytest.mark.parametrize("normalize", [0, 1], ids=["plain", "normalize"])
@pytest.mark.parametrize("dtype", [DT_F32, DT_BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("d", [5, 32, 100, 129, 256])
@pytest.mark.parametrize("n", [1, 257])
def test_score_prep(N, n, d, dtype, normalize):
    """score_prep_vec4_kernel<8 / 16 / 32> (d % 4 == 0) and score_prep_kernel (d = 5, 129) against NumPy.
    Bars (u = 2^-24): the squared norm is d fmaf terms in some order plus the butterfly, (d + 2) u relative; a normalised entry is
    x / sqrt(max(ss, 1e-12)) with half the norm's error, sqrtf, the division and the product: ((d + 2) / 2 + 4) u relative; its bf16 image
    lies between the roundings of the two ends of that interval (rounding is monotone)."""
    kpad = N.query("trec_score_kpad", d)
    rng = np.random.default_rng(1000 * n + d)
    x = (rng.standard_normal((n, d)) * rng.uniform(0.3, 3.0, (n, 1))).astype(F32)
    dx = dev(x)
    out = full((n + 1, kpad), SENT) if dtype == DT_F32 else torch.full((n + 1, kpad), 0x7B7B, dtype=torch.int16, device="cuda")
    sq = full((n + 1,), SENT)
    N.call("trec_score_prep", N.ptr(dx), n, d, kpad, normalize, dtype, N.ptr(out), N.ptr(sq))
    out, sq = out.cpu().numpy(), sq.cpu().numpy()
    assert sq[n] == SENT and np.all(out[n] == (SENT if dtype == DT_F32 else 0x7B7B)), "the row past the end was written"
    ss = (f64(x) ** 2).sum(1)
    assert np.all(np.abs(f64(sq[:n]) - ss) <= (d + 2) * R.U32 * ss)
    got = out[:n] if dtype == DT_F32 else R.bf16_value(out[:n].view(np.uint16))
    assert np.all(got[:, d:] == 0) and np.all(np.signbit(got[:, d:]) == 0), "padding columns are not +0"
    if not normalize:
        R.same_bits(got[:, :d], x if dtype == DT_F32 else R.bf16_value(R.bf16_bits(x)), "operand")
        return
    y = f64(x) / np.sqrt(np.maximum(ss, 1e-12))[:, None]
    bar = ((d + 2) / 2.0 + 4) * R.U32 * np.abs(y)
    if dtype == DT_F32:
        R.within(got[:, :d], y, bar, "normalised operand")
    else:
        lo, hi = R.bf16_value(R.bf16_bits((y - bar).astype(F32))), R.bf16_value(R.bf16_bits((y + bar).astype(F32)))
        assert np.all((got[:, :d] >= lo) & (got[:, :d] <= hi)), "normalised bf16 operand"


# ------------------------------------------------------------------------------------------------ housekeeping
def test_tunings_are_put_back(N):
    """every test above sets blockmax_pipelined / blockmax_pipelined_f32 inside `with kernel_tunings`, which restores them even when the
    body raises; none is set now (the module fixture checks the same once more after the last test)"""
    lib = N.load()
    before = [lib.trec_get_tuning(k.encode(), UNSET) for k in TUNINGS]
    with pytest.raises(RuntimeError, match="boom"):
        with kernel_tunings(N, "generic"):
            assert [lib.trec_get_tuning(k.encode(), UNSET) for k in TUNINGS] == [0, 0]
            raise RuntimeError("boom")
    assert [lib.trec_get_tuning(k.encode(), UNSET) for k in TUNINGS] == before
    with kernel_tunings(N, "pipelined"):
        assert [lib.trec_get_tuning(k.encode(), UNSET) for k in TUNINGS] == [1, 1]
    assert [lib.trec_get_tuning(k.encode(), UNSET) for k in TUNINGS] == before
