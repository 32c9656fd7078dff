"""The int8 stage (csrc/score_blockmax_i8.hip) at the places its tile body and its superblock end can go wrong, against tests/i8_reference.py,
bit for bit as in tests/test_gpu_i8_stage.py (same operands pool, same acceptance helpers).

The kernel takes the two max3 of a 16-item block's accumulators in front of the MFMA of the NEXT block that overwrites them, flushes the last
block of a tile behind the tile, and combines the four row-groups' maxima (item index mod 16 in 0-3, 4-7, 8-11, 12-15: the four accumulator
registers' rows, one row-group per 16 lanes) at a superblock end by a reduce-scatter of v_permlane32_swap / v_permlane16_swap, after which
row-group g owns the user blocks OW g .. OW g + OW - 1 of its wave.  What can go wrong: a block whose maxima are never taken (the first or the
last of a tile, the last of a chunk), a tile that is flushed into the wrong superblock, a lane of the reduce-scatter that is dropped or lands in
another user block's column.

test_item_and_user_edges     item counts that end a chunk on every kind of boundary (16, 17, 127, 129, sb_rows + 1, 2 sb_rows - 1; sb_rows 128 = one
                             tile per superblock: flush and combine at every tile, and 512; 1 and 2 chunks) x user counts W - 1, W, W + 1 (W rows
                             per workgroup: a workgroup with one live row, row-groups whose blocks are all padding)
test_planted_maximum         W users with all-positive rows, every superblock with ONE item of all +127 (and the largest bias): that item is the
                             strict maximum of its superblock for every user at once, so every user block of every wave depends on the one
                             row-group it sits in.  Over the superblocks of a problem and two problems the item stands in each of the four
                             row-groups, in the first and in the last block of a tile, in every tile of a superblock.
test_host_model_of_the_combine_rejects_a_missing_swap    (no GPU) a NumPy model of the per-lane maxima and the two swap rounds reproduces the
                             reference on the planted operands, and with any ONE swap left out R.check_table rejects its table.
Cases: TK 0, 10 and 16 at kpad 128, TK 10 at kpad 64; bias forms none and both (none on one scale, both on scale classes).
The file takes about 3 s of wall time on the MI355X."""
import numpy as np
import pytest

import i8_reference as R
from i8_reference import F32

SENT = F32(-12345.5)
GRID = {c.id: c for c in R.grid()}
CASES = [GRID[i] for i in ("k128-tk0-none-one_scale", "k128-tk0-both-classes", "k128-tk10-none-one_scale", "k128-tk10-both-classes",
                           "k128-tk16-none-one_scale", "k128-tk16-both-classes", "k64-tk10-none-one_scale", "k64-tk10-both-classes")]


@pytest.fixture(scope="module")
def N():
    from tensorrec_amd import _native
    _native.require_gpu()
    _native.load()
    return _native


def run_stage(N, p, n_chunks, top_k):
    """one trec_score_gemm_blockmax_i8 call on sentinel-filled outputs -> (table, lists or None) on the host"""
    import torch

    def dev(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    stride = p.n_users + 4
    t = dict(uq=dev(p.uq), iq=dev(p.iq), ub=dev(p.ub), bq=dev(p.bias_q), sbs=dev(p.sb_stats), err=dev(p.r_err), wgs=dev(p.wg_scale), wgc=dev(p.wg_class),
             scales=dev(p.scales if p.wg_scale is None else np.array([1e9, 0, 0], F32)))
    table = torch.full((p.n_sb, stride), float(SENT), dtype=torch.float32, device="cuda")
    ctop = torch.full((n_chunks * top_k, stride), float(SENT), dtype=torch.float32, device="cuda") if top_k else None
    N.call("trec_score_gemm_blockmax_i8", N.ptr(t["uq"]), N.ptr(t["iq"]), p.kt, p.n_users, p.n_items, N.ptr(t["ub"]), N.ptr(t["bq"]), N.ptr(t["scales"]),
           N.ptr(t["sbs"]), p.sb_rows, n_chunks, N.ptr(table), stride, N.ptr(t["err"] if top_k else None), N.ptr(ctop), top_k, N.ptr(t["wgs"]),
           N.ptr(t["wgc"]), p.wg_rows if p.wg_scale is not None else 0)
    return table.cpu().numpy(), (ctop.cpu().numpy() if top_k else None)


def check(N, p, what):
    want = R.stage_table(p)
    lb = R.lower_bounds(want, R.stage_bound(p)) if p.tk else None
    for n_chunks in (1, 2):
        table, ctop = run_stage(N, p, n_chunks, p.tk)
        R.check_table(table, want, p.written, SENT, "%s chunks %d: table" % (what, n_chunks))
        if p.tk:
            R.check_lists(ctop, R.lists(lb, p.n_items, n_chunks, p.sb_rows, p.tk), p.written, SENT, "%s chunks %d: lists" % (what, n_chunks))


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_item_and_user_edges(N, c):
    W = R.rows_per_workgroup(c.tk)
    for n_users in (W - 1, W, W + 1):
        for sb in (128, 512):
            for n_items in (16, 17, 127, 129, sb + 1, 2 * sb - 1):
                check(N, R.stage_problem(c, n_users, n_items, sb), "%s users %d items %d sb %d" % (c.id, n_users, n_items, sb))


# ------------------------------------------------------------------------------------------------ the planted maximum
N_SB = 5


def planted_item(s, shift, sb_rows):
    """superblock s of a problem: row-group (s + shift) % 4, the first block of a tile for (s + shift) % 8 < 4 and the last one else, tile s of the superblock"""
    combo = (s + shift) % 8
    g, blk, tile = combo % 4, (7 if combo >= 4 else 0), s % (sb_rows // R.BNQ)
    return s * sb_rows + tile * R.BNQ + blk * 16 + 4 * g + (s + shift) % 4, g, blk


def planted_problem(c, sb_rows, shift):
    W = R.rows_per_workgroup(c.tk)
    p = R.stage_problem(c, W, N_SB * sb_rows, sb_rows)
    rng = np.random.default_rng(17 * sb_rows + shift + c.kt)
    uq = np.maximum(np.abs(p.uq.astype(np.int16)), 1).astype(np.int8)          # every element of every user in 1 .. 127
    iq = np.minimum(p.iq, 126).astype(np.int8)                                 # no element of any other item reaches 127
    items = [planted_item(s, shift, sb_rows)[0] for s in range(N_SB)]
    iq[items] = 127
    if p.bias_q is not None:                                                   # small biases, the planted items with the largest of them
        bq = p.bias_q.copy()
        rows = [bq] if bq.ndim == 1 else [bq[cl] for cl in sorted(set(int(x) for x in p.wg_class if x >= 0))]
        for r in rows:
            r[:] = rng.integers(-3000, 3001, p.n_items)
            r[items] = 3001
        p.bias_q = bq
    p.uq, p.iq, p.dots, p.planted = uq, iq, R.int_dots(uq, iq), items
    return p


def integer_scores(p):
    s = p.dots.copy()
    if p.bias_q is not None:
        for cl in np.unique(p.class_u):
            s[p.class_u == cl] += R.f64(p.bias_q[max(cl, 0)] if p.bias_q.ndim == 2 else p.bias_q)[None, :]
    return s


def assert_planted(p):
    """the test's own premise: in every superblock the planted item is the strict maximum of every user"""
    s = integer_scores(p).reshape(p.n_users, p.n_sb, p.sb_rows)
    for j, item in enumerate(p.planted):
        blk = s[:, j, :]
        assert np.all(blk.argmax(1) == item - j * p.sb_rows)
        assert np.all(np.partition(blk, -2, axis=1)[:, -2] < blk.max(1))


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_planted_maximum(N, c):
    seen = set()
    for sb in (128, 512):
        for shift in (0, 4):
            p = planted_problem(c, sb, shift)
            assert_planted(p)
            seen |= {planted_item(s, shift, sb)[1:] for s in range(N_SB)}
            check(N, p, "%s planted sb %d shift %d" % (c.id, sb, shift))
    assert seen == {(g, blk) for g in range(4) for blk in (0, 7)}


# ------------------------------------------------------------------------------------------------ host model of the combine
def swap32(a, b):
    """v_permlane32_swap on [..., 4 rows of 16 lanes, 16]: the upper half of the first operand changes places with the lower half of the second"""
    r0, r1 = a.copy(), b.copy()
    r0[..., 2:4, :], r1[..., 0:2, :] = b[..., 0:2, :], a[..., 2:4, :]
    return r0, r1


def swap16(a, b):
    """v_permlane16_swap: the odd rows of the first operand change places with the even rows of the second"""
    r0, r1 = a.copy(), b.copy()
    r0[..., 1, :], r0[..., 3, :], r1[..., 0, :], r1[..., 2, :] = b[..., 0, :], b[..., 2, :], a[..., 1, :], a[..., 3, :]
    return r0, r1


def model_maxima(p, nub, skip=None):
    """[n_sb, n_users] integer maxima the way the kernel forms them: per lane (row-group g, user lu of block ub) the maximum over the superblock's
    items of row-group g, then the two swap rounds; skip = ("32", j) or ("16", o) leaves that one swap out (its operands stay where they are)"""
    ow = nub // 4
    s = integer_scores(p).reshape(p.n_users, p.n_sb, p.sb_rows // 16, 4, 4).max(axis=(2, 4))          # [user, sb, g]
    n_wave = p.n_users // (nub * 16)
    bm = s.reshape(n_wave, nub, 16, p.n_sb, 4).transpose(3, 0, 1, 4, 2)                               # [sb, wave, ub, g, lu]
    h = []
    for j in range(nub // 2):
        a, b = bm[:, :, j], bm[:, :, j + nub // 2]
        if skip != ("32", j):
            a, b = swap32(a, b)
        h.append(np.maximum(a, b))
    out = np.empty((p.n_sb, n_wave, nub, 16))
    for o in range(ow):
        a, b = h[o], h[o + ow]
        if skip != ("16", o):
            a, b = swap16(a, b)
        m = np.maximum(a, b)                                                                          # [sb, wave, g, lu]
        for g in range(4):
            out[:, :, ow * g + o, :] = m[:, :, g, :]                                                  # row-group g owns the blocks ow g + o
    return out.reshape(p.n_sb, p.n_users)


def table_of(p, m):
    """R.stage_table's conversion of integer maxima"""
    v = m.astype(F32) * (p.a_u[None, :] * p.sb_stats[:, 0][:, None])
    if p.case.bias != "none":
        v = v + (p.ub if p.ub is not None else np.zeros(p.n_users, F32))[None, :]
    return v


@pytest.mark.parametrize("c", [GRID["k128-tk10-both-classes"], GRID["k128-tk16-none-one_scale"]], ids=["nub12", "nub8"])
def test_host_model_of_the_combine_rejects_a_missing_swap(c):
    p = planted_problem(c, 128, 0)
    assert_planted(p)
    want = R.stage_table(p)
    R.check_table(table_of(p, model_maxima(p, c.nub)), want, p.written, SENT, "the model with every swap")
    for skip in [("32", j) for j in range(c.nub // 2)] + [("16", o) for o in range(c.nub // 4)]:
        with pytest.raises(AssertionError, match="entries differ"):
            R.check_table(table_of(p, model_maxima(p, c.nub, skip)), want, p.written, SENT, "the model without swap %s %d" % skip)
