"""The selection and glue kernels of the exact top-k against tests/topk_glue_reference.py, stage by stage, through _native.call with raw
tensors (tests/test_topk_glue_reference_host.py shows on the CPU that the case lists reach every instantiation and tell a subtly wrong
kernel from a right one).  The end-to-end tests (test_gpu_cascade.py, test_gpu_filter.py, test_gpu_candidates.py) only see the final lists,
and the three tiers of fallback behind predict_top_k keep those the same when a glue kernel flags too many users or empties a list.

Everything is compared for equality (floats by their bits) except the floors, which are held to the bracket of the reference's docstring,
and the lists whose order follows atomics (trec_topk_prerefine_rows_pos), which are held to their invariants.  Every call first asserts
that the dispatch rule sends it to the instantiation the case was written for.

With TREC_TOPK_GLUE_RATIOS_OUT=<file> the largest position of a floor inside its bracket (0 = the sound end, 1 = the tight end) is written
there at the end, per entry point (profiles/topk_glue_floor_ratios.json)."""
import json
import os

import numpy as np
import pytest
import torch

import topk_glue_reference as R
from topk_glue_reference import F32, I32, SENT_F, SENT_I, bits

pytestmark = pytest.mark.gpu

RATIOS = {}
UNSET = -(2 ** 31) + 12345                                    # no tuning holds this value


@pytest.fixture(scope="module")
def N():
    from tensorrec_amd import _native
    _native.require_gpu()
    _native.load()
    yield _native
    out = os.environ.get("TREC_TOPK_GLUE_RATIOS_OUT")
    if out:
        write_ratios(out)


def write_ratios(path):
    rec = {"what": "largest position of a floor inside its bracket [tau - mult E (1 + 2^-9) - 1e-29 - w, tau - mult E] (0 = the sound end, "
                   "1 = the tight end; tests/topk_glue_reference.py) per entry point over the cases of tests/test_gpu_topk_glue.py",
           "command": "TREC_TOPK_GLUE_RATIOS_OUT=<this file> python -m pytest -m gpu tests/test_gpu_topk_glue.py", "ratios": {}}
    if os.path.exists(path):
        with open(path) as f:
            rec["ratios"] = json.load(f).get("ratios", {})
    for k, v in RATIOS.items():
        rec["ratios"][k] = max(rec["ratios"].get(k, 0.0), float("%.4g" % v))
    rec["ratios"] = dict(sorted(rec["ratios"].items()))
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


def ratio(name, v):
    RATIOS[name] = max(RATIOS.get(name, 0.0), v)


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()


_ALIVE = []


@pytest.fixture(autouse=True)
def _release():
    yield
    torch.cuda.synchronize()
    del _ALIVE[:]


def P(N, a):
    """device pointer of a fresh device copy of a host array (None -> NULL); the copy lives until the test ends"""
    if a is None:
        return None
    _ALIVE.append(dev(a))
    return N.ptr(_ALIVE[-1])


def host(t):
    return t.cpu().numpy()


def table_dev(t):
    """the table on the device: a view `offset` floats into its flat buffer (offset 1: 4 bytes off 16-byte alignment)"""
    d = dev(t.flat)[t.offset:]
    assert (d.data_ptr() % 16 == 0) == (t.offset == 0)
    return d


def ifull(shape, v=SENT_I):
    return torch.full(shape, v, dtype=torch.int32, device="cuda")


def ffull(shape, v=float(SENT_F)):
    return torch.full(shape, v, dtype=torch.float32, device="cuda")


def same(got, want, what):
    got, want = host(got) if torch.is_tensor(got) else got, np.asarray(want)
    assert got.shape == want.shape, what
    if want.dtype == F32:
        got, want = bits(got), bits(want)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: %d entries differ, first at %s" % (what, len(bad), bad[0])


def set_select_tiled(N, value):
    """-> the value to put back (UNSET: it was not set)"""
    before = N.load().trec_get_tuning(b"select_tiled", UNSET)
    N.set_tuning("select_tiled", value)
    return before


def restore_select_tiled(N, before):
    if before == UNSET:
        N.clear_tuning("select_tiled")
    else:
        N.set_tuning("select_tiled", before)


# ------------------------------------------------------------------------------------------------------------------ 1. select
@pytest.mark.parametrize("k", R.SELECT_KS)
def test_select_blocks(N, k):
    """trec_topk_select_blocks (k <= 16, k_tau == k) / trec_topk_select_blocks_ex on all 30 shapes; both kernel forms wherever the table allows 16-byte loads"""
    for c in R.select_cases(k):
        t = R.make_table(c.n_sb, c.n_users, c.layout, c.kind, c.seed)
        d = table_dev(t)
        ref = R.select_blocks(t.table, c.n_users, k, c.k_tau)
        wide = R.wide_loads(c.n_users, c.layout)                            # (n_users + 1 is a multiple of 4 for n_users = 255)
        for tiled in ((1, 0) if wide else (1,)):
            want_form = "tiled" if (wide and c.n_sb >= 32 and tiled) else "lane"
            assert R.pick_select(k, c.n_sb, t.stride, d.data_ptr() % 16 == 0, tiled) == (R.select_ksel(k), want_form)
            sel = ifull((c.n_users, k))
            sel_max = None if c.nulls else ffull((k, c.n_users))
            tau = None if c.nulls else ffull((c.n_users,))
            before = set_select_tiled(N, tiled)
            try:
                if k <= 16 and c.k_tau == k:
                    N.call("trec_topk_select_blocks", N.ptr(d), c.n_sb, c.n_users, t.stride, k, N.ptr(sel), N.ptr(sel_max), N.ptr(tau))
                else:
                    N.call("trec_topk_select_blocks_ex", N.ptr(d), c.n_sb, c.n_users, t.stride, k, c.k_tau, N.ptr(sel), N.ptr(sel_max),
                           N.ptr(tau))
            finally:
                restore_select_tiled(N, before)
            what = "select k=%d k_tau=%d %s form=%s" % (k, c.k_tau, vars(c), want_form)
            same(sel, ref.sel, what + " sel")
            if not c.nulls:
                same(sel_max, ref.sel_max, what + " sel_max")
                same(tau, ref.tau, what + " tau")


# ------------------------------------------------------------------------------------------------------------------ 2. collect
@pytest.mark.parametrize("ksel", R.COLLECT_KSEL)
def test_collect_blocks(N, ksel):
    """trec_topk_collect_blocks and trec_topk_collect_blocks_masked: keys, count, flag, n_flagged; over-full users emptied and counted once;
    NaN entries and entries equal to the floor qualify; +inf floors; unmarked users (a whole workgroup of them) untouched"""
    for c in R.shapes(4 * R.COLLECT_KSEL.index(ksel) + 1, R.COLLECT_KINDS):
        t = R.make_table(c.n_sb, c.n_users, c.layout, c.kind, c.seed)
        d = table_dev(t)
        inp = R.collect_inputs(t.table, c.n_users, ksel, c.index)
        floor = dev(inp.floor)
        what = "collect ksel=%d %s" % (ksel, vars(c))
        # everybody
        ref = R.collect_blocks(t.table, c.n_users, inp.floor, ksel, inp.flag_in, inp.n_flagged_in)
        keys, count, flag, nfl = ifull((c.n_users, ksel)), ifull((c.n_users,)), dev(inp.flag_in), ifull((1,), inp.n_flagged_in)
        N.call("trec_topk_collect_blocks", N.ptr(d), c.n_sb, c.n_users, t.stride, N.ptr(floor), ksel, N.ptr(keys), N.ptr(count), N.ptr(flag),
               N.ptr(nfl))
        same(keys, ref.keys, what + " keys")
        same(count, ref.count, what + " count")
        same(flag, ref.flag, what + " flag")
        assert int(nfl.item()) == ref.n_flagged, what + " n_flagged"
        # the marked users only
        keys_in = np.full((c.n_users, ksel), SENT_I, dtype=I32)
        count_in = np.full(c.n_users, SENT_I, dtype=I32)
        ref = R.collect_blocks(t.table, c.n_users, inp.floor, ksel, inp.flag_in, inp.n_flagged_in, redo=inp.redo, keys_in=keys_in,
                               count_in=count_in)
        keys, count, flag, nfl = dev(keys_in), dev(count_in), dev(inp.flag_in), ifull((1,), inp.n_flagged_in)
        N.call("trec_topk_collect_blocks_masked", N.ptr(d), c.n_sb, c.n_users, t.stride, N.ptr(floor), ksel, N.ptr(keys), N.ptr(count),
               N.ptr(flag), N.ptr(nfl), P(N, inp.redo))
        same(keys, ref.keys, what + " masked keys")
        same(count, ref.count, what + " masked count")
        same(flag, ref.flag, what + " masked flag")
        assert int(nfl.item()) == ref.n_flagged, what + " masked n_flagged"


# ------------------------------------------------------------------------------------------------------------------ 3. scan + prune
@pytest.mark.parametrize("k", R.SCAN_KS)
def test_scan_prune_collect(N, k):
    """trec_topk_scan_blocks, trec_topk_prune_candidates and the masked collect behind them: each against its own reference, and the three
    together against the reference's select + collect over the table"""
    salt = R.SCAN_KS.index(k)
    assert R.pick_scan(k) == {1: 4, 4: 4, 5: 8, 8: 8, 9: 10, 10: 10, 11: 12, 12: 12, 13: 16, 16: 16}[k]
    for c in R.shapes(salt, R.COLLECT_KINDS):
        cap = R.SCAN_CAPS[(c.index + salt) % 3]
        ksel = R.COLLECT_KSEL[(c.index // 3 + salt) % 3]
        t = R.make_table(c.n_sb, c.n_users, c.layout, c.kind, c.seed)
        d = table_dev(t)
        inp = R.collect_inputs(t.table, c.n_users, ksel, c.index + 100)
        rng = np.random.default_rng(c.index)
        floor0 = (inp.floor - F32(0.25) * rng.integers(0, 3, c.n_users).astype(F32)).astype(F32)      # floor0 <= floor, often equal
        floor0[::6] = -np.inf
        what = "scan k=%d cap=%d ksel=%d %s" % (k, cap, ksel, vars(c))
        # --- scan
        ref = R.scan_blocks(t.table, c.n_users, k, floor0, cap)
        sel_max, tau = ffull((k, c.n_users)), ffull((c.n_users,))
        cs, cv, cn = ifull((cap, c.n_users)), ffull((cap, c.n_users)), ifull((c.n_users,))
        N.call("trec_topk_scan_blocks", N.ptr(d), c.n_sb, c.n_users, t.stride, k, P(N, floor0), cap, N.ptr(sel_max), N.ptr(tau),
               N.ptr(cs), N.ptr(cv), N.ptr(cn))
        clean = ~np.isnan(t.table[:, :c.n_users]).any(axis=0)          # (tau / sel_max of a column with a NaN: no contract)
        same(host(sel_max)[:, clean], ref.sel_max[:, clean], what + " sel_max")
        same(host(tau)[clean], ref.tau[clean], what + " tau")
        same(cs, ref.cand_s, what + " cand_s")
        same(cv, ref.cand_v, what + " cand_v")
        same(cn, ref.cand_n, what + " cand_n")
        # --- prune, from the kernel's own lists (they equal the reference's)
        pref = R.prune_candidates(ref.cand_s, ref.cand_v, ref.cand_n, cap, inp.floor, ksel, inp.flag_in, inp.n_flagged_in)
        keys, count, flag, nfl, redo = ifull((c.n_users, ksel)), ifull((c.n_users,)), dev(inp.flag_in), ifull((1,), inp.n_flagged_in), \
            ifull((c.n_users,))
        N.call("trec_topk_prune_candidates", N.ptr(cs), N.ptr(cv), N.ptr(cn), cap, P(N, inp.floor), ksel, c.n_users, N.ptr(keys),
               N.ptr(count), N.ptr(flag), N.ptr(nfl), N.ptr(redo))
        same(keys, pref.keys, what + " prune keys")
        same(count, pref.count, what + " prune count")
        same(flag, pref.flag, what + " prune flag")
        same(redo, pref.redo, what + " prune redo")
        assert int(nfl.item()) == pref.n_flagged, what + " prune n_flagged"
        # --- the masked collect finishes the marked users; together: the reference's collect over the table.  A user whose list was cut
        # short while its floor is +inf keeps what the cut list says (the contract of prune): left out of the composition
        N.call("trec_topk_collect_blocks_masked", N.ptr(d), c.n_sb, c.n_users, t.stride, P(N, inp.floor), ksel, N.ptr(keys),
               N.ptr(count), N.ptr(flag), N.ptr(nfl), N.ptr(redo))
        full = R.collect_blocks(t.table, c.n_users, inp.floor, ksel, inp.flag_in, inp.n_flagged_in)
        det = ~((ref.cand_n > cap) & np.isposinf(inp.floor))
        same(host(keys)[det], full.keys[det], what + " composed keys")
        same(host(count)[det], full.count[det], what + " composed count")
        same(host(flag)[det], full.flag[det], what + " composed flag")
        assert int(nfl.item()) == inp.n_flagged_in + int(((host(flag) != 0) & (inp.flag_in == 0)).sum()), what + " composed n_flagged"


# ------------------------------------------------------------------------------------------------------------------ 4. floors
@pytest.mark.parametrize("with_bias", (False, True))
@pytest.mark.parametrize("kdim", R.FLOOR_KDIMS)
@pytest.mark.parametrize("mult", R.FLOOR_MULTS)
def test_floors(N, mult, kdim, with_bias):
    """trec_topk_filter_floor_ex (flags given and NULL), trec_topk_filter_floor (mult 2) and trec_topk_cascade_floor (mult 1)"""
    for n_users in (1, 257, 700):
        inp = R.floor_inputs(n_users, kdim, with_bias, seed=int(mult))
        exp = R.floor_expect(inp, mult)
        tau, st, bias, gs = dev(inp.tau), dev(inp.ustats), dev(inp.bias), dev(inp.gstats)
        what = "floor mult=%g kdim=%d bias=%s n=%d" % (mult, kdim, with_bias, n_users)
        floor, flag, nfl = ffull((n_users,)), ifull((n_users,)), ifull((1,), 0)
        N.call("trec_topk_filter_floor_ex", N.ptr(tau), N.ptr(st), N.ptr(bias), N.ptr(gs), kdim, n_users, float(mult), N.ptr(floor),
               N.ptr(flag), N.ptr(nfl))
        ratio("filter_floor_ex", R.check_floor(host(floor), exp))
        same(flag, exp.flag, what + " flag")
        assert int(nfl.item()) == exp.n_flagged == int(host(flag).sum()), what + " n_flagged"
        floor2 = ffull((n_users,))
        N.call("trec_topk_filter_floor_ex", N.ptr(tau), N.ptr(st), N.ptr(bias), N.ptr(gs), kdim, n_users, float(mult), N.ptr(floor2), None, None)
        same(floor2, host(floor), what + " floor without flags")
        if mult == 2.0:
            floor3, flag3, nfl3 = ffull((n_users,)), ifull((n_users,)), ifull((1,), 0)
            N.call("trec_topk_filter_floor", N.ptr(tau), N.ptr(st), N.ptr(bias), N.ptr(gs), kdim, n_users, N.ptr(floor3), N.ptr(flag3),
                   N.ptr(nfl3))
            ratio("filter_floor", R.check_floor(host(floor3), exp))
            same(flag3, exp.flag, what + " filter_floor flag")
            assert int(nfl3.item()) == exp.n_flagged
        if mult == 1.0:
            for with_src in (False, True):
                src = None
                if with_src:
                    src = np.arange(n_users, dtype=I32)
                    src[6::4] = -1
                    src[:2] = -1                                           # (also a row whose statistics are bad: not flagged)
                cexp = R.floor_expect(inp, 1.0, cascade=True, src=src)
                tau_io, floor0, cflag, cnfl, cand_n = dev(inp.tau), ffull((n_users,)), ifull((n_users,)), ifull((1,), 0), ifull((n_users,))
                N.call("trec_topk_cascade_floor", N.ptr(tau_io), P(N, src), N.ptr(st), N.ptr(bias), N.ptr(gs), kdim, n_users,
                       N.ptr(floor0), N.ptr(cflag), N.ptr(cnfl), N.ptr(cand_n))
                ratio("cascade_floor", R.check_floor(host(floor0), cexp))
                same(tau_io, cexp.tau_out, what + " cascade tau")
                same(cflag, cexp.flag, what + " cascade flag")
                assert int(cnfl.item()) == cexp.n_flagged == int(host(cflag).sum())
                same(cand_n, np.zeros(n_users, I32), what + " cand_n")


# ------------------------------------------------------------------------------------------------------------------ 5. prerefine_rows_pos
@pytest.mark.parametrize("ci", range(len(R.PREREFINE_CASES)))
def test_prerefine_rows_pos(N, ci):
    c = R.PREREFINE_CASES[ci]
    inp = R.prerefine_inputs(ci)
    assert R.pick_prerefine(c.k) == ((16, 1024) if c.k <= 16 else (64, 256)) and c.n_users > R.pick_prerefine(c.k)[1]
    want, rc_ref = R.prerefine_want(inp.sel, inp.val, c.k, c.top_k, c.sb_per_chunk, c.n_sb, inp.src)
    assert not c.hot or rc_ref[0] > c.rcap
    sel_sb, sel_pos = ifull((c.n_users, c.k)), ifull((c.n_users, c.k))
    row_count, row_user, ok = ifull((c.n_sb,), 0), ifull((c.n_sb, c.rcap), -1), ifull((c.n_users,))
    N.call("trec_topk_prerefine_rows_pos", P(N, inp.sel), P(N, inp.val), c.k, c.top_k, c.sb_per_chunk, c.n_sb, c.n_users,
           P(N, inp.src), c.rcap, N.ptr(sel_sb), N.ptr(row_count), N.ptr(row_user), N.ptr(ok), N.ptr(sel_pos))
    R.check_prerefine(want, rc_ref, c.rcap, host(sel_sb), host(row_count), host(row_user), host(ok), host(sel_pos))


# ------------------------------------------------------------------------------------------------------------------ 6. prerefine_tau_listed
@pytest.mark.parametrize("k", R.TAU_LISTED_KS)
def test_prerefine_tau_listed(N, k):
    inp = R.tau_listed_inputs(k)
    exp = R.tau_listed_expect(inp)
    assert -(-k // 16) == {10: 1, 16: 1, 17: 2, 40: 3}[k]                  # rounds of 16 slots
    tau, vals, cf = dev(inp.tau), ffull((inp.n_users, k)), dev(inp.cand_floor)
    N.call("trec_topk_prerefine_tau_listed", P(N, inp.sel_sb), P(N, inp.sel_pos), P(N, inp.ok), k, P(N, inp.pre_max),
           inp.rcap, inp.n_users, P(N, inp.src), P(N, inp.ustats), P(N, inp.bias), P(N, inp.gstats), inp.kdim,
           N.ptr(tau), N.ptr(vals), N.ptr(cf))
    ratio("prerefine_tau_listed", R.check_tau_listed(inp, exp, host(tau), host(vals), host(cf)))


# ------------------------------------------------------------------------------------------------------------------ 7. rows_wg_map
@pytest.mark.parametrize("n_sb", R.WG_MAP_N_SB)
def test_rows_wg_map(N, n_sb):
    for wgs_per_row, short in ((1, False), (3, False), (3, True)):
        rc = R.wg_map_inputs(n_sb, wgs_per_row)
        total = int(R.rows_wg_map(rc, wgs_per_row, 1 << 20, guard=0).wg_start[-1])
        map_cap = max(total - 2, 0) if short else total + 5               # short: the map ends before the last entries
        ref = R.rows_wg_map(rc, wgs_per_row, map_cap)
        wg_start, wg_map = ifull((n_sb + 1,)), ifull((map_cap + 64,))
        N.call("trec_topk_rows_wg_map", P(N, rc), n_sb, wgs_per_row, N.ptr(wg_start), N.ptr(wg_map), map_cap)
        what = "wg_map n_sb=%d wgs_per_row=%d map_cap=%d" % (n_sb, wgs_per_row, map_cap)
        same(wg_start, ref.wg_start, what + " wg_start")
        same(wg_map, ref.wg_map, what + " wg_map (guard words included)")


# ------------------------------------------------------------------------------------------------------------------ 8. dense_users
@pytest.mark.parametrize("n_sb", R.DENSE_N_SB)
def test_dense_users(N, n_sb):
    for n_users, layout, limit in ((1, "aligned", 1), (255, "aligned", 16), (257, "odd", 32), (701, "offset", 20), (1026, "aligned", 24)):
        inp = R.dense_inputs(n_sb, n_users, layout, limit, seed=n_users)
        ref = R.dense_users(inp)
        d = dev(inp.flat)[inp.offset:]
        cf, flag, nfl = dev(inp.cand_floor), dev(inp.flag_in), ifull((1,), inp.n_flagged_in)
        N.call("trec_topk_dense_users", N.ptr(d), n_sb, n_users, inp.stride, P(N, inp.thr), P(N, inp.user_err),
               P(N, inp.sb_stats), inp.kdim, limit, N.ptr(cf), N.ptr(flag), N.ptr(nfl))
        what = "dense_users n_sb=%d n_users=%d %s limit=%d" % (n_sb, n_users, layout, limit)
        same(cf, ref.cand_floor, what + " cand_floor")
        same(flag, ref.flag, what + " flag")
        assert int(nfl.item()) == ref.n_flagged, what + " n_flagged"


# ------------------------------------------------------------------------------------------------------------------ 9. grouping glue
def test_group_keys(N):
    for k, n_users, with_floor in ((1, 257, True), (10, 700, True), (16, 255, False), (64, 33, True)):
        t = R.make_table(70, n_users, "aligned", "inf" if k > 1 else "ties", 3)
        s = R.select_blocks(t.table, n_users, k)
        floor = None
        if with_floor:
            floor = np.where(np.arange(n_users) % 3 == 0, s.sel_max[k // 2], np.float32(0.3)).astype(F32)   # entries EQUAL to the floor stay
            floor[1::7] = np.inf
            floor[2::7] = -np.inf
        keys = ifull((n_users * k,))
        N.call("trec_topk_group_keys", P(N, s.sel), P(N, s.sel_max), P(N, floor), n_users * k, k, 70, N.ptr(keys))
        same(keys, R.group_keys(s.sel, s.sel_max, floor, k), "group_keys k=%d floor=%s" % (k, with_floor))


@pytest.mark.parametrize("n", R.SCAN_NS)
def test_exclusive_scan_i32(N, n):
    rng = np.random.default_rng(n)
    counts = rng.integers(0, 5000, size=n).astype(I32)
    if n > 262144:
        counts[:] = 20000                                                  # the total passes 2^32: the sums are 64-bit
    out = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    ws = torch.full(((n + 1023) // 1024 + 1,), -1, dtype=torch.int64, device="cuda")
    N.call("trec_exclusive_scan_i32", P(N, counts), n, N.ptr(ws), N.ptr(out))
    same(out, R.exclusive_scan(counts), "exclusive_scan n=%d" % n)


@pytest.mark.parametrize("ci", range(len(R.FILL_CASES)))
def test_fill_groups(N, ci):
    """trec_topk_pad_counts + trec_exclusive_scan_i32 + trec_topk_fill_groups / _index on groups with empty ones at the start, in the middle
    and at the end, max_rows beyond the padded total"""
    inp = R.fill_inputs(ci)
    c = inp.case
    assert R.pick_fill(c.n_sb) == ("lds" if c.n_sb <= 2048 else "global")
    ref = R.fill_groups(inp)
    indptr, users_t, perm_t = dev(inp.indptr), dev(inp.users_t), dev(inp.perm_t)
    cnt_pad = ifull((c.n_sb + 1,))
    N.call("trec_topk_pad_counts", N.ptr(indptr), c.n_sb, c.rows_wg, N.ptr(cnt_pad))
    same(cnt_pad, inp.cnt_pad, "pad_counts")
    pstart = torch.full((c.n_sb + 2,), -1, dtype=torch.int64, device="cuda")
    ws = torch.zeros(((c.n_sb + 1 + 1023) // 1024 + 1,), dtype=torch.int64, device="cuda")
    N.call("trec_exclusive_scan_i32", N.ptr(cnt_pad), c.n_sb + 1, N.ptr(ws), N.ptr(pstart))
    same(pstart, inp.pstart, "pstart")
    R_, W = inp.max_rows, inp.max_rows // c.rows_wg
    G = torch.full((R_, c.row_bytes), 0x5A, dtype=torch.uint8, device="cuda")
    ex = c.extras
    g_bias, g_sq, g_tau = (ffull((R_,)) if ex else None for _ in range(3))
    row_pair, rb = ifull((R_,)), ifull((W,))
    N.call("trec_topk_fill_groups", N.ptr(pstart), N.ptr(indptr), N.ptr(users_t), N.ptr(perm_t), c.n_sb, c.rows_wg, R_, P(N, inp.users_op),
           c.row_bytes, P(N, inp.user_bias if ex else None), P(N, inp.user_sq if ex else None),
           P(N, inp.user_tau if ex else None), N.ptr(G), N.ptr(g_bias), N.ptr(g_sq), N.ptr(g_tau), N.ptr(row_pair), N.ptr(rb))
    same(G, ref.G, "fill_groups G")
    same(row_pair, ref.row_pair, "fill_groups row_pair")
    same(rb, ref.rblock_chunk, "fill_groups rblock_chunk")
    if ex:
        same(g_bias, ref.g_bias, "g_bias")
        same(g_sq, ref.g_sq, "g_sq")
        same(g_tau, ref.g_tau, "g_tau")
    row_user, row_pair, rb = ifull((R_,)), ifull((R_,)), ifull((W,))
    N.call("trec_topk_fill_groups_index", N.ptr(pstart), N.ptr(indptr), N.ptr(users_t), N.ptr(perm_t), c.n_sb, c.rows_wg, R_, N.ptr(row_user),
           N.ptr(row_pair), N.ptr(rb))
    same(row_user, ref.row_user, "fill_groups_index row_user")
    same(row_pair, ref.row_pair, "fill_groups_index row_pair")
    same(rb, ref.rblock_chunk, "fill_groups_index rblock_chunk")


# ------------------------------------------------------------------------------------------------------------------ 10. euclid_certify
@pytest.mark.parametrize("d", R.EUCLID_DS)
@pytest.mark.parametrize("kind", R.EUCLID_DATA)
def test_euclid_certify(N, kind, d):
    """soundness by enumeration: every user left unflagged has the whole catalogue's oracle top-k; the written lists are always the
    candidates by (score desc, id asc); holes, NaN and a negative weight flag; on "separated" the clearly certifiable users stay unflagged"""
    from oracle import oracle as O
    data = R.euclid_data(kind, d)
    nu, ni = R.EUCLID_USERS, R.EUCLID_ITEMS
    full = O.score_dense_euclid_exact(data.u, data.v, data.r_u, data.r_i, data.ub, data.ib)
    all_ids = np.tile(np.arange(ni, dtype=I32), (nu, 1))
    uu = np.arange(nu)
    hole, nan_g, nan_s = uu % 50 == 7, uu % 50 == 11, uu % 50 == 13
    for kc, k in R.EUCLID_KC_K:
        assert R.pick_certify(kc) == kc
        top_v, top_i = R.order_by_score(full, all_ids, k)
        for positive in (False, True):
            lam = R.euclid_lambda(data, positive)
            ids, g, gstats = R.euclid_candidates(data, kc, lam)
            exact = np.take_along_axis(full, ids.astype(np.int64), axis=1)
            must = R.euclid_must_certify(data, R.order_by_score(exact, ids, k)[0][:, k - 1], g[:, -1], lam) & ~(hole | nan_g | nan_s)
            ids, g, exact = ids.copy(), g.copy(), exact.copy()
            ids[hole, 3] = -1
            g[nan_g, kc - 1] = np.nan
            exact[nan_s, 0] = np.nan
            ref_v, ref_i = R.order_by_score(exact, ids, k)
            for lam_call in (lam, F32(-1.0)):
                ov, oi, flag, nfl = ffull((nu, k)), ifull((nu, k)), ifull((nu,)), ifull((1,), 0)
                N.call("trec_topk_euclid_certify", P(N, ids), P(N, g), P(N, exact), kc, k, P(N, data.r_u), P(N, data.ub), P(N, gstats),
                       P(N, np.array([data.ib.max()], F32)), d, nu, N.ptr(ov), N.ptr(oi), N.ptr(flag), N.ptr(nfl),
                       P(N, np.array([lam_call], F32)), P(N, np.array([data.ib.min()], F32)))
                what = "euclid_certify %s d=%d kc=%d k=%d lambda=%g" % (kind, d, kc, k, lam_call)
                fl = host(flag)
                same(host(ov)[~nan_s], ref_v[~nan_s], what + " values")
                same(host(oi)[~nan_s], ref_i[~nan_s], what + " ids")
                assert set(np.unique(fl)) <= {0, 1} and int(nfl.item()) == int(fl.sum()), what + " n_flagged"
                if lam_call < 0:
                    assert fl.all(), what + ": a negative weight certifies nothing"
                    continue
                assert fl[hole | nan_g | nan_s].all(), what + ": holes and NaN must flag"
                free = fl == 0
                same(host(oi)[free], top_i[free], what + " ids of the unflagged users against the whole catalogue")
                same(host(ov)[free], top_v[free], what + " values of the unflagged users against the whole catalogue")
                if kind == "separated":
                    assert not fl[must].any(), what + ": %d clearly certifiable users flagged" % int(fl[must].sum())


# ------------------------------------------------------------------------------------------------------------------ 11. exclusion lists
@pytest.mark.parametrize("kf", R.EXCLUDE_KF)
def test_exclude_filter_topk(N, kf):
    inp = R.exclude_inputs(kf)
    for k in sorted({1, kf}):
        ref = R.exclude_filter_topk(inp.vals, inp.idx, inp.ex, k)
        for rows in (None, inp.rows):
            ptr, idx = (inp.ex_ptr, inp.ex_idx) if rows is None else (inp.ex_ptr_rows, inp.ex_idx_rows)
            ov, oi, flag, nfl = ffull((inp.n_users, k)), ifull((inp.n_users, k)), ifull((inp.n_users,)), ifull((1,), 0)
            N.call("trec_exclude_filter_topk", P(N, inp.vals), P(N, inp.idx), kf, inp.n_users, k, P(N, ptr),
                   P(N, np.concatenate([idx, [0]]).astype(I32)), P(N, rows), N.ptr(ov), N.ptr(oi), N.ptr(flag), N.ptr(nfl))
            what = "exclude_filter kf=%d k=%d rows=%s" % (kf, k, rows is not None)
            same(ov, ref.vals, what + " vals")
            same(oi, ref.idx, what + " idx")
            same(flag, ref.flag, what + " flag")
            assert int(nfl.item()) == ref.n_flagged


def test_exclude_rank_adjust(N):
    inp = R.rank_adjust_inputs()
    counts = dev(inp.counts)
    N.call("trec_exclude_rank_adjust", P(N, inp.pair_ptr), P(N, inp.t_idx), P(N, inp.t_score), P(N, inp.ex_ptr),
           P(N, inp.ex_idx), P(N, inp.ex_score), inp.n_users, N.ptr(counts))
    same(counts, R.exclude_rank_adjust(inp), "rank_adjust counts")
