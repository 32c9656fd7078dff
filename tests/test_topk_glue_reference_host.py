"""tests/topk_glue_reference.py on the CPU: every reference on a hand-worked case; the case lists of tests/test_gpu_topk_glue.py reach every
instantiation and branch of the dispatch rules; the cases DISCRIMINATE (a deliberately wrong variant of each contract disagrees with the
true reference on at least one committed case, so a kernel with that defect would fail on the GPU without a faulty kernel ever running
there); the floor bracket is not too tight for the kernels' own float32 formula; the share of clearly certifiable users of the Euclidean
"separated" catalogue."""
import numpy as np
import pytest

import topk_glue_reference as R
from topk_glue_reference import F32, I32, NINF, PINF

inf = np.inf


def table(rows):
    return np.array(rows, dtype=F32)


# ------------------------------------------------------------------------------------------------------------------ hand-worked cases
def test_select_by_hand():
    #           user 0   user 1   user 2   (pad)
    t = table([[1.0,     2.0,    -inf,     9.0],
               [3.0,     2.0,    -inf,     9.0],
               [3.0,     0.0,     5.0,     9.0],
               [-inf,    2.0,    -inf,     9.0]])
    r = R.select_blocks(t, 3, 3, k_tau=2)
    assert r.sel.tolist() == [[1, 2, 0], [0, 1, 3], [2, -1, -1]]             # ties: the earlier superblock first; -inf never selected
    assert r.sel_max.tolist() == [[3.0, 2.0, 5.0], [3.0, 2.0, -inf], [1.0, 2.0, -inf]]      # [k][n_users]
    assert r.tau.tolist() == [3.0, 2.0, -inf]
    r = R.select_blocks(t, 3, 6)                                            # more slots than superblocks
    assert r.sel[0].tolist() == [1, 2, 0, -1, -1, -1] and r.tau.tolist() == [-inf] * 3


def test_collect_by_hand():
    t = table([[1.0, np.nan], [3.0, 0.0], [3.0, inf], [0.5, -inf]])
    floor = np.array([1.0, inf], dtype=F32)
    r = R.collect_blocks(t, 2, floor, 3, np.array([0, 0], I32), 4)
    assert r.keys.tolist() == [[0, 1, 2], [0, 2, -1]]                       # an entry equal to the floor, a NaN and +inf qualify
    assert r.count.tolist() == [3, 2] and r.flag.tolist() == [0, 0] and r.n_flagged == 4
    r = R.collect_blocks(t, 2, floor, 2, np.array([0, 1], I32), 4)
    assert r.keys.tolist() == [[-1, -1], [0, 2]] and r.count.tolist() == [0, 2] and r.flag.tolist() == [1, 1] and r.n_flagged == 5
    r = R.collect_blocks(t, 2, floor, 1, np.array([0, 1], I32), 4)           # user 1 was flagged before: counted once
    assert r.count.tolist() == [0, 0] and r.flag.tolist() == [1, 1] and r.n_flagged == 5
    keys_in, count_in = np.full((2, 2), 77, I32), np.full(2, 77, I32)
    r = R.collect_blocks(t, 2, floor, 2, np.array([0, 0], I32), 0, redo=np.array([0, 1], I32), keys_in=keys_in, count_in=count_in)
    assert r.keys.tolist() == [[77, 77], [0, 2]] and r.count.tolist() == [77, 2] and r.flag.tolist() == [0, 0] and r.n_flagged == 0


def test_scan_prune_by_hand():
    t = table([[1.0, 5.0], [3.0, 0.0], [3.0, 1.0], [0.5, 7.0]])
    f0 = np.array([1.0, 0.5], dtype=F32)
    s = R.scan_blocks(t, 2, 2, f0, 2)
    assert s.tau.tolist() == [3.0, 5.0] and s.sel_max.tolist() == [[3.0, 7.0], [3.0, 5.0]]
    assert s.cand_n.tolist() == [3, 3]                                      # uncapped
    assert s.cand_s.tolist() == [[0, 0], [1, 2]] and s.cand_v.tolist() == [[1.0, 5.0], [3.0, 1.0]]      # slot-major, superblock order
    p = R.prune_candidates(s.cand_s, s.cand_v, s.cand_n, 2, np.array([2.0, inf], F32), 2, np.array([0, 0], I32), 0)
    assert p.redo.tolist() == [1, 0] and p.count.tolist() == [0, 0] and p.flag.tolist() == [0, 0]       # cut list + finite floor: redo
    s = R.scan_blocks(t, 2, 2, f0, 4)
    assert s.cand_s[:, 0].tolist() == [0, 1, 2, R.SENT_I]
    p = R.prune_candidates(s.cand_s, s.cand_v, s.cand_n, 4, np.array([3.0, 1.0], F32), 2, np.array([0, 0], I32), 0)
    assert p.keys.tolist() == [[1, 2], [-1, -1]] and p.count.tolist() == [2, 0] and p.flag.tolist() == [0, 1] and p.n_flagged == 1


def test_floor_by_hand():
    st = np.array([[1.0, 2.0 ** -9]], dtype=F32)
    gs = np.array([2.0, 2.0 ** -8, 0.5], dtype=F32)
    E = R.eps_bound(st, [0.25], gs, 62)
    want = 2.0 ** -9 * 2 * (1 + 2.0 ** -8) + 2.0 ** -8 + 64 * 5 * 2.0 ** -24 * (2 * (1 + 2.0 ** -7) + 0.75)
    assert abs(E[0] - want) < 1e-15
    lo, hi = R.floor_bracket(np.array([1.0], F32), E, 2.0)
    assert hi[0] == 1.0 - 2 * want and lo[0] < hi[0] and hi[0] - lo[0] < 2 * want * 2.0 ** -9 + 13 * R.U23
    inp = R.floor_inputs(700, 64, True, 0)
    exp = R.floor_expect(inp, 2.0)
    assert exp.flag[:5].tolist() == [0, 1, 1, 1, 1] and exp.n_flagged == 4
    assert np.isneginf(exp.exact[:5]).all() and exp.bracketed[5:].all()
    src = np.arange(700, dtype=I32)
    src[[1, 9]] = -1
    exp = R.floor_expect(inp, 1.0, cascade=True, src=src)
    assert exp.flag[:5].tolist() == [0, 0, 1, 1, 1] and exp.exact[[1, 2, 9]].tolist() == [inf, inf, inf] and exp.exact[0] == NINF
    assert exp.tau_out[9] == PINF and exp.tau_out[10] == inp.tau[10]


def test_lb_tag_format():
    rng = np.random.default_rng(0)
    lb = np.concatenate([rng.standard_normal(2000) * np.exp(rng.uniform(-20, 20, 2000)), [0.0, -0.0, 1e-38, -1e-38]]).astype(F32)
    idx = rng.integers(0, 4096, len(lb))
    tg = R.lb_tag(lb, idx)
    assert np.array_equal(R.lb_tag_index(tg), idx)
    assert np.all(tg <= lb) and np.all(R.lb_key(lb) - R.lb_key(tg) <= 2 * 4096)        # at most two units of the tag below
    assert np.all(np.isneginf(R.lb_tag(np.array([-inf, inf, np.nan, 2e37], F32), 5)))
    assert R.lb_tag(F32(1.0), 3).view(np.uint32) == 0x3F800000 - 4096 + 3


def test_prerefine_by_hand():
    val = R.lb_tag(np.array([[1.0, 2.0, 0.5], [3.0, -inf, 0.25]], F32), np.array([[1, 0, 1], [0, 1, 1]]))        # [k][n_users]
    sel = np.array([[0, 16], [17, 3], [-1, 1]], dtype=I32)                                                   # rows: chunk = row // 16
    want, rc = R.prerefine_want(sel, val, 2, 16, 2, 4, np.array([0, 1, 2], I32))
    assert want.tolist() == [[1, 2], [2, -1], [-1, 1]] and rc.tolist() == [0, 2, 2, 0]
    want, rc = R.prerefine_want(sel, val, 2, 16, 2, 4, np.array([0, -1, 2], I32))
    assert want.tolist() == [[1, 2], [-1, -1], [-1, 1]] and rc.tolist() == [0, 2, 1, 0]
    sim = R.prerefine_simulate(want, 4, 512)
    assert sim.ok.tolist() == [1, 0, 0]
    R.check_prerefine(want, rc, 512, sim.sel_sb, sim.row_count, sim.row_user, sim.ok, sim.sel_pos)


def test_wg_map_by_hand():
    r = R.rows_wg_map(np.array([0, 1, 513, 5000], I32), 3, 5, guard=2)
    assert r.wg_start.tolist() == [0, 0, 1, 3, 6]
    assert r.wg_map.tolist() == [3, 6, 7, 9, 10, R.SENT_I, R.SENT_I]          # the sixth entry (11) lies at map_cap: not written


def test_grouping_by_hand():
    assert R.group_keys(np.array([[4, 2], [7, -1]], I32), np.array([[1.0, 3.0], [0.5, -inf]], F32), np.array([0.5, 3.5], F32), 2).tolist() == \
        [4, 2, -1, -1]
    assert R.group_keys(np.array([[4, 2], [7, -1]], I32), None, None, 2).tolist() == [4, 2, 7, -1]
    assert R.pad_counts([0, 0, 5, 5, 9, 11], 4, 4).tolist() == [0, 8, 0, 4, 0]
    assert R.exclusive_scan(np.array([3, 0, 2 ** 31 - 1, 2 ** 31 - 1], I32)).tolist() == [0, 3, 3, 2 ** 31 + 2, 2 ** 32 + 1]
    inp = R.fill_inputs(0)                                                  # n_sb 5, rows_wg 4: groups 1 (5 entries) and 3 (3 entries)
    assert inp.cnt_pad.tolist() == [0, 8, 0, 4, 0, 0] and inp.pstart.tolist() == [0, 0, 8, 8, 12, 12, 12] and inp.max_rows == 24
    r = R.fill_groups(inp)
    assert r.rblock_chunk.tolist() == [1, 1, 3, -1, -1, -1]
    assert (r.row_pair[:5] >= 0).all() and (r.row_pair[5:8] == -1).all() and (r.row_pair[8:11] >= 0).all() and (r.row_pair[11:] == -1).all()
    assert np.isposinf(r.g_tau[5:8]).all() and np.isposinf(r.g_tau[11:]).all() and np.isfinite(r.g_tau[:5]).all()
    assert (r.G[5:8] == 0xAB).all() and (r.row_user[5:8] == -1).all() and r.row_user[8] == inp.users_t[5]


def test_exclude_by_hand():
    vals = np.array([[5.0, 4.0, 4.0, 1.0], [5.0, 4.0, -inf, -inf]], dtype=F32)
    idx = np.array([[7, 2, 9, 3], [7, 2, -1, -1]], dtype=I32)
    r = R.exclude_filter_topk(vals, idx, [np.array([2, 3]), np.array([7, 2])], 3)
    assert r.idx.tolist() == [[7, 9, -1], [-1, -1, -1]] and r.vals[0].tolist() == [5.0, 4.0, -inf]
    assert r.flag.tolist() == [1, 0]                                        # user 1's list ran out of catalogue: exact with padding
    inp = R.SimpleNamespace(pair_ptr=np.array([0, 2]), t_idx=np.array([5, 1], I32), t_score=np.array([1.0, 2.0], F32), ex_ptr=np.array([0, 4]),
                            ex_idx=np.array([1, 4, 5, 6], I32), ex_score=np.array([2.0, 1.0, 1.0, 1.0], F32), counts=np.array([10, 10], I32),
                            n_users=1)
    assert R.exclude_rank_adjust(inp).tolist() == [8, 10]                   # ahead of (5, 1.0): item 1 (higher) and item 4 (tie, lower id)


def test_dense_by_hand():
    assert R.dense_sampled_rows(32).tolist() == list(range(32)) == R.dense_sampled_rows(33).tolist()
    assert R.dense_sampled_rows(70).tolist() == [s0 + r for s0 in (0, 16, 32, 48) for r in range(8)]
    inp = R.dense_inputs(33, 257, "odd", 16, 1)
    r = R.dense_users(inp)
    hit = (inp.n_keep >= 16) & np.isfinite(inp.cand_floor)
    assert hit.any() and (~hit).any() and np.isposinf(r.cand_floor[hit]).all() and (r.flag[hit] == 1).all()
    assert np.array_equal(r.cand_floor[~hit], inp.cand_floor[~hit]) and np.array_equal(r.flag[~hit], inp.flag_in[~hit])
    assert np.isposinf(inp.table[32, :257]).all()                            # the row outside the sample would count as kept


# ------------------------------------------------------------------------------------------------------------------ dispatch coverage
def test_cases_reach_every_instantiation():
    # select: every list length the k of the issue reach, each in both kernel forms; the rounded lengths from both ends of their range
    reached = set()
    combos = set()
    for k in R.SELECT_KS:
        taus = set()
        for c in R.select_cases(k):
            stride, off = R.layout_of(c.n_users, c.layout)
            for tiled in ((1, 0) if R.wide_loads(c.n_users, c.layout) else (1,)):
                reached.add(R.pick_select(k, c.n_sb, stride, off == 0, tiled))
            combos.add((c.layout, c.kind))
            taus.add(c.k_tau)
        assert taus == {1, k // 2 + 1, k}
        assert {c.n_users for c in R.select_cases(k)} == set(R.N_USERS) and {c.n_sb for c in R.select_cases(k)} == set(R.N_SB)
        assert any(c.nulls for c in R.select_cases(k)) and not all(c.nulls for c in R.select_cases(k))
    assert reached == {(R.select_ksel(k), f) for k in R.SELECT_KS for f in ("tiled", "lane")}
    assert {ks for ks, _ in reached} == {1, 2, 3, 5, 8, 10, 12, 16, 20, 24, 32, 40, 48, 64}
    assert [R.select_ksel(k) for k in (17, 20, 21, 24, 25, 32, 33, 40, 41, 48, 49, 64)] == [20, 20, 24, 24, 32, 32, 40, 40, 48, 48, 64, 64]
    assert combos == {(lay, kind) for lay in R.LAYOUTS for kind in R.KINDS}
    assert R.pick_select(10, 31, 256, True) == (10, "lane") and R.pick_select(10, 32, 256, True) == (10, "tiled")
    assert R.pick_select(10, 70, 258, True)[1] == "lane" and R.pick_select(10, 70, 256, False)[1] == "lane"
    # collect: every layout and value kind per ksel
    for ksel in R.COLLECT_KSEL:
        cs = R.shapes(4 * R.COLLECT_KSEL.index(ksel) + 1, R.COLLECT_KINDS)
        assert {c.layout for c in cs} == set(R.LAYOUTS) and {c.kind for c in cs} == set(R.COLLECT_KINDS)
    # scan: KS 4 / 8 / 10 / 12 / 16 from both ends; every cap with every ksel
    assert [R.pick_scan(k) for k in R.SCAN_KS] == [4, 4, 8, 8, 10, 10, 12, 12, 16, 16]
    pairs = {(R.SCAN_CAPS[(c.index + s) % 3], R.COLLECT_KSEL[(c.index // 3 + s) % 3]) for s in range(len(R.SCAN_KS)) for c in R.shapes(s)}
    assert pairs == {(a, b) for a in R.SCAN_CAPS for b in R.COLLECT_KSEL}
    # certify, pre-refinement, fill_groups
    assert {R.pick_certify(kc) for kc, _ in R.EUCLID_KC_K} == {16, 32, 64}
    assert {R.pick_prerefine(c.k)[0] for c in R.PREREFINE_CASES} == {16, 64}
    assert all(c.n_users > R.pick_prerefine(c.k)[1] for c in R.PREREFINE_CASES)          # more than one workgroup
    assert {c.k for c in R.PREREFINE_CASES} == {1, 10, 16, 17, 40, 64} and {c.n_sb for c in R.PREREFINE_CASES} == {3, 300}
    assert {R.pick_fill(c.n_sb) for c in R.FILL_CASES} == {"lds", "global"} and {c.n_sb for c in R.FILL_CASES} == {5, 2048, 2049}
    assert {(c.rows_wg, c.row_bytes) for c in R.FILL_CASES} == {(4, 16), (4, 512), (256, 16), (256, 512)}
    assert {c.extras for c in R.FILL_CASES if c.n_sb > 2048} == {True, False} == {c.extras for c in R.FILL_CASES if c.n_sb <= 2048}


def test_table_kinds_hold_what_they_promise():
    for kind in R.COLLECT_KINDS:
        t = R.make_table(70, 257, "offset", kind, 2)
        col = t.table[:, :257]
        assert t.offset == 1 and t.stride == 260 and np.isnan(t.table[:, 257:]).all()
        if kind == "ties":
            assert set(np.unique(col)) == {0.0, 1.0, 2.0, 3.0}
        if kind == "short":
            assert np.isfinite(col).sum(axis=0).max() == 3 and np.isfinite(col).sum(axis=0).min() == 0
        if kind in ("inf", "nan"):
            assert np.isposinf(col).any() and np.isneginf(col).any()
        assert np.isnan(col).any() == (kind == "nan")
    assert R.make_table(7, 255, "odd", "cont", 0).stride == 256 and R.make_table(7, 257, "odd", "cont", 0).stride == 258


# ------------------------------------------------------------------------------------------------------------------ discrimination
def differs(a, b, names):
    return any(not np.array_equal(np.asarray(getattr(a, n)), np.asarray(getattr(b, n))) for n in names)


def test_select_cases_discriminate():
    hit = {"tie_reversed": 0, "neg_inf_selected": 0}
    for k in R.SELECT_KS:
        for c in R.select_cases(k):
            t = R.make_table(c.n_sb, c.n_users, c.layout, c.kind, c.seed)
            ref = R.select_blocks(t.table, c.n_users, k, c.k_tau)
            for bug in hit:
                hit[bug] += differs(ref, R.select_blocks(t.table, c.n_users, k, c.k_tau, bug=bug), ("sel",))
        assert all(hit.values()), (k, hit)                                   # ... for every k
        hit = dict.fromkeys(hit, 0)


def test_collect_cases_discriminate():
    for ksel in R.COLLECT_KSEL:
        hit = {"over_not_emptied": 0, "count_reflagged": 0}
        marked_wg = False
        for c in R.shapes(4 * R.COLLECT_KSEL.index(ksel) + 1, R.COLLECT_KINDS):
            t = R.make_table(c.n_sb, c.n_users, c.layout, c.kind, c.seed)
            inp = R.collect_inputs(t.table, c.n_users, ksel, c.index)
            ref = R.collect_blocks(t.table, c.n_users, inp.floor, ksel, inp.flag_in, inp.n_flagged_in)
            for bug in hit:
                hit[bug] += differs(ref, R.collect_blocks(t.table, c.n_users, inp.floor, ksel, inp.flag_in, inp.n_flagged_in, bug=bug),
                                    ("keys", "count", "n_flagged"))
            marked_wg |= c.n_users == 700 and not inp.redo[256:512].any() and inp.redo[:256].any() and inp.redo[512:].any()
        assert all(hit.values()) and marked_wg, (ksel, hit)


def test_scan_cases_discriminate():
    """a slot-major list read user-major"""
    for s, k in enumerate(R.SCAN_KS):
        hit = 0
        for c in R.shapes(s, R.COLLECT_KINDS):
            cap = R.SCAN_CAPS[(c.index + s) % 3]
            t = R.make_table(c.n_sb, c.n_users, c.layout, c.kind, c.seed)
            f0 = np.full(c.n_users, -1.0, dtype=F32)
            hit += differs(R.scan_blocks(t.table, c.n_users, k, f0, cap), R.scan_blocks(t.table, c.n_users, k, f0, cap, bug="user_major"),
                           ("cand_s", "cand_v"))
        assert hit, k


def test_floor_bracket_holds_the_float32_formula_and_rejects_one_float_above():
    worst = 0.0
    for mult in R.FLOOR_MULTS:
        for kdim in R.FLOOR_KDIMS:
            for with_bias in (False, True):
                for n_users in (1, 257, 700):
                    inp = R.floor_inputs(n_users, kdim, with_bias, seed=int(mult))
                    exp = R.floor_expect(inp, mult)
                    bu = np.abs(inp.bias) if with_bias else np.zeros(n_users, F32)
                    f = R.floor_f32(inp.tau, inp.ustats, bu, inp.gstats, kdim, mult)
                    f[~exp.bracketed] = exp.exact[~exp.bracketed]
                    worst = max(worst, R.check_floor(f, exp))
                    g = R.floor_f32(inp.tau, inp.ustats, bu, inp.gstats, kdim, mult, bug="one_above")
                    g[~exp.bracketed] = exp.exact[~exp.bracketed]
                    with pytest.raises(AssertionError, match="unsound"):
                        R.check_floor(g, exp)
    assert 0.3 < worst < 1.0, worst                                          # the formula uses the bracket, and stays inside


def test_tau_listed_inputs_are_decided_and_cover_the_classes():
    for k in R.TAU_LISTED_KS:
        inp = R.tau_listed_inputs(k)
        exp = R.tau_listed_expect(inp)                                       # (asserts that every user's outcome is decided)
        assert exp.rises.any() and (~exp.rises).any()
        for cl in range(7):
            assert not exp.rises[inp.cls == cl].any() or cl in (4, 5), cl     # classes 0, 1, 2, 3, 6 keep tau
        assert exp.rises[inp.cls == 7].all() and exp.rises[inp.cls == 4].all()
        assert np.isnan(exp.vals).any() and np.isposinf(exp.vals).any()
        # the float32 formula passes the check, and a result that ignores `ok` does not
        bu = np.abs(inp.bias)
        m = np.min(np.where(np.isnan(exp.vals), NINF, exp.vals), axis=1)
        t = np.where(exp.rises, R.floor_f32(m, inp.ustats, bu, inp.gstats, inp.kdim, 1.0), inp.tau).astype(F32)
        cf = np.where(exp.rises & np.isfinite(inp.cand_floor),
                      np.maximum(inp.cand_floor, R.floor_f32(t, inp.ustats, bu, inp.gstats, inp.kdim, 1.0)), inp.cand_floor).astype(F32)
        assert 0.0 < R.check_tau_listed(inp, exp, t, exp.vals, cf) < 1.0
        wrong = t.copy()
        u = np.nonzero(inp.cls == 2)[0][0]
        wrong[u] = F32(0.0)
        with pytest.raises(AssertionError):
            R.check_tau_listed(inp, exp, wrong, exp.vals, cf)


def test_prerefine_cases_discriminate():
    for ci, c in enumerate(R.PREREFINE_CASES):
        inp = R.prerefine_inputs(ci)
        want, rc = R.prerefine_want(inp.sel, inp.val, c.k, c.top_k, c.sb_per_chunk, c.n_sb, inp.src)
        assert (inp.src < 0).any() and (want[inp.src < 0] == -1).all()
        assert (inp.sel < 0).any() or c.k == 1
        if c.hot:
            assert rc[0] > c.rcap
        sim = R.prerefine_simulate(want, c.n_sb, c.rcap)
        R.check_prerefine(want, rc, c.rcap, sim.sel_sb, sim.row_count, sim.row_user, sim.ok, sim.sel_pos)
        assert sim.ok.any() or c.k > c.n_sb
        assert not sim.ok.all()
        if rc.max() > c.rcap:
            bad = R.prerefine_simulate(want, c.n_sb, c.rcap, bug="dup")
            with pytest.raises(AssertionError):
                R.check_prerefine(want, rc, c.rcap, bad.sel_sb, bad.row_count, bad.row_user, bad.ok, bad.sel_pos)
        wrong_ok = sim.ok.copy()
        wrong_ok[:] = 1
        with pytest.raises(AssertionError, match="ok"):
            R.check_prerefine(want, rc, c.rcap, sim.sel_sb, sim.row_count, sim.row_user, wrong_ok, sim.sel_pos)


def test_wg_map_cases_discriminate():
    for n_sb in R.WG_MAP_N_SB:
        seen = set()
        for wpr in (1, 3):
            rc = R.wg_map_inputs(n_sb, wpr)
            seen |= set(rc.tolist())
            total = int(R.rows_wg_map(rc, wpr, 1 << 20, guard=0).wg_start[-1])
            if total > 2:
                assert differs(R.rows_wg_map(rc, wpr, total - 2), R.rows_wg_map(rc, wpr, total - 2, bug="no_cap"), ("wg_map",))
        if n_sb >= 255:
            assert {0, 1, 512, 513} <= seen and max(seen) > 3 * 512


def test_dense_cases_discriminate():
    for n_sb in R.DENSE_N_SB:
        for n_users, layout, limit in ((255, "aligned", 16), (257, "odd", 32), (701, "offset", 20)):
            inp = R.dense_inputs(n_sb, n_users, layout, limit, seed=n_users)
            assert n_users % 4 and differs(R.dense_users(inp), R.dense_users(inp, bug="limit_off_by_one"), ("cand_floor", "flag", "n_flagged"))
            hit = inp.n_keep >= limit
            assert (hit & np.isposinf(inp.cand_floor)).any() and (hit & (inp.flag_in == 1) & np.isfinite(inp.cand_floor)).any()


def test_fill_cases_discriminate():
    for ci, c in enumerate(R.FILL_CASES):
        inp = R.fill_inputs(ci)
        cnt = np.diff(inp.indptr)[:c.n_sb]
        assert cnt[0] == 0 and cnt[-1] == 0 and (cnt[1:-1] == 0).any() and (cnt > 0).sum() >= 2     # empty groups at the start, inside, at the end
        assert inp.max_rows > inp.pstart[c.n_sb] and inp.max_rows % c.rows_wg == 0
        ref = R.fill_groups(inp)
        assert differs(ref, R.fill_groups(inp, bug="finite_pad_tau"), ("g_tau",))
        assert differs(ref, R.fill_groups(inp, bug="chunk_beyond_total"), ("rblock_chunk",))
        assert (ref.row_pair[:inp.pstart[c.n_sb]] == -1).any()                # padding rows inside the padded total too


def test_exclude_cases_discriminate():
    for kf in R.EXCLUDE_KF:
        inp = R.exclude_inputs(kf)
        assert (inp.idx[:, -1] < 0).any() and (inp.idx[:, -1] >= 0).any()
        assert any(len(e) == 0 for e in inp.ex)
        hit = 0
        for k in sorted({1, kf}):
            ref = R.exclude_filter_topk(inp.vals, inp.idx, inp.ex, k)
            hit += differs(ref, R.exclude_filter_topk(inp.vals, inp.idx, inp.ex, k, bug="flag_short_lists"), ("flag",))
            assert ref.flag.any() and not ref.flag.all()
            assert (ref.idx[:, 0] < 0).any()                                 # a fully excluded list
        assert hit, kf
    inp = R.rank_adjust_inputs()
    assert not np.array_equal(R.exclude_rank_adjust(inp), R.exclude_rank_adjust(inp, bug="tie_reversed"))
    assert (np.diff(inp.pair_ptr) == 0).any() and (np.diff(inp.ex_ptr) == 0).any()


# ------------------------------------------------------------------------------------------------------------------ euclid
@pytest.mark.parametrize("d", R.EUCLID_DS)
def test_euclid_separated_is_mostly_certifiable(d):
    """the users the GPU test forbids to flag are at least 80 % of the "separated" catalogue, in every case: the test cannot pass by
    flagging everybody; and for none of them does the candidates' top-k differ from the whole catalogue's (the condition is sound)"""
    from oracle import oracle as O
    data = R.euclid_data("separated", d)
    full = O.score_dense_euclid_exact(data.u, data.v, data.r_u, data.r_i, data.ub, data.ib)
    all_ids = np.tile(np.arange(R.EUCLID_ITEMS, dtype=I32), (R.EUCLID_USERS, 1))
    for kc, k in R.EUCLID_KC_K:
        top_i = R.order_by_score(full, all_ids, k)[1]
        for positive in (False, True):
            lam = R.euclid_lambda(data, positive)
            assert (lam > 0) == positive
            ids, g, gstats = R.euclid_candidates(data, kc, lam)
            assert np.all(np.diff(g, axis=1) <= 0)
            exact = np.take_along_axis(full, ids.astype(np.int64), axis=1)
            ov, oi = R.order_by_score(exact, ids, k)
            must = R.euclid_must_certify(data, ov[:, k - 1], g[:, -1], lam)
            assert must.mean() >= 0.8, (d, kc, k, float(lam), must.mean())
            assert np.array_equal(oi[must], top_i[must])


def test_order_by_score_by_hand():
    ov, oi = R.order_by_score(np.array([[1.0, 2.0, 2.0, 9.0]], F32), np.array([[5, 8, 3, -1]], I32), 4)
    assert oi.tolist() == [[3, 8, 5, -1]] and ov.tolist() == [[2.0, 2.0, 1.0, -inf]]
