"""The six exact top-k "finish" entry points of csrc/topk_filter.hip, called directly on hand-built lists:

    trec_topk_candidates_finish (a wave per user, and 16 lanes per user), trec_topk_candidates_finish_mixed,
    trec_topk_candidates_finish_wide, trec_topk_filter_finish, trec_topk_filter_finish_wide.

Everything else reaches these kernels through a whole cascade at 300k items; here the lists, counts and floors are made by hand,
so the list-length boundaries, the flagging rules and the element-wise row path (a leading dimension that is no multiple of 4,
which the Python host never produces: its operands are kpad wide) are met in isolation.

Bar: values AND ids bit-identical to the oracle: O.score_dense_exact on the UNPADDED operands (the k-ordered fmaf chain, then
(s + b_u) + b_i) restricted to the items the kernel has to re-score, in the (value desc, id asc) order of O.topk_rows; empty
places are -inf / -1; rows nobody writes keep the sentinel the buffers were filled with; flag / n_flagged as the kernels'
comments state.

Input rule: every listed id lies in [item_index_base, item_index_base + n_items) (or is -1 in the filter's id lists, where -1
marks an empty place), and every count is consistent with its buffer: the kernels trust their lists."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS, BASE = 37, 300, 1000          # 37: neither the 4- nor the 16-users-per-workgroup grid ends on a full group
SENT_V, SENT_I = np.float32(12345.0), np.int32(-777)
DUP = (10, 11, 12)                              # three identical item rows (and biases): equal scores, id ascending
DUP_USER = 6                                    # ... whose row is parallel to theirs: they lead its list
# (kdim, ld_users, ld_items): full rows; the vector path with a scalar tail and NaN pads; the element-wise path
DIMS = [(128, 128, 128), (6, 8, 8), (5, 5, 9)]
CMAX = 64                                       # FILTER_CMAX: survivors a staged finish can re-score
SPEC = 24                                       # FILTER_SPEC: slots whose lists filter_finish_kernel fetches ahead of the count


@pytest.fixture(scope="module")
def N():
    from tensorrec_amd import _native
    _native.require_gpu()
    _native.load()
    return _native


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Problem:
    """Operands with NaN in every pad column, and the oracle's scores of the unpadded ones (computed once per shape)."""

    def __init__(self, dims):
        self.kdim, self.ld_u, self.ld_v = dims
        rng = np.random.default_rng(1000 + self.kdim)
        u = rng.standard_normal((N_USERS, self.kdim)).astype(np.float32)
        v = rng.standard_normal((N_ITEMS, self.kdim)).astype(np.float32)
        self.ub = (0.2 * rng.standard_normal(N_USERS)).astype(np.float32)
        self.ib = (0.2 * rng.standard_normal(N_ITEMS)).astype(np.float32)
        v[DUP[1]] = v[DUP[2]] = v[DUP[0]]
        self.ib[DUP[1]] = self.ib[DUP[2]] = self.ib[DUP[0]]
        u[DUP_USER] = 3.0 * v[DUP[0]]
        self.u_pad = np.full((N_USERS, self.ld_u), np.nan, np.float32)
        self.v_pad = np.full((N_ITEMS, self.ld_v), np.nan, np.float32)
        self.u_pad[:, :self.kdim] = u
        self.v_pad[:, :self.kdim] = v
        self.scores = {True: O.score_dense_exact(u, v, self.ub, self.ib), False: O.score_dense_exact(u, v, None, None)}
        for s in self.scores.values():
            s.setflags(write=False)


@functools.lru_cache(maxsize=None)
def problem(dims):
    return Problem(dims)


def expected_rows(scores, survivors, k):
    """Per user the k best of ``survivors[u]`` (local item ids) by the oracle's order; -inf / -1 past the end."""
    masked = np.full(scores.shape, -np.inf, np.float32)
    cnt = np.zeros(len(survivors), np.int64)
    for u, s in enumerate(survivors):
        s = np.unique(np.asarray(s, np.int64))
        masked[u, s] = scores[u, s]
        cnt[u] = len(s)
    ev, ei = O.topk_rows(masked, k)
    empty = np.arange(k)[None, :] >= cnt[:, None]
    return np.where(empty, np.float32(-np.inf), ev).astype(np.float32), np.where(empty, -1, ei + BASE).astype(np.int32)


def check_rows(got_v, got_i, exp_v, exp_i, rows, what):
    for r in rows:
        assert np.array_equal(got_i[r], exp_i[r]) and np.array_equal(got_v[r].view(np.int32), exp_v[r].view(np.int32)), \
            (what, "row", int(r), got_i[r], exp_i[r], got_v[r], exp_v[r])


def out_index_with_holes(rng):
    oi = rng.permutation(N_USERS).astype(np.int32)
    oi[[11, 20]] = -1                            # these users write nothing; the rows they would have had keep the sentinel
    return oi


# ------------------------------------------------------------------------------------------------------------------------------
# the candidate lists: trec_topk_candidates_finish / _mixed
# ------------------------------------------------------------------------------------------------------------------------------
class CandCase:
    """cand_n, the {id, score} lists, the floors and stats of one call, and what the wave-per-user form has to answer.

    regime "tight": all stats zero, so eps = 1e-30 (+ a term of |b_u| * 3e-7 * (kdim + 2) with biases: the builder asserts that
    no listed score lies that close under the floor) and the floor is two floats below the k-th largest LISTED score.
    regime "all": large finite stats, every listed entry survives.
    listed "exact": the listed score is the exact one; "perturbed": the order by listed score differs from the exact order."""

    def __init__(self, P, bias, cap, k, regime, listed, lane_cands=16, seed=0):
        rng = np.random.default_rng(seed)
        sc = P.scores[bias]
        self.cap, self.k = cap, k
        n = rng.integers(k, min(cap, 40) + 1, size=N_USERS)
        n[0] = cap                                                  # a full list: answered
        n[1] = cap + 1                                              # an incomplete list: flagged, -inf / -1
        tied = regime == "tight" and listed == "perturbed"         # 64 / 65 survivors out of a longer list, by ties at the top
        n[2] = min(cap, 100) if tied else 64                        # 64 survivors: not flagged
        n[3] = min(cap, 100) if tied else min(65, cap)              # 65 survivors (cap >= 128): flagged
        n[4] = k - 1                                                # fewer than k entries: the tail of the row is empty
        n[7], n[8] = lane_cands, lane_cands + 1                     # the 16-lane form's own boundary
        n[9] = 0
        self.floor0 = rng.standard_normal(N_USERS).astype(np.float32)
        self.floor0[5] = np.inf                                     # skipped, not flagged
        self.n = n.astype(np.int32)
        self.ids = np.zeros((N_USERS, cap), np.int64)
        self.sh = np.full((N_USERS, cap), 1e30, np.float32)        # past the count: a valid id with a huge score -- must be masked
        for u in range(N_USERS):
            m = min(int(n[u]), cap)
            ids = rng.permutation(N_ITEMS)[:cap]
            if u == DUP_USER:
                ids = np.concatenate([np.array(DUP[::-1]), ids[~np.isin(ids, DUP)]])[:cap]
            self.ids[u] = ids
            s = sc[u, ids[:m]].copy()
            if listed == "perturbed" and u != DUP_USER:
                s += (0.5 * rng.standard_normal(m)).astype(np.float32)
            if tied and u in (2, 3):
                s[:64 if u == 2 else min(65, m)] = 100.0
            self.sh[u, :m] = s
        if regime == "tight":
            self.ustats, self.gstats = np.zeros((N_USERS, 2), np.float32), np.zeros(3, np.float32)
        else:
            self.ustats, self.gstats = np.full((N_USERS, 2), 1e3, np.float32), np.full(3, 1e3, np.float32)
        self.out_index = out_index_with_holes(rng)
        # ---- the wave-per-user answer
        self.skip = ~(self.floor0 < np.inf) | (self.out_index < 0)
        self.over = self.n > cap
        survivors, self.n_surv = [], np.zeros(N_USERS, np.int64)
        for u in range(N_USERS):
            m = 0 if (self.skip[u] or self.over[u]) else int(n[u])
            s = self.sh[u, :m]
            keep = np.ones(m, bool)
            if regime == "tight" and m >= k:
                tau = np.sort(s)[::-1][k - 1]
                fl = np.nextafter(np.nextafter(tau, np.float32(-np.inf)), np.float32(-np.inf))
                keep = s >= fl
                if bias:                                            # (input validity: eps's bias term cannot change the set)
                    assert not np.any((s < fl) & (s >= tau - np.float32(1e-4))), ("a listed score in the floor's band", u)
            survivors.append(self.ids[u, :m][keep])
            self.n_surv[u] = keep.sum()
        self.survivors = survivors
        self.exp_v, self.exp_i = expected_rows(sc, survivors, k)
        if regime == "all" or tied:                                # the roles are what they claim to be
            assert self.n_surv[2] == 64 and (cap < 128 or self.n_surv[3] == 65)

    def cand(self):
        c = np.empty((N_USERS, self.cap, 2), np.int32)
        c[:, :, 0] = self.ids + BASE
        c[:, :, 1] = self.sh.view(np.int32)
        return c

    def expect(self, lane_limit=None):
        """(values, ids, rows to compare, flags): lane_limit = the 16-lane form's list length, beyond which it flags."""
        flag = np.zeros(N_USERS, np.int32)
        ev = np.full((N_USERS, self.k), SENT_V, np.float32)
        ei = np.full((N_USERS, self.k), SENT_I, np.int32)
        rows = []
        for u in range(N_USERS):
            uo = int(self.out_index[u])
            if uo < 0:
                continue
            too_long = self.over[u] or (lane_limit is not None and self.n[u] > lane_limit)
            if self.skip[u] or too_long:
                flag[u] = 0 if self.skip[u] else 1
                ev[uo], ei[uo] = -np.inf, -1
            elif self.n_surv[u] > CMAX:
                flag[u] = 1                                         # (the row is the caller's to re-do: not compared)
                continue
            else:
                ev[uo], ei[uo] = self.exp_v[u], self.exp_i[u]
            rows.append(uo)
        rows += [r for r in range(N_USERS) if r not in set(self.out_index.tolist())]      # sentinel rows
        return ev, ei, rows, flag


def run_candidates(N, P, bias, case, entry, **kw):
    ov = dev(np.full((N_USERS, case.k), SENT_V, np.float32))
    oi = dev(np.full((N_USERS, case.k), SENT_I, np.int32))
    flag = torch.zeros(N_USERS, dtype=torch.int32, device="cuda")
    n_flagged = torch.zeros(1, dtype=torch.int32, device="cuda")
    ub, ib = (dev(P.ub), dev(P.ib)) if bias else (None, None)
    keep = [dev(case.n), dev(case.cand()), dev(case.floor0), dev(case.ustats), dev(case.gstats), dev(P.u_pad), dev(P.v_pad),
            dev(case.out_index)]
    head = (N.ptr(keep[0]), N.ptr(keep[1]), case.cap, N.ptr(keep[2]), N.ptr(keep[3]), N.ptr(keep[4]), N.ptr(keep[5]),
            N.ptr(keep[6]), P.ld_u, P.ld_v, P.kdim, N.ptr(ub), N.ptr(ib), BASE, N_USERS, case.k, N.ptr(ov), N.ptr(oi),
            N.ptr(flag), N.ptr(n_flagged), N.ptr(keep[7]))
    over_count = None
    if entry == "mixed":
        over_list = torch.full((N_USERS,), -1, dtype=torch.int32, device="cuda")
        over_count = torch.zeros(1, dtype=torch.int32, device="cuda")
        N.call("trec_topk_candidates_finish_mixed", *head, kw["cands_per_lane"], N.ptr(over_list), N.ptr(over_count))
    else:
        N.call("trec_topk_candidates_finish", *head, kw["lanes_per_user"])
    torch.cuda.synchronize()
    return (ov.cpu().numpy(), oi.cpu().numpy(), flag.cpu().numpy(), int(n_flagged.item()),
            None if over_count is None else int(over_count.item()))


@pytest.mark.parametrize("listed", ["exact", "perturbed"])
@pytest.mark.parametrize("regime", ["tight", "all"])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "k%d_ldu%d_ldv%d" % d)
def test_candidates_finish(N, dims, bias, regime, listed):
    """Wave per user (lanes_per_user = 0) and 16 lanes per user, cand_cap 64 .. 256, k 1 / 10 / 16, every per-user condition of
    CandCase in one batch."""
    P = problem(dims)
    for cap, k in [(64, 10), (128, 1), (192, 16), (256, 10)]:
        case = CandCase(P, bias, cap, k, regime, listed, seed=cap + k)
        for lanes, limit in [(0, None), (16, 16)]:
            gv, gi, gflag, gn, _ = run_candidates(N, P, bias, case, "plain", lanes_per_user=lanes)
            ev, ei, rows, flag = case.expect(limit)
            what = (dims, bias, regime, listed, cap, k, lanes)
            assert np.array_equal(gflag, flag), (what, gflag, flag)
            assert gn == int(flag.sum()), what
            check_rows(gv, gi, ev, ei, rows, what)


@pytest.mark.parametrize("cands_per_lane", [1, 2, 4])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "k%d_ldu%d_ldv%d" % d)
def test_candidates_finish_mixed(N, dims, bias, cands_per_lane):
    """Lists of 16 c and 16 c + 1 entries: the longer one is handed to the listed kernel and answered, not flagged; everything
    equals the wave-per-user entry point on the same inputs; over_count = the users handed on."""
    P = problem(dims)
    lc = 16 * cands_per_lane
    for cap, k, regime in [(64, 10, "all"), (128, 16, "tight"), (256, 1, "all")]:
        case = CandCase(P, bias, cap, k, regime, "exact", lane_cands=lc, seed=7 * cap + cands_per_lane)
        assert case.n[7] == lc and case.n[8] == lc + 1
        wv, wi, wflag, wn, _ = run_candidates(N, P, bias, case, "plain", lanes_per_user=0)
        gv, gi, gflag, gn, over = run_candidates(N, P, bias, case, "mixed", cands_per_lane=cands_per_lane)
        ev, ei, rows, flag = case.expect(None)
        what = (dims, bias, cands_per_lane, cap, k, regime)
        assert np.array_equal(gflag, flag) and np.array_equal(wflag, flag) and gn == wn == int(flag.sum()), (what, gflag, flag)
        check_rows(gv, gi, ev, ei, rows, what)
        check_rows(gv, gi, wv, wi, rows, what)
        if lc + 1 <= min(cap, CMAX):
            assert flag[8] == 0 and case.out_index[8] >= 0          # 16 c + 1 entries: answered
        assert over == int(np.sum(~case.skip & ((case.n > lc) | case.over))), what


# ------------------------------------------------------------------------------------------------------------------------------
# trec_topk_candidates_finish_wide: no floor, no survivor limit -- the k best of the whole list
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap,k", [(256, 17), (512, 64), (1024, 17), (1024, 64)])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "k%d_ldu%d_ldv%d" % d)
def test_candidates_finish_wide(N, dims, bias, cap, k):
    """Lists of up to 1,024 entries, k 17 / 64: a full list is answered; n > cap and n < k flag; a user flagged on entry or with
    a +inf floor is skipped (-inf / -1, flag untouched); out_index with holes."""
    P = problem(dims)
    rng = np.random.default_rng(cap + k)
    sc = P.scores[bias]
    n = rng.integers(k, min(cap, N_ITEMS) + 1, size=N_USERS)
    n[0] = cap                                                      # a full list: answered (beyond 300 entries items repeat: equal
    n[1] = cap + 1                                                  #   keys leave together, the answer is over the distinct ids)
    n[2] = k - 1                                                    # fewer than k: flagged
    n[3] = k
    floor0 = rng.standard_normal(N_USERS).astype(np.float32)
    floor0[5] = np.inf
    flag_in = np.zeros(N_USERS, np.int32)
    flag_in[4] = 1                                                  # flagged on entry: skipped
    out_index = out_index_with_holes(rng)
    cand = np.empty((N_USERS, cap, 2), np.int32)
    survivors = []
    for u in range(N_USERS):
        ids = np.tile(rng.permutation(N_ITEMS), (cap + N_ITEMS - 1) // N_ITEMS)[:cap]
        if u == DUP_USER:
            ids[:3] = DUP[::-1]
        cand[u, :, 0] = ids + BASE
        cand[u, :, 1] = rng.standard_normal(cap).astype(np.float32).view(np.int32)      # the listed score is not read
        survivors.append(ids[:min(int(n[u]), cap)])
    exp_v, exp_i = expected_rows(sc, survivors, k)
    ev = np.full((N_USERS, k), SENT_V, np.float32)
    ei = np.full((N_USERS, k), SENT_I, np.int32)
    flag = flag_in.copy()
    for u in range(N_USERS):
        uo = int(out_index[u])
        if uo < 0:
            continue
        skip = not floor0[u] < np.inf or flag_in[u] != 0
        bad = n[u] > cap or n[u] < k
        if skip or bad:
            flag[u] = flag_in[u] if skip else 1
            ev[uo], ei[uo] = -np.inf, -1
        else:
            ev[uo], ei[uo] = exp_v[u], exp_i[u]
    ov = dev(np.full((N_USERS, k), SENT_V, np.float32))
    oi = dev(np.full((N_USERS, k), SENT_I, np.int32))
    dflag, n_flagged = dev(flag_in), torch.zeros(1, dtype=torch.int32, device="cuda")
    ub, ib = (dev(P.ub), dev(P.ib)) if bias else (None, None)
    keep = [dev(n.astype(np.int32)), dev(cand), dev(floor0), dev(P.u_pad), dev(P.v_pad), dev(out_index)]
    N.call("trec_topk_candidates_finish_wide", N.ptr(keep[0]), N.ptr(keep[1]), cap, N.ptr(keep[2]), N.ptr(keep[3]), N.ptr(keep[4]),
           P.ld_u, P.ld_v, P.kdim, N.ptr(ub), N.ptr(ib), BASE, N_USERS, k, N.ptr(ov), N.ptr(oi), N.ptr(dflag), N.ptr(n_flagged),
           N.ptr(keep[5]))
    torch.cuda.synchronize()
    what = (dims, bias, cap, k)
    assert np.array_equal(dflag.cpu().numpy(), flag), (what, dflag.cpu().numpy(), flag)
    assert int(n_flagged.item()) == int((flag - flag_in).sum()), what
    assert flag[0] == 0 and flag[1] == 1 and flag[2] == 1 and flag[3] == 0
    check_rows(ov.cpu().numpy(), oi.cpu().numpy(), ev, ei, range(N_USERS), what)


# ------------------------------------------------------------------------------------------------------------------------------
# the filter's id lists: trec_topk_filter_finish / _wide.  part_idx [n_users][ksel][2][capacity], -1 = empty; only the first
# count[u] slots of a user are lists of this call -- the others hold valid ids that must not be read as survivors
# ------------------------------------------------------------------------------------------------------------------------------
def fill_lists(rng, ksel, cap, count, total, full_list=False, items=None):
    """One user's [ksel][2][cap] id lists: ``total`` distinct items spread over the kept slots from the front of every list
    (never its last place, unless full_list: then list (0, 1) is filled to the end), other ids in the slots past the count."""
    perm = rng.permutation(N_ITEMS) if items is None else items
    pi = np.full((ksel, 2, cap), -1, np.int64)
    kept = min(count, ksel)
    places = [(s, h, p) for p in range(cap - 1) for s in range(kept) for h in range(2)]
    if full_list:
        places = [(0, 1, p) for p in range(cap)] + [x for x in places if x[:2] != (0, 1)]
        total = max(total, cap)
    assert total <= len(places)
    for j, (s, h, p) in enumerate(places[:total]):
        pi[s, h, p] = perm[j]
    for s in range(kept, ksel):
        pi[s, :, :cap // 2] = perm[-cap:][:cap // 2]
    return pi, perm[:total]


def run_filter(N, entry, P, bias, pi, ksel, cap, count, k, flag_in):
    ov = dev(np.full((N_USERS, k), SENT_V, np.float32))
    oi = dev(np.full((N_USERS, k), SENT_I, np.int32))
    dflag, n_flagged = dev(flag_in), torch.zeros(1, dtype=torch.int32, device="cuda")
    ub, ib = (dev(P.ub), dev(P.ib)) if bias else (None, None)
    keep = [dev((np.where(pi >= 0, pi + BASE, -1)).astype(np.int32)), dev(count.astype(np.int32)), dev(P.u_pad), dev(P.v_pad)]
    N.call(entry, N.ptr(keep[0]), cap, ksel, N.ptr(keep[1]), N.ptr(keep[2]), N.ptr(keep[3]), P.ld_u, P.ld_v, P.kdim, N.ptr(ub),
           N.ptr(ib), BASE, N_USERS, k, N.ptr(ov), N.ptr(oi), N.ptr(dflag), N.ptr(n_flagged))
    torch.cuda.synchronize()
    return ov.cpu().numpy(), oi.cpu().numpy(), dflag.cpu().numpy(), int(n_flagged.item())


# (ksel, capacity, k): ceil(ksel * 2 * capacity / 64) = 4, 8, 12, 15 -> 16, 30 -> 32 list entries per lane
@pytest.mark.parametrize("ksel,cap,k", [(12, 10, 10), (32, 8, 1), (40, 9, 16), (60, 8, 33), (60, 16, 64)])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "k%d_ldu%d_ldv%d" % d)
def test_filter_finish(N, dims, bias, ksel, cap, k):
    """Every CPL instantiation; count[u] below / at / above FILTER_SPEC; a list filled to its last place flags; 64 survivors are
    answered, 65 flag; ids in the slots past the count are not survivors."""
    P = problem(dims)
    rng = np.random.default_rng(ksel * cap + k)
    sc = P.scores[bias]
    count = rng.integers(1, ksel + 1, size=N_USERS)
    total = np.array([rng.integers(0, min(40, c * 2 * (cap - 1)) + 1) for c in count])
    count[0], count[1], count[2] = min(ksel, SPEC - 1), min(ksel, SPEC), min(ksel, SPEC + 6)   # below / at / above FILTER_SPEC
    total[:3] = np.minimum(2 * count[:3], CMAX)                                                 # every kept slot holds a survivor
    count[3] = ksel                                                                             # a list whose last slot is filled
    count[4], total[4] = ksel, CMAX                                                             # 64 survivors: not flagged
    count[5], total[5] = ksel, CMAX + 1                                                         # 65: flagged
    count[7], total[7] = 0, 0
    pi = np.empty((N_USERS, ksel, 2, cap), np.int64)
    survivors = []
    for u in range(N_USERS):
        items = None
        if u == DUP_USER:
            perm = rng.permutation(N_ITEMS)
            items = np.concatenate([np.array(DUP[::-1]), perm[~np.isin(perm, DUP)]])
            total[u] = max(total[u], 3)
        pi[u], s = fill_lists(rng, ksel, cap, int(count[u]), int(total[u]), full_list=(u == 3), items=items)
        survivors.append(s)
    n_surv = np.array([len(s) for s in survivors])
    flag = ((n_surv > CMAX) | (np.arange(N_USERS) == 3)).astype(np.int32)
    assert flag[4] == 0 and flag[5] == 1 and n_surv[7] == 0
    exp_v, exp_i = expected_rows(sc, survivors, k)
    gv, gi, gflag, gn = run_filter(N, "trec_topk_filter_finish", P, bias, pi, ksel, cap, count, k, np.zeros(N_USERS, np.int32))
    what = (dims, bias, ksel, cap, k)
    assert np.array_equal(gflag, flag) and gn == int(flag.sum()), (what, gflag, flag)
    check_rows(gv, gi, exp_v, exp_i, np.nonzero(n_surv <= CMAX)[0], what)


@pytest.mark.parametrize("k", [10, 16])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "k%d_ldu%d_ldv%d" % d)
def test_filter_finish_wide(N, dims, bias, k):
    """No capacity limits: ~150 survivors over 40 kept slots go through the queue's carry-over across the 48-entry batches and
    are answered; only a full list flags; count[u] > ksel is clamped to the ksel slots the buffer has."""
    P = problem(dims)
    ksel, cap = 48, 8
    rng = np.random.default_rng(k)
    sc = P.scores[bias]
    count = rng.integers(1, ksel + 1, size=N_USERS)
    total = np.array([rng.integers(0, min(100, c * 2 * (cap - 1)) + 1) for c in count])
    count[0], total[0] = 40, 150
    count[1] = 20                                                                               # a full list: flagged
    count[2], total[2] = ksel + 5, 2 * ksel                                                     # clamped: all ksel slots are read
    count[7], total[7] = 0, 0
    flag_in = np.zeros(N_USERS, np.int32)
    flag_in[9] = 1                                                                              # flagged before: answered all the same
    pi = np.empty((N_USERS, ksel, 2, cap), np.int64)
    survivors = []
    for u in range(N_USERS):
        items = None
        if u == DUP_USER:
            perm = rng.permutation(N_ITEMS)
            items = np.concatenate([np.array(DUP[::-1]), perm[~np.isin(perm, DUP)]])
            total[u] = max(total[u], 3)
        pi[u], s = fill_lists(rng, ksel, cap, int(count[u]), int(total[u]), full_list=(u == 1), items=items)
        survivors.append(s)
    assert len(survivors[0]) == 150 and np.all(pi[2, ksel - 1, :, 0] >= 0)
    flag = flag_in.copy()
    flag[1] = 1
    exp_v, exp_i = expected_rows(sc, survivors, k)
    gv, gi, gflag, gn = run_filter(N, "trec_topk_filter_finish_wide", P, bias, pi, ksel, cap, count, k, flag_in)
    what = (dims, bias, k)
    assert np.array_equal(gflag, flag) and gn == 1, (what, gflag, flag)
    check_rows(gv, gi, exp_v, exp_i, range(N_USERS), what)
