"""tests/step_reference.py means something: two float32 restatements of the WMRB step in different summation orders (one accumulator;
eight or sixteen interleaved partials added at the end, as the kernels do) lie inside every bar, every seeded one-line defect falls
outside one, and the case lists reach every instantiation and edge the GPU tests are meant to cover.  No GPU, no code under test."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import step_reference as SR
from pair_reference import MODE_DOT, MODE_EUCLID, f64

F = np.float32
osum = SR.osum
OUTPUTS = ("y_s", "y_p", "loss", "g_s", "g_p", "val_s", "val_p", "dU", "d_ub", "rowsum", "G", "dV", "d_ib")


def f32_step(case, biased, balanced, order, defect=None, ub=None, ib=None):
    """the step of csrc/wmrb_tiled_body.hpp restated in float32 numpy.  `defect` changes one line (see DEFECTS)."""
    U, V = case.U.astype(F), case.V.astype(F)
    ub = (case.ub if ub is None else ub).astype(F) if biased else None
    ib = (case.ib if ib is None else ib).astype(F) if biased else None
    w_all = SR.case_weights(case) if balanced else None
    nu, d, S, ni = case.n_users, case.d, case.S, case.n_items
    euclid = case.mode == MODE_EUCLID
    indptr, x_item, values = case.indptr, case.x_item.astype(np.int64), case.values
    pos = values > 0
    slot = np.cumsum(pos) - 1
    o = SimpleNamespace(y_s=np.zeros((nu, S), F), y_p=np.zeros(x_item.size, F), loss=np.zeros(int(pos.sum()), F),
                        g_s=np.zeros((nu, S), F), g_p=np.zeros(x_item.size, F), val_s=np.zeros((nu, S), F), val_p=np.zeros(x_item.size, F),
                        dU=np.zeros((nu, d), F), d_ub=np.zeros(nu, F), rowsum=np.zeros(nu, F), G=np.zeros((nu, ni), F),
                        dV=np.zeros((ni, d), F), d_ib=np.zeros(ni, F))
    ratio = F(ni // S) if defect == "ratio_integer_division" else F(ni) / F(S)
    users = range(nu) if order == "seq" else range(nu - 1, -1, -1)           # (the item side meets its pairs in another order)
    for u in users:
        idx = np.arange(indptr[u], indptr[u + 1])
        items = np.concatenate([case.samples[u].astype(np.int64), x_item[idx]])
        rows = V[items]
        if euclid:
            diff = U[u] - rows
            D = osum((diff * diff).T, order)
            y = -np.sqrt(np.maximum(D, F(1e-16)))
        else:
            D = None
            y = osum((U[u] * rows).T, order)
        if biased:
            y = (y + ub[u]) + ib[items]
        o.y_s[u], o.y_p[idx] = y[:S], y[S:]
        q = np.flatnonzero(pos[idx])
        if not q.size:
            continue
        base = F(1.0) - y[S + q]
        ys = y[:S]
        if defect == "padding_counted":                              # a sample past S - 1 clamped to S - 1 but still counted
            ys = np.concatenate([ys, np.repeat(ys[-1:], (-S) % 4)])
        H = base[:, None] + ys[None, :]
        act = (H > 0) if defect == "hinge_strict" else (H >= 0)
        hs = osum(np.maximum(H, F(0)).T, order)
        cnt = act.sum(1).astype(F)
        act = act[:, :S]
        smr = ratio * hs
        if balanced:
            smr = smr * w_all[idx[q]]
        c = ratio / (F(1.0) + smr)
        if balanced and defect != "weight_not_on_c":
            c = c * w_all[idx[q]]
        o.loss[slot[idx[q]]] = np.log(smr + F(1.0))
        g = np.zeros(items.size, F)
        g[:S] = osum(np.where(act, c[:, None], F(0)), order)
        g[S + q] = -c * cnt
        if euclid:
            if defect == "clamp_unclamped_coefficient":
                val = -g / np.sqrt(np.maximum(D, F(1e-16)))
            else:
                val = np.where(D >= F(1e-16), -g / np.sqrt(np.maximum(D, F(1e-30))), F(0))
            tu = U[u] - rows
        else:
            val, tu = g, rows
        o.g_s[u], o.g_p[idx], o.val_s[u], o.val_p[idx] = g[:S], g[S:], val[:S], val[S:]
        terms = val[:, None] * tu
        o.dU[u] = osum(terms[:-1] if defect == "last_row_left_out" else terms, order)
        o.d_ub[u], o.rowsum[u] = osum(g, order), osum(val, order)
        if defect == "duplicate_overwrites":
            o.G[u, items] = val
        else:
            np.add.at(o.G[u], items, val)
        tv = -tu if euclid else np.broadcast_to(U[u], rows.shape)
        np.add.at(o.dV, items, (val[:, None] * tv).astype(F))
        np.add.at(o.d_ib, items, g)
    return o


def ratios(out, ref, bars, names=OUTPUTS):
    """name -> largest |error| / bar (inf where the bar is 0 and the error is not)"""
    res = {}
    for n in names:
        got, want, bar = f64(getattr(out, n)), f64(getattr(ref, n)), f64(getattr(bars, n))
        err = np.abs(got - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, 0.0, err / bar)
        res[n] = float(r.max()) if r.size else 0.0
    return res


@functools.lru_cache(maxsize=4)
def fused(spec):
    return SR.fused_case(*spec)


@functools.lru_cache(maxsize=4)
def tiled(spec, mode):
    return SR.tiled_case(*spec, mode)


def check_properties(case, ref, bars):
    p = SR.case_properties(case, ref)
    assert SR.inputs_exact(case)
    assert 0.2 <= p["active_share"] <= 0.8, p["active_share"]
    assert p["no_interaction"] and p["nonpositive_only"] and p["one_positive"] and p["longest"] == case.longest
    assert p["inactive_users"] == [SR.U_INACTIVE]
    assert p["values_quarter"] and p["weights_not_one"]
    assert p["sample_is_positive"] and (p["duplicate_sample"] or case.S == 1)
    has_pos = np.array([u in ref.act for u in range(case.n_users)])
    if case.mode == MODE_DOT:
        hs = ref.hs * 64.0
        assert (hs == np.round(hs)).all() and hs.max() < 2 ** 24          # every hinge sum is exact in float32 in any order
        planted = has_pos.copy()
        planted[SR.U_INACTIVE] = False
        if case.S == 1:
            planted[SR.U_CLAMP] = False
        assert (p["zero_hinges"][planted] >= 1).all(), p["zero_hinges"]
    else:
        assert p["clamped"] and (p["zero_hinges"] == 0).all()
        assert np.isfinite(bars.min_abs_hinge) and p["n_hinges"] <= 400000


@pytest.mark.parametrize("spec", SR.FUSED_CASES, ids=lambda s: "S%d-L%d-d%d" % s)
def test_fused_cases_restated(spec):
    case = fused(spec)
    for biased, balanced in ((False, False), (True, True)):
        ref, bars = SR.case_ref(case, biased, balanced)
        check_properties(case, ref, bars)
        for order in ("seq", 8):
            r = ratios(f32_step(case, biased, balanced, order), ref, bars)
            assert max(r.values()) <= 1.0, (order, r)


@pytest.mark.parametrize("mode", [MODE_DOT, MODE_EUCLID], ids=["dot", "euclid"])
@pytest.mark.parametrize("spec", SR.TILED_CASES, ids=lambda s: "S%d-d%d" % s[:2])
def test_tiled_cases_restated(spec, mode):
    case = tiled(spec, mode)
    for biased, balanced in ((False, True), (True, False)):
        ref, bars = SR.case_ref(case, biased, balanced)
        check_properties(case, ref, bars)
        for order in ("seq", 16 if case.d <= 64 else 8):
            r = ratios(f32_step(case, biased, balanced, order), ref, bars)
            assert max(r.values()) <= 1.0, (order, r)


def test_tiled_big_case_restated():
    case = tiled(SR.TILED_BIG, MODE_DOT)
    ref, bars = SR.case_ref(case, True, True)
    check_properties(case, ref, bars)
    assert SR.tiled_lds_bytes(case.S, case.max_pos, case.d) > 65536 and case.max_pos == 1700
    for order in ("seq", 8):
        r = ratios(f32_step(case, True, True, order), ref, bars)
        assert max(r.values()) <= 1.0, (order, r)


def test_centred_dense_route_of_distances_restated():
    """d user_in = rowsum(G) (U - c) - G . (V - c) and d item_in = colsum(G) (V - c) - G^T . (U - c) with c the float32 mean item row, as
    ops_base.wmrb_tiled_step forms them on fp32 GEMMs, from the float32 G and row sums of the restated step: inside
    SR.dense_fp32_euclid_bars in both orders, while the bias-free form without the centring at an offset of 100 is not"""
    case = tiled(SR.TILED_CASES[4], MODE_EUCLID)
    ref, bars = SR.case_ref(case, True, True)
    bar_u, bar_v = SR.dense_fp32_euclid_bars(ref, bars, case.U, case.V, case.indptr, case.x_item, case.samples)
    assert (bar_u >= bars.dU * 0.999).all() and (bar_v >= bars.dV * 0.999).all()          # (the centred terms are no smaller)
    U, V = case.U.astype(F), case.V.astype(F)
    c = (osum(V, "seq") / F(case.n_items)).astype(F)
    uc, vc = U - c, V - c
    for order in ("seq", 8):
        o = f32_step(case, True, True, order)
        colsum = osum(o.G, order)
        d_u = o.rowsum[:, None] * uc - osum(o.G.T[:, :, None] * vc[:, None, :], order)
        d_v = colsum[:, None] * vc - osum(o.G[:, :, None] * uc[:, None, :], order)
        for got, want, bar, name in ((d_u, ref.dU, bar_u, "dU"), (d_v, ref.dV, bar_v, "dV")):
            err = np.abs(f64(got) - want)
            assert (err <= bar).all(), (order, name, float((err / np.maximum(bar, 1e-300)).max()))
    # the bar is no blanket: the same products taken about an origin 100 away (no centring) miss it
    far = F(100.0)
    d_u = o.rowsum[:, None] * (U + far) - osum(o.G.T[:, :, None] * (V + far)[:, None, :], 8)
    assert (np.abs(f64(d_u) - ref.dU) > bar_u).any()


# ------------------------------------------------------------------------------------------------ seeded defects
# defect -> (case, mode, biased, balanced, outputs of which at least one must leave its bar)
DEFECT_TILED = SR.TILED_CASES[2]                                    # S = 30, d = 68: 300 / 30 = 10 exactly ...
DEFECT_RATIO = SR.TILED_CASES[1]                                    # ... and 340 / 127 is no integer
DEFECTS = {
    "hinge_strict": (DEFECT_TILED, MODE_DOT, True, False, ("g_p", "g_s")),
    "last_row_left_out": (DEFECT_TILED, MODE_DOT, False, False, ("dU",)),
    "weight_not_on_c": (DEFECT_TILED, MODE_EUCLID, True, True, ("g_p", "g_s")),
    "ratio_integer_division": (DEFECT_RATIO, MODE_DOT, False, True, ("loss", "g_p")),
    "duplicate_overwrites": (DEFECT_TILED, MODE_DOT, False, False, ("G",)),
    "clamp_unclamped_coefficient": (DEFECT_TILED, MODE_EUCLID, False, False, ("val_s", "val_p", "dU")),
    "padding_counted": (DEFECT_TILED, MODE_EUCLID, True, False, ("loss", "g_p")),
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_seeded_defect_leaves_a_bar(defect):
    spec, mode, biased, balanced, where = DEFECTS[defect]
    case = tiled(spec, mode)
    ref, bars = SR.case_ref(case, biased, balanced)
    good = ratios(f32_step(case, biased, balanced, 8), ref, bars)
    assert max(good.values()) <= 1.0, good
    bad = ratios(f32_step(case, biased, balanced, 8, defect=defect), ref, bars)
    assert max(bad[n] for n in where) > 1.0, (defect, bad)


# ------------------------------------------------------------------------------------------------ the cooperative step
def f32_coop(case, biased, balanced, l2, order, defect=None):
    """tower forward, f32_step, tower backward and gg = g + l2 * w in float32"""
    X = case.X.tocsr()
    V = np.zeros((case.n_items, case.d), F)
    ib = np.zeros(case.n_items, F)
    for r in range(case.n_items):
        for j in range(X.indptr[r], X.indptr[r + 1]):
            V[r] = V[r] + F(X.data[j]) * case.Wi[X.indices[j]]
            ib[r] = ib[r] + F(X.data[j]) * case.bi[X.indices[j]]
    sub = SimpleNamespace(U=case.Wu, V=V, ub=case.bu, ib=ib, matrix=case.matrix, indptr=case.indptr, x_item=case.x_item, values=case.values,
                          samples=case.samples, S=case.S, d=case.d, mode=MODE_DOT, n_users=case.n_users, n_items=case.n_items)
    o = f32_step(sub, biased, balanced, order)
    o.V, o.ib = V, ib
    o.dWi, o.dbi = np.zeros_like(case.Wi), np.zeros_like(case.bi)
    rows = range(case.n_items) if order == "seq" else range(case.n_items - 1, -1, -1)
    for r in rows:
        for j in range(X.indptr[r], X.indptr[r + 1]):
            o.dWi[X.indices[j]] = o.dWi[X.indices[j]] + F(X.data[j]) * o.dV[r]
            o.dbi[X.indices[j]] = o.dbi[X.indices[j]] + F(X.data[j]) * o.d_ib[r]
    l2 = F(l2)
    o.gg = dict(Wu=o.dU + case.Wu * l2, Wi=o.dWi + case.Wi * l2)
    if biased:
        o.gg.update(bu=o.d_ub + case.bu * l2, bi=o.dbi + case.bi * l2)
        if defect == "bias_l2_left_out":
            o.gg.update(bu=o.d_ub, bi=o.dbi)
    return o


def coop_ref(case, biased, balanced, l2):
    w = SR.case_weights(case) if balanced else None
    ref = SR.ref_coop_step(case.Wu, case.Wi, case.bu if biased else None, case.bi if biased else None, case.X, case.indptr, case.x_item,
                           case.values, w, case.samples, case.n_items, l2)
    return ref, SR.coop_bars(ref, case.Wu, case.indptr, case.x_item, case.samples)


def gg_ratios(o, ref, bars):
    res = {}
    for k in ref.gg:
        err = np.abs(f64(o.gg[k]) - ref.gg[k])
        with np.errstate(divide="ignore", invalid="ignore"):
            res[k] = float(np.where(err == 0, 0.0, err / bars.gg[k]).max())
    return res


@pytest.mark.parametrize("spec", SR.COOP_CASES, ids=lambda s: "%dx%d-d%d-S%d" % s[:4])
def test_coop_cases_restated(spec):
    case = SR.coop_case(*spec)
    l2 = 3e-3
    for biased, balanced in ((True, True), (False, False)):
        ref, bars = coop_ref(case, biased, balanced, l2)
        hs = ref.hs * 64.0
        assert (hs == np.round(hs)).all() and hs.max() < 2 ** 18          # every hinge sum is exact in float32 in any order
        if spec[4] == "identity":
            # one user, one item: the only hinge there is is 1 - y + y = 1, active; no other condition can be planted
            assert ref.n_hinges == 1 and ref.n_active == 1
        else:
            p = SR.coop_case_properties(case, ref)
            assert 0.2 <= p.pop("active_share") <= 0.8
            assert p.pop("inactive_users") == [SR.U_INACTIVE]
            assert all(p.values()), p
        for order in ("seq", 8):
            o = f32_coop(case, biased, balanced, l2, order)
            r = ratios(o, ref, bars, names=OUTPUTS + (("dWi", "dbi") if biased else ("dWi",)))
            r.update(gg_ratios(o, ref, bars))
            assert max(r.values()) <= 1.0, (order, r)
    if spec[0] > 1:
        ref, bars = coop_ref(case, True, True, l2)
        bad = gg_ratios(f32_coop(case, True, True, l2, 8, defect="bias_l2_left_out"), ref, bars)
        assert bad["bu"] > 1.0 and bad["bi"] > 1.0, bad


# ------------------------------------------------------------------------------------------------ coverage of the instantiations
def test_case_lists_reach_every_instantiation_and_edge():
    took = {}
    for S, longest, d in SR.FUSED_CASES:
        took.setdefault(SR.fused_instantiation(S, longest, d), []).append(S + longest)
    assert set(took) == SR.ALL_FUSED_INSTANTIATIONS and len(SR.ALL_FUSED_INSTANTIATIONS) == 8
    rows = {(S + longest, SR.fused_rows_capacity(d)) for S, longest, d in SR.FUSED_CASES}
    assert (128, 128) in rows and (256, 256) in rows                # a case at each row capacity
    assert any(S + longest == 128 and d <= 128 for S, longest, d in SR.FUSED_CASES)       # the last shape of the 16-row kernels
    assert any(S + longest == 129 and d <= 128 for S, longest, d in SR.FUSED_CASES)       # the first of the 32-row ones
    assert SR.fused_instantiation(129, 128, 128) is None and SR.fused_instantiation(64, 65, 132) is None
    tiled_took = {SR.tiled_instantiation(d, mode) for _, d, _, _ in SR.TILED_CASES for mode in (0, 1)}
    assert tiled_took == SR.ALL_TILED_INSTANTIATIONS and len(SR.ALL_TILED_INSTANTIATIONS) == 8
    assert {d for _, d, _, _ in SR.TILED_CASES} == {4, 64, 68, 128, 132, 256, 260, 512}
    assert {S for S, _, _, _ in SR.TILED_CASES} >= {1, 1023, 1024, 1025}
    lens = set()
    for S, d, rows_, _ in SR.TILED_CASES:
        lens |= set(rows_)
        assert SR.tiled_lds_bytes(S, max(rows_), d) in range(1, 65537)
    assert lens >= {31, 32, 33, 65}
    for tile in (192, 96, 64, 32):                                  # R = S + rows at tile - 1, tile, tile + 1, 2 tile + 1
        assert any(SR.tiled_tile_rows(d) == tile and {tile - 1 - S, tile - S, tile + 1 - S, 2 * tile + 1 - S} <= set(rows_)
                   for S, d, rows_, _ in SR.TILED_CASES), tile
    S, d, _, _ = SR.TILED_BIG
    assert SR.tiled_lds_bytes(S, 1700, d) > 65536
    assert SR.tiled_lds_bytes(3000, 6000, 512) == -1


def test_coop_mirrors_on_the_case_list():
    segs = {SR.coop_seg_len(nu, d) for nu, _, d, _, _ in SR.COOP_CASES}
    assert 16 in segs and 128 in segs                               # the floor (fewer than 16 users) and the cap (eight live loads)
    assert SR.coop_seg_len(150, 68) == 19 and SR.coop_seg_len(1100, 16) == 128 and SR.coop_seg_len(257, 128) == 33
    for nu, ni, d, S, kind in SR.COOP_CASES:
        case = SR.coop_case(nu, ni, d, S, kind)
        assert SR.coop_workspace_floats(nu, ni, d, S, case.max_pos) == SR.coop_layout(nu, ni, d).total > 0
    X = SR.coop_features(333, "columns")
    sizes = np.bincount(X.indices, minlength=X.shape[1])
    assert list(sizes[333:]) == SR.COOP_COLUMN_SIZES and max(SR.COOP_COLUMN_SIZES) >= 200 and (sizes[:332] == 1).all()
    assert X.indptr[-1] == X.indptr[-2]                             # the last item holds no feature
    # a feature column longer than one phase-4 round on both kernels: 64 entries at 16 groups (d <= 64), 32 at 8
    longest_column = lambda ni: int(np.bincount(SR.coop_features(ni, "columns").indices).max())
    assert any(d <= 64 and k == "columns" and longest_column(ni) > 64 for _, ni, d, _, k in SR.COOP_CASES)
    assert any(d > 64 and k == "columns" and longest_column(ni) > 32 for _, ni, d, _, k in SR.COOP_CASES)
    assert any(ni < 16 for _, ni, _, _, _ in SR.COOP_CASES) and any(S == ni for _, ni, _, S, _ in SR.COOP_CASES)
