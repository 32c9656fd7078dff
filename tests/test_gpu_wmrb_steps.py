"""The one-pass WMRB step kernels a fit actually runs -- csrc/wmrb_fused.hip (trec_wmrb_fused_step), csrc/wmrb_tiled.hip +
csrc/wmrb_tiled_body.hpp (trec_wmrb_tiled_step), csrc/step_coop.hip (trec_fit_step_coop) -- against the float64 reference of
tests/step_reference.py, per element and per output, within the bars derived there (tests/test_step_reference_host.py shows on the CPU
that float32 restatements lie inside them and seeded defects outside).

* fused   every instantiation <ITERS, RMAX, SURE> at the smallest shapes that reach each edge (row counts at the register capacity,
          S on both sides of every SURE threshold), through ops.wmrb_fused_step (ranked grouping) and once per case at the ABI with
          the histogram and the ranks of the counting sort;
* tiled   every instantiation <ITERS, RB, MODE, LPR>, rows at tile - 1 / tile / tile + 1 / 2 tile + 1, the option combinations of the
          hosts and of the cooperative kernel (dU with dense_g), ldg > n_items, LDS above 64 KB, both host routes of ops.wmrb_tiled_step;
* coop    the workspace read through coop_layout after every call, so that a miss names its phase; Adam replayed bit for bit.

The largest error / bar per kernel and output is kept in RATIOS; with TREC_STEP_RATIOS_OUT=<file> it is written there at the end."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import step_reference as SR
from pair_reference import MODE_DOT, MODE_EUCLID, U32, f64
from test_gpu_pair_kernels import check, dev, tunings

pytestmark = pytest.mark.gpu

F = np.float32
RATIOS = {}


@pytest.fixture(scope="module")
def ops():
    from tensorrec_amd import ops as _ops, _native
    _native.require_gpu()
    _native.load()
    yield _ops
    out = os.environ.get("TREC_STEP_RATIOS_OUT")
    if out:
        write_ratios(out)


@pytest.fixture(scope="module")
def N(ops):
    from tensorrec_amd import _native
    return _native


def write_ratios(path):
    """profiles/wmrb_step_reference_ratios.json: the ratios of this run, merged (as maxima) into the record the file already holds, so
    that runs of parts of this module (-k fused, ...) into one file add up to the whole"""
    rec = {"what": "largest |kernel - float64 reference| / bar per kernel family and output over the cases of tests/test_gpu_wmrb_steps.py "
                   "(bars: tests/step_reference.py); a bar of 0 asks for equality and records 0",
           "command": "TREC_STEP_RATIOS_OUT=<this file> python -m pytest -m gpu tests/test_gpu_wmrb_steps.py", "ratios": {}}
    if os.path.exists(path):
        with open(path) as f:
            rec["ratios"] = json.load(f).get("ratios", {})
    for k, r in RATIOS.items():
        for n, v in r.items():
            rec["ratios"].setdefault(k, {})[n] = max(rec["ratios"].get(k, {}).get(n, 0.0), float("%.4g" % v))
    rec["ratios"] = {k: dict(sorted(r.items())) for k, r in sorted(rec["ratios"].items())}
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


def held(kernel, name, got, want, bar, what):
    """check(), with the largest error / bar kept per kernel and output (a bar of 0 asks for equality)"""
    g, w, b = f64(got).reshape(-1), f64(want).reshape(-1), f64(bar).reshape(-1)
    if g.shape == w.shape and g.size and np.isfinite(g).all():
        err = np.abs(g - w)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = float(np.where(err == 0, 0.0, err / b).max())
        RATIOS.setdefault(kernel, {})[name] = max(RATIOS.get(kernel, {}).get(name, 0.0), r)
    check(got, want, bar, "%s %s: %s" % (kernel, what, name))


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def interactions_of(case):
    from tensorrec_amd.sparse import Interactions
    inter = Interactions(case.matrix, case.n_users, case.n_items, "cuda")
    assert np.array_equal(inter.indptr.cpu().numpy(), case.indptr) and np.array_equal(inter.values.cpu().numpy(), case.values)
    assert np.array_equal(inter.x_item32.cpu().numpy(), case.x_item) and inter.max_row_nnz == case.max_pos
    # the weights are an input of the kernels: the reference takes the float32 values the kernels are handed
    assert np.array_equal(inter.balanced_weight().cpu().numpy(), SR.case_weights(case))
    return inter


@functools.lru_cache(maxsize=2)
def fused_inputs(spec):
    case = SR.fused_case(*spec)
    return case, {(b, w): SR.case_ref(case, b, w) for b in (False, True) for w in (False, True)}


@functools.lru_cache(maxsize=2)
def tiled_inputs(spec, mode):
    case = SR.tiled_case(*spec, mode)
    return case, {}


def tiled_ref(spec, mode, biased, balanced):
    case, refs = tiled_inputs(spec, mode)
    if (biased, balanced) not in refs:
        refs[(biased, balanced)] = SR.case_ref(case, biased, balanced)
    return case, refs[(biased, balanced)]


# ------------------------------------------------------------------------------------------------ fused
@pytest.mark.parametrize("balanced", [False, True], ids=["wmrb", "balanced"])
@pytest.mark.parametrize("biased", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("spec", SR.FUSED_CASES, ids=lambda s: "S%d-L%d-d%d" % s)
def test_fused_step_against_float64(ops, N, spec, biased, balanced):
    """all six results of ops.wmrb_fused_step: loss, serial predictions (dot scores of dyadic rows: bit for bit), d user_in, d item_in
    (transposed interactions + ranked counting sort + K1 gathers), d b_u (exactly 0 in exact arithmetic), d b_i"""
    case, refs = fused_inputs(spec)
    ref, bars = refs[(biased, balanced)]
    inst = SR.fused_instantiation(case.S, case.max_pos, case.d)
    assert inst is not None and N.query("trec_wmrb_fused_lds_bytes", case.S, case.max_pos, case.d) > 0
    assert N.query("trec_wmrb_fused_lds_bytes", case.S, SR.fused_rows_capacity(case.d) - case.S + 1, case.d) == -1
    inter = interactions_of(case)
    assert ops.wmrb_fused_supported(case.S, inter, case.d)
    loss, pred, d_u, d_v, d_ub, d_ib = ops.wmrb_fused_step(dev(case.U), dev(case.V), dev(case.ub) if biased else None,
                                                           dev(case.ib) if biased else None, inter, dev(case.samples), balanced=balanced)
    torch.cuda.synchronize()
    assert ops.LAST_FUSED_STATS["route"] == "ranked"
    what = "%s <%d,%d,%d> bias %d balanced %d" % ((spec,) + inst + (biased, balanced))
    assert (d_ub is None) == (not biased) and (d_ib is None) == (not biased)
    for name, got, want, bar in (("loss", loss, ref.loss, bars.loss), ("pred_serial", pred, ref.y_p, bars.y_p), ("dU", d_u, ref.dU, bars.dU),
                                 ("dV", d_v, ref.dV, bars.dV), ("d_ub", d_ub, ref.d_ub, bars.d_ub), ("d_ib", d_ib, ref.d_ib, bars.d_ib)):
        if got is not None:
            held("fused", name, got.cpu().numpy(), want, bar, what)
    assert not d_u.cpu().numpy()[[SR.U_NONE, SR.U_NONPOS, SR.U_INACTIVE]].any()


@pytest.mark.parametrize("spec", SR.FUSED_CASES, ids=lambda s: "S%d-L%d-d%d" % s)
def test_fused_step_abi_histogram_and_ranks(N, spec):
    """trec_wmrb_fused_step with sample_hist / sample_rank: the histogram is bincount(samples), the ranks of every item are a
    permutation of 0 .. count - 1 (users without interactions included), and the per-pair coefficients lie within their bars"""
    case, refs = fused_inputs(spec)
    ref, bars = refs[(True, True)]
    inter = interactions_of(case)
    nu, ni, S, d = case.n_users, case.n_items, case.S, case.d
    loss, pred, d_u, d_ub, coef_s, coef_p = nan(inter.n_positive), nan(inter.nnz), nan(nu, d), nan(nu), nan(nu, S), nan(inter.nnz)
    hist = torch.zeros(ni, dtype=torch.int32, device="cuda")
    ranks = torch.full((nu, S), -1, dtype=torch.int32, device="cuda")
    U, V, ub, ib, samples = dev(case.U), dev(case.V), dev(case.ub), dev(case.ib), dev(case.samples)
    N.call("trec_wmrb_fused_step", N.ptr(U), N.ptr(V), N.ptr(ub), N.ptr(ib), N.ptr(inter.indptr), N.ptr(inter.x_item32),
           N.ptr(inter.pos_slot), N.ptr(inter.balanced_weight()), N.ptr(samples), nu, ni, S, d, int(inter.max_row_nnz), N.ptr(loss),
           N.ptr(pred), N.ptr(d_u), N.ptr(d_ub), N.ptr(coef_s), N.ptr(coef_p), N.ptr(hist), N.ptr(ranks))
    torch.cuda.synchronize()
    assert np.array_equal(hist.cpu().numpy(), np.bincount(case.samples.reshape(-1), minlength=ni))
    rk, flat = ranks.cpu().numpy().reshape(-1), case.samples.reshape(-1)
    order = np.lexsort((rk, flat))
    want = np.concatenate([np.arange(c) for c in np.bincount(flat, minlength=ni)])
    assert np.array_equal(rk[order], want), "the ranks of an item are no permutation of 0 .. count - 1"
    what = "%s abi" % (spec,)
    for name, got, want_, bar in (("loss", loss, ref.loss, bars.loss), ("pred_serial", pred, ref.y_p, bars.y_p), ("dU", d_u, ref.dU, bars.dU),
                                  ("d_ub", d_ub, ref.d_ub, bars.d_ub), ("coef_samples", coef_s, ref.g_s, bars.g_s),
                                  ("coef_pairs", coef_p, ref.g_p, bars.g_p)):
        held("fused", name, got.cpu().numpy(), want_, bar, what)


# ------------------------------------------------------------------------------------------------ tiled: the entry point itself
# (biased, balanced, dU, dense_g, ldg beyond the padded items, val_rowsum): dU only (the grouped host route); dense_g + val_rowsum
# without dU (the dense host route) with ldg > n_items; dU + dense_g (what step_coop.hip asks of the body).  raw_* go with Euclidean
# scores and item biases, as in ops.wmrb_tiled_step.
TILED_VARIANTS = {"dU": (True, False, True, False, 0, False), "G+rowsum": (False, True, False, True, 8, True),
                  "dU+G": (True, True, True, True, 0, False)}


def run_tiled_abi(N, case, ref, bars, biased, balanced, want_dU, want_G, ldg_extra, want_rs, what):
    inter = interactions_of(case)
    nu, ni, S, d, mode = case.n_users, case.n_items, case.S, case.d, case.mode
    lds = N.query("trec_wmrb_tiled_lds_bytes", S, case.max_pos, d)
    assert lds == SR.tiled_lds_bytes(S, case.max_pos, d) > 0
    want_raw = mode == MODE_EUCLID and biased
    ldg = (ni + 3) // 4 * 4 + ldg_extra
    loss, pred, val_s, val_p = nan(inter.n_positive), nan(inter.nnz), nan(nu, S), nan(inter.nnz)
    d_u = nan(nu, d) if want_dU else None
    d_ub = nan(nu) if biased else None
    raw_s, raw_p = (nan(nu, S), nan(inter.nnz)) if want_raw else (None, None)
    G = torch.zeros((nu, ldg), dtype=torch.float32, device="cuda") if want_G else None
    rs = nan(nu) if want_rs else None
    U, V, samples = dev(case.U), dev(case.V), dev(case.samples)
    ub, ib = (dev(case.ub), dev(case.ib)) if biased else (None, None)
    weight = inter.balanced_weight() if balanced else None
    N.call("trec_wmrb_tiled_step", N.ptr(U), N.ptr(V), N.ptr(ub), N.ptr(ib), N.ptr(inter.indptr), N.ptr(inter.x_item32),
           N.ptr(inter.pos_slot), N.ptr(weight), N.ptr(samples), nu, ni, S, d, int(mode), int(inter.max_row_nnz), N.ptr(loss), N.ptr(pred),
           N.ptr(d_u), N.ptr(d_ub), N.ptr(val_s), N.ptr(val_p), N.ptr(raw_s), N.ptr(raw_p), N.ptr(G), ldg, N.ptr(rs))
    torch.cuda.synchronize()
    for name, got, want, bar in (("loss", loss, ref.loss, bars.loss), ("pred_serial", pred, ref.y_p, bars.y_p),
                                 ("val_samples", val_s, ref.val_s, bars.val_s), ("val_pairs", val_p, ref.val_p, bars.val_p),
                                 ("raw_samples", raw_s, ref.g_s, bars.g_s), ("raw_pairs", raw_p, ref.g_p, bars.g_p),
                                 ("dU", d_u, ref.dU, bars.dU), ("d_ub", d_ub, ref.d_ub, bars.d_ub), ("val_rowsum", rs, ref.rowsum, bars.rowsum)):
        if got is not None:
            held("tiled", name, got.cpu().numpy(), want, bar, what)
    if G is not None:
        g = G.cpu().numpy()
        held("tiled", "dense_g", g[:, :ni], ref.G, bars.G, what)
        assert not g[:, ni:].any(), what + ": a padding column of dense_g was written"
    if mode == MODE_EUCLID:
        # the clamped pairs of user 5 (its first interaction, its last sample): score -1e-8 + biases, value exactly 0
        b5 = case.indptr[SR.U_CLAMP]
        assert ref.D_p[b5] == 0 and ref.D_s[SR.U_CLAMP, S - 1] == 0 and ref.g_p[b5] != 0
        assert val_p.cpu().numpy()[b5] == 0 and val_s.cpu().numpy()[SR.U_CLAMP, S - 1] == 0
        if not biased:
            assert pred.cpu().numpy()[b5] == -np.sqrt(F(1e-16))


@pytest.mark.parametrize("variant", sorted(TILED_VARIANTS))
@pytest.mark.parametrize("mode", [MODE_DOT, MODE_EUCLID], ids=["dot", "euclid"])
@pytest.mark.parametrize("spec", SR.TILED_CASES, ids=lambda s: "S%d-d%d" % s[:2])
def test_tiled_step_abi_against_float64(N, spec, mode, variant):
    biased, balanced, want_dU, want_G, ldg_extra, want_rs = TILED_VARIANTS[variant]
    case, (ref, bars) = tiled_ref(spec, mode, biased, balanced)
    inst = SR.tiled_instantiation(case.d, mode)
    run_tiled_abi(N, case, ref, bars, biased, balanced, want_dU, want_G, ldg_extra, want_rs,
                  "S %d d %d <%d,%d,%d,%d> %s" % ((case.S, case.d) + inst + (variant,)))


@pytest.mark.parametrize("variant", ["dU+G", "G+rowsum"])
def test_tiled_step_lds_above_64k(N, variant):
    """S = 3,000, longest row 1,700, d = 512: 67,632 bytes of dynamic LDS, the hipFuncSetAttribute path (dot scores only: a distance case
    of this size would hold millions of hinges, some of them within the bars of their scores)"""
    biased, balanced, want_dU, want_G, ldg_extra, want_rs = TILED_VARIANTS[variant]
    case, (ref, bars) = tiled_ref(SR.TILED_BIG, MODE_DOT, biased, balanced)
    assert SR.tiled_lds_bytes(case.S, case.max_pos, case.d) > 65536
    run_tiled_abi(N, case, ref, bars, biased, balanced, want_dU, want_G, ldg_extra, want_rs, "LDS > 64 KB %s" % variant)


# ------------------------------------------------------------------------------------------------ tiled: the host routes
ROUTES = {"dense_split_bf16": (1, 1, "tiled+dense_g"), "dense_fp32": (1, 0, "tiled+dense_g"), "grouped": (0, 1, "tiled+grouped")}


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("mode", [MODE_DOT, MODE_EUCLID], ids=["dot", "euclid"])
@pytest.mark.parametrize("spec", [SR.TILED_CASES[1], SR.TILED_CASES[4]], ids=lambda s: "S%d-d%d" % s[:2])
def test_tiled_host_routes_against_float64(ops, N, spec, mode, route):
    """ops.wmrb_tiled_step on the dense-G route (split-bf16 and fp32 GEMMs) and on the grouped one.  d user_in / d item_in of the
    split-bf16 GEMMs take the 1e-4 bar include/tensorrec_hip.h documents for trec_gemm_f32_split_bf16, relative to the sum of the
    absolute terms of the products formed (Euclidean: centred at the mean item row); everything else the derived float32 bars.  On the
    fp32 dense route of distances the same centred products are formed: SR.dense_fp32_euclid_bars."""
    dense, split, name = ROUTES[route]
    case, (ref, bars) = tiled_ref(spec, mode, True, True)
    inter = interactions_of(case)
    with tunings(N, wmrb_dense_g=dense, dense_g_split_bf16=split):
        loss, pred, d_u, d_v, d_ub, d_ib = ops.wmrb_tiled_step(dev(case.U), dev(case.V), dev(case.ub), dev(case.ib), inter,
                                                               dev(case.samples), balanced=True, mode=mode)
        torch.cuda.synchronize()
    assert ops.LAST_FUSED_STATS["route"] == name
    bar_u, bar_v = bars.dU, bars.dV
    args = (ref, case.U, case.V, case.indptr, case.x_item, case.samples)
    if dense and split:
        bar_u, bar_v = SR.split_bf16_bars(*args)
    elif dense and mode == MODE_EUCLID:
        bar_u, bar_v = SR.dense_fp32_euclid_bars(ref, bars, case.U, case.V, case.indptr, case.x_item, case.samples)
    what = "S %d d %d mode %d %s" % (case.S, case.d, mode, route)
    kernel = "tiled_host_" + route
    for nm, got, want, bar in (("loss", loss, ref.loss, bars.loss), ("pred_serial", pred, ref.y_p, bars.y_p), ("dU", d_u, ref.dU, bar_u),
                               ("dV", d_v, ref.dV, bar_v), ("d_ub", d_ub, ref.d_ub, bars.d_ub), ("d_ib", d_ib, ref.d_ib, bars.d_ib)):
        held(kernel, nm, got.cpu().numpy(), want, bar, what)


# ------------------------------------------------------------------------------------------------ the cooperative step
def adam_elem(w, m, v, g, lr_t, beta1, beta2, eps, l2):
    """adam_elem of csrc/step_coop.hip:28-35 on float32 arrays, every operation rounded on its own; in place"""
    gg = g + w * F(l2) if l2 != 0 else g
    m += (gg - m) * (F(1.0) - F(beta1))
    v += (gg * gg - v) * (F(1.0) - F(beta2))
    w -= (m * F(lr_t)) / (np.sqrt(v) + F(eps))


class CoopState(object):
    NAMES = ("Wu", "Wi", "bu", "bi")

    def __init__(self, case, biased):
        self.biased = biased
        self.names = self.NAMES if biased else self.NAMES[:2]
        self.t = {}
        for n in self.names:
            w = dev(getattr(case, n).copy())
            self.t[n] = (w, torch.zeros_like(w), torch.zeros_like(w))

    def host(self):
        return {n: tuple(x.cpu().numpy().copy() for x in self.t[n]) for n in self.names}


def coop_call(N, case, inter, itf, state, weight, samples, lr_t, beta1, l2, ws, loss, pred, seed=0, step=0, user_base=0):
    lib = N.load()
    ft_indptr, ft_rows, ft_perm = itf.transposed()
    p = []
    for n in CoopState.NAMES:
        p += [N.ptr(x) for x in state.t[n]] if n in state.t else [None, None, None]
    rc = lib.trec_fit_step_coop(*p, N.ptr(itf.indptr), N.ptr(itf.indices), N.ptr(itf.values), N.ptr(ft_indptr), N.ptr(ft_rows), N.ptr(ft_perm),
                                N.ptr(inter.indptr), N.ptr(inter.x_item32), N.ptr(inter.pos_slot), N.ptr(weight), N.ptr(samples),
                                case.n_users, case.n_items, case.n_features, case.d, case.S, int(inter.max_row_nnz), int(user_base),
                                int(seed), int(step), float(lr_t), float(beta1), 0.999, 1e-8, float(l2), N.ptr(ws), int(ws.numel()),
                                N.ptr(loss), N.ptr(pred), N.stream())
    torch.cuda.synchronize()
    assert rc != 3, "trec_fit_step_coop: cooperative launch refused: %s" % lib.trec_last_error().decode()
    assert rc == 0, "trec_fit_step_coop failed (code %d): %s" % (rc, lib.trec_last_error().decode())


def coop_workspace(N, case):
    lay = SR.coop_layout(case.n_users, case.n_items, case.d)
    need = int(N.query("trec_fit_step_coop_workspace_floats", case.n_users, case.n_items, case.d, case.S, case.max_pos))
    assert need == lay.total == SR.coop_workspace_floats(case.n_users, case.n_items, case.d, case.S, case.max_pos)
    return lay, nan(need)


def read_workspace(ws, lay, case):
    w = ws.cpu().numpy()
    nu, ni, d = case.n_users, case.n_items, case.d
    return dict(V=w[lay.V:lay.V + ni * d].reshape(ni, d), ib=w[lay.ib:lay.ib + ni], G=w[lay.G:lay.G + nu * lay.ldg].reshape(nu, lay.ldg),
                dU=w[lay.dU:lay.dU + nu * d].reshape(nu, d), dub=w[lay.dub:lay.dub + nu], dV=w[lay.dV:lay.dV + ni * d].reshape(ni, d),
                dib=w[lay.dib:lay.dib + ni])


def check_coop_phases(wk, ref, bars, case, biased, what, loss, pred):
    ni = case.n_items
    held("coop", "V (phase 1)", wk["V"], ref.V, np.zeros_like(ref.V), what)
    if biased:
        held("coop", "ib (phase 1)", wk["ib"], ref.ib, np.zeros_like(ref.ib), what)
    held("coop", "loss (phase 2)", loss.cpu().numpy(), ref.loss, bars.loss, what)
    held("coop", "pred_serial (phase 2)", pred.cpu().numpy(), ref.y_p, bars.y_p, what)
    held("coop", "G (phase 2)", wk["G"][:, :ni], ref.G, bars.G, what)
    assert not wk["G"][:, ni:].any(), what + ": a padding column of G is not 0"
    held("coop", "dU (phase 2)", wk["dU"], ref.dU, bars.dU, what)
    held("coop", "dV (phase 3)", wk["dV"], ref.dV, bars.dV, what)
    if biased:
        held("coop", "dub (phase 2)", wk["dub"], ref.d_ub, bars.d_ub, what)
        held("coop", "dib (phase 3)", wk["dib"], ref.d_ib, bars.d_ib, what)


def phase4_gradients(wk, case, biased):
    """the gradients phase 4 hands to Adam, bit for bit: dU and dub as they stand; d W_i[f] / d beta_i[f] as step_coop.hip:210-253 sums
    them -- the column's entries in transposed-CSR order dealt to the 16 (d <= 64) or 8 groups in turn, a chain per group (fmaf with
    x = 1 is a plain addition), the groups' sums added in group order"""
    n_grp = 16 if case.d // 4 <= 16 else 8
    Xt = case.X.T.tocsr()
    Xt.sort_indices()
    assert (Xt.data == 1).all()
    dWi, dbi = np.zeros((case.n_features, case.d), F), np.zeros(case.n_features, F)
    for f in range(case.n_features):
        rows = Xt.indices[Xt.indptr[f]:Xt.indptr[f + 1]]
        if rows.size:
            dWi[f] = SR.osum(wk["dV"][rows], n_grp)
            if biased:
                dbi[f] = SR.osum(wk["dib"][rows], n_grp)
    g = dict(Wu=wk["dU"].copy(), Wi=dWi)
    if biased:
        g.update(bu=wk["dub"].copy(), bi=dbi)
    return g


def run_coop_case(N, ops, spec, biased, balanced, samples_from_kernel=False):
    from tensorrec_amd.sparse import SparseFeatures
    from oracle import oracle as O
    case = SR.coop_case(*spec)
    inter = interactions_of(case)
    itf = SparseFeatures(case.X, "cuda")
    assert itf.shape == (case.n_items, case.n_features)
    weight = inter.balanced_weight() if balanced else None
    what = "%dx%d d %d S %d bias %d balanced %d" % (spec[:4] + (biased, balanced))
    seed, step, user_base = 0x1234567890ABCDEF, 7, 1000
    if samples_from_kernel:
        table = ops.sample_items(case.n_users, case.n_items, case.S, False, seed, step, user_base=user_base)
        case.samples = table.cpu().numpy()
        assert all(np.unique(r).size == case.S for r in case.samples[:50])
    l2 = float(F(3e-3))
    w64 = SR.case_weights(case) if balanced else None
    ref = SR.ref_coop_step(case.Wu, case.Wi, case.bu if biased else None, case.bi if biased else None, case.X, case.indptr, case.x_item,
                           case.values, w64, case.samples, case.n_items, l2)
    bars = SR.coop_bars(ref, case.Wu, case.indptr, case.x_item, case.samples)
    hs = ref.hs * 64.0
    assert (hs == np.round(hs)).all() and hs.max() < 2 ** 18               # dyadic weights: every hinge sum is exact
    lay, ws = coop_workspace(N, case)
    loss, pred = nan(inter.n_positive), nan(inter.nnz)
    state = CoopState(case, biased)
    if samples_from_kernel:
        # the same call handed the table and drawing it itself: loss and serial predictions bit for bit (phase 3 adds with float atomics:
        # the gradients are held to the bars, not to each other)
        other, ws2, loss2, pred2 = CoopState(case, biased), nan(ws.numel()), nan(inter.n_positive), nan(inter.nnz)
        coop_call(N, case, inter, itf, other, weight, table, 0.0, 0.5, 0.0, ws2, loss2, pred2)
        coop_call(N, case, inter, itf, state, weight, None, 0.0, 0.5, 0.0, ws, loss, pred, seed=seed, step=step, user_base=user_base)
        assert torch.equal(loss, loss2) and torch.equal(pred, pred2), what + ": the in-kernel sampler drew other items"
        check_coop_phases(read_workspace(ws2, lay, case), ref, bars, case, biased, what + " (table)", loss2, pred2)
        check_coop_phases(read_workspace(ws, lay, case), ref, bars, case, biased, what + " (in-kernel sampler)", loss, pred)
        return
    table = dev(case.samples)
    # ---- first call: zero slots, beta1 = 0.5, l2 = 0: m = 0 + (g - 0) * 0.5, so 2 m is the gradient bit for bit.  lr_t = 0 leaves the
    # weights as they are (w - 0 / (sqrt(v) + eps)): the second call then runs on the state this call left -- its slots -- with inputs
    # that are still dyadic, i.e. with scores, hinges and active sets that are still exact
    before = state.host()
    coop_call(N, case, inter, itf, state, weight, table, 0.0, 0.5, 0.0, ws, loss, pred)
    wk = read_workspace(ws, lay, case)
    check_coop_phases(wk, ref, bars, case, biased, what + " call 1", loss, pred)
    grads = phase4_gradients(wk, case, biased)
    after = state.host()
    wants = dict(Wu=(ref.dU, bars.dU), Wi=(ref.dWi, bars.dWi))
    if biased:
        wants.update(bu=(ref.d_ub, bars.d_ub), bi=(ref.dbi, bars.dbi))
    for n in state.names:
        w, m, v = (x.copy() for x in before[n])
        assert np.array_equal(2.0 * after[n][1], grads[n]), "%s call 1: 2 m of %s is not the gradient phase 4 summed" % (what, n)
        held("coop", "gradient of %s (phase 4, 2 m)" % n, 2.0 * after[n][1], wants[n][0], wants[n][1], what + " call 1")
        adam_elem(w, m, v, grads[n], 0.0, 0.5, 0.999, 1e-8, 0.0)
        for k, (a, b) in enumerate(zip((w, m, v), after[n])):
            assert np.array_equal(a, b), "%s call 1: %s of %s is not the float32 replay of adam_elem" % (what, "wmv"[k], n)
    # ---- second call on that state: l2 != 0, beta1 = 0.9, a real step size
    lr_t = float(O.adam_lr_t(0.05, 2))
    before = after
    coop_call(N, case, inter, itf, state, weight, table, lr_t, 0.9, l2, ws, loss, pred)
    wk = read_workspace(ws, lay, case)
    check_coop_phases(wk, ref, bars, case, biased, what + " call 2", loss, pred)
    grads = phase4_gradients(wk, case, biased)
    after = state.host()
    omb1 = float(F(1.0) - F(0.9))
    for n in state.names:
        w, m, v = (x.copy() for x in before[n])
        # gg = g + l2 w recovered from the first moment: m' = m + (gg - m) (1 - beta1), three roundings on the way
        rec = (f64(after[n][1]) - f64(m)) / omb1 + f64(m)
        rec_bar = U32 * (3.0 * np.abs(ref.gg[n] - f64(m)) + 1.01 * np.abs(f64(after[n][1])) / omb1)
        held("coop", "g + l2 w of %s (phase 4, from m)" % n, rec, ref.gg[n], bars.gg[n] + rec_bar, what + " call 2")
        O.adam_tf_step(w, m, v, grads[n] + w * F(l2), lr_t)
        for k, (a, b) in enumerate(zip((w, m, v), after[n])):
            assert np.array_equal(a, b), "%s call 2: %s of %s is not the float32 replay of adam_elem" % (what, "wmv"[k], n)
        assert not np.array_equal(after[n][0], before[n][0])
    # ---- the first step of a fit as the trainer makes it: zero slots AND a real step size, on a fresh copy of the (dyadic) state
    fresh = CoopState(case, biased)
    before = fresh.host()
    lr_1 = float(O.adam_lr_t(0.05, 1))
    coop_call(N, case, inter, itf, fresh, weight, table, lr_1, 0.9, l2, ws, loss, pred)
    wk = read_workspace(ws, lay, case)
    check_coop_phases(wk, ref, bars, case, biased, what + " first step", loss, pred)
    grads = phase4_gradients(wk, case, biased)
    after = fresh.host()
    for n in fresh.names:
        w, m, v = (x.copy() for x in before[n])
        O.adam_tf_step(w, m, v, grads[n] + w * F(l2), lr_1)
        for k, (a, b) in enumerate(zip((w, m, v), after[n])):
            assert np.array_equal(a, b), "%s first step: %s of %s is not the float32 replay of adam_elem" % (what, "wmv"[k], n)
        assert not np.array_equal(after[n][0], before[n][0])


@pytest.mark.parametrize("biased,balanced", [(True, True), (False, False)], ids=["bias-balanced", "nobias-wmrb"])
@pytest.mark.parametrize("spec", SR.COOP_CASES, ids=lambda s: "%dx%d-d%d-S%d" % s[:4])
def test_coop_step_against_float64(ops, N, spec, biased, balanced):
    """three calls of trec_fit_step_coop as _CoopStep.run makes them (tensorrec.py), every phase read from the workspace: zero slots with
    beta1 = 0.5, l2 = 0 and lr_t = 0 (2 m is the gradient); on the state that left, l2 != 0, beta1 = 0.9 and a real step; and on a fresh
    state the first step of a fit, zero slots with a real step"""
    run_coop_case(N, ops, spec, biased, balanced)


@pytest.mark.parametrize("spec", [SR.COOP_CASES[2], SR.COOP_CASES[3]], ids=lambda s: "%dx%d-d%d-S%d" % s[:4])
def test_coop_step_in_kernel_sampler(ops, N, spec):
    """samples = NULL with (seed, step, user_base != 0) against the same call handed ops.sample_items(..., user_base=...)"""
    run_coop_case(N, ops, spec, True, False, samples_from_kernel=True)
