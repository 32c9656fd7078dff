"""K1 (csrc/spmm.hip) against tests/k1_reference.py: every instantiation of spmm_csr_vec4_kernel the entry points can launch, the scalar
fallback, spmm_one_per_row_kernel and the tower kernels (tests/test_k1_reference_host.py shows on the CPU that the case list reaches all of
them and that the bars are not too tight).

* bit for bit against oracle.spmm_exact: the gather under epilogues 0 and 3, max(chain + b, 0) under epilogue 2, the fp32 rows of the filter
  operand, packed entries, one non-zero per row; an accumulating call against the NumPy chain started from the base;
* within the derived bars of float64: normalised rows and 1 / norm, row sums, the filter operand's norms, row_l2norm_fwd / bwd, column sums
  and both towers (output, dW, db);
* every call first asserts that the dispatch rule (k1_reference.pick_kernel) sends it to the instantiation the case was written for.

The largest error / bar per group and output is kept in RATIOS; with TREC_K1_RATIOS_OUT=<file> it is written there at the end
(profiles/k1_reference_ratios.json)."""
import functools
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import k1_reference as R
from k1_reference import F32, f64
from oracle import oracle as O

pytestmark = pytest.mark.gpu

RATIOS = {}
UNSET = -(2 ** 31) + 12345                                    # no tuning holds this value


@pytest.fixture(scope="module")
def ops():
    from tensorrec_amd import ops as _ops, _native
    _native.require_gpu()
    _native.load()
    yield _ops
    out = os.environ.get("TREC_K1_RATIOS_OUT")
    if out:
        write_ratios(out)


@pytest.fixture(scope="module")
def N(ops):
    from tensorrec_amd import _native
    return _native


def write_ratios(path):
    """profiles/k1_reference_ratios.json: the ratios of this run, merged (as maxima) into the record the file already holds"""
    rec = {"what": "largest |result - float64 reference| / bar per case group and output over the cases of tests/test_gpu_k1.py (bars: "
                   "tests/k1_reference.py); outputs held to equality are not listed",
           "command": "TREC_K1_RATIOS_OUT=<this file> python -m pytest -m gpu tests/test_gpu_k1.py", "ratios": {}}
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


def dev(a):
    """a device copy (the cached inputs of k1_reference are read-only on the host)"""
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


class tunings(object):
    """``with tunings(N, spmm_nt=0):`` -- set through _native.set_tuning, put back on exit (a knob that was not set is cleared again)"""

    def __init__(self, N, **values):
        self.N, self.values = N, values

    def __enter__(self):
        lib = self.N.load()
        self.before = {k: lib.trec_get_tuning(k.encode(), UNSET) for k in self.values}
        for k, v in self.values.items():
            self.N.set_tuning(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.before.items():
            if v == UNSET:
                self.N.clear_tuning(k)
            else:
                self.N.set_tuning(k, v)
        return False


def within(group, name, got, want, bar, what):
    """|got - want| <= bar elementwise (a bar of 0 asks for equality), nothing left out; records the largest ratio"""
    got, want = f64(got), f64(want)
    assert got.shape == want.shape, what
    bar = np.broadcast_to(f64(bar), want.shape)
    assert np.isfinite(got).all(), "%s %s: %d entries not written or not finite" % (what, name, int((~np.isfinite(got)).sum()))
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bar)
    r = float(ratio.max()) if ratio.size else 0.0
    print("%s %s: largest error / bar %.3f" % (what, name, r))
    if np.isfinite(r):
        RATIOS.setdefault(group, {})[name] = max(RATIOS.get(group, {}).get(name, 0.0), r)
    bad = err > bar
    if bad.any():
        k = int(np.argmax(np.where(bad, ratio, 0)))
        raise AssertionError("%s %s: %d of %d outside the bar; worst at %d: got %r, float64 %r, bar %.3e (ratio %.2f)"
                             % (what, name, int(bad.sum()), got.size, k, got.reshape(-1)[k], want.reshape(-1)[k], bar.reshape(-1)[k],
                                ratio.reshape(-1)[k]))


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = ~((got == want) | ((got != got) & (want != want)))
    assert not bad.any(), "%s: %d of %d entries differ, first at %r: got %r, want %r" % (
        what, int(bad.sum()), got.size, tuple(np.argwhere(bad)[0]), got[bad][0], want[bad][0])


@functools.lru_cache(maxsize=None)
def exact(case_id):
    """the float32 chain of a case (oracle.spmm_exact on the values in CSR order), computed once"""
    case = next(c for c in R.CASES if c.id == case_id)
    m = case.matrix()
    _, _, vals = R.case_values(case)
    out = O.spmm_exact(sp.csr_matrix((vals, m.indices, m.indptr), shape=m.shape), R.weights(m.shape[1], case.d))
    out.setflags(write=False)
    return out


def by_group(*groups):
    return dict(argvalues=[c for c in R.CASES if c.group in groups], ids=lambda c: c.id)


def upload(case):
    m = case.matrix()
    store, perm, vals = R.case_values(case)
    return dict(indptr=dev(m.indptr.astype(np.int64)), indices=dev(m.indices.astype(np.int32)), values=dev(store), perm=dev(perm),
                W=dev(R.weights(m.shape[1], case.d)), b=dev(R.bias(case.d))), vals


# ------------------------------------------------------------------------------------------------ trec_spmm_csr
def run_csr(N, case, t, l):
    m = case.matrix()
    n, d = m.shape[0], case.d
    assert R.pick_kernel(n, m.nnz, d, l.epi, l.accumulate, l.tuning, l.entry) == l.expect, case.id
    if l.accumulate:
        base, rs_base = R.accumulate_base(n, d)
        out, aux = dev(base), dev(rs_base)
    else:
        out, aux = nan(n, d), nan(n)
    with tunings(N, **l.tuning):
        N.call("trec_spmm_csr", N.ptr(t["indptr"]), N.ptr(t["indices"]), N.ptr(t["values"]), N.ptr(t["perm"]), n, m.nnz, N.ptr(t["W"]), d,
               N.ptr(t["b"]) if l.epi == 2 else None, l.epi, l.accumulate, N.ptr(out), N.ptr(aux) if l.epi in (1, 3) else None)
    torch.cuda.synchronize()
    return out.cpu().numpy(), aux.cpu().numpy()


def check_csr(case, l, vals, got, aux):
    m = case.matrix()
    n, d = m.shape[0], case.d
    W, b = R.weights(m.shape[1], d), R.bias(d)
    chain = exact(case.id)
    empty = np.diff(m.indptr) == 0
    what = "%s epilogue %d%s %r" % (case.id, l.epi, " accumulate" if l.accumulate else "", l.expect)
    assert empty.sum() >= 2
    if l.accumulate:
        base, rs_base = R.accumulate_base(n, d)
        same(got, R.chain32(m.indptr, m.indices, vals, W, base), what + ": not the chain started from the base")
        same(got[empty], base[empty], what + ": an empty row is not its base")
        if l.epi == 3:
            s, bar = R.segsum_ref(m.indptr, vals, rs_base)
            within(case.group, "row sums on a base", aux, s, bar, what)
        return
    if l.epi in (0, 3):
        same(got, chain, what + ": not the oracle's chain")
        assert (got[empty] == 0).all()
    if l.epi == 3:
        s, bar = R.segsum_ref(m.indptr, vals)
        within(case.group, "row sums", aux, s, bar, what)
        assert (aux[empty] == 0).all()
    if l.epi == 2:
        same(got, np.maximum(chain + b, F32(0)), what + ": not max(chain + b, 0)")
        same(got[empty], np.broadcast_to(np.maximum(b, F32(0)), got[empty].shape), what + ": an empty row is not relu(b)")
        assert (got[R.ROW_RELU0] == 0).all()
    if l.epi == 1:
        nr = R.normalize_ref(chain)
        within(case.group, "normalised rows", got, nr.y, nr.bar_y, what)
        within(case.group, "1 / norm", aux, nr.inv, nr.bar_inv, what)
        zero = nr.ss == 0
        assert zero[empty].all() and zero[R.ROW_ZERO_W] and (got[zero] == 0).all() and (aux[zero] == R.INV_EPS32).all(), what
        assert aux[R.ROW_CLAMPED] == R.INV_EPS32 and aux[R.ROW_SMALL] < R.INV_EPS32, what


@pytest.mark.parametrize("case", **by_group("r4", "r4wide", "r4plain", "r4perm", "scalar"))
def test_spmm_csr(ops, N, case):
    t, vals = upload(case)
    for l in case.launches:
        got, aux = run_csr(N, case, t, l)
        check_csr(case, l, vals, got, aux)


@pytest.mark.parametrize("case", **by_group("r1"))
def test_spmm_csr_one_row_per_subgroup(ops, N, case):
    """R = 1; the 4,095-row matrix is the head of the 4,099-row one, which takes R = 4: the same bits, row for row"""
    t, vals = upload(case)
    big = getattr(case, "same_as_r4", False)
    if big:
        mb = R.short_csr(4099, R.F_BIG, R.SEED, 2)
        tb = dict(t, indptr=dev(mb.indptr.astype(np.int64)), indices=dev(mb.indices.astype(np.int32)), values=dev(mb.data))
        assert np.array_equal(R.prefix_csr(mb, 4095).toarray(), case.matrix().toarray())
    for l in case.launches:
        got, aux = run_csr(N, case, t, l)
        check_csr(case, l, vals, got, aux)
        if big:
            n = mb.shape[0]
            assert R.pick_kernel(n, mb.nnz, case.d, l.epi)[2] == 4
            out, inv = nan(n, case.d), nan(n)
            N.call("trec_spmm_csr", N.ptr(tb["indptr"]), N.ptr(tb["indices"]), N.ptr(tb["values"]), None, n, mb.nnz, N.ptr(tb["W"]), case.d,
                   N.ptr(tb["b"]) if l.epi == 2 else None, l.epi, 0, N.ptr(out), N.ptr(inv) if l.epi in (1, 3) else None)
            torch.cuda.synchronize()
            same(out.cpu().numpy()[:4095], got, "%s epilogue %d: R = 1 and R = 4 differ" % (case.id, l.epi))
            if l.epi in (1, 3):
                same(inv.cpu().numpy()[:4095], aux, "%s epilogue %d: R = 1 and R = 4 differ in the second output" % (case.id, l.epi))


# ------------------------------------------------------------------------------------------------ trec_spmm_csr_filter
@pytest.mark.parametrize("case", **by_group("filter"))
def test_spmm_csr_filter(ops, N, case):
    t, _ = upload(case)
    m = case.matrix()
    n, d = m.shape[0], case.d
    (l,) = case.launches
    assert R.pick_kernel(n, m.nnz, d, 4, 0, l.tuning) == l.expect, case.id
    out, stats = nan(n, d), nan(n, 2)
    bf16 = torch.full((n, d), float("nan"), dtype=torch.bfloat16, device="cuda")
    gstats = torch.zeros((3,), dtype=torch.float32, device="cuda")
    with tunings(N, **l.tuning):
        N.call("trec_spmm_csr_filter", N.ptr(t["indptr"]), N.ptr(t["indices"]), N.ptr(t["values"]), n, m.nnz, N.ptr(t["W"]), d, N.ptr(out),
               N.ptr(bf16), N.ptr(stats), N.ptr(gstats))
    torch.cuda.synchronize()
    chain, what = exact(case.id), "%s %r" % (case.id, l.expect)
    fr = R.filter_ref(chain)
    same(out.cpu().numpy(), chain, what + ": fp32 rows are not the oracle's chain")
    same(bf16.view(torch.int16).cpu().numpy().view(np.uint16), fr.bits, what + ": bf16 image is not the round-to-nearest-even of the row")
    st = stats.cpu().numpy()
    within("filter", "row norms", st[:, 0], fr.stats[:, 0], fr.bar[:, 0], what)
    within("filter", "rounding error norms", st[:, 1], fr.stats[:, 1], fr.bar[:, 1], what)
    empty = np.diff(m.indptr) == 0
    assert empty.sum() >= 2 and (st[empty] == 0).all() and (out.cpu().numpy()[empty] == 0).all() and (fr.bits[empty] == 0).all()
    same(gstats.cpu().numpy(), np.array([st[:, 0].max(), st[:, 1].max(), 0], F32), what + ": running maxima")


# ------------------------------------------------------------------------------------------------ trec_spmm_csr_packed
@pytest.mark.parametrize("case", **by_group("packed"))
def test_spmm_csr_packed(ops, N, case):
    t, vals = upload(case)
    m = case.matrix()
    n, d = m.shape[0], case.d
    entries = dev(R.packed_entries(m))
    W = R.weights(m.shape[1], d)
    for l in case.launches:
        assert R.pick_kernel(n, m.nnz, d, l.epi, l.accumulate, entry="packed") == l.expect
        base, rs_base = R.accumulate_base(n, d)
        out, rs = (dev(base), dev(rs_base)) if l.accumulate else (nan(n, d), nan(n))
        N.call("trec_spmm_csr_packed", N.ptr(t["indptr"]), N.ptr(entries), n, N.ptr(t["W"]), d, l.epi, l.accumulate, N.ptr(out),
               N.ptr(rs) if l.epi == 3 else None)
        torch.cuda.synchronize()
        what = "%s epilogue %d accumulate %d" % (case.id, l.epi, l.accumulate)
        same(out.cpu().numpy(), R.chain32(m.indptr, m.indices, vals, W, base) if l.accumulate else exact(case.id), what)
        if l.epi == 3:
            s, bar = R.segsum_ref(m.indptr, vals, rs_base if l.accumulate else None)
            within("packed", "row sums", rs.cpu().numpy(), s, bar, what)


# ------------------------------------------------------------------------------------------------ trec_spmm_one_per_row
@pytest.mark.parametrize("case", **by_group("one_per_row"))
def test_spmm_one_per_row(ops, N, case):
    t, _ = upload(case)
    m = case.matrix()
    n, d = m.shape[0], case.d
    assert R.pick_kernel(n, m.nnz, d, 0, entry="one_per_row") == case.launches[0].expect
    assert m.nnz == n and np.array_equal(m.indptr, np.arange(n + 1)) and m.indices.max() < m.shape[1]
    out = nan(n, d)
    N.call("trec_spmm_one_per_row", N.ptr(t["indices"]), N.ptr(t["values"]), n, N.ptr(t["W"]), d, N.ptr(out))
    torch.cuda.synchronize()
    same(out.cpu().numpy(), exact(case.id), case.id)


# ------------------------------------------------------------------------------------------------ row kernels
@pytest.mark.parametrize("n,d", R.ROWNORM_CASES)
def test_row_l2norm_fwd_bwd(ops, N, n, d):
    x, dy = R.dense_rows(n, d, R.SEED), R.gradient(n, d, 3)
    nr = R.normalize_ref(x)
    what = "%d x %d" % (n, d)
    tx, y, inv = dev(x), nan(n, d), nan(n)
    N.call("trec_row_l2norm_fwd", N.ptr(tx), n, d, N.ptr(y), N.ptr(inv))
    torch.cuda.synchronize()
    within("row_l2norm", "fwd y", y.cpu().numpy(), nr.y, nr.bar_y, what)
    within("row_l2norm", "fwd 1 / norm", inv.cpu().numpy(), nr.inv, nr.bar_inv, what)
    same(inv.cpu().numpy()[nr.clamped], np.full(int(nr.clamped.sum()), R.INV_EPS32), what + ": a clamped row's 1 / norm")
    if n >= 16:
        assert nr.clamped[[1, n - 1, R.ROW_CLAMPED]].all() and not nr.clamped[R.ROW_SMALL] and (y.cpu().numpy()[[1, n - 1]] == 0).all()
    y32, inv32 = R.l2norm_bwd_inputs(nr)
    want, bar = R.l2norm_bwd_ref(nr, dy)
    ty, tinv, tdy, dx = dev(y32), dev(inv32), dev(dy), nan(n, d)
    N.call("trec_row_l2norm_bwd", N.ptr(ty), N.ptr(tinv), N.ptr(tdy), n, d, N.ptr(dx))
    torch.cuda.synchronize()
    within("row_l2norm", "bwd dx", dx.cpu().numpy(), want, bar, what)


def test_csr_to_dense_and_segment_sums(ops, N):
    """rows of 0, 1, 64, 65 and 200 entries: the wave's second and fourth turn over a row, 16 lanes' thirteenth"""
    m = R.long_rows_csr()
    n, F = m.shape
    indptr, indices, values = dev(m.indptr.astype(np.int64)), dev(m.indices.astype(np.int32)), dev(m.data)
    out = nan(n, F)
    N.call("trec_csr_to_dense", N.ptr(indptr), N.ptr(indices), N.ptr(values), n, F, N.ptr(out))
    torch.cuda.synchronize()
    same(out.cpu().numpy(), m.toarray(), "CSR -> dense")
    for mm in (m, R.dense_csr(203, R.F_SMALL, 0.15, R.SEED)):
        ip, va, rs = dev(mm.indptr.astype(np.int64)), dev(mm.data), nan(mm.shape[0])
        N.call("trec_spmv_csr", N.ptr(ip), None, N.ptr(va), None, mm.shape[0], None, N.ptr(rs))
        torch.cuda.synchronize()
        s, bar = R.segsum_ref(mm.indptr, mm.data)
        within("segment sums", "row sums", rs.cpu().numpy(), s, bar, "%d rows" % mm.shape[0])


@pytest.mark.parametrize("n,d", [(150, 12), (4099, 260), (257, 65)])
def test_colsum(ops, n, d):
    """one slice (fewer than 512 rows), several slices with a ragged last one, d off the 64-column tile"""
    x = R.gradient(n, d, 11)
    s, bar = R.colsum_ref(x)
    within("colsum", "column sums", ops.colsum(dev(x)).cpu().numpy(), s, bar, "%d x %d" % (n, d))


# ------------------------------------------------------------------------------------------------ towers
@pytest.mark.parametrize("name,d", R.TOWER_CASES)
def test_towers(ops, name, d):
    """sparse_dense_matmul_l2norm (gather -> row_l2norm_bwd -> transposed gather) and sparse_dense_matmul_bias_relu (gather -> relu_bwd ->
    transposed gather + colsum): output and gradients of sum g * out against the closed forms in float64"""
    from tensorrec_amd.sparse import SparseFeatures
    m = R.tower_matrix(name)
    n, F = m.shape
    W, b, g = R.weights(F, d, R.TOWER_SEED), R.bias(d, R.TOWER_SEED), R.gradient(n, d, 5)
    feats, tg = SparseFeatures(m, "cuda"), dev(g)
    what = "%s d %d" % (name, d)

    w = dev(W).requires_grad_(True)
    y = ops.sparse_dense_matmul_l2norm(feats, w)
    y.backward(tg)
    ref = R.norm_tower_ref(m, W, g)
    within("normalise tower", "y", y.detach().cpu().numpy(), ref.y, ref.bar_y, what)
    within("normalise tower", "dW", w.grad.cpu().numpy(), ref.dW, ref.bar_dW, what)

    w, tb = dev(W).requires_grad_(True), dev(b).requires_grad_(True)
    out = ops.sparse_dense_matmul_bias_relu(feats, w, tb)
    out.backward(tg)
    ref = R.relu_tower_ref(m, W, b, g)
    same(out.detach().cpu().numpy(), np.maximum(O.spmm_exact(m, W) + b, F32(0)), what + ": ReLU tower output")
    within("ReLU tower", "out", out.detach().cpu().numpy(), ref.out, ref.bar_out, what)
    within("ReLU tower", "dW", w.grad.cpu().numpy(), ref.dW, ref.bar_dW, what)
    within("ReLU tower", "db", tb.grad.cpu().numpy().reshape(-1), ref.db, ref.bar_db, what)
    assert (w.grad.cpu().numpy()[F - R.N_SPECIAL] == 0).all(), what + ": a pre-activation of exactly 0 passed its gradient"
