"""The chunked gathers of csrc/spmm_split.hip against tests/split_reference.py, bit for bit: every instantiation of split_rows_kernel /
split_chunks_kernel<ITERS, PACKED, VEC> (and the val_perm fork) and of split_reduce_kernel<ITERS, VEC>, the SpMV / segment-sum kernels of the
same plan, and the autograd route ops._prefer_split takes (tests/test_split_reference_host.py shows on the CPU that the case list reaches all
of them, every chunk tail 1 .. 8 and the second step of every grid-stride loop, and that the reference tells a wrong order apart).

* out and rowsum equal the reference with np.array_equal (zeros of either sign count as equal); two calls give the same bits; the plain,
  permuted and packed sources give the same bits as each other;
* without accumulate out and rowsum start as NaN: every row, empty ones included, has to be written;
* the workspace is carved out of a larger buffer and filled with 0xFF bytes: nothing may depend on its contents, and the bytes around
  trec_csr_split_workspace_bytes() have to come back untouched;
* a width outside the rule or a workspace one byte short is refused before anything is launched."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import split_reference as R
from k1_reference import F32
from oracle import oracle as O

pytestmark = pytest.mark.gpu

UNSET = -(2 ** 31) + 12345                                    # no tuning holds this value
GUARD_FRONT, GUARD_BACK = 256, 4096
TREC_ERR_INVALID = 1


@pytest.fixture(scope="module")
def ops():
    from tensorrec_amd import ops as _ops, _native
    _native.require_gpu()
    _native.load()
    return _ops


@pytest.fixture(scope="module")
def N(ops):
    from tensorrec_amd import _native
    return _native


class split_t(object):
    """``with split_t(N, 16):`` -- the threshold through _native.set_tuning, put back on exit (cleared again if it was not set)"""

    def __init__(self, N, value):
        assert value >= 2
        self.N, self.value = N, value

    def __enter__(self):
        self.before = self.N.load().trec_get_tuning(b"split_t", UNSET)
        self.N.set_tuning("split_t", self.value)
        return self

    def __exit__(self, *exc):
        if self.before == UNSET:
            self.N.clear_tuning("split_t")
        else:
            self.N.set_tuning("split_t", self.before)
        return False


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if not np.array_equal(got, want):
        bad = got != want
        rows = np.unique(np.argwhere(bad)[:, 0])
        raise AssertionError("%s: %d of %d elements differ in %d rows (first rows %r), first at %r: got %r, want %r (%d not written)" % (
            what, int(bad.sum()), got.size, rows.size, rows[:8].tolist(), tuple(np.argwhere(bad)[0]), got[bad][0], want[bad][0],
            int(np.isnan(got).sum())))


class Workspace(object):
    """trec_csr_split_workspace_bytes() bytes inside a larger buffer, everything 0xFF"""

    def __init__(self, N, nnz, d):
        self.nbytes = int(N.query("trec_csr_split_workspace_bytes", int(nnz), int(d)))
        assert self.nbytes > 0
        self.buf = torch.full((GUARD_FRONT + self.nbytes + GUARD_BACK,), 0xFF, dtype=torch.uint8, device="cuda")
        self.ws = self.buf[GUARD_FRONT:GUARD_FRONT + self.nbytes]
        assert self.ws.data_ptr() % 16 == 0

    def guards_intact(self):
        return bool((self.buf[:GUARD_FRONT] == 0xFF).all()) and bool((self.buf[GUARD_FRONT + self.nbytes:] == 0xFF).all())

    def untouched(self):
        return bool((self.buf == 0xFF).all())


def upload(m):
    store, perm = R.perm_values(m)
    return dict(indptr=dev(m.indptr.astype(np.int64)), indices=dev(m.indices.astype(np.int32)), values=dev(m.data.astype(F32)),
                store=dev(store), perm=dev(perm), packed=dev(R.packed_entries(m)))


def source_args(N, t, source):
    """(indices, values, val_perm, packed_entries) of a source"""
    if source == "packed":
        return None, None, None, N.ptr(t["packed"])
    if source == "perm":
        return N.ptr(t["indices"]), N.ptr(t["store"]), N.ptr(t["perm"]), None
    return N.ptr(t["indices"]), N.ptr(t["values"]), None, None


def run_gather(N, case, x, t, l):
    """one launch of the case; (out, rowsum or None) on the host"""
    n, d, nnz = x.m.shape[0], case.d, x.m.nnz
    out = dev(x.base) if l.accumulate else nan(n, d)
    rs = None if not l.rowsum else (dev(x.base_rowsum) if l.accumulate else nan(n))
    ws = Workspace(N, nnz, d)
    assert ws.nbytes == R.workspace_bytes(nnz, d, case.split_t)
    indices, values, perm, packed = source_args(N, t, l.source)
    N.call("trec_spmm_csr_split", N.ptr(t["indptr"]), indices, values, perm, packed, n, nnz, N.ptr(t["W"]), d,
           N.ptr(t["own"]) if l.own else None, 1 if l.accumulate else 0, N.ptr(out), N.ptr(rs), N.ptr(ws.ws), ws.nbytes)
    torch.cuda.synchronize()
    assert ws.guards_intact(), "%s %s: bytes outside the workspace were written" % (case.id, l.name)
    return out.cpu().numpy(), None if rs is None else rs.cpu().numpy()


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_split_gather_equals_the_chunk_chain_reference(ops, N, case):
    x = R.case_inputs(case)
    t = upload(x.m)
    t.update(W=dev(x.W), own=dev(x.own))
    by_option = {}
    with split_t(N, case.split_t):
        for l in case.launches:
            packed, perm = R.SOURCES[l.source]
            assert R.pick_split(case.d, packed, perm) in R.ALL_SPLIT_KERNELS
            want, want_rs = R.expected(case.id, l.own, l.accumulate)
            what = "%s %s %r" % (case.id, l.name, R.pick_split(case.d, packed, perm))
            got, rs = run_gather(N, case, x, t, l)
            same(got, want, what + ": out is not the chunk chains added in chunk order")
            if l.rowsum:
                same(rs, want_rs, what + ": rowsum")
            again, rs2 = run_gather(N, case, x, t, l)
            same(again, got, what + ": two calls differ")
            if l.rowsum:
                same(rs2, rs, what + ": two calls differ in rowsum")
            first = by_option.setdefault((l.own, l.accumulate, l.rowsum), (l.name, got, rs))
            same(got, first[1], "%s: %s and %s differ" % (case.id, l.name, first[0]))
            if l.rowsum:
                same(rs, first[2], "%s: %s and %s differ in rowsum" % (case.id, l.name, first[0]))
    empty = np.diff(x.m.indptr) == 0
    if case.group != "stride":
        assert empty.any() and (R.expected(case.id, False, False)[0][empty] == 0).all()


def test_split_entry_refuses_bad_widths_and_a_short_workspace(ops, N):
    """d = 0, 257, 1028 and a workspace one byte short: TREC_ERR_INVALID, out and the workspace as they were"""
    m = R.lens_csr(R.LENS16, R.N_COLS16, 16)
    t = upload(m)
    lib = N.load()
    n, nnz = m.shape[0], m.nnz
    W = nan(R.N_COLS16, 1028)
    with split_t(N, 16):
        for d, short_by in ((0, 0), (257, 0), (1028, 0), (12, 1), (65, 1)):
            assert R.accepts(d) == bool(short_by)
            ws = Workspace(N, nnz, max(d, 1))
            out, rs = nan(n, max(d, 1)), nan(n)
            rc = lib.trec_spmm_csr_split(N.ptr(t["indptr"]), N.ptr(t["indices"]), N.ptr(t["values"]), None, None, n, nnz, N.ptr(W), d, None, 0,
                                         N.ptr(out), N.ptr(rs), N.ptr(ws.ws), ws.nbytes - short_by, N.stream())
            torch.cuda.synchronize()
            assert rc == TREC_ERR_INVALID and lib.trec_last_error(), d
            assert bool(torch.isnan(out).all()) and bool(torch.isnan(rs).all()) and ws.untouched(), d
        ws = Workspace(N, nnz, 1)
        out = nan(n)
        rc = lib.trec_spmv_csr_split(N.ptr(t["indptr"]), N.ptr(t["indices"]), N.ptr(t["values"]), None, n, nnz, None, N.ptr(out), N.ptr(ws.ws),
                                     ws.nbytes - 1, N.stream())
        torch.cuda.synchronize()
        assert rc == TREC_ERR_INVALID and bool(torch.isnan(out).all()) and ws.untouched()


@pytest.mark.parametrize("case", R.SPMV_CASES, ids=lambda c: c.id)
def test_split_spmv_equals_the_lane_and_butterfly_reference(ops, N, case):
    m = case.matrix()
    n, nnz = m.shape[0], m.nnz
    t = upload(m)
    beta = dev(R.beta_of(m.shape[1]))
    short = np.diff(m.indptr) <= case.split_t
    with split_t(N, case.split_t):
        for with_beta in (True, False):
            want = R.expected_spmv(case.id, with_beta)
            b = N.ptr(beta) if with_beta else None
            results = []
            for values, perm in ((t["values"], None), (t["store"], t["perm"]), (t["values"], None)):
                ws = Workspace(N, nnz, 1)
                out = nan(n)
                N.call("trec_spmv_csr_split", N.ptr(t["indptr"]), N.ptr(t["indices"]), N.ptr(values), N.ptr(perm), n, nnz, b, N.ptr(out),
                       N.ptr(ws.ws), ws.nbytes)
                torch.cuda.synchronize()
                assert ws.guards_intact()
                results.append(out.cpu().numpy())
                same(results[-1], want, "%s beta %d perm %d" % (case.id, with_beta, perm is not None))
            plain = nan(n)
            N.call("trec_spmv_csr", N.ptr(t["indptr"]), N.ptr(t["indices"]), N.ptr(t["values"]), None, n, b, N.ptr(plain))
            torch.cuda.synchronize()
            assert short.any() or case.id.startswith("stride")                                       # (the stride matrices hold long rows only)
            assert np.array_equal(results[0][short], plain.cpu().numpy()[short])                     # the same chains as trec_spmv_csr


def test_prefer_split_route_through_autograd(ops, N):
    """d = 70 (two iterations of single-column lanes, values through val_perm), 69,120 non-zeros and no long column: dW of
    sparse_dense_matmul comes from trec_spmm_csr_split on the transposed CSR and is its chain, bit for bit"""
    from tensorrec_amd.sparse import SparseFeatures
    n, f, d = 3000, 64, 70
    m = sp.random(n, f, density=0.36, random_state=7, dtype=np.float32, format="csr")
    m.data[:] = np.sign(m.data - 0.5) * (0.05 + m.data)
    m.sort_indices()
    feats = SparseFeatures(m, "cuda")
    assert feats.nnz >= 65536 and feats.max_col_nnz <= ops.SPLIT_T and ops._prefer_split(d, feats.nnz)
    assert R.pick_split(d, perm=True) == (2, False, 1, True)
    g = R.rows_f32(n, d, 5)
    w = dev(R.weights(f, d)).requires_grad_(True)
    out = ops.sparse_dense_matmul(feats, w)
    ops.KERNEL_EVENTS = []
    try:
        out.backward(dev(g))
        names = {name for name, _, _ in ops.KERNEL_EVENTS}
    finally:
        ops.KERNEL_EVENTS = None
    assert "spmm_csr_split" in names, names
    t = sp.csr_matrix(m.T)
    t.sort_indices()
    want, _ = R.split_gather_ref(t.indptr, t.indices, t.data, g, R.SPLIT_T_DEFAULT)
    same(w.grad.cpu().numpy(), want, "dW through _prefer_split")
    assert np.array_equal(want, O.spmm_exact(t, g))
    same(out.detach().cpu().numpy(), O.spmm_exact(m, R.weights(f, d)), "the forward gather")
