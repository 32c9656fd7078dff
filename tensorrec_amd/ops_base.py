"""
ops_base -- the kernels of the path that are NOT the user x item contraction: K1 (sparse features x weights, its backward and
epilogues), the fp32 MFMA GEMM, K3 pair scores, the device grouping of pair lists by item, K9 mixture of tastes, K6 losses (WMRB
fused and unfused, RMSE, dense / separation), K4 ranks of a score slab, K7 sampler, K8 Adam.  Thin autograd wrappers over
libtensorrec_hip.so (tensorrec_amd/_native.py); the public module is tensorrec_amd.ops, which re-exports everything here.
"""
from __future__ import annotations

import math

import torch

from . import _native as N
from .sparse import SparseFeatures, Interactions, PairIndex

DTYPE_F32, DTYPE_BF16 = 0, 1

# bench.py sets this to a list to collect (start, end) HIP events around every launch of the named kernels on the
# launching stream (the kernels run on torch's current stream, so torch.cuda.Event brackets exactly them)
KERNEL_EVENTS = None


class _timed(object):
    """Brackets a launch (or a group of launches) with HIP events; brackets nested inside another one are not recorded,
    so a composite step (e.g. the exact fallback of the filtered top-k) does not pollute its inner kernels' statistics."""
    depth = 0

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.on = KERNEL_EVENTS is not None and _timed.depth == 0
        _timed.depth += 1
        if self.on:
            self.s = torch.cuda.Event(enable_timing=True)
            self.e = torch.cuda.Event(enable_timing=True)
            self.s.record()
        return self

    def __exit__(self, *exc):
        _timed.depth -= 1
        if self.on and KERNEL_EVENTS is not None:
            self.e.record()
            KERNEL_EVENTS.append((self.name, self.s, self.e))
        return False
MODE_DOT, MODE_EUCLIDEAN = 0, 1
EPI_NONE, EPI_L2NORM, EPI_BIAS_RELU, EPI_ROWSUM = 0, 1, 2, 3


def _f32c(t):
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


# ------------------------------------------------------------------------------------------------ K1
def spmm_raw(indptr, indices, values, perm, n_rows, nnz, w, col_bias=None, epilogue=EPI_NONE, accumulate=False,
             out=None, want_inv=False, one_per_row=False):
    w = _f32c(w)
    d = w.shape[1]
    if out is None:
        out = torch.empty((n_rows, d), dtype=torch.float32, device=w.device)
    if one_per_row and perm is None and epilogue == EPI_NONE and not accumulate and not want_inv and d % 4 == 0 \
            and d <= 1024 and nnz == n_rows and N.load().trec_get_tuning(b"spmm_one_per_row", 1):
        # identity / indicator features (SparseFeatures.one_per_row): the row pointer is the identity and is not read
        with _timed("spmm_csr"):
            N.call("trec_spmm_one_per_row", N.ptr(indices), N.ptr(values), n_rows, N.ptr(w), d, N.ptr(out))
        return out
    inv = torch.empty((n_rows,), dtype=torch.float32, device=w.device) if want_inv else None
    with _timed("spmm_csr"):
        N.call("trec_spmm_csr", N.ptr(indptr), N.ptr(indices), N.ptr(values), N.ptr(perm), n_rows, nnz, N.ptr(w), d,
               N.ptr(col_bias), epilogue, 1 if accumulate else 0, N.ptr(out), N.ptr(inv))
    return (out, inv) if want_inv else out


# rows longer than this are cut into chunks by the split gathers (csrc/spmm_split.hip: SPLIT_T_DEFAULT)
SPLIT_T = 2048
# uniform samples: a bucket of mean m holds at most ~m + 4.5 sqrt(m) pairs; above this mean some bucket passes SPLIT_T
_SPLIT_MEAN = 1700


def _split_workspace(nnz, d, dev):
    nbytes = N.query("trec_csr_split_workspace_bytes", int(nnz), int(d))
    if nbytes < 0:
        raise ValueError("split gather: no workspace for nnz=%d, d=%d (the tuning split_t must be at least 2)" % (nnz, d))
    return torch.empty((nbytes,), dtype=torch.uint8, device=dev), nbytes


def spmm_split(indptr, indices, values, perm, n_rows, nnz, w, own=None, accumulate=False, out=None, want_rowsum=False,
               packed=None):
    """K1 for skewed row lengths (trec_spmm_csr_split): rows of more than SPLIT_T non-zeros are summed as chunks by the
    whole chip; ``own``: gather (own[row] - w[col]) -- the Euclidean pair gradient."""
    w = _f32c(w)
    d = w.shape[1]
    if out is None:
        out = torch.empty((n_rows, d), dtype=torch.float32, device=w.device)
    rowsum = torch.empty((n_rows,), dtype=torch.float32, device=w.device) if want_rowsum is True else \
        (want_rowsum if isinstance(want_rowsum, torch.Tensor) else None)
    ws, nbytes = _split_workspace(nnz, d, w.device)
    own = _f32c(own) if own is not None else None
    with _timed("spmm_csr_split"):
        N.call("trec_spmm_csr_split", N.ptr(indptr), N.ptr(indices), N.ptr(values), N.ptr(perm), N.ptr(packed), n_rows,
               nnz, N.ptr(w), d, N.ptr(own), 1 if accumulate else 0, N.ptr(out), N.ptr(rowsum), N.ptr(ws), nbytes)
    return (out, rowsum) if want_rowsum is True else out


def spmv_raw(indptr, indices, values, perm, n_rows, nnz, beta, long_rows=False):
    """out[r] = sum_j values[j] * beta[indices[j]] (beta None: plain segment sums); ``long_rows``: some row may exceed
    SPLIT_T non-zeros -> the chunked form."""
    out = torch.empty((n_rows,), dtype=torch.float32, device=indptr.device)
    if long_rows:
        ws, nbytes = _split_workspace(nnz, 1, indptr.device)
        N.call("trec_spmv_csr_split", N.ptr(indptr), N.ptr(indices), N.ptr(values), N.ptr(perm), n_rows, nnz,
               N.ptr(beta), N.ptr(out), N.ptr(ws), nbytes)
    else:
        N.call("trec_spmv_csr", N.ptr(indptr), N.ptr(indices), N.ptr(values), N.ptr(perm), n_rows, N.ptr(beta),
               N.ptr(out))
    return out


def _split_ok(d):
    """widths the chunked gathers cover: float4 lanes up to 1024 columns, single-column lanes (any d) up to 256"""
    return (d % 4 == 0 and d <= 1024) or d <= 256


def _prefer_split(d, nnz):
    """d % 4 != 0 has no float4 kernel: K1's fallback walks a row with one load in flight per thread, the chunked form
    keeps four -- worth its three extra launches on large gathers"""
    return d % 4 != 0 and d <= 256 and nnz >= 65536


def _sampled_buckets_long(n_pairs, n_items):
    """pairs grouped by sampled item on the device: bucket sizes are not known to the host.  Uniform samples stay under
    SPLIT_T up to a mean of _SPLIT_MEAN; large problems take the split form regardless (three small extra launches) so
    that a skewed custom sampler does not serialise on its popular items."""
    return n_pairs >= (1 << 20) or n_pairs > n_items * _SPLIT_MEAN


def _spmm_t(feats: SparseFeatures, dout):
    """dW[F, d] = X^T . dOut -- the same gather kernel on the transposed CSR (chunked where a feature column is long:
    indicator columns of side features hold thousands of rows)."""
    indptr_t, rows_t, perm_t = feats.transposed()
    d = dout.shape[1]
    if (feats.max_col_nnz > SPLIT_T or _prefer_split(d, feats.nnz)) and _split_ok(d):
        return spmm_split(indptr_t, rows_t, feats.values, perm_t, feats.shape[1], feats.nnz, dout)
    return spmm_raw(indptr_t, rows_t, feats.values, perm_t, feats.shape[1], feats.nnz, dout)


class _SpMM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w, feats):
        ctx.feats = feats
        return spmm_raw(feats.indptr, feats.indices, feats.values, None, feats.shape[0], feats.nnz, w,
                        one_per_row=getattr(feats, 'one_per_row', False))

    @staticmethod
    def backward(ctx, dout):
        return _spmm_t(ctx.feats, _f32c(dout)), None


class _SpMMNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w, feats):
        y, inv = spmm_raw(feats.indptr, feats.indices, feats.values, None, feats.shape[0], feats.nnz, w,
                          epilogue=EPI_L2NORM, want_inv=True)
        ctx.feats = feats
        ctx.save_for_backward(y, inv)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, inv = ctx.saved_tensors
        dx = torch.empty_like(y)
        N.call("trec_row_l2norm_bwd", N.ptr(y), N.ptr(inv), N.ptr(_f32c(dy)), y.shape[0], y.shape[1], N.ptr(dx))
        return _spmm_t(ctx.feats, dx), None


class _SpMMBiasRelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w, bias, feats):
        b = _f32c(bias).reshape(-1)
        out = spmm_raw(feats.indptr, feats.indices, feats.values, None, feats.shape[0], feats.nnz, w, col_bias=b,
                       epilogue=EPI_BIAS_RELU)
        ctx.feats = feats
        ctx.bias_shape = bias.shape
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, dout):
        (out,) = ctx.saved_tensors
        dpre = torch.empty_like(out)
        N.call("trec_relu_bwd", N.ptr(out), N.ptr(_f32c(dout)), out.numel(), N.ptr(dpre))
        return _spmm_t(ctx.feats, dpre), colsum(dpre).reshape(ctx.bias_shape), None


def colsum(x):
    """Column sums of a [n_rows, d] matrix (gradient of a broadcast bias): row slices in parallel, added in slice order."""
    x = _f32c(x)
    n_rows, d = x.shape
    out = torch.empty((d,), dtype=torch.float32, device=x.device)
    n_slices = max(1, min(512, n_rows // 256))
    ws = torch.empty((n_slices, d), dtype=torch.float32, device=x.device) if n_slices > 1 else None
    with _timed("colsum"):
        N.call("trec_colsum", N.ptr(x), n_rows, d, N.ptr(out), N.ptr(ws), n_slices)
    return out


def _note_row_support(w, feats):
    """A trainable table multiplied with a sparse feature matrix receives gradient only in the rows that matrix has columns
    for.  The table remembers WHICH matrices it met this fit call (``w._trec_feats``); the data-parallel fit turns them into
    the rows this rank can touch and skips the gradient exchange of tables whose row supports are rank-disjoint
    (TensorRec._dp_make_plan, sharding.plan_gradient_exchange).  Any other use of a table leaves it unmarked: its gradient is
    exchanged in full."""
    if isinstance(w, torch.Tensor) and w.requires_grad and w.is_leaf:
        met = getattr(w, "_trec_feats", None)
        if met is None:
            met = w._trec_feats = set()
        met.add(id(feats))


def sparse_dense_matmul(feats: SparseFeatures, w):
    """tf.sparse_tensor_dense_matmul(features, w)"""
    _note_row_support(w, feats)
    if getattr(feats, "is_identity", False) and w.dim() == 2 and w.shape[0] == feats.shape[1] and w.dtype == torch.float32 \
            and w.is_contiguous() and N.load().trec_get_tuning(b"identity_alias", 1) != 0:
        # identity features: the product IS the table (1.0 * w + 0 exactly).  A view, not a copy: 0.33 ms of K1 forward and
        # 0.46 ms of its gather-copy backward per epoch of the 1M x 1M fit; the gradient of the view is the table's gradient
        out = w.view(w.shape)
        out._trec_alias_of = w
        return out
    return _SpMM.apply(w, feats)


def accumulate_grads(tensors, grads):
    """torch.autograd.backward(tensors, grads) for the hand-made gradients of the fused steps -- except that a tensor which is
    a plain alias of a leaf table (identity features, sparse_dense_matmul) hands its gradient to the table directly:
    AccumulateGrad would clone it (the caller still holds a reference), 512 MB per side at 1M x 128."""
    rest_t, rest_g = [], []
    for t, g in zip(tensors, grads):
        if g is None or not t.requires_grad:
            continue
        leaf = getattr(t, "_trec_alias_of", None)
        if leaf is not None and leaf.is_leaf and leaf.grad is None and g.shape == leaf.shape and g.dtype == leaf.dtype:
            leaf.grad = g
        else:
            rest_t.append(t)
            rest_g.append(g)
    if rest_t:
        torch.autograd.backward(rest_t, rest_g)


def sparse_dense_matmul_l2norm(feats, w):
    _note_row_support(w, feats)
    return _SpMMNorm.apply(w, feats)


def sparse_dense_matmul_bias_relu(feats, w, bias):
    _note_row_support(w, feats)
    return _SpMMBiasRelu.apply(w, bias, feats)


class _SpMV(torch.autograd.Function):
    @staticmethod
    def forward(ctx, beta, feats):
        ctx.feats = feats
        ctx.beta_shape = beta.shape
        return spmv_raw(feats.indptr, feats.indices, feats.values, None, feats.shape[0], feats.nnz,
                        _f32c(beta).reshape(-1), feats.max_row_nnz > SPLIT_T)

    @staticmethod
    def backward(ctx, dout):
        feats = ctx.feats
        indptr_t, rows_t, perm_t = feats.transposed()
        dbeta = spmv_raw(indptr_t, rows_t, feats.values, perm_t, feats.shape[1], feats.nnz, _f32c(dout),
                         feats.max_col_nnz > SPLIT_T)
        return dbeta.reshape(ctx.beta_shape), None


def sparse_matvec(feats, beta):
    _note_row_support(beta, feats)
    return _SpMV.apply(beta, feats)


def sparse_to_dense(feats: SparseFeatures):
    out = torch.empty(feats.shape, dtype=torch.float32, device=feats.device)
    N.call("trec_csr_to_dense", N.ptr(feats.indptr), N.ptr(feats.indices), N.ptr(feats.values), feats.shape[0],
           feats.shape[1], N.ptr(out))
    return out


class _RowL2Norm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _f32c(x)
        y = torch.empty_like(x)
        inv = torch.empty((x.shape[0],), dtype=torch.float32, device=x.device)
        N.call("trec_row_l2norm_fwd", N.ptr(x), x.shape[0], x.shape[1], N.ptr(y), N.ptr(inv))
        ctx.save_for_backward(y, inv)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, inv = ctx.saved_tensors
        dx = torch.empty_like(y)
        N.call("trec_row_l2norm_bwd", N.ptr(y), N.ptr(inv), N.ptr(_f32c(dy)), y.shape[0], y.shape[1], N.ptr(dx))
        return dx


def l2_normalize_rows(x):
    """tf.nn.l2_normalize(x, 1)"""
    return _RowL2Norm.apply(x)


def gemm_raw(a, b, trans_a=False, trans_b=False, split_bf16=False, a_colsum=False):
    """fp32 C = op(a) . op(b).  ``split_bf16``: both operands as two bf16 terms on bf16 MFMA (three products, fp32 accumulation:
    ~1e-5 relative to the product) -- for gradients held to 1e-4 whose products are not much larger than the gradient itself,
    never for a value the oracle's fmaf chain is compared with.  ``a_colsum`` (with
    split_bf16 and trans_a): also returns the column sums of the stored ``a`` -- (C, colsum) -- taken while ``a`` is staged."""
    a, b = _f32c(a), _f32c(b)
    m = a.shape[1] if trans_a else a.shape[0]
    k = a.shape[0] if trans_a else a.shape[1]
    n = b.shape[0] if trans_b else b.shape[1]
    c = torch.empty((m, n), dtype=torch.float32, device=a.device)
    # few output tiles and a long K (dW2 = Relu^T . dOut: [relu_size, n_components] over all users): split K so that the
    # launch has ~1024 workgroups; the slices are added in order (deterministic)
    tiles = ((m + 127) // 128) * ((n + 127) // 128)
    splits = max(1, min(1024 // max(tiles, 1), k // 512)) if tiles < 512 else 1
    ws = torch.empty((splits, m, n), dtype=torch.float32, device=a.device) if splits > 1 else None
    if split_bf16:
        k_per = -(-(-(-k // splits)) // 64) * 64                           # (the slices the entry point makes: whole 64-wide slabs)
        n_slices = max(1, -(-k // max(k_per, 64)))
        parts = torch.empty((n_slices, m), dtype=torch.float32, device=a.device) if (a_colsum and trans_a) else None
        N.call("trec_gemm_f32_split_bf16", 1 if trans_a else 0, 1 if trans_b else 0, m, n, k, N.ptr(a), a.shape[1], N.ptr(b),
               b.shape[1], N.ptr(c), n, 0, N.ptr(ws), splits, N.ptr(parts))
        if a_colsum:
            return c, (parts.sum(dim=0) if parts is not None else colsum(a))
        return c
    N.call("trec_gemm_f32", 1 if trans_a else 0, 1 if trans_b else 0, m, n, k, N.ptr(a), a.shape[1], N.ptr(b),
           b.shape[1], N.ptr(c), n, 0, N.ptr(ws), splits)
    return (c, colsum(a)) if a_colsum else c


class _MatMul(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        return gemm_raw(a, b)

    @staticmethod
    def backward(ctx, dc):
        a, b = ctx.saved_tensors
        dc = _f32c(dc)
        return gemm_raw(dc, b, trans_b=True), gemm_raw(a, dc, trans_a=True)


def matmul(a, b):
    """tf.matmul(a, b) for the dense layer of ReLURepresentationGraph"""
    return _MatMul.apply(a, b)


# ------------------------------------------------------------------------------------------------ K3
def _idx32(x):
    if isinstance(x, PairIndex):
        return x.idx32, x.pairs_per_user
    return x.to(torch.int32).contiguous(), 0


class _PairScore(torch.autograd.Function):
    """Forward: K3.  Backward, for structured pair lists (a user's pairs are consecutive):
      * user side -- pairs are user-major (CSR over users: interactions, or S consecutive samples per user), so
        dU = G . V is the K1 gather kernel with the pair gradients as values: deterministic, no atomics;
      * item side -- dV = G^T . U is the same kernel on the pairs grouped by item: interactions carry that structure,
        sampled pairs (random items) are grouped by a counting sort on the device;
      * Euclidean pairs: the values are c_p = -g_p / sqrt(D_p) (trec_pair_euclid_coef) and every gathered row is
        (own - other), i.e. dU[u] = sum_p c_p (U[u] - V[i_p]), dV[i] = sum_p c_p (V[i] - U[u_p]);
      * rows longer than SPLIT_T pairs (popular items of Zipf-shaped data) are summed as chunks (spmm_split.hip).
    Unstructured index tensors use the atomic kernel for both sides."""

    @staticmethod
    def forward(ctx, u, v, ub, ib, xu32, xi32, pairs_per_user, mode, inter):
        u, v = _f32c(u), _f32c(v)
        n_pairs = xi32.numel()
        out = torch.empty((n_pairs,), dtype=torch.float32, device=u.device)
        # Euclidean pairs keep their squared distances: the backward coefficients -g / sqrt(D) need no second gather
        keep = mode == MODE_EUCLIDEAN and (ctx.needs_input_grad[0] or ctx.needs_input_grad[1])
        sqdist = torch.empty((n_pairs,), dtype=torch.float32, device=u.device) if keep else None
        N.call("trec_pair_score_fwd", N.ptr(u), N.ptr(v), N.ptr(xu32), N.ptr(xi32), n_pairs, pairs_per_user, u.shape[1],
               mode, N.ptr(ub), N.ptr(ib), N.ptr(out), N.ptr(sqdist))
        ctx.sqdist = sqdist
        ctx.stable_grouping = _LOCAL.deterministic_grouping      # (read here: the engine runs backward() on a thread of its own)
        ctx.save_for_backward(u, v)
        ctx.meta = (xu32, xi32, pairs_per_user, mode, ub is not None, ib is not None, inter)
        return out

    @staticmethod
    def backward(ctx, g):
        u, v = ctx.saved_tensors
        xu32, xi32, ppu, mode, has_ub, has_ib, inter = ctx.meta
        g = _f32c(g)
        n_pairs = xi32.numel()
        n_users, n_items, dev = u.shape[0], v.shape[0], u.device
        d = u.shape[1]
        structured = (ppu > 0 or inter is not None) and (mode == MODE_DOT or _split_ok(d))
        if not structured:
            du, dv = torch.zeros_like(u), torch.zeros_like(v)
            dub = torch.zeros((n_users,), dtype=torch.float32, device=dev) if has_ub else None
            dib = torch.zeros((n_items,), dtype=torch.float32, device=dev) if has_ib else None
            N.call("trec_pair_score_bwd", N.ptr(u), N.ptr(v), N.ptr(xu32), N.ptr(xi32), N.ptr(g), n_pairs, ppu,
                   u.shape[1], mode, N.ptr(du), N.ptr(dv), N.ptr(dub), N.ptr(dib))
            return du, dv, dub, dib, None, None, None, None, None
        euclid = mode == MODE_EUCLIDEAN
        vals = g
        if euclid:       # dU[u] = sum_p c_p (U[u] - V[i_p]),  dV[i] = sum_p c_p (V[i] - U[u_p])
            vals = torch.empty_like(g)
            N.call("trec_pair_euclid_coef", N.ptr(u), N.ptr(v), N.ptr(xu32), N.ptr(xi32), N.ptr(g), N.ptr(ctx.sqdist),
                   n_pairs, ppu, d, N.ptr(vals))
        can_split = _split_ok(d)
        prefer = _prefer_split(d, n_pairs)
        # ---- user side: segmented gather over each user's pairs (K1 with values = g)
        if inter is not None:
            indptr_u, long_u = inter.indptr, inter.max_row_nnz > SPLIT_T
        else:
            indptr_u = torch.arange(0, (n_users + 1) * ppu, ppu, dtype=torch.int64, device=dev)
            long_u = ppu > SPLIT_T
        if euclid or ((long_u or prefer) and can_split):
            du = spmm_split(indptr_u, xi32, vals, None, n_users, n_pairs, v, own=u if euclid else None)
        else:
            du = spmm_raw(indptr_u, xi32, vals, None, n_users, n_pairs, v)
        dub = spmv_raw(indptr_u, xi32, g, None, n_users, n_pairs, None, long_u) if has_ub else None
        # ---- item side: interactions carry their transposed structure; sampled pairs (random items, no structure) are
        # grouped by item on the device (counting sort) -- then the same segmented gather instead of n_pairs * d atomics
        if inter is not None:
            indptr_t, users_t, perm_t = inter.transposed()
            long_i = inter.max_col_nnz > SPLIT_T
        else:
            indptr_t, users_t, perm_t = group_pairs_by_item(xu32, xi32, ppu, n_items, stable=ctx.stable_grouping)
            long_i = _sampled_buckets_long(n_pairs, n_items)
        if euclid or ((long_i or prefer) and can_split):
            dv = spmm_split(indptr_t, users_t, vals, perm_t, n_items, n_pairs, u, own=v if euclid else None)
        else:
            dv = spmm_raw(indptr_t, users_t, vals, perm_t, n_items, n_pairs, u)
        dib = spmv_raw(indptr_t, users_t, g, perm_t, n_items, n_pairs, None, long_i) if has_ib else None
        return du, dv, dub, dib, None, None, None, None, None


import threading as _threading


class _Local(_threading.local):
    deterministic_grouping = False
    loss_group = None          # (process group,) while a user-sharded fit step builds its loss: scalar losses span ALL shards


_LOCAL = _Local()       # per THREAD: two models fitting in different threads must not switch each other's grouping mode


class deterministic_grouping(object):
    """``with ops.deterministic_grouping(flag):`` -- group_pairs_by_item uses the stable (bit-reproducible) grouping inside the
    block, in this thread only; the previous mode returns on exit (TensorRec(deterministic=True) wraps its fit calls in it).
    The autograd functions whose backward groups pairs (pair_score, collapse_tastes) read the mode in their FORWARD pass and
    hand it to their backward pass: the autograd engine runs backward() on its own thread, where this thread's mode is not seen."""

    def __init__(self, flag=True):
        self.flag = bool(flag)

    def __enter__(self):
        self.prev = _LOCAL.deterministic_grouping
        _LOCAL.deterministic_grouping = self.flag
        return self

    def __exit__(self, *exc):
        _LOCAL.deterministic_grouping = self.prev
        return False


class scalar_loss_group(object):
    """``with ops.scalar_loss_group(group):`` -- inside, the scalar losses (RMSE, RMSEDense, Separation, SeparationDense:
    loss_graphs.py:58-134) are those of the UNION of every rank's interactions: their sums are all-reduced over ``group``
    (a collective: every rank of the group must build the same loss) and the backward pass differentiates the global scalar
    with respect to this rank's predictions.  TensorRec's data-parallel step wraps its loss construction in it."""

    def __init__(self, group, active=True):
        self.value = (group,) if active else None

    def __enter__(self):
        self.prev = _LOCAL.loss_group
        _LOCAL.loss_group = self.value
        return self

    def __exit__(self, *exc):
        _LOCAL.loss_group = self.prev
        return False


def _loss_all_reduce(t):
    """SUM over the ranks of the current scalar_loss_group, in place (float64 / float32 device tensor)."""
    import torch.distributed as dist
    dist.all_reduce(t, op=dist.ReduceOp.SUM, group=_LOCAL.loss_group[0])
    return t


def group_pairs_by_item(xu32, xi32, pairs_per_user, n_items, workspace_with_counts=None, ranks=None, values=None, stable=None):
    """(indptr_t int64 [n_items+1], users_t int32 [n_pairs], perm_t int32 [n_pairs]) for a pair list, built on the
    device; the order of pairs inside an item's bucket is not fixed (atomic slot assignment).
    ``workspace_with_counts``: an int32 [2 * n_items] workspace whose first half already holds the histogram of the
    items (counted by the kernel that consumed the pairs) -- the histogram pass is then skipped; ``ranks`` (with it): the
    values those histogram atomics returned, which makes the fill pass atomic-free; ``values`` (with ranks): per-pair
    values to carry along -- the result is then (indptr_t, entries int32 [n_pairs, 2] = {user, value bits}, None): one
    8-byte scattered store per pair, consumed by trec_spmm_csr_packed.  ``stable``: the stable grouping or not; None: this
    thread's ops.deterministic_grouping mode."""
    dev = xi32.device
    n_pairs = xi32.numel()
    if (_LOCAL.deterministic_grouping if stable is None else stable) and n_pairs:
        # bit-reproducible fits (TensorRec(deterministic=True)): a STABLE sort by item keeps the pairs of a bucket in pair
        # order, so the fp32 sums over a bucket are added in the same order every run (the counting sort below orders a
        # bucket by atomic arrival).  Negative keys sort to the front and fall before indptr[0].
        order = torch.sort(xi32, stable=True).indices
        sorted_keys = xi32[order]
        indptr_t = torch.searchsorted(sorted_keys, torch.arange(n_items + 1, dtype=torch.int32, device=dev)).to(torch.int64)
        users = xu32[order] if xu32 is not None else torch.div(order, pairs_per_user, rounding_mode="floor").to(torch.int32)
        if values is not None and ranks is not None:
            entries = torch.stack([users.to(torch.int32), values[order].contiguous().view(torch.int32)], dim=1).contiguous()
            return indptr_t, entries, None
        return indptr_t, users.to(torch.int32).contiguous(), order.to(torch.int32).contiguous()
    n_runs = int(N.query("trec_group_pairs_lds_runs", int(n_pairs), int(n_items))) \
        if workspace_with_counts is None and ranks is None and N.load().trec_get_tuning(b"group_pairs_lds", 1) != 0 else 0
    if n_runs > 0:
        # few buckets, very many pairs (MovieLens-shaped catalogues): counters in LDS, no global atomics (csrc/segment.hip)
        ws32 = torch.empty((n_items,), dtype=torch.int32, device=dev)
        ws64 = torch.empty(((n_items + 1023) // 1024 + 1,), dtype=torch.int64, device=dev)
        run_counts = torch.empty((n_runs, n_items), dtype=torch.int32, device=dev)
        indptr_t = torch.empty((n_items + 1,), dtype=torch.int64, device=dev)
        users_t = torch.empty((n_pairs,), dtype=torch.int32, device=dev)
        perm_t = torch.empty((n_pairs,), dtype=torch.int32, device=dev)
        with _timed("group_pairs_by_item"):
            N.call("trec_group_pairs_by_item_lds", N.ptr(xu32), N.ptr(xi32), n_pairs, pairs_per_user, n_items, N.ptr(ws32),
                   N.ptr(ws64), N.ptr(run_counts), N.ptr(indptr_t), N.ptr(users_t), N.ptr(perm_t))
        return indptr_t, users_t, perm_t
    ws32 = workspace_with_counts if workspace_with_counts is not None else \
        torch.empty((2 * n_items,), dtype=torch.int32, device=dev)
    ws64 = torch.empty(((n_items + 1023) // 1024 + 1,), dtype=torch.int64, device=dev)
    indptr_t = torch.empty((n_items + 1,), dtype=torch.int64, device=dev)
    carry = values is not None and ranks is not None
    users_t = None if carry else torch.empty((n_pairs,), dtype=torch.int32, device=dev)
    if carry:      # packed: entries int2 {user, value bits}, one 8-byte scattered store per pair; (indptr, entries, None)
        entries = torch.empty((n_pairs, 2), dtype=torch.int32, device=dev)
        lib = N.load()
        if workspace_with_counts is not None and lib.trec_get_tuning(b"group_pairs_staged", 1) != 0 and \
                n_pairs >= lib.trec_get_tuning(b"group_pairs_staged_min", 1 << 24):
            # very many pairs: the fill in two levels (csrc/segment.hip) -- appended to the staging region of their destination
            # window first, placed window by window afterwards, instead of 8-byte stores scattered over the whole 800 MB of
            # entries.  Windows of 2^22 entries measured best at 1e8 pairs (fill + scan 3.1 ms against 3.7 in one level; 2^17:
            # 6.0, 2^19: 4.4, 2^21: 3.5, 2^23: 3.5, 2^24: 3.7 -- the staging pass pays per window, the placing pass per entry)
            wlog = int(lib.trec_get_tuning(b"group_pairs_window_log2", 22))
            sbytes = int(N.query("trec_group_pairs_staged_bytes", int(n_pairs), wlog))
            if sbytes > 0:
                staging = torch.empty((sbytes,), dtype=torch.uint8, device=dev)
                with _timed("group_pairs_staged"):
                    N.call("trec_group_pairs_by_item_staged", N.ptr(xu32), N.ptr(xi32), n_pairs, pairs_per_user, n_items,
                           N.ptr(ws32), N.ptr(ws64), N.ptr(indptr_t), N.ptr(entries), N.ptr(ranks), N.ptr(values),
                           N.ptr(staging), sbytes, wlog)
                return indptr_t, entries, None
        N.call("trec_group_pairs_by_item", N.ptr(xu32), N.ptr(xi32), n_pairs, pairs_per_user, n_items, N.ptr(ws32),
               N.ptr(ws64), N.ptr(indptr_t), N.ptr(entries), None, 1, N.ptr(ranks), N.ptr(values), None)
        return indptr_t, entries, None
    perm_t = torch.empty((n_pairs,), dtype=torch.int32, device=dev)
    N.call("trec_group_pairs_by_item", N.ptr(xu32), N.ptr(xi32), n_pairs, pairs_per_user, n_items, N.ptr(ws32),
           N.ptr(ws64), N.ptr(indptr_t), N.ptr(users_t), N.ptr(perm_t), 1 if workspace_with_counts is not None else 0,
           N.ptr(ranks), None, None)
    return indptr_t, users_t, perm_t


_ones_cache = {}


def _ones(n, dev):
    key = (n, str(dev))
    if key not in _ones_cache:
        _ones_cache.clear()
        _ones_cache[key] = torch.ones((n,), dtype=torch.float32, device=dev)
    return _ones_cache[key]


def pair_score(user_repr, item_repr, x_user, x_item, mode=MODE_DOT, user_bias=None, item_bias=None):
    """Serial prediction for (x_user[p], x_item[p]) pairs, optionally fused with the serial bias add."""
    xu32, ppu = _idx32(x_user)
    xi32, _ = _idx32(x_item)
    inter = getattr(x_user, "interactions", None) if isinstance(x_user, PairIndex) else None
    if inter is not None and (getattr(x_item, "interactions", None) is not inter or xi32.numel() != inter.nnz):
        inter = None
    if ppu > 0:
        xu32 = None                      # implicit users: pair p -> p // pairs_per_user
    ub = _f32c(user_bias) if user_bias is not None else None
    ib = _f32c(item_bias) if item_bias is not None else None
    return _PairScore.apply(user_repr, item_repr, ub, ib, xu32, xi32, ppu, mode, inter)


# ------------------------------------------------------------------------------------------------ K9
def _pair_bias_grads(g, xu32, xi32, ppu, inter, n_users, n_items, want_ub, want_ib, stable=None):
    """d user_bias / d item_bias of out[p] = ... + ub[user(p)] + ib[item(p)]: g summed per user / per item with the
    segmented K1 matvec over the pair structure (interactions: CSR + its transpose; samples: ppu consecutive pairs per
    user + a device counting sort by item).  Unstructured pair lists fall back to index_add_."""
    dev = g.device
    n_pairs = xi32.numel()
    dub = dib = None
    if inter is None and ppu <= 0:
        if want_ub:
            dub = torch.zeros((n_users,), dtype=torch.float32, device=dev).index_add_(0, xu32.long(), g)
        if want_ib:
            dib = torch.zeros((n_items,), dtype=torch.float32, device=dev).index_add_(0, xi32.long(), g)
        return dub, dib
    if want_ub:
        indptr_u = inter.indptr if inter is not None else \
            torch.arange(0, (n_users + 1) * ppu, ppu, dtype=torch.int64, device=dev)
        long_u = (inter.max_row_nnz if inter is not None else ppu) > SPLIT_T
        dub = spmv_raw(indptr_u, xi32, g, None, n_users, n_pairs, None, long_u)
    if want_ib:
        indptr_t, users_t, perm_t = inter.transposed() if inter is not None else \
            group_pairs_by_item(xu32, xi32, ppu, n_items, stable=stable)
        long_i = inter.max_col_nnz > SPLIT_T if inter is not None else _sampled_buckets_long(n_pairs, n_items)
        dib = spmv_raw(indptr_t, users_t, g, perm_t, n_items, n_pairs, None, long_i)
    return dub, dib


class _CollapseTastes(torch.autograd.Function):
    """K9 forward / backward; ``meta`` = (bias_mode, xu32, xi32, span, inter)."""

    @staticmethod
    def forward(ctx, preds, attn, ub, ib, meta):
        bias_mode, xu32, xi32, span, inter = meta
        preds = _f32c(preds)
        attn = _f32c(attn) if attn is not None else None
        T = preds.shape[0]
        n = preds[0].numel()
        out = torch.empty(preds.shape[1:], dtype=torch.float32, device=preds.device)
        N.call("trec_collapse_tastes_fwd", N.ptr(preds), N.ptr(attn), T, n, bias_mode, N.ptr(ub), N.ptr(ib),
               N.ptr(xu32), N.ptr(xi32), span, N.ptr(out))
        ctx.save_for_backward(preds, attn)
        ctx.meta = meta
        ctx.bias_shapes = (None if ub is None else ub.numel(), None if ib is None else ib.numel())
        ctx.stable_grouping = _LOCAL.deterministic_grouping      # (as _PairScore: backward() runs on the engine's thread)
        return out

    @staticmethod
    def backward(ctx, g):
        preds, attn = ctx.saved_tensors
        bias_mode, xu32, xi32, span, inter = ctx.meta
        n_ub, n_ib = ctx.bias_shapes
        g = _f32c(g)
        T = preds.shape[0]
        n = preds[0].numel()
        d_preds = torch.empty_like(preds)
        d_attn = torch.empty_like(attn) if attn is not None else None
        N.call("trec_collapse_tastes_bwd", N.ptr(preds), N.ptr(attn), N.ptr(g), T, n, N.ptr(d_preds), N.ptr(d_attn))
        dub = dib = None
        if bias_mode == 1 and (n_ub is not None or n_ib is not None):
            ppu = span if xu32 is None else 0
            n_users = inter.shape[0] if inter is not None else (n // ppu if ppu > 0 else (n_ub or 0))
            n_items = inter.shape[1] if inter is not None else (n_ib or 0)
            dub, dib = _pair_bias_grads(g.reshape(-1), xu32, xi32, ppu, inter, n_users, n_items, n_ub is not None,
                                        n_ib is not None, stable=ctx.stable_grouping)
        elif bias_mode == 2:
            g2 = g.reshape(-1, span)
            if n_ub is not None:
                dub = gemm_raw(g2, _ones(span, g.device).reshape(span, 1)).reshape(-1)
            if n_ib is not None:
                dib = colsum(g2)
        return d_preds, d_attn, dub, dib, None


def collapse_tastes(tastes_predictions, tastes_attentions=None, user_bias=None, item_bias=None, x_user=None,
                    x_item=None):
    """collapse_mixture_of_tastes (recommendation_graphs.py:85-109) in one pass (K9), optionally fused with the bias add
    that follows it: serial predictions pass the pair indices, dense [n_users, n_items] predictions pass none."""
    def stacked(x):
        return x if isinstance(x, torch.Tensor) else torch.stack(list(x))

    preds = stacked(tastes_predictions)
    attn = stacked(tastes_attentions) if tastes_attentions is not None else None
    if preds.shape[0] > 16:
        # the collapse kernel holds <= 16 tastes: a maximum is a maximum of group maxima (exact, bias add on the last
        # call only); the attention form (softmax over ALL tastes) is composed from torch ops -- same arithmetic order as
        # recommendation_graphs.py:96-105 (stack, softmax, multiply, reduce_sum), then the bias adds
        if attn is None:
            groups = [collapse_tastes(preds[g:g + 16]) if preds[g:g + 16].shape[0] > 1 else preds[g]
                      for g in range(0, preds.shape[0], 16)]
            return collapse_tastes(torch.stack(groups), None, user_bias, item_bias, x_user, x_item)
        out = (preds * torch.softmax(attn, dim=0)).sum(dim=0)
        if user_bias is None and item_bias is None:
            return out
        if x_item is not None:
            xu, xi = x_user.long(), x_item.long()
            if user_bias is not None:
                out = out + user_bias[xu]
            if item_bias is not None:
                out = out + item_bias[xi]
            return out
        if user_bias is not None:
            out = out + user_bias.reshape(-1, 1)
        if item_bias is not None:
            out = out + item_bias.reshape(1, -1)
        return out
    ub = _f32c(user_bias) if user_bias is not None else None
    ib = _f32c(item_bias) if item_bias is not None else None
    if ub is None and ib is None:
        meta = (0, None, None, 0, None)
    elif x_item is not None:
        xu32, ppu = _idx32(x_user)
        xi32, _ = _idx32(x_item)
        inter = getattr(x_user, "interactions", None) if isinstance(x_user, PairIndex) else None
        if inter is not None and (getattr(x_item, "interactions", None) is not inter or xi32.numel() != inter.nnz):
            inter = None
        if ppu > 0:
            xu32 = None
        meta = (1, xu32, xi32, ppu, inter)
    else:
        if preds.dim() != 3:
            raise ValueError("dense bias add needs [n_tastes, n_users, n_items] predictions")
        meta = (2, None, None, preds.shape[2], None)
    return _CollapseTastes.apply(preds, attn, ub, ib, meta)


# ------------------------------------------------------------------------------------------------ K6
class _WMRB(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred_serial, sample_pred, inter: Interactions, weight):
        pred_serial, sample_pred = _f32c(pred_serial), _f32c(sample_pred)
        n_users, n_items = inter.shape
        S = sample_pred.shape[1]
        loss = torch.empty((inter.n_positive,), dtype=torch.float32, device=pred_serial.device)
        smr = torch.empty_like(loss)
        N.call("trec_wmrb_fwd", N.ptr(inter.indptr), N.ptr(inter.pos_slot), N.ptr(weight), N.ptr(pred_serial),
               N.ptr(sample_pred), n_users, n_items, S, N.ptr(loss), N.ptr(smr))
        ctx.inter, ctx.weight = inter, weight
        ctx.save_for_backward(pred_serial, sample_pred, smr)
        return loss

    @staticmethod
    def backward(ctx, gl):
        pred_serial, sample_pred, smr = ctx.saved_tensors
        inter = ctx.inter
        n_users, n_items = inter.shape
        S = sample_pred.shape[1]
        dp = torch.empty_like(pred_serial)
        ds = torch.empty_like(sample_pred)
        N.call("trec_wmrb_bwd", N.ptr(inter.indptr), N.ptr(inter.pos_slot), N.ptr(ctx.weight), N.ptr(pred_serial),
               N.ptr(sample_pred), N.ptr(smr), N.ptr(_f32c(gl)), n_users, n_items, S, N.ptr(dp), N.ptr(ds))
        return dp, ds, None, None


class _SampledSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred_serial, sample_pred, inter: Interactions, inv_temperature):
        pred_serial, sample_pred = _f32c(pred_serial), _f32c(sample_pred)
        n_users = inter.shape[0]
        S = sample_pred.shape[1]
        loss = torch.empty((inter.n_positive,), dtype=torch.float32, device=pred_serial.device)
        row_max = torch.empty((n_users,), dtype=torch.float32, device=pred_serial.device)
        row_sum = torch.empty_like(row_max)
        N.call("trec_sampled_softmax_fwd", N.ptr(inter.indptr), N.ptr(inter.pos_slot), N.ptr(pred_serial), N.ptr(sample_pred),
               n_users, S, inv_temperature, N.ptr(loss), N.ptr(row_max), N.ptr(row_sum))
        ctx.inter, ctx.inv_temperature = inter, inv_temperature
        ctx.save_for_backward(pred_serial, sample_pred, row_max, row_sum)
        return loss

    @staticmethod
    def backward(ctx, gl):
        pred_serial, sample_pred, row_max, row_sum = ctx.saved_tensors
        inter = ctx.inter
        S = sample_pred.shape[1]
        dp = torch.empty_like(pred_serial)
        ds = torch.empty_like(sample_pred)
        N.call("trec_sampled_softmax_bwd", N.ptr(inter.indptr), N.ptr(inter.pos_slot), N.ptr(pred_serial), N.ptr(sample_pred),
               N.ptr(row_max), N.ptr(row_sum), N.ptr(_f32c(gl)), inter.shape[0], S, ctx.inv_temperature, N.ptr(dp), N.ptr(ds))
        return dp, ds, None, None


class _BPR(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred_serial, sample_pred, inter: Interactions):
        pred_serial, sample_pred = _f32c(pred_serial), _f32c(sample_pred)
        S = sample_pred.shape[1]
        loss = torch.empty((inter.n_positive,), dtype=torch.float32, device=pred_serial.device)
        N.call("trec_bpr_fwd", N.ptr(inter.indptr), N.ptr(inter.pos_slot), N.ptr(pred_serial), N.ptr(sample_pred), inter.shape[0], S,
               N.ptr(loss))
        ctx.inter = inter
        ctx.save_for_backward(pred_serial, sample_pred)
        return loss

    @staticmethod
    def backward(ctx, gl):
        pred_serial, sample_pred = ctx.saved_tensors
        inter = ctx.inter
        S = sample_pred.shape[1]
        dp = torch.empty_like(pred_serial)
        ds = torch.empty_like(sample_pred)
        N.call("trec_bpr_bwd", N.ptr(inter.indptr), N.ptr(inter.pos_slot), N.ptr(pred_serial), N.ptr(sample_pred), N.ptr(_f32c(gl)),
               inter.shape[0], S, N.ptr(dp), N.ptr(ds))
        return dp, ds, None


class _SampledSoftmaxAdjusted(torch.autograd.Function):
    """trec_sampled_softmax_adj_fwd / _bwd: hits removed and / or the logQ correction; ``adj`` = (sample_items, log_q or None,
    log_q_uniform, log_q_correction, remove_hits)"""

    @staticmethod
    def forward(ctx, pred_serial, sample_pred, inter: Interactions, inv_temperature, adj):
        pred_serial, sample_pred = _f32c(pred_serial), _f32c(sample_pred)
        items, log_q, lq_uniform, use_q, no_hits = adj
        n_users, n_items = inter.shape
        S = sample_pred.shape[1]
        loss = torch.empty((inter.n_positive,), dtype=torch.float32, device=pred_serial.device)
        rows = torch.empty((3, n_users), dtype=torch.float32, device=pred_serial.device)
        N.call("trec_sampled_softmax_adj_fwd", N.ptr(inter.indptr), N.ptr(inter.x_item32), N.ptr(inter.pos_slot), N.ptr(pred_serial),
               N.ptr(sample_pred), N.ptr(items), N.ptr(log_q), lq_uniform, n_users, n_items, S, inv_temperature, use_q, no_hits,
               N.ptr(loss), N.ptr(rows[0]), N.ptr(rows[1]), N.ptr(rows[2]))
        ctx.inter, ctx.inv_temperature, ctx.adj = inter, inv_temperature, adj
        ctx.save_for_backward(pred_serial, sample_pred, rows)
        return loss

    @staticmethod
    def backward(ctx, gl):
        pred_serial, sample_pred, rows = ctx.saved_tensors
        inter = ctx.inter
        items, log_q, lq_uniform, use_q, no_hits = ctx.adj
        n_users, n_items = inter.shape
        S = sample_pred.shape[1]
        dp = torch.empty_like(pred_serial)
        ds = torch.empty_like(sample_pred)
        N.call("trec_sampled_softmax_adj_bwd", N.ptr(inter.indptr), N.ptr(inter.x_item32), N.ptr(inter.pos_slot), N.ptr(pred_serial),
               N.ptr(sample_pred), N.ptr(items), N.ptr(log_q), lq_uniform, N.ptr(rows[0]), N.ptr(rows[1]), N.ptr(rows[2]),
               N.ptr(_f32c(gl)), n_users, n_items, S, ctx.inv_temperature, use_q, no_hits, N.ptr(dp), N.ptr(ds))
        return dp, ds, None, None, None


class _BPRAdjusted(torch.autograd.Function):
    """trec_bpr_adj_fwd / _bwd: accidental hits removed"""

    @staticmethod
    def forward(ctx, pred_serial, sample_pred, inter: Interactions, items):
        pred_serial, sample_pred = _f32c(pred_serial), _f32c(sample_pred)
        S = sample_pred.shape[1]
        loss = torch.empty((inter.n_positive,), dtype=torch.float32, device=pred_serial.device)
        N.call("trec_bpr_adj_fwd", N.ptr(inter.indptr), N.ptr(inter.x_item32), N.ptr(inter.pos_slot), N.ptr(pred_serial),
               N.ptr(sample_pred), N.ptr(items), inter.shape[0], S, 1, N.ptr(loss))
        ctx.inter, ctx.items = inter, items
        ctx.save_for_backward(pred_serial, sample_pred)
        return loss

    @staticmethod
    def backward(ctx, gl):
        pred_serial, sample_pred = ctx.saved_tensors
        inter = ctx.inter
        S = sample_pred.shape[1]
        dp = torch.empty_like(pred_serial)
        ds = torch.empty_like(sample_pred)
        N.call("trec_bpr_adj_bwd", N.ptr(inter.indptr), N.ptr(inter.x_item32), N.ptr(inter.pos_slot), N.ptr(pred_serial),
               N.ptr(sample_pred), N.ptr(ctx.items), N.ptr(_f32c(gl)), inter.shape[0], S, 1, N.ptr(dp), N.ptr(ds))
        return dp, ds, None, None


class _WARP(torch.autograd.Function):
    """trec_warp_fwd / _bwd; ``items``: the int32 sample ids when accidental hits are removed, else None"""

    @staticmethod
    def forward(ctx, pred_serial, sample_pred, inter: Interactions, items):
        pred_serial, sample_pred = _f32c(pred_serial), _f32c(sample_pred)
        n_users, n_items = inter.shape
        S = sample_pred.shape[1]
        dev = pred_serial.device
        loss = torch.empty((inter.n_positive,), dtype=torch.float32, device=dev)
        first = torch.empty((pred_serial.numel(),), dtype=torch.int32, device=dev)
        weight = torch.empty((pred_serial.numel(),), dtype=torch.float32, device=dev)
        hits = items is not None
        N.call("trec_warp_fwd", N.ptr(inter.indptr), N.ptr(inter.x_item32) if hits else None, N.ptr(inter.pos_slot), N.ptr(pred_serial),
               N.ptr(sample_pred), N.ptr(items), n_users, n_items, S, 1 if hits else 0, N.ptr(loss), N.ptr(first), N.ptr(weight))
        ctx.inter, ctx.sample_shape = inter, tuple(sample_pred.shape)
        ctx.save_for_backward(first, weight)
        return loss

    @staticmethod
    def backward(ctx, gl):
        first, weight = ctx.saved_tensors
        inter = ctx.inter
        dp = torch.empty_like(weight)
        ds = torch.empty(ctx.sample_shape, dtype=torch.float32, device=weight.device)
        N.call("trec_warp_bwd", N.ptr(inter.indptr), N.ptr(inter.pos_slot), N.ptr(first), N.ptr(weight), N.ptr(_f32c(gl)),
               inter.shape[0], ctx.sample_shape[1], N.ptr(dp), N.ptr(ds))
        return dp, ds, None, None


import os as _os

# sampled pairs from which the rank-free binned grouping replaces histogram atomics + ranked fill (TREC_BINNED_MIN_PAIRS: A/B runs)
LAST_FUSED_STATS = {}          # filled while KERNEL_EVENTS is collecting: sampled pairs / the pairs the item side kept (device scalar)
GROUP_BINNED_MIN_PAIRS = int(_os.environ.get("TREC_BINNED_MIN_PAIRS", 1 << 22))     # (2^22: the kernels' own minimum; one rank of 8 at
                                                                                     # 1M x 1M has 1.25e7 pairs: 3.91 vs 4.10 ms per step)


def step_switch(name):
    """Is the tuning switch ``name`` of the training step on?  (All default on; "softmax_shared" defaults to SOFTMAX_SHARED_DEFAULT,
    "softmax_full" to SOFTMAX_FULL_DEFAULT, "warp_fused" to WARP_FUSED_DEFAULT, "softmax_tiled" to SOFTMAX_TILED_DEFAULT, "bpr_fused" to
    BPR_FUSED_DEFAULT, "softmax_shared_hits" to SOFTMAX_SHARED_HITS_DEFAULT.)"""
    default = {"softmax_shared": SOFTMAX_SHARED_DEFAULT, "softmax_full": SOFTMAX_FULL_DEFAULT, "warp_fused": WARP_FUSED_DEFAULT,
               "softmax_tiled": SOFTMAX_TILED_DEFAULT, "bpr_fused": BPR_FUSED_DEFAULT,
               "softmax_shared_hits": SOFTMAX_SHARED_HITS_DEFAULT}.get(name, 1)
    return N.load().trec_get_tuning(name.encode(), default) != 0


def step_covers(kernel, n_sampled, max_row_nnz, d):
    """Does the one-pass step ``kernel`` ("wmrb_fused", "wmrb_tiled", "softmax_fused", "softmax_tiled", "warp_fused", "bpr_fused", "softmax_shared", "softmax_shared_hits") cover this shape?  The ONE
    statement of the coverage: the native library's shape query (host arithmetic, needs no GPU); step_plan.kernel and the
    ``*_supported`` functions below both ask here."""
    if kernel in ("softmax_shared", "softmax_shared_hits"):     # (the interactions do not restrict it: the positives are O(P) work on
                                                                # K3's scores; the masked instantiations cover what the plain ones do)
        return bool(N.query("trec_softmax_shared_supported", int(n_sampled), int(d)))
    return N.query("trec_%s_lds_bytes" % kernel, int(n_sampled), int(max_row_nnz), int(d)) >= 0


def _step_supported(kernel, n_sampled, interactions, d):
    return step_switch(kernel) and step_covers(kernel, n_sampled, interactions.max_row_nnz, d)


def wmrb_fused_supported(n_sampled, interactions, d):
    """Can the one-pass WMRB step (csrc/wmrb_fused.hip) run this shape, and is tuning ``wmrb_fused`` on?"""
    return _step_supported("wmrb_fused", n_sampled, interactions, d)


def _step_operands(user_in, item_in, user_bias, item_bias):
    """(u, v, ub, ib) of a one-pass step: detached, float32, contiguous; absent biases stay None."""
    return tuple(_f32c(x.detach()) if x is not None else None for x in (user_in, item_in, user_bias, item_bias))


def _checked_temperature(temperature):
    temperature = float(temperature)
    if not (temperature > 0.0 and temperature != float("inf")):
        raise ValueError("temperature must be a finite float > 0, got %r" % (temperature,))
    return temperature


def _checked_log_q(sample_log_q, n_items):
    if sample_log_q.numel() != n_items:
        raise ValueError("sample_log_q has %d entries, the interactions %d items" % (sample_log_q.numel(), n_items))
    return _f32c(sample_log_q).reshape(-1)


def _fused_step_buffers(user_in, item_in, user_bias, item_bias, interactions, samples):
    """What the per-user fused steps start from: the [n_users, n_sampled] table checked, then (u, v, ub, ib) of _step_operands and what
    all three allocate: (loss [P+], pred [P], d_u, d_ub or None, coef_s [U, S], coef_p [P], the int32 sample table, the same flattened,
    _fused_sample_grouping's triple)."""
    if samples.dim() != 2 or samples.shape[0] != interactions.shape[0]:
        raise ValueError("samples must be an [n_users, n_sampled] table")
    u, v, ub, ib = _step_operands(user_in, item_in, user_bias, item_bias)
    n_users, n_items = interactions.shape
    S, dev, nnz = int(samples.shape[1]), u.device, interactions.nnz
    loss = torch.empty((interactions.n_positive,), dtype=torch.float32, device=dev)
    pred = torch.empty((nnz,), dtype=torch.float32, device=dev)
    d_u = torch.empty_like(u)
    d_ub = torch.empty((n_users,), dtype=torch.float32, device=dev) if ub is not None else None
    coef_s = torch.empty((n_users, S), dtype=torch.float32, device=dev)
    coef_p = torch.empty((nnz,), dtype=torch.float32, device=dev)
    samples = samples.to(torch.int32).contiguous()
    xs = samples.reshape(-1)
    return u, v, ub, ib, loss, pred, d_u, d_ub, coef_s, coef_p, samples, xs, _fused_sample_grouping(xs, n_users, n_items, S, dev)


def _fused_sample_grouping(xs, n_users, n_items, S, dev):
    """How the item side of a one-pass fused step groups the sampled pairs: (binned_bytes, ws32, ranks).  Very many sampled pairs: grouped
    by item through a two-level LDS partition that needs no ranks (csrc/segment.hip, "binned") -- the fused kernel then issues no
    histogram atomics at all (ws32 = ranks = None); otherwise the histogram rides in the fused kernel and the ranks its atomics return
    make the fill atomic-free."""
    binned_bytes = 0
    if xs.numel() >= GROUP_BINNED_MIN_PAIRS and not _LOCAL.deterministic_grouping and \
            N.load().trec_get_tuning(b"group_pairs_binned", 1) != 0:
        binned_bytes = int(N.query("trec_group_pairs_binned_bytes", int(xs.numel()), int(n_items)))
    if binned_bytes > 0:
        return binned_bytes, None, None
    ws32 = torch.zeros((2 * n_items,), dtype=torch.int32, device=dev)     # [sample histogram | cursors] of the sort below
    ranks = torch.empty((n_users, S), dtype=torch.int32, device=dev)
    return binned_bytes, ws32, ranks


def _gather_over_items(interactions, coef, u, d_ib, accumulate=False, out=None):
    """d item_in's share of the interactions (nnz >= 1): the per-pair coefficients ``coef`` gathered over the transposed interactions
    (K1), with the row-sum epilogue -- epilogue 3 of K1: d b_i = the per-item sums into ``d_ib`` come out of the same pass -- where
    there is an item bias (d_ib is not None); rows of popular items, above SPLIT_T, are summed as chunks."""
    n_items, nnz = interactions.shape[1], interactions.nnz
    indptr_t, users_t, perm_t = interactions.transposed()
    if interactions.max_col_nnz > SPLIT_T:
        return spmm_split(indptr_t, users_t, coef, perm_t, n_items, nnz, u, accumulate=accumulate, out=out, want_rowsum=d_ib)
    return _spmm_rowsum(indptr_t, users_t, coef, perm_t, n_items, nnz, u, EPI_ROWSUM if d_ib is not None else EPI_NONE, accumulate, out,
                        d_ib)


def _gather_over_users(interactions, coef, v):
    """d user_in's share of the interactions (nnz >= 1): ``coef`` gathered over the interactions (K1), chunked above SPLIT_T."""
    gather = spmm_split if interactions.max_row_nnz > SPLIT_T else spmm_raw
    return gather(interactions.indptr, interactions.x_item32, coef, None, interactions.shape[0], interactions.nnz, v)


def _fused_item_side(u, v, ib, interactions, xs, S, coef_s, coef_p, loss, binned_bytes, ws32, ranks):
    """The item side of a one-pass fused step (wmrb_fused_step, softmax_fused_step, warp_fused_step, bpr_fused_step): d item_in = G^T . user_in over both pair lists,
    d b_i = per-item sums of the coefficients -- the static transposed structure for the interactions, the binned or ranked grouping
    (_fused_sample_grouping) for the samples, the packed K1 gather with the row-sum epilogue.  Returns (d_v, d_ib)."""
    n_users, n_items = interactions.shape
    d = u.shape[1]
    dev = u.device
    nnz = interactions.nnz
    # (MEASURED and dropped, profiles/r05_fit_overlap_ab.txt: the sort on a second stream -- whole, next to the fused kernel with
    # the coefficients read through the pair permutation: 34.4 ms per epoch against 25.7; only its fill, next to the item-side
    # gather of the interactions: 26.2 against 26.1 -- every kernel of this step is bound by the same fabric, an overlapped pair
    # slows down by exactly what it hides)
    d_v = torch.zeros_like(v) if nnz == 0 else None
    d_ib = torch.zeros((n_items,), dtype=torch.float32, device=dev) if ib is not None else None
    epi = EPI_ROWSUM if ib is not None else EPI_NONE
    if nnz:
        d_v = _gather_over_items(interactions, coef_p, u, d_ib)
    split_samples = xs.numel() > n_items * _SPLIT_MEAN
    if binned_bytes > 0:
        ind_s = torch.empty((n_items + 1,), dtype=torch.int64, device=dev)
        entries = torch.empty((xs.numel(), 2), dtype=torch.int32, device=dev)
        bws = torch.empty((binned_bytes,), dtype=torch.uint8, device=dev)
        # a sample whose coefficient is exactly 0 (WMRB: it violates no margin of its user; softmax: an accidental hit, an underflow)
        # adds nothing to its item's gradient: such pairs are left out of the sort and of the item-side gather (the chunked gather
        # below is sized by the pair count: all pairs there)
        drop_zero = 0 if split_samples else int(N.load().trec_get_tuning(b"group_pairs_drop_zero", 1) != 0)
        with _timed("group_pairs_binned"):
            N.call("trec_group_pairs_by_item_binned", None, N.ptr(xs), N.ptr(coef_s.reshape(-1)), int(xs.numel()), S, n_items,
                   drop_zero, N.ptr(bws), binned_bytes, N.ptr(ind_s), N.ptr(entries))
    else:
        ind_s, entries, _ = group_pairs_by_item(None, xs, S, n_items, workspace_with_counts=ws32, ranks=ranks.reshape(-1),
                                                values=coef_s.reshape(-1))
    # which grouping this call took (host-side facts only: parity records and tests assert the route they mean to cover)
    LAST_FUSED_STATS["route"] = "binned" if binned_bytes > 0 else "ranked"
    LAST_FUSED_STATS["drop_zero"] = bool(binned_bytes > 0 and drop_zero)
    if KERNEL_EVENTS is not None:                        # (measurement runs only: how many sampled pairs the item side still sees)
        LAST_FUSED_STATS["sampled_pairs"] = int(xs.numel())
        LAST_FUSED_STATS["sampled_pairs_kept"] = ind_s[-1:].clone()
        LAST_FUSED_STATS["sampled_pairs_with_coefficient_0"] = (coef_s == 0).sum()
        LAST_FUSED_STATS["loss_mean"] = loss.mean()
    if split_samples:                                    # few items: every bucket of samples is long
        spmm_split(ind_s, None, None, None, n_items, xs.numel(), u, accumulate=True, out=d_v, want_rowsum=d_ib,
                   packed=entries)
    else:
        with _timed("spmm_csr"):
            N.call("trec_spmm_csr_packed", N.ptr(ind_s), N.ptr(entries), n_items, N.ptr(u), d, epi, 1, N.ptr(d_v),
                   N.ptr(d_ib))
    return d_v, d_ib


def wmrb_fused_step(user_in, item_in, user_bias, item_bias, interactions, samples, balanced=False):
    """One WMRB / BalancedWMRB step for dot scores on (user_in, item_in), upstream gradient 1 (the trainer minimises
    the SUM of the loss vector): returns (loss [P+], pred_serial [P], d user_in, d item_in, d user_bias, d item_bias).
    The user side -- predictions of the interactions and of the sampled pairs, loss, dU, d b_u -- is one kernel with
    every item row gathered once; the item side groups the per-pair coefficients by item (static transposed structure
    for the interactions, device counting sort for the samples) and runs the segmented K1 gathers / segment sums."""
    u, v, ub, ib, loss, pred, d_u, d_ub, coef_s, coef_p, samples, xs, (binned_bytes, ws32, ranks) = \
        _fused_step_buffers(user_in, item_in, user_bias, item_bias, interactions, samples)
    n_users, n_items = interactions.shape
    S, d = int(samples.shape[1]), u.shape[1]
    weight = interactions.balanced_weight() if balanced else None
    with _timed("wmrb_fused_step"):
        N.call("trec_wmrb_fused_step", N.ptr(u), N.ptr(v), N.ptr(ub), N.ptr(ib), N.ptr(interactions.indptr),
               N.ptr(interactions.x_item32), N.ptr(interactions.pos_slot), N.ptr(weight), N.ptr(samples), n_users,
               n_items, S, d, int(interactions.max_row_nnz), N.ptr(loss), N.ptr(pred), N.ptr(d_u), N.ptr(d_ub),
               N.ptr(coef_s), N.ptr(coef_p), N.ptr(ws32), N.ptr(ranks))
    d_v, d_ib = _fused_item_side(u, v, ib, interactions, xs, S, coef_s, coef_p, loss, binned_bytes, ws32, ranks)
    return loss, pred, d_u, d_v, d_ub, d_ib


def softmax_fused_supported(n_sampled, interactions, d):
    """Can the one-pass sampled-softmax step (csrc/softmax_fused.hip) run this shape, and is tuning ``softmax_fused`` on?"""
    return _step_supported("softmax_fused", n_sampled, interactions, d)


def softmax_fused_step(user_in, item_in, user_bias, item_bias, interactions, samples, temperature, sample_log_q=None,
                       log_q_correction=False, remove_accidental_hits=False):
    """One sampled-softmax step for dot scores on (user_in, item_in), upstream gradient 1: wmrb_fused_step with the loss of
    sampled_softmax_loss (``temperature``, ``sample_log_q``, ``log_q_correction``, ``remove_accidental_hits`` as there).  Returns
    (loss [P+], pred_serial [P], d user_in, d item_in, d user_bias, d item_bias); the item side is wmrb_fused_step's."""
    temperature = _checked_temperature(temperature)
    u, v, ub, ib, loss, pred, d_u, d_ub, coef_s, coef_p, samples, xs, (binned_bytes, ws32, ranks) = \
        _fused_step_buffers(user_in, item_in, user_bias, item_bias, interactions, samples)
    n_users, n_items = interactions.shape
    S, d = int(samples.shape[1]), u.shape[1]
    log_q = _checked_log_q(sample_log_q, n_items) if log_q_correction and sample_log_q is not None else None
    with _timed("softmax_fused_step"):
        N.call("trec_softmax_fused_step", N.ptr(u), N.ptr(v), N.ptr(ub), N.ptr(ib), N.ptr(interactions.indptr),
               N.ptr(interactions.x_item32), N.ptr(interactions.pos_slot), N.ptr(samples), n_users, n_items, S, d,
               int(interactions.max_row_nnz), 1.0 / temperature, N.ptr(log_q), -math.log(n_items), 1 if log_q_correction else 0,
               1 if remove_accidental_hits else 0, N.ptr(loss), N.ptr(pred), N.ptr(d_u), N.ptr(d_ub), N.ptr(coef_s), N.ptr(coef_p),
               N.ptr(ws32), N.ptr(ranks))
    d_v, d_ib = _fused_item_side(u, v, ib, interactions, xs, S, coef_s, coef_p, loss, binned_bytes, ws32, ranks)
    return loss, pred, d_u, d_v, d_ub, d_ib


WARP_FUSED_DEFAULT = 0           # tuning "warp_fused" when nobody set it: the route is opt-in (docs/sampled_losses.md, "The one-pass fused step (WARP)")


def warp_fused_supported(n_sampled, interactions, d):
    """Can the one-pass WARP step (csrc/warp_fused.hip) run this shape, and is tuning ``warp_fused`` on (it defaults to off)?"""
    return _step_supported("warp_fused", n_sampled, interactions, d)


def warp_fused_step(user_in, item_in, user_bias, item_bias, interactions, samples, remove_accidental_hits=False, return_first=False):
    """One WARP step for dot scores on (user_in, item_in), upstream gradient 1: softmax_fused_step with the loss of warp_loss
    (``remove_accidental_hits`` as there; n_items is the interactions').  Returns (loss [P+], pred_serial [P], d user_in, d item_in,
    d user_bias, d item_bias), and with ``return_first`` the int32 [P] first violator of every interaction (-1: none) behind them;
    the item side is wmrb_fused_step's.  A positive moves ONE sample slot: at least S - n_u of a user's S sample coefficients are
    exact zeros, which the binned grouping drops from the item-side gather."""
    u, v, ub, ib, loss, pred, d_u, d_ub, coef_s, coef_p, samples, xs, (binned_bytes, ws32, ranks) = \
        _fused_step_buffers(user_in, item_in, user_bias, item_bias, interactions, samples)
    n_users, n_items = interactions.shape
    S, d = int(samples.shape[1]), u.shape[1]
    first = torch.empty((interactions.nnz,), dtype=torch.int32, device=u.device) if return_first else None
    with _timed("warp_fused_step"):
        N.call("trec_warp_fused_step", N.ptr(u), N.ptr(v), N.ptr(ub), N.ptr(ib), N.ptr(interactions.indptr),
               N.ptr(interactions.x_item32), N.ptr(interactions.pos_slot), N.ptr(samples), n_users, n_items, S, d,
               int(interactions.max_row_nnz), 1 if remove_accidental_hits else 0, N.ptr(loss), N.ptr(pred), N.ptr(d_u), N.ptr(d_ub),
               N.ptr(coef_s), N.ptr(coef_p), N.ptr(first), N.ptr(ws32), N.ptr(ranks))
    d_v, d_ib = _fused_item_side(u, v, ib, interactions, xs, S, coef_s, coef_p, loss, binned_bytes, ws32, ranks)
    out = (loss, pred, d_u, d_v, d_ub, d_ib)
    return out + (first,) if return_first else out


BPR_FUSED_DEFAULT = 0            # tuning "bpr_fused" when nobody set it: the route is opt-in (docs/sampled_losses.md, "The one-pass fused step (BPR)")


def bpr_fused_supported(n_sampled, interactions, d):
    """Can the one-pass BPR step (csrc/bpr_fused.hip) run this shape, and is tuning ``bpr_fused`` on (it defaults to off)?"""
    return _step_supported("bpr_fused", n_sampled, interactions, d)


def bpr_fused_step(user_in, item_in, user_bias, item_bias, interactions, samples, remove_accidental_hits=False):
    """One BPR step for dot scores on (user_in, item_in), upstream gradient 1: warp_fused_step with the loss of bpr_loss
    (``remove_accidental_hits`` as there).  Returns (loss [P+], pred_serial [P], d user_in, d item_in, d user_bias, d item_bias);
    the item side is wmrb_fused_step's.  Every kept sample of a user with a positive has a coefficient > 0 (sigma never reaches 0
    short of underflow): the item side sees all sampled pairs but the hits."""
    u, v, ub, ib, loss, pred, d_u, d_ub, coef_s, coef_p, samples, xs, (binned_bytes, ws32, ranks) = \
        _fused_step_buffers(user_in, item_in, user_bias, item_bias, interactions, samples)
    n_users, n_items = interactions.shape
    S, d = int(samples.shape[1]), u.shape[1]
    with _timed("bpr_fused_step"):
        N.call("trec_bpr_fused_step", N.ptr(u), N.ptr(v), N.ptr(ub), N.ptr(ib), N.ptr(interactions.indptr),
               N.ptr(interactions.x_item32), N.ptr(interactions.pos_slot), N.ptr(samples), n_users, n_items, S, d,
               int(interactions.max_row_nnz), 1 if remove_accidental_hits else 0, N.ptr(loss), N.ptr(pred), N.ptr(d_u), N.ptr(d_ub),
               N.ptr(coef_s), N.ptr(coef_p), N.ptr(ws32), N.ptr(ranks))
    d_v, d_ib = _fused_item_side(u, v, ib, interactions, xs, S, coef_s, coef_p, loss, binned_bytes, ws32, ranks)
    return loss, pred, d_u, d_v, d_ub, d_ib


SOFTMAX_SHARED_DEFAULT = 1       # tuning "softmax_shared" when nobody set it (docs/sampled_losses.md, "Shared negatives": the measurement)
SOFTMAX_SHARED_MAX_D = 128


def _f32r(x):
    """x rounded to float32, as a Python float"""
    import struct
    return struct.unpack("f", struct.pack("f", x))[0]


def softmax_shared_supported(n_sampled, interactions, d):
    """Can the shared-negatives MFMA step (csrc/softmax_shared.hip) run this shape, and is tuning ``softmax_shared`` on?"""
    return _step_supported("softmax_shared", n_sampled, interactions, d)


def _streamed_softmax_positives(name, u, vs, ub, bs, cs, v, ib, interactions, inv_t):
    """What the two streamed softmax steps (``name``: "softmax_shared", "softmax_full") share up to the tiles' gradients: the row
    statistics of the streamed [S, d] operand (vs, bs, cs), then the positives -- K3 scores, the loss and d y_p per interaction, K_u
    per user -- and their gradient over the users on K1's route.  Returns (loss, pred, d_pred, stat_m, t_k, d_u, d_ub)."""
    n_users, S, d, dev, nnz = interactions.shape[0], int(vs.shape[0]), int(u.shape[1]), u.device, interactions.nnz
    loss = torch.empty((interactions.n_positive,), dtype=torch.float32, device=dev)
    pred = torch.empty((nnz,), dtype=torch.float32, device=dev)
    d_pred = torch.empty((nnz,), dtype=torch.float32, device=dev)
    stat_m = torch.empty((n_users,), dtype=torch.float32, device=dev)
    stat_z = torch.empty((n_users,), dtype=torch.float32, device=dev)
    t_k = torch.empty((n_users,), dtype=torch.float32, device=dev)
    d_ub = torch.empty((n_users,), dtype=torch.float32, device=dev) if ub is not None else None
    with _timed(name + "_stats"):
        N.call("trec_softmax_shared_stats", N.ptr(u), N.ptr(vs), N.ptr(ub), N.ptr(bs), N.ptr(cs), n_users, S, d, inv_t,
               N.ptr(stat_m), N.ptr(stat_z))
    if nnz:
        N.call("trec_pair_score_fwd", N.ptr(u), N.ptr(v), N.ptr(interactions.x_user32), N.ptr(interactions.x_item32), nnz, 0, d,
               MODE_DOT, N.ptr(ub), N.ptr(ib), N.ptr(pred), None)
    N.call("trec_%s_positives" % name, N.ptr(interactions.indptr), N.ptr(interactions.pos_slot), N.ptr(pred), N.ptr(stat_m),
           N.ptr(stat_z), n_users, inv_t, N.ptr(loss), N.ptr(d_pred), N.ptr(t_k), N.ptr(d_ub))
    d_u = _gather_over_users(interactions, d_pred, v) if nnz else torch.zeros_like(u)
    return loss, pred, d_pred, stat_m, t_k, d_u, d_ub


def softmax_shared_step(user_in, item_in, user_bias, item_bias, interactions, samples, temperature, sample_log_q=None,
                        log_q_correction=False):
    """One sampled-softmax step for dot scores on (user_in, item_in) whose ``samples`` -- int32 [S] -- are shared by every user: the
    step softmax_fused_step would make of the [n_users, S] table that repeats them, accidental hits kept, upstream gradient 1.
    Returns (loss [P+], pred_serial [P], d user_in, d item_in, d user_bias, d item_bias).  The [U, S] logits exist only as MFMA
    tiles: row statistics, then the positives (K3 scores, O(P)), then the samples' gradients in both directions; the [S, d] sample
    gradient reaches d item_in through a stable sort of the ids (duplicates are added in slot order).  Nothing is read on the host."""
    temperature = _checked_temperature(temperature)
    u, v, ub, ib = _step_operands(user_in, item_in, user_bias, item_bias)
    n_users, n_items = interactions.shape
    if samples.dim() != 1 or samples.numel() < 1:
        raise ValueError("samples must be a vector of n_sampled >= 1 item ids")
    S, d, dev, nnz = int(samples.numel()), int(u.shape[1]), u.device, interactions.nnz
    if not step_covers("softmax_shared", S, 0, d):
        raise ValueError("softmax_shared_step covers d %% 4 == 0, 4 <= d <= %d; got d = %d" % (SOFTMAX_SHARED_MAX_D, d))
    inv_t = 1.0 / temperature
    samples = samples.to(torch.int32).contiguous()
    ids = samples.long()
    vs = v.index_select(0, ids)                                   # the [S, d] operand, 2 MB at S = 4096
    bs = ib.index_select(0, ids) if ib is not None else None
    cs = None
    if log_q_correction:
        if sample_log_q is not None:
            cs = -(_checked_log_q(sample_log_q, n_items).index_select(0, ids) + _f32r(math.log(S)))
        else:
            cs = torch.full((S,), -_f32r(_f32r(math.log(S)) + _f32r(-math.log(n_items))), dtype=torch.float32, device=dev)
    d_vs = torch.empty((S, d), dtype=torch.float32, device=dev)
    d_bs = torch.empty((S,), dtype=torch.float32, device=dev) if ib is not None else None
    loss, pred, d_pred, stat_m, t_k, d_u, d_ub = _streamed_softmax_positives("softmax_shared", u, vs, ub, bs, cs, v, ib, interactions, inv_t)
    d_ib = torch.zeros((n_items,), dtype=torch.float32, device=dev) if ib is not None else None
    d_v = _gather_over_items(interactions, d_pred, u, d_ib) if nnz else torch.zeros_like(v)
    # ---- the samples: dU += P . Vs, dVs = P^T . U in slices of the users, d b_s = the row sums
    n_slices = int(N.query("trec_softmax_shared_slices", n_users, S, d))
    ws = torch.empty((n_slices * S * (d + 1),), dtype=torch.float32, device=dev) if n_slices > 1 else None
    with _timed("softmax_shared_grads"):
        N.call("trec_softmax_shared_grads", N.ptr(u), N.ptr(vs), N.ptr(ub), N.ptr(bs), N.ptr(cs), N.ptr(stat_m), N.ptr(t_k),
               n_users, S, d, inv_t, n_slices, N.ptr(ws), N.ptr(d_u), N.ptr(d_vs), N.ptr(d_bs))
    sorted_ids, order = torch.sort(samples, stable=True)
    N.call("trec_softmax_shared_scatter", N.ptr(sorted_ids.contiguous()), N.ptr(order.contiguous()), N.ptr(d_vs), N.ptr(d_bs), S, d,
           n_items, N.ptr(d_v), N.ptr(d_ib))
    return loss, pred, d_u, d_v, d_ub, d_ib


SOFTMAX_SHARED_HITS_DEFAULT = 0  # tuning "softmax_shared_hits" when nobody set it: the route is opt-in (docs/sampled_losses.md, "Accidental hits on the shared route")


def softmax_shared_hits_supported(n_sampled, interactions, d):
    """Can the shared-negatives MFMA step with accidental hits removed run this shape, and is tuning ``softmax_shared_hits`` on (it
    defaults to off)?"""
    return _step_supported("softmax_shared_hits", n_sampled, interactions, d)


def softmax_shared_hits_step(user_in, item_in, user_bias, item_bias, interactions, samples, temperature, sample_log_q=None,
                             log_q_correction=False):
    """softmax_shared_step with ACCIDENTAL HITS REMOVED: the step softmax_fused_step(remove_accidental_hits=True) would make of the
    [n_users, S] table that repeats ``samples`` -- a column whose id is the item of one of the user's interactions with pos_slot >= 0
    leaves that user's M and Z and has a coefficient of exactly 0; c_s keeps the full S.  Returns (loss [P+], pred_serial [P],
    d user_in, d item_in, d user_bias, d item_bias).  The columns are worked in SORTED id order (the sort the scatter needs anyway):
    a user's hits are then ascending column ranges (trec_softmax_shared_hit_ranges: nnz pairs, n_users counts) and the users a
    column is masked for are a row of interactions.transposed_positive().  Nothing of size [U, S] exists, every workspace is sized
    from (nnz, n_users, S) alone, there are no float atomics and nothing is read on the host."""
    temperature = _checked_temperature(temperature)
    u, v, ub, ib = _step_operands(user_in, item_in, user_bias, item_bias)
    n_users, n_items = interactions.shape
    if samples.dim() != 1 or samples.numel() < 1:
        raise ValueError("samples must be a vector of n_sampled >= 1 item ids")
    S, d, dev, nnz = int(samples.numel()), int(u.shape[1]), u.device, interactions.nnz
    if not step_covers("softmax_shared_hits", S, 0, d):
        raise ValueError("softmax_shared_hits_step covers d %% 4 == 0, 4 <= d <= %d; got d = %d" % (SOFTMAX_SHARED_MAX_D, d))
    inv_t = 1.0 / temperature
    sorted_ids, _ = torch.sort(samples.to(torch.int32).contiguous(), stable=True)
    ids = sorted_ids.long()
    vs = v.index_select(0, ids)
    bs = ib.index_select(0, ids) if ib is not None else None
    cs = None
    if log_q_correction:                                          # (the same floats as softmax_shared_step's, in sorted order)
        if sample_log_q is not None:
            cs = -(_checked_log_q(sample_log_q, n_items).index_select(0, ids) + _f32r(math.log(S)))
        else:
            cs = torch.full((S,), -_f32r(_f32r(math.log(S)) + _f32r(-math.log(n_items))), dtype=torch.float32, device=dev)
    hit_rng = torch.empty((max(nnz, 1), 2), dtype=torch.int32, device=dev)
    hit_cnt = torch.empty((n_users,), dtype=torch.int32, device=dev)
    indptr_tp, users_tp = interactions.transposed_positive()
    N.call("trec_softmax_shared_hit_ranges", N.ptr(interactions.indptr), N.ptr(interactions.x_item32), N.ptr(interactions.pos_slot),
           N.ptr(sorted_ids), n_users, S, N.ptr(hit_rng), N.ptr(hit_cnt))
    loss = torch.empty((interactions.n_positive,), dtype=torch.float32, device=dev)
    pred = torch.empty((nnz,), dtype=torch.float32, device=dev)
    d_pred = torch.empty((nnz,), dtype=torch.float32, device=dev)
    stat_m = torch.empty((n_users,), dtype=torch.float32, device=dev)
    stat_z = torch.empty((n_users,), dtype=torch.float32, device=dev)
    t_k = torch.empty((n_users,), dtype=torch.float32, device=dev)
    d_ub = torch.empty((n_users,), dtype=torch.float32, device=dev) if ub is not None else None
    with _timed("softmax_shared_hits_stats"):
        N.call("trec_softmax_shared_hits_stats", N.ptr(u), N.ptr(vs), N.ptr(ub), N.ptr(bs), N.ptr(cs), N.ptr(interactions.indptr),
               N.ptr(hit_rng), N.ptr(hit_cnt), n_users, S, d, inv_t, N.ptr(stat_m), N.ptr(stat_z))
    if nnz:
        N.call("trec_pair_score_fwd", N.ptr(u), N.ptr(v), N.ptr(interactions.x_user32), N.ptr(interactions.x_item32), nnz, 0, d,
               MODE_DOT, N.ptr(ub), N.ptr(ib), N.ptr(pred), None)
    # (M = -inf, Z = 0 of a user whose samples are all hits: the unchanged kernel gives loss 0, d y_p -0, tK 0 -- m = w_p, b = 0, D = 1)
    N.call("trec_softmax_shared_positives", N.ptr(interactions.indptr), N.ptr(interactions.pos_slot), N.ptr(pred), N.ptr(stat_m),
           N.ptr(stat_z), n_users, inv_t, N.ptr(loss), N.ptr(d_pred), N.ptr(t_k), N.ptr(d_ub))
    d_u = _gather_over_users(interactions, d_pred, v) if nnz else torch.zeros_like(u)
    d_ib = torch.zeros((n_items,), dtype=torch.float32, device=dev) if ib is not None else None
    d_v = _gather_over_items(interactions, d_pred, u, d_ib) if nnz else torch.zeros_like(v)
    d_vs = torch.empty((S, d), dtype=torch.float32, device=dev)
    d_bs = torch.empty((S,), dtype=torch.float32, device=dev) if ib is not None else None
    n_slices = int(N.query("trec_softmax_shared_slices", n_users, S, d))
    ws = torch.empty((n_slices * S * (d + 1),), dtype=torch.float32, device=dev) if n_slices > 1 else None
    with _timed("softmax_shared_hits_grads"):
        N.call("trec_softmax_shared_hits_grads", N.ptr(u), N.ptr(vs), N.ptr(ub), N.ptr(bs), N.ptr(cs), N.ptr(stat_m), N.ptr(t_k),
               N.ptr(interactions.indptr), N.ptr(hit_rng), N.ptr(hit_cnt), N.ptr(sorted_ids), N.ptr(indptr_tp), N.ptr(users_tp),
               n_items, n_users, S, d, inv_t, n_slices, N.ptr(ws), N.ptr(d_u), N.ptr(d_vs), N.ptr(d_bs))
    order = torch.arange(S, dtype=torch.int64, device=dev)        # the rows of d_vs ARE in sorted order: runs of equal ids fold in place
    N.call("trec_softmax_shared_scatter", N.ptr(sorted_ids), N.ptr(order), N.ptr(d_vs), N.ptr(d_bs), S, d, n_items, N.ptr(d_v),
           N.ptr(d_ib))
    return loss, pred, d_u, d_v, d_ub, d_ib


SOFTMAX_FULL_DEFAULT = 0         # tuning "softmax_full" when nobody set it (docs/sampled_losses.md, "Full softmax": the measurement)


def softmax_full_step(user_in, item_in, user_bias, item_bias, interactions, temperature):
    """One step of the FULL softmax over the catalogue (SoftmaxDenseLossGraph) for dot scores on (user_in, item_in), upstream gradient
    1: softmax_shared_step with the item representation itself as the streamed matrix (Vs = item_in, bs = item_bias, no constants,
    S = n_items) -- no gather, no sort, no scatter, and the positives are in the denominator.  Returns (loss [P+], pred_serial [P],
    d user_in, d item_in, d user_bias, d item_bias); d user_bias is an exact 0.  Nothing of size [n_users, n_items] exists and nothing
    is read on the host."""
    temperature = _checked_temperature(temperature)
    u, v, ub, ib = _step_operands(user_in, item_in, user_bias, item_bias)
    n_users, n_items = interactions.shape
    if u.dim() != 2 or v.dim() != 2 or u.shape[0] != n_users or v.shape[0] != n_items or u.shape[1] != v.shape[1] or n_users < 1:
        raise ValueError("softmax_full_step needs [n_users, d] and [n_items, d] representations of the interactions' shape")
    d, dev, nnz = int(u.shape[1]), u.device, interactions.nnz
    if not step_covers("softmax_shared", n_items, 0, d):
        raise ValueError("softmax_full_step covers d %% 4 == 0, 4 <= d <= %d; got d = %d" % (SOFTMAX_SHARED_MAX_D, d))
    inv_t = 1.0 / temperature
    # The tile kernel's DU role ADDS to d user_in and its DV role OVERWRITES d item_in / d item_bias.  So the positives' K1 gather
    # over the users runs BEFORE the tiles (it writes d_u, the tiles add the softmax's share onto it) and their K1 gather over the
    # items runs AFTER them, accumulating (it adds -t u_u per positive, and -t per positive through the row-sum epilogue, onto what
    # the tiles wrote): no buffer is zeroed, every cell has one writer at a time, the order of every sum is fixed.
    loss, pred, d_pred, stat_m, t_k, d_u, d_ub = _streamed_softmax_positives("softmax_full", u, v, ub, ib, None, v, ib, interactions, inv_t)
    d_v = torch.empty_like(v)
    d_ib = torch.empty((n_items,), dtype=torch.float32, device=dev) if ib is not None else None
    n_slices = int(N.query("trec_softmax_shared_slices", n_users, n_items, d))
    ws = torch.empty((n_slices * n_items * (d + 1),), dtype=torch.float32, device=dev) if n_slices > 1 else None
    with _timed("softmax_full_grads"):
        N.call("trec_softmax_shared_grads", N.ptr(u), N.ptr(v), N.ptr(ub), N.ptr(ib), None, N.ptr(stat_m), N.ptr(t_k), n_users,
               n_items, d, inv_t, n_slices, N.ptr(ws), N.ptr(d_u), N.ptr(d_v), N.ptr(d_ib))
    if nnz:
        _gather_over_items(interactions, d_pred, u, d_ib, accumulate=True, out=d_v)
    return loss, pred, d_u, d_v, d_ub, d_ib


DENSE_G_MIN_DENSITY = 1.0 / 32.0     # pairs per user / items from which the item side of the tiled step is a GEMM (G^T . U)


def wmrb_tiled_supported(n_sampled, interactions, d):
    """Can the tiled one-pass WMRB step (csrc/wmrb_tiled.hip: any S, dot or Euclidean scores) run this shape, and is tuning
    ``wmrb_tiled`` on?"""
    return _step_supported("wmrb_tiled", n_sampled, interactions, d)


def _dense_g_fits(n_users, n_items, n_sampled, nnz, dev):
    """The dense coefficient matrix G [n_users, n_items] pays when the pairs of a user are a sizeable share of the items (the
    GEMM does n_items * d MACs per user on fp32 MFMA, the gathers move pairs * d * 4 bytes twice) and fits beside everything else."""
    if not N.load().trec_get_tuning(b"wmrb_dense_g", 1) or n_users == 0:
        return False
    if (n_sampled + nnz / float(n_users)) < DENSE_G_MIN_DENSITY * n_items:
        return False
    need = float(n_users) * ((n_items + 3) // 4 * 4) * 4.0
    if need <= float(1 << 30):                # (small models: no memory query -- the step may be inside a HIP-graph capture)
        return True
    if torch.cuda.is_current_stream_capturing():
        return False
    free, _ = torch.cuda.mem_get_info(dev)
    free += torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
    return need <= 0.4 * free


def _tiled_step_buffers(user_in, item_in, user_bias, item_bias, interactions, samples, mode):
    """What the tiled one-pass steps (wmrb_tiled_step, softmax_tiled_step) start from: (u, v, ub, ib) of _step_operands, the int32
    sample table, and a dict of what both allocate -- loss [P+], pred [P], d_u (None on the dense-G route: dU comes from G . V),
    d_ub or None, val_s [U, S], val_p [P], raw_s / raw_p (Euclidean with item biases, else None), G [n_users, ldg] zeroed or None,
    ldg, val_rs [U] or None -- plus xs (the table flattened), euclid and dense (is the item side the dense-G GEMMs)."""
    u, v, ub, ib = _step_operands(user_in, item_in, user_bias, item_bias)
    n_users, n_items = interactions.shape
    S, dev, nnz = int(samples.shape[1]), u.device, interactions.nnz
    euclid = mode == MODE_EUCLIDEAN
    t = dict(euclid=euclid)
    t["loss"] = torch.empty((interactions.n_positive,), dtype=torch.float32, device=dev)
    t["pred"] = torch.empty((nnz,), dtype=torch.float32, device=dev)
    t["d_ub"] = torch.empty((n_users,), dtype=torch.float32, device=dev) if ub is not None else None
    t["val_s"] = torch.empty((n_users, S), dtype=torch.float32, device=dev)
    t["val_p"] = torch.empty((nnz,), dtype=torch.float32, device=dev)
    need_raw = euclid and ib is not None
    t["raw_s"] = torch.empty((n_users, S), dtype=torch.float32, device=dev) if need_raw else None
    t["raw_p"] = torch.empty((nnz,), dtype=torch.float32, device=dev) if need_raw else None
    samples = samples.to(torch.int32).contiguous()
    t["xs"] = samples.reshape(-1)
    dense = _dense_g_fits(n_users, n_items, S, nnz, dev) and not _LOCAL.deterministic_grouping
    t["dense"] = dense
    t["ldg"] = (n_items + 3) // 4 * 4
    t["G"] = torch.zeros((n_users, t["ldg"]), dtype=torch.float32, device=dev) if dense else None
    # with G the user side needs no second sweep over the rows either: dU = G . V (euclidean: rowsum(G) U - G . V)
    t["d_u"] = None if dense else torch.empty_like(u)
    t["val_rs"] = torch.empty((n_users,), dtype=torch.float32, device=dev) if dense else None
    return u, v, ub, ib, samples, t


def _tiled_item_side(u, v, ib, interactions, S, t):
    """The item side of a tiled one-pass step (wmrb_tiled_step, softmax_tiled_step) from the values its kernel left in ``t``
    (_tiled_step_buffers): the dense-G GEMMs when G was filled, otherwise the grouped gathers; trec_item_weighted_hist for Euclidean
    scores with item biases.  Returns (d_u, d_v, d_ib)."""
    n_users, n_items = interactions.shape
    d, dev, nnz = u.shape[1], u.device, interactions.nnz
    euclid, dense, ldg, xs = t["euclid"], t["dense"], t["ldg"], t["xs"]
    val_s, val_p, raw_s, raw_p, val_rs, d_u = t["val_s"], t["val_p"], t["raw_s"], t["raw_p"], t["val_rs"], t["d_u"]
    need_raw = raw_s is not None
    LAST_FUSED_STATS["route"] = "tiled+dense_g" if dense else "tiled+grouped"
    LAST_FUSED_STATS["drop_zero"] = False
    d_ib = None
    if dense:
        G = t.pop("G")
        # d item_in: dot  dV[i] = sum_u G[u, i] U[u];  euclidean  dV[i] = sum c (V[i] - U[u]) = colsum(G)[i] V[i] - (G^T U)[i]
        # (both GEMMs are gradients, held to 1e-4: split-bf16 operands on bf16 MFMA, bound by reading G instead of by the fp32
        # matrix pipe -- tuning dense_g_split_bf16 = 0: exact fp32 products)
        split = N.load().trec_get_tuning(b"dense_g_split_bf16", 1) != 0
        # euclidean: both gradients are the difference of two products that grow with the rows' common offset (scores do not
        # see it; trained or ReLU rows carry one), while the split product's error is relative to the product -- so the rows are
        # taken about c = mean item row first: dU = rowsum(G) (U - c) - G . (V - c), dV = colsum(G) (V - c) - G^T . (U - c),
        # the same values, with products of the size of the rows' spread (tests/test_gpu_fit_euclid.py)
        c = v.mean(0) if euclid else None
        vc = v - c if euclid else v
        uc = u - c if euclid else u
        v_pad = vc if ldg == n_items else torch.cat([vc, torch.zeros((ldg - n_items, d), dtype=torch.float32, device=dev)])
        with _timed("dense_g_gemm"):
            gv = gemm_raw(G, v_pad, split_bf16=split)          # [n_users, d]
        d_u = val_rs.unsqueeze(1) * uc - gv if euclid else gv
        want_cs = euclid or ib is not None
        with _timed("dense_g_gemm"):                          # (the column sums of G ride in the threads that stage it)
            tg = gemm_raw(G, uc, trans_a=True, split_bf16=split, a_colsum=want_cs and split)
            tg, cs = tg if (want_cs and split) else (tg, None)
            tg = tg[:n_items]
        if want_cs:
            cs = cs[:n_items] if cs is not None else colsum(G)[:n_items]
        d_v = cs.unsqueeze(1) * vc - tg if euclid else tg.contiguous()
        if ib is not None and not euclid:
            d_ib = cs.contiguous()
        del G
    else:
        d_v = torch.zeros_like(v) if nnz == 0 else None
        want_rs = ib is not None and not euclid
        if want_rs:
            d_ib = torch.zeros((n_items,), dtype=torch.float32, device=dev)
        if nnz:
            indptr_t, users_t, perm_t = interactions.transposed()
            d_v = spmm_split(indptr_t, users_t, val_p, perm_t, n_items, nnz, u, own=v if euclid else None,
                             want_rowsum=d_ib if want_rs else False)
        ind_s, users_s, perm_s = group_pairs_by_item(None, xs, S, n_items)
        spmm_split(ind_s, users_s, val_s.reshape(-1), perm_s, n_items, xs.numel(), u, own=v if euclid else None,
                   accumulate=True, out=d_v, want_rowsum=d_ib if want_rs else False)      # (row sums accumulate with the rows)
    if need_raw:
        d_ib = torch.zeros((n_items,), dtype=torch.float32, device=dev)
        with _timed("item_weighted_hist"):
            N.call("trec_item_weighted_hist", N.ptr(xs), N.ptr(raw_s.reshape(-1)), int(xs.numel()), N.ptr(interactions.x_item32),
                   N.ptr(raw_p), int(nnz), int(n_items), N.ptr(d_ib))
    return d_u, d_v, d_ib


def wmrb_tiled_step(user_in, item_in, user_bias, item_bias, interactions, samples, balanced=False, mode=MODE_DOT):
    """wmrb_fused_step for S in the thousands, long rows and Euclidean scores: (loss [P+], pred_serial [P], d user_in, d item_in,
    d user_bias, d item_bias), upstream gradient 1.  User side: ONE kernel, the user's item rows streamed twice (scores into LDS,
    then dU).  Item side (_tiled_item_side): when a user's pairs are a sizeable share of the catalogue (configs[4]: 10 %), the
    pairs' values were also added into a dense G [n_users, n_items] and d item_in is G^T . U on fp32 MFMA -- no sort, no second
    gather of 3.7e8 rows; otherwise the grouped gathers of the composed path (transposed interactions + counting sort of the
    samples)."""
    u, v, ub, ib, samples, t = _tiled_step_buffers(user_in, item_in, user_bias, item_bias, interactions, samples, mode)
    n_users, n_items = interactions.shape
    S, d = int(samples.shape[1]), u.shape[1]
    weight = interactions.balanced_weight() if balanced else None
    with _timed("wmrb_tiled_step"):
        N.call("trec_wmrb_tiled_step", N.ptr(u), N.ptr(v), N.ptr(ub), N.ptr(ib), N.ptr(interactions.indptr),
               N.ptr(interactions.x_item32), N.ptr(interactions.pos_slot), N.ptr(weight), N.ptr(samples), n_users, n_items, S, d,
               int(mode), int(interactions.max_row_nnz), N.ptr(t["loss"]), N.ptr(t["pred"]), N.ptr(t["d_u"]), N.ptr(t["d_ub"]),
               N.ptr(t["val_s"]), N.ptr(t["val_p"]), N.ptr(t["raw_s"]), N.ptr(t["raw_p"]), N.ptr(t["G"]), t["ldg"],
               N.ptr(t["val_rs"]))
    d_u, d_v, d_ib = _tiled_item_side(u, v, ib, interactions, S, t)
    return t["loss"], t["pred"], d_u, d_v, t["d_ub"], d_ib


SOFTMAX_TILED_DEFAULT = 0        # tuning "softmax_tiled" when nobody set it: the route is opt-in (docs/sampled_losses.md, "The tiled one-pass step (sampled softmax)")


def softmax_tiled_supported(n_sampled, interactions, d):
    """Can the tiled one-pass sampled-softmax step (csrc/softmax_tiled.hip: any S, long rows, dot or Euclidean scores) run this
    shape, and is tuning ``softmax_tiled`` on (it defaults to off)?"""
    return _step_supported("softmax_tiled", n_sampled, interactions, d)


def softmax_tiled_step(user_in, item_in, user_bias, item_bias, interactions, samples, temperature, sample_log_q=None,
                       log_q_correction=False, remove_accidental_hits=False, mode=MODE_DOT):
    """softmax_fused_step for S in the thousands, long rows and Euclidean scores (``mode``): the frame and the item side of
    wmrb_tiled_step around the loss of sampled_softmax_loss (``temperature``, ``sample_log_q``, ``log_q_correction``,
    ``remove_accidental_hits`` as there).  Returns (loss [P+], pred_serial [P], d user_in, d item_in, d user_bias, d item_bias),
    upstream gradient 1."""
    temperature = _checked_temperature(temperature)
    if samples.dim() != 2 or samples.shape[0] != interactions.shape[0]:
        raise ValueError("samples must be an [n_users, n_sampled] table")
    if mode not in (MODE_DOT, MODE_EUCLIDEAN):
        raise ValueError("mode must be MODE_DOT or MODE_EUCLIDEAN, got %r" % (mode,))
    u, v, ub, ib, samples, t = _tiled_step_buffers(user_in, item_in, user_bias, item_bias, interactions, samples, mode)
    n_users, n_items = interactions.shape
    S, d = int(samples.shape[1]), u.shape[1]
    log_q = _checked_log_q(sample_log_q, n_items) if log_q_correction and sample_log_q is not None else None
    with _timed("softmax_tiled_step"):
        N.call("trec_softmax_tiled_step", N.ptr(u), N.ptr(v), N.ptr(ub), N.ptr(ib), N.ptr(interactions.indptr),
               N.ptr(interactions.x_item32), N.ptr(interactions.pos_slot), N.ptr(samples), n_users, n_items, S, d, int(mode),
               int(interactions.max_row_nnz), 1.0 / temperature, N.ptr(log_q), -math.log(n_items), 1 if log_q_correction else 0,
               1 if remove_accidental_hits else 0, N.ptr(t["loss"]), N.ptr(t["pred"]), N.ptr(t["d_u"]), N.ptr(t["d_ub"]),
               N.ptr(t["val_s"]), N.ptr(t["val_p"]), N.ptr(t["raw_s"]), N.ptr(t["raw_p"]), N.ptr(t["G"]), t["ldg"],
               N.ptr(t["val_rs"]))
    d_u, d_v, d_ib = _tiled_item_side(u, v, ib, interactions, S, t)
    return t["loss"], t["pred"], d_u, d_v, t["d_ub"], d_ib


def _spmm_rowsum(indptr, indices, values, perm, n_rows, nnz, w, epilogue, accumulate, out, rowsum):
    w = _f32c(w)
    if out is None:
        out = torch.empty((n_rows, w.shape[1]), dtype=torch.float32, device=w.device)
    with _timed("spmm_csr"):
        N.call("trec_spmm_csr", N.ptr(indptr), N.ptr(indices), N.ptr(values), N.ptr(perm), n_rows, nnz, N.ptr(w),
               w.shape[1], None, epilogue, 1 if accumulate else 0, N.ptr(out), N.ptr(rowsum) if epilogue == EPI_ROWSUM else None)
    return out


def wmrb_loss(pred_serial, sample_pred, interactions, balanced=False):
    if sample_pred.shape[0] != interactions.shape[0]:
        raise ValueError("tf_sample_predictions must have one row per user")
    weight = interactions.balanced_weight() if balanced else None
    return _WMRB.apply(pred_serial, sample_pred, interactions, weight)


def _checked_sample_items(sample_items, sample_pred):
    """the int32 [n_users, S] id table behind ``sample_pred``, for the options that need it"""
    if sample_items is None:
        raise ValueError("log_q_correction / remove_accidental_hits need sample_items, the [n_users, n_sampled] ids of the samples")
    if tuple(sample_items.shape) != tuple(sample_pred.shape):
        raise ValueError("sample_items has shape %s, the sample predictions %s" % (tuple(sample_items.shape), tuple(sample_pred.shape)))
    return sample_items.to(torch.int32).contiguous()


def sampled_softmax_loss(pred_serial, sample_pred, interactions, temperature=1.0, sample_items=None, sample_log_q=None,
                         log_q_correction=False, remove_accidental_hits=False):
    """[n_positive] vector log(1 + sum_s exp((y_us - y_p) / temperature)) (csrc/loss_sampled.hip); non-positive interactions are
    ignored, a sampled item that is one of the user's positives stays a negative.

    ``remove_accidental_hits``: a sample whose item (``sample_items`` int32 [n_users, S]) is one of the user's positive interactions
    of this batch leaves the sum.  ``log_q_correction``: every kept sample's logit gets -log(S q(item)), ``sample_log_q`` float32
    [n_items] holding log q (None: uniform, q = 1 / n_items); the correction is the one for S independent draws.  With both off
    the call is the plain one: the same autograd Function and launches."""
    if sample_pred.shape[0] != interactions.shape[0]:
        raise ValueError("tf_sample_predictions must have one row per user")
    temperature = float(temperature)
    if not (temperature > 0.0 and temperature != float("inf")):
        raise ValueError("temperature must be a finite float > 0, got %r" % (temperature,))
    if not (log_q_correction or remove_accidental_hits):
        return _SampledSoftmax.apply(pred_serial, sample_pred, interactions, 1.0 / temperature)
    items = _checked_sample_items(sample_items, sample_pred)
    n_items = interactions.shape[1]
    log_q = None
    if log_q_correction and sample_log_q is not None:
        if sample_log_q.numel() != n_items:
            raise ValueError("sample_log_q has %d entries, the interactions %d items" % (sample_log_q.numel(), n_items))
        log_q = _f32c(sample_log_q).reshape(-1)
    adj = (items, log_q, -math.log(n_items), 1 if log_q_correction else 0, 1 if remove_accidental_hits else 0)
    return _SampledSoftmaxAdjusted.apply(pred_serial, sample_pred, interactions, 1.0 / temperature, adj)


def bpr_loss(pred_serial, sample_pred, interactions, sample_items=None, sample_log_q=None, log_q_correction=False,
             remove_accidental_hits=False):
    """[n_positive] vector mean_s softplus(y_us - y_p) (csrc/loss_sampled.hip); conventions of sampled_softmax_loss.
    ``remove_accidental_hits`` as there, the sum still divided by S.  BPR has no logQ term: ``log_q_correction`` must stay False
    (``sample_log_q`` is accepted and ignored, so both losses take the same keywords)."""
    if sample_pred.shape[0] != interactions.shape[0]:
        raise ValueError("tf_sample_predictions must have one row per user")
    if log_q_correction:
        raise ValueError("BPR has no logQ term: log_q_correction is not available for bpr_loss")
    if not remove_accidental_hits:
        return _BPR.apply(pred_serial, sample_pred, interactions)
    return _BPRAdjusted.apply(pred_serial, sample_pred, interactions, _checked_sample_items(sample_items, sample_pred))


def warp_loss(pred_serial, sample_pred, interactions, sample_items=None, remove_accidental_hits=False):
    """[n_positive] vector of the WARP loss (csrc/loss_warp.hip): a user's samples are tried in table order, the first one with
    v = (1 - y_p) + y_us > 0 gives loss_p = log(max((n_items - 1) div N_p, 1)) * v, N_p the number of trials up to it; no violator:
    0.  The rank weight is not differentiated.  ``remove_accidental_hits`` as for bpr_loss: a hit is no trial.  n_items is
    ``interactions.shape[1]``."""
    if sample_pred.shape[0] != interactions.shape[0]:
        raise ValueError("tf_sample_predictions must have one row per user")
    items = _checked_sample_items(sample_items, sample_pred) if remove_accidental_hits else None
    return _WARP.apply(pred_serial, sample_pred, interactions, items)


class _RMSE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, y):
        pred, y = _f32c(pred), _f32c(y)
        n = pred.numel()
        loss = torch.empty((1,), dtype=torch.float32, device=pred.device)
        n_div = n
        if n:
            n_partial = max(1, min(1024, (n + 4095) // 4096))
            ws = torch.empty((n_partial,), dtype=torch.float32, device=pred.device)
            N.call("trec_rmse_fwd", N.ptr(y), N.ptr(pred), n, N.ptr(ws), n_partial, N.ptr(loss))
        else:
            loss.zero_()
        if _LOCAL.loss_group is not None:
            # user shards: sqrt(sum of every rank's squared errors / all interactions) -- this rank's sum is loss^2 * n; the
            # backward kernel divides by (n_div * loss), now the global count and the global loss
            sums = torch.stack([loss.double()[0] ** 2 * float(n), torch.tensor(float(n), dtype=torch.float64, device=pred.device)])
            _loss_all_reduce(sums)
            loss = torch.sqrt(sums[0] / sums[1]).to(torch.float32).reshape(1)
            n_div = int(sums[1].item())
        ctx.save_for_backward(pred, y, loss)
        ctx.n_div = n_div
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gl):
        pred, y, loss = ctx.saved_tensors
        dp = torch.empty_like(pred)
        n = pred.numel()
        g = _f32c(gl).reshape(1)
        if ctx.n_div != n and n:
            g = g * (float(n) / float(ctx.n_div))         # (the kernel's divisor is its own n)
        if n:
            N.call("trec_rmse_bwd", N.ptr(y), N.ptr(pred), N.ptr(loss), N.ptr(g), n, N.ptr(dp))
        return dp, None


def rmse_loss(pred_serial, interactions_serial):
    return _RMSE.apply(pred_serial, interactions_serial)


# ------------------------------------------------------------------------------------------------ dense / separation losses
DENSE_LOSS_SEPARATION, DENSE_LOSS_SEPARATION_DENSE, DENSE_LOSS_RMSE_DENSE = 0, 1, 2


class _DenseLoss(torch.autograd.Function):
    """RMSEDense / Separation / SeparationDense (loss_graphs.py:62-134) as streaming reductions (csrc/loss_dense.hip): the
    predictions are read once per pass, the interactions enter as their sparse list, the statistics stay on the device in a
    double[16] block that the backward kernels read."""

    @staticmethod
    def forward(ctx, pred, kind, xu32, xi32, values):
        pred = _f32c(pred)
        if kind == DENSE_LOSS_SEPARATION:
            rows, cols = int(pred.numel()), 1
        else:
            rows, cols = int(pred.shape[0]), int(pred.shape[1])
        n_pairs = int(values.numel())
        st = torch.empty((16,), dtype=torch.float64, device=pred.device)
        loss = torch.empty((1,), dtype=torch.float32, device=pred.device)
        if _LOCAL.loss_group is None:
            N.call("trec_dense_loss_fwd", kind, N.ptr(pred), rows, cols, N.ptr(xu32), N.ptr(xi32), N.ptr(values), n_pairs, N.ptr(st),
                   N.ptr(loss))
        else:
            # user shards: the sums of both passes are those of every rank's predictions (csrc/loss_dense.hip, "phase")
            n_all = torch.tensor([float(rows * cols)], dtype=torch.float64, device=pred.device)
            n_all_total = int(_loss_all_reduce(n_all).item()) if kind != DENSE_LOSS_SEPARATION else 0
            for phase in (0, 1, 2):
                N.call("trec_dense_loss_fwd_phase", kind, phase, N.ptr(pred), rows, cols, N.ptr(xu32), N.ptr(xi32), N.ptr(values),
                       n_pairs, n_all_total, N.ptr(st), N.ptr(loss))
                if phase == 0 or (phase == 1 and kind != DENSE_LOSS_RMSE_DENSE):
                    _loss_all_reduce(st[:10])
        ctx.save_for_backward(pred, st)
        ctx.meta = (kind, rows, cols, xu32, xi32, values, n_pairs)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gl):
        pred, st = ctx.saved_tensors
        kind, rows, cols, xu32, xi32, values, n_pairs = ctx.meta
        d_pred = torch.empty_like(pred)
        N.call("trec_dense_loss_bwd", kind, N.ptr(pred), rows, cols, N.ptr(xu32), N.ptr(xi32), N.ptr(values), n_pairs, N.ptr(st),
               N.ptr(_f32c(gl).reshape(1)), N.ptr(d_pred))
        return d_pred, None, None, None, None


class FactoredPrediction(object):
    """The dense prediction of a dot-product (or cosine: rows normalised) model kept as its FACTORS -- user / item
    representations, biases -- plus the serial predictions of the interactions.  TensorRec hands it to the built-in dense losses
    in place of the [n_users, n_items] tensor (which is 4 TB at 1M x 1M): they need two Gram matrices, not the predictions."""

    def __init__(self, user_repr, item_repr, user_bias, item_bias, pred_serial):
        self.user_repr, self.item_repr, self.user_bias, self.item_bias, self.pred_serial = \
            user_repr, item_repr, user_bias, item_bias, pred_serial
        self.shape = (int(user_repr.shape[0]), int(item_repr.shape[0]))


def _augment(rows, bias, ones_first):
    """X = [u | b_u | 1] (ones_first False) / Y = [v | 1 | b_i] (True), float32, contiguous; a missing bias is a zero column"""
    n = rows.shape[0]
    one = torch.ones((n, 1), dtype=torch.float32, device=rows.device)
    b = bias.detach().reshape(n, 1).to(torch.float32) if bias is not None else torch.zeros_like(one)
    return torch.cat([rows.detach().to(torch.float32), one, b] if ones_first else [rows.detach().to(torch.float32), b, one], dim=1).contiguous()


class _FactoredDenseLoss(torch.autograd.Function):
    """RMSEDense / SeparationDense (loss_graphs.py:62-72, :100-134) of p_ui = x_u . y_i from the Gram matrices X^T X, Y^T Y (double,
    csrc/loss_dense.hip): forward O((U + I) d^2) instead of O(U I d), no [U, I] tensor; backward dX = A X (Y^T Y) + B 1 (sum y)^T
    on fp32 MFMA.  The interaction cells' corrections flow into the serial predictions' gradient (K3 backward)."""

    @staticmethod
    def forward(ctx, user_repr, item_repr, user_bias, item_bias, pred_serial, kind, values):
        X, Y = _augment(user_repr, user_bias, False), _augment(item_repr, item_bias, True)
        dev, D, d = X.device, X.shape[1], user_repr.shape[1]
        gx = torch.empty((D, D), dtype=torch.float64, device=dev)
        gy = torch.empty((D, D), dtype=torch.float64, device=dev)
        with _timed("gram_f64"):
            N.call("trec_gram_f64", N.ptr(X), X.shape[0], D, D, N.ptr(gx))
            N.call("trec_gram_f64", N.ptr(Y), Y.shape[0], D, D, N.ptr(gy))
        # sum p = (sum x) . (sum y): the column of ones makes row d + 1 of X^T X the column sums of X (row d of Y^T Y those of Y)
        m = torch.stack([(gx[d + 1] * gy[d]).sum(), (gx * gy).sum()]).contiguous()
        ps = _f32c(pred_serial.detach()).reshape(-1)
        n_pairs = int(values.numel())
        n_local = int(X.shape[0]) * int(Y.shape[0])
        st = torch.empty((16,), dtype=torch.float64, device=dev)
        loss = torch.empty((1,), dtype=torch.float32, device=dev)
        n_total = n_local
        if _LOCAL.loss_group is not None:
            n_total = int(_loss_all_reduce(torch.tensor([float(n_local)], dtype=torch.float64, device=dev)).item())
        for phase in (0, 1, 2):
            N.call("trec_dense_loss_factored_phase", kind, phase, N.ptr(m), N.ptr(ps), N.ptr(values), n_pairs, n_local, n_total,
                   N.ptr(st), N.ptr(loss))
            if _LOCAL.loss_group is not None and (phase == 0 or (phase == 1 and kind != DENSE_LOSS_RMSE_DENSE)):
                _loss_all_reduce(st[:10])
        ctx.save_for_backward(X, Y, gx, gy, ps, st)
        ctx.meta = (kind, values, n_pairs, d, user_bias is not None, item_bias is not None)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gl):
        X, Y, gx, gy, ps, st = ctx.saved_tensors
        kind, values, n_pairs, d, has_ub, has_ib = ctx.meta
        dev = X.device
        d_serial = torch.empty_like(ps)
        coef = torch.empty((2,), dtype=torch.float64, device=dev)
        N.call("trec_dense_loss_factored_bwd", kind, N.ptr(ps), N.ptr(values), n_pairs, N.ptr(st), N.ptr(_f32c(gl).reshape(1)),
               N.ptr(d_serial), N.ptr(coef))
        a, b = coef[0].to(torch.float32), coef[1].to(torch.float32)
        # dX = A X Gy + B 1 sy^T, dY = A Y Gx + B 1 sx^T   (sx = row d + 1 of Gx, sy = row d of Gy); the scalars stay on the device
        dX = gemm_raw(X, gy.to(torch.float32)) * a + (gy[d].to(torch.float32) * b).unsqueeze(0)
        dY = gemm_raw(Y, gx.to(torch.float32)) * a + (gx[d + 1].to(torch.float32) * b).unsqueeze(0)
        du, dv = dX[:, :d].contiguous(), dY[:, :d].contiguous()
        dub = dX[:, d].contiguous() if has_ub else None            # X = [u | b_u | 1]
        dib = dY[:, d + 1].contiguous() if has_ib else None        # Y = [v | 1 | b_i]
        return du, dv, dub, dib, d_serial, None, None


def factored_dense_loss(pred, interactions, kind):
    ub = pred.user_bias.reshape(-1) if pred.user_bias is not None else None
    ib = pred.item_bias.reshape(-1) if pred.item_bias is not None else None
    return _FactoredDenseLoss.apply(pred.user_repr, pred.item_repr, ub, ib, pred.pred_serial, kind, interactions.values)


def separation_loss(pred_serial, interactions_serial):
    """SeparationLossGraph (loss_graphs.py:75-97): 1 - Normal(mu_n - mu_p, sqrt(var_n + var_p)).cdf(0) over the interactions"""
    return _DenseLoss.apply(pred_serial.reshape(-1), DENSE_LOSS_SEPARATION, None, None, _f32c(interactions_serial).reshape(-1))


def separation_dense_loss(prediction, interactions):
    """SeparationDenseLossGraph (loss_graphs.py:100-134): the same over every user-item pair, non-positives as negatives"""
    if isinstance(prediction, FactoredPrediction):
        return factored_dense_loss(prediction, interactions, DENSE_LOSS_SEPARATION_DENSE)
    return _DenseLoss.apply(prediction, DENSE_LOSS_SEPARATION_DENSE, interactions.x_user32, interactions.x_item32, interactions.values)


def rmse_dense_loss(prediction, interactions):
    """RMSEDenseLossGraph (loss_graphs.py:62-72): RMSE against the dense interaction matrix"""
    if isinstance(prediction, FactoredPrediction):
        return factored_dense_loss(prediction, interactions, DENSE_LOSS_RMSE_DENSE)
    return _DenseLoss.apply(prediction, DENSE_LOSS_RMSE_DENSE, interactions.x_user32, interactions.x_item32, interactions.values)


def _row_strided(pred, n_items):
    """(tensor, row stride) of a float32 [n_users, n_items] prediction whose rows are contiguous -- a view of a wider tensor is passed
    as it is, its stride honoured by the kernels -- or a contiguous copy of anything else"""
    if pred.dtype != torch.float32:
        pred = pred.float()
    if n_items > 1 and pred.stride(1) == 1 and pred.stride(0) >= n_items:
        return pred, int(pred.stride(0))
    return pred.contiguous(), n_items


def _ptr_rows(t):
    """device pointer of a tensor whose rows are contiguous (_row_strided); the checks of N.ptr but for the row stride"""
    if not t.is_cuda or t.device.index != torch.cuda.current_device():
        raise N.NativeLibraryError("expected a tensor on the current GPU, got device=%s" % t.device)
    import ctypes
    return ctypes.c_void_p(t.data_ptr())


class _SoftmaxDense(torch.autograd.Function):
    """trec_softmax_dense_fwd / _bwd (csrc/loss_dense.hip): the full softmax over the catalogue on a real [n_users, n_items]
    prediction; the row statistics (M, Z) are kept for the backward pass, which writes the dense gradient in one streaming pass."""

    @staticmethod
    def forward(ctx, pred, inter: Interactions, inv_temperature):
        n_users, n_items = inter.shape
        if pred.dim() != 2 or tuple(pred.shape) != (n_users, n_items):
            raise ValueError("tf_prediction has shape %s, the interactions %s" % (tuple(pred.shape), (n_users, n_items)))
        pred, ld = _row_strided(pred, n_items)
        dev = pred.device
        loss = torch.empty((max(1, inter.n_positive),), dtype=torch.float32, device=dev)[:inter.n_positive]     # (never a null pointer)
        row_max = torch.empty((n_users,), dtype=torch.float32, device=dev)
        row_sum = torch.empty_like(row_max)
        N.call("trec_softmax_dense_fwd", _ptr_rows(pred), ld, N.ptr(inter.indptr), N.ptr(inter.x_item32), N.ptr(inter.pos_slot),
               n_users, n_items, inv_temperature, N.ptr(loss), N.ptr(row_max), N.ptr(row_sum))
        ctx.inter, ctx.inv_temperature, ctx.ld = inter, inv_temperature, ld
        ctx.save_for_backward(pred, row_max, row_sum)
        return loss

    @staticmethod
    def backward(ctx, gl):
        pred, row_max, row_sum = ctx.saved_tensors
        inter = ctx.inter
        n_users, n_items = inter.shape
        d_pred = torch.empty((n_users, n_items), dtype=torch.float32, device=pred.device)
        N.call("trec_softmax_dense_bwd", _ptr_rows(pred), ctx.ld, N.ptr(inter.indptr), N.ptr(inter.x_item32), N.ptr(inter.pos_slot),
               N.ptr(row_max), N.ptr(row_sum), N.ptr(_f32c(gl) if gl.numel() else gl.new_zeros((1,))), n_users, n_items, ctx.inv_temperature, N.ptr(d_pred))
        return d_pred, None, None


def softmax_dense_loss(prediction, interactions, temperature=1.0):
    """SoftmaxDenseLossGraph's generic form: the [n_positive] vector log sum_i exp((y_ui - y_up) / temperature) over EVERY item of the
    catalogue, on a real [n_users, n_items] prediction (any prediction graph).  Magnitudes are ignored; an interaction of value <= 0
    is not a positive, its item still counts in the sum; nothing is clamped."""
    return _SoftmaxDense.apply(prediction, interactions, 1.0 / _checked_temperature(temperature))



RANK_SORT_MAX = 32768            # csrc/rank.hip: the longest row one workgroup sorts in LDS


def rank_rows(scores):
    """rank_predictions (recommendation_graphs.py:73-82) of a score slab [n_users, n_items] -> int32 ranks, 1 = best,
    ties to the lower index.  Rows up to 32768 items are sorted in LDS by one workgroup; longer rows are sorted in
    32768-item chunks and every item binary-searches the other chunks (trec_rank_rows_chunked)."""
    scores = _f32c(scores)
    n_u, n_i = scores.shape
    ranks = torch.empty(scores.shape, dtype=torch.int32, device=scores.device)
    if n_i > RANK_SORT_MAX and n_u > 0 and N.load().trec_get_tuning(b"rank_chunked", 1):
        per_user = N.query("trec_rank_rows_workspace_bytes", 1, n_i)
        slab = int(max(1, min(65535, (4 << 30) // per_user, n_u)))
        nbytes = N.query("trec_rank_rows_workspace_bytes", slab, n_i)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=scores.device)
        for s in range(0, n_u, slab):
            e = min(s + slab, n_u)
            with _timed("rank_rows_chunked"):
                N.call("trec_rank_rows_chunked", N.ptr(scores[s:e]), e - s, n_i, scores.stride(0), N.ptr(ranks[s:e]),
                       ranks.stride(0), N.ptr(ws), nbytes)
        return ranks
    N.call("trec_rank_rows", N.ptr(scores), n_u, n_i, scores.stride(0), N.ptr(ranks), ranks.stride(0))
    return ranks


def pair_scores_exact(users_f32, items_f32, kpad, d, xu32, xi32, user_bias=None, item_bias=None, mode=MODE_DOT,
                      user_sq=None, item_sq=None, item_index_base=0):
    """Exact fp32 scores of (user row, GLOBAL item id) pairs: the k-ordered fmaf chain of the fp32 MFMA kernels and of the
    oracle, biases / Euclidean transform in the reference's order (trec_pair_score_exact)."""
    n_pairs = int(xi32.numel())
    out = torch.empty((n_pairs,), dtype=torch.float32, device=users_f32.device)
    N.call("trec_pair_score_exact", N.ptr(users_f32), N.ptr(items_f32), kpad, int(d), N.ptr(xu32), N.ptr(xi32), n_pairs,
           N.ptr(user_bias), N.ptr(item_bias), mode, N.ptr(user_sq), N.ptr(item_sq), int(item_index_base), N.ptr(out))
    return out


def rank_counts_fused(users_f32, items_f32, kpad, d, pair_indptr, xi32, user_bias=None, item_bias=None, mode=MODE_DOT,
                      user_sq=None, item_sq=None, item_index_base=0, n_chunks=0, target_scores=None):
    """Partial rank counts of pairs grouped by user, with NO score slab (csrc/score_rank.hip): the exact fp32 MFMA score
    tile is compared with the users' targets in registers.  ``users_f32`` / ``items_f32``: fp32 operands [n, kpad] from
    score_prep; ``pair_indptr``: host int64 [n_users + 1]; ``xi32``: device int32 [n_pairs] GLOBAL item ids of the pairs,
    sorted by user.  Returns int32 [n_pairs] counts over this call's items (rank = count + 1 once every item shard's
    counts are summed).  Users with more than 32 targets occupy several resident rows.  ``target_scores``: the pairs'
    exact scores when this call's items are a shard that does not hold every target (the owning shard computes them
    with pair_scores_exact); default: computed here from the operands."""
    import numpy as np
    dev = users_f32.device
    n_pairs = int(xi32.numel())
    counts = torch.zeros((n_pairs,), dtype=torch.int32, device=dev)
    if n_pairs == 0:
        return counts
    qmax = N.query("trec_score_rankcount_max_targets")
    indptr = np.asarray(pair_indptr, dtype=np.int64)
    per_user = np.diff(indptr)
    rows_per_user = -(-per_user // qmax)
    row_user = np.repeat(np.arange(len(per_user), dtype=np.int64), rows_per_user)
    first_row = np.concatenate([[0], np.cumsum(rows_per_user)[:-1]])
    j = np.arange(len(row_user), dtype=np.int64) - first_row[row_user]            # group number inside the user
    row_t0 = indptr[row_user] + qmax * j
    row_tn = np.minimum(qmax, per_user[row_user] - qmax * j)
    xu32 = torch.from_numpy(np.repeat(np.arange(len(per_user), dtype=np.int32), per_user)).to(dev)
    row_user_d = torch.from_numpy(row_user.astype(np.int32)).to(dev)
    row_t0_d = torch.from_numpy(row_t0.astype(np.int32)).to(dev)
    row_tn_d = torch.from_numpy(row_tn.astype(np.int32)).to(dev)
    tgt = target_scores if target_scores is not None else \
        pair_scores_exact(users_f32, items_f32, kpad, d, xu32, xi32, user_bias, item_bias, mode, user_sq, item_sq,
                          item_index_base)
    with _timed("score_gemm_rankcount"):
        N.call("trec_score_gemm_rankcount", N.ptr(users_f32), N.ptr(items_f32), kpad, len(row_user), items_f32.shape[0],
               int(item_index_base), N.ptr(user_bias), N.ptr(item_bias), mode, N.ptr(user_sq), N.ptr(item_sq),
               N.ptr(row_user_d), N.ptr(row_t0_d), N.ptr(row_tn_d), N.ptr(xi32), N.ptr(tgt), int(n_chunks), N.ptr(counts))
    return counts


def rank_of_pairs(scores, col_offset, begin, end, xu32, xi32, target_scores, add_one=True):
    out = torch.empty((xu32.numel(),), dtype=torch.int32, device=scores.device)
    N.call("trec_rank_of_pairs", N.ptr(scores), scores.stride(0), col_offset, begin, end, N.ptr(xu32), N.ptr(xi32),
           N.ptr(target_scores), xu32.numel(), 1 if add_one else 0, N.ptr(out))
    return out


def rank_of_pairs_by_user(scores, col_offset, begin, end, pair_indptr, xi32, target_scores, add_one=True):
    """rank_of_pairs for pairs grouped by user (pair_indptr int64 [n_users + 1] over the rows of ``scores``): a user's
    row is read once for all of the user's targets."""
    n_pairs = xi32.numel()
    out = torch.empty((n_pairs,), dtype=torch.int32, device=scores.device)
    N.call("trec_rank_of_pairs_by_user", N.ptr(scores), scores.stride(0), col_offset, begin, end, N.ptr(pair_indptr),
           N.ptr(xi32), N.ptr(target_scores), scores.shape[0], n_pairs, 1 if add_one else 0, N.ptr(out))
    return out


def sample_items(n_users, n_items, n_sampled, replace, seed, step, device="cuda", user_base=0):
    out = torch.empty((n_users, n_sampled), dtype=torch.int32, device=device)
    with _timed("sample_items"):
        N.call("trec_sample_items", n_users, int(user_base), n_items, n_sampled, 1 if replace else 0,
               int(seed) & (2 ** 64 - 1), int(step) & 0xFFFFFFFF, N.ptr(out))
    return out


def sample_items_alias(n_users, n_items, n_sampled, thr, alias, seed, step, device="cuda", user_base=0):
    """int32 [n_users, n_sampled] drawn with replacement from the alias table (thr: uint32 bits in an int32 tensor [n_items], alias
    int32 [n_items]); csrc/sampler_alias.hip"""
    if thr.numel() != n_items or alias.numel() != n_items:
        raise ValueError("the alias table has %d / %d entries, expected n_items = %d" % (thr.numel(), alias.numel(), n_items))
    out = torch.empty((n_users, n_sampled), dtype=torch.int32, device=device)
    if n_users == 0:                    # (an empty tensor has no address to hand over)
        return out
    with _timed("sample_items_alias"):
        N.call("trec_sample_items_alias", n_users, int(user_base), n_items, n_sampled, N.ptr(thr), N.ptr(alias),
               int(seed) & (2 ** 64 - 1), int(step) & 0xFFFFFFFF, N.ptr(out))
    return out


def hard_negatives_supported(n_candidates, n_sampled, d):
    """Does csrc/sampler_hard.hip cover this shape?  The native library's own statement (host arithmetic, needs no GPU)."""
    return bool(N.query("trec_hard_negatives_supported", int(n_candidates), int(n_sampled), int(d)))


def select_hard_negatives(user_in, item_in, item_bias, interactions, candidates, n_sampled, n_hard=None, exclude=True,
                          return_scores=False):
    """int32 [n_users, n_sampled] chosen from the int32 [n_users, M] table ``candidates`` by the scores user_in . item_in
    (+ item_bias): the ``n_hard`` (None: all) highest-scoring first, then the first of the rest by position; with ``exclude`` the
    accidental hits of ``interactions`` go last (csrc/sampler_hard.hip, the definition: docs/hard_negatives.md).  ``interactions``
    may be None without ``exclude``.  With ``return_scores`` also the float32 [n_users, M] scores.  Nothing is checked on the host
    but the shapes, and nothing is read back: an id outside [0, n_items) is the caller's error."""
    u, v, _, ib = _step_operands(user_in, item_in, None, item_bias)
    if candidates.dim() != 2 or candidates.shape[0] != u.shape[0]:
        raise ValueError("candidates must be an [n_users, n_candidates] table")
    candidates = candidates.to(torch.int32).contiguous()
    n_users, M, d = int(u.shape[0]), int(candidates.shape[1]), int(u.shape[1])
    n_sampled = int(n_sampled)
    n_hard = n_sampled if n_hard is None else int(n_hard)
    out = torch.empty((n_users, n_sampled), dtype=torch.int32, device=u.device)
    scores = torch.empty((n_users, M), dtype=torch.float32, device=u.device) if return_scores else None
    if n_users == 0:                    # (an empty tensor has no address to hand over)
        return (out, scores) if return_scores else out
    exclude = bool(exclude) and interactions.nnz > 0          # (nor have the arrays of a batch without interactions: nothing hits)
    rows = (interactions.indptr, interactions.x_item32, interactions.pos_slot) if exclude else (None, None, None)
    with _timed("select_hard_negatives"):
        N.call("trec_select_hard_negatives", N.ptr(u), N.ptr(v), N.ptr(ib), N.ptr(rows[0]), N.ptr(rows[1]), N.ptr(rows[2]),
               N.ptr(candidates), n_users, int(v.shape[0]), M, n_sampled, n_hard, d, 1 if exclude else 0, N.ptr(out), N.ptr(scores))
    return (out, scores) if return_scores else out


def adam_tf_step(w, m, v, grad, lr_t, l2_coef, beta1=0.9, beta2=0.999, eps=1e-8):
    with _timed("adam_tf_step"):
        N.call("trec_adam_tf_step", N.ptr(w), N.ptr(m), N.ptr(v), N.ptr(_f32c(grad)), w.numel(), float(lr_t), beta1, beta2,
               eps, float(l2_coef))


# ------------------------------------------------------------------------------------------------ schedule on the device
def adam_schedule_advance(state, learning_rate, beta1=0.9, beta2=0.999, bump_sample_step=False):
    N.call("trec_adam_schedule_advance", N.ptr(state), float(learning_rate), float(beta1), float(beta2),
           1 if bump_sample_step else 0)


def adam_tf_step_dev(w, m, v, grad, state, l2_coef, beta1=0.9, beta2=0.999, eps=1e-8):
    N.call("trec_adam_tf_step_dev", N.ptr(w), N.ptr(m), N.ptr(v), N.ptr(_f32c(grad)), w.numel(), N.ptr(state),
           float(beta1), float(beta2), float(eps), float(l2_coef))


def sample_items_dev(n_users, n_items, n_sampled, replace, seed, state, device="cuda", user_base=0):
    """trec_sample_items with the step read from word 3 of the schedule state (uint32 bits)."""
    import ctypes
    out = torch.empty((n_users, n_sampled), dtype=torch.int32, device=device)
    step_ptr = ctypes.c_void_p(state.data_ptr() + 12)
    N.call("trec_sample_items_dev", n_users, int(user_base), n_items, n_sampled, 1 if replace else 0,
           int(seed) & (2 ** 64 - 1), step_ptr, N.ptr(out))
    return out


def exclude_rank_adjust(pair_ptr, t_idx, t_score, ex_ptr, ex_idx, ex_score, counts):
    """Pair rank counts over every item -> counts over the non-excluded items, in place (csrc/exclude.hip): for each target t of
    user u, minus #{x in E_u : s_x > s_t or (s_x == s_t and x < t)}.  ``pair_ptr`` / ``ex_ptr``: device int64 [n_users + 1] over the
    same user rows (absolute positions into t_* / ex_*); scores from the same chain as the counts."""
    n_users = int(pair_ptr.numel()) - 1
    with _timed("exclude_rank_adjust"):
        N.call("trec_exclude_rank_adjust", N.ptr(pair_ptr), N.ptr(t_idx), N.ptr(t_score), N.ptr(ex_ptr), N.ptr(ex_idx),
               N.ptr(ex_score), n_users, N.ptr(counts))
    return counts
