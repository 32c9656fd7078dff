"""The dense / separation loss kernels (csrc/loss_dense.hip) and four small entry points of the training paths, each called
directly through the C ABI and held to a plain float64 restatement of loss_graphs.py:62-134 written here.

The reference never sees a GPU result: float32 inputs are converted exactly to float64, moments are numpy float64 sums, gradients
are closed forms whose agreement with CPU torch.float64 autograd is pinned by a non-GPU test, and the factored form is compared with
CPU torch.float64 autograd of the materialised formula.

Bars (derived from the number formats, not measured):

* loss (float[1])          2 float32 ulps of the float64 reference rounded to float32 (every sum is double; one rounding at the end);
* st[0..15], coef[0..1]    a sum of n terms in double is off by at most n * 2^-53 * sum |term|; n <= 1e8 gives 1e-8 * 2^-53 ~ 1.1e-12, so
                           RTOL = 1e-11 times the sum of the absolute terms (= the value itself for counts and centred moments).  Means,
                           loc, scale, st[15] and coef carry the first-order propagation of those bars (Slot tolerances below);
* materialised gradients   per cell |got - ref| <= 4 * 2^-24 * (|A p| + |B| + |A y|), the cell's own A, B (positive / negative class);
* trec_gram_f64            entrywise n * 2^-53 * (|X|^T |X|), and G == G^T bit for bit;
* factored backward        row by row 2^-24 * ((D + 5) |A| (|X| |G|) + 3 |B| |s| + |dX|): (D + 2) for the float32 GEMM over K = D, one for
                           G narrowed to float32, two for A narrowed to float32 and the scaling product, three for B and s narrowed and
                           their product, one for the final addition;
* d_serial                 4 * 2^-24 * (|g_pos| parts + |g_neg| parts): two float32 roundings and their difference.

The predictions with mean / sigma = 1000 use RTOL = 1e-9 on st and coef: float32 predictions near 1000 sigma make m[1] - 2 mu m[0] + n mu^2
(factored_moments_add_kernel) cancel six digits of the double, and the same six digits go where the positives' and the negatives' means
are subtracted.  At mean / sigma = 10 the plain 1e-11 holds (two digits lost of sixteen); the derived bar stops holding near
mean / sigma ~ 300 (1e-16 * 300^2 ~ 1e-11)."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import oracle as O

gpu = pytest.mark.gpu

U32 = 2.0 ** -24
U64 = 2.0 ** -53
RTOL = 1e-11
RTOL_OFFSET_1000 = 1e-9
SEP, SEP_DENSE, RMSE_DENSE = 0, 1, 2


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


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def f64(a):
    return np.asarray(a, dtype=np.float64)


# ------------------------------------------------------------------------------------------------ the float64 reference
class Ref(object):
    """Moments, loss and gradient coefficients of one loss over float64 inputs.

    ``dense``: the [rows, cols] predictions (None for the serial form); ``xp``: the predictions at the interactions; ``y``: their values.
    ``slots``: {index of st: (value, tolerance per unit of RTOL)} by the layout documented above separation_finish_kernel."""

    def __init__(self, kind, dense, xp, y, gl=1.0, n_all=None):
        xp, y = f64(xp).reshape(-1), f64(y).reshape(-1)
        pos = y > 0.0
        self.kind, self.gl, self.pos, self.degenerate = kind, float(gl), pos, False
        n_pos, n_exp = float(pos.sum()), float((~pos).sum())
        s_pos, s_exp = xp[pos].sum(), xp[~pos].sum()
        cross, cross_mag = (y * y - 2.0 * y * xp).sum(), (y * y + 2.0 * np.abs(y * xp)).sum()
        if dense is not None:
            dense = f64(dense)
            n_all = float(dense.size) if n_all is None else float(n_all)
            s_all, a_all = dense.sum(), np.abs(dense).sum()
        else:
            n_all, s_all, a_all = -1.0, 0.0, 0.0
        a_pos, a_exp = np.abs(xp[pos]).sum(), np.abs(xp[~pos]).sum()
        self.n_all, self.n_pos = n_all, n_pos
        s = {2: (n_pos, n_pos), 3: (s_pos, a_pos), 6: (n_exp, n_exp), 7: (s_exp, a_exp), 9: (cross, cross_mag), 10: (n_all, 0.0)}
        if kind == RMSE_DENSE:
            q_all = (dense * dense).sum()
            q_pos, q_exp = (xp[pos] ** 2).sum(), (xp[~pos] ** 2).sum()
            mse = (q_all + cross) / n_all
            self.loss = math.sqrt(max(mse, 0.0))
            self.defined = True
            rel_mse = (q_all + cross_mag) / (q_all + cross) if mse > 0.0 else 0.0
            c = 1.0 / (self.loss * n_all) if self.loss > 0.0 else 0.0
            s.update({0: (s_all, a_all), 1: (q_all, q_all), 4: (q_pos, q_pos), 5: (q_pos, q_pos), 8: (q_exp, q_exp),
                      11: (0.0, 0.0), 12: (0.0, 0.0), 13: (0.0, 0.0), 14: (0.0, 0.0), 15: (c, abs(c) * (1.0 + 0.5 * rel_mse))})
            self.A_neg, self.B_neg = self.gl * c, 0.0
            self.slots = s
            return
        n_neg = n_all - n_pos if dense is not None else n_exp
        self.n_neg = n_neg
        self.defined = n_pos > 0 and n_neg > 0
        if not self.defined:                      # tf.nn.moments of an empty class: NaN
            self.loss, self.slots = float("nan"), s
            return
        mu_p = s_pos / n_pos
        if dense is not None:
            mu_n, a_neg = (s_all - s_pos) / n_neg, a_all + a_pos
        else:
            mu_n, a_neg = s_exp / n_neg, a_exp
        q_pp, q_pn = ((xp[pos] - mu_p) ** 2).sum(), ((xp[pos] - mu_n) ** 2).sum()
        q_en = ((xp[~pos] - mu_n) ** 2).sum()
        if dense is not None:
            q_all = ((dense - mu_n) ** 2).sum()
            q_n = q_all - q_pn
            s.update({0: (s_all, a_all), 1: (q_all, q_all)})
        else:
            q_n = q_en
            s.update({0: (0.0, 0.0), 1: (0.0, 0.0)})
        var_p, var_n = q_pp / n_pos, q_n / n_neg
        loc, scale = mu_n - mu_p, math.sqrt(var_n + var_p)
        self.degenerate = not scale > 0.0
        if self.degenerate:
            # one positive and one negative (or constant classes): Normal(loc, 0).cdf(0) is a step, erf(-loc / 0) = -+1; the gradient
            # coefficient -phi(z) / scale is 0 / 0 there, in the reference too, and is not compared
            self.defined = loc != 0.0
            self.loss = (1.0 if loc > 0.0 else 0.0) if self.defined else float("nan")
            s.update({4: (q_pp, q_pp), 5: (q_pn, q_pn), 8: (q_en, q_en), 11: (mu_p, a_pos / n_pos), 12: (mu_n, a_neg / n_neg),
                      13: (0.0, 0.0), 14: (loc, a_pos / n_pos + a_neg / n_neg)})
            self.slots = s
            return
        z = -loc / scale
        self.loss = 1.0 - 0.5 * (1.0 + math.erf(z / math.sqrt(2.0)))
        c = -math.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi) / scale
        # first-order propagation, per unit of RTOL: mu = sum / n; loc = mu_n - mu_p; z = -loc / scale; c = -phi(z) / scale
        t_mu_p, t_mu_n = a_pos / n_pos, a_neg / n_neg
        t_loc = t_mu_p + t_mu_n
        t_z = t_loc / scale + abs(z)
        t_c = abs(c) * (1.0 + abs(z) * t_z)
        s.update({4: (q_pp, q_pp), 5: (q_pn, q_pn), 8: (q_en, q_en), 11: (mu_p, t_mu_p), 12: (mu_n, t_mu_n),
                  13: (scale, scale), 14: (loc, t_loc), 15: (c, t_c)})
        s2 = scale * scale
        g = self.gl
        self.mu_p, self.mu_n, self.loc, self.scale, self.c = mu_p, mu_n, loc, scale, c
        self.A_pos, self.B_pos = g * c / n_pos * loc / s2, g * c / n_pos * (1.0 - loc * mu_p / s2)
        self.A_neg, self.B_neg = g * c / n_neg * loc / s2, g * c / n_neg * (-1.0 - loc * mu_n / s2)
        # per unit of RTOL: A = g c loc / (n s2), B = g c / n (-1 - loc mu_n / s2)
        self.t_A = abs(self.A_neg) * (t_c / abs(c) + 3.0) + abs(g * c / n_neg / s2) * t_loc
        self.t_B = abs(g * c / n_neg) * (t_c / abs(c) + 1.0) * (1.0 + abs(loc * mu_n) / s2) \
            + abs(g * c / n_neg / s2) * (t_loc * abs(mu_n) + abs(loc) * t_mu_n + 2.0 * abs(loc * mu_n))
        self.slots = s

    # gradient of a cell of the given class and the bound 4 * 2^-24 * (|A p| + |B| + |A y|)
    def grad(self, p, positive, y=None):
        p = f64(p)
        if self.kind == RMSE_DENSE:
            yy = np.zeros_like(p) if y is None else f64(y)
            return self.A_neg * (p - yy), 4.0 * U32 * (np.abs(self.A_neg * p) + np.abs(self.A_neg * yy))
        A = np.where(positive, self.A_pos, self.A_neg)
        B = np.where(positive, self.B_pos, self.B_neg)
        return A * p + B, 4.0 * U32 * (np.abs(A * p) + np.abs(B))


def ulps32(got, ref64):
    r = np.float32(ref64)
    return abs(float(np.float32(got)) - float(r)) / float(np.spacing(np.abs(r)))


def check_loss(got, ref, what):
    if not ref.defined:
        assert math.isnan(float(got)), "%s: an empty class makes the reference NaN, the kernel gave %r" % (what, float(got))
        return
    n = ulps32(got, ref.loss)
    assert n <= 2.0, "%s: loss %r vs float64 reference %r: %.1f float32 ulps (bar 2)" % (what, float(got), ref.loss, n)


def check_st(st, ref, what, rtol=RTOL, slots=None):
    st = np.asarray(st, dtype=np.float64)
    for j in sorted(ref.slots if slots is None else slots):
        if j not in ref.slots:
            continue
        want, mag = ref.slots[j]
        err = abs(st[j] - want)
        assert err <= rtol * mag, "%s: st[%d] = %r, float64 reference %r: |diff| %.3e > %.0e * %.6e" % (what, j, st[j], want, err, rtol, mag)


def check_cells(got, want, bound, what):
    got, want, bound = f64(got).reshape(-1), f64(want).reshape(-1), f64(bound).reshape(-1)
    assert got.shape == want.shape
    assert np.isfinite(got).all(), "%s: %d cells not written or not finite" % (what, int((~np.isfinite(got)).sum()))
    bad = np.abs(got - want) > bound
    if bad.any():
        k = int(np.argmax(np.abs(got - want) - bound))
        raise AssertionError("%s: %d of %d cells outside the bound; worst at %d: got %r, reference %r, bound %.3e (ratio %.2f)"
                             % (what, int(bad.sum()), got.size, k, got[k], want[k], bound[k], abs(got[k] - want[k]) / max(bound[k], 1e-300)))


def dense_of(shape, xu, xi, y):
    m = np.zeros(shape, dtype=np.float64)
    m[xu, xi] = y
    return m


def ref_rmse_dense(P, xu, xi, y):
    return math.sqrt(((dense_of(P.shape, xu, xi, f64(y)) - f64(P)) ** 2).mean())


def ref_separation(pos, neg):
    pos, neg = f64(pos), f64(neg)
    loc = neg.mean() - pos.mean()
    scale = math.sqrt(((neg - neg.mean()) ** 2).mean() + ((pos - pos.mean()) ** 2).mean())
    return 1.0 - 0.5 * (1.0 + math.erf((0.0 - loc) / scale / math.sqrt(2.0)))


def ref_separation_dense(P, xu, xi, y):
    d = dense_of(P.shape, xu, xi, f64(y)).reshape(-1)
    p = f64(P).reshape(-1)
    return ref_separation(p[d > 0.0], p[d <= 0.0])


# ------------------------------------------------------------------------------------------------ the reference itself (no GPU)
def _dummy_60_90():
    from tensorrec_amd import util
    inter, _, _ = util.generate_dummy_data(num_users=60, num_items=90, interaction_density=.08, num_user_features=40,
                                           num_item_features=50, n_features_per_user=6, n_features_per_item=7, random_state=0)
    m = sp.coo_matrix(sp.csr_matrix(inter))
    m.eliminate_zeros()
    P = np.random.default_rng(3).standard_normal((60, 90)).astype(np.float32)
    return m, P


def test_reference_agrees_with_the_committed_oracle():
    """The float64 restatement == oracle.rmse_dense_loss / separation_loss / separation_dense_loss on the 60 x 90 dummy data to float32
    rounding (rtol 1e-6); the Ref class gives the same losses from its moments."""
    m, P = _dummy_60_90()
    xu, xi, y = m.row, m.col, m.data.astype(np.float32)
    serial = P[xu, xi]
    cases = [(ref_rmse_dense(P, xu, xi, y), O.rmse_dense_loss(P, m), Ref(RMSE_DENSE, P, serial, y)),
             (ref_separation(serial[y > 0], serial[y <= 0]), O.separation_loss(serial, y), Ref(SEP, None, serial, y)),
             (ref_separation_dense(P, xu, xi, y), O.separation_dense_loss(P, m), Ref(SEP_DENSE, P, serial, y))]
    for mine, oracle, ref in cases:
        assert abs(mine - float(oracle)) <= 1e-6 * abs(mine), (mine, oracle)
        assert abs(ref.loss - mine) <= 1e-14 * abs(mine), (ref.loss, mine)


def test_reference_gradients_agree_with_float64_autograd():
    """The closed forms A p + B of Ref.grad == torch.float64 autograd of the three losses on the CPU (1e-12 relative to the bound's
    magnitude |A p| + |B| + |A y|)."""
    m, P = _dummy_60_90()
    xu, xi, y = m.row, m.col, m.data.astype(np.float32)
    yt = torch.from_numpy(f64(y))
    pos_t = yt > 0
    sq2 = math.sqrt(2.0)

    def sep(pos, neg):
        loc = neg.mean() - pos.mean()
        scale = torch.sqrt(((neg - neg.mean()) ** 2).mean() + ((pos - pos.mean()) ** 2).mean())
        return 1.0 - 0.5 * (1.0 + torch.erf((0.0 - loc) / scale / sq2))

    Pt = torch.from_numpy(f64(P)).requires_grad_()
    dense_y = torch.from_numpy(dense_of(P.shape, xu, xi, f64(y)))
    # RMSE dense
    (0.75 * torch.sqrt(((dense_y - Pt) ** 2).mean())).backward()
    r = Ref(RMSE_DENSE, P, P[xu, xi], y, gl=0.75)
    want, bound = r.grad(P, False, dense_y.numpy())
    assert (np.abs(Pt.grad.numpy() - want) <= 1e-12 / (4.0 * U32) * bound + 1e-300).all()
    # separation dense
    Pt.grad = None
    flat, dy = Pt.reshape(-1), dense_y.reshape(-1)
    (0.75 * sep(flat[dy > 0], flat[dy <= 0])).backward()
    r = Ref(SEP_DENSE, P, P[xu, xi], y, gl=0.75)
    want, bound = r.grad(P, (dense_y > 0).numpy())
    assert (np.abs(Pt.grad.numpy() - want) <= 1e-12 / (4.0 * U32) * bound).all()
    # separation, serial
    st = torch.from_numpy(f64(P[xu, xi])).requires_grad_()
    (0.75 * sep(st[pos_t], st[~pos_t])).backward()
    r = Ref(SEP, None, P[xu, xi], y, gl=0.75)
    want, bound = r.grad(P[xu, xi], pos_t.numpy())
    assert (np.abs(st.grad.numpy() - want) <= 1e-12 / (4.0 * U32) * bound).all()


# ------------------------------------------------------------------------------------------------ inputs
SIGMA = 0.7


def make_pairs(rows, cols, pattern, rng):
    """One entry per cell, as the upload guarantees.  none / pos / mixed (both signs, 0.0 and -0.0) / all (every cell, mixed)."""
    n = rows * cols
    if pattern == "none":
        k = 0
    elif pattern == "all":
        k = n
    else:
        k = min(n, max(2, min(n // 13, 200000)))
    if k == n:
        cells = np.arange(n, dtype=np.int64)
    else:
        cells = np.unique(rng.integers(0, n, size=k))
    rng.shuffle(cells)
    k = cells.size
    if pattern == "pos":
        y = rng.uniform(0.5, 2.0, size=k)
    else:
        y = rng.standard_normal(k)
        y[2::7] = 0.0
        y[3::11] = -0.0
        if k >= 1:
            y[0] = 1.25
        if k >= 2:
            y[1] = -0.5
    return (cells // cols).astype(np.int32), (cells % cols).astype(np.int32), y.astype(np.float32)


def make_dense(rows, cols, pattern, offset, seed):
    rng = np.random.default_rng(seed)
    xu, xi, y = make_pairs(rows, cols, pattern, rng)
    P = SIGMA * (offset + rng.standard_normal((rows, cols)))
    P[xu, xi] += 0.6 * SIGMA * (y > 0)
    return P.astype(np.float32), xu, xi, y


def takes_vector_branch(pred, cols):
    """the condition of dense_moments_kernel's float4 branch (ld == cols always holds for the entry points)"""
    return cols % 4 == 0 and pred.data_ptr() % 16 == 0


def run_dense(N, kind, pred, xu, xi, y, gl):
    """trec_dense_loss_fwd + trec_dense_loss_bwd -> loss, st (host), d_pred (host); outputs start as NaN"""
    if kind == SEP:
        rows, cols = int(pred.numel()), 1
    else:
        rows, cols = int(pred.shape[0]), int(pred.shape[1])
    st = torch.full((16,), float("nan"), dtype=torch.float64, device="cuda")
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")
    N.call("trec_dense_loss_fwd", kind, N.ptr(pred), rows, cols, N.ptr(xu), N.ptr(xi), N.ptr(y), int(y.numel()), N.ptr(st), N.ptr(loss))
    d_pred = torch.full(pred.shape, float("nan"), dtype=torch.float32, device="cuda")
    glt = torch.tensor([gl], dtype=torch.float32, device="cuda")
    N.call("trec_dense_loss_bwd", kind, N.ptr(pred), rows, cols, N.ptr(xu), N.ptr(xi), N.ptr(y), int(y.numel()), N.ptr(st), N.ptr(glt),
           N.ptr(d_pred))
    torch.cuda.synchronize()
    return float(loss.cpu()[0]), st.cpu().numpy(), d_pred.cpu().numpy()


def check_dense_case(N, kind, P, xu, xi, y, gl, what, rtol=RTOL, pred=None):
    pred = dev(P) if pred is None else pred
    dxu, dxi, dy = dev(xu), dev(xi), dev(y)
    loss, st, d_pred = run_dense(N, kind, pred, dxu, dxi, dy, gl)
    ref = Ref(kind, P, P[xu, xi], y, gl=gl)
    check_loss(loss, ref, what)
    if not ref.defined:
        return
    check_st(st, ref, what, rtol)
    assert not ref.degenerate
    yd = dense_of(P.shape, xu, xi, f64(y))
    want, bound = ref.grad(P, yd > 0.0, yd)
    check_cells(d_pred, want, bound, what + " d_pred")


# ------------------------------------------------------------------------------------------------ 1. shapes of the dense pass
DENSE_SHAPES = [(1, 1), (3, 4), (7, 333), (64, 1024), (257, 4100), (1000, 1001), (4100, 4100)]
VECTOR_SHAPES = {(3, 4), (64, 1024), (257, 4100), (4100, 4100)}


@gpu
@pytest.mark.parametrize("kind", [SEP_DENSE, RMSE_DENSE])
@pytest.mark.parametrize("rows,cols", DENSE_SHAPES)
def test_dense_shapes(N, kind, rows, cols):
    """(3, 4), (64, 1024), (257, 4100), (4100, 4100): the float4 / non-temporal branch of dense_moments_kernel ((4100, 4100) is the one above
    the 4,096-workgroup cap of every grid-stride kernel); the others the scalar branch.  (1, 1) has one class only: SeparationDense is
    NaN there, as tf.nn.moments of an empty tensor."""
    P, xu, xi, y = make_dense(rows, cols, "mixed", 0.0, seed=rows * 7919 + cols)
    pred = dev(P)
    assert takes_vector_branch(pred, cols) == ((rows, cols) in VECTOR_SHAPES)
    check_dense_case(N, kind, P, xu, xi, y, 0.75, "kind %d %dx%d" % (kind, rows, cols), pred=pred)


@gpu
@pytest.mark.parametrize("kind", [SEP_DENSE, RMSE_DENSE])
def test_dense_unaligned_view_takes_scalar_branch(N, kind):
    """cols % 4 == 0 but the predictions start one element into a larger buffer: 4-byte, not 16-byte aligned"""
    rows, cols = 64, 1024
    P, xu, xi, y = make_dense(rows, cols, "mixed", 0.0, seed=5)
    buf = torch.full((rows * cols + 8,), float("nan"), dtype=torch.float32, device="cuda")
    pred = buf[1:1 + rows * cols].view(rows, cols)
    pred.copy_(torch.from_numpy(P))
    assert cols % 4 == 0 and pred.data_ptr() % 16 == 4 and pred.is_contiguous()
    assert not takes_vector_branch(pred, cols)
    check_dense_case(N, kind, P, xu, xi, y, 1.0, "kind %d unaligned" % kind, pred=pred)


# ------------------------------------------------------------------------------------------------ 2. interactions
@gpu
@pytest.mark.parametrize("kind", [SEP_DENSE, RMSE_DENSE])
@pytest.mark.parametrize("rows,cols,pattern", [(7, 333, "none"), (7, 333, "pos"), (7, 333, "mixed"), (64, 1024, "none"),
                                               (64, 1024, "pos"), (64, 1024, "mixed"), (3, 4, "all"), (9, 13, "all")])
def test_dense_interaction_patterns(N, kind, rows, cols, pattern):
    """no interaction at all (SeparationDense: no positive, NaN as the reference; RMSEDense: the plain root mean square), positives only,
    explicit non-positives of both signs with 0.0 and -0.0, and every cell of a small matrix"""
    P, xu, xi, y = make_dense(rows, cols, pattern, 0.0, seed=rows + 31 * cols)
    assert np.unique(xu.astype(np.int64) * cols + xi).size == y.size
    if pattern == "mixed":
        assert (y > 0).any() and (y < 0).any() and (y == 0).any() and np.signbit(y[y == 0]).any()
    check_dense_case(N, kind, P, xu, xi, y, 1.0, "kind %d %dx%d %s" % (kind, rows, cols, pattern))


# ------------------------------------------------------------------------------------------------ 3. offsets
def rtol_for(offset):
    return RTOL_OFFSET_1000 if offset == 1000.0 else RTOL


@gpu
@pytest.mark.parametrize("kind", [SEP_DENSE, RMSE_DENSE])
@pytest.mark.parametrize("offset", [0.0, 10.0, 1000.0])
@pytest.mark.parametrize("rows,cols", [(7, 333), (64, 1024)])
def test_dense_offsets(N, kind, rows, cols, offset):
    """predictions with mean / sigma in {0, 10, 1000}: the materialised passes centre before they square, so only the means' own digits
    go; RTOL 1e-9 at 1000 (module docstring), 1e-11 otherwise"""
    P, xu, xi, y = make_dense(rows, cols, "mixed", offset, seed=int(offset) + rows)
    check_dense_case(N, kind, P, xu, xi, y, 1.0, "kind %d %dx%d offset %g" % (kind, rows, cols, offset), rtol=rtol_for(offset))


# ------------------------------------------------------------------------------------------------ 4. separation, serial
def make_serial(n_pairs, seed, offset=0.0):
    rng = np.random.default_rng(seed)
    y = rng.standard_normal(n_pairs)
    y[2::7] = 0.0
    y[0], y[1] = 1.5, -1.0
    x = SIGMA * (offset + rng.standard_normal(n_pairs)) + 0.6 * SIGMA * (y > 0)
    return x.astype(np.float32), y.astype(np.float32)


@gpu
@pytest.mark.parametrize("n_pairs", [2, 255, 256, 257, 1000003])
def test_separation_serial(N, n_pairs):
    x, y = make_serial(n_pairs, seed=n_pairs)
    loss, st, dx = run_dense(N, SEP, dev(x), None, None, dev(y), 0.75)
    ref = Ref(SEP, None, x, y, gl=0.75)
    assert ref.defined
    check_loss(loss, ref, "serial %d" % n_pairs)
    check_st(st, ref, "serial %d" % n_pairs)
    assert ref.degenerate == (n_pairs == 2)
    if ref.degenerate:
        return
    want, bound = ref.grad(x, y > 0)
    check_cells(dx, want, bound, "serial %d dx" % n_pairs)


# ------------------------------------------------------------------------------------------------ 5. phases
def split_rows(rows, parts, with_empty):
    """row ranges of the "ranks"; with_empty puts a part of zero rows in the middle"""
    cuts = np.linspace(0, rows, parts + 1).astype(np.int64)
    cuts[1] = max(1, cuts[1] - 3) if rows > 4 else cuts[1]                  # uneven parts
    ranges = [(int(cuts[i]), int(cuts[i + 1])) for i in range(parts)]
    if with_empty:
        ranges.insert(1, (ranges[0][1], ranges[0][1]))
    return ranges


def all_reduce_st(sts):
    """what the data-parallel fit does between the phases: st[0..9] summed over the ranks (here on the host, in float64)"""
    total = np.sum([s[:10].cpu().numpy() for s in sts], axis=0)
    t = torch.from_numpy(total).cuda()
    for s in sts:
        s[:10].copy_(t)
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("parts", [2, 3])
@pytest.mark.parametrize("kind", [SEP, SEP_DENSE, RMSE_DENSE])
def test_phased_forward_equals_reference(N, kind, parts):
    """the rows (kind 0: the pairs) cut into 2 and 3 parts plus one EMPTY part (rows = 0, a one-element dummy buffer) and one part without
    interactions; phase 0 / add / phase 1 / add / phase 2: every part's loss, st and gradients meet the bars of the one-call form"""
    rows, cols = 96, 500
    if kind == SEP:
        x, y = make_serial(5003, seed=parts)
        bounds = split_rows(x.size, parts, True)
        locals_ = [(x[a:b], None, None, y[a:b]) for a, b in bounds]
        ref = Ref(SEP, None, x, y, gl=0.75)
        n_total = 0
    else:
        P, xu, xi, y = make_dense(rows, cols, "mixed", 0.0, seed=11 + parts)
        bounds = split_rows(rows, parts, True)
        quiet = bounds[-1]                                                  # the last part keeps its rows but loses its interactions
        keep = ~((xu >= quiet[0]) & (xu < quiet[1]))
        xu, xi, y = xu[keep], xi[keep], y[keep]
        locals_ = []
        for a, b in bounds:
            sel = (xu >= a) & (xu < b)
            locals_.append((P[a:b], (xu[sel] - a).astype(np.int32), xi[sel], y[sel]))
        assert locals_[-1][3].size == 0 and locals_[1][0].shape[0] == 0
        ref = Ref(kind, P, P[xu, xi], y, gl=0.75)
        n_total = rows * cols
    assert ref.defined
    dummy = torch.zeros((1,), dtype=torch.float32, device="cuda")
    parts_dev = []
    for p, lu, li, ly in locals_:
        n_rows = p.shape[0]
        pred = dev(p) if n_rows else dummy
        parts_dev.append(dict(pred=pred, rows=n_rows, cols=1 if kind == SEP else cols, xu=dev(lu) if lu is not None else None,
                              xi=dev(li) if li is not None else None, y=dev(ly), n=int(ly.size),
                              st=torch.full((16,), float("nan"), dtype=torch.float64, device="cuda"),
                              loss=torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")))
    for phase in (0, 1, 2):
        for q in parts_dev:                                                # (an empty part: the call must succeed)
            N.call("trec_dense_loss_fwd_phase", kind, phase, N.ptr(q["pred"]), q["rows"], q["cols"], N.ptr(q["xu"]), N.ptr(q["xi"]),
                   N.ptr(q["y"]), q["n"], n_total, N.ptr(q["st"]), N.ptr(q["loss"]))
        torch.cuda.synchronize()
        if phase == 0 or (phase == 1 and kind != RMSE_DENSE):
            all_reduce_st([q["st"] for q in parts_dev])
    glt = torch.tensor([0.75], dtype=torch.float32, device="cuda")
    for r, (q, (p, lu, li, ly)) in enumerate(zip(parts_dev, locals_)):
        what = "kind %d part %d of %d" % (kind, r, len(parts_dev))
        check_loss(float(q["loss"].cpu()[0]), ref, what)
        check_st(q["st"].cpu().numpy(), ref, what)
        d_pred = torch.full(q["pred"].shape, float("nan"), dtype=torch.float32, device="cuda")
        N.call("trec_dense_loss_bwd", kind, N.ptr(q["pred"]), q["rows"], q["cols"], N.ptr(q["xu"]), N.ptr(q["xi"]), N.ptr(q["y"]), q["n"],
               N.ptr(q["st"]), N.ptr(glt), N.ptr(d_pred))
        torch.cuda.synchronize()
        if q["rows"] == 0:
            assert torch.isnan(d_pred).all()                               # nothing to write
            continue
        if kind == SEP:
            want, bound = ref.grad(p, ly > 0)
        else:
            yd = dense_of(p.shape, lu, li, f64(ly))
            want, bound = ref.grad(p, yd > 0.0, yd)
        check_cells(d_pred.cpu().numpy(), want, bound, what + " d_pred")


# ------------------------------------------------------------------------------------------------ 6. trec_gram_f64
def gram_ref(X):
    """X^T X and |X|^T |X| of a float32 matrix in float64.  The products are exact in double; the additions are made in long double
    (row blocks of 4,096 through float64 BLAS, whose own error -- 4,096 * 2^-53 relative to |X|^T |X| at worst -- is a fraction of the
    bar for the n where it is used; n <= 64 row by row in long double, where the bar is tight)."""
    n, D = X.shape
    G = np.zeros((D, D), dtype=np.longdouble)
    Ga = np.zeros((D, D), dtype=np.float64)
    if n <= 64:
        for r in range(n):
            x = X[r].astype(np.longdouble)
            G += np.outer(x, x)
            Ga += np.abs(np.outer(f64(X[r]), f64(X[r])))
        return G.astype(np.float64), Ga
    for r0 in range(0, n, 4096):
        b = f64(X[r0:r0 + 4096])
        G += b.T @ b
        b = np.abs(b)
        Ga += b.T @ b
    return G.astype(np.float64), Ga


def call_gram(N, Xd, n, D, ld):
    G = torch.full((D, D), float("nan"), dtype=torch.float64, device="cuda")
    N.call("trec_gram_f64", N.ptr(Xd), n, D, ld, N.ptr(G))
    torch.cuda.synchronize()
    return G.cpu().numpy()


@gpu
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("D", [1, 2, 31, 32, 33, 64, 130, 1024])
def test_gram_f64(N, D, pad):
    """D: one tile (2,048 row slices), a partial last tile, several tiles with the mirrored lower triangle; n: nothing, one row, around one
    32-row block, slices that do not divide n; ld = D and D + 3 (the padding holds NaN: it must not be read into G).  The last column is
    ones, so the last row of G holds the column sums.

    Regression: G == G^T failed here at n = 70,001 for every D >= 31 while both triangles were accumulated by atomicAdd chains of their
    own (the slices arrive in a different order at G[i][j] and G[j][i], so the two sums round differently); trec_gram_f64 now accumulates
    the upper triangle only and copies it below the diagonal."""
    ld = D + pad
    rng = np.random.default_rng(100 * D + pad)
    for n in [0, 1, 31, 32, 33, 70001] + ([1000000] if D <= 34 else []):
        buf = np.full((max(n, 1), ld), np.nan, dtype=np.float32)
        X = (rng.standard_normal((n, D)) * np.exp(rng.uniform(-3, 3, size=(1, D)))).astype(np.float32)
        X[:, D - 1] = 1.0
        buf[:n, :D] = X
        G = call_gram(N, dev(buf), n, D, ld)
        what = "D %d ld %d n %d" % (D, ld, n)
        assert np.isfinite(G).all(), what
        assert np.array_equal(G, G.T), what + ": G != G^T bit for bit"
        if n == 0:
            assert not G.any(), what
            continue
        want, mag = gram_ref(X)
        bad = np.abs(G - want) > n * U64 * mag
        assert not bad.any(), "%s: %d entries outside n * 2^-53 * |X|^T |X|, worst ratio %.2f" % (
            what, int(bad.sum()), float((np.abs(G - want) / (n * U64 * mag)).max()))
        col = f64(X).sum(axis=0)
        assert (np.abs(G[D - 1] - col) <= n * U64 * np.abs(f64(X)).sum(axis=0)).all(), what + ": the row of the ones column != column sums"


@gpu
def test_gram_f64_exact_on_a_binary_grid(N):
    """entries k / 64 with |k| <= 1024: every partial sum of up to 2^20 products is a multiple of 2^-12 below 2^41, exact in double in any
    order -- the slices' atomicAdd order cannot show, G is the exact integer arithmetic bit for bit"""
    rng = np.random.default_rng(7)
    for n, D in [(70001, 33), (1000000, 31), (4097, 130)]:
        k = rng.integers(-1024, 1025, size=(n, D))
        X = (k / 64.0).astype(np.float32)
        want = (f64(k).T @ f64(k)) / 4096.0                                # (integers below 2^41: the float64 product is exact too)
        G = call_gram(N, dev(X), n, D, D)
        assert np.array_equal(G, want), "n %d D %d" % (n, D)


@gpu
def test_gram_f64_refuses_bad_arguments(N):
    X = torch.zeros((4, 1025), dtype=torch.float32, device="cuda")
    G = torch.zeros((1025, 1025), dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match=r"code 1\): trec_gram_f64"):
        N.call("trec_gram_f64", N.ptr(X), 4, 1025, 1025, N.ptr(G))                    # D > 1024
    with pytest.raises(RuntimeError, match=r"code 1\): trec_gram_f64"):
        N.call("trec_gram_f64", N.ptr(X), 4, 64, 63, N.ptr(G))                        # ld < D
    with pytest.raises(RuntimeError, match=r"code 1\): trec_gram_f64"):
        N.call("trec_gram_f64", None, 4, 64, 64, N.ptr(G))                            # NULL X
    with pytest.raises(RuntimeError, match=r"code 1\): trec_gram_f64"):
        N.call("trec_gram_f64", N.ptr(X), 4, 64, 64, None)                            # NULL G
    torch.cuda.synchronize()
    assert not G.any()                                                                  # nothing was launched


# ------------------------------------------------------------------------------------------------ the factored form, entry points
def augment(u, ub, v, ib):
    """X = [u | b_u | 1], Y = [v | 1 | b_i] (float32), as ops_base._augment lays them out"""
    U, I = u.shape[0], v.shape[0]
    X = np.concatenate([u, (ub if ub is not None else np.zeros(U, np.float32)).reshape(U, 1), np.ones((U, 1), np.float32)], axis=1)
    Y = np.concatenate([v, np.ones((I, 1), np.float32), (ib if ib is not None else np.zeros(I, np.float32)).reshape(I, 1)], axis=1)
    return np.ascontiguousarray(X, dtype=np.float32), np.ascontiguousarray(Y, dtype=np.float32)


def make_factors(U, I, d, offset, seed, with_ub=True, with_ib=True, pattern="mixed"):
    """factors whose predictions have sigma ~ SIGMA and mean ~ offset * SIGMA; ps: the interaction cells' predictions rounded to float32
    (the serial predictions the model hands over)"""
    rng = np.random.default_rng(seed)
    u = (rng.standard_normal((U, d)) * math.sqrt(SIGMA / math.sqrt(d))).astype(np.float32)
    v = (rng.standard_normal((I, d)) * math.sqrt(SIGMA / math.sqrt(d))).astype(np.float32)
    ub = (SIGMA * offset + 0.2 * rng.standard_normal(U)).astype(np.float32) if with_ub else None
    ib = (0.2 * rng.standard_normal(I) + (0.0 if with_ub else SIGMA * offset)).astype(np.float32) if with_ib else None
    xu, xi, y = make_pairs(U, I, pattern, rng)
    X, Y = augment(u, ub, v, ib)
    ps = np.einsum("pk,pk->p", f64(X[xu]), f64(Y[xi])).astype(np.float32)
    return u, v, ub, ib, X, Y, xu, xi, y, ps


def factored_m(N, Xd, Yd, d):
    D = Xd.shape[1]
    gx = torch.full((D, D), float("nan"), dtype=torch.float64, device="cuda")
    gy = torch.full((D, D), float("nan"), dtype=torch.float64, device="cuda")
    N.call("trec_gram_f64", N.ptr(Xd), Xd.shape[0], D, D, N.ptr(gx))
    N.call("trec_gram_f64", N.ptr(Yd), Yd.shape[0], D, D, N.ptr(gy))
    return torch.stack([(gx[d + 1] * gy[d]).sum(), (gx * gy).sum()]).contiguous()      # as _FactoredDenseLoss.forward


def check_factored_bwd(N, kind, st, ps, y, ref, gl, what, rtol):
    """trec_dense_loss_factored_bwd: coef = {A, B} and the interaction cells' corrections"""
    n = int(y.size)
    psd, yd = dev(ps), dev(y)
    d_serial = torch.full((max(n, 1),), float("nan"), dtype=torch.float32, device="cuda")
    coef = torch.full((2,), float("nan"), dtype=torch.float64, device="cuda")
    glt = torch.tensor([gl], dtype=torch.float32, device="cuda")
    N.call("trec_dense_loss_factored_bwd", kind, N.ptr(psd), N.ptr(yd), n, N.ptr(st), N.ptr(glt), N.ptr(d_serial), N.ptr(coef))
    torch.cuda.synchronize()
    coef = coef.cpu().numpy()
    if kind == RMSE_DENSE:
        t_A, t_B = ref.slots[15][1] * abs(gl), 0.0
    else:
        t_A, t_B = ref.t_A, ref.t_B
    assert abs(coef[0] - ref.A_neg) <= rtol * t_A, "%s: coef[0] %r vs %r" % (what, coef[0], ref.A_neg)
    assert abs(coef[1] - ref.B_neg) <= rtol * t_B, "%s: coef[1] %r vs %r" % (what, coef[1], ref.B_neg)
    if n:
        want, bound = serial_correction(ref, ps, y)
        check_cells(d_serial.cpu().numpy()[:n], want, bound, what + " d_serial")
    return coef


def serial_correction(ref, ps, y):
    """g_pos(p) - g_neg(p) at the positives, 0 elsewhere (separation); -A y (RMSE)"""
    ps, y = f64(ps), f64(y)
    if ref.kind == RMSE_DENSE:
        return -ref.A_neg * y, 4.0 * U32 * np.abs(ref.A_neg * y)
    pos = y > 0.0
    gp = ref.A_pos * ps + ref.B_pos
    gn = ref.A_neg * ps + ref.B_neg
    mag = np.abs(ref.A_pos * ps) + abs(ref.B_pos) + np.abs(ref.A_neg * ps) + abs(ref.B_neg)
    return np.where(pos, gp - gn, 0.0), np.where(pos, 4.0 * U32 * mag, 0.0)


@gpu
@pytest.mark.parametrize("kind", [SEP_DENSE, RMSE_DENSE])
@pytest.mark.parametrize("offset", [0.0, 10.0, 1000.0])
@pytest.mark.parametrize("pattern", ["mixed", "none", "pos"])
def test_factored_phase_entry_points(N, kind, offset, pattern):
    """trec_gram_f64 -> m -> trec_dense_loss_factored_phase -> trec_dense_loss_factored_bwd against the float64 moments of the
    materialised P = X Y^T (float64, CPU), at mean / sigma in {0, 10, 1000}: m[1] - 2 mu m[0] + n mu^2 is where the cancellation shows"""
    U, I, d = 301, 1024, 30
    u, v, ub, ib, X, Y, xu, xi, y, ps = make_factors(U, I, d, offset, seed=int(offset) + 1, pattern=pattern)
    P = f64(X) @ f64(Y).T
    assert abs(P.mean() / P.std() - offset) < 0.1 * offset + 0.2
    ref = Ref(kind, P, ps, y, gl=0.75)
    Xd, Yd, psd, yd = dev(X), dev(Y), dev(ps), dev(y)
    m = factored_m(N, Xd, Yd, d)
    st = torch.full((16,), float("nan"), dtype=torch.float64, device="cuda")
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")
    for phase in (0, 1, 2):
        N.call("trec_dense_loss_factored_phase", kind, phase, N.ptr(m), N.ptr(psd), N.ptr(yd), int(y.size), U * I, U * I, N.ptr(st),
               N.ptr(loss))
    torch.cuda.synchronize()
    what = "factored kind %d offset %g %s" % (kind, offset, pattern)
    check_loss(float(loss.cpu()[0]), ref, what)
    if not ref.defined:
        return
    check_st(st.cpu().numpy(), ref, what, rtol_for(offset))
    check_factored_bwd(N, kind, st, ps, y, ref, 0.75, what, rtol_for(offset))


@gpu
@pytest.mark.parametrize("parts", [2, 3])
@pytest.mark.parametrize("kind", [SEP_DENSE, RMSE_DENSE])
def test_factored_phases_over_user_parts(N, kind, parts):
    """the users cut into 2 and 3 parts plus a part with ZERO rows of X and a part without interactions; every part holds all items"""
    U, I, d = 203, 500, 14
    u, v, ub, ib, X, Y, xu, xi, y, ps = make_factors(U, I, d, 0.0, seed=parts)
    bounds = split_rows(U, parts, True)
    quiet = bounds[-1]
    keep = ~((xu >= quiet[0]) & (xu < quiet[1]))
    xu, xi, y, ps = xu[keep], xi[keep], y[keep], ps[keep]
    ref = Ref(kind, f64(X) @ f64(Y).T, ps, y, gl=1.0)
    assert ref.defined
    Yd = dev(Y)
    state = []
    for a, b in bounds:
        sel = (xu >= a) & (xu < b)
        Xd = dev(X[a:b]) if b > a else torch.zeros((1, d + 2), dtype=torch.float32, device="cuda")   # (n = 0: never read, but not NULL)
        gx = torch.full((d + 2, d + 2), float("nan"), dtype=torch.float64, device="cuda")
        gy = torch.full((d + 2, d + 2), float("nan"), dtype=torch.float64, device="cuda")
        N.call("trec_gram_f64", N.ptr(Xd), b - a, d + 2, d + 2, N.ptr(gx))
        N.call("trec_gram_f64", N.ptr(Yd), I, d + 2, d + 2, N.ptr(gy))
        m = torch.stack([(gx[d + 1] * gy[d]).sum(), (gx * gy).sum()]).contiguous()
        if b == a:
            assert not m.cpu().numpy().any()
        state.append(dict(m=m, ps=ps[sel], y=y[sel], psd=dev(ps[sel]), yd=dev(y[sel]), n_local=(b - a) * I,
                          st=torch.full((16,), float("nan"), dtype=torch.float64, device="cuda"),
                          loss=torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")))
    assert state[-1]["y"].size == 0 and state[1]["n_local"] == 0
    for phase in (0, 1, 2):
        for q in state:
            N.call("trec_dense_loss_factored_phase", kind, phase, N.ptr(q["m"]), N.ptr(q["psd"]), N.ptr(q["yd"]), int(q["y"].size),
                   q["n_local"], U * I, N.ptr(q["st"]), N.ptr(q["loss"]))
        torch.cuda.synchronize()
        if phase == 0 or (phase == 1 and kind != RMSE_DENSE):
            all_reduce_st([q["st"] for q in state])
    for r, q in enumerate(state):
        what = "factored kind %d part %d of %d" % (kind, r, len(state))
        check_loss(float(q["loss"].cpu()[0]), ref, what)
        check_st(q["st"].cpu().numpy(), ref, what)
        check_factored_bwd(N, kind, q["st"], q["ps"], q["y"], ref, 1.0, what, RTOL)


# ------------------------------------------------------------------------------------------------ 7. factored, end to end
def factored_reference(kind, u, v, ub, ib, ps, xu, xi, y, gl):
    """CPU torch.float64 autograd of the materialised formula.  The interaction cells enter through ps (their serial predictions, an
    input of its own), every cell of P = u v^T + b_u + b_i as a negative: d loss / d ps is then the cells' correction."""
    t = lambda a: torch.from_numpy(f64(a)).requires_grad_()
    ut, vt, pst = t(u), t(v), t(ps)
    ubt = t(ub) if ub is not None else None
    ibt = t(ib) if ib is not None else None
    yt = torch.from_numpy(f64(y))
    P = ut @ vt.T
    if ubt is not None:
        P = P + ubt[:, None]
    if ibt is not None:
        P = P + ibt[None, :]
    n_all = float(P.numel())
    if kind == RMSE_DENSE:
        loss = torch.sqrt(((P * P).sum() + (yt * yt - 2.0 * yt * pst).sum()) / n_all)
    else:
        pos = pst[yt > 0]
        n_pos = float(pos.numel())
        n_neg = n_all - n_pos
        mu_p = pos.sum() / n_pos
        mu_n = (P.sum() - pos.sum()) / n_neg
        var_p = ((pos - mu_p) ** 2).sum() / n_pos
        var_n = (((P - mu_n) ** 2).sum() - ((pos - mu_n) ** 2).sum()) / n_neg
        loss = 1.0 - 0.5 * (1.0 + torch.erf((0.0 - (mu_n - mu_p)) / torch.sqrt(var_n + var_p) / math.sqrt(2.0)))
    (gl * loss).backward()
    g = lambda a: a.grad.numpy() if a is not None else None
    return float(loss.detach()), g(ut), g(vt), g(ubt), g(ibt), g(pst), P.detach().numpy()


def gemm_bound(A, B, X, G, s, dX):
    """row-by-row bound of dX = A X G + B 1 s^T computed in float32 from double G (module docstring)"""
    D = X.shape[1]
    E = np.abs(f64(X)) @ np.abs(G)
    return U32 * ((D + 5) * abs(A) * E + 3.0 * abs(B) * np.abs(s)[None, :] + np.abs(dX))


FACTORED_CASES = [(150, 333, d, ub, ib) for d in (4, 30, 62, 510) for ub in (True, False) for ib in (True, False)] \
    + [(1000, 1024, d, True, True) for d in (4, 30, 62, 510)] + [(1000, 1024, 30, False, False)] \
    + [(20000, 3000, 30, True, True), (20000, 3000, 510, True, False), (20000, 3000, 62, False, True)]


@gpu
@pytest.mark.parametrize("kind", [SEP_DENSE, RMSE_DENSE])
@pytest.mark.parametrize("U,I,d,with_ub,with_ib", FACTORED_CASES)
def test_factored_dense_loss_end_to_end(ops, kind, U, I, d, with_ub, with_ib):
    """ops_base.factored_dense_loss on a FactoredPrediction built here: loss and du, dv, dub, dib, d_serial against CPU float64 autograd
    of the materialised formula, every element; d_serial also against the closed g_pos(p) - g_neg(p) / -A y."""
    gl = 0.75
    u, v, ub, ib, X, Y, xu, xi, y, ps = make_factors(U, I, d, 0.0, seed=U + d, with_ub=with_ub, with_ib=with_ib)
    leaf = lambda a: dev(a).requires_grad_() if a is not None else None
    ut, vt, ubt, ibt, pst = leaf(u), leaf(v), leaf(ub), leaf(ib), leaf(ps)
    pred = ops.FactoredPrediction(ut, vt, ubt, ibt, pst)
    loss = ops.factored_dense_loss(pred, SimpleNamespace(values=dev(y)), kind)
    (loss * gl).backward()
    torch.cuda.synchronize()
    what = "e2e kind %d %dx%d d %d ub %d ib %d" % (kind, U, I, d, with_ub, with_ib)
    ref_loss, du, dv, dub, dib, dps, P = factored_reference(kind, u, v, ub, ib, ps, xu, xi, y, gl)
    ref = Ref(kind, P, ps, y, gl=gl)
    assert ref.defined and abs(ref.loss - ref_loss) <= 1e-12 * abs(ref_loss)
    check_loss(float(loss.detach().cpu()), ref, what)
    # the interaction cells' correction, on its own: closed form == autograd (reference against reference), then the kernel against it
    want, bound = serial_correction(ref, ps, y)
    assert (np.abs(dps - want) <= 1e-9 * bound / (4.0 * U32) + 1e-300).all()
    check_cells(pst.grad.cpu().numpy(), want, bound, what + " d_serial")
    # dX = A X Gy + B 1 sy^T, dY = A Y Gx + B 1 sx^T from the reference's own A, B, Gram matrices
    del P
    A, B = ref.A_neg, ref.B_neg
    Gx, Gy = f64(X).T @ f64(X), f64(Y).T @ f64(Y)
    sx, sy = Gx[d + 1], Gy[d]
    dX = A * (f64(X) @ Gy) + B * sy[None, :]
    dY = A * (f64(Y) @ Gx) + B * sx[None, :]
    bX, bY = gemm_bound(A, B, X, Gy, sy, dX), gemm_bound(A, B, Y, Gx, sx, dY)
    # (the closed form is the autograd gradient: 1e-9 of the bound's magnitude)
    assert (np.abs(dX[:, :d] - du) <= 1e-9 * bX[:, :d] / U32).all() and (np.abs(dY[:, :d] - dv) <= 1e-9 * bY[:, :d] / U32).all()
    check_cells(ut.grad.cpu().numpy(), du, bX[:, :d], what + " du")
    check_cells(vt.grad.cpu().numpy(), dv, bY[:, :d], what + " dv")
    if with_ub:
        check_cells(ubt.grad.cpu().numpy(), dub, bX[:, d], what + " dub")
    if with_ib:
        check_cells(ibt.grad.cpu().numpy(), dib, bY[:, d + 1], what + " dib")


# ------------------------------------------------------------------------------------------------ 8. small entry points
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@gpu
@pytest.mark.parametrize("n", [1, 3, 4, 1027, 1000001])
def test_relu_bwd_bit_exact(N, n):
    """dpre = dout where out > 0 (relu_bwd_kernel, csrc/spmm.hip; tf.nn.relu's ReluGrad), else +0.0 -- bit for bit.  A positive denormal
    is > 0 and passes the gradient; +0.0, -0.0, negative values and negative denormals do not."""
    rng = np.random.default_rng(n)
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 1.0, -1.0, np.float32(np.finfo(np.float32).tiny)], dtype=np.float32)
    out = np.maximum(rng.standard_normal(n), 0.0).astype(np.float32)
    idx = rng.permutation(n)[:min(n, 4 * special.size)]
    out[idx] = special[(np.arange(idx.size) + n) % special.size]
    dout = rng.standard_normal(n).astype(np.float32)
    dout[::5] = -0.0
    dout[1::7] = 1e-42
    dpre = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    d_out, d_dout = dev(out), dev(dout)                                    # kept alive: N.ptr() takes raw pointers
    N.call("trec_relu_bwd", N.ptr(d_out), N.ptr(d_dout), n, N.ptr(dpre))
    torch.cuda.synchronize()
    want = np.where(f64(out) > 0.0, dout, np.float32(0.0)).astype(np.float32)
    assert np.array_equal(bits(dpre.cpu().numpy()), bits(want))


def hist_case(N, n_items, n_a, n_b, seed):
    rng = np.random.default_rng(seed)

    def ids(k):
        a = rng.integers(0, n_items, size=k).astype(np.int32)
        a[::17] = n_items                                                  # one past the end
        a[5::19] = -1
        a[7::23] = np.iinfo(np.int32).min
        a[11::29] = np.iinfo(np.int32).max
        return a

    ia, ib = ids(n_a), ids(n_b)
    va, vb = rng.standard_normal(n_a).astype(np.float32), rng.standard_normal(n_b).astype(np.float32)
    va[3::13] = 0.0
    out0 = rng.standard_normal(n_items).astype(np.float32)
    out = dev(out0.copy())
    d_ia, d_va, d_ib, d_vb = dev(ia), dev(va), dev(ib), dev(vb)            # kept alive: N.ptr() takes raw pointers (empty: NULL)
    N.call("trec_item_weighted_hist", N.ptr(d_ia), N.ptr(d_va), n_a, N.ptr(d_ib), N.ptr(d_vb), n_b, n_items, N.ptr(out))
    torch.cuda.synchronize()
    i_all, v_all = np.concatenate([ia, ib]).astype(np.int64), f64(np.concatenate([va, vb]))
    ok = (i_all >= 0) & (i_all < n_items)
    want, mag, count = f64(out0), np.abs(f64(out0)), np.zeros(n_items)
    np.add.at(want, i_all[ok], v_all[ok])
    np.add.at(mag, i_all[ok], np.abs(v_all[ok]))
    np.add.at(count, i_all[ok], 1.0)
    # count_i additions of float32 in any order: gamma_k = k u / (1 - k u) times the sum of the absolute terms (the item's start included)
    bound = count * U32 / (1.0 - count * U32) * mag
    got = f64(out.cpu().numpy())
    bad = np.abs(got - want) > bound
    assert not bad.any(), "n_items %d n_a %d n_b %d: %d items outside the bound, first at item %d: got %r, reference %r, bound %.3e" % (
        n_items, n_a, n_b, int(bad.sum()), int(np.argmax(bad)), got[np.argmax(bad)], want[np.argmax(bad)], bound[np.argmax(bad)])
    untouched = count == 0
    assert np.array_equal(bits(out.cpu().numpy()[untouched]), bits(out0[untouched]))


@gpu
@pytest.mark.parametrize("n_items", [1, 333, 26744, 32768, 32769, 1000000])
def test_item_weighted_hist(N, n_items):
    """n_items <= 32,768: one LDS histogram per workgroup (26,744 and 32,768 need more than 64 KB of it, 32,768 all 128 KB); above: global
    atomics.  Both lists, either empty, both empty; ids outside [0, n_items) and negative ids skipped; out is added to, not cleared."""
    k = 3000 if n_items == 1 else 200000                                   # (200,000 pairs: four workgroups of the LDS form)
    hist_case(N, n_items, k, k // 3, seed=n_items)
    hist_case(N, n_items, k, 0, seed=n_items + 1)
    hist_case(N, n_items, 0, 777, seed=n_items + 2)
    hist_case(N, n_items, 0, 0, seed=n_items + 3)
    if n_items == 1000000:
        hist_case(N, n_items, 4300000, 100001, seed=9)                     # more than 4,096 workgroups' worth: the grid-stride loop wraps


@gpu
def test_adam_schedule_advance_reproduces_the_host_schedule(ops):
    """1,000 advances: state = {beta1^t, beta2^t, lr_t, step} equals the host's float32 running powers and tensorrec._adam_lr_t bit for
    bit; the step word counts up only when bump_sample_step is set"""
    from tensorrec_amd.tensorrec import _adam_lr_t, ADAM_BETA1, ADAM_BETA2
    lr = 0.0123
    state = torch.tensor([1.0, 1.0, 0.0, 0.0], dtype=torch.float32, device="cuda")
    state.view(torch.int32)[3] = 41
    b1p, b2p, step = np.float32(1.0), np.float32(1.0), 41
    for t in range(1, 1001):
        bump = t % 3 == 0
        ops.adam_schedule_advance(state, lr, ADAM_BETA1, ADAM_BETA2, bump_sample_step=bump)
        b1p, b2p = np.float32(b1p * np.float32(ADAM_BETA1)), np.float32(b2p * np.float32(ADAM_BETA2))
        step += 1 if bump else 0
        got = state.cpu().numpy()
        want = np.array([b1p, b2p, np.float32(_adam_lr_t(lr, t))], dtype=np.float32)
        assert np.array_equal(bits(got[:3]), bits(want)), "step %d: %r vs %r" % (t, got[:3], want)
        assert int(bits(got)[3]) == step, "step %d: sample step word %d, expected %d" % (t, int(bits(got)[3]), step)
    assert step == 41 + 333


@gpu
@pytest.mark.parametrize("n", [1, 3, 1027])
def test_adam_tf_step_dev_equals_host_lr_form(ops, n):
    """trec_adam_tf_step_dev (lr_t read from the schedule state) == trec_adam_tf_step with the same lr_t, bit for bit, over three steps"""
    from tensorrec_amd.tensorrec import ADAM_BETA1, ADAM_BETA2
    rng = np.random.default_rng(n)
    w0 = rng.standard_normal(n).astype(np.float32)
    wa, ma, va = dev(w0.copy()), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    wb, mb, vb = dev(w0.copy()), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    state = torch.tensor([1.0, 1.0, 0.0, 0.0], dtype=torch.float32, device="cuda")
    for t in range(3):
        g = dev(rng.standard_normal(n).astype(np.float32))
        ops.adam_schedule_advance(state, 0.05, ADAM_BETA1, ADAM_BETA2)
        lr_t = float(state.cpu().numpy()[2])
        ops.adam_tf_step(wa, ma, va, g, lr_t, 0.01, ADAM_BETA1, ADAM_BETA2, 1e-8)
        ops.adam_tf_step_dev(wb, mb, vb, g, state, 0.01, ADAM_BETA1, ADAM_BETA2, 1e-8)
        torch.cuda.synchronize()
        for a, b, name in ((wa, wb, "w"), (ma, mb, "m"), (va, vb, "v")):
            assert np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy())), "%s differs at step %d" % (name, t)
    assert not np.array_equal(wa.cpu().numpy(), w0)


@gpu
@pytest.mark.parametrize("replace", [True, False])
@pytest.mark.parametrize("n_sampled", [3, 40])
def test_sample_items_dev_equals_host_step_form(ops, replace, n_sampled):
    """trec_sample_items_dev (step read from word 3 of the schedule state) == trec_sample_items at the same step, bit for bit; the next
    step gives another table (n_sampled >= 8 without replacement is the keyed kernel, the others the plain one)"""
    n_users, n_items, seed = 517, 1000, 0x1234567890ABCDEF
    state = torch.tensor([1.0, 1.0, 0.0, 0.0], dtype=torch.float32, device="cuda")
    tables = []
    for step in (0, 1, 77, 2 ** 32 - 1):
        state.view(torch.int32)[3] = step if step < 2 ** 31 else step - 2 ** 32
        a = ops.sample_items(n_users, n_items, n_sampled, replace, seed, step)
        b = ops.sample_items_dev(n_users, n_items, n_sampled, replace, seed, state)
        torch.cuda.synchronize()
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert np.array_equal(a, b), "step %d" % step
        assert a.min() >= 0 and a.max() < n_items
        if not replace:
            assert all(np.unique(r).size == n_sampled for r in a)
        tables.append(a)
    assert not np.array_equal(tables[0], tables[1])
