"""Integer restatement of the alias sampler (csrc/sampler_alias.hip, tensorrec.PopularitySampler): NumPy only, nothing of the code under
test.  The table builder (Walker / Vose, float64, two stacks filled in index order and popped from the end), the exact distribution a
table implements, the kernel's draw in uint64 arithmetic on the Philox4x32-10 restatement of oracle/device_sampler.py, the weight
vectors the tests use and the chi-square rule of tests/test_gpu_sampler_quality.py.

    draw   block = Philox4x32-10(counter (u_lo, s >> 1, step, 0x414C4953 + u_hi), key (seed_lo, seed_hi)),  u = user_base + row
           (w0, w1) = words (0, 1) of the block for an even s, words (2, 3) for an odd one
           j = (w0 * n_items) >> 32;   item = j if w1 < thr[j] else alias[j]          (strictly below)
    q      q_i * n_items * 2^32 = thr[i] + sum_{j: alias[j] = i} (2^32 - thr[j]), an integer; the sum over i is n_items * 2^32
"""
import numpy as np

from oracle import device_sampler as DS

ALIAS_STREAM = 0x414C4953
ONE = (1 << 32) - 1
N_ITEMS = [1, 2, 3, 1000, 70001]


def build_table(weights):
    w = np.asarray(weights, np.float64)
    n = w.size
    p = list(w * (n / w.sum()))
    prob, alias = [1.0] * n, list(range(n))
    small = [i for i in range(n) if p[i] < 1.0]
    large = [i for i in range(n) if p[i] >= 1.0]
    while small and large:
        s, g = small.pop(), large.pop()
        prob[s], alias[s] = p[s], g
        p[g] = (p[g] + p[s]) - 1.0
        (small if p[g] < 1.0 else large).append(g)
    thr = [ONE if alias[j] == j else min(ONE, int(np.floor(prob[j] * 4294967296.0 + 0.5))) for j in range(n)]
    return np.array(thr, np.uint32), np.array(alias, np.int32)


def table_counts(thr, alias):
    """q_i n 2^32 as Python integers"""
    num = [int(t) for t in thr]
    for j, a in enumerate(alias):
        num[int(a)] += (1 << 32) - int(thr[j])
    return num


def table_q(thr, alias):
    return np.array(table_counts(thr, alias), np.float64) / (float(len(thr)) * 4294967296.0)


def draw(n_users, n_items, n_sampled, thr, alias, seed, step, user_base=0):
    seed = int(seed) & (2 ** 64 - 1)
    u = np.repeat(np.arange(n_users, dtype=np.uint64) + np.uint64(user_base), n_sampled)
    s = np.tile(np.arange(n_sampled, dtype=np.uint32), n_users)
    u_lo, u_hi = (u & DS.U32).astype(np.uint32), (u >> np.uint64(32)).astype(np.uint32)
    with np.errstate(over="ignore"):
        c3 = (np.uint32(ALIAS_STREAM) + u_hi).astype(np.uint32)
    r = DS.philox4x32_10(u_lo, s >> np.uint32(1), np.full(u.shape, step, np.uint32), c3, seed & 0xFFFFFFFF, seed >> 32)
    odd = (s & np.uint32(1)) == 1
    w0, w1 = np.where(odd, r[2], r[0]), np.where(odd, r[3], r[1])
    j = ((w0.astype(np.uint64) * np.uint64(n_items)) >> np.uint64(32)).astype(np.int64)
    out = np.where(w1 < np.asarray(thr, np.uint32)[j], j, np.asarray(alias, np.int64)[j])
    return out.astype(np.int32).reshape(n_users, n_sampled)


# ------------------------------------------------------------------------------------------------ weights
def weights(kind, n):
    if kind == "zipf":
        return 1.0 / np.arange(1, n + 1, dtype=np.float64)
    if kind == "uniform":
        return np.ones(n)
    if kind == "one-hot":
        w = np.zeros(n)
        w[n // 2] = 1.0
        return w
    if kind == "two-level":                      # every third item 100 times as likely; every fifth never drawn (item 0 stays)
        w = np.where(np.arange(n) % 3 == 0, 100.0, 1.0)
        w[np.arange(n) % 5 == 4] = 0.0
        return w
    raise ValueError(kind)


KINDS = ["zipf", "uniform", "one-hot", "two-level"]


# ------------------------------------------------------------------------------------------------ statistics
def chi2_z(observed, expected, dof=None):
    """tests/test_gpu_sampler_quality.py's rule: z = (chi2 - dof) / sqrt(2 dof), accepted within 5"""
    observed, expected = np.asarray(observed, np.float64).reshape(-1), np.asarray(expected, np.float64).reshape(-1)
    chi2 = float(((observed - expected) ** 2 / expected).sum())
    dof = dof if dof is not None else observed.size - 1
    return (chi2 - dof) / np.sqrt(2.0 * dof)


def pooled_cells(q, n_draws, least=50.0):
    """items -> cells of expected count >= ``least``: items in index order are pooled until the cell is full, the remainder joins the
    last cell; items of q = 0 get cell -1 (they must not appear).  Returns (cell of every item, expected count per cell)."""
    cell = np.full(q.size, -1, np.int64)
    exp, acc, k = [], 0.0, 0
    for i in np.flatnonzero(q > 0):
        cell[i] = k
        acc += q[i] * n_draws
        if acc >= least:
            exp.append(acc)
            acc, k = 0.0, k + 1
    if acc > 0:
        if exp:
            cell[cell == k] = k - 1
            exp[-1] += acc
        else:
            exp.append(acc)
    return cell, np.array(exp)


def marginal_z(samples, q):
    """z of the pooled marginal counts against the exact table q; raises if an item of q = 0 appears"""
    samples = np.asarray(samples).reshape(-1)
    cell, exp = pooled_cells(q, samples.size)
    got = cell[samples]
    assert (got >= 0).all(), "an item of probability 0 was drawn"
    return chi2_z(np.bincount(got, minlength=exp.size), exp)


def contingency_z(x, y, q, B=16):
    """independence of two draws: items are cut into B groups of (nearly) equal probability, the B x B table against n q_a q_b"""
    order = np.cumsum(q)
    group = np.minimum((order / order[-1] * B).astype(np.int64), B - 1)
    pg = np.bincount(group, weights=q, minlength=B)
    x, y = np.asarray(x).reshape(-1), np.asarray(y).reshape(-1)
    t = np.bincount(group[x] * B + group[y], minlength=B * B)
    keep = np.outer(pg, pg).reshape(-1) > 0
    return chi2_z(t[keep], (x.size * np.outer(pg, pg)).reshape(-1)[keep], dof=int(keep.sum()) - 1)
