"""The float64 reference of the hard-negative selection (csrc/sampler_hard.hip, docs/hard_negatives.md) and what the tests around it
share: the definition as a plain per-user Python sort, a float32 restatement of the scores in two summation orders, the score bar
for generic inputs, and makers of dyadic inputs on which every float32 order is exact.

THE DEFINITION.  User u with candidates c_0 .. c_{M-1}:
  score  y_j = sum_k U[u,k] V[c_j,k] (+ item_bias[c_j]); the user bias is constant per user and does not enter.
  hit    with ``exclude``: c_j is the column of an interaction of u with pos_slot >= 0.
  order  non-hits before hits; non-hits by descending score (NaN counts as -inf), equal scores by ascending position j; hits by
         ascending j.  The same item at two positions is two candidates.
  row    slots [0, H): the first H candidates of that order.  Slots [H, S): the first S - H of the REMAINING candidates in the order
         "non-hits before hits, ascending j".

THE BAR of a float32 score against the float64 one: bar_j = 2 gamma_d sum_k |u_k v_k| + 2^-23 |y_j| with gamma_d = d 2^-24 /
(1 - d 2^-24) -- a float32 dot product of d terms in ANY order (fused or not) is within gamma_d sum |u_k v_k| (Higham, Accuracy and
Stability of Numerical Algorithms, section 3.1; the unit roundoff of float32 is 2^-24), the factor 2 leaves room for the bias addition
and the comparison of two such scores, and 2^-23 |y| covers the rounding of the result itself.  Derived from the format, not tuned.
"""
import numpy as np

F32_U = 2.0 ** -24


def f64(a):
    return np.asarray(a, dtype=np.float64)


# ------------------------------------------------------------------------------------------------ scores
def scores64(U, V, ib, C):
    """float64 [n_users, M]: y[u, j] = U[u] . V[C[u, j]] (+ ib[C[u, j]]); NaN / inf propagate as IEEE says"""
    U, V, C = f64(U), f64(V), np.asarray(C, dtype=np.int64)
    y = np.zeros(C.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        for u in range(C.shape[0]):                    # (per user: V[C] as a whole is n_users * M * d numbers)
            y[u] = V[C[u]] @ U[u]
        if ib is not None:
            y = y + f64(ib).reshape(-1)[C]
    return y


def abs_scores64(U, V, C):
    """float64 [n_users, M]: sum_k |U[u, k] V[C[u, j], k]|"""
    C, aU, aV = np.asarray(C, dtype=np.int64), np.abs(f64(U)), np.abs(f64(V))
    a = np.zeros(C.shape)
    for u in range(C.shape[0]):
        a[u] = aV[C[u]] @ aU[u]
    return a


def score_bar(U, V, ib, C):
    d = np.asarray(U).shape[1]
    gamma = d * F32_U / (1.0 - d * F32_U)
    return 2.0 * gamma * abs_scores64(U, V, C) + 2.0 ** -23 * np.abs(scores64(U, V, ib, C))


def scores32_forward(U, V, ib, C):
    """float32, one product and one add at a time, k ascending, the bias last"""
    U, V, C = np.asarray(U, np.float32), np.asarray(V, np.float32), np.asarray(C, dtype=np.int64)
    acc = np.zeros(C.shape, np.float32)
    for k in range(U.shape[1]):
        acc = (acc + (U[:, k:k + 1] * V[C, k]).astype(np.float32)).astype(np.float32)
    if ib is not None:
        acc = (acc + np.asarray(ib, np.float32).reshape(-1)[C]).astype(np.float32)
    return acc


def scores32_pairwise(U, V, ib, C):
    """float32, the bias FIRST, then the products added as a halving tree from the far end"""
    U, V, C = np.asarray(U, np.float32), np.asarray(V, np.float32), np.asarray(C, dtype=np.int64)
    terms = [(U[:, k:k + 1] * V[C, k]).astype(np.float32) for k in reversed(range(U.shape[1]))]
    while len(terms) > 1:
        nxt = [(terms[i] + terms[i + 1]).astype(np.float32) for i in range(0, len(terms) - 1, 2)]
        if len(terms) % 2:
            nxt.append(terms[-1])
        terms = nxt
    acc = terms[0]
    if ib is not None:
        acc = (np.asarray(ib, np.float32).reshape(-1)[C] + acc).astype(np.float32)
    return acc


# ------------------------------------------------------------------------------------------------ hits and the selection
def hits_of(indptr, x_item, pos_slot, C, exclude=True):
    """bool [n_users, M]: candidate j of user u is the column of an interaction of u with pos_slot >= 0"""
    C = np.asarray(C)
    hit = np.zeros(C.shape, bool)
    if not exclude:
        return hit
    for u in range(C.shape[0]):
        b, e = int(indptr[u]), int(indptr[u + 1])
        positives = set(int(c) for c, s in zip(x_item[b:e], pos_slot[b:e]) if s >= 0)
        hit[u] = [int(c) in positives for c in C[u]]
    return hit


def select_positions(y, hit, S, H):
    """The positions j of one user's output row: a plain sort on the tuple (hit, -score, j), then the tail by (hit, j)"""
    M = len(y)
    value = [float("-inf") if np.isnan(v) else float(v) for v in y]
    order = sorted(range(M), key=lambda j: (bool(hit[j]), 0.0 if hit[j] else -value[j], j))
    hard = order[:H]
    chosen = set(hard)
    rest = sorted((j for j in range(M) if j not in chosen), key=lambda j: (bool(hit[j]), j))
    return hard + rest[:S - H]


def select(y, hit, C, S, H=None):
    """(items int32 [n_users, S], positions int64 [n_users, S]) of the definition from scores y and hit flags"""
    C = np.asarray(C)
    H = S if H is None else H
    assert 1 <= H <= S <= C.shape[1]
    pos = np.zeros((C.shape[0], S), np.int64)
    for u in range(C.shape[0]):
        pos[u] = select_positions(y[u], hit[u], S, H)
    items = np.take_along_axis(C, pos, axis=1).astype(np.int32) if C.shape[0] else np.zeros((0, S), np.int32)
    return items, pos


def reference(U, V, ib, indptr, x_item, pos_slot, C, S, H=None, exclude=True):
    """(items, positions, float64 scores, hits) of the definition"""
    y = scores64(U, V, ib, C)
    hit = hits_of(indptr, x_item, pos_slot, C, exclude)
    items, pos = select(y, hit, C, S, H)
    return items, pos, y, hit


def check_within_bar(out, C, y, bar, hit, S, H):
    """What a float32 selection ``out`` (items, int [n_users, S]) must satisfy on generic inputs, given the float64 scores ``y``, their
    bars and the hits.  With t the float64 score of the H-th non-hit: every hard slot is a distinct non-hit candidate position with
    y >= t - bar, every unselected non-hit has y <= t + bar, the hard slots are ordered within bar, and the tail is EXACTLY the first
    S - H unselected positions by (hit, j).  Rows with fewer than H non-hits are compared exactly.  Returns the largest
    violation / bar seen (<= 1 passes); raises AssertionError otherwise."""
    C = np.asarray(C)
    worst = 0.0
    for u in range(C.shape[0]):
        clear = np.flatnonzero(~hit[u])
        if len(clear) < H or not np.isfinite(y[u]).all():
            want = C[u][select_positions(y[u], hit[u], S, H)]
            assert np.array_equal(out[u], want), "user %d: rows with hits among the hard slots / non-finite scores are exact" % u
            continue
        t = np.sort(y[u][clear])[::-1][H - 1]
        # positions of the hard slots: the item may stand at several positions -- take, per slot, the unused position of that item whose
        # score is largest (equal items score equally: any is the same candidate up to position)
        used, hard = set(), []
        for s in range(H):
            cands = [j for j in clear if C[u, j] == out[u, s] and j not in used]
            assert cands, "user %d slot %d: item %d is no unused non-hit candidate" % (u, s, out[u, s])
            j = cands[0]
            used.add(j)
            hard.append(j)
        for s, j in enumerate(hard):
            slack = (t - bar[u, j]) - y[u, j]
            worst = max(worst, (t - y[u, j]) / bar[u, j] if bar[u, j] > 0 else 0.0)
            assert slack <= 0, "user %d slot %d: score %.9g below t - bar = %.9g" % (u, s, y[u, j], t - bar[u, j])
            if s:
                i = hard[s - 1]
                assert y[u, i] + bar[u, i] >= y[u, j] - bar[u, j], "user %d: hard slots %d, %d out of order beyond the bars" % (u, s - 1, s)
        for j in clear:
            if j not in used:
                worst = max(worst, (y[u, j] - t) / bar[u, j] if bar[u, j] > 0 else 0.0)
                assert y[u, j] <= t + bar[u, j], "user %d: unselected position %d scores %.9g above t + bar" % (u, j, y[u, j])
        rest = sorted((j for j in range(C.shape[1]) if j not in used), key=lambda j: (bool(hit[u, j]), j))[:S - H]
        assert np.array_equal(out[u, H:], C[u, rest]), "user %d: the tail is not the first unselected positions" % u
    return worst


# ------------------------------------------------------------------------------------------------ dyadic inputs
def dyadic_tables(rng, n_users, n_items, d, biased=True):
    """U, V with entries k / 8, |k| <= 16, and item biases k / 64, |k| <= 16: every product is a multiple of 1/64 below 4, every sum of up
    to 256 of them (and the bias) is below 2^11 with 6 fractional bits -- exact in float32 in any order; ties are frequent"""
    U = (rng.integers(-16, 17, size=(n_users, d)) / 8.0).astype(np.float32)
    V = (rng.integers(-16, 17, size=(n_items, d)) / 8.0).astype(np.float32)
    ib = (rng.integers(-16, 17, size=n_items) / 64.0).astype(np.float32) if biased else None
    return U, V, ib


def interaction_rows(rng, n_items, lengths, negative_share=0.25):
    """CSR rows of the given lengths: sorted distinct columns, pos_slot >= 0 (running) or -1 for about ``negative_share`` of them"""
    indptr, cols, slots, k = [0], [], [], 0
    for n in lengths:
        c = np.sort(rng.choice(n_items, size=n, replace=False)).astype(np.int32)
        neg = rng.random(n) < negative_share
        for col, ng in zip(c, neg):
            cols.append(col)
            slots.append(-1 if ng else k)
            k += 0 if ng else 1
        indptr.append(len(cols))
    return np.asarray(indptr, np.int64), np.asarray(cols, np.int32), np.asarray(slots, np.int32)


def candidates_with_planted_hits(rng, n_items, indptr, x_item, M, share=0.25, duplicates=True):
    """int32 [n_users, M]: uniform draws with replacement (duplicates happen), about ``share`` of each row replaced by columns of
    the user's own interactions (positives and non-positives alike)"""
    n_users = len(indptr) - 1
    C = rng.integers(0, n_items, size=(n_users, M)).astype(np.int32)
    for u in range(n_users):
        row = x_item[indptr[u]:indptr[u + 1]]
        if len(row):
            where = np.flatnonzero(rng.random(M) < share)
            C[u, where] = rng.choice(row, size=len(where))
        if duplicates and M >= 4:
            C[u, M - 1] = C[u, 0]
    return C
