"""
EXTENSION: host side of ``predict_top_k(..., candidates=)`` and ``predict_rank_of_interactions(..., candidates=)``
(docs/candidate_sets.md).

``candidate_csr`` turns the caller's scipy matrix into the sorted, de-duplicated int32 CSR the kernels of csrc/candidate_sets.hip
read (the convention and the code of exclusion.exclusion_csr), ``difference_csr`` takes a second CSR out of it (C \\ E, one pass of
int64 keys, no loop over users), ``cut_batches`` cuts the users into batches by stored entries so that a batch's scores and ids stay
under a byte budget, and ``long_rows`` lists the segments the wave-per-segment top-k does not take.
"""
import numpy as np

from .exclusion import exclusion_csr

SHORT_SEGMENT_MAX = 256            # csrc/candidate_sets.hip: the longest segment one wave ranks (CS_SHORT)
BATCH_BYTES = 1 << 30              # scores (4 B) + ids (4 B) of one batch of the pairs form
PAIRS_D_MAX = 256                  # the pairs form reads score_prep's fp32 operands: n_components <= 256


def candidate_csr(candidates, n_users, n_items):
    """(indptr int64 [n_users + 1], indices int32 [nnz]): every stored entry != 0 of ``candidates`` (negative values included,
    explicit zeros not, duplicates once), rows sorted; missing rows are empty sets.  ValueError for a matrix that is not scipy
    sparse or is larger than [n_users, n_items]."""
    try:
        return exclusion_csr(candidates, n_users, n_items)
    except ValueError as exc:
        raise ValueError(str(exc).replace("exclude", "candidates").replace("exclusions", "candidate sets")) from None


def row_keys(indptr, indices, n_items):
    """int64 key row * n_items + col of every entry of a canonical CSR: strictly increasing."""
    rows = np.repeat(np.arange(len(indptr) - 1, dtype=np.int64), np.diff(indptr))
    return rows * np.int64(n_items) + indices.astype(np.int64)


def difference_csr(c_indptr, c_indices, e_indptr, e_indices, n_items):
    """The canonical CSR of C \\ E for two canonical CSRs over the same users."""
    if len(c_indices) == 0 or len(e_indices) == 0:
        return c_indptr, c_indices
    c_key = row_keys(c_indptr, c_indices, n_items)
    keep = ~np.isin(c_key, row_keys(e_indptr, e_indices, n_items), assume_unique=True)
    n_users = len(c_indptr) - 1
    rows = c_key[keep] // np.int64(n_items)
    indptr = np.searchsorted(rows, np.arange(n_users + 1, dtype=np.int64)).astype(np.int64)
    return indptr, np.ascontiguousarray(c_indices[keep])


def default_user_batch(indptr, budget_bytes=BATCH_BYTES):
    """Users per batch of the pairs form when the caller names none: as many as keep an average batch's scores + ids under the
    budget -- a function of the stored entries, not of the catalogue."""
    n_users = len(indptr) - 1
    nnz = int(indptr[-1] - indptr[0])
    if n_users <= 0 or nnz * 8 <= budget_bytes:
        return max(1, n_users)
    return max(1, int(n_users * (budget_bytes / (8.0 * nnz))))


def cut_batches(indptr, user_batch_size, budget_bytes=BATCH_BYTES):
    """[(s, e), ...]: consecutive user ranges that cover every user once; a range holds at most ``user_batch_size`` users and, unless
    it is a single user, at most budget_bytes / 8 stored entries.  A user is never split."""
    n_users = len(indptr) - 1
    ubs = max(1, int(user_batch_size))
    cap = max(1, int(budget_bytes) // 8)
    out, s = [], 0
    while s < n_users:
        # the last user whose segment still ends inside the entry budget of a batch starting at s
        e = int(np.searchsorted(indptr, indptr[s] + cap, side="right")) - 1
        e = max(s + 1, min(e, s + ubs, n_users))
        out.append((s, e))
        s = e
    return out


def long_rows(indptr, s=0, e=None):
    """int32 rows (counted from ``s``) of users [s, e) whose segment is longer than SHORT_SEGMENT_MAX."""
    e = len(indptr) - 1 if e is None else e
    return np.nonzero(np.diff(indptr[s:e + 1]) > SHORT_SEGMENT_MAX)[0].astype(np.int32)


def check_call(k, item_sharded, item_offset, k_max):
    """The ValueError cases of predict_top_k(candidates=...) that need no matrix."""
    if bool(item_sharded) or int(item_offset) != 0:
        raise ValueError("predict_top_k(candidates=...) does not support item shards (item_sharded / item_offset)")
    if int(k) > int(k_max):
        raise ValueError("predict_top_k(candidates=...) supports k <= %d (got %d)" % (int(k_max), int(k)))
