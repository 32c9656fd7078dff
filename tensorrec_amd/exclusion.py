"""
EXTENSION: host side of ``predict_top_k(..., exclude=)`` and ``predict_rank_of_interactions(..., exclude=)`` (docs/exclusion.md).

``exclusion_csr`` turns the caller's scipy matrix into the sorted, de-duplicated int32 CSR the kernels of csrc/exclude.hip
binary-search; ``fetch_k`` is the over-fetch policy of tier 1: how many places the route that ``k`` selects is asked for so that
the first k non-excluded items are usually inside its list, never more than that route accepts.
"""
import numpy as np
import scipy.sparse as sp

from . import topk_plan


def exclusion_csr(exclude, n_users, n_items):
    """(indptr int64 [n_users + 1], indices int32 [nnz]) of the entries of ``exclude`` whose stored value is != 0 -- negative
    values included (a negative interaction is "seen" too), explicit zeros not, duplicates once.  Every row is sorted.
    ``exclude`` may be any scipy sparse matrix of at most [n_users, n_items]: missing rows and columns exclude nothing."""
    if not sp.issparse(exclude):
        raise ValueError("exclude must be a scipy sparse matrix (got %s)" % type(exclude).__name__)
    n_rows, n_cols = exclude.shape
    if n_rows > n_users or n_cols > n_items:
        raise ValueError("exclude of shape %s does not fit the feature matrices (%d users x %d items)"
                         % (exclude.shape, n_users, n_items))
    if n_items > np.iinfo(np.int32).max:
        raise ValueError("exclusions need item ids that fit int32")
    if sp.isspmatrix_csr(exclude) and exclude.has_canonical_format and bool(np.all(exclude.data != 0)):
        # already what the kernels read (sorted rows, no duplicates, no explicit zeros): no host sort of every entry
        indptr = np.empty(n_users + 1, np.int64)
        indptr[:n_rows + 1] = exclude.indptr
        indptr[n_rows + 1:] = exclude.indptr[-1]
        return indptr, exclude.indices.astype(np.int32, copy=False)
    coo = exclude.tocoo()                                   # (keeps duplicates: each stored entry counts on its own)
    keep = np.asarray(coo.data) != 0
    r = np.asarray(coo.row)[keep].astype(np.int64)
    c = np.asarray(coo.col)[keep].astype(np.int64)
    if r.size and (r.min() < 0 or c.min() < 0 or r.max() >= n_rows or c.max() >= n_cols):
        raise ValueError("exclude holds indices outside its shape")
    key = np.unique(r * np.int64(n_items) + c)              # sorted: row-major, columns ascending, duplicates merged
    rows = key // n_items
    indices = (key - rows * n_items).astype(np.int32)
    indptr = np.searchsorted(rows, np.arange(n_users + 1, dtype=np.int64)).astype(np.int64)
    return indptr, indices


def fetch_cap(route, k):
    """Largest k the route ``route`` (predict_top_k's last_route["route"] for this k) accepts -- over-fetching stays inside the
    route family that k selected; None for the slab route, which masks its score slabs directly and fetches nothing extra."""
    return topk_plan.route_cap(route, k)


def fetch_k(route, k, max_excluded):
    """k' of tier 1: ``k`` plus the most exclusions any user of the batch has, capped at what the same route accepts; ``k`` itself
    when the batch excludes nothing, k is already at the cap, or the route is the slab route."""
    cap = fetch_cap(route, k)
    if cap is None or int(max_excluded) <= 0:
        return int(k)
    return max(int(k), min(cap, int(k) + int(max_excluded)))


def max_excluded(indptr, s, e):
    """The most exclusions of one user among users [s, e)."""
    if e <= s:
        return 0
    return int(np.diff(indptr[s:e + 1]).max())


def overlap_count(indptr, indices, rows, cols):
    """How many of the pairs (rows, cols) are also in the exclusion CSR."""
    if len(rows) == 0 or len(indices) == 0:
        return 0
    n_cols = int(max(int(np.max(cols)), int(indices.max()))) + 1
    ex_rows = np.repeat(np.arange(len(indptr) - 1, dtype=np.int64), np.diff(indptr))
    ex_key = ex_rows * n_cols + indices.astype(np.int64)
    key = np.asarray(rows, np.int64) * n_cols + np.asarray(cols, np.int64)
    return int(np.isin(key, ex_key).sum())
