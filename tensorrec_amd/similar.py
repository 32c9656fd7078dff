"""
EXTENSION: host side of ``predict_similar_items_top_k`` (docs/similar_items.md) -- pure NumPy, no GPU.

``query_ids`` validates the caller's item ids before anything is launched and normalises them to the two forms the device
side reads (int64 to gather representation rows, int32 to compare against the ids of the top-k lists); ``k_fetch`` is how many
places the fused routes are asked for; ``batch_plan`` the query batches a given ``item_batch_size`` walks.
"""
import numpy as np


def check_k(k):
    """``k`` as an int; ValueError below 1."""
    if int(k) < 1:
        raise ValueError("predict_similar_items_top_k needs k >= 1 (got %r)" % (k,))
    return int(k)


def query_ids(item_ids, n_items):
    """(ids int64 [Q], ids int32 [Q], all_items) of the query items.  ``item_ids`` None: every item in order (``all_items`` True --
    the caller slices the item representation instead of gathering a copy of it).  Otherwise any integer sequence or array;
    repeats are allowed and the order is kept.  An id outside [0, n_items) raises ValueError."""
    n_items = int(n_items)
    if n_items > np.iinfo(np.int32).max:
        raise ValueError("item ids must fit int32")
    if item_ids is None:
        ids = np.arange(n_items, dtype=np.int64)
        return ids, ids.astype(np.int32), True
    ids = np.asarray(item_ids)
    if ids.ndim != 1:
        raise ValueError("item_ids must be one-dimensional (got shape %s)" % (ids.shape,))
    if ids.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int32), False
    if ids.dtype == np.bool_ or not np.issubdtype(ids.dtype, np.integer):
        raise ValueError("item_ids must be integers (got dtype %s)" % ids.dtype)
    lo, hi = int(ids.min()), int(ids.max())
    if lo < 0 or hi >= n_items:
        raise ValueError("item_ids must lie in [0, %d) (got %d)" % (n_items, lo if lo < 0 else hi))
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    return ids, ids.astype(np.int32), False


def k_fetch(k, exclude_self, slab_route=False):
    """Places the route is chosen for and asked for: k + 1 with ``exclude_self`` -- a query is (almost) always its own best match,
    so k places would leave every row one short -- except on the slab route, whose score slabs are masked directly."""
    return int(k) + 1 if exclude_self and not slab_route else int(k)


def batch_plan(n_queries, item_batch_size):
    """[(start, end), ...] of the query batches ``item_batch_size`` walks (ValueError below 1); the whole range as one batch for
    None, where the device's free memory decides at run time.  No batch is empty, so no queries means no batches."""
    n = int(n_queries)
    if item_batch_size is None:
        return [(0, n)] if n > 0 else []
    size = int(item_batch_size)
    if size < 1:
        raise ValueError("item_batch_size must be >= 1 (got %r)" % (item_batch_size,))
    return [(s, min(s + size, n)) for s in range(0, n, size)]
