"""Host side of the exclusions (tensorrec_amd/exclusion.py): the CSR the kernels binary-search, and the over-fetch policy k' of
tier 1 -- capped at what the route that k selects accepts, so that excluding items never moves a call onto another route."""
import numpy as np
import pytest
import scipy.sparse as sp

from tensorrec_amd import exclusion as X


def _rows(indptr, indices):
    return [list(indices[indptr[u]:indptr[u + 1]]) for u in range(len(indptr) - 1)]


def test_csr_sorts_dedups_and_keeps_nonzero_values_only():
    # COO with duplicates, unsorted columns, an explicit zero, a negative value and a pair that sums to zero
    r = np.array([0, 0, 0, 1, 1, 2, 2, 2])
    c = np.array([5, 1, 5, 3, 0, 4, 4, 2])
    v = np.array([1., 2., 1., 0., -1., 1., -1., 3.], np.float32)
    m = sp.coo_matrix((v, (r, c)), shape=(3, 6))
    indptr, indices = X.exclusion_csr(m, 4, 8)
    assert indptr.dtype == np.int64 and indices.dtype == np.int32
    assert indptr.shape == (5,)                       # (the fourth user is beyond the matrix: nothing excluded)
    # row 1: the explicit zero at 3 is not excluded, the negative at 0 is; row 2: (2, 4) is stored twice, each entry != 0
    assert _rows(indptr, indices) == [[1, 5], [0], [2, 4], []]


@pytest.mark.parametrize("fmt", ["csr", "csc", "coo", "lil"])
def test_csr_any_scipy_format(fmt):
    rng = np.random.default_rng(0)
    dense = (rng.random((7, 9)) < 0.3) * rng.choice([-2., 1., 3.], size=(7, 9))
    m = sp.csr_matrix(dense).asformat(fmt)
    indptr, indices = X.exclusion_csr(m, 7, 9)
    assert _rows(indptr, indices) == [list(np.nonzero(dense[u])[0]) for u in range(7)]


def test_csr_csr_with_explicit_zeros_and_unsorted_indices():
    m = sp.csr_matrix((np.array([0., 1., 1.]), np.array([4, 2, 0]), np.array([0, 3])), shape=(1, 5))
    assert not m.has_sorted_indices
    indptr, indices = X.exclusion_csr(m, 1, 5)
    assert _rows(indptr, indices) == [[0, 2]]


def test_csr_smaller_shape_and_empty():
    indptr, indices = X.exclusion_csr(sp.csr_matrix((2, 3)), 5, 10)
    assert list(indptr) == [0] * 6 and len(indices) == 0
    indptr, indices = X.exclusion_csr(sp.csr_matrix(np.array([[0, 0, 1.]])), 5, 10)
    assert _rows(indptr, indices) == [[2], [], [], [], []]


def test_csr_rejects_malformed_input():
    with pytest.raises(ValueError):
        X.exclusion_csr(sp.csr_matrix((6, 3)), 5, 10)          # more rows than users
    with pytest.raises(ValueError):
        X.exclusion_csr(sp.csr_matrix((5, 11)), 5, 10)         # more columns than items
    with pytest.raises(ValueError):
        X.exclusion_csr(np.zeros((2, 2)), 5, 10)               # not a scipy matrix


def test_fetch_k_caps_per_route():
    for route in ("direct", "two_stage", "cascade_int8", "bf16_filter"):
        assert X.fetch_k(route, 10, 3) == 13
        assert X.fetch_k(route, 10, 64) == 16
        assert X.fetch_k(route, 16, 5) == 16                   # k at the cap: k' = k
        assert X.fetch_k(route, 1, 1000) == 16
    assert X.fetch_k("euclid_certified", 10, 50) == 12         # the narrow certified route stays narrow
    assert X.fetch_k("euclid_certified", 12, 50) == 12
    assert X.fetch_k("euclid_certified", 13, 50) == 48         # ... and the wide one stays below its limit
    assert X.fetch_k("euclid_certified", 20, 3) == 23
    assert X.fetch_k("wide_cascade", 32, 20) == 52
    assert X.fetch_k("wide_cascade", 32, 1000) == 64
    assert X.fetch_k("wide_cascade", 64, 1) == 64
    assert X.fetch_k("slab", 100, 1000) == 100                 # the slab route masks its slabs: no over-fetch


def test_fetch_k_no_exclusions_in_the_batch():
    for route in ("direct", "cascade_int8", "euclid_certified", "wide_cascade", "slab"):
        assert X.fetch_k(route, 10 if route != "wide_cascade" else 20, 0) == (10 if route != "wide_cascade" else 20)
    indptr, _ = X.exclusion_csr(sp.csr_matrix(np.array([[0, 1.], [0, 0], [0, 0], [1, 1]])), 4, 2)
    assert X.max_excluded(indptr, 1, 3) == 0 and X.max_excluded(indptr, 0, 4) == 2 and X.max_excluded(indptr, 2, 2) == 0
    assert X.fetch_k("direct", 10, X.max_excluded(indptr, 1, 3)) == 10


def test_fetch_k_never_leaves_the_route_family():
    """k' never exceeds the largest k of the route k picked -- whatever the exclusions, for every k that route takes."""
    families = {"direct": range(1, 17), "cascade_int8": range(1, 17), "wide_cascade": range(17, 65),
                "euclid_certified": list(range(1, 13)) + list(range(13, 49))}
    for route, ks in families.items():
        for k in ks:
            for e in (0, 1, 5, 40, 10 ** 6):
                kk = X.fetch_k(route, k, e)
                assert k <= kk <= X.fetch_cap(route, k)
                if route == "euclid_certified":
                    assert (k <= 12) == (kk <= 12)


def test_overlap_count():
    indptr, indices = X.exclusion_csr(sp.csr_matrix(np.array([[0, 1., 1.], [1., 0, 0]])), 2, 3)
    assert X.overlap_count(indptr, indices, np.array([0, 0, 1]), np.array([0, 2, 0])) == 2
    assert X.overlap_count(indptr, indices, np.array([0]), np.array([0])) == 0
