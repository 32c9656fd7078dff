"""Host side of the candidate-set calls (tensorrec_amd/candidate_sets.py, docs/candidate_sets.md): CSR canonicalisation, C \\ E,
batch cutting by stored entries, the short / long split and the argument errors.  No GPU."""
import numpy as np
import pytest
import scipy.sparse as sp

from tensorrec_amd import candidate_sets as cs


def test_canonicalisation():
    # unsorted, a duplicate (3, 7), an explicit zero at (0, 5), a negative value at (1, 2); fewer rows and columns than the features
    r = np.array([3, 0, 3, 1, 0, 3, 0])
    c = np.array([7, 9, 1, 2, 5, 7, 4])
    v = np.array([1.0, 2.0, 1.0, -1.0, 0.0, 1.0, 3.0], np.float32)
    m = sp.coo_matrix((v, (r, c)), shape=(4, 10))
    indptr, indices = cs.candidate_csr(m, 6, 12)
    assert indptr.dtype == np.int64 and indices.dtype == np.int32
    assert indptr.tolist() == [0, 2, 3, 3, 5, 5, 5]
    assert indices.tolist() == [4, 9, 2, 1, 7]
    # a canonical csr comes back as it is
    can = sp.csr_matrix(m)
    can.sum_duplicates()
    can.eliminate_zeros()
    can.sort_indices()
    p2, i2 = cs.candidate_csr(can, 6, 12)
    assert p2.tolist() == indptr.tolist() and i2.tolist() == indices.tolist()
    # an empty matrix: every set empty
    p3, i3 = cs.candidate_csr(sp.csr_matrix((0, 0), dtype=np.float32), 3, 3)
    assert p3.tolist() == [0, 0, 0, 0] and len(i3) == 0


def test_difference_against_python_sets():
    nu, ni = 50, 300
    c = sp.random(nu, ni, density=0.2, random_state=1, format="csr", dtype=np.float32)
    e = sp.random(nu, ni, density=0.3, random_state=2, format="csr", dtype=np.float32)
    c, e = c.tolil(), e.tolil()
    c[3, :] = 0                                 # an empty candidate row
    e[5, :] = c[5, :]                           # exclusions that empty a row
    e[6, :] = 1.0
    e[7, :] = 0                                 # nothing excluded
    c, e = sp.csr_matrix(c), sp.csr_matrix(e)
    cp, ci = cs.candidate_csr(c, nu, ni)
    ep, ei = cs.candidate_csr(e, nu, ni)
    dp, di = cs.difference_csr(cp, ci, ep, ei, ni)
    assert dp.dtype == np.int64 and di.dtype == np.int32 and len(dp) == nu + 1
    for u in range(nu):
        want = sorted(set(ci[cp[u]:cp[u + 1]].tolist()) - set(ei[ep[u]:ep[u + 1]].tolist()))
        assert di[dp[u]:dp[u + 1]].tolist() == want
    assert dp[6] == dp[5] == dp[7] and dp[4] == dp[3]
    # nothing to take away: the same arrays
    p0, i0 = cs.difference_csr(cp, ci, np.zeros(nu + 1, np.int64), np.zeros(0, np.int32), ni)
    assert p0 is cp and i0 is ci


@pytest.mark.parametrize("ubs,budget", [(7, 1 << 30), (1000, 8 * 50), (3, 8 * 20), (1, 8), (1000, 1 << 30)])
def test_batches_cover_every_user_once(ubs, budget):
    rng = np.random.default_rng(3)
    lens = rng.integers(0, 40, size=101)
    lens[10] = 500                              # one user beyond any small budget: a batch of its own, never split
    lens[50:60] = 0
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    batches = cs.cut_batches(indptr, ubs, budget)
    assert batches[0][0] == 0 and batches[-1][1] == 101
    for (s, e), nxt in zip(batches, batches[1:] + [(101, None)]):
        assert s < e <= s + ubs and e == nxt[0]
        assert e - s == 1 or (indptr[e] - indptr[s]) * 8 <= budget
    assert cs.cut_batches(np.zeros(1, np.int64), 5) == []


def test_default_batch_follows_stored_entries():
    indptr = np.arange(0, 1001 * 1000, 1000, dtype=np.int64)          # 1,000 users x 1,000 candidates
    assert cs.default_user_batch(indptr) == 1000
    assert cs.default_user_batch(indptr, budget_bytes=8 * 1000 * 100) == 100
    assert cs.default_user_batch(np.zeros(1, np.int64)) == 1


def test_short_long_split():
    lens = np.array([0, 1, 256, 257, 0, 5000, 256])
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    lr = cs.long_rows(indptr)
    assert lr.dtype == np.int32 and lr.tolist() == [3, 5]
    assert cs.long_rows(indptr, 2, 6).tolist() == [1, 3]           # (counted from the batch's first user)
    assert cs.long_rows(indptr, 0, 3).tolist() == []
    assert cs.SHORT_SEGMENT_MAX == 256


def test_value_errors():
    with pytest.raises(ValueError, match="item shards"):
        cs.check_call(10, True, 0, 1024)
    with pytest.raises(ValueError, match="item shards"):
        cs.check_call(10, False, 5, 1024)
    with pytest.raises(ValueError, match="k <= 1024"):
        cs.check_call(1025, False, 0, 1024)
    cs.check_call(1024, False, 0, 1024)
    ok = sp.identity(4, dtype=np.float32, format="csr")
    with pytest.raises(ValueError, match="candidates of shape"):
        cs.candidate_csr(ok, 3, 4)
    with pytest.raises(ValueError, match="candidates of shape"):
        cs.candidate_csr(ok, 4, 3)
    with pytest.raises(ValueError, match="candidates must be a scipy sparse matrix"):
        cs.candidate_csr(np.eye(3), 3, 3)
