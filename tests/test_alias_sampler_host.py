"""The alias sampler on the CPU: the table tensorrec.PopularitySampler builds against the restatement of tests/alias_sampler_reference.py,
the exact distribution of a table, the constructor, pickling, the entry point's argument checks, and the restatement's own draws
against the chi-square rule the GPU test applies to the kernel (so the reference alone is known to pass)."""
import ctypes
import pickle

import numpy as np
import pytest
import scipy.sparse as sp

import alias_sampler_reference as A


@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("n", A.N_ITEMS)
def test_table_implements_the_weights_exactly_enough(kind, n):
    from tensorrec_amd.tensorrec import build_alias_table, alias_table_counts
    w = A.weights(kind, n)
    thr, alias = A.build_table(w)
    got_thr, got_alias = build_alias_table(w)
    assert got_thr.dtype == np.uint32 and got_alias.dtype == np.int32
    assert np.array_equal(got_thr, thr) and np.array_equal(got_alias, alias)
    assert ((alias >= 0) & (alias < n)).all()
    counts = A.table_counts(thr, alias)
    assert sum(counts) == n << 32                                                   # exactly, in integers
    assert [int(c) for c in alias_table_counts(got_thr, got_alias)] == counts
    q, target = A.table_q(thr, alias), w / w.sum()
    assert np.abs(q - target).max() <= n * 2.0 ** -32
    assert all(c == 0 for c, wi in zip(counts, w) if wi == 0)                       # a zero weight is never drawn
    full = (alias == np.arange(n))
    assert (thr[full] == A.ONE).all()                                                # probability 1: 2^32 - 1 and its own alias


def test_constructor_counts_powers_and_errors():
    from tensorrec_amd import PopularitySampler
    counts = np.array([4.0, 0.0, 1.0, 16.0])
    s = PopularitySampler(counts, power=0.5, seed=3)
    assert s.n_items == 4 and s.seed == 3
    q = s.probabilities()
    assert np.abs(q - np.array([2, 0, 1, 4]) / 7.0).max() <= 4 * 2.0 ** -32 and q[1] == 0
    assert np.abs(PopularitySampler(counts, power=0).probabilities() - 0.25).max() <= 4 * 2.0 ** -32     # power 0: uniform
    assert np.abs(PopularitySampler(counts, power=1, smoothing=1.0).probabilities() - np.array([5, 1, 2, 17]) / 25.0).max() <= 2.0 ** -30
    m = sp.csr_matrix(np.array([[1.0, -1.0, 0.0, 2.0], [3.0, 0.0, 0.0, 1.0], [0.0, -2.0, 0.0, 0.5]], np.float32))
    sm = PopularitySampler(m, power=1.0)                                            # entries > 0 per item: 2, 0, 0, 3
    assert np.abs(sm.probabilities() - np.array([2, 0, 0, 3]) / 5.0).max() <= 2.0 ** -30
    for bad in ([1.0, -1.0], [1.0, float("nan")], [1.0, float("inf")], []):
        with pytest.raises(ValueError):
            PopularitySampler(np.array(bad))
    with pytest.raises(ValueError):
        PopularitySampler(counts, power=-0.5)
    with pytest.raises(ValueError):
        PopularitySampler(np.zeros(5))
    with pytest.raises(ValueError):
        s.sample(5, 2, 3, False, 1, "cpu")                                          # n_items disagrees: refused before any device work


def test_pickling_drops_the_device_copies():
    from tensorrec_amd import PopularitySampler
    s = PopularitySampler(A.weights("zipf", 100), seed=9)
    s._device["sentinel"] = object()                                                # stands for uploaded tensors: must not be pickled
    t = pickle.loads(pickle.dumps(s))
    assert t._device == {} and t.seed == 9 and t.n_items == 100
    assert np.array_equal(t.thr, s.thr) and np.array_equal(t.alias, s.alias)


def test_loss_graph_options_validate():
    from tensorrec_amd.loss_graphs import AbstractLossGraph, SampledSoftmaxLossGraph, BPRLossGraph, WMRBLossGraph
    assert AbstractLossGraph.wants_sample_items is False and WMRBLossGraph().wants_sample_items is False
    assert SampledSoftmaxLossGraph().wants_sample_items is False and BPRLossGraph().wants_sample_items is False
    assert SampledSoftmaxLossGraph(0.5, log_q_correction=True).wants_sample_items is True
    assert SampledSoftmaxLossGraph(remove_accidental_hits=True).wants_sample_items is True
    assert BPRLossGraph(remove_accidental_hits=True).wants_sample_items is True
    g = pickle.loads(pickle.dumps(SampledSoftmaxLossGraph(0.5, True, True)))
    assert g.log_q_correction and g.remove_accidental_hits and g.wants_sample_items and g.temperature == 0.5
    for bad in (1, "yes", None):
        with pytest.raises(ValueError):
            SampledSoftmaxLossGraph(log_q_correction=bad)
        with pytest.raises(ValueError):
            SampledSoftmaxLossGraph(remove_accidental_hits=bad)
        with pytest.raises(ValueError):
            BPRLossGraph(remove_accidental_hits=bad)


def test_entry_point_refuses_bad_arguments_before_any_launch():
    from tensorrec_amd import _native
    lib = _native.load()
    p = ctypes.c_void_p(8)
    for args in ((1, 0, 5, 3, None, p, 0, 0, p), (1, 0, 5, 3, p, None, 0, 0, p), (1, 0, 5, 3, p, p, 0, 0, None)):
        assert lib.trec_sample_items_alias(*args, None) == 1
        assert lib.trec_last_error() == b"trec_sample_items_alias: null pointer"
    for n_items, n_sampled in ((0, 3), (5, 0), (-1, 3)):
        assert lib.trec_sample_items_alias(1, 0, n_items, n_sampled, p, p, 0, 0, p, None) == 1
        assert lib.trec_last_error() == b"trec_sample_items_alias: n_items and n_sampled must be >= 1"
    assert lib.trec_sample_items_alias(0, 0, 5, 3, p, p, 0, 0, p, None) == 0        # n_users == 0: nothing to do


def test_restatement_passes_the_distribution_checks():
    """what tests/test_gpu_alias_sampler.py asks of the kernel, asked of the restatement: same shapes, seed and rule"""
    n, U, S = 1000, 2000, 100
    thr, alias = A.build_table(A.weights("zipf", n) ** 0.75)
    q = A.table_q(thr, alias)
    a = A.draw(U, n, S, thr, alias, seed=4242, step=5)
    b = A.draw(U, n, S, thr, alias, seed=4242, step=6)
    assert abs(A.marginal_z(a, q)) <= 5.0
    assert abs(A.contingency_z(a[:, : S // 2], a[:, S // 2:], q)) <= 5.0
    assert abs(A.contingency_z(a, b, q)) <= 5.0
    assert abs(A.contingency_z(a[:-1], a[1:], q)) <= 5.0
    thr_u, alias_u = A.build_table(np.ones(n))
    assert abs(A.marginal_z(A.draw(U, n, S, thr_u, alias_u, seed=4242, step=5), np.full(n, 1.0 / n))) <= 5.0
    thr_z, alias_z = A.build_table(A.weights("two-level", n))
    qz = A.table_q(thr_z, alias_z)
    drawn = A.draw(U, n, S, thr_z, alias_z, seed=4242, step=5)
    assert (qz[drawn] > 0).all() and abs(A.marginal_z(drawn, qz)) <= 5.0
