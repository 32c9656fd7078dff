"""tests/hard_negative_reference.py on the CPU: the definition against a second, independent formulation (stable argsorts and masks
instead of a tuple sort), both float32 summation orders equal to float64 on the dyadic inputs, seeded defects that the comparison
must catch, and the host side of HardNegativeSampler: its constructor, the TypeError of plain ``sample``, pickling, the coverage
query, and the two ``scored_sampler`` keywords of step_plan."""
import pickle

import numpy as np
import pytest

import hard_negative_reference as R


def make_case(seed, n_users=9, n_items=40, d=8, M=24, biased=True, lengths=None):
    rng = np.random.default_rng(seed)
    U, V, ib = R.dyadic_tables(rng, n_users, n_items, d, biased)
    lengths = lengths if lengths is not None else [int(x) for x in rng.integers(0, 12, size=n_users)]
    indptr, x_item, pos_slot = R.interaction_rows(rng, n_items, lengths)
    C = R.candidates_with_planted_hits(rng, n_items, indptr, x_item, M)
    return U, V, ib, indptr, x_item, pos_slot, C


def select_by_argsort(y, hit, C, S, H):
    """The definition again without tuples: a stable argsort of the negated scores puts equal scores in ascending position; a stable
    argsort of the hit flags then puts the hits last without disturbing either group -- but hits are ordered by POSITION, so their
    scores are levelled first.  The tail: a mask of what is left, stable-sorted by the hit flag."""
    out = np.zeros((C.shape[0], S), np.int64)
    for u in range(C.shape[0]):
        v = np.where(np.isnan(y[u]), -np.inf, y[u])
        v = np.where(hit[u], 0.0, v)
        by_score = np.argsort(-v, kind="stable")
        order = by_score[np.argsort(hit[u][by_score], kind="stable")]
        left = np.ones(C.shape[1], bool)
        left[order[:H]] = False
        rest = np.flatnonzero(left)
        rest = rest[np.argsort(hit[u][rest], kind="stable")]
        out[u] = np.concatenate([order[:H], rest[:S - H]])
    return out


@pytest.mark.parametrize("exclude", [True, False])
@pytest.mark.parametrize("S,H", [(1, 1), (12, 1), (12, 6), (12, 12), (24, 24), (24, 7)])
def test_reference_against_argsort_formulation(S, H, exclude):
    for seed in range(4):
        U, V, ib, indptr, x_item, pos_slot, C = make_case(seed)
        items, pos, y, hit = R.reference(U, V, ib, indptr, x_item, pos_slot, C, S, H, exclude)
        assert exclude == bool(hit.any())
        if seed == 1:                                            # a NaN, a -inf and an all-equal row
            y[0, 3], y[0, 5] = np.nan, -np.inf
            y[1, :] = 0.25
            items, pos = R.select(y, hit, C, S, H)
        assert np.array_equal(pos, select_by_argsort(y, hit, C, S, H))
        assert np.array_equal(items, np.take_along_axis(C, pos, axis=1))
        for u in range(C.shape[0]):
            assert len(set(pos[u])) == S                          # positions, not items, are distinct
            n_clear = int((~hit[u]).sum())
            assert not hit[u][pos[u][:min(S, n_clear)]].any() and hit[u][pos[u][min(S, n_clear):]].all()


def test_float32_orders_are_exact_on_dyadic_inputs():
    for d in (4, 64, 132, 256):
        U, V, ib, _, _, _, C = make_case(d, n_users=5, n_items=30, d=d, M=16)
        y = R.scores64(U, V, ib, C)
        assert np.abs(y).max() < 2 ** 11 and np.array_equal(y * 64, np.round(y * 64))
        assert np.array_equal(R.scores32_forward(U, V, ib, C).astype(np.float64), y)
        assert np.array_equal(R.scores32_pairwise(U, V, ib, C).astype(np.float64), y)
        ties = sum(len(row) - len(set(row)) for row in y)
        assert d > 4 or ties > 0                                  # (few columns: ties are frequent)


def test_float32_orders_lie_within_the_bar_on_gaussian_inputs():
    rng = np.random.default_rng(5)
    U, V = rng.standard_normal((6, 128)).astype(np.float32), rng.standard_normal((50, 128)).astype(np.float32)
    ib = rng.standard_normal(50).astype(np.float32)
    C = rng.integers(0, 50, size=(6, 32))
    y, bar = R.scores64(U, V, ib, C), R.score_bar(U, V, ib, C)
    for f in (R.scores32_forward, R.scores32_pairwise):
        assert (np.abs(f(U, V, ib, C).astype(np.float64) - y) <= 0.5 * bar).all()


def defect_ties_descending(y, hit, C, S, H):
    pos = np.zeros((C.shape[0], S), np.int64)
    for u in range(C.shape[0]):
        order = sorted(range(C.shape[1]), key=lambda j: (bool(hit[u, j]), 0.0 if hit[u, j] else -y[u, j], -j))
        rest = sorted((j for j in range(C.shape[1]) if j not in set(order[:H])), key=lambda j: (bool(hit[u, j]), j))
        pos[u] = order[:H] + rest[:S - H]
    return pos


def defect_hits_not_last(y, hit, C, S, H):
    return R.select(y, np.zeros_like(hit), C, S, H)[1]


def defect_tail_from_selected(y, hit, C, S, H):
    pos = R.select(y, hit, C, S, H)[1]
    for u in range(C.shape[0]):
        rest = sorted(range(C.shape[1]), key=lambda j: (bool(hit[u, j]), j))
        pos[u, H:] = rest[:S - H]
    return pos


def defect_nan_first(y, hit, C, S, H):
    return R.select(np.where(np.isnan(y), np.inf, y), hit, C, S, H)[1]


@pytest.mark.parametrize("defect", [defect_ties_descending, defect_hits_not_last, defect_tail_from_selected, defect_nan_first],
                         ids=lambda f: f.__name__)
def test_seeded_defects_are_caught(defect):
    U, V, ib, indptr, x_item, pos_slot, C = make_case(2, d=4)
    S, H = 12, 6
    items, pos, y, hit = R.reference(U, V, ib, indptr, x_item, pos_slot, C, S, H)
    y[0, 3] = np.nan
    items, pos = R.select(y, hit, C, S, H)
    wrong = np.take_along_axis(C, defect(y, hit, C, S, H), axis=1)
    assert not np.array_equal(wrong, items)
    if defect is not defect_nan_first and defect is not defect_ties_descending:
        with pytest.raises(AssertionError):                      # the check for generic inputs sees these too
            finite = np.where(np.isnan(y), 0.0, y)
            wrong = np.take_along_axis(C, defect(finite, hit, C, S, H), axis=1)
            R.check_within_bar(wrong, C, finite, np.zeros_like(finite), hit, S, H)


def test_check_within_bar_accepts_the_reference_and_near_ties():
    rng = np.random.default_rng(3)
    U, V = rng.standard_normal((5, 16)).astype(np.float32), rng.standard_normal((60, 16)).astype(np.float32)
    indptr, x_item, pos_slot = R.interaction_rows(rng, 60, [0, 3, 9, 1, 20])
    C = R.candidates_with_planted_hits(rng, 60, indptr, x_item, 40)
    items, pos, y, hit = R.reference(U, V, None, indptr, x_item, pos_slot, C, 10, 5)
    bar = R.score_bar(U, V, None, C)
    assert R.check_within_bar(items, C, y, bar, hit, 10, 5) <= 1.0
    y32 = R.scores32_forward(U, V, None, C).astype(np.float64)          # a float32 selection passes against the float64 scores
    assert R.check_within_bar(R.select(y32, hit, C, 10, 5)[0], C, y, bar, hit, 10, 5) <= 1.0


# ------------------------------------------------------------------------------------------------ the sampler's host side
def test_constructor_validation():
    import tensorrec_amd as T
    for bad in (0, -3, 2.5, None, True):
        with pytest.raises(ValueError, match="n_candidates"):
            T.HardNegativeSampler(bad)
    for bad in (0, -1, 1.5, "3", False):
        with pytest.raises(ValueError, match="n_hard"):
            T.HardNegativeSampler(8, n_hard=bad)
    with pytest.raises(ValueError, match="base"):
        T.HardNegativeSampler(8, base=T.HardNegativeSampler(16))
    s = T.HardNegativeSampler(8, n_hard=3, exclude_positives=False, seed=11)
    assert (s.n_candidates, s.n_hard, s.exclude_positives, s.keep_last) == (8, 3, False, False)
    assert type(s.base) is T.DeviceSampler and s.base.seed == 11
    assert T.HardNegativeSampler.scored is True and not hasattr(s, "log_q")
    assert "HardNegativeSampler" in T.__all__


def test_plain_sample_raises_type_error():
    import tensorrec_amd as T
    with pytest.raises(TypeError, match="sample_scored"):
        T.HardNegativeSampler(8).sample(10, 2, 4, False, 1, "cpu")


def test_pickling_drops_device_state():
    import tensorrec_amd as T
    s = T.HardNegativeSampler(8, base=T.ReplaySampler([np.zeros((2, 8), np.int32)]), n_hard=2, keep_last=True)
    s.last_table, s.last_candidates = object(), object()          # (stand-ins for device tensors: they must not be pickled)
    t = pickle.loads(pickle.dumps(s))
    assert t.last_table is None and t.last_candidates is None and s.last_table is not None
    assert (t.n_candidates, t.n_hard, t.keep_last, t.exclude_positives, t.seed) == (8, 2, True, True, 0)
    assert type(t.base) is T.ReplaySampler and np.array_equal(t.base.tables[0], s.base.tables[0])


def test_coverage_query():
    from tensorrec_amd import ops
    ok = ops.hard_negatives_supported
    assert all(ok(256, 100, d) for d in range(4, 257, 4))
    assert ok(1, 1, 4) and ok(4096, 4096, 256) and ok(4096, 1, 128)
    assert not ok(4097, 10, 64) and not ok(10, 11, 64) and not ok(10, 0, 64) and not ok(0, 0, 64)
    assert not ok(64, 8, 0) and not ok(64, 8, 6) and not ok(64, 8, 260)


def test_step_plan_keywords():
    from tensorrec_amd import step_plan
    sw = step_plan.Switches(True, True, True, True, True)
    graph = (True, False, False, False, False, True, True, 0, 1000, 10, 20, 5, False)
    assert step_plan.graph_eligible(*graph) is True
    assert step_plan.graph_eligible(*graph, scored_sampler=False) is True
    assert step_plan.graph_eligible(*graph, scored_sampler=True) is False
    coop = (False, False, False, False, False, True, True, True, True, True, 10, 10, 20, 8, 5, 4)
    covered = step_plan.coop_covered(*coop, switches=sw)
    assert covered is True
    assert step_plan.coop_covered(*coop, switches=sw, scored_sampler=False) is covered
    assert step_plan.coop_covered(*coop, switches=sw, scored_sampler=True) is False
