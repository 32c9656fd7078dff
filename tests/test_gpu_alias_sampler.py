"""The alias sampler kernel (csrc/sampler_alias.hip) bit for bit against the integer restatement of tests/alias_sampler_reference.py, and
its draws against the exact distribution of the table: chi-square tests accepted within 5 standard deviations (the rule of
tests/test_gpu_sampler_quality.py, restated in the reference module), fixed seeds, so the tests are deterministic.
tests/test_alias_sampler_host.py shows on the CPU that the restatement itself passes the same distribution checks."""
import functools

import numpy as np
import pytest
import torch

import alias_sampler_reference as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from tensorrec_amd import ops as _ops, _native
    _native.require_gpu()
    _native.load()
    return _ops


@functools.lru_cache(maxsize=None)
def table(kind, n, power=1.0):
    thr, alias = A.build_table(A.weights(kind, n) ** power)
    return thr, alias, A.table_q(thr, alias)


def dev_table(thr, alias):
    return torch.from_numpy(thr.view(np.int32)).cuda(), torch.from_numpy(alias).cuda()


@pytest.mark.parametrize("n_items", A.N_ITEMS)
def test_bit_for_bit_against_the_restatement(ops, n_items):
    thr, alias, _ = table("zipf", n_items, 0.75)
    t, a = dev_table(thr, alias)
    for S in (1, 2, 7, 8, 100, 257):
        for n_users in (0, 1, 300):
            for user_base in (0, 2 ** 32 + 5):
                for seed in (0, 0xDEADBEEF12345678):
                    for step in (1, 2):
                        got = ops.sample_items_alias(n_users, n_items, S, t, a, seed, step, "cuda", user_base)
                        assert got.dtype == torch.int32 and tuple(got.shape) == (n_users, S)
                        want = A.draw(n_users, n_items, S, thr, alias, seed, step, user_base)
                        assert np.array_equal(got.cpu().numpy(), want), (n_items, S, n_users, user_base, seed, step)


def test_steps_seeds_and_samplers_differ(ops):
    """another step, another seed and K7 under the same seed give other tables"""
    n, U, S = 1000, 50, 20
    thr, alias, _ = table("uniform", n)
    t, a = dev_table(thr, alias)
    base = ops.sample_items_alias(U, n, S, t, a, 7, 1)
    assert not torch.equal(base, ops.sample_items_alias(U, n, S, t, a, 7, 2))
    assert not torch.equal(base, ops.sample_items_alias(U, n, S, t, a, 8, 1))
    assert not torch.equal(base, ops.sample_items(U, n, S, True, 7, 1))
    assert torch.equal(base[10:], ops.sample_items_alias(U - 10, n, S, t, a, 7, 1, "cuda", 10))        # a shard draws the same rows


def test_popularity_sampler_class(ops):
    from tensorrec_amd import PopularitySampler
    n = 1000
    s = PopularitySampler(A.weights("zipf", n), power=0.75, seed=11)
    thr, alias, q = table("zipf", n, 0.75)
    assert np.array_equal(s.thr, thr) and np.array_equal(s.alias, alias)
    got = s.sample(n, 40, 9, False, 3, "cuda", user_base=5)                            # `replace` is ignored
    assert np.array_equal(got.cpu().numpy(), A.draw(40, n, 9, thr, alias, 11, 3, 5))
    lq = s.log_q("cuda")
    assert lq.dtype == torch.float32 and tuple(lq.shape) == (n,) and lq is s.log_q("cuda")     # uploaded once
    assert np.abs(lq.cpu().numpy().astype(np.float64) - np.log(q)).max() <= 2.0 ** -24 * np.abs(np.log(q)).max()
    z = PopularitySampler(A.weights("two-level", n), power=1.0)
    lz = z.log_q("cuda").cpu().numpy()
    assert np.isneginf(lz[4]) and np.isfinite(lz[0])
    with pytest.raises(ValueError):
        s.sample(n + 1, 4, 3, False, 1, "cuda")


N, U, S = 1000, 2000, 100


def test_marginals_follow_the_table(ops):
    """Zipf ** 0.75, uniform (power 0) and a table with items of weight 0, 2,000 users x 100 samples: pooled cells of expected count
    >= 50 against the exact table q; an item of q = 0 never appears"""
    for kind, power in (("zipf", 0.75), ("zipf", 0.0), ("two-level", 1.0)):
        thr, alias, q = table(kind, N, power)
        t, a = dev_table(thr, alias)
        got = ops.sample_items_alias(U, N, S, t, a, 4242, 5).cpu().numpy()
        assert got.min() >= 0 and got.max() < N
        assert (q[got] > 0).all(), "an item of probability 0 was drawn"
        z = A.marginal_z(got, q)
        print("%s ** %g: marginal z = %.2f" % (kind, power, z))
        assert abs(z) <= 5.0, (kind, power, z)
    assert np.abs(table("zipf", N, 0.0)[2] - 1.0 / N).max() <= N * 2.0 ** -32


def test_positions_steps_and_neighbouring_users_are_independent(ops):
    thr, alias, q = table("zipf", N, 0.75)
    t, a = dev_table(thr, alias)
    x = ops.sample_items_alias(U, N, S, t, a, 4242, 5).cpu().numpy()
    y = ops.sample_items_alias(U, N, S, t, a, 4242, 6).cpu().numpy()
    checks = {"first half vs second half of the positions": A.contingency_z(x[:, : S // 2], x[:, S // 2:], q),
              "even vs odd positions (the two halves of a Philox block)": A.contingency_z(x[:, 0::2], x[:, 1::2], q),
              "same position, next step": A.contingency_z(x, y, q),
              "same position, next user": A.contingency_z(x[:-1], x[1:], q)}
    print(", ".join("%s z=%.2f" % kv for kv in checks.items()))
    for k, z in checks.items():
        assert abs(z) <= 5.0, (k, z)
