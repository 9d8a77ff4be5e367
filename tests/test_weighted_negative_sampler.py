"""`WeightedShardedNegativeSampler` and `degree_weights` (besskge/negative_sampler.py): negatives in proportion to
integer entity weights.  The reference has no such sampler; the oracle is an independent restatement of the class's
formula - a Python loop over the raw 64-bit draws with `bisect.bisect_right` on running sums built with Python ints."""

import bisect

import numpy as np
import pytest

from besskge.negative_sampler import RandomShardedNegativeSampler, WeightedShardedNegativeSampler, degree_weights
from besskge.sharding import Sharding

N_ENT, N_SHARD, PER = 1000, 3, 8


def sharding3():
    sh = Sharding.create(N_ENT, N_SHARD, seed=17)
    assert sorted(sh.shard_counts.tolist()) == [333, 333, 334] and sh.max_entity_per_shard == 334  # pads exist
    return sh


def running_sums(sharding, weights):
    """Per shard: the inclusive running sums of its real rows, as Python ints."""
    out = []
    for s in range(sharding.n_shard):
        acc, row = 0, []
        for i in range(int(sharding.shard_counts[s])):
            acc += int(weights[sharding.shard_and_idx_to_entity[s, i]])
            row.append(acc)
        out.append(row)
    return out


def restated(sharding, weights, seed, shapes):
    """The draws of consecutive calls with output shapes `shapes`, from one generator."""
    sums = running_sums(sharding, weights)
    rng = np.random.default_rng(seed)
    calls = []
    for shape in shapes:
        raw = rng.integers(1 << 63, size=shape)
        out = np.empty(shape, dtype=np.int64)
        for at in np.ndindex(*shape):
            src = at[1]
            out[at] = bisect.bisect_right(sums[src], int(raw[at]) % sums[src][-1])
        calls.append(out)
    return calls


def sample_idx(n_step, n_shard, per, pair):
    """Only its shape is read by these samplers."""
    return np.zeros((n_step, n_shard, n_shard, per) if pair else (n_step, n_shard, per), dtype=np.int64)


def skewed_weights(seed=3):
    rng = np.random.default_rng(seed)
    w = np.floor(rng.zipf(1.6, size=N_ENT).astype(np.float64) ** 0.75 * 1024).astype(np.int64)
    w[rng.choice(N_ENT, size=100, replace=False)] = 0
    return w


@pytest.mark.parametrize("scheme", ["h", "t", "ht"])
@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("local", [False, True])
def test_call_equals_the_bisect_restatement(scheme, flat, local):
    sh = sharding3()
    w = skewed_weights()
    K = 5
    ns = WeightedShardedNegativeSampler(w, K, sh, seed=11, corruption_scheme=scheme, local_sampling=local,
                                        flat_negative_format=flat)
    uni = RandomShardedNegativeSampler(K, sh, seed=11, corruption_scheme=scheme, local_sampling=local,
                                       flat_negative_format=flat)
    idxs = [sample_idx(2, N_SHARD, PER, pair=True), sample_idx(3, N_SHARD, PER, pair=False)]
    got = [ns(i) for i in idxs]
    ref = [uni(i) for i in idxs]
    B = [(2 if scheme == "ht" else 1) if flat else b for b in (N_SHARD * PER, PER)]
    shapes = [(2, N_SHARD, N_SHARD, B[0], K), (3, N_SHARD, N_SHARD, B[1], K)]
    want = restated(sh, w, 11, shapes)  # the second call continues the stream of the first
    for g, r, x, shape in zip(got, ref, want, shapes):
        assert list(g) == list(r) == ["negative_entities"]
        rows = g["negative_entities"]
        assert rows.dtype == np.int32  # (what the batch sampler casts the uniform class's rows to)
        assert rows.shape == r["negative_entities"].shape == shape
        assert np.array_equal(rows, x)
        assert rows.min() >= 0 and np.all(rows < sh.shard_counts.reshape(1, -1, 1, 1, 1))
        assert np.all(w[sh.shard_and_idx_to_entity[np.arange(N_SHARD).reshape(1, -1, 1, 1, 1), rows]] > 0)
    # same seed, same output
    again = WeightedShardedNegativeSampler(w, K, sh, seed=11, corruption_scheme=scheme, local_sampling=local,
                                           flat_negative_format=flat)
    assert np.array_equal(again(idxs[0])["negative_entities"], got[0]["negative_entities"])
    assert not np.array_equal(again(idxs[0])["negative_entities"], got[0]["negative_entities"])  # the stream moved on


def test_constructor_tables():
    sh = sharding3()
    w = skewed_weights()
    ns = WeightedShardedNegativeSampler(w.astype(np.int32), 4, sh, 0, "t", False)
    assert ns.entity_weights.dtype == np.int64 and np.array_equal(ns.entity_weights, w)
    assert ns.cum_weights.dtype == np.int64 and ns.cum_weights.shape == (N_SHARD, sh.max_entity_per_shard)
    assert ns.shard_totals.dtype == np.int64 and ns.shard_totals.shape == (N_SHARD,)
    sums = running_sums(sh, w)
    for s in range(N_SHARD):
        c = int(sh.shard_counts[s])
        assert ns.cum_weights[s, :c].tolist() == sums[s]
        assert np.all(ns.cum_weights[s, c:] == sums[s][-1])  # flat over the pads
        assert int(ns.shard_totals[s]) == sums[s][-1]
    assert int(ns.shard_totals.sum()) == int(w.sum())


def test_zero_runs_at_both_ends_of_a_shard_are_never_drawn():
    sh = sharding3()
    w = np.full(N_ENT, 3, dtype=np.int64)
    dead = []
    for s in range(N_SHARD):
        c = int(sh.shard_counts[s])
        dead.append(np.r_[0:5, 100:103, c - 7:c])  # rows 0-4, 100-102 and the last 7
        w[sh.shard_and_idx_to_entity[s, dead[-1]]] = 0
    ns = WeightedShardedNegativeSampler(w, 64, sh, 5, "t", False)
    rows = ns(sample_idx(4, N_SHARD, 32, pair=False))["negative_entities"]
    for s in range(N_SHARD):
        c = int(sh.shard_counts[s])
        hit = np.bincount(rows[:, s].reshape(-1), minlength=c)
        assert hit.shape[0] == c and not hit[dead[s]].any()
        assert hit[5] > 0 and hit[c - 8] > 0 and (hit > 0).sum() > 0.9 * (c - 15)  # their neighbours are


def test_one_heavy_entity_takes_almost_every_draw():
    sh = sharding3()
    w = np.ones(N_ENT, dtype=np.int64)
    heavy = int(sh.shard_and_idx_to_entity[1, 77])
    w[heavy] = 2 ** 40
    ns = WeightedShardedNegativeSampler(w, 50, sh, 9, "h", False)
    rows = ns(sample_idx(2, N_SHARD, 40, pair=False))["negative_entities"]
    # the other 332 rows of shard 1 together weigh 332 / 2^40: 12000 draws hit one with probability 4e-6
    assert np.all(rows[:, 1] == 77)
    assert len(np.unique(rows[:, 0])) > 300 and len(np.unique(rows[:, 2])) > 300  # the other shards stay uniform


@pytest.mark.parametrize("weight", [1, 2 ** 31])
def test_constant_weights_every_draw_lands_on_a_running_sum(weight):
    """Weights all 1: total == count and u is itself a running sum minus one - `side="right"` decides every draw, and
    row == u.  Weights all 2^31: totals pass 2^32 (and 2^39), row == u >> 31."""
    sh = sharding3()
    w = np.full(N_ENT, weight, dtype=np.int64)
    ns = WeightedShardedNegativeSampler(w, 9, sh, 21, "ht", False)
    assert ns.shard_totals.tolist() == [weight * int(c) for c in sh.shard_counts]
    assert weight == 1 or int(ns.shard_totals.min()) > 2 ** 39
    shape = (2, N_SHARD, N_SHARD, 16, 9)
    rows = ns(sample_idx(2, N_SHARD, 16, pair=False))["negative_entities"]
    raw = np.random.default_rng(21).integers(1 << 63, size=shape)
    want = (raw % (weight * sh.shard_counts.reshape(1, -1, 1, 1, 1))) // weight
    assert np.array_equal(rows, want)
    assert np.array_equal(rows, restated(sh, w, 21, [shape])[0])
    # uniform, yet not the uniform class's rows for the same seed: that class takes 32-bit draws
    uni = RandomShardedNegativeSampler(9, sh, 21, "ht", False)(sample_idx(2, N_SHARD, 16, pair=False))
    assert not np.array_equal(uni["negative_entities"], rows)


def test_frequencies_follow_the_weights():
    """20 seeds of a [4, 3, 3, 64, 37] draw (N = 4 * 3 * 64 * 37 = 28,416 draws per source shard and seed): every
    entity with expected count N p >= 50 stays within 5 sigma of it, sigma^2 = N p (1 - p).  Rarer entities are
    left to the zero-weight check: the normal bound does not describe them."""
    sh = sharding3()
    w = skewed_weights(seed=8)
    assert (w == 0).sum() == 100
    checked = 0
    for seed in range(20):
        ns = WeightedShardedNegativeSampler(w, 37, sh, seed, "t", False)
        rows = ns(sample_idx(4, N_SHARD, 64, pair=False))["negative_entities"]
        assert rows.shape == (4, 3, 3, 64, 37)
        for s in range(N_SHARD):
            c = int(sh.shard_counts[s])
            local_w = w[sh.shard_and_idx_to_entity[s, :c]].astype(np.float64)
            p = local_w / local_w.sum()
            n = rows[:, s].size
            count = np.bincount(rows[:, s].reshape(-1), minlength=c)
            assert not count[local_w == 0].any()
            big = n * p >= 50
            assert big.sum() >= 3
            dev = np.abs(count[big] - n * p[big]) / np.sqrt(n * p[big] * (1 - p[big]))
            assert dev.max() <= 5.0, (seed, s, float(dev.max()))
            checked += int(big.sum())
    assert checked > 20 * N_SHARD * 3


def test_refusals():
    sh = sharding3()
    ok = np.ones(N_ENT, dtype=np.int64)

    def build(w):
        return WeightedShardedNegativeSampler(w, 4, sh, 0, "t", False)

    build(ok)
    with pytest.raises(ValueError, match="shape"):
        build(ok[:-1])
    with pytest.raises(ValueError, match="shape"):
        build(np.ones((N_ENT, 1), dtype=np.int64))
    neg = ok.copy()
    neg[5] = -1
    with pytest.raises(ValueError, match=">= 0"):
        build(neg)
    with pytest.raises(ValueError, match="integers"):
        build(ok.astype(np.float64))
    with pytest.raises(ValueError, match="integers"):
        build(ok.astype(bool))
    empty = ok.copy()
    empty[sh.shard_and_idx_to_entity[2, : sh.shard_counts[2]]] = 0
    with pytest.raises(ValueError, match="shard 2 has total weight 0"):
        build(empty)
    big = ok.copy()
    big[sh.shard_and_idx_to_entity[0, :4]] = 2 ** 60  # 4 * 2^60 = 2^62
    with pytest.raises(ValueError, match="2\\*\\*62"):
        build(big)
    big[sh.shard_and_idx_to_entity[0, 0]] = 2 ** 60 - int(sh.shard_counts[0])  # total 2^62 - 4: accepted
    assert int(build(big).shard_totals[0]) == 2 ** 62 - 4
    with pytest.raises(ValueError, match="2\\*\\*62"):
        build(np.full(N_ENT, 2 ** 63, dtype=np.uint64))


def test_degree_weights_on_a_hand_counted_graph():
    #            h  r  t
    a = np.array([[0, 0, 1], [0, 1, 2], [0, 0, 3], [1, 0, 0]])
    b = np.array([[2, 1, 0], [2, 0, 2]])
    # entity      0  1  2  3  4
    as_head = [3, 1, 2, 0, 0]
    as_tail = [2, 1, 2, 1, 0]
    for side, deg in (("h", as_head), ("t", as_tail), ("both", [h + t for h, t in zip(as_head, as_tail)])):
        got = degree_weights([a, b], 5, alpha=1.0, scale=10, min_weight=0, side=side)
        assert got.dtype == np.int64 and got.tolist() == [10 * d for d in deg]
        got = degree_weights([a, b], 5, alpha=1.0, scale=10, min_weight=1, side=side)
        assert got.tolist() == [max(1, 10 * d) for d in deg]
    # defaults: both sides, degree ** 0.75 * 1024 rounded down, never below 1
    got = degree_weights([a, b], 5)
    assert got.tolist() == [int(np.floor(d ** 0.75 * 1024)) if d else 1 for d in (5, 2, 4, 1, 0)]
    assert got.tolist() == [3423, 1722, 2896, 1024, 1]
    assert degree_weights([a, b], 5, min_weight=0)[4] == 0
    with pytest.raises(ValueError):
        degree_weights([a], 5, side="ht")
    # feeds the sampler: entity 4 (never seen, weight 0) is not drawn
    sh = Sharding.create(5, 1, seed=0)
    ns = WeightedShardedNegativeSampler(degree_weights([a, b], 5, min_weight=0), 200, sh, 1, "t", False)
    rows = ns(sample_idx(1, 1, 4, pair=False))["negative_entities"]
    assert set(sh.shard_and_idx_to_entity[0, rows.reshape(-1)].tolist()) == {0, 1, 2, 3}
