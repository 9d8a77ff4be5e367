"""`WeightedShardedNegativeSampler(return_logq=True)` on the host: the log-proposal table and the layout of
`negative_logq` against a Python-loop restatement of their formulas, and the statistical reason for the option - the
sampled-softmax estimate of `sum_e exp(s_e)` is only consistent when every candidate's logit is lowered by the log of
its expected count among the candidates."""

import math

import numpy as np
import pytest

from besskge.negative_sampler import WeightedShardedNegativeSampler
from besskge.sharding import Sharding

N_ENTITY, N_SHARD, K = 1000, 3, 7


def sharding_334():
    """3 shards of 334 / 333 / 333 rows in some order (two of them end in a padding row)."""
    sh = Sharding.create(N_ENTITY, N_SHARD, seed=7)
    assert sorted(sh.shard_counts.tolist(), reverse=True) == [334, 333, 333] and sh.max_entity_per_shard == 334
    return sh


def weights_with_zeros(seed=5):
    rng = np.random.default_rng(seed)
    w = rng.integers(1, 5000, size=N_ENTITY).astype(np.int64)
    w[rng.choice(N_ENTITY, size=60, replace=False)] = 0
    return w


def make(sh, w, scheme, flat, local, return_logq, seed=3):
    return WeightedShardedNegativeSampler(w, K, sh, seed, scheme, local, flat_negative_format=flat,
                                          return_logq=return_logq)


def test_log_q_table_is_the_formula():
    sh, w = sharding_334(), weights_with_zeros()
    for local in (False, True):
        ns = make(sh, w, "t", True, local, True)
        assert ns.log_q.dtype == np.float32 and ns.log_q.shape == (N_SHARD, sh.max_entity_per_shard)
        for s in range(N_SHARD):
            total = sum(int(w[sh.shard_and_idx_to_entity[s, i]]) for i in range(sh.shard_counts[s]))
            assert total == int(ns.shard_totals[s])
            for i in range(sh.max_entity_per_shard):
                wi = int(w[sh.shard_and_idx_to_entity[s, i]]) if i < sh.shard_counts[s] else 0
                if wi == 0:
                    assert ns.log_q[s, i] == 0.0  # weight 0 or padding: never drawn, nothing non-finite
                else:
                    want = math.log(wi / total) - (0.0 if local else math.log(N_SHARD))
                    assert ns.log_q[s, i] == np.float32(want)
    assert not hasattr(make(sh, w, "t", True, False, False), "log_q")


@pytest.mark.parametrize("local", [False, True])
@pytest.mark.parametrize("flat", [True, False])
@pytest.mark.parametrize("scheme", ["h", "t", "ht"])
def test_negative_logq_layout_and_unchanged_draws(scheme, flat, local):
    sh, w = sharding_334(), weights_with_zeros()
    with_q, without = make(sh, w, scheme, flat, local, True), make(sh, w, scheme, flat, local, False)
    n_step, ppp = 2, 4
    sample_idx = np.zeros((n_step, N_SHARD, ppp), dtype=np.int64)
    B = (2 if scheme == "ht" else 1) if flat else ppp
    for _ in range(2):  # (two calls: the stream position moves the same way)
        a, b = with_q(sample_idx), without(sample_idx)
        assert set(b) == {"negative_entities"} and set(a) == {"negative_entities", "negative_logq"}
        np.testing.assert_array_equal(a["negative_entities"], b["negative_entities"])
        assert with_q.rng.bit_generator.state == without.rng.bit_generator.state
        ne, lq = a["negative_entities"], a["negative_logq"]
        assert ne.shape == (n_step, N_SHARD, N_SHARD, B, K)
        assert lq.dtype == np.float32 and lq.shape == (n_step, N_SHARD, B, N_SHARD, K) and lq.flags["C_CONTIGUOUS"]
        assert np.isfinite(lq).all()
        for step in range(n_step):
            for d in range(N_SHARD):
                for bb in range(B):
                    for j in range(N_SHARD):
                        for k in range(K):
                            if local:
                                want = with_q.log_q[d, ne[step, d, j, bb, k]]
                            else:
                                want = with_q.log_q[j, ne[step, j, d, bb, k]]
                            assert lq[step, d, bb, j, k] == want
                            assert want < 0.0  # a drawn row has a positive weight below its shard's total


def test_batch_sampler_passes_negative_logq_through():
    from besskge.batch_sampler import RigidShardedBatchSampler
    from besskge.dataset import KGDataset
    from besskge.sharding import PartitionedTripleSet

    rng = np.random.default_rng(0)
    triples = np.stack([rng.integers(N_ENTITY, size=600), rng.integers(5, size=600), rng.integers(N_ENTITY, size=600)],
                       axis=1)
    sh = sharding_334()
    ds = KGDataset(n_entity=N_ENTITY, n_relation_type=5, triples={"train": triples},
                   original_triple_ids={"train": np.arange(triples.shape[0])})
    part = PartitionedTripleSet.create_from_dataset(ds, "train", sh, partition_mode="ht_shardpair")
    ns = make(sh, weights_with_zeros(), "t", True, False, True)
    bs = RigidShardedBatchSampler(partitioned_triple_set=part, negative_sampler=ns, shard_bs=12, batches_per_step=2, seed=1)
    batch = bs[list(bs.get_dataloader_sampler(shuffle=False))[0]]
    lq, neg = batch["negative_logq"], batch["negative"]
    assert tuple(lq.shape) == (2, N_SHARD, 1, N_SHARD, K) and np.asarray(lq).dtype == np.float32
    assert tuple(neg.shape) == (2, N_SHARD, N_SHARD, 1, K)
    want = ns.log_q[np.arange(N_SHARD).reshape(1, -1, 1, 1, 1), np.asarray(neg)].transpose(0, 2, 3, 1, 4)
    assert np.array_equal(np.asarray(lq), want)


def test_corrected_estimator_is_consistent_and_the_uncorrected_is_not():
    """600 sampled-softmax estimates of Z = sum over w > 0 of exp(s_e) (200 calls x 3 scoring shards, flat "t", K = 256,
    N = 3 * 256 candidates each): with the correction the mean of sum_j exp(s_j - log N - logq_j) is within 5 standard
    errors of Z; the uncorrected estimate sum_j exp(s_j + log(n_entity - 1) - log N) of a sampler whose scores grow with
    the weights is at least 2x too large."""
    n_entity, n_shard, k = 1000, 3, 256
    sh = Sharding.create(n_entity, n_shard, seed=7)
    rng = np.random.default_rng(2024)
    w = np.floor(np.minimum(rng.zipf(1.6, size=n_entity).astype(np.float64), 1e6) ** 0.75 * 1024).astype(np.int64)
    w[rng.choice(n_entity, size=20, replace=False)] = 0
    score = rng.normal(0.0, 0.5, size=n_entity) + 0.5 * np.log(np.maximum(w, 1) / 1024.0)
    truth = float(np.exp(score[w > 0]).sum())
    ns = WeightedShardedNegativeSampler(w, k, sh, 99, "t", False, flat_negative_format=True, return_logq=True)
    sample_idx = np.zeros((1, n_shard, 4), dtype=np.int64)
    corrected, plain = [], []
    n_cand = n_shard * k
    for _ in range(200):
        out = ns(sample_idx)
        ne, lq = out["negative_entities"][0], out["negative_logq"][0].astype(np.float64)  # [s, d, 1, K], [d, 1, s, K]
        for d in range(n_shard):
            ent = sh.shard_and_idx_to_entity[np.arange(n_shard)[:, None], ne[:, d, 0, :]]  # [s, K] global ids
            s = score[ent]
            corrected.append(np.exp(s - math.log(n_cand) - lq[d, 0]).sum())
            plain.append(np.exp(s + math.log(n_entity - 1) - math.log(n_cand)).sum())
    corrected, plain = np.array(corrected), np.array(plain)
    assert corrected.size == 600
    sem = corrected.std(ddof=1) / math.sqrt(corrected.size)
    z = (corrected.mean() - truth) / sem
    print(f"truth {truth:.4f} corrected {corrected.mean():.4f} (z = {z:+.2f}) uncorrected {plain.mean():.4f} "
          f"({plain.mean() / truth:.2f}x)")
    assert abs(z) <= 5.0
    assert plain.mean() >= 2.0 * truth


def test_entry_points_refuse_before_any_launch():
    """No device needed: `bess_loss_fwd_bwd_logq` takes the sampled-softmax loss only, 1, 2 or n_triple rows and at most
    n_neg columns; `bess_gather_negative_logq` the blocks its layout reads.  Empty problems are no launch."""
    import ctypes

    from besskge import _native as nat

    assert {"bess_loss_fwd_bwd_logq", "bess_gather_negative_logq"} <= set(nat.SIGNATURES)
    lib = nat.load()
    buf = (ctypes.c_float * 256)()
    p = ctypes.addressof(buf)
    err = ctypes.create_string_buffer(256)

    def loss(kind=nat.LOSS_SSCE, n_triple=8, n_neg=12, logq=p, rows=1, cols=12, ppp=0):
        l = nat.LossDesc()
        l.kind, l.loss_scale = kind, 1.0
        rc = lib.bess_loss_fwd_bwd_logq(ctypes.byref(l), p, p, n_triple, n_neg, n_neg, p, 1, p, p, None, None, 0, None, None,
                                        logq, rows, cols, ppp, 0.0, None)
        lib.bess_last_error(err, 256)
        return rc, err.value.decode()

    for kind in (nat.LOSS_LOGSIGMOID, nat.LOSS_MARGIN, 9):
        rc, msg = loss(kind=kind)
        assert rc == -1 and "sampled-softmax" in msg
    rc, msg = loss(rows=3)
    assert rc == -1 and "logq_rows" in msg
    rc, msg = loss(cols=13)
    assert rc == -1 and "logq_cols" in msg
    assert loss(cols=0)[0] == -1 and loss(logq=None)[0] == -1
    rc, msg = loss(rows=2, ppp=3)
    assert rc == -1 and "even block size" in msg
    assert loss(rows=2, ppp=0)[0] == -1 and loss(rows=2, ppp=6)[0] == -1  # (6 does not divide 8 triples)

    def gather(n_step=1, n_shard=3, src_begin=0, src_count=3, dst_begin=0, dst_count=3, B=2, K=5, local=0, neg=p,
               table=p, ld=4, out=p):
        return lib.bess_gather_negative_logq(neg, table, ld, n_step, n_shard, src_begin, src_count, dst_begin, dst_count,
                                             B, K, local, out, None)

    for empty in (dict(n_step=0), dict(dst_count=0), dict(B=0), dict(K=0)):
        assert gather(**empty, neg=None, table=None, out=None) == 0
    for null in ("neg", "table", "out"):
        assert gather(**{null: None}) == -1
    assert gather(src_begin=1, src_count=2) == -1  # every source shard is read without local sampling
    assert gather(src_begin=1, src_count=3) == -1 and gather(dst_begin=2, dst_count=2) == -1 and gather(dst_begin=-1) == -1
    assert gather(local=1, src_begin=1, src_count=1, dst_begin=0, dst_count=1) == -1  # not the scoring shard's blocks
    assert gather(ld=0) == -1 and gather(K=-1) == -1
