"""`WeightedShardedNegativeSampler` on the device (`bess_sample_negatives_weighted`, csrc/sampler.hip): the 64-bit draws
of the host class's numpy stream and its `searchsorted` over the running weight sums, reproduced in HBM.  Integer
arithmetic only, so every comparison is `torch.equal` against the host class (whose own formula is checked against a
`bisect` restatement in tests/test_weighted_negative_sampler.py).  Sizes sit where the stream arithmetic can go wrong:
7 negatives (no multiple of the 8 draws of a thread), uneven shards, blocks that end inside a thread's stretch."""

import ctypes

import numpy as np
import pytest
import torch

from besskge.batch_sampler import RandomShardedBatchSampler, RigidShardedBatchSampler
from besskge.dataset import KGDataset
from besskge.negative_filter import KnownTripleFilter
from besskge.negative_sampler import WeightedShardedNegativeSampler
from besskge.sharding import PartitionedTripleSet, Sharding


def skewed(n_entity, seed):
    """floor(zipf ** 0.75 * 1024) with a tenth of the entities at weight 0."""
    rng = np.random.default_rng(seed)
    w = np.floor(rng.zipf(1.6, size=n_entity).astype(np.float64) ** 0.75 * 1024).astype(np.int64)
    w[rng.choice(n_entity, size=n_entity // 10, replace=False)] = 0
    return w


def make(n_shard, shard_bs, scheme, flat, local, rigid, weights="skewed", n_entity=1000, n_rel=7, n_triple=4000, K=7,
         bps=2, seed=31, triples=None):
    """Two identical batch samplers (the host reference and the one handed to the device twin)."""
    rng = np.random.default_rng(seed)
    if triples is None:
        triples = np.stack([rng.integers(n_entity, size=n_triple), rng.integers(n_rel, size=n_triple),
                            rng.integers(n_entity, size=n_triple)], axis=1)
    ds = KGDataset(n_entity=n_entity, n_relation_type=n_rel, triples={"train": triples},
                   original_triple_ids={"train": np.arange(triples.shape[0])})
    sharding = Sharding.create(n_entity, n_shard, seed=seed)
    pts = PartitionedTripleSet.create_from_dataset(ds, "train", sharding, partition_mode="ht_shardpair")
    w = skewed(n_entity, seed + 5) if isinstance(weights, str) else np.asarray(weights)

    def build():
        ns = WeightedShardedNegativeSampler(w, K, sharding, seed + 1, scheme, local, flat_negative_format=flat)
        cls = RigidShardedBatchSampler if rigid else RandomShardedBatchSampler
        return cls(partitioned_triple_set=pts, negative_sampler=ns, shard_bs=shard_bs, batches_per_step=bps, seed=seed + 2)

    return build(), build()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda", 0)


def same(got, want, key):
    assert got.is_cuda
    g = got.cpu()
    assert g.dtype == want.dtype and tuple(g.shape) == tuple(want.shape), (key, g.dtype, want.dtype, g.shape, want.shape)
    assert torch.equal(g, want), key


def same_stream(a, b):
    sa, sb = a.rng.bit_generator.state, b.rng.bit_generator.state
    assert sa["state"] == sb["state"] and sa["has_uint32"] == sb["has_uint32"] == 0


def follow(dev, host, twin, steps=3, **kw):
    """`steps` consecutive device draws against the host's, then the stream handed back to the host class."""
    from besskge.device_sampler import DeviceBatchSampler

    dbs = DeviceBatchSampler(twin, dev, **kw)
    order = list(host.get_dataloader_sampler(shuffle=False))
    for step in range(steps):
        idx = order[step % len(order)]
        want, got = host[idx], dbs.sample(idx)
        assert list(got.keys()) == list(want.keys()) and "negative" in want
        for k in want:
            same(got[k], want[k], f"{step}/{k}")
    dbs.sync_host()
    same_stream(host.negative_sampler, twin.negative_sampler)
    a, b = host[order[0]], twin[order[0]]
    for k in a:
        assert torch.equal(a[k], b[k]), k
    return want


# ------------------------------------------------------------------ no GPU
def test_binding_and_refusals_before_any_launch():
    """No device needed: the entry point validates first, and an empty problem is no launch."""
    from besskge import _native as nat

    assert "bess_sample_negatives_weighted" in nat.SIGNATURES
    lib = nat.load()
    gen = nat.Pcg64State()
    buf = (ctypes.c_int64 * 256)()
    p = ctypes.addressof(buf)

    def call(n_step=1, n_shard=2, src_begin=0, src_count=2, B=3, K=5, ld=4, g=ctypes.byref(gen), table=p, cum=p, counts=p,
             out=p):
        return lib.bess_sample_negatives_weighted(g, table, n_step, n_shard, src_begin, src_count, B, K, cum, ld, counts,
                                                  out, None)

    for empty in (dict(n_step=0), dict(src_count=0), dict(B=0), dict(K=0)):
        assert call(**empty, g=None, table=None, cum=None, counts=None, out=None) == 0
    for null in ("g", "table", "cum", "counts", "out"):
        assert call(**{null: None}) == -1
    assert call(src_begin=1, src_count=2) == -1 and call(src_begin=-1) == -1 and call(src_begin=2, src_count=1) == -1
    assert call(ld=0) == -1
    err = ctypes.create_string_buffer(256)
    lib.bess_last_error(err, 256)
    assert "ld_cum" in err.value.decode()
    assert call(K=-1) == -1


# --------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("n_shard", [1, 3])
@pytest.mark.parametrize("scheme", ["h", "t", "ht"])
@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("local", [False, True])
def test_device_twin_equals_the_host_class(dev, n_shard, scheme, flat, local):
    """shard_bs 6 and 48, rigid and random batch samplers: three consecutive draws (the stream continues), the
    position handed back to the host."""
    for shard_bs in (6, 48):
        for rigid in (False, True):
            host, twin = make(n_shard, shard_bs, scheme, flat, local, rigid)
            assert len(set(host.negative_sampler.shard_counts.tolist())) == (2 if n_shard == 3 else 1)  # uneven shards
            want = follow(dev, host, twin)
            K = 7
            B = (2 if scheme == "ht" else 1) if flat else shard_bs
            assert tuple(want["negative"].shape) == (2, n_shard, n_shard, B, K) and want["negative"].dtype == torch.int32


@pytest.mark.gpu
@pytest.mark.parametrize("flat", [False, True])
def test_rank_slices_come_from_the_common_stream(dev, flat):
    from besskge.device_sampler import DeviceBatchSampler

    n = 3
    host, _ = make(n, 48, "ht", flat, False, False)
    ranks = []
    for r in range(n):
        _, twin = make(n, 48, "ht", flat, False, False)
        ranks.append((DeviceBatchSampler(twin, dev, shards=range(r, r + 1)), twin))
        assert tuple(ranks[-1][0]._cum_weights.shape) == (1, twin.negative_sampler.cum_weights.shape[1])  # one row up
    for step in range(3):
        want = host[[0]]
        for r, (dbs, _) in enumerate(ranks):
            got = dbs.sample()
            for k in want:
                same(got[k], want[k][:, r: r + 1], f"{step}/{r}/{k}")
    for dbs, twin in ranks:
        dbs.sync_host()
        same_stream(host.negative_sampler, twin.negative_sampler)


@pytest.mark.gpu
@pytest.mark.parametrize("weights", ["skewed", "ones"])
def test_long_search_and_every_boundary(dev, weights):
    """One shard of 70,001 rows (17 search levels), 2 x 3584 draws a call (two workgroups per step).  All weights 1:
    every u is a running sum minus one, `side="right"` decides each draw."""
    n_entity = 70001
    w = weights if weights == "skewed" else np.ones(n_entity, dtype=np.int64)
    host, twin = make(1, 512, "t", False, False, False, weights=w, n_entity=n_entity, n_triple=3000, seed=41)
    want = follow(dev, host, twin, steps=2)
    rows = want["negative"].numpy().reshape(-1)
    assert rows.max() > 60000 or weights == "skewed"
    if weights == "skewed":
        ns = host.negative_sampler
        assert np.all(ns.entity_weights[ns.sharding.shard_and_idx_to_entity[0, rows]] > 0)
        assert len(np.unique(rows)) > 1000


@pytest.mark.gpu
def test_totals_above_32_bits(dev):
    w = np.full(1000, 2 ** 31, dtype=np.int64)
    host, twin = make(3, 48, "t", False, False, False, weights=w)
    assert int(host.negative_sampler.shard_totals.min()) > 2 ** 39
    want = follow(dev, host, twin)
    assert len(np.unique(want["negative"].numpy())) > 300


@pytest.mark.gpu
def test_wrapper_refuses_wrong_arguments(dev):
    from besskge import _native as nat
    from besskge.device_sampler import Pcg64Stream

    st = Pcg64Stream.from_generator(np.random.default_rng(3))
    table = torch.from_numpy(st.jump_table().view(np.int64)).to(dev)
    cum = torch.arange(1, 21, dtype=torch.int64, device=dev).reshape(2, 10)
    counts = torch.tensor([10, 10], dtype=torch.int32, device=dev)

    def call(table=table, n_shard=2, src_begin=0, src_count=2, cum=cum, counts=counts):
        return nat.sample_negatives_weighted(st.native(), table, 1, n_shard, src_begin, src_count, 3, 5, cum, counts)

    out = call()
    assert out.dtype == torch.int32 and tuple(out.shape) == (1, 2, 2, 3, 5)
    rows = out.cpu().numpy()
    raw = np.random.default_rng(3).integers(1 << 63, size=(1, 2, 2, 3, 5))
    total = np.array([10, 20]).reshape(1, 2, 1, 1, 1)
    base = np.array([0, 10]).reshape(1, 2, 1, 1, 1)
    assert np.array_equal(rows, np.maximum(raw % total - base, 0))  # (row 1 starts at 11: u < 11 is its row 0)
    one = call(src_begin=1, src_count=1, cum=cum[1:])  # a rank's slice: its own row of running sums only
    assert torch.equal(one, out[:, 1:])
    with pytest.raises(ValueError, match="cum_weights"):
        call(cum=cum.to(torch.int32))
    with pytest.raises(ValueError, match="cum_weights"):
        call(cum=cum[:1])
    with pytest.raises(ValueError, match="cum_weights"):
        call(cum=cum.reshape(-1))
    with pytest.raises(ValueError, match="cum_weights"):
        call(cum=cum[:, :5])  # not contiguous
    with pytest.raises(ValueError, match="shard_counts"):
        call(counts=counts.to(torch.int64))
    with pytest.raises(ValueError, match="shard_counts"):
        call(n_shard=3)
    with pytest.raises(ValueError, match="jump_table"):
        call(table=table[:32])
    with pytest.raises(ValueError, match="source shards"):
        call(src_begin=1)
    with pytest.raises(RuntimeError):
        call(cum=cum.cpu())


# ----------------------------------------------------- filter and training step
N_ENT, N_REL, N_TRIPLE = 40, 5, 600  # a random candidate is a known triple with probability 600 / 8000 = 7.5 %


def graph40():
    rng = np.random.default_rng(40)
    flat = rng.choice(N_ENT * N_REL * N_ENT, size=N_TRIPLE, replace=False)
    h, rest = np.divmod(flat, N_REL * N_ENT)
    r, t = np.divmod(rest, N_ENT)
    return np.stack([h, r, t], axis=1).astype(np.int64)


def host_batch_mask(flt, batch, sharding, scheme, flat):
    """negative_mask [step, shard, S, shard, K] with `KnownTripleFilter.mask_host`, from the batch's own tensors."""
    head, rel, tail, neg = (batch[k].cpu().numpy() for k in ("head", "relation", "tail", "negative"))
    l2g = sharding.shard_and_idx_to_entity
    n_step, n, _, per = head.shape
    K = neg.shape[-1]
    p = np.arange(n * per) % per
    heads_replaced = {"h": np.ones(n * per, bool), "t": np.zeros(n * per, bool), "ht": p < per // 2}[scheme]
    out = np.ones((n_step, n, n * per, n, K), dtype=bool)
    for s in range(n_step):
        for d in range(n):
            h = np.concatenate([l2g[d, head[s, d, j]] for j in range(n)])
            t = np.concatenate([l2g[j, tail[s, j, d]] for j in range(n)])
            r = rel[s, d].reshape(-1)
            kept = np.where(heads_replaced, t, h)
            for src in range(n):
                block = neg[s, src, d]  # [B, K]
                if flat:
                    block = block[(~heads_replaced).astype(int) if scheme == "ht" else np.zeros(n * per, int)]
                out[s, d, :, src] = flt.mask_host(kept, r, heads_replaced.astype(np.uint8), l2g[src, block])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n_shard", [1, 2])
@pytest.mark.parametrize("scheme, flat", [("t", False), ("ht", False), ("h", True), ("ht", True)])
def test_filter_masks_the_weighted_draw(dev, n_shard, scheme, flat):
    """With `filter_triples` the batch gains the mask of `mask_host` on the same draw; nothing else changes - also for
    a rank that draws one shard and has to fetch the other shards' running sums for the filter."""
    from besskge.device_sampler import DeviceBatchSampler

    triples = graph40()
    w = 1 + (np.arange(N_ENT) % 5) * 1000
    kw = dict(weights=w, n_entity=N_ENT, n_rel=N_REL, triples=triples, K=6)
    host, twin = make(n_shard, 8 * n_shard, scheme, flat, False, False, **kw)
    sharding = host.negative_sampler.sharding
    flt = KnownTripleFilter([triples], N_ENT, N_REL)
    filtered = DeviceBatchSampler(twin, dev, filter_triples=[triples])
    _, twin_r = make(n_shard, 8 * n_shard, scheme, flat, False, False, **kw)
    last = DeviceBatchSampler(twin_r, dev, shards=range(n_shard - 1, n_shard), filter_triples=flt)
    for step in range(2):
        want, got, own = host[[0]], filtered.sample(), last.sample()
        assert set(got) == set(want) | {"negative_mask"}
        for k in want:
            same(got[k], want[k], k)
            same(own[k], want[k][:, n_shard - 1:], k)
        mask = host_batch_mask(flt, want, sharding, scheme, flat)
        assert mask.any() and not mask.all()
        assert got["negative_mask"].dtype == torch.bool
        assert np.array_equal(got["negative_mask"].cpu().numpy(), mask)
        assert np.array_equal(own["negative_mask"].cpu().numpy(), mask[:, n_shard - 1:])


@pytest.mark.gpu
def test_device_sampled_batch_feeds_the_training_step(dev):
    """One `EmbeddingMovingBessKGE` SGD step (TransE, d = 32, two shards in lock-step) on the device-sampled batch and
    on the host-sampled batch moved to the device: the same tensors go in, so loss and tables come out equal bit for
    bit.  Two things keep the step itself reproducible, so that the comparison says something about its inputs:
    SGD with momentum sums every entity row's contributions in a fixed order (`bess_coalesced_update`; plain SGD adds
    them with fp32 atomics, whose order changes from run to run), and every triple has a relation of its own, drawn
    once (rigid batch sampler) - the relation gradient is summed with fp32 atomics under every optimiser, and a sum of
    at most two terms (a triple's positive and its negatives) does not depend on their order.  With 7 relations shared
    by the 96 triples the two runs' relation tables differed by 1.8e-7 on an MI355X, loss and entity table were equal."""
    from besskge import runtime
    from besskge.bess import EmbeddingMovingBessKGE
    from besskge.device_sampler import DeviceBatchSampler
    from besskge.loss import LogSigmoidLoss
    from besskge.scoring import TransE

    n_shard, d, n_rel = 2, 32, 4000
    rng = np.random.default_rng(6)
    triples = np.stack([rng.integers(1000, size=n_rel), np.arange(n_rel), rng.integers(1000, size=n_rel)], axis=1)
    host, twin = make(n_shard, 48, "t", False, False, True, bps=1, n_rel=n_rel, triples=triples)
    sharding = host.negative_sampler.sharding
    idx = list(host.get_dataloader_sampler(shuffle=False))[0]
    from_host = {k: v.to(dev) for k, v in host[idx].items()}
    from_dev = DeviceBatchSampler(twin, dev).sample(idx)
    assert bool(from_host["triple_mask"].all()) and len(np.unique(from_host["relation"].cpu().numpy())) == 2 * 48
    gen = torch.Generator().manual_seed(5)
    ent = 0.5 * torch.randn(n_shard, sharding.max_entity_per_shard, d, generator=gen)
    rel = 0.5 * torch.randn(n_rel, d, generator=gen)
    res = []
    for batch in (from_host, from_dev):
        fn = TransE(False, 1, sharding, n_rel, d, ent.clone(), rel.clone())
        model = EmbeddingMovingBessKGE(host.negative_sampler, fn, LogSigmoidLoss(3.0, True, 0.5))
        runner = runtime.training_model(model, runtime.Options(device_iterations=1), runtime.SGD(lr=0.1, momentum=0.9),
                                        device=dev)
        out = runner(**{k: batch[k][0] for k in ("head", "relation", "tail", "negative")})
        torch.cuda.synchronize()
        res.append((out["loss"].detach().cpu().clone(), fn.entity_embedding.detach().cpu().clone(),
                    fn.relation_embedding.detach().cpu().clone()))
    assert not torch.equal(res[0][1], ent) and not torch.equal(res[0][2], rel)  # the step moved both tables
    for a, b, what in zip(res[0], res[1], ("loss", "entity table", "relation table")):
        assert torch.equal(a, b), (what, float((a - b).abs().max()))
