"""Filtered evaluation with the filter made on the device (`AllScoresPipeline(filter_triples=KnownTripleFilter(...))`,
`device_filter=True`): the `rank_filter` of a sampler batch equals the host builders' (`get_entity_filter` +
`rank_filter_pairs`) element for element, and ranks, metrics and top-k lists are those of the host path on the
counted-ranks path, the fused top-k path and the matrix path - without `get_entity_filter`, without
`return_triple_idx` on the sampler."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
N_ENTITY, N_REL, D, SHARD_BS, K = 300, 30, 64, 16, 10


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda", 0)


_CASES = {}


def case(scorer, dtype, n_shard, scheme, dev):
    """300 entities, d = 64, one sampler call of 3 (one shard) or 2 (three shards) micro-batches of 16 triples per
    shard, the last one partly padding; filter triples that share (h, r) / (r, t) with test queries, hold the test
    triples themselves and repeat rows; a subset of 240 candidate entities."""
    from besskge.dataset import KGDataset
    from besskge.scoring import ComplEx, TransE
    from besskge.sharding import PartitionedTripleSet, Sharding

    key = (scorer, dtype, n_shard, scheme)
    if key in _CASES:
        return _CASES[key]
    seed = 77 + n_shard
    bps = 3 if n_shard == 1 else 2
    n_triple = bps * n_shard * SHARD_BS - 11
    rng = np.random.default_rng(seed)
    gen = torch.Generator().manual_seed(seed)
    sharding = Sharding.create(N_ENTITY, n_shard, seed=seed)
    width = 2 * D if scorer == "ComplEx" else D
    ent = torch.randn(n_shard, sharding.max_entity_per_shard, width, generator=gen) * 0.3
    rel = torch.randn(N_REL, width, generator=gen) * 0.3
    if dtype == F16:
        ent, rel = ent.half().float(), rel.half().float()
    triples = np.stack([rng.integers(N_ENTITY, size=n_triple), rng.integers(N_REL, size=n_triple),
                        rng.integers(N_ENTITY, size=n_triple)], axis=1)
    extra = np.stack([rng.integers(N_ENTITY, size=600), rng.integers(N_REL, size=600),
                      rng.integers(N_ENTITY, size=600)], axis=1)
    extra[:200, :2] = triples[rng.integers(n_triple, size=200), :2]  # share (h, r) with test queries
    extra[200:400, 1:] = triples[rng.integers(n_triple, size=200), 1:]  # share (r, t)
    extra[400:430] = triples[:30]  # the test triples themselves: their true completion stays
    extra[430:490] = extra[:60]  # repeated rows
    ds = KGDataset(n_entity=N_ENTITY, n_relation_type=N_REL, triples={"test": triples},
                   original_triple_ids={"test": np.arange(n_triple)})
    pts = PartitionedTripleSet.create_from_dataset(ds, "test", sharding,
                                                   partition_mode="h_shard" if scheme == "t" else "t_shard")
    if scorer == "ComplEx":
        fn = ComplEx(True, sharding, N_REL, D, ent, rel)
    else:
        fn = TransE(True, 1, sharding, N_REL, D, ent, rel)
    fn = fn.to(dev)
    if dtype == F16:
        fn = fn.half()
    fn.eval()
    cand = np.sort(rng.choice(N_ENTITY, size=240, replace=False))
    _CASES[key] = dict(sharding=sharding, triples=triples, extra=extra, pts=pts, fn=fn, cand=cand, bps=bps,
                       n_triple=n_triple)
    return _CASES[key]


def sampler(c, scheme, return_triple_idx=True):
    from besskge.batch_sampler import RigidShardedBatchSampler
    from besskge.negative_sampler import PlaceholderNegativeSampler

    return RigidShardedBatchSampler(c["pts"], PlaceholderNegativeSampler(scheme), shard_bs=SHARD_BS,
                                    batches_per_step=c["bps"], seed=5, return_triple_idx=return_triple_idx)


def pipeline(c, scheme, dev, filter_triples, with_cand, bs=None, **kw):
    from besskge.metric import Evaluation
    from besskge.pipeline import AllScoresPipeline

    ev = Evaluation(["mrr", "hits@10"], mode="average", reduction="sum", return_ranks=True)
    return AllScoresPipeline(bs if bs is not None else sampler(c, scheme), scheme, c["fn"], evaluation=ev,
                             filter_triples=filter_triples, candidate_ents=c["cand"] if with_cand else None,
                             window_size=c["sharding"].max_entity_per_shard, device=dev, **kw)


def known_filter(c):
    from besskge.negative_filter import KnownTripleFilter

    return KnownTripleFilter([c["extra"][:350], c["extra"][300:]], N_ENTITY, N_REL)


def same_results(a, b, what):
    assert set(a) == set(b), what
    for key in ("ranks", "topk_global_id", "triple_idx"):
        if key in a:
            assert a[key].dtype == b[key].dtype and torch.equal(a[key], b[key]), f"{what}: {key}"
    for key in ("metrics", "metrics_avg"):
        for m in a[key]:
            assert torch.equal(a[key][m], b[key][m]), f"{what}: {key}[{m}]"


@pytest.mark.parametrize("with_truth", [True, False])
@pytest.mark.parametrize("with_cand", [False, True])
@pytest.mark.parametrize("scheme", ["h", "t"])
@pytest.mark.parametrize("n_shard", [1, 3])
def test_rank_filter_of_a_batch_equals_the_host_builders(dev, n_shard, scheme, with_cand, with_truth):
    """The two builders on one sampler batch: the same [rows, P, 2] tensor - pairs, (slot, entity) order, -1
    padding - and the same number of filtered completions per kept triple."""
    c = case("TransE", F16, n_shard, scheme, dev)
    host = pipeline(c, scheme, dev, [c["extra"]], with_cand)
    device = pipeline(c, scheme, dev, [c["extra"]], with_cand, device_filter=True)
    assert host.known_filter is None and device.known_filter is not None
    assert device.filter_triples is None and not hasattr(device, "triples")  # no host copy of the triples
    batch = dict(next(iter(host.dl)))
    mask = batch.pop("triple_mask")
    truth = batch.pop("head" if scheme == "h" else "tail")
    triple_id = batch.pop("triple_idx")
    assert tuple(mask.shape) == (c["bps"], n_shard, SHARD_BS) and bool(mask.any()) and not bool(mask.all())
    if not with_truth:
        truth = None
    want_filt, want_per_kept = host._filter_pairs(truth, mask, triple_id)
    filt, per_kept = device._filter_pairs(truth, mask, None, batch)
    assert filt.device.type == "cuda" and filt.dtype == want_filt.dtype == torch.int32
    assert tuple(filt.shape) == tuple(want_filt.shape) and want_filt.shape[1] > 4
    assert torch.equal(filt.cpu(), want_filt)
    assert per_kept.dtype == want_per_kept.dtype and torch.equal(per_kept.cpu(), want_per_kept)
    assert int(want_per_kept.max()) >= 2 and int(want_per_kept.min()) < int(want_per_kept.max())
    if with_truth:  # no pair names its query's true completion although the filter holds test triples
        flat_truth = truth.flatten(end_dim=1)
        rows = torch.arange(filt.shape[0])[:, None].expand(filt.shape[:2])
        live = want_filt[..., 0] >= 0
        assert not bool((flat_truth[rows[live], want_filt[..., 0][live].long()] == want_filt[..., 1][live]).any())


RESULT_CASES = [("TransE", F16, 1, "t", True), ("TransE", F16, 3, "h", False),
                ("ComplEx", F32, 3, "t", True), ("ComplEx", F32, 1, "h", False)]


@pytest.mark.parametrize("path", ["counted_ranks", "fused_topk", "matrix"])
@pytest.mark.parametrize("scorer,dtype,n_shard,scheme,with_cand", RESULT_CASES)
def test_results_equal_the_host_filter(dev, scorer, dtype, n_shard, scheme, with_cand, path):
    """A `KnownTripleFilter`, `device_filter=True` and the plain list (the host path) return identical ranks,
    metrics and top-k lists."""
    c = case(scorer, dtype, n_shard, scheme, dev)
    kw = dict(counted_ranks={}, fused_topk=dict(return_topk=True, k=K),
              matrix=dict(return_topk=True, k=K, fused_ranks=False))[path]
    plain = pipeline(c, scheme, dev, [c["extra"]], with_cand, **kw)
    given = pipeline(c, scheme, dev, known_filter(c), with_cand, **kw)
    built = pipeline(c, scheme, dev, [c["extra"]], with_cand, device_filter=True, **kw)
    for pipe in (plain, given, built):
        assert pipe.fused_ranks == (path != "matrix") and pipe.fused_topk == (path == "fused_topk")
    assert given.known_filter is not None and built.known_filter is not None and plain.known_filter is None
    want = plain()
    assert want["ranks"].shape == (c["n_triple"],) and ("topk_global_id" in want) == (path != "counted_ranks")
    same_results(given(), want, "KnownTripleFilter")
    same_results(built(), want, "device_filter=True")
    unfiltered = pipeline(c, scheme, dev, None, with_cand, **kw)()
    assert not torch.equal(unfiltered["ranks"], want["ranks"])  # (the filter matters for these queries)


@pytest.mark.parametrize("path", ["fused_topk", "matrix"])
def test_device_filter_needs_neither_the_host_filter_nor_triple_ids(dev, monkeypatch, path):
    """A sampler without `return_triple_idx` - which the host path refuses - and `get_entity_filter` out of reach:
    the same metrics and lists."""
    import besskge.pipeline

    scheme = "t"
    c = case("TransE", F16, 3, scheme, dev)
    kw = dict(return_topk=True, k=K, fused_ranks=path != "matrix")
    want = pipeline(c, scheme, dev, [c["extra"]], True, **kw)()
    bare = sampler(c, scheme, return_triple_idx=False)
    with pytest.raises(ValueError, match="return_triple_idx"):
        pipeline(c, scheme, dev, [c["extra"]], True, bs=bare, **kw)()

    def unreachable(*a, **k):
        raise AssertionError("get_entity_filter was called")

    monkeypatch.setattr(besskge.pipeline, "get_entity_filter", unreachable)
    for flt, flags in ((known_filter(c), {}), ([c["extra"]], dict(device_filter=True))):
        got = pipeline(c, scheme, dev, flt, True, bs=sampler(c, scheme, return_triple_idx=False), **flags, **kw)()
        assert "triple_idx" not in got
        want_rest = {k: v for k, v in want.items() if k != "triple_idx"}
        same_results(got, want_rest, str(flags))


def test_a_filter_over_other_entities_is_refused(dev):
    from besskge.negative_filter import KnownTripleFilter

    c = case("TransE", F16, 1, "t", dev)
    other = KnownTripleFilter([c["extra"]], N_ENTITY + 1, N_REL)
    with pytest.raises(ValueError, match="301 entities"):
        pipeline(c, "t", dev, other, False)
