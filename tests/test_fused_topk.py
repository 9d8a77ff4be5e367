"""Filtered top-k over all entities without the score matrix: the ordered top-k kernels with exclusion lists
(`bess_topk_update_excl`, `bess_topk_update_flagged_excl`) against a CPU statement of their rule, and
`AllScoresPipeline(fused_topk=True)` against the matrix path (`fused_topk=False`: the code the library had before),
against the unsharded CPU oracle, and against a memory bound that the matrix cannot meet.

Share of top-10 positions that agree with the unsharded oracle (`test_topk_against_the_unsharded_oracle` prints
them before it asserts): see DESIGN.md, "Filtered top-k without the score matrix"."""

import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import kge  # noqa: E402

from test_hip_parity import make_scorer, widths  # noqa: E402
from test_oracle import T  # noqa: E402

ID_NONE = 2**31 - 1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------ the kernels' rule
def rule_topk(scores, ids, excluded, kk, round16):
    """The rule, on the CPU: remove the excluded candidates, sort the rest by (score descending, id ascending) -
    a stable sort by descending score of the candidates laid out by ascending id - and keep kk.  `round16`: the
    fp16-rounded scores are what is sorted (and returned).  Every row must keep kk candidates (asserted)."""
    s = scores.half().float() if round16 else scores.clone()
    assert bool(torch.isfinite(s).all())
    assert int((~excluded).sum(-1).min()) >= kk
    by_id = torch.sort(ids.long(), dim=1, stable=True)
    s = torch.gather(torch.where(excluded, torch.full_like(s, -torch.inf), s), 1, by_id.indices)
    top = torch.sort(s, dim=1, descending=True, stable=True)
    return top.values[:, :kk].contiguous(), torch.gather(by_id.values, 1, top.indices[:, :kk]).to(torch.int32)


def csr(excl_lists, dev):
    ptr = np.zeros(len(excl_lists) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(x) for x in excl_lists])
    flat = np.concatenate([np.sort(np.asarray(x, dtype=np.int64)) for x in excl_lists] + [np.zeros(0, dtype=np.int64)])
    return (torch.from_numpy(ptr.astype(np.int32)).to(dev), torch.from_numpy(flat.astype(np.int32)).to(dev))


def empty_lists(rows, kk, dev):
    return (torch.full((rows, kk), -torch.inf, device=dev),
            torch.full((rows, kk), ID_NONE, dtype=torch.int32, device=dev))


def padded(x, pad, dev):
    """`x` on the device with 16-B aligned rows (the kernels' vector loads) or as it is (scalar loads)."""
    if not pad:
        return x.to(dev)
    ld = (x.shape[1] + 3) // 4 * 4
    buf = torch.zeros(x.shape[0], ld, device=dev)
    buf[:, : x.shape[1]] = x.to(dev)
    return buf[:, : x.shape[1]]


@pytest.mark.parametrize("kk", [1, 10, 64, 65, 128])
@pytest.mark.parametrize("rows,L,pad,id_mode,round16", [
    (37, 2051, True, "shuffled_rows", False),   # four waves per row, 16-B loads, per-row ids in shuffled order
    (37, 2051, False, "base", True),            # scalar loads (odd leading dimension), id_base, fp16 ranking
    (6200, 701, True, "shuffled_one", True),    # one wave per row, one shared row of shuffled ids
    (6200, 701, False, "base", False),
])
def test_ordered_topk_with_exclusions_follows_the_rule(dev, rows, L, pad, id_mode, round16, kk):
    """Scores drawn from eight values (ties dominate; with `round16` some of the eight collapse in fp16); rows
    without exclusions, rows whose every top-valued candidate is excluded, rows with random exclusions; two tiles
    merged into one list in both orders."""
    from besskge import _native as nat

    gen = torch.Generator().manual_seed(rows + L + kk)
    vals = 1.0 + torch.arange(8).float() * (3e-4 if round16 else 0.37)  # (fp16 spacing at 1: 9.8e-4)
    sc = vals[torch.randint(0, 8, (rows, L), generator=gen)]
    base = 1000
    if id_mode == "base":
        ids = (base + torch.arange(L, dtype=torch.int32))[None, :].expand(rows, L).contiguous()
    elif id_mode == "shuffled_one":
        ids = (base + torch.randperm(L, generator=gen).to(torch.int32))[None, :].expand(rows, L).contiguous()
    else:
        ids = base + torch.argsort(torch.rand(rows, L, generator=gen), dim=1).to(torch.int32)
    excluded = torch.zeros(rows, L, dtype=torch.bool)
    top_valued = sc == vals[-1]
    excluded[1::3] = top_valued[1::3]
    excluded[2::3] = torch.rand(rows, L, generator=gen)[2::3] < 0.02
    lists = [ids[r][excluded[r]].tolist() + ([7, base + L + 5] if r % 2 else []) for r in range(rows)]  # (+ ids no candidate has)
    ptr, flat = csr(lists, dev)
    want_s, want_i = rule_topk(sc, ids, excluded, kk, round16)
    cut = L // 2 + 3
    for order in ((0, 1), (1, 0)):
        bs, bi = empty_lists(rows, kk, dev)
        for t in order:
            c0, c1 = (0, cut) if t == 0 else (cut, L)
            tile = padded(sc[:, c0:c1], pad, dev)
            kw = dict(excl_ptr=ptr, excl_ids=flat, round_f16=round16)
            if id_mode == "base":
                nat.topk_update_excl(tile, bs, bi, id_base=base + c0, **kw)
            elif id_mode == "shuffled_one":
                nat.topk_update_excl(tile, bs, bi, ids=ids[:1, c0:c1].contiguous().to(dev), **kw)
            else:
                nat.topk_update_excl(tile, bs, bi, ids=ids[:, c0:c1].contiguous().to(dev), **kw)
        torch.cuda.synchronize()
        assert torch.equal(bs.cpu(), want_s), f"scores, tiles in order {order}"
        assert torch.equal(bi.cpu(), want_i), f"ids, tiles in order {order}"
    assert bool((want_s[:, 1:] == want_s[:, :-1]).any()) or kk == 1  # (the case has ties inside the lists)


@pytest.mark.parametrize("kk", [10, 100])
def test_a_row_with_five_thousand_exclusions(dev, kk):
    """A hub query: one row leaves out 5000 candidates, among them all of its best ones; its neighbours none."""
    from besskge import _native as nat

    gen = torch.Generator().manual_seed(kk)
    rows, L = 9, 9001
    sc = torch.randn(rows, L, generator=gen)
    sc[:, 0:9000:5] = sc[:, 1:9001:5]  # and equal scores
    ids = torch.argsort(torch.rand(rows, L, generator=gen), dim=1).to(torch.int32)
    excluded = torch.zeros(rows, L, dtype=torch.bool)
    hub = 4
    excluded[hub, torch.topk(sc[hub], 3000).indices] = True
    excluded[hub, torch.randperm(L, generator=gen)[:2500]] = True
    extra = torch.randperm(L, generator=gen)
    extra = extra[~excluded[hub, extra]][: 5000 - int(excluded[hub].sum())]
    excluded[hub, extra] = True
    assert int(excluded[hub].sum()) == 5000
    excluded[7, torch.topk(sc[7], 3).indices] = True
    ptr, flat = csr([ids[r][excluded[r]].tolist() for r in range(rows)], dev)
    want_s, want_i = rule_topk(sc, ids, excluded, kk, False)
    bs, bi = empty_lists(rows, kk, dev)
    nat.topk_update_excl(padded(sc, True, dev), bs, bi, ids=ids.to(dev), excl_ptr=ptr, excl_ids=flat)
    torch.cuda.synchronize()
    assert torch.equal(bs.cpu(), want_s) and torch.equal(bi.cpu(), want_i)


@pytest.mark.parametrize("scorer,dtype,W,kk", [("TransE", torch.float16, 64, 10), ("TransE", torch.float16, 64, 100),
                                               ("ComplEx", torch.float32, 128, 10), ("ComplEx", torch.float32, 128, 65)])
def test_flagged_ordered_topk_follows_the_rule(dev, scorer, dtype, W, kk):
    """A dense first tile, then a tile pruned by `bess_neg_score_shared_fwd_pruned` against thresholds strictly
    below the rows' k-th scores, read through its flags: the lists of the rule applied to all the scores (those of
    the pruned kernel with nothing pruned), with shuffled global ids and exclusion lists; fp16 tables rank
    fp16-rounded scores, where ties are frequent."""
    from besskge import _native as nat
    from besskge.query import threshold_below

    gen = torch.Generator().manual_seed(W + kk)
    nq, n_ent, first = 300, 40_000 - 37, 8192
    half = dtype == torch.float16
    table = (torch.randn(n_ent, W, generator=gen) * 0.3).to(dtype).to(dev)
    q = (torch.randn(nq, W, generator=gen) * 0.3).to(dev)
    code = dict(ComplEx=nat.COMPLEX, TransE=nat.TRANSE)[scorer]
    d = nat.make_desc(code, 1 if scorer == "TransE" else 0, table, W)
    gid = torch.randperm(n_ent + 500, generator=gen)[:n_ent].to(torch.int32)
    a = nat.neg_score_shared_fwd(d, q, nat.RowSource(table[:first]), pad_ld=True)
    everything = torch.full((nq,), -torch.inf, device=dev)
    b_all, f_all = nat.neg_score_shared_fwd_pruned(d, q, nat.RowSource(table[first:]), everything)
    assert bool(f_all[:, : (n_ent - first + 63) // 64].bool().all())
    full = torch.cat([a[:, :first], b_all[:, : n_ent - first]], dim=1).cpu()
    if half:
        full = full.half().float()
    excluded = torch.zeros(nq, n_ent, dtype=torch.bool)
    best = torch.topk(full, 40, dim=1).indices
    excluded[torch.arange(nq)[:, None], best[:, ::2]] = True  # every other one of the 40 best
    excluded[::4] = False
    ids2d = gid[None, :].expand(nq, n_ent)
    ptr, flat = csr([gid[excluded[r]].tolist() for r in range(nq)], dev)
    want_s, want_i = rule_topk(full, ids2d, excluded, kk, half)
    bs, bi = empty_lists(nq, kk, dev)
    kw = dict(excl_ptr=ptr, excl_ids=flat, round_f16=half)
    nat.topk_update_excl(a, bs, bi, ids=gid[None, :first].contiguous().to(dev), **kw)
    thr = threshold_below(bs[:, kk - 1], half)
    b, flags = nat.neg_score_shared_fwd_pruned(d, q, nat.RowSource(table[first:]), thr)
    nat.topk_update_excl(b, bs, bi, ids=gid[None, first:].contiguous().to(dev), flags=flags, **kw)
    torch.cuda.synchronize()
    share = float(flags[:, : (n_ent - first + 63) // 64].bool().float().mean())
    ties = float((want_s[:, 1:] == want_s[:, :-1]).float().mean())
    print(f"{scorer} kk={kk}: {share:.3f} of the second tile's blocks flagged; {ties:.3f} of neighbours in the lists tie")
    assert share < 0.9, "nothing was pruned: the flagged path was not exercised"
    assert torch.equal(bs.cpu(), want_s)
    assert torch.equal(bi.cpu(), want_i)
    if half:
        assert ties > 0


# ------------------------------------------------------------------------------------------------ the pipeline
def pipeline_case(scorer, dtype, n_entity, n_shard, shard_bs, scheme, dev, seed=99, d=64, n_rel=30, scale=0.3):
    """The construction of tests/test_query.py:262-285 (filter triples that share (h, r) / (r, t) with many test
    queries, the test triples themselves and duplicates among them; a candidate subset; a padded last batch)."""
    from besskge.batch_sampler import RigidShardedBatchSampler
    from besskge.dataset import KGDataset
    from besskge.negative_sampler import PlaceholderNegativeSampler
    from besskge.sharding import PartitionedTripleSet, Sharding

    n_triple = 3 * n_shard * shard_bs - 17
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    sharding = Sharding.create(n_entity, n_shard, seed=seed)
    ew, rw = widths(scorer, d)
    ent = torch.randn(n_shard, sharding.max_entity_per_shard, ew) * scale
    rel = torch.randn(n_rel, rw) * scale
    if dtype == torch.float16:
        ent, rel = ent.half().float(), rel.half().float()
    triples = np.stack([rng.integers(n_entity, size=n_triple), rng.integers(n_rel, size=n_triple),
                        rng.integers(n_entity, size=n_triple)], axis=1)
    extra = np.stack([rng.integers(n_entity, size=4000), rng.integers(n_rel, size=4000),
                      rng.integers(n_entity, size=4000)], axis=1)
    extra[:1500, :2] = triples[rng.integers(n_triple, size=1500), :2]  # share (h, r) with test queries
    extra[1500:3000, 1:] = triples[rng.integers(n_triple, size=1500), 1:]  # share (r, t)
    extra[3000:3200] = triples[:200]  # the test triples themselves: their true completion must stay
    extra[3200:3400] = extra[:200]    # duplicates
    ds = KGDataset(n_entity=n_entity, n_relation_type=n_rel, triples={"test": triples},
                   original_triple_ids={"test": np.arange(n_triple)})
    pts = PartitionedTripleSet.create_from_dataset(ds, "test", sharding,
                                                   partition_mode="h_shard" if scheme == "t" else "t_shard")
    p = 0 if scorer in ("ComplEx", "DistMult") else 1
    fn = make_scorer(scorer, p, True, n_rel, d, ent, rel, dev, dtype=dtype, sharding=sharding)
    fn.eval()
    bs = RigidShardedBatchSampler(pts, PlaceholderNegativeSampler(scheme), shard_bs=shard_bs, batches_per_step=2,
                                  seed=seed, return_triple_idx=True)
    cand = np.sort(rng.choice(n_entity, size=max(4000, int(0.8 * n_entity)), replace=False))
    return dict(sharding=sharding, ent=ent, rel=rel, triples=triples, extra=extra, pts=pts, fn=fn, bs=bs, cand=cand,
                n_triple=n_triple, p=p)


def spy(pipe, name):
    seen = []
    inner = getattr(pipe, name)
    setattr(pipe, name, lambda *a, **k: (seen.append(inner(*a, **k)), seen[-1])[1])
    return seen


F16, F32 = torch.float16, torch.float32
PIPELINE_CASES = [  # scorer, dtype, n_entity, n_shard, shard_bs, scheme, k, evaluation
    # one per-element arithmetic whatever the window: exact equality at any window_size
    ("PairRE", F16, 20_000, 1, 80, "t", 10, True),
    ("PairRE", F16, 20_000, 2, 80, "h", 100, False),
    ("PairRE", F16, 20_000, 4, 40, "t", 100, True),
    ("TranS", F32, 6_000, 2, 80, "h", 10, True),
    ("TranS", F32, 6_000, 4, 40, "t", 100, False),
    ("BoxE", F32, 6_000, 1, 80, "t", 100, True),
    ("BoxE", F32, 6_000, 2, 80, "h", 10, False),
    # windows that take the same kernel as the all-entity pass (tests/test_query.py:570-572)
    ("ComplEx", F32, 60_000, 2, 160, "t", 10, True),
    ("ComplEx", F32, 60_000, 2, 160, "h", 100, False),
    ("TransE", F16, 20_000, 2, 80, "t", 100, True),
    ("TransE", F16, 20_000, 4, 40, "h", 10, False),
    ("TransE", F16, 20_000, 1, 80, "h", 10, True),
]


@pytest.mark.parametrize("scorer,dtype,n_entity,n_shard,shard_bs,scheme,k,with_ev", PIPELINE_CASES)
def test_pipeline_topk_lists_equal_the_matrix_path(dev, scorer, dtype, n_entity, n_shard, shard_bs, scheme, k, with_ev):
    """`topk_global_id` of `fused_topk=True` is that of `fused_topk=False` (filter, candidate subset, padded last
    batch; every query keeps far more than k candidates, so every position of the matrix path's lists holds a
    finite score); with an evaluation the ranks are those of the counted path alone."""
    from besskge.metric import Evaluation
    from besskge.pipeline import AllScoresPipeline

    c = pipeline_case(scorer, dtype, n_entity, n_shard, shard_bs, scheme, dev)
    sharding = c["sharding"]
    ev = Evaluation(["mrr", "hits@10"], mode="average", reduction="sum", return_ranks=True)
    window = sharding.max_entity_per_shard if scorer == "ComplEx" else 1000
    kw = dict(evaluation=ev, filter_triples=[c["extra"]], candidate_ents=c["cand"], window_size=window, device=dev)
    fused = AllScoresPipeline(c["bs"], scheme, c["fn"], return_topk=True, k=k, **kw)
    plain = AllScoresPipeline(c["bs"], scheme, c["fn"], return_topk=True, k=k, fused_topk=False, **kw)
    assert fused.fused_topk and fused.fused_ranks and not plain.fused_topk and not plain.fused_ranks
    if scorer == "ComplEx":
        # (the split-fp16 product needs 256 output tiles: one tile per shard, the shape the matrix path's window has)
        fused.bess_module.topk_first_tile = sharding.max_entity_per_shard
    else:
        fused.bess_module.topk_first_tile = 1024  # several pruned tiles per shard
    if not with_ev:
        # (the constructor insists on something to return next to the lists: the evaluation is taken away after it)
        for pipe in (fused, plain):
            pipe.evaluation = None
            pipe.fused_ranks = False
    seen = spy(fused, "_topk_by_lists")
    a, b = fused(), plain()
    assert seen and all(t is not None for t in seen), "a batch left the fused path"
    assert torch.equal(a["triple_idx"], b["triple_idx"])
    assert a["topk_global_id"].shape == (c["n_triple"], k) and a["topk_global_id"].dtype == b["topk_global_id"].dtype
    diff = (a["topk_global_id"] != b["topk_global_id"])
    print(f"{scorer} n_shard={n_shard} {scheme} k={k}: {int(diff.sum())} of {diff.numel()} positions differ")
    assert torch.equal(a["topk_global_id"], b["topk_global_id"])
    # the lists honour the filter and the subset, and keep the true completion of a test triple that is filtered
    order = c["pts"].triple_sort_idx[a["triple_idx"].numpy()]
    tr = c["triples"][order]
    col, other = (0, 2) if scheme == "t" else (2, 0)
    is_cand = np.zeros(n_entity, dtype=bool)
    is_cand[c["cand"]] = True
    lists = a["topk_global_id"].numpy()
    assert is_cand[lists].all()
    for i in range(0, len(tr), 7):
        hit = c["extra"][(c["extra"][:, col] == tr[i, col]) & (c["extra"][:, 1] == tr[i, 1])][:, other]
        assert not (set(hit.tolist()) - {int(tr[i, other])}) & set(lists[i].tolist())
    if with_ev:
        only_ranks = AllScoresPipeline(c["bs"], scheme, c["fn"], **kw)
        assert only_ranks.fused_ranks and not only_ranks.fused_topk
        r = only_ranks()
        assert torch.equal(a["ranks"], r["ranks"]) and torch.equal(a["ranks"], b["ranks"])
        torch.testing.assert_close(a["metrics"]["mrr"], b["metrics"]["mrr"], rtol=1e-3, atol=1e-3)
    else:
        assert "metrics" not in a and "ranks" not in a


@pytest.mark.parametrize("scheme", ["h", "t"])
def test_topk_against_the_unsharded_oracle(dev, scheme):
    """The construction of tests/test_query.py:288-323 (ComplEx, 4 shards, filter + candidate subset): the share
    of top-10 positions that agree with the CPU oracle stays above the 0.99 which that test demands of the matrix
    path - checked for the matrix path first, then for the lists."""
    from besskge.batch_sampler import RigidShardedBatchSampler
    from besskge.dataset import KGDataset
    from besskge.metric import Evaluation
    from besskge.negative_sampler import PlaceholderNegativeSampler
    from besskge.pipeline import AllScoresPipeline
    from besskge.scoring import ComplEx
    from besskge.sharding import PartitionedTripleSet, Sharding

    seed, n_entity, n_rel, n_shard, n_triple, d = 1234, 5000, 50, 4, 640, 64
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    sharding = Sharding.create(n_entity, n_shard, seed=seed)
    ent = torch.randn(n_shard, sharding.max_entity_per_shard, 2 * d)
    rel = torch.randn(n_rel, 2 * d)
    triples = np.stack([rng.integers(n_entity, size=n_triple), rng.integers(n_rel, size=n_triple),
                        rng.integers(n_entity, size=n_triple)], axis=1)
    extra = np.stack([rng.integers(n_entity, size=3000), rng.integers(n_rel, size=3000),
                      rng.integers(n_entity, size=3000)], axis=1)
    extra[:600, :2] = triples[rng.integers(n_triple, size=600), :2]
    extra[600:1200, 1:] = triples[rng.integers(n_triple, size=600), 1:]
    ds = KGDataset(n_entity=n_entity, n_relation_type=n_rel, triples={"test": triples},
                   original_triple_ids={"test": np.arange(n_triple)})
    pts = PartitionedTripleSet.create_from_dataset(ds, "test", sharding,
                                                   partition_mode="h_shard" if scheme == "t" else "t_shard")
    fn = ComplEx(True, sharding, n_rel, d, ent, rel)
    bs = RigidShardedBatchSampler(pts, PlaceholderNegativeSampler(scheme), shard_bs=80, batches_per_step=2,
                                  seed=seed, return_triple_idx=True)
    ev = Evaluation(["mrr", "hits@10"], mode="average", reduction="sum", return_ranks=True)
    cand_ents = np.sort(rng.choice(n_entity, size=4000, replace=False))
    kw = dict(evaluation=ev, filter_triples=[extra], candidate_ents=cand_ents, return_topk=True, k=10,
              window_size=500, device=dev)
    shares = {}
    for fused_topk in (False, True):
        pipe = AllScoresPipeline(bs, scheme, fn, fused_topk=fused_topk, **kw)
        assert pipe.fused_topk == fused_topk
        pipe.bess_module.topk_first_tile = 512
        out = pipe()
        tr = triples[pts.triple_sort_idx[out["triple_idx"].numpy()]]
        flat = ent[sharding.entity_to_shard, sharding.entity_to_idx]
        known, truth = (tr[:, 0], tr[:, 2]) if scheme == "t" else (tr[:, 2], tr[:, 0])
        want = kge.score_candidates("ComplEx", 0, True, scheme, flat[known], rel, T(tr[:, 1]), flat[None])
        rows = torch.arange(len(tr))
        want[:, T(np.setdiff1d(np.arange(n_entity), cand_ents))] = -torch.inf
        true_sc = want[rows, T(truth)].clone()
        col, other = (0, 2) if scheme == "t" else (2, 0)
        for i, (a_, r_) in enumerate(zip(tr[:, col], tr[:, 1])):
            want[i, T(extra[(extra[:, col] == a_) & (extra[:, 1] == r_)][:, other])] = -torch.inf
        want[rows, T(truth)] = true_sc
        top = torch.topk(want, 10, dim=-1)
        finite = torch.isfinite(top.values).all(-1)
        shares[fused_topk] = float((out["topk_global_id"][finite] == top.indices[finite]).float().mean())
        print(f"scheme {scheme} fused_topk={fused_topk}: share of top-10 positions equal to the oracle's "
              f"{shares[fused_topk]:.5f}")
    assert shares[False] > 0.99, "the seeds do not meet the bound on the matrix path"
    assert shares[True] > 0.99


def test_no_score_matrix_is_made(dev):
    """With the score-tile budget at 8 MiB and a [queries, n_entity] fp32 matrix of 156 MiB per sampler batch, the
    call's peak allocation rises by less than half the matrix with `fused_topk=True` - and by more than the matrix
    without."""
    from besskge.metric import Evaluation
    from besskge.pipeline import AllScoresPipeline

    n_entity, shard_bs = 40_000, 512
    c = pipeline_case("TransE", F16, n_entity, 1, shard_bs, "t", dev)
    ev = Evaluation(["mrr"], mode="average", reduction="sum", return_ranks=True)
    kw = dict(evaluation=ev, filter_triples=[c["extra"]], return_topk=True, k=10, window_size=1000, device=dev)
    n_query = 2 * shard_bs  # one sampler batch: batches_per_step x shards x shard_bs
    matrix = n_query * n_entity * 4
    assert matrix >= 64 << 20
    rise = {}
    for fused_topk in (True, False):
        pipe = AllScoresPipeline(c["bs"], "t", c["fn"], fused_topk=fused_topk, **kw)
        pipe.bess_module.topk_tile_bytes = 8 << 20
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = pipe()
        torch.cuda.synchronize()
        rise[fused_topk] = torch.cuda.max_memory_allocated() - before
        assert out["topk_global_id"].shape == (c["n_triple"], 10)
        del pipe, out
    print(f"matrix {matrix} B; rise of the peak allocation: fused {rise[True]} B, matrix path {rise[False]} B")
    assert rise[True] < matrix // 2
    assert rise[False] > matrix


def test_half_precision_model_ties_inside_the_lists(dev):
    """The relation table is fp16, so scores are ranked after rounding to fp16: the lists equal the matrix path's
    although equal scores sit inside them (asserted on the module's own `topk_scores`)."""
    from besskge.metric import Evaluation
    from besskge.pipeline import AllScoresPipeline

    k = 50
    c = pipeline_case("TransE", F16, 20_000, 2, 80, "t", dev, seed=7)
    assert c["fn"].relation_embedding.dtype == torch.float16
    ev = Evaluation(["mrr"], mode="average", reduction="sum", return_ranks=True)
    kw = dict(evaluation=ev, filter_triples=[c["extra"]], candidate_ents=c["cand"], return_topk=True, k=k,
              window_size=1000, device=dev)
    fused = AllScoresPipeline(c["bs"], "t", c["fn"], **kw)
    fused.bess_module.topk_first_tile = 1024
    plain = AllScoresPipeline(c["bs"], "t", c["fn"], fused_topk=False, **kw)
    a, b = fused(), plain()
    assert torch.equal(a["topk_global_id"], b["topk_global_id"])
    batch = next(iter(fused.dl))
    rows = batch["head"].flatten(end_dim=1)
    res = fused.runner(step=torch.zeros((rows.shape[0], 1), dtype=torch.int32), head=rows,
                       relation=batch["relation"].flatten(end_dim=1),
                       topk_k=torch.full((rows.shape[0], 1), k, dtype=torch.int32))
    s = res["topk_scores"]
    assert not bool(res["out_of_range"].any()) and bool(torch.isfinite(s).all())
    assert torch.equal(s, s.half().float())
    tied_rows = (s[:, 1:] == s[:, :-1]).any(dim=1)
    print(f"{float(tied_rows.float().mean()):.3f} of the queries have equal scores inside their top-{k}")
    assert bool(tied_rows.any()), "no equal scores inside any list: the case shows nothing"
    # within a run of equal scores the ids ascend
    g = res["topk_global_id"]
    assert bool((g[:, 1:] > g[:, :-1])[s[:, 1:] == s[:, :-1]].all())


def test_out_of_range_batches_fall_back_to_the_matrix(dev):
    """An operand outside the fp16 range of the split product: the batch is flagged (`out_of_range`) and the
    pipeline takes the matrix path for it - the same lists as the pipeline that never fuses."""
    from besskge.metric import Evaluation
    from besskge.pipeline import AllScoresPipeline

    c = pipeline_case("ComplEx", F32, 60_000, 2, 160, "t", dev, seed=5)
    sharding = c["sharding"]
    h0 = int(c["triples"][7, 0])  # the head of one query: its row makes that query's row of the product huge
    with torch.no_grad():
        c["fn"].entity_embedding.data[sharding.entity_to_shard[h0], sharding.entity_to_idx[h0], :4] = 3.0e5
    ev = Evaluation(["mrr"], mode="average", reduction="sum", return_ranks=True)
    kw = dict(evaluation=ev, filter_triples=[c["extra"]], return_topk=True, k=10,
              window_size=sharding.max_entity_per_shard, device=dev)
    fused = AllScoresPipeline(c["bs"], "t", c["fn"], **kw)
    plain = AllScoresPipeline(c["bs"], "t", c["fn"], fused_topk=False, **kw)
    assert fused.fused_topk
    fused.bess_module.topk_first_tile = sharding.max_entity_per_shard
    # with an evaluation the counted ranks meet the same operand first and send the batch to the matrix before the
    # lists are asked for: the lists' own flag is seen without one (taken away after the constructor, which insists
    # on something to return next to the lists)
    for pipe in (fused, plain):
        pipe.evaluation = None
        pipe.fused_ranks = False
    seen = spy(fused, "_topk_by_lists")
    a, b = fused(), plain()
    # (the huge row is an entity of the table, hence a candidate of every query: every batch's product meets it)
    assert seen and all(t is None for t in seen), "the range flag was lost: a batch did not fall back to the score matrix"
    assert torch.equal(a["topk_global_id"], b["topk_global_id"])
    # and the module's own output says which queries were flagged
    found = False
    for batch in fused.dl:
        rows = batch["head"].flatten(end_dim=1)
        res = fused.runner(step=torch.zeros((rows.shape[0], 1), dtype=torch.int32), head=rows,
                           relation=batch["relation"].flatten(end_dim=1),
                           topk_k=torch.full((rows.shape[0], 1), 10, dtype=torch.int32))
        found |= bool(res["out_of_range"].any())
    assert found
