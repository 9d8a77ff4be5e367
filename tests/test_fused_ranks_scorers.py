"""Ranks counted in the scoring kernels for PairRE / TripleRE / InterHT / TranS (csrc/affine.hip), BoxE
(csrc/boxe.hip) and ConvE (DistMult's kernels): `bess_neg_score_table_fwd_counts` / `_pairs` and
`AllScoresPipeline(fused_ranks=True)` against the score matrix of `nat.neg_score_shared_fwd` - exact equality,
the two paths run one per-element arithmetic - and against the unsharded CPU oracle.

Share of ranks that differ from the oracle at numerical ties, matrix path (`fused_ranks=False`, the path and the
arithmetic the library had before the counted one existed; the counted path inherits the figure through the exact
equality), printed by `test_pipeline_counts_ranks_for_every_scorer` before it asserts: see DESIGN.md, "Counted
ranks for the affine scorers and BoxE"."""

import contextlib
import ctypes

import numpy as np
import pytest
import torch

from oracle import kge  # noqa: E402

from conftest import load_golden  # noqa: E402
from test_hip_parity import make_scorer, widths  # noqa: E402
from test_oracle import T  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda", 0)


def _affine_desc(nat, n_part, d, dtype_code, normalize=True, member=0):
    desc = nat.ModelDesc()
    desc.scorer, desc.norm_p, desc.dtype = nat.AFFINE, 1, dtype_code
    desc.width, desc.rel_width = n_part * d, {0: 2, 1: 3, 2: 1, 3: 3}[member] * d
    desc.reserved[0], desc.reserved[1] = n_part, int(normalize) | (member << 8)
    return desc


# ---------------------------------------------------------------------------------------------- no GPU needed
def test_counting_workspaces_hold_no_scores():
    """Host arithmetic: BoxE counts in its kernel (no workspace - it used to be a 64 MiB score tile); the affine
    family's raw-table form asks for the inverse norms of one candidate chunk, whatever the number of queries."""
    from besskge import _native as nat

    lib = nat.load()
    box = nat.ModelDesc()
    box.scorer, box.norm_p, box.dtype, box.width, box.rel_width = nat.BOXE, 1, nat.F32, 256, 4 * 128 + 2
    box.reserved[0] = 3
    assert lib.bess_neg_score_shared_fwd_counts_workspace(ctypes.byref(box), 4096, 1 << 20) == 0
    assert lib.bess_neg_score_table_fwd_counts_workspace(ctypes.byref(box), 4096, 1 << 20) == 0
    assert lib.bess_neg_score_shared_fwd_pairs_workspace(ctypes.byref(box), 4096, 1 << 20) == 0
    for n_part, dtype_code, member in ((1, nat.F16, 0), (2, nat.F32, 3)):
        aff = _affine_desc(nat, n_part, 256, dtype_code, member=member)
        chunk = nat.affine_count_chunk_rows(aff)
        assert chunk % 64 == 0 and chunk * aff.width * (4 if dtype_code == nat.F32 else 2) <= nat.AFFINE_COUNT_CHUNK_BYTES
        ws = lib.bess_neg_score_table_fwd_counts_workspace(ctypes.byref(aff), 4096, 1 << 20)
        assert ws == lib.bess_neg_score_table_fwd_counts_workspace(ctypes.byref(aff), 17, 1 << 20)
        assert 0 < ws <= chunk * n_part * 4 + 256
        # fewer candidates than a chunk: their norms only
        assert lib.bess_neg_score_table_fwd_counts_workspace(ctypes.byref(aff), 4096, 1000) <= 1000 * n_part * 4 + 256
        aff.reserved[1] &= ~1  # entities not normalised: no norm pass, no workspace
        assert lib.bess_neg_score_table_fwd_counts_workspace(ctypes.byref(aff), 4096, 1 << 20) == 0
        assert lib.bess_neg_score_table_fwd_pairs_workspace(ctypes.byref(aff), 4096, 1 << 20) < (4 << 20)
    # the other scorers: the raw-table names forward to the shared ones
    dm = nat.ModelDesc()
    dm.scorer, dm.norm_p, dm.dtype, dm.width, dm.rel_width = nat.DISTMULT, 0, nat.F32, 128, 128
    for n in ((4096, 1 << 20), (300, 5000)):
        assert lib.bess_neg_score_table_fwd_counts_workspace(ctypes.byref(dm), *n) == \
            lib.bess_neg_score_shared_fwd_counts_workspace(ctypes.byref(dm), *n)
        assert lib.bess_neg_score_table_fwd_pairs_workspace(ctypes.byref(dm), *n) == \
            lib.bess_neg_score_shared_fwd_pairs_workspace(ctypes.byref(dm), *n)


def test_every_scorer_with_a_descriptor_counts_its_ranks():
    from besskge.pipeline import _counting_scorer

    n_rel, d = 5, 8
    cpu = torch.device("cpu")
    for name in ("TransE", "DistMult", "PairRE", "TripleRE", "InterHT", "TranS", "BoxE", "BoxEnt"):
        ew, rw = widths(name, d)
        fn = make_scorer(name, 1 if name not in ("DistMult",) else 0, True, n_rel, d, torch.randn(1, 12, ew),
                         torch.randn(n_rel, rw), cpu)
        assert _counting_scorer(fn), name
    assert not _counting_scorer(object())


# -------------------------------------------------------------------------------------------------------- GPU
CASES = [  # name, p, dtype, indexed, d
    ("PairRE", 1, torch.float16, False, 128),   # normalised, fp16 table, dense
    ("TranS", 2, torch.float32, True, 64),      # two parts, indexed, p = 2
    ("InterHTnn", 1, torch.float32, False, 52),  # not normalised: no norm pass (d % 16 != 0: a zero-filled last stage)
    ("InterHT", 1, torch.float16, True, 52),
    ("BoxE", 1, torch.float32, False, 64),
    ("BoxEnt", 2, torch.float16, True, 64),
    ("PairRE", 2, torch.float16, False, 128),   # the table form at p = 2: one part, both table types ...
    ("PairRE", 2, torch.float32, True, 64),
    ("TranS", 2, torch.float16, True, 64),      # ... and two parts on an fp16 table (tests/test_fused_step_kernels.py)
]


def _scorer_and_queries(name, p, dtype, d, n_ent, nq, dev, gen):
    from besskge import _native as nat

    n_rel = 11
    ew, rw = widths(name.replace("InterHTnn", "InterHT"), d)
    ent = torch.randn(1, n_ent, ew, generator=gen) * 0.3
    rel = torch.randn(n_rel, rw, generator=gen) * 0.3
    if name == "InterHTnn":
        from besskge.scoring import InterHT
        from besskge.sharding import Sharding

        fn = InterHT(True, p, Sharding.create(n_ent, 1, seed=0), n_rel, d, ent, rel, normalize_entities=False, offset=1.0)
        fn = fn.to(dev).half() if dtype == torch.float16 else fn.to(dev)
    else:
        fn = make_scorer(name, p, True, n_rel, d, ent, rel, dev, dtype=dtype)
    table = fn.entity_embedding.data[0]
    known = torch.randint(0, n_ent, (nq,), generator=gen).to(torch.int32).to(dev)
    rid = torch.randint(0, n_rel, (nq,), generator=gen).to(torch.int32).to(dev)
    q = fn.query_fwd(nat.CORRUPT_TAIL, nat.RowSource(table, known), rid)[0]
    return fn, fn.kernel_desc(), table, q


@pytest.mark.gpu
@pytest.mark.parametrize("name,p,dtype,indexed,d", CASES)
def test_counts_in_the_kernel_equal_counts_of_the_stored_scores(dev, name, p, dtype, indexed, d):
    """`nat.neg_score_shared_counts` for the affine family and BoxE: the counts of the stored score matrix of
    `nat.neg_score_shared_fwd`, exactly - with no score matrix, score tile or f32 copy of the candidates made."""
    from besskge import _native as nat

    gen = torch.Generator().manual_seed(d + int(indexed))
    nq, n_ent = 300, 40_000
    n_cand = n_ent - 37  # a ragged last tile
    fn, desc, table, q = _scorer_and_queries(name, p, dtype, d, n_ent, nq, dev, gen)
    if indexed:
        idx = torch.randperm(n_ent, generator=gen)[:n_cand].to(torch.int32).to(dev)
        src = nat.RowSource(table, idx)
    else:
        src = nat.RowSource(table[:n_cand])
    sc = nat.neg_score_shared_fwd(desc, q, src)
    excl = torch.randint(0, n_cand, (nq,), generator=gen).to(torch.int32)
    excl[::7] = -1
    excl[5], excl[6] = 0, n_cand - 1  # first and last column
    excl = excl.to(dev)
    rows = torch.arange(nq, device=dev)
    thr = torch.where(excl >= 0, sc[rows, excl.clamp(min=0).long()], sc[rows, 17])
    thr[3] = float("inf")
    thr[4] = -float("inf")
    thr = thr.contiguous()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    counts = nat.neg_score_shared_counts(desc, q, src, thr, excl)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - torch.cuda.memory_allocated()
    print(f"{name}: peak allocation added by the counting call {extra} B")
    assert extra < nq * n_cand * 4, "a score matrix / tile was allocated"
    if desc.scorer == nat.AFFINE:
        assert extra < n_cand * desc.width * 4, "an f32 copy of the candidates was allocated"
    keep = torch.ones_like(sc, dtype=torch.bool)
    keep[rows[excl >= 0], excl[excl >= 0].long()] = False
    assert torch.equal(counts[:, 0].long(), ((sc > thr[:, None]) & keep).sum(-1))
    assert torch.equal(counts[:, 1].long(), ((sc == thr[:, None]) & keep).sum(-1))
    assert int(counts[excl < 0][:, 1].min()) >= 1  # (rows without an exclusion tie with their column 17)
    assert int(counts[3].sum()) == 0 and int(counts[4, 0]) == n_cand - 1
    # accumulation over two windows into the same counters
    half = (n_cand // 2) // 64 * 64 + 13
    if indexed:
        a, b = nat.RowSource(table, idx[:half].contiguous()), nat.RowSource(table, idx[half:].contiguous())
    else:
        a, b = nat.RowSource(table[:half]), nat.RowSource(table[half:n_cand])
    c2 = nat.neg_score_shared_counts(desc, q, a, thr, torch.where(excl < half, excl, torch.full_like(excl, -1)))
    ex_b = torch.where(excl >= half, excl - half, torch.full_like(excl, -1))
    c2 = nat.neg_score_shared_counts(desc, q, b, thr, ex_b, counts=c2)
    assert torch.equal(c2, counts)
    # a half-precision model ranks fp16 scores: many ties
    sc16, thr16 = sc.half().float(), thr.half().float().contiguous()
    c16 = nat.neg_score_shared_counts(desc, q, src, thr16, excl, round_f16=True)
    assert torch.equal(c16[:, 0].long(), ((sc16 > thr16[:, None]) & keep).sum(-1))
    assert torch.equal(c16[:, 1].long(), ((sc16 == thr16[:, None]) & keep).sum(-1))
    assert int(c16[:, 1].sum()) > int(counts[:, 1].sum())


@pytest.mark.gpu
@pytest.mark.parametrize("name,p,dtype,indexed,d", CASES)
def test_pair_scores_equal_the_score_matrix_elements(dev, name, p, dtype, indexed, d):
    """`nat.neg_score_shared_pairs`: score(query i, table row c_i) is element [i, c_i] of the stored matrix, bit
    for bit - diagonal tiles of the affine tile kernel (more than one chunk of 8192 pairs, a ragged last tile),
    BoxE's kernel with one candidate per query."""
    from besskge import _native as nat

    gen = torch.Generator().manual_seed(d)
    nq, n_cand = 300, 3_000
    fn, desc, table, q = _scorer_and_queries(name, p, dtype, d, n_cand + 50, nq, dev, gen)
    sc = nat.neg_score_shared_fwd(desc, q, nat.RowSource(table[:n_cand]))
    n_pair = 8192 + 1000 + 37
    g = torch.randint(0, nq, (n_pair,), generator=gen).to(dev)
    cols = torch.randint(0, n_cand, (n_pair,), generator=gen).to(torch.int32).to(dev)
    got = nat.neg_score_shared_pairs(desc, q[g].contiguous(), nat.RowSource(table, cols), nq, n_cand)
    assert torch.equal(got, sc[g, cols.long()])


PIPELINE_SCORERS = [
    ("PairRE", torch.float16, 20_000, 2, 80),
    ("TripleRE", torch.float32, 6_000, 3, 40),
    ("TranS", torch.float32, 5_000, 4, 80),
    ("BoxE", torch.float32, 6_000, 2, 80),
    ("BoxEnt", torch.float16, 5_000, 3, 40),
    ("ConvE", torch.float32, 5_000, 2, 80),  # (DistMult's kernels: a pin; ConvE scores tails only)
]
PIPELINE_RUNS = [("t", False, "average"), ("h", True, "optimistic"), ("t", True, "pessimistic")]


@pytest.mark.gpu
@pytest.mark.parametrize("scorer,dtype,n_entity,n_shard,shard_bs,scheme,filtered,mode",
                         [s + r for s in PIPELINE_SCORERS for r in PIPELINE_RUNS if not (s[0] == "ConvE" and r[0] == "h")])
def test_pipeline_counts_ranks_for_every_scorer(dev, scorer, dtype, n_entity, n_shard, shard_bs, scheme, filtered, mode):
    """AllScoresPipeline with only metrics / ranks asked for takes the counted path for the affine family, BoxE
    and ConvE: the ranks of the matrix path to the last bit, and the ranks of the unsharded CPU oracle up to
    numerical ties (0.03 of the ranks in fp32, 0.05 in fp16: the bounds of the four native scorers' test)."""
    from besskge.batch_sampler import RigidShardedBatchSampler
    from besskge.dataset import KGDataset
    from besskge.metric import Evaluation
    from besskge.negative_sampler import PlaceholderNegativeSampler
    from besskge.pipeline import AllScoresPipeline
    from besskge.sharding import PartitionedTripleSet, Sharding

    seed, n_rel, d = 99, 30, 64
    net = None
    if scorer == "ConvE":
        g = load_golden("scoring_conve")
        d = int(g["args"][2])
        net = {k[len("net_"):]: T(g[k]) for k in g.files if k.startswith("net_")}
    n_triple = 3 * n_shard * shard_bs - 17  # a padded last batch
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    sharding = Sharding.create(n_entity, n_shard, seed=seed)
    ew, rw = widths(scorer, d)
    ent = torch.randn(n_shard, sharding.max_entity_per_shard, ew) * 0.3
    rel = torch.randn(n_rel, rw) * 0.3
    if dtype == torch.float16:
        ent, rel = ent.half().float(), rel.half().float()
    triples = np.stack([rng.integers(n_entity, size=n_triple), rng.integers(n_rel, size=n_triple),
                        rng.integers(n_entity, size=n_triple)], axis=1)
    extra = np.stack([rng.integers(n_entity, size=4000), rng.integers(n_rel, size=4000),
                      rng.integers(n_entity, size=4000)], axis=1)
    extra[:1500, :2] = triples[rng.integers(n_triple, size=1500), :2]  # share (h, r) with test queries
    extra[1500:3000, 1:] = triples[rng.integers(n_triple, size=1500), 1:]  # share (r, t)
    extra[3000:3200] = triples[:200]  # the test triples themselves (filtered and true completion at once)
    extra[3200:3400] = extra[:200]    # duplicates in the filter set
    ds = KGDataset(n_entity=n_entity, n_relation_type=n_rel, triples={"test": triples},
                   original_triple_ids={"test": np.arange(n_triple)})
    pts = PartitionedTripleSet.create_from_dataset(ds, "test", sharding,
                                                   partition_mode="h_shard" if scheme == "t" else "t_shard")
    p = 0 if scorer == "ConvE" else 1
    fn = make_scorer(scorer, p, True, n_rel, d, ent, rel, dev, dtype=dtype, sharding=sharding, net=net)
    fn.eval()
    bs = RigidShardedBatchSampler(pts, PlaceholderNegativeSampler(scheme), shard_bs=shard_bs, batches_per_step=2,
                                  seed=seed, return_triple_idx=True)
    ev = Evaluation(["mrr", "hits@10"], mode=mode, reduction="sum", return_ranks=True)
    cand_ents = np.sort(rng.choice(n_entity, size=int(0.8 * n_entity), replace=False)) if filtered else None
    kw = dict(evaluation=ev, filter_triples=[extra] if filtered else None, candidate_ents=cand_ents, window_size=1000,
              device=dev)
    fused = AllScoresPipeline(bs, scheme, fn, **kw)
    assert fused.fused_ranks
    seen = []
    inner = fused._ranks_by_counting
    fused._ranks_by_counting = lambda *a, **k: (seen.append(inner(*a, **k)), seen[-1])[1]
    plain = AllScoresPipeline(bs, scheme, fn, fused_ranks=False, **kw)
    assert not plain.fused_ranks
    a, b = fused(), plain()
    assert seen and all(r is not None for r in seen), "a batch left the counted path"
    assert torch.equal(a["triple_idx"], b["triple_idx"]) and len(a["ranks"]) == n_triple
    same = torch.equal(a["ranks"], b["ranks"])
    # and the unsharded oracle
    order = pts.triple_sort_idx[a["triple_idx"].numpy()]
    tr = triples[order]
    flat = ent[sharding.entity_to_shard, sharding.entity_to_idx]
    known, truth = (tr[:, 0], tr[:, 2]) if scheme == "t" else (tr[:, 2], tr[:, 0])
    half = dtype == torch.float16
    with (kge.half_queries() if half else contextlib.nullcontext()):
        full = kge.score_candidates(scorer, p, True, scheme, flat[known], rel, T(tr[:, 1]), flat[None], net=net,
                                    training=False)
    if half:
        full = full.half().float()
    rows = torch.arange(len(tr))
    if filtered:
        full[:, T(np.setdiff1d(np.arange(n_entity), cand_ents))] = -torch.inf
    true_sc = torch.nan_to_num(full[rows, T(truth)].clone(), neginf=torch.finfo(torch.float32).min)
    if filtered:
        col, other = (0, 2) if scheme == "t" else (2, 0)
        for i, (e_, r_) in enumerate(zip(tr[:, col], tr[:, 1])):
            full[i, T(extra[(extra[:, col] == e_) & (extra[:, 1] == r_)][:, other])] = -torch.inf
    full[rows, T(truth)] = -torch.inf
    gt, ge = (full > true_sc[:, None]).sum(-1).float(), (full >= true_sc[:, None]).sum(-1).float()
    want = 1 + dict(optimistic=gt, pessimistic=ge, average=0.5 * (gt + ge))[mode]
    share_counted = float((a["ranks"] != want).float().mean())
    share_matrix = float((b["ranks"] != want).float().mean())
    print(f"{scorer} {scheme} filtered={filtered} {mode}: share of ranks off the oracle - matrix path "
          f"{share_matrix:.5f}, counted path {share_counted:.5f}; counted == matrix: {same}")
    assert same
    assert share_counted < (0.05 if half else 0.03)
