"""The `RESCAL` scorer and TuckER's `query_route="relation"` against float64 `einsum` + autograd on the UNSHARDED
tables, as tests/test_tucker.py does it (its sizes, batch layout, label matrix and tolerance: rtol 1e-4, atol 1e-5).

Bound of the ops-level route test.  M = R @ core is rounded once after a dr-term sum of unspecified order (<= dr u
sum |terms|, u = 2^-24), then enters the kernel's chain of de fused multiply-adds: q and d_x are within (de + dr) u of
the sum of absolute terms.  d_M is a chain over the <= S rows of a relation; the relation-table gradient d_M @ W^T adds
a de^2-term sum of unspecified order, the core's gradient R^T @ d_M an n_rel-term one: (de^2 + S) u and (n_rel + S) u."""

import numpy as np
import pytest
import torch

from besskge import bess, ops, runtime
from besskge.batch_sampler import RigidShardedBatchSampler
from besskge.dataset import KGDataset
from besskge.k_vs_all import KvsAllBessKGE
from besskge.loss import AllEntitiesBCELoss, LogSigmoidLoss, SampledSoftmaxCrossEntropyLoss
from besskge.metric import Evaluation
from besskge.negative_sampler import PlaceholderNegativeSampler, RandomShardedNegativeSampler
from besskge.one_vs_all import OneVsAllBessKGE
from besskge.pipeline import AllScoresPipeline
from besskge.scoring import RESCAL, TuckER
from besskge.sharding import PartitionedTripleSet, Sharding
from oracle import kge

from test_k_vs_all import N_REL, BatchTriples
from test_one_vs_all import LR, dev  # noqa: F401
from test_tucker import DE, DR, N_ENT, TOL, K, replica_rows
from test_tucker_kernels import U, product64


def rescal64(x, rid, R, side):
    return torch.einsum("ib,iab->ia" if side == "h" else "ia,iab->ib", x, R[rid].view(-1, DE, DE))


def tucker_bn64(x, rid, R, side, C):
    """TuckER's query with both batch-norms in training mode (weight 1, bias 0: their initial values)"""
    def bn(v):
        return (v - v.mean(0)) / (v.var(0, unbiased=False) + 1e-5).sqrt()
    return bn(torch.einsum("ik,ib,kab->ia" if side == "h" else "ik,ia,kab->ib", R[rid], bn(x), C.view(DR, DE, DE)))


def make_rescal(dev, n):
    torch.manual_seed(n)
    fn = RESCAL(True, Sharding.create(N_ENT, n, seed=0), N_REL, DE, device=dev).to(dev)
    return fn, rescal64, lambda: [fn.entity_embedding, fn.relation_embedding]


def make_tucker(dev, n):
    torch.manual_seed(n)
    fn = TuckER(True, Sharding.create(N_ENT, n, seed=0), N_REL, DE, DR, batch_normalization=True,
                query_route="relation", device=dev).to(dev)
    return fn, tucker_bn64, lambda: [fn.entity_embedding, fn.relation_embedding, fn.core]


def tables64(tables):
    return [p.detach().double().cpu().clone() for p in tables()]

def check_step(model, batch, n, dev, tables, replica_loss, loss_tol):
    """One SGD step of `model` on `batch` against sum_r replica_loss(r, E, R[, C]) in float64."""
    before = tables64(tables)
    P = [p.clone().requires_grad_() for p in before]
    want = [replica_loss(r, *P) for r in range(n)]
    grads = torch.autograd.grad(sum(want), P)
    runner = runtime.training_model(model, runtime.Options(device_iterations=1), runtime.SGD(lr=LR), device=dev)
    out = runner(**batch)
    torch.testing.assert_close(out["loss"].double().cpu().reshape(-1), torch.stack(want).detach(), **loss_tol)
    for p0, g, p1 in zip(before, grads, tables64(tables)):
        print(f"{tuple(p0.shape)}: largest update {float((LR * g).abs().max()):.3e}, "
              f"largest deviation {float((p1 - (p0 - LR * g)).abs().max()):.3e}")
        torch.testing.assert_close(p1, p0 - LR * g, **TOL)


@pytest.mark.gpu
def test_scores_against_float64(dev):
    fn = make_rescal(dev, 1)[0]
    gen = torch.Generator().manual_seed(3)
    h, t = (0.25 * torch.randn(20, DE, generator=gen) for _ in range(2))
    cand = 0.25 * torch.randn(1, 50, DE, generator=gen)
    rid = torch.randint(N_REL, (20,), generator=gen, dtype=torch.int32)
    R = fn.relation_embedding.detach().double().cpu()
    q = {s: rescal64(x.double(), rid.long(), R, s) for s, x in (("t", h), ("h", t))}
    hd, rd, td, cd = (v.to(dev) for v in (h, rid, t, cand))
    with torch.no_grad():
        got = [fn.score_triple(hd, rd, td), fn.score_tails(hd, rd, cd), fn.score_heads(cd, rd, td)]
    want = [(q["t"] * t.double()).sum(-1), q["t"] @ cand[0].double().T, q["h"] @ cand[0].double().T]
    for g, w in zip(got, want):
        torch.testing.assert_close(g.double().cpu(), w, **TOL)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("scheme_cls", ["EmbeddingMovingBessKGE", "ScoreMovingBessKGE"])
def test_sampled_negatives_sgd_step(dev, scheme_cls, n):
    """Shared ("flat") negatives, the two layouts of tests/test_tucker.py."""
    fn, query, tables = make_rescal(dev, n)
    ns = RandomShardedNegativeSampler(K, fn.sharding, 0, "t", local_sampling=False, flat_negative_format=True)
    rng = np.random.default_rng(n)
    m = int(fn.sharding.shard_counts.min())
    batch = {k: torch.from_numpy(rng.integers(N_REL if k == "relation" else m, size=s).astype(np.int32))
             for k, s in (("head", (n, n, 16)), ("relation", (n, n, 16)), ("tail", (n, n, 16)), ("negative", (n, n, 1, K)))}
    model = getattr(bess, scheme_cls)(ns, fn, LogSigmoidLoss(1.0, True, 0.5))
    neg = batch["negative"].long()
    def replica_loss(r, E, R):
        h, t, rid = replica_rows(E, batch, r, n)
        cand = torch.cat([E[j][(neg[j, r, 0] if scheme_cls[0] == "E" else neg[j].reshape(-1))] for j in range(n)])
        q = query(h, rid, R, "t")
        return kge.loss_value("logsigmoid", (q * t).sum(-1), q @ cand.T, torch.ones(1, dtype=torch.float64),
                              margin=1.0, adversarial=True, adversarial_scale=0.5)
    check_step(model, batch, n, dev, tables, replica_loss, dict(rtol=1e-5, atol=1e-5))


@pytest.mark.gpu
@pytest.mark.parametrize("make,training,n", [(make_rescal, "kvsall", 1), (make_rescal, "kvsall", 2),
                                             (make_rescal, "1vsall", 1), (make_rescal, "1vsall", 2),
                                             (make_tucker, "kvsall", 1)])
def test_all_entity_sgd_step(dev, make, training, n):
    """The loss over all entities in float64; the TuckER case is a batch-normalised model on the relation route."""
    bt = BatchTriples(N_ENT, n)
    fn, query, tables = make(dev, n)
    sharding, batch, known = bt.sharding, bt.batch, bt.hrt[1:]
    if training == "kvsall":
        loss_fn = AllEntitiesBCELoss(N_ENT, label_smoothing=0.1, loss_scale=1.5 / N_ENT)
        model = KvsAllBessKGE(PlaceholderNegativeSampler("t"), fn, loss_fn, [known])
    else:
        loss_fn = SampledSoftmaxCrossEntropyLoss(N_ENT, loss_scale=1.5)
        model = OneVsAllBessKGE(PlaceholderNegativeSampler("t"), fn, loss_fn)
    counts = [int(c) for c in sharding.shard_counts]
    col_of = np.concatenate([[0], np.cumsum(counts)])[sharding.entity_to_shard] + sharding.entity_to_idx
    tails = {}
    for hh, rr, tt in known:
        tails.setdefault((int(hh), int(rr)), []).append(int(tt))

    def replica_loss(r, E, R, *C):
        h, t, rid = replica_rows(E, batch, r, n)
        w = batch["triple_weight"][r].double() * batch["triple_mask"][r].reshape(-1).double()
        q = query(h, rid, R, "t", *C)
        sc = q @ torch.cat([E[s, : counts[s]] for s in range(n)]).T
        if training == "1vsall":
            return float(loss_fn.loss_scale) * (w * (torch.logsumexp(sc, dim=1) - (q * t).sum(-1))).sum()
        y = torch.zeros_like(sc)
        for i, row in enumerate(bt.per_replica[r]):
            y[i, col_of[tails.get((int(row[0]), int(row[1])), []) + [int(row[2])]]] = 1.0
        bce = torch.nn.functional.binary_cross_entropy_with_logits(
            sc, loss_fn.positive_weight * y + loss_fn.smooth, reduction="none").sum(dim=1)
        return float(loss_fn.loss_scale) * (w * bce).sum()
    check_step(model, batch, n, dev, tables, replica_loss, dict(rtol=1e-5, atol=1e-4))


@pytest.mark.gpu
def test_all_scores_pipeline_ranks(dev):
    """Counted ranks of held-out (h, r, ?) queries = ranks from the float64 score matrix (continuous random scores)."""
    fn, query, tables = make_rescal(dev, 2)
    fn.eval()
    rng = np.random.default_rng(0)
    test = np.unique(np.stack([rng.integers(N_ENT, size=200), rng.integers(N_REL, size=200),
                               rng.integers(N_ENT, size=200)], axis=1), axis=0)
    ds = KGDataset(n_entity=N_ENT, n_relation_type=N_REL, triples={"test": test},
                   original_triple_ids={"test": np.arange(len(test))})
    pts = PartitionedTripleSet.create_from_dataset(ds, "test", fn.sharding, partition_mode="h_shard")
    bs = RigidShardedBatchSampler(pts, PlaceholderNegativeSampler("t"), shard_bs=64, batches_per_step=2, seed=0,
                                  return_triple_idx=True)
    ev = Evaluation(["mrr"], mode="average", reduction="none", return_ranks=True)
    res = AllScoresPipeline(bs, "t", fn, evaluation=ev, device=dev)()
    E, R = tables64(tables)
    ent = E[fn.sharding.entity_to_shard, fn.sharding.entity_to_idx]  # row = global id
    glob, first = np.copy(bs.triples), np.concatenate([[0], np.cumsum(bs.triple_counts)])
    for s in range(2):  # the sampler's heads are rows of their shard
        glob[first[s]:first[s + 1], 0] = fn.sharding.shard_and_idx_to_entity[s][glob[first[s]:first[s + 1], 0]]
    hrt = torch.from_numpy(glob[res["triple_idx"].numpy()]).long()
    sc = query(ent[hrt[:, 0]], hrt[:, 1], R, "t") @ ent.T
    assert torch.equal(res["ranks"].long().cpu(), 1 + (sc > sc.gather(1, hrt[:, 2:3])).sum(1))


@pytest.mark.gpu
@pytest.mark.parametrize("swap", [0, 1])
@pytest.mark.parametrize("S,de,dr", [(70, 36, 7), (130, 200, 30)])
def test_tucker_relation_route_products(dev, S, de, dr, swap):
    """`R @ core` + `ops.RelationQuery` + autograd against the float64 einsum of tests/test_tucker_kernels.py."""
    n_rel = 5
    gen = torch.Generator().manual_seed(S + de + dr + swap)
    x, R, core, dq = (torch.randn(s, generator=gen) for s in ((S, de), (n_rel, dr), (dr * de, de), (S, de)))
    rid = torch.randint(n_rel, (S,), generator=gen)

    def reference(x, R, core, dq):
        q, d_x, d_rows, d_core = product64(x, R[rid], core, dq, swap)
        return q, d_x, torch.zeros(n_rel, dr, dtype=torch.float64).index_add_(0, rid, d_rows), d_core
    want, terms = reference(x, R, core, dq), reference(x.abs(), R.abs(), core.abs(), dq.abs())
    gx, gR, gcore = (t.to(dev).requires_grad_() for t in (x, R, core))
    q = ops.RelationQuery.apply(gx, gR @ gcore.view(dr, de * de), rid.to(dev), bool(swap))
    got = [q.detach(), *torch.autograd.grad(q, [gx, gR, gcore], dq.to(dev))]
    for name, g, w, t, n in zip(("q", "d_x", "d_rel", "d_core"), got, want, terms,
                                (de + dr, de + dr, de * de + S, n_rel + S)):
        err = (g.double().cpu() - w).abs()
        print(f"{name} ({S}, {de}, {dr}) swap {swap}: largest error / bound {float((err / (n * U * t)).max()):.3e}")
        assert bool((err <= n * U * t).all()), name


def test_constructor_errors():
    sharding = Sharding.create(50, 2, seed=0)
    with pytest.raises(ValueError, match="query_route"):
        TuckER(True, sharding, 4, 12, 5, query_route="grouped")
    with pytest.raises(ValueError, match="embedding_size"):
        RESCAL(True, sharding, 4, 0)
    fn = RESCAL(True, sharding, 4, 6, inverse_relations=True)
    assert tuple(fn.relation_embedding.shape) == (8, 36) and fn.kernel_desc().rel_width == 6
