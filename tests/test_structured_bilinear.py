"""`scoring.StructuredBilinear` and its presets against explicit float64 formulas on the UNSHARDED tables, with the
sizes, batch layouts and tolerance of tests/test_rescal.py (rtol 1e-4, atol 1e-5: the project's fp32 figures)."""

import numpy as np
import pytest
import torch

from besskge import bess, scoring
from besskge.batch_sampler import RigidShardedBatchSampler
from besskge.dataset import KGDataset
from besskge.k_vs_all import KvsAllBessKGE
from besskge.loss import AllEntitiesBCELoss, LogSigmoidLoss, SampledSoftmaxCrossEntropyLoss
from besskge.metric import Evaluation
from besskge.negative_sampler import PlaceholderNegativeSampler, RandomShardedNegativeSampler
from besskge.one_vs_all import OneVsAllBessKGE
from besskge.pipeline import AllScoresPipeline
from besskge.sharding import PartitionedTripleSet, Sharding
from oracle import kge

from test_k_vs_all import N_REL, BatchTriples
from test_one_vs_all import dev  # noqa: F401
from test_rescal import check_step
from test_tucker import N_ENT, TOL, K, replica_rows

D = 6
pytestmark = pytest.mark.gpu


def hamilton(a, b):
    """a (x) b on [S, 4, d] quaternion rows."""
    a0, a1, a2, a3 = a.unbind(1)
    b0, b1, b2, b3 = b.unbind(1)
    return torch.stack([a0 * b0 - a1 * b1 - a2 * b2 - a3 * b3, a0 * b1 + a1 * b0 + a2 * b3 - a3 * b2,
                        a0 * b2 - a1 * b3 + a2 * b0 + a3 * b1, a0 * b3 + a1 * b2 - a2 * b1 + a3 * b0], 1)


def quate64(x, rid, R, side):
    """<h (x) r^, t> = <h, t (x) conj r^>: the query for candidate tails is h (x) r^, for heads t (x) conj r^."""
    r = R[rid].view(-1, 4, D)
    r = r / r.pow(2).sum(1, keepdim=True).sqrt()
    if side == "h":
        r = r * torch.tensor([1.0, -1.0, -1.0, -1.0], dtype=r.dtype).view(1, 4, 1)
    return hamilton(x.view(-1, 4, D), r).flatten(1)


def make_quate(dev, n):
    torch.manual_seed(n)
    fn = scoring.QuatE(True, Sharding.create(N_ENT, n, seed=0), N_REL, D, device=dev).to(dev)
    return fn, lambda: [fn.entity_embedding, fn.relation_embedding]


def rows(gen, *shape):
    return 0.5 * torch.randn(*shape, generator=gen)


def tri(a, b, c):  # [S, N] of sum_x a b c, the candidates [N, d] in the place of a or c
    return torch.einsum("sd,nd->sn", a * b, c) if a.shape[0] == b.shape[0] else torch.einsum("nd,sd->sn", a, b * c)


PRESETS = {  # K and the score of block views h, r, t [*, K, D]; SimplE: [head role | tail role], [r | r_inv]
    "DistMult": (1, lambda h, r, t: tri(h[:, 0], r[:, 0], t[:, 0])),
    "ComplEx": (2, lambda h, r, t: tri(h[:, 0], r[:, 0], t[:, 0]) + tri(h[:, 1], r[:, 0], t[:, 1])
                + tri(h[:, 0], r[:, 1], t[:, 1]) - tri(h[:, 1], r[:, 1], t[:, 0])),
    "SimplE": (2, lambda h, r, t: 0.5 * (tri(h[:, 0], r[:, 0], t[:, 1]) + tri(h[:, 1], r[:, 1], t[:, 0]))),
    "QuatE": (4, None)}


@pytest.mark.parametrize("preset", list(PRESETS))
def test_presets_against_float64(dev, preset):
    """The DistMult / ComplEx tables and scoring.DistMult / ComplEx on the same tables, both against float64; QuatE
    against the explicit Hamilton product, SimplE against the average of its two CP scores."""
    sharding, gen, (K_, formula) = Sharding.create(40, 1, seed=0), torch.Generator().manual_seed(5), PRESETS[preset]
    R = rows(gen, N_REL, K_ * D) + 0.3
    args = dict(entity_initializer=rows(gen, 40, K_ * D), relation_initializer=R.clone(), device=dev)
    fns = [getattr(scoring, preset)(True, sharding, N_REL, D, **args).to(dev)]
    if preset in ("DistMult", "ComplEx"):
        terms = scoring.DISTMULT_TERMS if preset == "DistMult" else scoring.COMPLEX_TERMS
        fns.append(scoring.StructuredBilinear(True, sharding, N_REL, D, terms, K_, K_, **args).to(dev))
    h, t, cand = rows(gen, 12, K_ * D), rows(gen, 12, K_ * D), rows(gen, 1, 30, K_ * D)
    rid = torch.randint(N_REL, (12,), generator=gen, dtype=torch.int32)
    h64, t64, c64, R64 = h.double(), t.double(), cand[0].double(), R.double()
    if formula is None:
        qt, qh = quate64(h64, rid.long(), R64, "t"), quate64(t64, rid.long(), R64, "h")
        want = [(qt * t64).sum(-1), qt @ c64.T, qh @ c64.T]
    else:
        blk = lambda v: v.view(-1, K_, D)  # noqa: E731
        r = blk(R64[rid.long()])
        want = [formula(blk(h64), r, blk(t64)).diagonal(), formula(blk(h64), r, blk(c64)), formula(blk(c64), r, blk(t64))]
    hd, rd, td, cd = (v.to(dev) for v in (h, rid, t, cand))
    for fn in fns:
        with torch.no_grad():
            got = [fn.score_triple(hd, rd, td), fn.score_tails(hd, rd, cd), fn.score_heads(cd, rd, td)]
        for g, w in zip(got, want):
            torch.testing.assert_close(g.double().cpu(), w, **TOL)


@pytest.mark.parametrize("n, shared", [(1, False), (2, True)])
def test_embedding_moving_sgd_step(dev, n, shared):
    """Per-triple negatives on one shard; shared ("flat") negatives on two shards in lock-step."""
    fn, tables = make_quate(dev, n)
    fn.negative_sample_sharing = shared
    ns = RandomShardedNegativeSampler(K, fn.sharding, 0, "t", local_sampling=False, flat_negative_format=shared)
    rng = np.random.default_rng(n)
    m = int(fn.sharding.shard_counts.min())
    batch = {k: torch.from_numpy(rng.integers(N_REL if k == "relation" else m, size=s).astype(np.int32))
             for k, s in (("head", (n, n, 12)), ("relation", (n, n, 12)), ("tail", (n, n, 12)),
                          ("negative", (n, n, 1 if shared else 12, K)))}
    model = bess.EmbeddingMovingBessKGE(ns, fn, LogSigmoidLoss(1.0, True, 0.5))
    neg = batch["negative"].long()

    def replica_loss(r, E, R):
        h, t, rid = replica_rows(E, batch, r, n)
        q = quate64(h, rid, R, "t")
        if shared:
            sc = q @ torch.cat([E[j][neg[j, r, 0]] for j in range(n)]).T
        else:
            sc = torch.einsum("sw,skw->sk", q, E[0][neg[0, 0]])
        return kge.loss_value("logsigmoid", (q * t).sum(-1), sc, torch.ones(1, dtype=torch.float64),
                              margin=1.0, adversarial=True, adversarial_scale=0.5)
    check_step(model, batch, n, dev, tables, replica_loss, dict(rtol=1e-5, atol=1e-5))


@pytest.mark.parametrize("training, scheme", [("1vsall", "t"), ("1vsall", "h"), ("kvsall", "t"), ("kvsall", "h")])
def test_all_entity_sgd_step(dev, training, scheme):
    n = 2
    bt = BatchTriples(N_ENT, n)
    fn, tables = make_quate(dev, n)
    sharding, batch, known = bt.sharding, bt.batch, bt.hrt[1:]
    if training == "kvsall":
        loss_fn = AllEntitiesBCELoss(N_ENT, label_smoothing=0.1, loss_scale=1.5 / N_ENT)
        model = KvsAllBessKGE(PlaceholderNegativeSampler(scheme), fn, loss_fn, [known])
    else:
        loss_fn = SampledSoftmaxCrossEntropyLoss(N_ENT, loss_scale=1.5)
        model = OneVsAllBessKGE(PlaceholderNegativeSampler(scheme), fn, loss_fn)
    counts = [int(c) for c in sharding.shard_counts]
    col_of = np.concatenate([[0], np.cumsum(counts)])[sharding.entity_to_shard] + sharding.entity_to_idx
    kept, found = (0, 2) if scheme == "t" else (2, 0)  # columns of (h, r, t): the query's entity, the label
    labels = {}
    for row in known:
        labels.setdefault((int(row[kept]), int(row[1])), []).append(int(row[found]))

    def replica_loss(r, E, R):
        h, t, rid = replica_rows(E, batch, r, n)
        w = batch["triple_weight"][r].double() * batch["triple_mask"][r].reshape(-1).double()
        q = quate64(h if scheme == "t" else t, rid, R, scheme)
        sc = q @ torch.cat([E[s, : counts[s]] for s in range(n)]).T
        if training == "1vsall":
            return float(loss_fn.loss_scale) * (w * (torch.logsumexp(sc, dim=1) - (q * (t if scheme == "t" else h)).sum(-1))).sum()
        y = torch.zeros_like(sc)
        for i, row in enumerate(bt.per_replica[r]):
            y[i, col_of[labels.get((int(row[kept]), int(row[1])), []) + [int(row[found])]]] = 1.0
        bce = torch.nn.functional.binary_cross_entropy_with_logits(
            sc, loss_fn.positive_weight * y + loss_fn.smooth, reduction="none").sum(dim=1)
        return float(loss_fn.loss_scale) * (w * bce).sum()
    check_step(model, batch, n, dev, tables, replica_loss, dict(rtol=1e-5, atol=1e-4))


def test_all_scores_pipeline_ranks(dev):
    """Counted ranks (DistMult's road) = the ranks from the score matrix."""
    fn, _ = make_quate(dev, 2)
    fn.eval()
    rng = np.random.default_rng(0)
    test = np.unique(np.stack([rng.integers(N_ENT, size=150), rng.integers(N_REL, size=150),
                               rng.integers(N_ENT, size=150)], axis=1), axis=0)
    ds = KGDataset(n_entity=N_ENT, n_relation_type=N_REL, triples={"test": test},
                   original_triple_ids={"test": np.arange(len(test))})
    pts = PartitionedTripleSet.create_from_dataset(ds, "test", fn.sharding, partition_mode="h_shard")
    ranks = []
    for fused in (True, False):
        bs = RigidShardedBatchSampler(pts, PlaceholderNegativeSampler("t"), shard_bs=64, batches_per_step=2, seed=0,
                                      return_triple_idx=True)
        ev = Evaluation(["mrr"], mode="average", reduction="none", return_ranks=True)
        res = AllScoresPipeline(bs, "t", fn, evaluation=ev, device=dev, fused_ranks=fused)()
        ranks.append(res["ranks"].long().cpu()[torch.argsort(res["triple_idx"])])
    assert torch.equal(*ranks)
