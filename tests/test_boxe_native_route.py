"""`scoring.BoxE(query_route="native")` in a training step, in the public scoring methods and in evaluation.  The step's
reference is a float64 deep copy of the model on the CPU on the torch route (tests/test_conve_fused.py), at the
tolerances of the BoxE training cases of tests/test_hip_parity.py (loss 1e-4 / 1e-4, tables 1e-4 / 2e-5)."""

import copy

import numpy as np
import pytest
import torch

from besskge import _native as nat
from besskge import runtime
from besskge.batch_sampler import RigidShardedBatchSampler
from besskge.bess import EmbeddingMovingBessKGE
from besskge.dataset import KGDataset
from besskge.loss import LogSigmoidLoss
from besskge.metric import Evaluation
from besskge.negative_sampler import PlaceholderNegativeSampler, RandomShardedNegativeSampler
from besskge.pipeline import AllScoresPipeline
from besskge.scoring import BoxE
from besskge.sharding import PartitionedTripleSet, Sharding
from oracle import kge

from test_one_vs_all import LR, dev  # noqa: F401
from test_step_context import logged

pytestmark = pytest.mark.gpu
N_ENT, N_REL, D, B, K = 300, 5, 16, 32, 8


def make_fn(dev, route="native", sharing=False, p=2):
    torch.manual_seed(3)  # drawn on the CPU: the seed means the same model on every device
    return BoxE(sharing, p, Sharding.create(N_ENT, 1, seed=0), N_REL, D, query_route=route).to(dev)


def negatives64(fn64, side, kept, rid, cand):
    """scores [S, N] of candidates cand [S, N, 2 d] through the scorer's own query"""
    q = fn64._query_torch(side, kept, fn64.relation_embedding, rid).view(-1, 1, 2, 3, D)
    return fn64._box_distance(cand.view(*cand.shape[:2], 2, D) + q[..., 0, :], q[..., 1, :], q[..., 2, :])


@pytest.mark.parametrize("scheme", ["h", "ht"])
def test_sgd_step_equals_float64(dev, scheme):
    fn = make_fn(dev)
    ns = RandomShardedNegativeSampler(K, fn.sharding, 0, scheme, local_sampling=False, flat_negative_format=False)
    rng = np.random.default_rng(1)
    batch = {k: torch.from_numpy(rng.integers(N_REL if k == "relation" else N_ENT, size=s).astype(np.int32))
             for k, s in (("head", (1, 1, B)), ("relation", (1, 1, B)), ("tail", (1, 1, B)), ("negative", (1, 1, B, K)))}
    model = EmbeddingMovingBessKGE(ns, fn, LogSigmoidLoss(1.0, True, 0.5))
    fn64 = copy.deepcopy(fn).cpu().double()
    fn64.query_route = "torch"
    E, rid = fn64.entity_embedding[0], batch["relation"].reshape(-1)
    h, t, cand = E[batch["head"].reshape(-1).long()], E[batch["tail"].reshape(-1).long()], E[batch["negative"][0, 0].long()]
    cut = B // 2 if scheme == "ht" else B  # the first triples corrupt heads, the others tails
    sc = torch.cat([negatives64(fn64, nat.CORRUPT_HEAD, t[:cut], rid[:cut], cand[:cut]),
                    negatives64(fn64, nat.CORRUPT_TAIL, h[cut:], rid[cut:], cand[cut:])])
    want = kge.loss_value("logsigmoid", fn64._triple_torch(h, fn64.relation_embedding, rid, t), sc,
                          torch.ones(1, dtype=torch.float64), margin=1.0, adversarial=True, adversarial_scale=0.5)
    want.backward()
    (out, names) = logged(lambda: runtime.training_model(model, runtime.Options(device_iterations=1),
                                                         runtime.SGD(lr=LR), device=dev)(**batch))
    torch.testing.assert_close(out["loss"].double().cpu().reshape(()), want.detach(), rtol=1e-4, atol=1e-4)
    for name, p in fn64.named_parameters():
        got = dict(fn.named_parameters())[name].detach().double().cpu()
        torch.testing.assert_close(got, (p - LR * p.grad).detach(), rtol=1e-4, atol=2e-5)
    # the step's own calls: the new entry points, and no row gather in front of them
    assert "bess_boxe_query_fwd" in names and "bess_boxe_query_bwd" in names and "bess_gather_rows" not in names


@pytest.mark.parametrize("sharing", [True, False])
def test_public_scores_and_gradients_agree_between_the_routes(dev, sharing):
    fn = make_fn(dev, sharing=sharing, p=1)
    gen = torch.Generator().manual_seed(0)
    h, t = (torch.rand(20, 2 * D, generator=gen).to(dev) for _ in range(2))
    cand = torch.rand(1 if sharing else 20, 7, 2 * D, generator=gen).to(dev)
    rid = torch.randint(N_REL, (20,), generator=gen, dtype=torch.int32).to(dev)
    results = {}
    for route in ("torch", "native"):
        fn.query_route = route
        leaves = [x.clone().requires_grad_() for x in (h, t, cand)]
        fn.relation_embedding.grad = None
        scores = [fn.score_triple(leaves[0], rid, leaves[1]), fn.score_tails(leaves[0], rid, leaves[2]),
                  fn.score_heads(leaves[2], rid, leaves[1])]
        sum((s * torch.linspace(0.5, 1.5, s.numel(), device=dev).view(s.shape)).sum() for s in scores).backward()
        results[route] = [s.detach() for s in scores] + [x.grad for x in leaves] + [fn.relation_embedding.grad.clone()]
    for a, b in zip(results["native"], results["torch"]):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=2e-5)


def test_all_scores_pipeline_ranks_are_the_torch_route_s(dev):
    fn = make_fn(dev, sharing=True).eval()
    rng = np.random.default_rng(0)
    test = np.unique(np.stack([rng.integers(N_ENT, size=200), rng.integers(N_REL, size=200),
                               rng.integers(N_ENT, size=200)], axis=1), axis=0)
    ds = KGDataset(n_entity=N_ENT, n_relation_type=N_REL, triples={"test": test},
                   original_triple_ids={"test": np.arange(len(test))})
    pts = PartitionedTripleSet.create_from_dataset(ds, "test", fn.sharding, partition_mode="h_shard")
    ranks = {}
    for route in ("torch", "native"):
        fn.query_route = route
        bs = RigidShardedBatchSampler(pts, PlaceholderNegativeSampler("t"), shard_bs=64, batches_per_step=2, seed=0,
                                      return_triple_idx=True)
        ev = Evaluation(["mrr"], mode="average", reduction="none", return_ranks=True)
        ranks[route] = AllScoresPipeline(bs, "t", fn, evaluation=ev, device=dev)()["ranks"].cpu()
    assert torch.equal(ranks["native"], ranks["torch"])
