"""`scoring.HAKE` in the training step and in the all-entity evaluation.

One SGD step against a restatement of the step in float64 torch; the same restatement in float32 on the CPU gives the
tolerance: 4 x its largest deviation from float64, for the loss and for each updated table.  Ranks counted in the
kernel's epilogue against ranks from the score matrix: identical."""
import numpy as np
import pytest
import torch

from besskge import bess, runtime, scoring
from besskge.batch_sampler import RigidShardedBatchSampler
from besskge.dataset import KGDataset
from besskge.loss import LogSigmoidLoss
from besskge.metric import Evaluation
from besskge.negative_sampler import PlaceholderNegativeSampler, RandomShardedNegativeSampler
from besskge.pipeline import AllScoresPipeline
from besskge.sharding import PartitionedTripleSet, Sharding
from oracle import kge

pytestmark = pytest.mark.gpu

N_ENT, N_REL, D, S, K, LR = 300, 5, 16, 32, 24, 1.0  # (a step large enough that the gradient's error, not the
# rounding of the stored row, is what the table comparison sees)
LM, LP = 0.75, 0.375  # (float32-exact: the scorer keeps them in float32 buffers)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda", 0)


def make_hake(dev):
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(1)
    ent = torch.cat([(torch.rand(1, N_ENT, D, generator=gen) * 2 - 1) * 3.0, torch.randn(1, N_ENT, D, generator=gen)], -1)
    rel = torch.cat([(torch.rand(N_REL, D, generator=gen) * 2 - 1) * 3.0, torch.randn(N_REL, 2 * D, generator=gen)], -1)
    return scoring.HAKE(True, Sharding.create(N_ENT, 1, seed=0), N_REL, D, modulus_weight=LM, phase_weight=LP,
                        entity_initializer=ent, relation_initializer=rel, device=dev).to(dev)


def step(E, R, batch, shared):
    """(loss, updated E, updated R) of one SGD step in the dtype of E and R"""
    E, R = E.clone().requires_grad_(), R.clone().requires_grad_()
    h, t = E[0][batch["head"].long().reshape(-1)], E[0][batch["tail"].long().reshape(-1)]
    r = R[batch["relation"].long().reshape(-1)]
    neg = E[0][batch["negative"].long().reshape(-1, K)]  # [1 | S, K, 2 D]
    r_p, r_m, b = r.chunk(3, dim=-1)
    b = torch.maximum(b.clamp(max=1.0), -r_m.abs())

    def score(h_p, h_m, t_p, t_m):
        return -(LM * torch.norm(h_m * (r_m.abs() + b) - t_m * (1 - b), dim=-1)
                 + LP * torch.sin((h_p + r_p - t_p) / 2).abs().sum(-1))
    (h_p, h_m), (t_p, t_m), (n_p, n_m) = (x.chunk(2, dim=-1) for x in (h, t, neg))
    r_p, r_m, b = (x.unsqueeze(1) for x in (r_p, r_m, b))
    neg_score = score(h_p.unsqueeze(1), h_m.unsqueeze(1), n_p, n_m)
    r_p, r_m, b = (x.squeeze(1) for x in (r_p, r_m, b))
    loss = kge.loss_value("logsigmoid", score(h_p, h_m, t_p, t_m), neg_score, torch.ones(1, dtype=E.dtype),
                          margin=1.0, adversarial=True, adversarial_scale=0.5)
    gE, gR = torch.autograd.grad(loss, [E, R])
    return tuple(x.detach().double() for x in (loss, E - LR * gE, R - LR * gR))


@pytest.mark.parametrize("shared", [False, True], ids=["pertriple", "shared"])
def test_sgd_step(dev, shared):
    fn = make_hake(dev)
    fn.negative_sample_sharing = shared
    ns = RandomShardedNegativeSampler(K, fn.sharding, 0, "t", local_sampling=False, flat_negative_format=shared)
    rng = np.random.default_rng(3)
    batch = {k: torch.from_numpy(rng.integers(N_REL if k == "relation" else N_ENT, size=s).astype(np.int32))
             for k, s in (("head", (1, 1, S)), ("relation", (1, 1, S)), ("tail", (1, 1, S)),
                          ("negative", (1, 1, 1 if shared else S, K)))}
    loss_fn = LogSigmoidLoss(1.0, True, 0.5)
    model = (bess.ScoreMovingBessKGE if shared else bess.EmbeddingMovingBessKGE)(ns, fn, loss_fn)
    E, R = fn.entity_embedding.detach().cpu(), fn.relation_embedding.detach().cpu()
    want, low = step(E.double(), R.double(), batch, shared), step(E, R, batch, shared)
    runner = runtime.training_model(model, runtime.Options(device_iterations=1), runtime.SGD(lr=LR), device=dev)
    out = runner(**batch)
    got = (out["loss"].reshape(()), fn.entity_embedding, fn.relation_embedding)
    for name, g, w, l in zip(("loss", "entities", "relations"), got, want, low):
        err, tol = float((g.detach().double().cpu() - w).abs().max()), 4 * float((l - w).abs().max())
        print(f"{name}: error {err:.3e}, allowed {tol:.3e} (4 x the float32 deviation)")
        assert err <= tol, name


def test_all_scores_pipeline_ranks(dev):
    """counted ranks = the ranks from the score matrix"""
    fn = make_hake(dev)
    fn.eval()
    rng = np.random.default_rng(0)
    test = np.unique(np.stack([rng.integers(N_ENT, size=150), rng.integers(N_REL, size=150),
                               rng.integers(N_ENT, size=150)], axis=1), axis=0)
    ds = KGDataset(n_entity=N_ENT, n_relation_type=N_REL, triples={"test": test},
                   original_triple_ids={"test": np.arange(len(test))})
    pts = PartitionedTripleSet.create_from_dataset(ds, "test", fn.sharding, partition_mode="h_shard")
    ranks = []
    for fused in (True, False):
        bs = RigidShardedBatchSampler(pts, PlaceholderNegativeSampler("t"), shard_bs=S, batches_per_step=2, seed=0,
                                      return_triple_idx=True)
        ev = Evaluation(["mrr"], mode="average", reduction="none", return_ranks=True)
        pipe = AllScoresPipeline(bs, "t", fn, evaluation=ev, device=dev, fused_ranks=fused)
        assert pipe.fused_ranks == fused
        res = pipe()
        ranks.append(res["ranks"].long().cpu()[torch.argsort(res["triple_idx"])])
    assert torch.equal(*ranks)
