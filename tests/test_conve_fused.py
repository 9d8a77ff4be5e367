"""`scoring.ConvE(query_route="fused")` against a float64 replica of the same model: a deep copy on the CPU in double
precision on the torch route, whose network is called once for the candidates' query and once for the positives, as
the steps do - over the same row sets and in the same order, so batch statistics and the running statistics they move
agree: EmbeddingMoving runs it on a replica's own rows twice, ScoreMoving once per shard on the gathered rows of all
replicas (the candidates' queries) and once per replica on its own rows (the positives).  One SGD step each; tables,
every dense parameter and the batch-norm buffers at the step tolerance of tests/test_rescal.py (rtol 1e-4, atol 1e-5).

A ReLU decision that differed from the reference's would exceed that tolerance: `relu_margin` asserts, on the float64
replica alone, that every |z| is above 64 (Cin kh kw + 2) 2^-24 times the sum of its absolute terms; the seeds of
`make_fn` satisfy it."""

import copy

import numpy as np
import pytest
import torch

from besskge import bess, runtime
from besskge.batch_sampler import RigidShardedBatchSampler
from besskge.dataset import KGDataset
from besskge.k_vs_all import KvsAllBessKGE
from besskge.loss import AllEntitiesBCELoss, LogSigmoidLoss, SampledSoftmaxCrossEntropyLoss
from besskge.metric import Evaluation
from besskge.negative_sampler import PlaceholderNegativeSampler, RandomShardedNegativeSampler
from besskge.one_vs_all import OneVsAllBessKGE
from besskge.pipeline import AllScoresPipeline
from besskge.scoring import ConvE
from besskge.sharding import PartitionedTripleSet, Sharding
from oracle import kge

from test_k_vs_all import N_REL, BatchTriples
from test_one_vs_all import LR, dev  # noqa: F401
from test_tucker import N_ENT, TOL, K, replica_rows

D, U = 36, 2.0 ** -24


def make_fn(dev, seed=1, route="fused", n=1, **kw):
    torch.manual_seed(seed)
    kw = dict(dict(input_dropout=0.0, feature_map_dropout=0.0, hidden_dropout=0.0), **kw)
    fn = ConvE(True, Sharding.create(N_ENT, n, seed=0), N_REL, D, 6, 6, inverse_relations=False, output_channels=4,
               query_route=route, **kw)  # drawn on the CPU: the seed means the same model on every device
    with torch.no_grad():  # batch-norm weights and the tail bias away from their trivial initial values
        for p in fn.dense_parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
        fn.entity_embedding[..., -1] = 0.1 * torch.randn_like(fn.entity_embedding[..., -1])
    return fn.to(dev)


def replica64(fn):
    fn64 = copy.deepcopy(fn).cpu().double()
    fn64.query_route = "torch"
    return fn64


def relu_margin(fn64, h, r):
    """every pre-ReLU z of the network on (h, r) is clear of zero by 64 (KK + 2) u sum |terms| (on a copy: no state moves)"""
    net = copy.deepcopy(fn64)
    layers = list(net.conv_layers)
    at = next(i for i, m in enumerate(layers) if isinstance(m, torch.nn.Conv2d))
    x = torch.cat([h[:, :-1].reshape(-1, 1, 6, 6), r.reshape(-1, 1, 6, 6)], dim=-2)
    for m in layers[:at]:
        x = m(x)
    conv, nxt = layers[at], layers[at + 1]
    c = torch.nn.functional.conv2d(x, conv.weight)
    terms = torch.nn.functional.conv2d(x.abs(), conv.weight.abs()) + conv.bias.abs().view(1, -1, 1, 1)
    z = c + conv.bias.view(1, -1, 1, 1)
    if isinstance(nxt, torch.nn.BatchNorm2d):
        mean, var = z.mean(dim=(0, 2, 3)), z.var(dim=(0, 2, 3), unbiased=False)
        a = (nxt.weight / torch.sqrt(var + nxt.eps)).view(1, -1, 1, 1)
        z = (z - mean.view(1, -1, 1, 1)) * a + nxt.bias.view(1, -1, 1, 1)
        terms = (terms + mean.abs().view(1, -1, 1, 1)) * a.abs() + nxt.bias.abs().view(1, -1, 1, 1)
    kk = conv.weight[0].numel()
    assert bool((z.abs() > 64 * (kk + 2) * U * terms).all()), "a ReLU decision is within rounding of zero: pick another seed"


def check_step(fn, model, batch, dev, loss64):
    """One SGD step of `model` against the sum of the replicas' losses `loss64(fn64)` and its autograd in float64."""
    fn64 = replica64(fn)
    want = torch.stack(loss64(fn64))
    want.sum().backward()
    out = runtime.training_model(model, runtime.Options(device_iterations=1), runtime.SGD(lr=LR), device=dev)(**batch)
    torch.testing.assert_close(out["loss"].double().cpu().reshape(-1), want.detach(), rtol=1e-5, atol=1e-4)
    after = {k: v.detach().double().cpu() for k, v in fn.state_dict().items()}
    grads = {k: p.grad for k, p in fn64.named_parameters()}
    for name, v64 in fn64.state_dict().items():
        if name.endswith("num_batches_tracked"):
            assert int(after[name]) == int(v64), name
            continue
        expect = v64 - LR * grads[name] if grads.get(name) is not None else v64
        print(f"{name}: largest deviation {float((after[name] - expect).abs().max()):.3e}")
        torch.testing.assert_close(after[name], expect.detach(), **TOL)


def net64(fn64, h, rid, t=None):
    """the network on rows (h, relation ids), its ReLU margins asserted first; with tail rows t: the positive scores"""
    rel = fn64.relation_embedding[rid]
    relu_margin(fn64, h, rel)
    q = fn64._net(h, rel)
    return q if t is None else (q * t[:, :-1]).sum(-1) + t[:, -1]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("scheme_cls", ["EmbeddingMovingBessKGE", "ScoreMovingBessKGE"])
def test_sampled_negatives_sgd_step(dev, scheme_cls, n):  # train mode, batch-norm, shared negatives, 1 and 2 shards
    fn = make_fn(dev, n=n)
    ns = RandomShardedNegativeSampler(K, fn.sharding, 0, "t", local_sampling=False, flat_negative_format=True)
    rng, m = np.random.default_rng(1), int(fn.sharding.shard_counts.min())
    batch = {k: torch.from_numpy(rng.integers(N_REL if k == "relation" else m, size=s).astype(np.int32))
             for k, s in (("head", (n, n, 16)), ("relation", (n, n, 16)), ("tail", (n, n, 16)), ("negative", (n, n, 1, K)))}
    model = getattr(bess, scheme_cls)(ns, fn, LogSigmoidLoss(1.0, True, 0.5))

    def loss64(fn64):  # per replica, the network called as the scheme calls it
        E, neg = fn64.entity_embedding, batch["negative"].long()
        rows = [replica_rows(E, batch, r, n) for r in range(n)]
        score = lambda q, cand: q @ cand[:, :-1].T + cand[:, -1]  # noqa: E731
        if scheme_cls[0] == "S":  # every shard transforms the gathered heads of all replicas, then the positives
            h_all, rid_all = torch.cat([x[0] for x in rows]), torch.cat([x[2] for x in rows])
            q_shard = [net64(fn64, h_all, rid_all) for _ in range(n)]
        out = []
        for r, (h, t, rid) in enumerate(rows):
            pos, S = net64(fn64, h, rid, t), h.shape[0]
            if scheme_cls[0] == "E":  # the replica's own rows against the negatives every shard sent it
                sc = score(net64(fn64, h, rid), torch.cat([E[j][neg[j, r, 0]] for j in range(n)]))
            else:
                sc = torch.cat([score(q_shard[j][r * S:(r + 1) * S], E[j][neg[j].reshape(-1)]) for j in range(n)], dim=1)
            out.append(kge.loss_value("logsigmoid", pos, sc, torch.ones(1, dtype=torch.float64), margin=1.0,
                                      adversarial=True, adversarial_scale=0.5))
        return out
    check_step(fn, model, batch, dev, loss64)


@pytest.mark.gpu
@pytest.mark.parametrize("training,norm", [("1vsall", True), ("kvsall", True), ("1vsall", False)])
def test_all_entity_sgd_step(dev, training, norm):  # 1vsAll, KvsAll with eps 0.1, and a model without batch-norm
    bt = BatchTriples(N_ENT, 1)
    fn = make_fn(dev, batch_normalization=norm)
    batch, known = bt.batch, bt.hrt[1:]
    if training == "kvsall":
        loss_fn = AllEntitiesBCELoss(N_ENT, label_smoothing=0.1, loss_scale=1.5 / N_ENT)
        model = KvsAllBessKGE(PlaceholderNegativeSampler("t"), fn, loss_fn, [known])
    else:
        loss_fn = SampledSoftmaxCrossEntropyLoss(N_ENT, loss_scale=1.5)
        model = OneVsAllBessKGE(PlaceholderNegativeSampler("t"), fn, loss_fn)
    n_real = int(bt.sharding.shard_counts[0])
    tails = {}
    for hh, rr, tt in known:
        tails.setdefault((int(hh), int(rr)), []).append(int(tt))

    def loss64(fn64):
        E = fn64.entity_embedding
        h, t, rid = replica_rows(E, batch, 0, 1)
        w = batch["triple_weight"][0].double() * batch["triple_mask"][0].reshape(-1).double()
        q, pos = net64(fn64, h, rid), net64(fn64, h, rid, t)  # (the network runs twice, as in the step)
        sc = q @ E[0, :n_real, :-1].T + E[0, :n_real, -1]
        if training == "1vsall":
            return [float(loss_fn.loss_scale) * (w * (torch.logsumexp(sc, dim=1) - pos)).sum()]
        y = torch.zeros_like(sc)
        for i, row in enumerate(bt.per_replica[0]):
            y[i, bt.sharding.entity_to_idx[tails.get((int(row[0]), int(row[1])), []) + [int(row[2])]]] = 1.0
        bce = torch.nn.functional.binary_cross_entropy_with_logits(
            sc, loss_fn.positive_weight * y + loss_fn.smooth, reduction="none").sum(dim=1)
        return [float(loss_fn.loss_scale) * (w * bce).sum()]
    check_step(fn, model, batch, dev, loss64)


@pytest.mark.gpu
def test_all_scores_pipeline_ranks(dev):
    """Eval mode: counted ranks of held-out (h, r, ?) queries on the fused route = ranks from the float64 scores."""
    fn = make_fn(dev).eval()
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
    fn64 = replica64(fn)
    ent = fn64.entity_embedding[fn.sharding.entity_to_shard, fn.sharding.entity_to_idx].detach()  # row = global id
    glob = np.copy(bs.triples)
    glob[:, 0] = fn.sharding.shard_and_idx_to_entity[0][glob[:, 0]]
    hrt = torch.from_numpy(glob[res["triple_idx"].numpy()]).long()
    with torch.no_grad():
        sc = fn64._net(ent[hrt[:, 0]], fn64.relation_embedding[hrt[:, 1]]) @ ent[:, :-1].T + ent[:, -1]
    assert torch.equal(res["ranks"].long().cpu(), 1 + (sc > sc.gather(1, hrt[:, 2:3])).sum(1))


@pytest.mark.gpu
def test_routes_share_a_state_dict_and_dropout_steps(dev):
    """A state dict saved on the torch route scores identically (eval mode, the step tolerance) on the fused route;
    with feature-map dropout 0.5 a fused training step runs and moves the parameters."""
    src = make_fn(dev, route="torch").eval()
    fn = make_fn(dev, seed=7, feature_map_dropout=0.5)
    fn.load_state_dict(src.state_dict())
    gen = torch.Generator().manual_seed(0)
    h, t = (torch.randn(20, D + 1, generator=gen).to(dev) for _ in range(2))
    rid = torch.randint(N_REL, (20,), generator=gen, dtype=torch.int32).to(dev)
    with torch.no_grad():
        torch.testing.assert_close(fn.eval().score_triple(h, rid, t), src.score_triple(h, rid, t), **TOL)
    fn.train()
    bt = BatchTriples(N_ENT, 1)
    model = OneVsAllBessKGE(PlaceholderNegativeSampler("t"), fn, SampledSoftmaxCrossEntropyLoss(N_ENT))
    before = fn.fc_layers[0].weight.detach().clone()
    torch.manual_seed(3)
    out = runtime.training_model(model, runtime.Options(device_iterations=1), runtime.SGD(lr=LR), device=dev)(**bt.batch)
    assert bool(torch.isfinite(out["loss"]).all()) and not torch.equal(before, fn.fc_layers[0].weight.detach())
