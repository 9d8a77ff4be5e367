"""The `TuckER` scorer against float64 `einsum` + autograd on the UNSHARDED tables: its public scores, one plain-SGD
step of EmbeddingMoving and ScoreMoving (sampled negatives), KvsAll (label smoothing 0.1) and 1vsAll, the ranks of
`AllScoresPipeline` and a checkpoint round trip.  Steps are compared on the tables after the step at the project's
fp32-path tolerance (rtol 1e-4, atol 1e-5); batch layout, filter and label matrix are tests/test_k_vs_all.py's."""

import numpy as np
import pytest
import torch

from besskge import bess, checkpoint, runtime
from besskge.batch_sampler import RigidShardedBatchSampler
from besskge.dataset import KGDataset
from besskge.k_vs_all import KvsAllBessKGE
from besskge.loss import AllEntitiesBCELoss, LogSigmoidLoss, SampledSoftmaxCrossEntropyLoss
from besskge.metric import Evaluation
from besskge.negative_sampler import PlaceholderNegativeSampler, RandomShardedNegativeSampler
from besskge.one_vs_all import OneVsAllBessKGE
from besskge.pipeline import AllScoresPipeline
from besskge.scoring import TuckER
from besskge.sharding import PartitionedTripleSet, Sharding
from oracle import kge

from test_k_vs_all import N_REL, BatchTriples
from test_one_vs_all import LR, dev  # noqa: F401

N_ENT, DE, DR, K = 300, 36, 7, 24
TOL = dict(rtol=1e-4, atol=1e-5)


def query64(x, r, core, side):
    w = core.view(DR, DE, DE)
    return torch.einsum("ik,ib,kab->ia" if side == "h" else "ik,ia,kab->ib", r, x, w)


def make_fn(dev, n, **kw):
    torch.manual_seed(n)
    return TuckER(True, Sharding.create(N_ENT, n, seed=0), N_REL, DE, DR, device=dev, **kw).to(dev)


def params(fn):
    return [p.detach().double().cpu().clone() for p in (fn.entity_embedding, fn.relation_embedding, fn.core)]


def replica_rows(E, batch, r, n):
    """(head rows, tail rows, relation ids) of replica r's triples (tests/test_one_vs_all.py's layout)"""
    h = E[r][batch["head"][r].long().reshape(-1)]
    t = torch.stack([E[j][batch["tail"][j][r].long()] for j in range(n)]).reshape(h.shape)
    return h, t, batch["relation"][r].long().reshape(-1)


def check_step(model, batch, n, dev, replica_loss, loss_tol):
    """One SGD step of `model` on `batch` against sum_r replica_loss(r, E, R, C) in float64."""
    fn = model.score_fn
    before = params(fn)
    E, R, C = (p.clone().requires_grad_() for p in before)
    want = [replica_loss(r, E, R, C) for r in range(n)]
    grads = torch.autograd.grad(sum(want), [E, R, C])
    runner = runtime.training_model(model, runtime.Options(device_iterations=1), runtime.SGD(lr=LR), device=dev)
    out = runner(**batch)
    torch.testing.assert_close(out["loss"].double().cpu().reshape(-1), torch.stack(want).detach(), **loss_tol)
    for name, p0, g, p1 in zip(("entities", "relations", "core"), before, grads, params(fn)):
        print(f"{name}: largest update {float((LR * g).abs().max()):.3e}, "
              f"largest deviation {float((p1 - (p0 - LR * g)).abs().max()):.3e}")
        torch.testing.assert_close(p1, p0 - LR * g, **TOL)


@pytest.mark.gpu
@pytest.mark.parametrize("bn", [False, True])
def test_scores_against_float64(dev, bn):
    fn = make_fn(dev, 1, batch_normalization=bn).eval()
    gen = torch.Generator().manual_seed(3)
    norms = [fn.input_layers[0], fn.hidden_layers[0]] if bn else [None, None]
    for m in norms if bn else []:  # non-trivial running statistics and affine parameters
        for t, lo in ((m.running_mean, -0.5), (m.running_var, 0.5), (m.weight.data, 0.5), (m.bias.data, -0.5)):
            t.copy_(torch.rand(DE, generator=gen) + lo)

    def bn64(x, m):
        if m is None:
            return x
        return (x - m.running_mean.double().cpu()) / (m.running_var.double().cpu() + m.eps).sqrt() \
            * m.weight.detach().double().cpu() + m.bias.detach().double().cpu()

    h, t = (0.25 * torch.randn(20, DE, generator=gen) for _ in range(2))
    cand = 0.25 * torch.randn(1, 50, DE, generator=gen)
    rid = torch.randint(N_REL, (20,), generator=gen, dtype=torch.int32)
    _, R, C = params(fn)
    q = {s: bn64(query64(bn64(x.double(), norms[0]), R[rid.long()], C, s), norms[1]) for s, x in (("t", h), ("h", t))}
    with torch.no_grad():
        got = [f(h.to(dev), rid.to(dev), t.to(dev)) for f in (fn.score_triple,)] + [
            fn.score_tails(h.to(dev), rid.to(dev), cand.to(dev)), fn.score_heads(cand.to(dev), rid.to(dev), t.to(dev))]
    want = [(q["t"] * t.double()).sum(-1), q["t"] @ cand[0].double().T, q["h"] @ cand[0].double().T]
    for g, w in zip(got, want):
        torch.testing.assert_close(g.double().cpu(), w, **TOL)


def sampled_model(dev, n, scheme_cls, **kw):
    fn = make_fn(dev, n, **kw)
    ns = RandomShardedNegativeSampler(K, fn.sharding, 0, "t", local_sampling=False, flat_negative_format=True)
    rng = np.random.default_rng(n)
    m = int(fn.sharding.shard_counts.min())
    batch = {k: torch.from_numpy(rng.integers(N_REL if k == "relation" else m, size=s).astype(np.int32))
             for k, s in (("head", (n, n, 16)), ("relation", (n, n, 16)), ("tail", (n, n, 16)),
                          ("negative", (n, n, 1, K)))}
    return getattr(bess, scheme_cls)(ns, fn, LogSigmoidLoss(1.0, True, 0.5)), batch


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("scheme_cls", ["EmbeddingMovingBessKGE", "ScoreMovingBessKGE"])
def test_sampled_negatives_sgd_step(dev, scheme_cls, n):
    """Shared ("flat") negatives: EmbeddingMoving scores replica r's queries against the rows every shard sampled FOR
    r, ScoreMoving against all the rows every shard sampled (oracle/kge.py's two layouts)."""
    model, batch = sampled_model(dev, n, scheme_cls)
    neg = batch["negative"].long()

    def replica_loss(r, E, R, C):
        h, t, rid = replica_rows(E, batch, r, n)
        cand = torch.cat([E[j][(neg[j, r, 0] if scheme_cls[0] == "E" else neg[j].reshape(-1))] for j in range(n)])
        q = query64(h, R[rid], C, "t")
        return kge.loss_value("logsigmoid", (q * t).sum(-1), q @ cand.T, torch.ones(1, dtype=torch.float64),
                              margin=1.0, adversarial=True, adversarial_scale=0.5)

    check_step(model, batch, n, dev, replica_loss, dict(rtol=1e-5, atol=1e-5))


@pytest.mark.gpu
def test_checkpoint_restores_core_batch_norm_and_optimiser_state(dev, tmp_path):
    """Two Adam steps, save, a third step and a shifted core, load: core, batch-norm and Adam state to the bit."""
    model, batch = sampled_model(dev, 2, "EmbeddingMovingBessKGE", batch_normalization=True)
    fn = model.score_fn
    runner = runtime.training_model(model, runtime.Options(device_iterations=1), runtime.Adam(lr=0.01), device=dev)

    def state():
        dense = {k: v.detach().clone() for k, v in fn.state_dict().items() if "embedding" not in k}
        st = model.update_state.get(fn.core)
        return dense, [s.clone() for s in st.s], st.true_step()

    runner(**batch)
    runner(**batch)
    dense, adam, step = state()
    assert "core" in dense and "input_layers.0.running_var" in dense and len(adam) == 2 and step == 2
    checkpoint.save_checkpoint(model, tmp_path / "ckpt")
    runner(**batch)
    with torch.no_grad():
        fn.core.add_(1.0)
    assert not torch.equal(state()[1][0], adam[0])
    checkpoint.load_checkpoint(model, tmp_path / "ckpt")
    dense1, adam1, step1 = state()
    assert step1 == step and all(torch.equal(a, b) for a, b in zip(adam1, adam))
    assert set(dense1) == set(dense) and all(torch.equal(dense1[k], dense[k]) for k in dense)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("training", ["kvsall", "1vsall"])
def test_all_entity_sgd_step(dev, training, n):
    """The loss over all entities in float64: a dense `BCEWithLogits` on the label matrix (label smoothing 0.1) /
    the cross entropy of the true tail.  Loss tolerance: those of tests/test_k_vs_all.py and test_one_vs_all.py at
    these sizes (sums of 64 terms of magnitude <= ~10: rtol 1e-5, atol 1e-4)."""
    bt = BatchTriples(N_ENT, n)
    fn = make_fn(dev, n)
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

    def replica_loss(r, E, R, C):
        h, t, rid = replica_rows(E, batch, r, n)
        w = batch["triple_weight"][r].double() * batch["triple_mask"][r].reshape(-1).double()
        q = query64(h, R[rid], C, "t")
        sc = q @ torch.cat([E[s, : counts[s]] for s in range(n)]).T
        if training == "1vsall":
            return float(loss_fn.loss_scale) * (w * (torch.logsumexp(sc, dim=1) - (q * t).sum(-1))).sum()
        y = torch.zeros_like(sc)
        for i, row in enumerate(bt.per_replica[r]):
            y[i, col_of[tails.get((int(row[0]), int(row[1])), []) + [int(row[2])]]] = 1.0
        bce = torch.nn.functional.binary_cross_entropy_with_logits(
            sc, loss_fn.positive_weight * y + loss_fn.smooth, reduction="none").sum(dim=1)
        return float(loss_fn.loss_scale) * (w * bce).sum()

    check_step(model, batch, n, dev, replica_loss, dict(rtol=1e-5, atol=1e-4))


@pytest.mark.gpu
def test_all_scores_pipeline_ranks(dev):
    """Counted ranks (DistMult's epilogue) of held-out (h, r, ?) queries = ranks from the float64 score matrix; the
    scores are continuous random numbers, so no two of a row agree to fp32 rounding."""
    fn = make_fn(dev, 2).eval()
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
    E, R, C = params(fn)
    ent = E[fn.sharding.entity_to_shard, fn.sharding.entity_to_idx]  # row = global id
    glob, first = np.copy(bs.triples), np.concatenate([[0], np.cumsum(bs.triple_counts)])
    for s in range(2):  # the sampler's heads are rows of their shard
        glob[first[s]:first[s + 1], 0] = fn.sharding.shard_and_idx_to_entity[s][glob[first[s]:first[s + 1], 0]]
    hrt = torch.from_numpy(glob[res["triple_idx"].numpy()]).long()
    sc = query64(ent[hrt[:, 0]], R[hrt[:, 1]], C, "t") @ ent.T
    want = 1 + (sc > sc.gather(1, hrt[:, 2:3])).sum(1)
    assert torch.equal(res["ranks"].long().cpu(), want)
