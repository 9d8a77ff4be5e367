"""`OneVsAllBessKGE`: training steps whose softmax runs over all 101 entities, against float64 autograd on the
UNSHARDED entity table (the loss of `tests/test_one_vs_all_host.py`, which that file anchors to the oracle).

Replica r's triple (j, q) has head E[r, head[r, j, q]], tail E[j, tail[j, r, q]] and relation R[relation[r, j, q]];
its candidates are the real rows of every shard (3 shards of 34 rows hold 101 entities: one pad row, which no step
may touch).

Tolerances.  Gradients are read off a plain-SGD step as (before - after) / lr: the kernels' own deviation is the
project's shared-negative tolerance (rtol 1e-4, atol 1e-5, fp32 paths only at these sizes), the differencing adds
two roundings of a table entry |x| <= 1 divided by lr = 0.5: 2 * 2^-24 / 0.5 < 3e-7, and a row that is both a
candidate and a head / tail sums its parts in one more fp32 addition - atol 2e-5 in all.  The loss is a sum of 8 n
terms of magnitude <= ~10, each within the log-sum-exp tolerance of tests/test_one_vs_all_kernels.py (< 1e-5 here):
rtol 1e-5, atol 1e-4."""

import numpy as np
import pytest
import torch

from test_regularizer import phi

N_ENTITY, N_REL, D, PPP = 101, 5, 16, 8
LR = 0.5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda", 0)


def make_model(dev, scorer, n, scheme, reg=None, loss_scale=1.0, seed=0):
    from besskge import scoring
    from besskge.loss import SampledSoftmaxCrossEntropyLoss
    from besskge.negative_sampler import PlaceholderNegativeSampler
    from besskge.one_vs_all import OneVsAllBessKGE
    from besskge.sharding import Sharding

    sharding = Sharding.create(N_ENTITY, n, seed=0)
    torch.manual_seed(seed)
    if scorer in ("TransE", "RotatE"):
        fn = getattr(scoring, scorer)(True, 1, sharding, N_REL, D, device=dev)
    else:
        fn = getattr(scoring, scorer)(True, sharding, N_REL, D, device=dev)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():  # uniform in [-1, 1]
        fn.entity_embedding.copy_(torch.rand(fn.entity_embedding.shape, generator=gen) * 2 - 1)
        fn.relation_embedding.copy_(torch.rand(fn.relation_embedding.shape, generator=gen) * 2 - 1)
    return OneVsAllBessKGE(PlaceholderNegativeSampler(scheme), fn,
                           SampledSoftmaxCrossEntropyLoss(N_ENTITY, loss_scale=loss_scale), regularizer=reg)


def make_batch(sharding, n, micro=1, seed=0, weight=False, mask=False):
    rng = np.random.default_rng(seed)
    rows = micro * n
    counts = np.tile(sharding.shard_counts, micro).reshape(rows, 1, 1)  # a replica's head / tail rows are its shard's
    b = dict(head=(rng.random((rows, n, PPP)) * counts).astype(np.int32),
             relation=rng.integers(N_REL, size=(rows, n, PPP)).astype(np.int32),
             tail=(rng.random((rows, n, PPP)) * counts).astype(np.int32))
    b = {k: torch.from_numpy(v) for k, v in b.items()}
    if weight:
        b["triple_weight"] = torch.from_numpy(rng.random(size=(rows, n * PPP)).astype(np.float32) + 0.5)
    if mask:
        m = np.ones((rows, n, PPP), dtype=bool)
        m[:, 0, 1] = False
        m[:, n - 1, 5] = False
        b["triple_mask"] = torch.from_numpy(m)
    return b


def scores_all(scorer, scheme, ent, rel, cand):
    """float64 scores [S, n_entity] of the queries (kept entity, relation) against every entity"""
    from oracle import kge

    name = {"TransE": kge.TRANSE, "RotatE": kge.ROTATE, "DistMult": kge.DISTMULT, "ComplEx": kge.COMPLEX}[scorer]
    q = kge.query(name, scheme, ent, rel)
    if scorer in ("TransE", "RotatE"):
        return -torch.cdist(q, cand, p=1.0)
    return q @ cand.T


def reference(model, sharding, batch, scorer, scheme, n, row0=0, grad_scale=1.0):
    """(loss per replica, penalty per replica, d / d E [n, M, W], d / d R) in float64 of the micro-batch in rows
    row0 .. row0 + n of `batch`, at the model's current tables."""
    from oracle import kge

    name = {"TransE": kge.TRANSE, "RotatE": kge.ROTATE, "DistMult": kge.DISTMULT, "ComplEx": kge.COMPLEX}[scorer]
    E = model.score_fn.entity_embedding.detach().double().cpu().requires_grad_(True)
    R = model.score_fn.relation_embedding.detach().double().cpu().requires_grad_(True)
    real = torch.cat([E[s, : int(sharding.shard_counts[s])] for s in range(n)])  # every real entity, pads left out
    assert real.shape[0] == N_ENTITY
    reg, scale = model.regularizer, float(model.loss_fn.loss_scale)
    flags = model._regularizer_flags if reg is not None else 0
    losses, pens = [], []
    for r in range(n):
        h = E[r][batch["head"][row0 + r].long().reshape(-1)]
        t = torch.stack([E[j][batch["tail"][row0 + j][r].long()] for j in range(n)]).reshape(h.shape)
        rid = batch["relation"][row0 + r].long().reshape(-1)
        w = batch["triple_weight"][row0 + r].double() if "triple_weight" in batch else torch.ones(1, dtype=torch.float64)
        if "triple_mask" in batch:
            w = w * batch["triple_mask"][row0 + r].reshape(-1).double()
        pos = kge.score_triple(name, 1, h, R, rid, t)
        sc = scores_all(scorer, scheme, h if scheme == "t" else t, R[rid], real)
        losses.append(scale * (w * (torch.logsumexp(sc, dim=1) - pos)).sum())
        if reg is not None:
            pens.append((scale * w * (reg.entity_coef * (phi(h, reg.p, flags & 1) + phi(t, reg.p, flags & 1))
                                      + reg.relation_coef * phi(R[rid], reg.p, flags & 2))).sum())
        else:
            pens.append(torch.zeros((), dtype=torch.float64))
    (grad_scale * (sum(losses) + sum(pens))).backward()
    return torch.stack(losses).detach(), torch.stack(pens).detach(), E.grad, R.grad


def tables(model):
    return (model.score_fn.entity_embedding.detach().double().cpu().clone(),
            model.score_fn.relation_embedding.detach().double().cpu().clone())


def check_sgd_step(model, sharding, batch, scorer, scheme, n, dev):
    from besskge import runtime

    want_loss, want_pen, dE, dR = reference(model, sharding, batch, scorer, scheme, n)
    E0, R0 = tables(model)
    runner = runtime.training_model(model, runtime.Options(device_iterations=1), runtime.SGD(lr=LR), device=dev)
    out = runner(**batch)
    E1, R1 = tables(model)
    torch.testing.assert_close(out["loss"].double().cpu().reshape(-1), want_loss + want_pen, rtol=1e-5, atol=1e-4)
    if model.regularizer is not None:
        torch.testing.assert_close(out["regularization"].double().cpu().reshape(-1), want_pen, rtol=1e-4, atol=1e-6)
    torch.testing.assert_close((E0 - E1) / LR, dE, rtol=1e-4, atol=2e-5)
    torch.testing.assert_close((R0 - R1) / LR, dR, rtol=1e-4, atol=2e-5)
    for s in range(n):  # pad rows are no entities: never touched
        assert torch.equal(E0[s, int(sharding.shard_counts[s]):], E1[s, int(sharding.shard_counts[s]):])
    assert int(sharding.shard_counts.sum()) == N_ENTITY


@pytest.mark.gpu
@pytest.mark.parametrize("reg", [False, True])
@pytest.mark.parametrize("scheme", ["t", "h"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("scorer", ["ComplEx", "DistMult", "TransE", "RotatE"])
def test_sgd_step_against_float64(dev, scorer, n, scheme, reg):
    from besskge.regularizer import EmbeddingRegularizer

    model = make_model(dev, scorer, n, scheme, EmbeddingRegularizer.n3(1e-2) if reg else None, loss_scale=1.5)
    batch = make_batch(model.sharding, n, seed=n + len(scorer), weight=reg)
    check_sgd_step(model, model.sharding, batch, scorer, scheme, n, dev)


@pytest.mark.gpu
def test_masked_triples_are_no_terms_of_the_loss(dev):
    from besskge.regularizer import EmbeddingRegularizer

    model = make_model(dev, "ComplEx", 3, "t", EmbeddingRegularizer.n3(1e-2))
    batch = make_batch(model.sharding, 3, seed=7, weight=True, mask=True)
    check_sgd_step(model, model.sharding, batch, "ComplEx", "t", 3, dev)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3])
def test_two_adagrad_steps(dev, n):
    """Adagrad from zero state, restated in float64: acc += g^2, x -= lr g / (sqrt(acc) + eps).  Entries whose
    gradient all but cancels are left out of the comparison (g / sqrt(g^2) turns rounding into a full step, as in
    tests/test_optimizers.py); the tolerance is the one tests/test_accumulation.py holds sign-normalising optimisers
    to on fp32 tables (rtol 2e-3, atol 5e-5)."""
    from besskge import runtime

    scorer, scheme, lr, eps = "ComplEx", "t", 0.1, 1e-10
    model = make_model(dev, scorer, n, scheme)
    sharding = model.sharding
    batch = make_batch(sharding, n, micro=2, seed=3)
    runner = runtime.training_model(model, runtime.Options(device_iterations=1), runtime.Adagrad(lr=lr, eps=eps),
                                    device=dev)
    E, R = tables(model)
    accE, accR = torch.zeros_like(E), torch.zeros_like(R)
    solid, solid_r = torch.ones_like(E, dtype=torch.bool), torch.ones_like(R, dtype=torch.bool)
    for it in range(2):
        step = {k: v[it * n:(it + 1) * n] for k, v in batch.items()}
        _, _, dE, dR = reference(model, sharding, step, scorer, scheme, n)
        runner(**step)
        accE, accR = accE + dE ** 2, accR + dR ** 2
        E = E - lr * dE / (accE.sqrt() + eps)
        R = R - lr * dR / (accR.sqrt() + eps)
        solid &= (dE.abs() > 1e-4) | (dE == 0)
        solid_r &= (dR.abs() > 1e-4) | (dR == 0)
    E1, R1 = tables(model)
    torch.testing.assert_close(E1[solid], E[solid], rtol=2e-3, atol=5e-5)
    torch.testing.assert_close(R1[solid_r], R[solid_r], rtol=2e-3, atol=5e-5)
    assert float(solid.float().mean()) > 0.9 and float(solid_r.float().mean()) > 0.9


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3])
def test_gradient_accumulation(dev, n):
    """k = 2 micro-batches accumulated = one plain-SGD step on the sum of their gradients."""
    from besskge import runtime

    scorer, scheme = "DistMult", "h"
    model = make_model(dev, scorer, n, scheme)
    sharding = model.sharding
    batch = make_batch(sharding, n, micro=2, seed=5)
    grads = [reference(model, sharding, batch, scorer, scheme, n, row0=it * n) for it in range(2)]
    E0, R0 = tables(model)
    options = runtime.Options(device_iterations=1, gradient_accumulation=2)
    runner = runtime.training_model(model, options, runtime.SGD(lr=LR), device=dev)
    runner(**batch)
    E1, R1 = tables(model)
    torch.testing.assert_close((E0 - E1) / LR, grads[0][2] + grads[1][2], rtol=1e-4, atol=4e-5)
    torch.testing.assert_close((R0 - R1) / LR, grads[0][3] + grads[1][3], rtol=1e-4, atol=4e-5)


@pytest.mark.gpu
def test_a_capturing_stream_is_refused(dev, monkeypatch):
    """(the step reads a flag on the host: it says so instead of recording a graph that would not replay it)"""
    from besskge import _native as nat

    model = make_model(dev, "DistMult", 1, "t")
    batch = make_batch(model.sharding, 1)
    from besskge import runtime

    runner = runtime.training_model(model, runtime.Options(device_iterations=1), runtime.SGD(lr=LR), device=dev)
    monkeypatch.setattr(nat, "_capturing", lambda d: True)
    with pytest.raises(RuntimeError, match="eagerly"):
        runner(**batch)


@pytest.mark.gpu
def test_example_trains_one_vs_all():
    """examples/train_and_evaluate.py --training 1vsall: ComplEx-N3 over all entities learns the synthetic graph
    (the thresholds of the example's other tests)."""
    import importlib.util
    import os

    from conftest import REPO

    spec = importlib.util.spec_from_file_location("train_and_evaluate",
                                                  os.path.join(REPO, "examples", "train_and_evaluate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = mod.main(["--training", "1vsall", "--scorer", "ComplEx", "--regularizer", "n3", "--n-shard", "2",
                    "--steps", "150"])
    assert res["losses"][-1] < 0.5 * res["losses"][0], res
    assert res["hits@10"] > 0.2 and res["mrr"] > 0.1, res
