"""`OneVsAllBessKGE(relation_prediction_weight=0.5)`: one plain-SGD step against a float64 restatement of the whole
loss with autograd on the unsharded tables - the entity term of tests/test_one_vs_all.py, plus

    0.5 * loss_scale * sum_i w_i (log sum_{r' < n_relation} exp(<R[r'], g(h_i, t_i)>) - pos_i)

plus N3 in one case.  41 entities (two shards: unequal, one pad row), 5 relations, rows of 8 scalars, 12 triples per
replica with non-unit weights and masked triples.  Tolerances: the project's for fp32 paths (rtol 1e-4, atol 1e-5)."""

import numpy as np
import pytest
import torch

import test_k_vs_all as kva
from test_one_vs_all import dev, scores_all, tables  # noqa: F401
from test_regularizer import phi
from test_relation_lse_kernels import g64

N_ENTITY, N_REL, W, S = 41, 5, 8, 12
LR, WEIGHT, TOL = 0.5, 0.5, dict(rtol=1e-4, atol=1e-5)


def make_model(dev, scorer, n, scheme, reg=None, n_rel=N_REL, **kw):
    from besskge import scoring
    from besskge.loss import SampledSoftmaxCrossEntropyLoss
    from besskge.negative_sampler import PlaceholderNegativeSampler
    from besskge.one_vs_all import OneVsAllBessKGE
    from besskge.sharding import Sharding

    sharding = Sharding.create(N_ENTITY, n, seed=0)
    fn = getattr(scoring, scorer)(True, sharding, n_rel, W // 2 if scorer == "ComplEx" else W, device=dev)
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():  # uniform in [-1, 1]
        fn.entity_embedding.copy_(torch.rand(fn.entity_embedding.shape, generator=gen) * 2 - 1)
        fn.relation_embedding.copy_(torch.rand(fn.relation_embedding.shape, generator=gen) * 2 - 1)
    return OneVsAllBessKGE(PlaceholderNegativeSampler(scheme), fn, SampledSoftmaxCrossEntropyLoss(N_ENTITY, loss_scale=1.5),
                           regularizer=reg, **kw)


def make_batch(sharding, n, seed):
    rng = np.random.default_rng(seed)
    counts, ppp = sharding.shard_counts.reshape(n, 1, 1), S // n
    b = dict(head=(rng.random((n, n, ppp)) * counts).astype(np.int32),
             relation=rng.integers(N_REL, size=(n, n, ppp)).astype(np.int32),
             tail=(rng.random((n, n, ppp)) * counts).astype(np.int32),
             triple_weight=rng.random(size=(n, S)).astype(np.float32) + 0.5, triple_mask=np.ones((n, n, ppp), dtype=bool))
    b["relation"][0, 0, 0] = N_REL - 1
    b["triple_mask"][:, 0, 1] = b["triple_mask"][:, n - 1, 4] = False
    return {k: torch.from_numpy(v) for k, v in b.items()}


def replica_rows(E, batch, r, n):
    """(head rows, tail rows, relation ids, weights) of replica r's triples, (j, q) order"""
    h = E[r][batch["head"][r].long().reshape(-1)]
    t = torch.stack([E[j][batch["tail"][j][r].long()] for j in range(n)]).reshape(h.shape)
    w = batch["triple_weight"][r].double() * batch["triple_mask"][r].reshape(-1).double()
    return h, t, batch["relation"][r].long().reshape(-1), w


def relation_terms(E, R, batch, n, scale, cplx):
    """per replica: scale * sum_i w_i (logsumexp_r' <R[r'], g(h_i, t_i)> - <R[r_i], g(h_i, t_i)>), float64"""
    out = []
    for r in range(n):
        h, t, rid, w = replica_rows(E, batch, r, n)
        s = g64(h, t, cplx) @ R.T
        out.append(scale * (w * (torch.logsumexp(s, dim=1) - s[torch.arange(len(rid)), rid])).sum())
    return torch.stack(out)


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["t", "h"])
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("scorer", ["DistMult", "ComplEx"])
def test_sgd_step_against_float64(dev, scorer, n, scheme):
    from besskge import runtime
    from besskge.regularizer import EmbeddingRegularizer

    reg = EmbeddingRegularizer.n3(1e-2) if (scorer, n) == ("ComplEx", 2) else None
    model = make_model(dev, scorer, n, scheme, reg, relation_prediction_weight=WEIGHT)
    sharding, scale = model.sharding, float(model.loss_fn.loss_scale)
    batch = make_batch(sharding, n, seed=n)
    E0, R0 = tables(model)
    E, R = E0.clone().requires_grad_(True), R0.clone().requires_grad_(True)
    real = torch.cat([E[s, : int(sharding.shard_counts[s])] for s in range(n)])
    rp = relation_terms(E, R, batch, n, scale, scorer == "ComplEx")
    loss = []
    for r in range(n):
        h, t, rid, w = replica_rows(E, batch, r, n)
        sc = scores_all(scorer, scheme, h if scheme == "t" else t, R[rid], real)
        pos = (g64(h, t, scorer == "ComplEx") * R[rid]).sum(dim=1)
        loss.append(scale * (w * (torch.logsumexp(sc, dim=1) - pos)).sum() + WEIGHT * rp[r])
        if reg is not None:
            loss[-1] = loss[-1] + (scale * w * (reg.entity_coef * (phi(h, reg.p, model._regularizer_flags & 1)
                                                                   + phi(t, reg.p, model._regularizer_flags & 1))
                                                + reg.relation_coef * phi(R[rid], reg.p, model._regularizer_flags & 2))).sum()
    sum(loss).backward()
    out = runtime.training_model(model, runtime.Options(device_iterations=1), runtime.SGD(lr=LR), device=dev)(**batch)
    E1, R1 = tables(model)
    torch.testing.assert_close(out["loss"].double().cpu().reshape(-1), torch.stack(loss).detach(), **TOL)
    torch.testing.assert_close(out["relation_prediction"].double().cpu().reshape(-1), rp.detach(), **TOL)
    torch.testing.assert_close(E1, E0 - LR * E.grad, **TOL)
    torch.testing.assert_close(R1, R0 - LR * R.grad, **TOL)


@pytest.mark.gpu
def test_k_vs_all_step(dev):
    """tests/test_k_vs_all.py's ComplEx step (300 entities, one shard) with the relation term added to its reference."""
    from besskge import runtime
    from besskge.k_vs_all import KvsAllBessKGE

    bt = kva.BatchTriples(300, 1)
    plain, known = kva.make_model(dev, "ComplEx", 300, 1, "t", 0.1, bt)
    model = KvsAllBessKGE(plain.negative_sampler, plain.score_fn, plain.loss_fn, [known], relation_prediction_weight=WEIGHT)
    want_loss, _, dE, dR, tols = kva.reference(model, bt, known, "ComplEx", "t", 1)
    E0, R0 = tables(model)
    E, R = E0.clone().requires_grad_(True), R0.clone().requires_grad_(True)
    rp = relation_terms(E, R, bt.batch, 1, float(model.loss_fn.loss_scale), True)
    rp.sum().backward()
    out = runtime.training_model(model, runtime.Options(device_iterations=1), runtime.SGD(lr=LR), device=dev)(**bt.batch)
    E1, R1 = tables(model)
    torch.testing.assert_close(out["relation_prediction"].double().cpu().reshape(-1), rp.detach(), **TOL)
    torch.testing.assert_close(out["loss"].double().cpu().reshape(-1), want_loss + WEIGHT * rp.detach(), rtol=1e-4,
                               atol=1e-5 + tols[0])
    torch.testing.assert_close(E1, E0 - LR * (dE + WEIGHT * E.grad), **TOL)
    torch.testing.assert_close(R1, R0 - LR * (dR + WEIGHT * R.grad), **TOL)


@pytest.mark.gpu
def test_weight_zero_is_the_step_without_the_argument(dev):
    from besskge import runtime

    """A step is bitwise reproducible only where no float atomics meet: momentum SGD sums the entity gradients per
    unique row in a fixed order, and with every relation named by one triple a row of the relation gradient gets
    two addends (positive score, query), whose sum does not depend on their order."""
    got = []
    for kw in ({}, dict(relation_prediction_weight=0.0)):
        model = make_model(dev, "ComplEx", 1, "t", n_rel=S, **kw)
        batch = make_batch(model.sharding, 1, seed=2)
        batch["relation"] = torch.arange(S, dtype=torch.int32).reshape(1, 1, S)
        out = runtime.training_model(model, runtime.Options(device_iterations=1), runtime.SGD(lr=LR, momentum=0.5),
                                     device=dev)(**batch)
        assert "relation_prediction" not in out
        got.append(tables(model))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
