"""`KvsAllBessKGE`: one plain-SGD step whose binary cross entropy runs over all entities, against a float64 torch
restatement of the whole loss (`BCEWithLogits` on a dense label matrix, autograd) on the UNSHARDED entity table.

The batch layout is tests/test_one_vs_all.py's.  The filter holds the batch's triples but one (whose completion must
be labelled all the same), extra completions of batch queries on BOTH shards, and 40 completions of one hub query.
300 entities fill one and two shards exactly; 301 over two shards gives unequal shards and a pad row, which no step
may touch.

Tolerances.  Gradients, read off the step as (before - after) / lr: those of tests/test_one_vs_all.py (rtol 1e-4,
atol 2e-5: the fp32 kernels' shared-negative tolerance, the differencing and one more fp32 addition for rows that
are candidate and head / tail).  The loss is sum_i coef_i (A_i - smooth B_i - pw (C_i + pos_i)); with the per-row
bounds of tests/test_k_vs_all_kernels.py (delta = W 2^-24 max(1, max|s|), L <= 5 + 6 + 1 + n_shard levels) it is off
by at most sum_i coef_i ((2 N + K_i + 1) delta + (L + 2) 2^-24 (A_i + sum_e |s_ie|)), plus S 2^-24 sum_i |term_i|
for the final sum over the S rows."""

import numpy as np
import pytest
import torch

from test_one_vs_all import LR, dev, make_batch, scores_all, tables  # noqa: F401

N_REL, W, S_SHARD = 6, 32, 64


def make_model(dev, scorer, n_entity, n, scheme, eps, batch_triples):
    """(model, known triples [k, 3] global ids): the filter of the module docstring around the batch's triples"""
    from besskge import scoring
    from besskge.k_vs_all import KvsAllBessKGE
    from besskge.loss import AllEntitiesBCELoss
    from besskge.negative_sampler import PlaceholderNegativeSampler

    sharding = batch_triples.sharding
    torch.manual_seed(0)
    if scorer == "TransE":
        fn = scoring.TransE(True, 1, sharding, N_REL, W, device=dev)
    else:
        fn = scoring.ComplEx(True, sharding, N_REL, W // 2, device=dev)
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():  # uniform in [-1, 1]
        fn.entity_embedding.copy_(torch.rand(fn.entity_embedding.shape, generator=gen) * 2 - 1)
        fn.relation_embedding.copy_(torch.rand(fn.relation_embedding.shape, generator=gen) * 2 - 1)
    hrt = batch_triples.hrt
    rng = np.random.default_rng(5)
    kept = 0 if scheme == "t" else 2
    extra = []
    for i in rng.choice(hrt.shape[0], 12, replace=False):  # completions anywhere: on the other shard too
        for e in rng.choice(n_entity, 3, replace=False):
            extra.append([e, hrt[i, 1], hrt[i, 2]] if kept == 2 else [hrt[i, 0], hrt[i, 1], e])
    for e in rng.choice(n_entity, 40, replace=False):  # a hub
        extra.append([e, hrt[1, 1], hrt[1, 2]] if kept == 2 else [hrt[1, 0], hrt[1, 1], e])
    known = np.concatenate([hrt[1:], np.array(extra, dtype=np.int64)])  # (triple 0 of the batch is not in the filter)
    loss = AllEntitiesBCELoss(n_entity, label_smoothing=eps, loss_scale=1.5 / n_entity)
    return KvsAllBessKGE(PlaceholderNegativeSampler(scheme), fn, loss, [known]), known


class BatchTriples:
    """The batch of `make_batch` and its triples in global ids, row-aligned with replica r's (j, q) order."""

    def __init__(self, n_entity, n):
        from besskge.sharding import Sharding

        self.sharding = Sharding.create(n_entity, n, seed=0)
        import test_one_vs_all as ova

        ova.PPP, ova.N_REL, keep = S_SHARD // n, N_REL, (ova.PPP, ova.N_REL)
        try:
            self.batch = make_batch(self.sharding, n, seed=n, weight=True, mask=True)
        finally:
            ova.PPP, ova.N_REL = keep
        l2g = self.sharding.shard_and_idx_to_entity
        b = {k: v.numpy() for k, v in self.batch.items()}
        self.per_replica = []
        for r in range(n):
            h = l2g[r][b["head"][r].reshape(-1)]
            t = np.stack([l2g[j][b["tail"][j][r]] for j in range(n)]).reshape(-1)
            self.per_replica.append(np.stack([h, b["relation"][r].reshape(-1), t], axis=1).astype(np.int64))
        self.hrt = np.concatenate(self.per_replica)


def reference(model, bt, known, scorer, scheme, n):
    """(loss per replica, positive scores per replica, d / d E, d / d R, loss tolerance per replica) in float64"""
    from oracle import kge

    sharding, batch, loss_fn = bt.sharding, bt.batch, model.loss_fn
    name = {"TransE": kge.TRANSE, "ComplEx": kge.COMPLEX}[scorer]
    E = model.score_fn.entity_embedding.detach().double().cpu().requires_grad_(True)
    R = model.score_fn.relation_embedding.detach().double().cpu().requires_grad_(True)
    counts = [int(c) for c in sharding.shard_counts]
    real = torch.cat([E[s, : counts[s]] for s in range(n)])  # every real entity, shard by shard
    col_of = np.concatenate([[0], np.cumsum(counts)])[sharding.entity_to_shard] + sharding.entity_to_idx
    kept, comp = (0, 2) if scheme == "t" else (2, 0)
    completions = {}
    for row in known:
        completions.setdefault((int(row[kept]), int(row[1])), []).append(int(row[comp]))
    losses, poss, tols = [], [], []
    for r in range(n):
        h = E[r][batch["head"][r].long().reshape(-1)]
        t = torch.stack([E[j][batch["tail"][j][r].long()] for j in range(n)]).reshape(h.shape)
        rid = batch["relation"][r].long().reshape(-1)
        w = batch["triple_weight"][r].double() * batch["triple_mask"][r].reshape(-1).double()
        y = torch.zeros(h.shape[0], real.shape[0], dtype=torch.float64)
        for i, row in enumerate(bt.per_replica[r]):
            y[i, col_of[completions.get((int(row[kept]), int(row[1])), []) + [int(row[comp])]]] = 1.0
        sc = scores_all(scorer, scheme, h if scheme == "t" else t, R[rid], real)
        bce = torch.nn.functional.binary_cross_entropy_with_logits(
            sc, loss_fn.positive_weight * y + loss_fn.smooth, reduction="none").sum(dim=1)
        coef = float(loss_fn.loss_scale) * w
        losses.append((coef * bce).sum())
        poss.append(kge.score_triple(name, 1, h, R, rid, t).detach())
        s = sc.detach()
        delta = W * 2.0 ** -24 * max(1.0, float(s.abs().max()))
        per_row = (2 * s.shape[1] + y.sum(1) + 1) * delta + (14 + n) * 2.0 ** -24 * (
            torch.nn.functional.softplus(s).sum(1) + s.abs().sum(1))
        tols.append(float((coef * per_row).sum() + h.shape[0] * 2.0 ** -24 * (coef * bce.detach()).abs().sum()))
    sum(losses).backward()
    return torch.stack(losses).detach(), poss, E.grad, R.grad, tols


@pytest.mark.gpu
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("n_entity,n", [(300, 1), (300, 2), (301, 2)])
@pytest.mark.parametrize("scheme", ["t", "h"])
@pytest.mark.parametrize("scorer", ["ComplEx", "TransE"])
def test_sgd_step_against_float64(dev, scorer, scheme, n_entity, n, eps):
    from besskge import runtime

    bt = BatchTriples(n_entity, n)
    model, known = make_model(dev, scorer, n_entity, n, scheme, eps, bt)
    sharding = bt.sharding
    want_loss, want_pos, dE, dR, tols = reference(model, bt, known, scorer, scheme, n)
    E0, R0 = tables(model)
    runner = runtime.training_model(model, runtime.Options(device_iterations=1), runtime.SGD(lr=LR), device=dev)
    out = runner(**bt.batch)
    E1, R1 = tables(model)
    got = out["loss"].double().cpu().reshape(-1)
    print(f"loss {got.tolist()} want {want_loss.tolist()} |err| {(got - want_loss).abs().tolist()} bound {tols}")
    assert bool(((got - want_loss).abs() <= torch.tensor(tols)).all())
    torch.testing.assert_close(out["positive_score"].double().cpu().reshape(n, -1), torch.stack(want_pos),
                               rtol=1e-4, atol=1e-5)
    torch.testing.assert_close((E0 - E1) / LR, dE, rtol=1e-4, atol=2e-5)
    torch.testing.assert_close((R0 - R1) / LR, dR, rtol=1e-4, atol=2e-5)
    for s in range(n):  # pad rows are no entities: bitwise unchanged
        assert torch.equal(E0[s, int(sharding.shard_counts[s]):], E1[s, int(sharding.shard_counts[s]):])
    assert int(sharding.shard_counts.sum()) == n_entity and (n_entity == 300 or sharding.shard_counts.min() < 151)
