"""The distance route of TransE / RotatE at p = 2 (`distance_route="gram"`, BESS_FLAG_GRAM_L2): the split-fp16
matrix-core product with the distance transform in front of its epilogues (csrc/gemm_split.hip) and the two
matrix-core products of its backward, against float64 on the CPU.

Scores hold the project's parity tolerance (rtol 1e-4, atol 1e-5): pairs that are not recomputed have
d^2 >= TAU (nq + ne), where the expanded form is off by at most c 2^-22 (nq + ne) / (2 d) - the test prints c (DESIGN
section 38 derives c <= 3.2 as the limit for TAU = 2^-8).  Gradients: `GRAM_GRAD_MEASURED` is the largest deviation
from float64 autograd, relative to the row's largest |gradient element|, measured on the MI355X over the cases of
`test_backward`; the test holds 4 x that."""

import ctypes

import pytest
import torch

from test_one_vs_all_kernels import F64, dev, grad_deviation, lse_of, make_desc, problem, ref_scores  # noqa: F401

TAU = 2.0 ** -8
NQ, N_NEG = 2048, 2048 + 37  # 16 x 17 = 272 tiles of 128 x 128: just over the gate of 256, ragged last tile
#: largest gradient deviation of the gram route measured on the MI355X (see the module docstring)
GRAM_GRAD_MEASURED = 7.95e-7  # 2026-11-26 (d_query, fp16 table, W = 64, 2048 x 2053; the direct kernels, which take
#                              the 256 x 389 cases - too few tiles for the backward products - deviate by up to 1.05e-6)


def gram_desc(name, dtype, W):
    from besskge import _native as nat

    d = make_desc(name, 2, dtype, W)
    d.reserved[0] |= nat.FLAG_GRAM_L2
    return d


def planted(name, dtype, W, nq, n_neg, big=False):
    """(query, table, idx, float64 scores): 24 queries sit on / next to a candidate - 8 exact duplicates, 8 at
    |delta| = 1e-3 |q|, 8 just outside the recompute threshold |delta|^2 = TAU (nq + ne)"""
    query, table = problem(name, dtype, W, nq, n_neg + 100, seed=W + len(name))
    g = torch.Generator().manual_seed(W)
    idx = torch.randperm(n_neg + 100, generator=g)[:n_neg].to(torch.int32)
    rows = table[idx.long()].float()
    for k in range(24):
        e = rows[3 + (n_neg // 25) * k]
        u = torch.randn(W, generator=g)
        step = (0.0, 1e-3, 1.05 * (2 * TAU) ** 0.5)[k // 8] * float(e.norm())
        query[7 + (nq // 25) * k] = e + u / u.norm() * step
    if big:
        query[5, 3] = 1e5  # outside the fp16 range: the pre-pass raises the flag, the direct kernels score
    return query, table, idx, ref_scores(name, 2, query.double(), rows.double())


CASES = [("TransE", torch.float32), ("TransE", torch.float16), ("RotatE", torch.float32)]


@pytest.mark.gpu
@pytest.mark.parametrize("W,big", [(64, False), (100, False), (512, False), (64, True)])
@pytest.mark.parametrize("name,dtype", CASES)
def test_scores(dev, name, dtype, W, big):
    from besskge import _native as nat

    d = gram_desc(name, dtype, W)
    assert nat.load().bess_neg_score_shared_workspace(ctypes.byref(d), NQ, N_NEG) > 0  # (0 without the route)
    query, table, idx, want = planted(name, dtype, W, NQ, N_NEG, big)
    got = nat.neg_score_shared_fwd(d, query.to(dev), nat.RowSource(table.to(dev), idx.to(dev))).double().cpu()
    nn = (query.double() ** 2).sum(1)[:, None] + (table[idx.long()].double() ** 2).sum(1)[None, :]
    far = want ** 2 >= TAU * nn  # (pairs the kernel does not recompute, up to its own rounding of the test)
    unit = 2.0 ** -22 * nn / (2 * want.abs().clamp_min(1e-30))
    print(f"{name} {dtype} W={W} big={big}: c = {float(((got - want).abs() / unit)[far].max()):.3f}, "
          f"{int((~far).sum())} close pairs, max |err| {float((got - want).abs().max()):.3e}")
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-5)
    dup = [(7 + (NQ // 25) * k, 3 + (N_NEG // 25) * k) for k in range(8)]
    if not big:
        assert all(float(got[q, j]) == 0.0 for q, j in dup), "an exact duplicate scores exactly 0"


@pytest.mark.gpu
@pytest.mark.parametrize("W", [64, 100])
@pytest.mark.parametrize("name,dtype", CASES)
def test_epilogues(dev, name, dtype, W):
    """Counts, pair scores, pruned stores and log-sum-exp come out of the same transform as the stored scores."""
    from besskge import _native as nat

    d = gram_desc(name, dtype, W)
    query, table, idx, want = planted(name, dtype, W, NQ, N_NEG)
    q, neg = query.to(dev), nat.RowSource(table.to(dev), idx.to(dev))
    scores = nat.neg_score_shared_fwd(d, q, neg)
    excl = (torch.arange(NQ, dtype=torch.int32) * 7 % N_NEG).to(dev)
    thr = scores.gather(1, excl.long()[:, None]).reshape(-1).contiguous()
    gt, eq = scores > thr[:, None], scores == thr[:, None]
    keep = torch.ones_like(gt).scatter_(1, excl.long()[:, None], False)
    counts = nat.neg_score_shared_counts(d, q, neg, thr, excl)
    assert torch.equal(counts.long(), torch.stack([(gt & keep).sum(1), (eq & keep).sum(1)], dim=1))
    # nothing excluded: the threshold's own column ties only if the counting epilogue makes the stored score's bits
    every = nat.neg_score_shared_counts(d, q, neg, thr, torch.full_like(excl, -1))
    assert torch.equal(every.long(), torch.stack([gt.sum(1), eq.sum(1)], dim=1))
    pairs = nat.neg_score_shared_pairs(d, q, nat.RowSource(neg.base, neg.idx[excl.long()].contiguous()), NQ, N_NEG)
    assert torch.equal(pairs, thr), "pair scores are the all-entities scores, to the last bit"
    pruned, flags = nat.neg_score_shared_fwd_pruned(d, q, neg, thr)
    block = flags[:, :(N_NEG + 63) // 64].bool().repeat_interleave(64, dim=1)[:, :N_NEG]
    assert torch.equal(pruned[block], scores[block]) and not bool((gt & ~block).any())
    tol = 1e-4 * float(want.abs().max()) + 1e-5  # (the log-sum-exp is 1-Lipschitz in the scores)
    ref = torch.logsumexp(want, dim=1)
    state = nat.neg_score_shared_lse(d, q, neg)
    err = float((lse_of(state) - ref).abs().max())
    print(f"{name} {dtype} W={W}: lse max |err| {err:.3e}  tolerance {tol:.3e}")
    assert err <= tol
    # a second pass over the candidates in reversed order accumulates into the state: every term twice
    two = nat.neg_score_shared_lse(d, q, nat.RowSource(neg.base, idx.flip(0).contiguous().to(dev)), state_ml=state.clone())
    assert float((lse_of(two) - ref - torch.log(torch.tensor(2.0, dtype=F64))).abs().max()) <= tol


@pytest.mark.gpu
@pytest.mark.parametrize("nq,n_neg", [(256, 384 + 5), (2048, 2048 + 5)])  # (the second: both products on the matrix cores)
@pytest.mark.parametrize("W", [64, 100])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_backward(dev, dtype, W, nq, n_neg):
    from besskge import _native as nat

    name = "TransE"
    d = gram_desc(name, dtype, W)
    on_route = nat.load().bess_neg_score_shared_bwd_workspace(ctypes.byref(d), nq, n_neg) > 0
    assert on_route == (nq == 2048)  # (256 x 389 has too few tiles for the backward products: the direct kernels)
    query, table = problem(name, dtype, W, nq, n_neg, seed=W + nq)
    query[11] = table[17].float()  # an exact duplicate: its term of the gradient is 0, nothing is NaN
    g = torch.randn(nq, n_neg, generator=torch.Generator().manual_seed(9))
    qr = query.double().clone().requires_grad_(True)
    er = table.double().clone().requires_grad_(True)
    (ref_scores(name, 2, qr, er) * g.double()).sum().backward()
    q, neg = query.to(dev), nat.RowSource(table.to(dev))
    out = nat.neg_score_shared_fwd(d, q, neg)
    dq, dn = nat.neg_score_shared_bwd(d, q, neg, out, g.to(dev))
    assert bool(torch.isfinite(dq).all()) and bool(torch.isfinite(dn).all())
    dev_q, dev_e = grad_deviation(dq, qr.grad), grad_deviation(dn, er.grad)
    print(f"{dtype} W={W} {nq} x {n_neg}: gradient deviation d_query {dev_q:.3e}  d_neg {dev_e:.3e}")
    assert max(dev_q, dev_e) <= 4 * GRAM_GRAD_MEASURED
    if on_route:  # (the direct kernels join the slices of their reduction with fp32 atomics)
        dq2, dn2 = nat.neg_score_shared_bwd(d, q, neg, out, g.to(dev))
        assert torch.equal(dq, dq2) and torch.equal(dn, dn2), "bitwise reproducible"


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1024, 2048])  # (2048: the backward products are on the matrix cores as well)
@pytest.mark.parametrize("scorer", ["TransE", "RotatE"])
def test_one_vs_all_step(dev, scorer, S):
    """One SGD step of 1vsAll training on one shard of 4224 entities, W = 64, against float64 autograd + SGD."""
    from besskge import runtime, scoring
    from besskge.loss import SampledSoftmaxCrossEntropyLoss
    from besskge.negative_sampler import PlaceholderNegativeSampler
    from besskge.one_vs_all import OneVsAllBessKGE
    from besskge.sharding import Sharding
    from oracle import kge

    n_entity, n_rel, lr = 4224, 5, 0.5
    sharding = Sharding.create(n_entity, 1, seed=0)
    fn = getattr(scoring, scorer)(True, 2, sharding, n_rel, 64 if scorer == "TransE" else 32, device=dev,
                                  distance_route="gram")
    g = torch.Generator().manual_seed(S)
    with torch.no_grad():  # uniform in [-1, 1]
        fn.entity_embedding.copy_(torch.rand(fn.entity_embedding.shape, generator=g) * 2 - 1)
        fn.relation_embedding.copy_(torch.rand(fn.relation_embedding.shape, generator=g) * 2 - 1)
    model = OneVsAllBessKGE(PlaceholderNegativeSampler("t"), fn, SampledSoftmaxCrossEntropyLoss(n_entity))
    batch = {k: torch.randint(n_rel if k == "relation" else n_entity, (1, 1, S), generator=g, dtype=torch.int32)
             for k in ("head", "relation", "tail")}
    E = fn.entity_embedding.detach().double().cpu().requires_grad_(True)
    R = fn.relation_embedding.detach().double().cpu().requires_grad_(True)
    h, t, rid = E[0][batch["head"].long().reshape(-1)], E[0][batch["tail"].long().reshape(-1)], batch["relation"].long().reshape(-1)
    sc = -torch.cdist(kge.query(scorer, "t", h, R[rid]), E[0][:n_entity], p=2.0)
    loss = float(model.loss_fn.loss_scale) * (torch.logsumexp(sc, dim=1) - kge.score_triple(scorer, 2, h, R, rid, t)).sum()
    loss.backward()
    E0 = fn.entity_embedding.detach().double().cpu().clone()
    out = runtime.training_model(model, runtime.Options(device_iterations=1), runtime.SGD(lr=lr), device=dev)(**batch)
    torch.testing.assert_close(out["loss"].double().cpu().reshape(-1), loss.detach().reshape(-1), rtol=1e-5, atol=1e-4)
    torch.testing.assert_close((E0 - fn.entity_embedding.detach().double().cpu()) / lr, E.grad, rtol=1e-4, atol=2e-5)


@pytest.mark.parametrize("scorer", ["TransE", "RotatE"])
def test_public_switch(scorer):
    from besskge import _native as nat
    from besskge import scoring
    from besskge.sharding import Sharding

    sharding = Sharding.create(64, 1, seed=0)
    with pytest.raises(ValueError):
        getattr(scoring, scorer)(True, 1, sharding, 4, 8, distance_route="gram")
    gram = getattr(scoring, scorer)(True, 2, sharding, 4, 8, distance_route="gram")
    direct = getattr(scoring, scorer)(True, 2, sharding, 4, 8)
    assert gram.kernel_desc().reserved[0] & nat.FLAG_GRAM_L2 and not direct.kernel_desc().reserved[0] & nat.FLAG_GRAM_L2
    assert gram.state_dict().keys() == direct.state_dict().keys()
