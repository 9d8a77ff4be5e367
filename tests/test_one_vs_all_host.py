"""1vsAll training, host side (no GPU): what `OneVsAllBessKGE` refuses, the identity that anchors the loss the
GPU tests restate to the project's oracle, and the workspace queries of the two entry points."""

import ctypes

import pytest
import torch

from oracle import kge

from test_hip_parity import make_scorer, widths


def _scorer(name, n_entity=50, n_shard=1, d=8, sharing=True):
    from besskge.sharding import Sharding

    sharding = Sharding.create(n_entity, n_shard, seed=0)
    ew, rw = widths(name, d)
    ent = torch.randn(n_shard, sharding.max_entity_per_shard, ew)
    return make_scorer(name, 1, sharing, 5, d, ent, torch.randn(5, rw), torch.device("cpu"), sharding=sharding)


def test_constructor_refusals():
    from besskge.loss import LogSigmoidLoss, SampledSoftmaxCrossEntropyLoss
    from besskge.negative_sampler import PlaceholderNegativeSampler, RandomShardedNegativeSampler
    from besskge.one_vs_all import OneVsAllBessKGE

    fn = _scorer("ComplEx")
    loss = SampledSoftmaxCrossEntropyLoss(n_entity=50)
    ok = OneVsAllBessKGE(PlaceholderNegativeSampler("t"), fn, loss)
    assert ok.loss_fn is loss and not ok.return_scores
    OneVsAllBessKGE(PlaceholderNegativeSampler("h"), _scorer("TransE"), loss)
    with pytest.raises(ValueError, match="PlaceholderNegativeSampler"):
        OneVsAllBessKGE(PlaceholderNegativeSampler("ht"), fn, loss)
    sampled = RandomShardedNegativeSampler(n_negative=4, sharding=fn.sharding, seed=1, corruption_scheme="t",
                                           local_sampling=False, flat_negative_format=True)
    with pytest.raises(ValueError, match="PlaceholderNegativeSampler"):
        OneVsAllBessKGE(sampled, fn, loss)
    with pytest.raises(ValueError, match="SampledSoftmaxCrossEntropyLoss"):
        OneVsAllBessKGE(PlaceholderNegativeSampler("t"), fn, LogSigmoidLoss(margin=1.0, negative_adversarial_sampling=False))
    with pytest.raises(ValueError, match="n_entity"):
        OneVsAllBessKGE(PlaceholderNegativeSampler("t"), fn, SampledSoftmaxCrossEntropyLoss(n_entity=49))
    with pytest.raises(ValueError, match="proposal_correction"):
        OneVsAllBessKGE(PlaceholderNegativeSampler("t"), fn,
                        SampledSoftmaxCrossEntropyLoss(n_entity=50, proposal_correction=True))
    with pytest.raises(ValueError, match="TransE, RotatE, DistMult or ComplEx"):
        OneVsAllBessKGE(PlaceholderNegativeSampler("t"), _scorer("PairRE"), loss)
    with pytest.raises(ValueError, match="return_scores"):
        OneVsAllBessKGE(PlaceholderNegativeSampler("t"), fn, loss, return_scores=True)


def test_one_vs_all_loss_is_the_oracles_sampled_softmax_over_all_other_entities():
    """float64, 50 entities: loss_scale * sum_i w_i (logsumexp_e score(q_i, e) - pos_i) equals the oracle's "ssce"
    with the N = n_entity - 1 other entities as negatives (shift log(N) - log(N) = 0): value and gradient."""
    g = torch.Generator().manual_seed(0)
    n_entity, S = 50, 12
    table = torch.randn(n_entity, 6, generator=g, dtype=torch.float64).requires_grad_(True)
    q = torch.randn(S, 6, generator=g, dtype=torch.float64).requires_grad_(True)
    tails = torch.randint(n_entity, (S,), generator=g)
    w = torch.rand(S, generator=g, dtype=torch.float64)
    w[3] = 0.0
    scale = 1.7

    def grads(loss):
        out = torch.autograd.grad(loss, (table, q), retain_graph=True)
        return out

    scores = q @ table.T
    pos = scores[torch.arange(S), tails]
    mine = scale * (w * (torch.logsumexp(scores, dim=1) - pos)).sum()
    others = torch.stack([torch.cat([torch.arange(t), torch.arange(t + 1, n_entity)]) for t in tails.tolist()])
    neg = torch.gather(scores, 1, others)
    theirs = kge.loss_value("ssce", pos, neg, w, loss_scale=scale, n_entity=n_entity)
    torch.testing.assert_close(mine, theirs, rtol=1e-13, atol=1e-13)
    for a, b in zip(grads(mine), grads(theirs)):
        torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-13)


def test_workspace_queries_are_host_arithmetic():
    from besskge import _native as nat

    lib = nat.load()
    shapes = [("DistMult", 0, nat.F32, 20, 70, 333), ("ComplEx", 0, nat.F16, 32, 70, 333),
              ("TransE", 1, nat.F32, 24, 70, 333), ("TransE", 2, nat.F32, 24, 70, 333), ("RotatE", 1, nat.F16, 16, 70, 333),
              ("DistMult", 0, nat.F32, 64, 512, 8192 + 37), ("ComplEx", 0, nat.F16, 64, 512, 8192 + 37),
              ("DistMult", 0, nat.F32, 32, 128, 65536 + 200), ("TransE", 1, nat.F32, 8, 1, 1),
              ("ComplEx", 0, nat.F32, 256, 4096, 93773)]
    for name, p, dtype, W, nq, n_neg in shapes:
        d = nat.ModelDesc()
        d.scorer = {"TransE": nat.TRANSE, "RotatE": nat.ROTATE, "DistMult": nat.DISTMULT, "ComplEx": nat.COMPLEX}[name]
        d.norm_p, d.dtype, d.width, d.rel_width = p, dtype, W, (W // 2 if name == "RotatE" else W)
        fwd = lib.bess_neg_score_shared_fwd_lse_workspace(ctypes.byref(d), nq, n_neg)
        bwd = lib.bess_neg_score_shared_bwd_softmax_workspace(ctypes.byref(d), nq, n_neg)
        assert fwd > 0 and bwd > 0, (name, nq, n_neg)
        # bounded: a 64 MiB tile (or the split product's images of at most 65,536 rows), never the score matrix
        assert fwd < (1 << 30) and bwd < (1 << 30)
        if lib.bess_neg_score_shared_workspace(ctypes.byref(d), nq, n_neg) == 0:
            cols = min((64 << 20) // 4 // nq // 64 * 64, (n_neg + 63) // 64 * 64)
            assert fwd == nq * cols * 4
            assert bwd == (nq * W * 4 + 255) // 256 * 256 + 2 * nq * cols * 4
    # the state of a row does not depend on n_neg beyond one chunk of the split product
    d = nat.ModelDesc()
    d.scorer, d.norm_p, d.dtype, d.width, d.rel_width = nat.COMPLEX, 0, nat.F32, 256, 256
    assert lib.bess_neg_score_shared_fwd_lse_workspace(ctypes.byref(d), 4096, 1 << 17) == \
        lib.bess_neg_score_shared_fwd_lse_workspace(ctypes.byref(d), 4096, 1 << 22)
    box = nat.ModelDesc()
    box.scorer, box.norm_p, box.dtype, box.width, box.rel_width = nat.BOXE, 1, nat.F32, 16, 34
    box.reserved[0] = 3
    assert lib.bess_neg_score_shared_fwd_lse_workspace(ctypes.byref(box), 64, 64) == 0
