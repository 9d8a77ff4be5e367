"""KvsAll training, host side (no GPU): what `KvsAllBessKGE` and `AllEntitiesBCELoss` refuse."""

import numpy as np
import pytest
import torch

from test_one_vs_all_host import _scorer


def test_loss_arguments():
    from besskge.loss import AllEntitiesBCELoss

    loss = AllEntitiesBCELoss(50, label_smoothing=0.1, loss_scale=2.0)
    assert loss.smooth == pytest.approx(0.002) and loss.positive_weight == pytest.approx(0.9)
    assert float(loss.loss_scale) == 2.0 and AllEntitiesBCELoss(50).smooth == 0.0
    for bad in (-0.1, 1.0):
        with pytest.raises(ValueError, match="label_smoothing"):
            AllEntitiesBCELoss(50, label_smoothing=bad)
    with pytest.raises(ValueError, match="n_entity"):
        AllEntitiesBCELoss(0)
    with pytest.raises(RuntimeError, match="score matrices"):
        loss(torch.zeros(3), torch.zeros(3, 50), torch.ones(1))


def test_constructor_refusals():
    from besskge.k_vs_all import KvsAllBessKGE
    from besskge.loss import AllEntitiesBCELoss, SampledSoftmaxCrossEntropyLoss
    from besskge.negative_filter import KnownTripleFilter
    from besskge.negative_sampler import PlaceholderNegativeSampler

    fn = _scorer("ComplEx")  # 50 entities, 5 relation types
    loss = AllEntitiesBCELoss(50, label_smoothing=0.1)
    triples = np.array([[0, 1, 2], [0, 1, 3], [4, 0, 2]])
    ok = KvsAllBessKGE(PlaceholderNegativeSampler("t"), fn, loss, [triples])
    assert ok.loss_fn is loss and ok.known_triples.n_triple == 3
    KvsAllBessKGE(PlaceholderNegativeSampler("h"), _scorer("TransE"), loss, KnownTripleFilter([triples], 50, 5))
    with pytest.raises(ValueError, match="PlaceholderNegativeSampler"):
        KvsAllBessKGE(PlaceholderNegativeSampler("ht"), fn, loss, [triples])
    with pytest.raises(ValueError, match="TransE, RotatE, DistMult or ComplEx"):
        KvsAllBessKGE(PlaceholderNegativeSampler("t"), _scorer("PairRE"), loss, [triples])
    with pytest.raises(ValueError, match="AllEntitiesBCELoss"):
        KvsAllBessKGE(PlaceholderNegativeSampler("t"), fn, SampledSoftmaxCrossEntropyLoss(n_entity=50), [triples])
    with pytest.raises(ValueError, match="AllEntitiesBCELoss"):
        KvsAllBessKGE(PlaceholderNegativeSampler("t"), fn, AllEntitiesBCELoss(49), [triples])
    for sizes in ((51, 5), (50, 6)):
        with pytest.raises(ValueError, match="the filter indexes"):
            KvsAllBessKGE(PlaceholderNegativeSampler("t"), fn, loss, KnownTripleFilter([triples], *sizes))
