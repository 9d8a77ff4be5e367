"""ConvE's `query_route` and its acceptance by the all-entities steps: what is decided on the host (no GPU needed)."""

import numpy as np
import pytest

from besskge.k_vs_all import KvsAllBessKGE
from besskge.loss import AllEntitiesBCELoss, SampledSoftmaxCrossEntropyLoss
from besskge.negative_sampler import PlaceholderNegativeSampler
from besskge.one_vs_all import OneVsAllBessKGE
from besskge.scoring import ConvE
from besskge.sharding import Sharding

N_ENT = 50


def conve(route="fused", **kw):
    return ConvE(True, Sharding.create(N_ENT, 2, seed=0), 4, 36, 6, 6, inverse_relations=False, output_channels=4,
                 query_route=route, **kw)


def test_query_route_is_validated():
    with pytest.raises(ValueError, match="query_route"):
        conve("miopen")
    assert conve("torch").query_route == "torch" and ConvE(True, Sharding.create(N_ENT, 1, seed=0), 4, 36, 6, 6).query_route == "torch"
    names = [sorted(conve(r).state_dict()) for r in ("torch", "fused")]
    assert names[0] == names[1] and len(conve("fused").dense_parameters()) == len(conve("torch").dense_parameters())


def test_fused_route_refuses_images_beyond_the_lds_limit():
    sharding = Sharding.create(N_ENT, 1, seed=0)
    with pytest.raises(RuntimeError, match="bytes of LDS"):
        ConvE(True, sharding, 4, 1024, 32, 32, query_route="fused")
    ConvE(True, sharding, 4, 1024, 32, 32)  # the torch route has no such limit
    ConvE(True, sharding, 4, 200, 10, 20, query_route="fused")  # the paper's shape


@pytest.mark.parametrize("route", ["torch", "fused"])
def test_all_entities_steps_accept_conve(route):
    fn = conve(route)
    OneVsAllBessKGE(PlaceholderNegativeSampler("t"), fn, SampledSoftmaxCrossEntropyLoss(N_ENT))
    known = [np.zeros((1, 3), dtype=np.int64)]
    KvsAllBessKGE(PlaceholderNegativeSampler("t"), fn, AllEntitiesBCELoss(N_ENT, label_smoothing=0.1), known)
    for make in (lambda: OneVsAllBessKGE(PlaceholderNegativeSampler("h"), fn, SampledSoftmaxCrossEntropyLoss(N_ENT)),
                 lambda: KvsAllBessKGE(PlaceholderNegativeSampler("h"), fn, AllEntitiesBCELoss(N_ENT), known)):
        with pytest.raises(NotImplementedError, match="ConvE should not be used with head corruption"):
            make()
