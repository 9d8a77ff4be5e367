"""Relation prediction, host side (no GPU): what the constructors take and refuse."""

import pytest

from besskge.loss import SampledSoftmaxCrossEntropyLoss
from besskge.negative_sampler import PlaceholderNegativeSampler
from besskge.one_vs_all import OneVsAllBessKGE
from besskge.scoring import RESCAL, ComplEx, ConvE, DistMult, RotatE, TransE, TuckER
from besskge.sharding import Sharding

N_ENT = 50


def scorers():
    sh = Sharding.create(N_ENT, 1, seed=0)
    return dict(TransE=lambda: TransE(True, 1, sh, 4, 8), RotatE=lambda: RotatE(True, 1, sh, 4, 8),
                TuckER=lambda: TuckER(True, sh, 4, 12, 5), RESCAL=lambda: RESCAL(True, sh, 4, 6),
                ConvE=lambda: ConvE(True, sh, 4, 36, 6, 6, inverse_relations=False),
                DistMult=lambda: DistMult(True, sh, 4, 8), ComplEx=lambda: ComplEx(True, sh, 4, 8))


def build(name, **kw):
    return OneVsAllBessKGE(PlaceholderNegativeSampler("t"), scorers()[name](), SampledSoftmaxCrossEntropyLoss(N_ENT), **kw)


@pytest.mark.parametrize("name", ["TransE", "RotatE", "TuckER", "RESCAL", "ConvE"])
def test_other_scorers_are_refused_by_name(name):
    assert build(name).relation_prediction_weight == 0.0  # (the scorer itself is fine for 1vsAll)
    with pytest.raises(ValueError, match="DistMult or ComplEx"):
        build(name, relation_prediction_weight=0.5)


def test_weight_default_and_sign():
    assert build("ComplEx").relation_prediction_weight == 0.0
    assert build("DistMult", relation_prediction_weight=0.25).relation_prediction_weight == 0.25
    for bad in (-0.5, float("nan")):
        with pytest.raises(ValueError, match="relation_prediction_weight"):
            build("ComplEx", relation_prediction_weight=bad)
