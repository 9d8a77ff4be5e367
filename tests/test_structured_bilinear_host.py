"""Host-only: the constructor's refusals and the preset term tables of `scoring.StructuredBilinear`."""

import pytest

from besskge import scoring
from besskge.sharding import Sharding

SH = Sharding.create(40, 2, seed=0)


@pytest.mark.parametrize("terms, K, Kr, match", [
    ([(0, 0, 2, 1.0)], 2, 2, "outside"), ([(0, 2, 0, 1.0)], 2, 2, "outside"), ([(0, 0, 0, float("nan"))], 1, 1, "finite"),
    ([(0, 0, 0, float("inf"))], 1, 1, "finite"), ([(0, 0, 0, 1.0), (0, 0, 0, 2.0)], 1, 1, "twice"),
    ([(i % 8, i // 8 % 8, i // 64, 1.0) for i in range(65)], 8, 8, "64 terms"), ([], 1, 1, "64 terms"),
    ([(0, 0, 0, 1.0)], 9, 1, "blocks")])
def test_malformed_term_tables(terms, K, Kr, match):
    with pytest.raises(ValueError, match=match):
        scoring.StructuredBilinear(True, SH, 5, 6, terms, K, Kr)


def test_preset_tables():
    q = scoring.QuatE(True, SH, 5, 6)
    assert q.relation_unit_norm and tuple(q.entity_embedding.shape[-1:]) == (24,) and q.kernel_desc().rel_width == 24
    signs = {(i, j): (k, c) for i, j, k, c in q.terms}  # Hamilton: 1 i j k rows times 1 i j k columns
    assert signs == {(0, 0): (0, 1), (0, 1): (1, 1), (0, 2): (2, 1), (0, 3): (3, 1),
                     (1, 0): (1, 1), (1, 1): (0, -1), (1, 2): (3, 1), (1, 3): (2, -1),
                     (2, 0): (2, 1), (2, 1): (3, -1), (2, 2): (0, -1), (2, 3): (1, 1),
                     (3, 0): (3, 1), (3, 1): (2, 1), (3, 2): (1, -1), (3, 3): (0, -1)}
    assert scoring.SimplE(True, SH, 5, 6).terms == [(0, 0, 1, 0.5), (1, 1, 0, 0.5)]
    cp = scoring.CP(True, SH, 5, 6, inverse_relations=True)
    assert cp.terms == [(0, 0, 1, 1.0)] and tuple(cp.relation_embedding.shape) == (10, 6)
    an = scoring.ANALOGY(True, SH, 5, 8)
    assert an.block_size == 2 and an.terms == [(0, 0, 0, 1.0), (1, 1, 1, 1.0), (2, 2, 2, 1.0), (3, 3, 2, -1.0),
                                                (2, 3, 3, 1.0), (3, 2, 3, 1.0)]
    sf = scoring.StructuredBilinear.from_autosf(True, SH, 5, 6, [[1, 0], [0, -2]])
    assert sf.terms == [(0, 0, 0, 1.0), (1, 1, 1, -1.0)] and sf.n_relation_blocks == 2
