"""TuckER without a GPU: the scorer's parameters, and the C entry points' refusals (nothing is launched)."""

import ctypes

import torch

from besskge import _native as nat
from besskge.scoring import TuckER
from besskge.sharding import Sharding


def test_parameters_and_dense_list():
    sharding = Sharding.create(50, 2, seed=0)
    fn = TuckER(True, sharding, 4, 12, 5, inverse_relations=True)
    assert tuple(fn.entity_embedding.shape) == (2, sharding.max_entity_per_shard, 12)
    assert tuple(fn.relation_embedding.shape) == (8, 5)
    assert tuple(fn.core.shape) == (5 * 12, 12) and fn.core.dtype == torch.float32
    assert float(fn.core.detach().abs().max()) <= 1.0
    assert [p is q for p, q in zip(fn.dense_parameters(), [fn.core])] == [True]
    d = fn.kernel_desc()
    assert (d.scorer, d.width, d.rel_width) == (nat.DISTMULT, 12, 12)
    bn = TuckER(True, sharding, 4, 12, 5, batch_normalization=True, input_dropout=0.2, hidden_dropout=0.3)
    dense = bn.dense_parameters()
    assert dense[0] is bn.core and [tuple(p.shape) for p in dense[1:]] == [(12,)] * 4
    assert set(dict(bn.named_parameters())) >= {"core", "input_layers.0.weight", "hidden_layers.0.bias"}


def test_entry_points_refuse_without_a_launch():
    lib = nat.load()
    nbytes = ctypes.c_int64(-1)
    assert lib.bess_tucker_query_workspace(4096, 200, 200, ctypes.byref(nbytes)) == 0
    assert 0 < nbytes.value < 64 << 20 and nbytes.value == 8 * 4 * 4096 * 200
    assert lib.bess_tucker_query_workspace(4096, 200, 200, None) == -1
    assert lib.bess_tucker_query_workspace(-1, 200, 200, ctypes.byref(nbytes)) == -1
    assert lib.bess_tucker_query_workspace(8, 545, 2, ctypes.byref(nbytes)) == -2  # BESS_EUNSUPPORTED: de above 544
    p = 256  # (never dereferenced: every call below is refused before a launch)
    assert lib.bess_tucker_query_fwd(0, 8, p, 2, p, 0, p, 8, 4, 8, 2, 0, 0, 0) == -1  # NULL x
    assert lib.bess_tucker_query_fwd(p, 8, p, 2, p, 0, p, 8, 4, 0, 2, 0, 0, 0) == -1  # de = 0
    assert lib.bess_tucker_query_fwd(p, 8, p, 2, p, 2, p, 8, 4, 8, 2, 0, 0, 0) == -1  # swap_axes = 2
    assert lib.bess_tucker_query_fwd(p, 4, p, 2, p, 0, p, 8, 4, 8, 2, 0, 0, 0) == -1  # ldx < de
    assert lib.bess_tucker_query_bwd(p, 8, p, 2, p, 0, 0, 8, p, 8, p, 2, p, 4, 8, 2, p, 1 << 20, 0) == -1  # NULL dq
    assert lib.bess_tucker_query_bwd(p, 8, p, 2, p, 0, p, 8, p, 8, p, 2, p, -4, 8, 2, p, 1 << 20, 0) == -1  # S < 0
    assert lib.bess_tucker_query_workspace(4, 8, 2, ctypes.byref(nbytes)) == 0
    assert lib.bess_tucker_query_bwd(p, 8, p, 2, p, 0, p, 8, p, 8, p, 2, p, 4, 8, 2, p, nbytes.value - 1, 0) == -1
    buf = ctypes.create_string_buffer(256)
    lib.bess_last_error(buf, 256)
    assert "workspace too small" in buf.value.decode()
    assert lib.bess_tucker_query_fwd(0, 8, 0, 2, 0, 0, 0, 8, 0, 8, 2, 0, 0, 0) == 0  # S = 0: nothing to do
