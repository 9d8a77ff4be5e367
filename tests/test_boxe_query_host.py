"""`scoring.BoxE(query_route=...)` and the host side of `bess_boxe_query_*` (csrc/boxe_query.hip): no device, no launch."""

import ctypes

import pytest
import torch

from besskge import _native as nat
from besskge.scoring import BoxE
from besskge.sharding import Sharding


def make(d, **kw):
    return BoxE(False, 2, Sharding.create(20, 1, seed=0), 3, d, **kw)


def desc(d, dtype=nat.F32, flags=3, p=2):
    m = nat.ModelDesc()
    m.scorer, m.norm_p, m.dtype, m.width, m.rel_width = nat.BOXE, p, dtype, 2 * d, 4 * d + 2
    m.reserved[0] = flags
    return m


def test_query_route_is_validated_and_defaults_to_torch():
    assert make(8).query_route == "torch"
    assert make(8, query_route="native").query_route == "native"
    with pytest.raises(ValueError, match="query_route"):
        make(8, query_route="fused")


@pytest.mark.parametrize("d", [516, 130])
def test_native_route_refuses_rows_the_kernels_do_not_take(d):
    with pytest.raises(ValueError, match="embedding_size"):
        make(d, query_route="native")
    assert make(d).query_route == "torch"  # the default route has no such limit


@pytest.mark.parametrize("d, S, n_rel, slots", [(256, 4096, 50, 50), (256, 4096, 1000, 129), (6, 31, 5, 1), (40, 64, 2, 2)])
def test_workspace_is_host_arithmetic(d, S, n_rel, slots):
    """min(n_rel, S / 32 + 1) slots of 16 shares of a relation row"""
    assert nat.boxe_query_workspace(desc(d), S, n_rel) == slots * 16 * (4 * d + 2) * 4
    nbytes = ctypes.c_int64(0)
    assert nat.load().bess_boxe_query_workspace(ctypes.byref(desc(516)), S, n_rel, ctypes.byref(nbytes)) == -2
    assert nat.load().bess_boxe_query_workspace(ctypes.byref(desc(d)), S, 0, ctypes.byref(nbytes)) == -1


def test_entry_points_check_their_operands_before_any_launch():
    lib, m = nat.load(), desc(8)
    fwd = lambda S, ent, q, eps=1e-6, side=nat.CORRUPT_TAIL, md=m: lib.bess_boxe_query_fwd(  # noqa: E731
        ctypes.byref(md), side, eps, ent, 16, 0, 0, 16, 0, 0, 34, 0, S, q, 48, 0, 0)
    bwd = lambda S, ent, md=m: lib.bess_boxe_query_bwd(  # noqa: E731
        ctypes.byref(md), nat.CORRUPT_TAIL, 1e-6, ent, 16, 0, 0, 16, 0, 0, 34, 3, 0, 0, 0, 0, 0, S, 0, 48, 0, 0, 16, 0, 16,
        0, 34, 0, 0, 0)
    assert fwd(0, 0, 0) == 0 and bwd(0, 0) == 0  # an empty batch is fine
    assert fwd(5, 0, 0) == -1 and bwd(5, 0) == -1  # NULL operands with rows to read
    assert fwd(0, 0, 0, eps=0.0) == -1 and fwd(0, 0, 0, side=7) == -1
    assert fwd(0, 0, 0, md=desc(130)) == -2 and bwd(0, 0, md=desc(516)) == -2
    wrong = desc(8)
    wrong.scorer = nat.TRANSE
    wrong.rel_width = 16
    assert fwd(0, 0, 0, md=wrong) == -1
