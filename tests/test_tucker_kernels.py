"""`bess_tucker_query_fwd / _bwd` (csrc/tucker.hip) against float64 `einsum` + autograd on the CPU.

Bound.  Every output element is a sum of n products of three fp32 numbers, accumulated by a chain of fp32
fused multiply-adds on the matrix cores (one rounding per added term: <= n 2^-24 sum |terms| to first order) plus c
further roundings of each term on its way:

  q, d_x   n = dr de    c = 1: `x * rel` (`dq * rel`) is rounded when the MFMA operand is formed on the LDS read.
  d_core   n = S        c = 1: the rows of x (dq) are scaled by rel[m, k] as they are staged.
  d_rel    n = de de    the inner sums over one core axis are chains of de <= n steps; c = 1 (the product with dq)
                        + 5 (the sum over a wave's 32 columns: 4 DPP steps and one exchange) + 2 ceil(de / 64) (the
                        fixed-order merge of one partial per 32-column wave tile).

so |got - want| <= (n + c) 2^-24 sum |terms|, the sum of absolute terms being the same einsum (and the same
autograd) on the operands' absolute values in float64.  No measured constant enters."""

import functools

import pytest
import torch

from besskge import _native as nat

SHAPES = [(1, 4, 1), (33, 5, 3), (70, 36, 7), (64, 128, 64), (130, 200, 30), (40, 264, 2),
          (33, 512, 2), (3, 544, 1)]  # 150,528 and 158,848 bytes of LDS: the widest de the entry points take
U = 2.0 ** -24


def product64(x, rel, core, dq, swap):
    """(q, d_x, d_rel, d_core) in float64 for dq"""
    ops = [t.double().requires_grad_() for t in (x, rel, core)]
    w = ops[2].view(rel.shape[1], x.shape[1], x.shape[1])
    q = torch.einsum("ik,ib,kab->ia" if swap else "ik,ia,kab->ib", ops[1], ops[0], w)
    return [q.detach(), *torch.autograd.grad(q, ops, dq.double())]


@functools.lru_cache(maxsize=None)
def case(S, de, dr, swap):
    gen = torch.Generator().manual_seed(1000 * S + de + dr + swap)
    x, rel, core, dq = (torch.randn(s, generator=gen) for s in ((S, de), (S, dr), (dr * de, de), (S, de)))
    want = product64(x, rel, core, dq, swap)
    terms = product64(x.abs(), rel.abs(), core.abs(), dq.abs(), swap)
    parts = 2 * ((de + 63) // 64)
    n_c = [dr * de + 1, dr * de + 1, de * de + 6 + parts, S + 1]
    return (x, rel, core, dq), want, [nc * U * t for nc, t in zip(n_c, terms)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("swap", [0, 1])
@pytest.mark.parametrize("S,de,dr", SHAPES)
def test_products_against_float64(dev, S, de, dr, swap):
    ops, want, bound = case(S, de, dr, swap)
    x, rel, core, dq = (t.to(dev) for t in ops)
    got = [nat.tucker_query_fwd(x, rel, core, swap), *nat.tucker_query_bwd(x, rel, core, swap, dq)]
    again = [nat.tucker_query_fwd(x, rel, core, swap), *nat.tucker_query_bwd(x, rel, core, swap, dq)]
    for name, g, g2, w, b in zip(("q", "d_x", "d_rel", "d_core"), got, again, want, bound):
        err = (g.double().cpu() - w).abs()
        print(f"{name} ({S}, {de}, {dr}) swap {swap}: largest error {float(err.max()):.3e}, "
              f"largest error / bound {float((err / b).max()):.3e}")
        assert bool((err <= b).all()), name
        assert torch.equal(g, g2), f"{name} differs between two runs"
    # a NULL output skips its product and leaves the others as they were
    for keep in range(3):
        only = nat.tucker_query_bwd(x, rel, core, swap, dq, want=[i == keep for i in range(3)])
        assert [o is None for o in only] == [i != keep for i in range(3)]
        assert torch.equal(only[keep], got[1 + keep])


@pytest.mark.gpu
def test_no_per_triple_matrix_is_allocated(dev):
    """Forward + backward at the paper's widths allocate less than ONE [S, de, de] buffer (20.8 MB here) - the
    outputs are under 1 MB, the workspace is S dr 8 floats."""
    S, de, dr = 130, 200, 30
    x, rel, core, dq = (t.to(dev) for t in case(S, de, dr, 0)[0])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    q = nat.tucker_query_fwd(x, rel, core, False)
    grads = nat.tucker_query_bwd(x, rel, core, False, dq)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated(dev) - before
    print(f"peak allocation over forward + backward: {grown} bytes; [S, de, de] fp32: {S * de * de * 4}")
    assert grown < S * de * de * 4
    assert q.shape == (S, de) and grads[2].shape == core.shape
