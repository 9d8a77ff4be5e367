"""`bess_relation_query_fwd / _bwd` (csrc/relation_query.hip) against a float64 gather + `einsum` + autograd on the CPU.

Bound.  Every output element is a sum of n products of two fp32 numbers (exact in the matrix cores' fp32 multiply-add),
accumulated by one chain of fp32 fused multiply-adds, one rounding per added term: to first order
|got - want| <= n 2^-24 sum |terms|, with

  q, d_x   n = de: the reduction runs over one axis of the relation's matrix (slices that are padded with zeros add
           exact zeros);
  d_M      n = the number of batch rows that name the element's relation: one workgroup walks the whole segment, so
           there is no merge of partial sums;

and c = 0 further roundings: no operand is scaled or converted on its way, nothing is merged.  The sum of absolute
terms is the same float64 computation on the operands' absolute values.  No measured constant enters."""

import functools

import pytest
import torch

from besskge import _native as nat

# (S, de, n_rel, pattern): "skewed" = relation ids drawn with probability ~ 1 / (1 + id)^2, "last" = every row in the
# highest relation, "own" = row i in relation n_rel - 1 - i
SHAPES = [(1, 4, 1, "last"), (33, 5, 3, "skewed"), (70, 36, 7, "skewed"), (130, 72, 3, "last"), (40, 72, 64, "own"),
          (257, 36, 2, "skewed"), (130, 200, 5, "skewed"), (40, 264, 2, "skewed")]
U = 2.0 ** -24


def product64(x, M, rel, dq, swap):
    x, M = (t.double().requires_grad_() for t in (x, M))
    q = torch.einsum("ib,iab->ia" if swap else "ia,iab->ib", x, M[rel.long()].view(-1, x.shape[1], x.shape[1]))
    return [q.detach(), *torch.autograd.grad(q, [x, M], dq.double())]


@functools.lru_cache(maxsize=None)
def case(S, de, n_rel, pattern, swap):
    gen = torch.Generator().manual_seed(1000 * S + de + n_rel + swap)
    x, M, dq = (torch.randn(s, generator=gen) for s in ((S, de), (n_rel, de * de), (S, de)))
    if pattern == "skewed":
        rel = torch.multinomial(1.0 / (1.0 + torch.arange(n_rel)) ** 2, S, replacement=True, generator=gen)
        rel[0] = n_rel - 1  # the highest id is used
    else:
        rel = torch.full((S,), n_rel - 1) if pattern == "last" else n_rel - 1 - torch.arange(S)
    rel = rel.to(torch.int32)
    want = product64(x, M, rel, dq, swap)
    terms = product64(x.abs(), M.abs(), rel, dq.abs(), swap)
    count = torch.bincount(rel.long(), minlength=n_rel).double().view(-1, 1)
    return (x, M, rel, dq), want, [de * U * terms[0], de * U * terms[1], count * U * terms[2]]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda", 0)


def padded(t, pad):  # `t` as a view of the leading columns of a buffer `pad` columns wider (filled with NaN)
    buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=t.dtype, device=t.device)
    buf[:, : t.shape[1]] = t
    return buf[:, : t.shape[1]]


def check(name, shape, got, again, want, bound):
    err = (got.double().cpu() - want).abs()
    print(f"{name} {shape}: largest error {float(err.max()):.3e}, largest error / bound "
          f"{float((err / bound.clamp_min(1e-300)).max()):.3e}")
    assert bool((err <= bound).all()), name
    assert torch.equal(got, again), f"{name} differs between two runs"


@pytest.mark.gpu
@pytest.mark.parametrize("swap", [0, 1])
@pytest.mark.parametrize("S,de,n_rel,pattern", SHAPES)
def test_products_against_float64(dev, S, de, n_rel, pattern, swap):
    ops, want, bound = case(S, de, n_rel, pattern, swap)
    x, M, rel, dq = (t.to(dev) for t in ops)
    seg = nat.SegmentIndex(rel, n_rel)
    got, again = ([nat.relation_query_fwd(x, M, seg, swap), *nat.relation_query_bwd(x, M, seg, swap, dq)] for _ in "ab")
    for name, g, g2, w, b in zip(("q", "d_x", "d_M"), got, again, want, bound):
        check(name, (S, de, n_rel, pattern, swap), g, g2, w, b)
    assert not bool(got[2][torch.bincount(rel.long(), minlength=n_rel) == 0].any()), "d_M of an absent relation"
    for keep in range(2):  # a NULL output skips its product and leaves the other as it was
        only = nat.relation_query_bwd(x, M, seg, swap, dq, want=[i == keep for i in range(2)])
        assert only[1 - keep] is None and torch.equal(only[keep], got[1 + keep])


@pytest.mark.gpu
@pytest.mark.parametrize("swap", [0, 1])
def test_padded_leading_dimensions(dev, swap):
    """Every operand and every output a view of a wider buffer; an odd pad takes the scalar-load class."""
    S, de, n_rel = 70, 36, 7
    ops, want, bound = case(S, de, n_rel, "skewed", swap)
    x, M, rel, dq = (t.to(dev) for t in ops)
    seg = nat.SegmentIndex(rel, n_rel)
    for pad in (4, 3):
        xp, Mp, dqp = (padded(t, pad) for t in (x, M, dq))
        outs = [padded(torch.empty_like(t), pad) for t in (x, x, M)]
        got = [nat.relation_query_fwd(xp, Mp, seg, swap, out=outs[0]),
               *nat.relation_query_bwd(xp, Mp, seg, swap, dqp, out=outs[1:])]
        for name, g, w, b in zip(("q", "d_x", "d_M"), got, want, bound):
            check(name, (S, de, n_rel, "pad", pad, swap), g, g, w, b)


@pytest.mark.gpu
def test_no_per_triple_matrix_is_allocated(dev):
    """Forward + backward at the paper's width allocate, beyond the d_M output, less than ONE [S, de, de] buffer."""
    S, de, n_rel = 130, 200, 5
    x, M, rel, dq = (t.to(dev) for t in case(S, de, n_rel, "skewed", 0)[0])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    seg = nat.SegmentIndex(rel, n_rel)
    q, (d_x, d_M) = nat.relation_query_fwd(x, M, seg, False), nat.relation_query_bwd(x, M, seg, False, dq)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated(dev) - before - d_M.numel() * 4
    print(f"peak allocation beyond d_M over index + forward + backward: {grown} bytes; [S, de, de] fp32: {S * de * de * 4}")
    assert grown < S * de * de * 4 and q.shape == d_x.shape == (S, de) and d_M.shape == M.shape
