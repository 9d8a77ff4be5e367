"""`bess_struct_query_fwd / _bwd` (csrc/struct_query.hip) against the score formula in float64 on the CPU, gradients by
autograd; fp16 cases from the fp16 values upcast.  Bounds, u = 2^-24, on float64 sums of absolute terms, none measured:
  q      a chain of T fused multiply-adds (T terms reach the block) of products rounded once: (T + 3) u sum |c e r|;
         unit norm: Kr <= 4 roundings in the sum of squares, halved by the root, the root, the quotient: + 4
  pos    the dot product with the other row over W columns: + W;   d_ent: the query gradient rounded once: + 1;
         d_other = d_pos * q: + 1
  d_rel  a segment of L triples: (L + T + 3) u; through the norm's Jacobian + Kr + 4 on (|g| + |r^| <|g|, |r^|>) / n"""

import ctypes
import functools

import pytest
import torch

from besskge import _native as nat

pytestmark = pytest.mark.gpu
U = 2.0 ** -24

QUAT = [(i, j, k, c) for i, row in enumerate([[(0, 1), (1, 1), (2, 1), (3, 1)], [(1, 1), (0, -1), (3, 1), (2, -1)],
                                              [(2, 1), (3, -1), (0, -1), (1, 1)], [(3, 1), (2, 1), (1, -1), (0, -1)]])
        for j, (k, c) in enumerate(row)]  # h_i r_j enters component k of the Hamilton product h (x) r with sign c
_gen = torch.Generator().manual_seed(64)
TABLES = {  # name -> (K, Kr, terms, relation_unit_norm)
    "distmult": (1, 1, [(0, 0, 0, 1.0)], False),
    "complex": (2, 2, [(0, 0, 0, 1.0), (1, 1, 0, -1.0), (0, 1, 1, 1.0), (1, 0, 1, 1.0)], False),
    "quate": (4, 4, QUAT, False),
    "quate_norm": (4, 4, QUAT, True),
    "cp": (2, 1, [(0, 0, 1, 1.0)], False),
    "rand64": (8, 8, [(n // 64, n // 8 % 8, n % 8, float(c)) for n, c in
                      zip(torch.randperm(512, generator=_gen)[:64].tolist(), torch.randn(64, generator=_gen))], False),
}
# (table, d, S, relations, side, dtype, fused positive, dense rows)
CASES = [("distmult", 1, 1, "rand7", nat.CORRUPT_TAIL, torch.float32, False, False),
         ("distmult", 260, 70, "sparse400", nat.CORRUPT_HEAD, torch.float16, True, True),
         ("complex", 3, 5, "rand7", nat.CORRUPT_HEAD, torch.float32, True, False),
         ("complex", 64, 300, "one", nat.CORRUPT_TAIL, torch.float16, False, True),
         ("quate", 64, 300, "one", nat.CORRUPT_TAIL, torch.float32, True, False),
         ("quate", 5, 70, "sparse400", nat.CORRUPT_HEAD, torch.float32, False, True),
         ("quate", 1, 5, "rand7", nat.CORRUPT_TAIL, torch.float16, True, False),
         ("quate_norm", 64, 70, "rand7", nat.CORRUPT_TAIL, torch.float32, True, True),
         ("quate_norm", 260, 300, "one", nat.CORRUPT_HEAD, torch.float32, True, False),
         ("quate_norm", 3, 5, "rand7", nat.CORRUPT_TAIL, torch.float16, False, False),
         ("cp", 5, 300, "rand7", nat.CORRUPT_TAIL, torch.float32, True, True),
         ("cp", 64, 1, "rand7", nat.CORRUPT_HEAD, torch.float16, True, False),
         ("rand64", 64, 70, "rand7", nat.CORRUPT_TAIL, torch.float32, True, False),
         ("rand64", 5, 300, "one", nat.CORRUPT_HEAD, torch.float16, False, True),
         ("rand64", 260, 70, "sparse400", nat.CORRUPT_TAIL, torch.float32, True, False)]


def query64(terms, K, d, side, e, r):
    """q [S, K d] from the score formula: e, r [S, blocks, d] float64 (r already normalised)."""
    q = [0.0] * K
    for i, j, k, c in terms:
        a, o = (i, k) if side == nat.CORRUPT_TAIL else (k, i)
        q[o] = q[o] + c * e[:, a] * r[:, j]
    return torch.stack([x + torch.zeros_like(e[:, 0]) for x in q], 1).flatten(1)


def outputs64(terms, K, Kr, d, side, norm, ent, oth, rel, ridx, dq, dpos):
    """[q, pos, d_ent, d_other, d_rel] in float64 (dpos None: no positive score, pos and d_other are None)."""
    ent, oth, rel = (t.double().requires_grad_() for t in (ent, oth, rel))
    r = rel[ridx.long()].view(-1, Kr, d)
    if norm:
        r = r / r.pow(2).sum(1, keepdim=True).sqrt()
    q = query64(terms, K, d, side, ent.view(-1, K, d), r)
    loss = (q * dq.double()).sum()
    pos = None
    if dpos is not None:
        pos = (q * oth).sum(-1)
        loss = loss + (pos * dpos.double()).sum()
    g = torch.autograd.grad(loss, [ent, oth, rel], allow_unused=True)
    return [q.detach(), None if pos is None else pos.detach(), g[0], g[1] if dpos is not None else None, g[2]]


@functools.lru_cache(maxsize=None)
def case(name, d, S, rels, side, dtype, fused):
    K, Kr, terms, norm = TABLES[name]
    gen = torch.Generator().manual_seed(1000 * S + d + len(terms))
    n_rel = {"one": 1, "sparse400": 400, "rand7": 7}[rels]
    n_ent = 50
    table, rel = torch.randn(n_ent, K * d, generator=gen), torch.randn(n_rel, Kr * d, generator=gen)
    rel[:, :d] = torch.sign(rel[:, :d]) * (rel[:, :d].abs() + 0.1)  # per-column block norms >= 0.1
    table, rel = table.to(dtype), rel.to(dtype)
    eidx, oidx = (torch.randint(0, n_ent, (S,), generator=gen, dtype=torch.int32) for _ in range(2))
    ridx = torch.randint(0, n_rel, (S,), generator=gen, dtype=torch.int32)
    dq, dpos = torch.randn(S, K * d, generator=gen), (torch.randn(S, generator=gen) if fused else None)
    ent, oth = table[eidx.long()], table[oidx.long()]
    want = outputs64(terms, K, Kr, d, side, norm, ent, oth, rel, ridx, dq, dpos)
    # sums of absolute terms: the same computation on absolute values, the relation rows normalised beforehand
    r64 = rel.double().view(n_rel, Kr, d)
    rn = r64.pow(2).sum(1, keepdim=True).sqrt() if norm else torch.ones(n_rel, 1, d, dtype=torch.float64)
    rhat = (r64 / rn).abs().flatten(1)
    absolute = outputs64([(i, j, k, abs(c)) for i, j, k, c in terms], K, Kr, d, side, False, ent.abs(), oth.abs(), rhat,
                         ridx, dq.abs(), None if dpos is None else dpos.abs())
    kept, out = (0, 2) if side == nat.CORRUPT_TAIL else (2, 0)
    n_to = lambda pos, blocks: torch.tensor([sum(t[pos] == b for t in terms) for b in range(blocks)],  # noqa: E731
                                            dtype=torch.float64).repeat_interleave(d)
    extra = 4 if norm else 0
    L = torch.bincount(ridx.long(), minlength=n_rel).double().view(-1, 1)
    g_abs = absolute[4].view(n_rel, Kr, d)
    rel_abs = ((g_abs + rhat.view(n_rel, Kr, d) * (g_abs * rhat.view(n_rel, Kr, d)).sum(1, keepdim=True)) / rn).flatten(1)
    bounds = [(n_to(out, K) + 3 + extra) * U * absolute[0],
              None if dpos is None else (len(terms) + 3 + extra + K * d) * U * absolute[1],
              (n_to(kept, K) + 4 + extra) * U * absolute[2],
              None if dpos is None else (n_to(out, K) + 4 + extra) * U * absolute[3],
              (L + n_to(1, Kr) + 3 + (Kr + 4 if norm else 0)) * U * rel_abs]
    return (K, Kr, terms, norm, table, rel, eidx, oidx, ridx, dq, dpos), want, bounds


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda", 0)


def padded(t, pad=4):  # `t` as a view of the leading columns of a NaN-filled buffer `pad` columns wider
    buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=t.dtype, device=t.device)
    buf[:, : t.shape[1]] = t
    return buf[:, : t.shape[1]]


def operands(c, dev, dense):
    K, Kr, terms, norm, table, rel, eidx, oidx, ridx, dq, dpos = c
    table, rel, eidx, oidx, ridx, dq = (t.to(dev) for t in (table, rel, eidx, oidx, ridx, dq))
    dpos = None if dpos is None else dpos.to(dev)
    if dense:
        ent, oth = nat.RowSource(padded(table[eidx.long()])), nat.RowSource(padded(table[oidx.long()]))
        rel, dq = padded(rel), padded(dq)
    else:
        ent, oth = nat.RowSource(table, eidx), nat.RowSource(table, oidx)
    desc = nat.struct_desc(table, K, Kr, rel.shape[1] // Kr, terms, norm)
    return desc, ent, (oth if dpos is not None else None), rel, ridx, dq, dpos


def check(got, want, bound, what):
    err = (got.double().cpu() - want).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    print(f"{what}: largest error / bound = {worst:.3f}")
    assert (err <= bound).all(), (what, worst)


@pytest.mark.parametrize("name, d, S, rels, side, dtype, fused, dense", CASES)
def test_forward(dev, name, d, S, rels, side, dtype, fused, dense):
    c, want, bounds = case(name, d, S, rels, side, dtype, fused)
    desc, ent, oth, rel, ridx, dq, dpos = operands(c, dev, dense)
    out = padded(torch.empty(S, want[0].shape[1], device=dev)) if dense else None
    q, pos = nat.struct_query_fwd(desc, side, ent, rel, ridx, other=oth, out=out)
    check(q, want[0], bounds[0], "q")
    if dense:
        assert torch.isnan(out._base[:, want[0].shape[1]:]).all()  # nothing written beside the view
    again = nat.struct_query_fwd(desc, side, ent, rel, ridx, other=oth)
    assert torch.equal(again[0], q)
    if fused:
        check(pos, want[1], bounds[1], "pos")
        assert torch.equal(again[1], pos)
        assert torch.equal(nat.struct_query_fwd(desc, side, ent, rel, ridx)[0], q)  # a NULL pos_out leaves q as it is


@pytest.mark.parametrize("name, d, S, rels, side, dtype, fused, dense", CASES)
def test_backward(dev, name, d, S, rels, side, dtype, fused, dense):
    c, want, bounds = case(name, d, S, rels, side, dtype, fused)
    desc, ent, oth, rel, ridx, dq, dpos = operands(c, dev, dense)

    def run():
        d_rel = torch.zeros(rel.shape, dtype=torch.float32, device=dev)
        return (*nat.struct_query_bwd(desc, side, ent, rel, ridx, dq, d_rel, other=oth, d_pos=dpos), d_rel)

    got = run()
    check(got[0], want[2], bounds[2], "d_ent")
    if fused:
        check(got[1], want[3], bounds[3], "d_other")
    check(got[2], want[4], bounds[4], "d_rel")
    for a, b in zip(got, run()):
        assert (a is None and b is None) or torch.equal(a, b)


def test_refusals(dev):
    """Past the documented limits: BESS_EUNSUPPORTED before any launch, outputs untouched."""
    table, rel = torch.randn(4, 9 * 4, device=dev), torch.randn(2, 4, device=dev)
    idx, q = torch.zeros(3, dtype=torch.int32, device=dev), torch.full((3, 36), float("nan"), device=dev)
    desc = nat.struct_desc(table, 9, 1, 4, [(0, 0, 0, 1.0)])
    nbytes = ctypes.c_int64(0)
    assert nat.load().bess_struct_query_workspace(ctypes.byref(desc), 3, 2, ctypes.byref(nbytes)) == -2
    with pytest.raises(RuntimeError, match="at most 8 entity / relation blocks and 64 terms"):
        nat.struct_query_fwd(desc, nat.CORRUPT_TAIL, nat.RowSource(table, idx), rel, idx, out=q)
    d_rel = torch.full((2, 4), float("nan"), device=dev)
    with pytest.raises(RuntimeError, match="at most 8"):
        nat.struct_query_bwd(desc, nat.CORRUPT_TAIL, nat.RowSource(table, idx), rel, idx, q, d_rel)
    torch.cuda.synchronize()
    assert torch.isnan(q).all() and torch.isnan(d_rel).all()
    desc = nat.struct_desc(table[:, :4], 1, 1, 4, [(0, 0, 0, 1.0)])
    desc.n_terms = 65
    assert nat.load().bess_struct_query_workspace(ctypes.byref(desc), 3, 2, ctypes.byref(nbytes)) == -2
