"""HAKE's candidate kernels (csrc/hake.hip) against the scorer's formula in float64 torch, on the values as stored.

Tolerance: the same formula evaluated in float32 torch on the CPU deviates from float64 by some largest amount over
the inputs of a (d, table type) set; the kernel is allowed 4 x that (another summation order, and the three extra
roundings per element of the sine-difference identity of the tile form).  The set is the 65 x 129 problem and the
smaller shapes are its sub-blocks.  Scores and per-reference gradients are elementwise in (query, candidate): their
deviation is taken over the whole set.  A gradient that sums over k candidates (or queries) is held to the deviation
of that sum over k, taken over all 65 queries (all 129 candidates) of the set, not only the block's few.  Counts
against ranks of stored scores, and pairs against stored scores, share their arithmetic and are compared bitwise.
"""
import functools

import pytest
import torch

from besskge import _native as nat
from besskge._native import RowSource

pytestmark = pytest.mark.gpu

F32, F16, F64 = torch.float32, torch.float16, torch.float64
DS = [5, 16, 40, 130]
M, S, N = 150, 65, 129  # table rows; the full problem: one past each tile edge, two (three) column tiles
LP, PS = 0.5, 1.0

sets = pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
widths = pytest.mark.parametrize("d", DS)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda", 0)


def hake_desc(table, row_form=False, lp=LP, ps=PS):
    d = nat.make_desc(nat.HAKE, 2, table, int(table.shape[1]) // 2 * 3)
    d.reserved[0] = nat.FLAG_FP32_MATH if row_form else 0
    d.reserved[1], d.reserved[2] = (int(torch.tensor(v, dtype=F32).view(torch.int32)) for v in (lp, ps))
    return d


def rule(q, rows, dtype, lp=LP, ps=PS):
    """scores of q [S, 3 d] against rows [S, n, 2 d] (or [n, 2 d]: shared), in `dtype`"""
    u, r, qp = q.to(dtype).unsqueeze(1).chunk(3, dim=-1)
    cp, cm = rows.to(dtype).chunk(2, dim=-1)
    return -(torch.norm(u * cm + r, dim=-1) + lp * torch.sin((qp - ps * cp) / 2).abs().sum(-1))


def with_grads(q, rows, g, dtype):
    """(scores, d_query, d_rows) of `rule` in `dtype`, as float64"""
    q, rows = (x.to(dtype).clone().requires_grad_(True) for x in (q, rows))
    sc = rule(q, rows, dtype)
    sc.backward(g.to(dtype))
    return tuple(x.detach().double() for x in (sc, q.grad, rows.grad))


@functools.lru_cache(maxsize=None)
def case(d, dtype):
    """Inputs of one (d, table type) set: table, queries, one shared and one per-query candidate list, score gradients."""
    gen = torch.Generator().manual_seed(7000 + d)
    table = torch.cat([(torch.rand(M, d, generator=gen) * 2 - 1) * 3.14, torch.randn(M, d, generator=gen)], -1).to(dtype)
    q = torch.cat([torch.randn(S, 2 * d, generator=gen), (torch.rand(S, d, generator=gen) * 2 - 1) * 3.14], -1)
    shared = torch.randint(M, (N,), generator=gen, dtype=torch.int32)
    shared[5] = shared[70]  # (repeated rows)
    own = torch.randint(M, (S, N), generator=gen, dtype=torch.int32)
    own[:, 3] = own[:, 0]
    g = torch.randn(S, N, generator=gen)
    c = dict(table=table, q=q, shared=shared, own=own, g=g)
    c["rows"] = dict(shared=table.float()[shared.long()], own=table.float()[own.long()])
    return c


@functools.lru_cache(maxsize=None)
def block(d, dtype, layout, ns, nn):
    """(float64 results, 4 x the float32 deviations) of queries [:ns] against candidates [:nn] of the set"""
    c = case(d, dtype)
    rows = c["rows"][layout][:nn] if layout == "shared" else c["rows"][layout][:ns, :nn]
    args = (c["q"][:ns], rows, c["g"][:ns, :nn])
    want = with_grads(*args, F64)
    return want, [4 * float((a - b).abs().max()) for a, b in zip(want, with_grads(*args, F32))]


def within(got, want, tol, what):
    err = float((got.detach().cpu().double() - want).abs().max())
    print(f"{what}: error {err:.3e}, allowed {tol:.3e} (4 x the float32 deviation)")
    assert err <= tol, what


@widths
@sets
@pytest.mark.parametrize("nq,nn", [(1, 1), (7, 5), (3, 70), (S, N)])
def test_pertriple_forward_and_backward(dev, dtype, d, nq, nn):
    c = case(d, dtype)
    want = block(d, dtype, "own", nq, nn)[0]
    tol = block(d, dtype, "own", S, N)[1]
    tb, q, g = c["table"].to(dev), c["q"][:nq].to(dev), c["g"][:nq, :nn].contiguous().to(dev)
    idx = c["own"][:nq, :nn].reshape(-1).contiguous().to(dev)
    desc = hake_desc(tb)
    out = nat.neg_score_pertriple_fwd(desc, q, RowSource(tb, idx), nn)
    within(out, want[0], tol[0], "scores")
    dq, dn = nat.neg_score_pertriple_bwd(desc, q, RowSource(tb, idx), nn, g)
    within(dq, want[1], block(d, dtype, "own", S, nn)[1][1], "d_query")
    within(dn.reshape(nq, nn, 2 * d), want[2], tol[2], "d_neg")


@sets
def test_pertriple_d_neg_by_row(dev, dtype, d=40):
    """every row named once: the gradient rows land at their table rows"""
    c = case(d, dtype)
    nq, nn = 7, 5
    tb, q, g = c["table"].to(dev), c["q"][:nq].to(dev), c["g"][:nq, :nn].contiguous().to(dev)
    idx = torch.randperm(M, generator=torch.Generator().manual_seed(1))[: nq * nn].to(torch.int32)
    _, dn = nat.neg_score_pertriple_bwd(hake_desc(tb), q, RowSource(tb, idx.to(dev)), nn, g)
    by_row = torch.zeros(M, 2 * d, device=dev)
    nat.neg_score_pertriple_bwd(hake_desc(tb), q, RowSource(tb, idx.to(dev)), nn, g, d_neg_rows=by_row)
    assert torch.equal(by_row[idx.long().to(dev)], dn)


@widths
@sets
@pytest.mark.parametrize("row_form", [False, True], ids=["tile", "rows"])
@pytest.mark.parametrize("ns,nn", [(1, 1), (S, N)])
def test_shared_forward_counts_pairs(dev, dtype, d, row_form, ns, nn):
    c = case(d, dtype)
    tb, q, idx = c["table"].to(dev), c["q"][:ns].to(dev), c["shared"][:nn].to(dev)
    desc, src = hake_desc(tb, row_form), RowSource(tb, idx)
    out = nat.neg_score_shared_fwd(desc, q, src)
    within(out, block(d, dtype, "shared", ns, nn)[0][0], block(d, dtype, "shared", S, N)[1][0], "scores")
    # ranks counted in the epilogue == ranks of the stored scores, with the true completion left out
    excl = (torch.arange(ns, dtype=torch.int32) * 7 % nn).to(dev)
    excl[::3] = -1
    pair_idx = idx[(torch.arange(ns) * 7 % nn).to(dev)]
    thr = nat.neg_score_shared_pairs(desc, q, RowSource(tb, pair_idx), ns, nn)
    assert torch.equal(thr, out[torch.arange(ns), (torch.arange(ns) * 7 % nn)])
    counts = nat.neg_score_shared_counts(desc, q, src, thr, excl)
    keep = torch.arange(nn, device=dev)[None, :] != excl[:, None]
    above = ((out > thr[:, None]) & keep).sum(1)
    equal = ((out == thr[:, None]) & keep).sum(1)
    assert torch.equal(counts.long(), torch.stack([above, equal], 1))


def test_counting_walk_and_chunks(dev, d=5):
    """Enough candidates (indices into the small table: many exact ties) for a workgroup to walk 8 column tiles and for
    a second 32 MiB chunk of rows, whose columns start at col0 != 0; `excl` in both chunks and on their edges."""
    c = case(d, F32)
    tb, q = c["table"].to(dev), c["q"].to(dev)
    chunk = (32 << 20) // (2 * d * 4) // 64 * 64
    nn = chunk + 200
    idx = (torch.arange(nn, dtype=torch.int64) * 37 % M).to(torch.int32).to(dev)
    desc, src = hake_desc(tb), RowSource(tb, idx)
    out = nat.neg_score_shared_fwd(desc, q, src)
    where = torch.tensor([0, 63, 64, 511, 512, chunk - 1, chunk, chunk + 199, -1], device=dev)
    excl = where[torch.arange(S, device=dev) % len(where)].to(torch.int32)
    thr = out[torch.arange(S), (torch.arange(S) * 12345 % nn)].contiguous()
    counts = nat.neg_score_shared_counts(desc, q, src, thr, excl)
    keep = torch.arange(nn, device=dev)[None, :] != excl[:, None]
    want = torch.stack([((out > thr[:, None]) & keep).sum(1), ((out == thr[:, None]) & keep).sum(1)], 1)
    assert int(want[:, 1].max()) > 1 and torch.equal(counts.long(), want)


@widths
@sets
@pytest.mark.parametrize("row_form", [False, True], ids=["tile", "rows"])
@pytest.mark.parametrize("ns,nn", [(1, 1), (S, N)])
def test_shared_backward(dev, dtype, d, row_form, ns, nn):
    c = case(d, dtype)
    tb, q, idx = c["table"].to(dev), c["q"][:ns].to(dev), c["shared"][:nn].to(dev)
    desc, src = hake_desc(tb, row_form), RowSource(tb, idx)
    out = nat.neg_score_shared_fwd(desc, q, src)
    dq, dn = nat.neg_score_shared_bwd(desc, q, src, out, c["g"][:ns, :nn].contiguous().to(dev))
    want = block(d, dtype, "shared", ns, nn)[0]
    within(dq, want[1], block(d, dtype, "shared", S, nn)[1][1], "d_query")
    within(dn, want[2], block(d, dtype, "shared", ns, N)[1][2], "d_neg")


@widths
@sets
def test_segment_gradient(dev, dtype, d):
    """own-shard negatives: per-row sums of d_neg, one row referenced more than SEGMENT_CAP times (the long tier)"""
    c = case(d, dtype)
    nq, nn = 40, 9
    tb, q, g = c["table"].to(dev), c["q"][:nq].to(dev), c["g"][:nq, :nn].contiguous().to(dev)
    own = c["own"][:nq, :nn].clone()
    own[:30] = 41
    idx = own.reshape(-1).contiguous()
    assert int((idx == 41).sum()) > nat.SEGMENT_CAP
    rows = c["table"].float()[own.long()]  # (the hot row changes the inputs: this shape's own deviation)
    dn64, dn32 = (with_grads(c["q"][:nq], rows, c["g"][:nq, :nn], t)[2].reshape(-1, 2 * d) for t in (F64, F32))
    # (the float32 restatement sums its float32 terms in float32 too)
    want, low = (torch.zeros(M, 2 * d, dtype=t).index_add_(0, idx.long(), x.to(t)).double()
                 for x, t in ((dn64, F64), (dn32, F32)))
    seg = nat.SegmentIndex(idx.to(dev), M, width=2 * d)
    assert int(seg.long_segs[0].item()) == 1
    n_seg = int(seg.n_seg.item())
    got = nat.neg_pertriple_grad_segments(hake_desc(tb), q, tb, nn, g, seg)
    uniq = seg.seg_rows[:n_seg].long().cpu()
    within(got[:n_seg], want[uniq], 4 * float((want - low).abs().max()), "segment sums")


@pytest.mark.parametrize("kink", ["phase", "modulus"])
def test_kink_conventions(dev, kink, d=16):
    """candidate phase == query phase: sin = 0 has gradient 0; U c + R = 0: the zero norm has gradient 0"""
    gen = torch.Generator().manual_seed(3)
    tb = torch.randn(4, 2 * d, generator=gen)
    q = torch.randn(4, 3 * d, generator=gen)
    if kink == "phase":
        q[:, 2 * d:] = tb[:, :d]
    else:
        q[:, :d], q[:, d: 2 * d] = 1.0, -tb[:, d:]
    idx = torch.arange(4, dtype=torch.int32)
    dq, dn = nat.neg_score_pertriple_bwd(hake_desc(tb), q.to(dev), RowSource(tb.to(dev), idx.to(dev)), 1,
                                         torch.ones(4, 1, device=dev))
    part = slice(2 * d, None) if kink == "phase" else slice(0, 2 * d)
    assert not dq[:, part].any() and not (dn[:, :d] if kink == "phase" else dn[:, d:]).any()
    assert dq.isfinite().all() and dn.isfinite().all()
