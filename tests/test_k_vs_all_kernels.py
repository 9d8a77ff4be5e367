"""`bess_neg_score_shared_fwd_bce` / `bess_label_score_sums` / `bess_neg_score_shared_bwd_bce` (csrc/neg_shared.hip,
the BCE epilogue of csrc/gemm_split.hip) against float64 `BCEWithLogits` on a DENSE label matrix built from the
ragged labels, autograd supplying the gradients.

Forward tolerances, per row, with delta = W * 2^-24 * max(1, max|s|) (a score is a chain of W fp32 operations on
terms of magnitude <= max|s|, as in tests/test_one_vs_all_kernels.py) and L the depth of the summation tree that is
implemented (`merge_depth` of that file: the sums of this pass take the places of its merges):
    |A - A64| <= n_neg * delta + (L + 2) * 2^-24 * A64        A = sum_j softplus(s_j)
    |B - B64| <= n_neg * delta + L * 2^-24 * sum_j |s_j|      B = sum_j s_j
    |C - C64| <= len_row * (delta + 2^-24 * sum |s_labelled|) C = sum over the row's labels, a chain of len_row terms
softplus is 1-Lipschitz, so a score's error enters A at most once (n_neg * delta); all terms of A are positive, so
every level of the tree and the two roundings of a softplus (exp, log) cost 2^-24 of A at most.
Gradients: the fp32 paths hold the project's shared-negative tolerance (rtol 1e-4, atol 1e-5); on the split-fp16 path
`SPLIT_BCE_GRAD_MEASURED` is the largest deviation from float64 relative to the row's largest |gradient element|
measured on the MI355X over `test_fused_epilogue`, and the test holds 4 x that (the margin of SPLIT_GRAD_MEASURED)."""

import ctypes

import pytest
import torch

from test_one_vs_all_kernels import (FUSED_CASES, TILE_CASES, dev, fused_problems, grad_deviation, make_desc,  # noqa: F401
                                     merge_depth, problem, ref_scores)

EPS24 = 2.0 ** -24
SMOOTH, PW = 0.1 / 333, 0.9
#: largest |gradient - float64| / max |row of the float64 gradient| on the MI355X (see the module docstring)
SPLIT_BCE_GRAD_MEASURED = 6.08e-6  # (d_query, ComplEx fp16 table, 512 x 8229; d_neg at most 1.9e-6)


def make_labels(nq, n_neg, seed, full_row=None):
    """(ptr int64 [nq + 1], col int32, dense float64 [nq, n_neg]): 0-7 labels per row, every fifth row empty, in no
    order; `full_row` gets the columns listed for it"""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for q in range(nq):
        k = 0 if q % 5 == 4 else int(torch.randint(0, 8, (1,), generator=g))
        rows.append(torch.randperm(n_neg, generator=g)[:k])
    if full_row is not None:
        rows[full_row[0]] = torch.tensor(full_row[1])
    ptr = torch.zeros(nq + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(torch.tensor([len(r) for r in rows]), 0)
    dense = torch.zeros(nq, n_neg, dtype=torch.float64)
    for q, r in enumerate(rows):
        dense[q, r] = 1.0
    return ptr, torch.cat(rows).to(torch.int32), dense


def reference(name, p, query, rows, dense, coef):
    """float64 (scores, d_query, d_rows) of sum_q coef_q sum_j BCEWithLogits(s_qj, PW * dense + SMOOTH)"""
    q = query.double().clone().requires_grad_(True)
    e = rows.double().clone().requires_grad_(True)
    s = ref_scores(name, p, q, e)
    bce = torch.nn.functional.binary_cross_entropy_with_logits(s, PW * dense + SMOOTH, reduction="none")
    (coef.double() * bce.sum(dim=1)).sum().backward()
    return s.detach(), q.grad, e.grad


def check_ab(state, s, depth, W, what, base=None):
    n_neg = s.shape[1]
    delta = W * EPS24 * max(1.0, float(s.abs().max()))
    a64, b64, mag = torch.nn.functional.softplus(s).sum(1), s.sum(1), s.abs().sum(1)
    if base is not None:  # (a state accumulated earlier: one more addition)
        a64, b64, mag, depth = a64 + base[:, 0], b64 + base[:, 1], mag + base[:, 1].abs(), depth + 1
    err_a = (state[:, 0].double().cpu() - a64).abs() - (n_neg * delta + (depth + 2) * EPS24 * a64)
    err_b = (state[:, 1].double().cpu() - b64).abs() - (n_neg * delta + depth * EPS24 * mag)
    print(f"{what}: max(|A err| - bound) {float(err_a.max()):.3e}  max(|B err| - bound) {float(err_b.max()):.3e}  "
          f"(|A err| {float((state[:, 0].double().cpu() - a64).abs().max()):.3e}, "
          f"|B err| {float((state[:, 1].double().cpu() - b64).abs().max()):.3e}, delta {delta:.3e})")
    assert torch.isfinite(state).all()
    assert float(err_a.max()) <= 0 and float(err_b.max()) <= 0, what


def check_c(c, s, dense, W, what):
    delta = W * EPS24 * max(1.0, float(s.abs().max()))
    bound = dense.sum(1) * (delta + EPS24 * (s.abs() * dense).sum(1))
    err = (c.double().cpu() - (s * dense).sum(1)).abs()
    print(f"{what}: C max |err| {float(err.max()):.3e}  largest bound {float(bound.max()):.3e}")
    assert bool((err <= bound).all()), what


@pytest.mark.gpu
@pytest.mark.parametrize("indexed", [False, True])
@pytest.mark.parametrize("name,p,dtype,W", TILE_CASES)
def test_tile_path(dev, name, p, dtype, W, indexed):
    """A workspace of exactly 64 columns: chunks of 64 + ... + a ragged 13; row 3 has a label in every chunk."""
    from besskge import _native as nat

    nq, n_neg, half = 70, 333, 160
    query, table = problem(name, dtype, W, nq, 400 if indexed else n_neg, seed=W + p)
    idx = torch.randperm(400, generator=torch.Generator().manual_seed(1))[:n_neg].to(torch.int32) if indexed else None
    rows = table[idx.long()] if indexed else table
    ptr, col, dense = make_labels(nq, n_neg, 3, full_row=(3, [332, 0, 64, 63, 130, 200, 270]))
    coef = torch.rand(nq, generator=torch.Generator().manual_seed(2)) + 0.5
    coef[7] = 0.0
    s, want_q, want_e = reference(name, p, query, rows, dense, coef)
    d = make_desc(name, p, dtype, W)
    q, t = query.to(dev), table.to(dev)
    neg = nat.RowSource(t, idx.to(dev) if indexed else None)
    what = f"{name} p={p} {dtype} tile"
    state = nat.neg_score_shared_bce(d, q, neg, workspace_bytes=nq * 64 * 4)
    check_ab(state, s, merge_depth("tile", n_neg, 64), W, what)
    # two calls on two halves of the candidates accumulate
    lo = nat.RowSource(t, idx[:half].to(dev)) if indexed else nat.RowSource(t[:half])
    hi = nat.RowSource(t, idx[half:].to(dev)) if indexed else nat.RowSource(t[half:])
    two = nat.neg_score_shared_bce(d, q, lo, workspace_bytes=nq * 64 * 4)
    two = nat.neg_score_shared_bce(d, q, hi, state_ab=two, workspace_bytes=nq * 64 * 4)
    check_ab(two, s, merge_depth("tile", half, 64) + merge_depth("tile", n_neg - half, 64), W, what + ", two calls")
    check_c(nat.label_score_sums(d, q, neg, ptr.to(dev), col.to(dev)), s, dense, W, what)
    filled = torch.randn(nq, W, generator=torch.Generator().manual_seed(13))
    fixed = (nq * W * 4 + 255) // 256 * 256
    dq, dn = nat.neg_score_shared_bwd_bce(d, q, neg, SMOOTH, PW, ptr.to(dev), col.to(dev), coef.to(dev),
                                          d_query=filled.to(dev).clone(), workspace_bytes=fixed + 2 * nq * 64 * 4)
    torch.testing.assert_close(dq.cpu().double(), filled.double() + want_q, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(dn.cpu().double(), want_e, rtol=1e-4, atol=1e-5)
    assert torch.equal(dq[7].cpu(), filled[7]), "coef == 0: exact zeros are added"


@pytest.mark.gpu
@pytest.mark.parametrize("name,p,dtype,W", [("DistMult", 0, torch.float32, 260), ("TransE", 1, torch.float32, 321),
                                            ("TransE", 3, torch.float16, 130), ("ComplEx", 0, torch.float16, 1032)])
def test_label_score_sums_row_classes(dev, name, p, dtype, W):
    """Widths whose rows take 2 and more vector chunks per lane, at every vector width (4, 1, 2, 8 scalars);
    positions outside the list (-1, n_neg) are skipped."""
    from besskge import _native as nat

    nq, n_neg = 9, 50
    query, table = problem(name, dtype, W, nq, n_neg, seed=W, scale=0.2)
    ptr, col, dense = make_labels(nq, n_neg, W)
    s = ref_scores(name, p, query.double(), table.double())
    d = make_desc(name, p, dtype, W)
    outside = torch.cat([col[: int(ptr[1])], torch.tensor([-1, n_neg], dtype=torch.int32), col[int(ptr[1]):]])
    ptr2 = ptr.clone()
    ptr2[1:] += 2
    c = nat.label_score_sums(d, query.to(dev), nat.RowSource(table.to(dev)), ptr2.to(dev), outside.to(dev))
    check_c(c, s, dense, W, f"{name} p={p} {dtype} W={W}")


@pytest.mark.gpu
@pytest.mark.parametrize("name,dtype", FUSED_CASES)
def test_fused_epilogue(dev, fused_problems, name, dtype):
    """512 x 8229, W = 64: the epilogue of the split-fp16 product (ragged last tiles on both axes), bitwise
    reproducible; the backward at that shape with labels that include the last column."""
    from besskge import _native as nat

    W, nq, n_neg = 64, 512, 8192 + 37
    query, table, _ = fused_problems[(name, dtype)]
    ptr, col, dense = make_labels(nq, n_neg, 5, full_row=(0, [n_neg - 1, 0, 4096]))
    coef = torch.rand(nq, generator=torch.Generator().manual_seed(3)) + 0.5
    s, want_q, want_e = reference(name, 0, query, table, dense, coef)
    d = make_desc(name, 0, dtype, W)
    assert nat.load().bess_neg_score_shared_workspace(ctypes.byref(d), nq, n_neg) > 0  # the split product's shape
    q, neg = query.to(dev), nat.RowSource(table.to(dev))
    state = nat.neg_score_shared_bce(d, q, neg)
    check_ab(state, s, merge_depth("fused", n_neg), W, f"{name} {dtype} fused")
    assert torch.equal(state, nat.neg_score_shared_bce(d, q, neg)), "state_ab must be bitwise reproducible"
    dq, dn = nat.neg_score_shared_bwd_bce(d, q, neg, SMOOTH, PW, ptr.to(dev), col.to(dev), coef.to(dev))
    dev_q, dev_e = grad_deviation(dq, want_q), grad_deviation(dn, want_e)
    print(f"{name} {dtype}: gradient deviation d_query {dev_q:.3e}  d_neg {dev_e:.3e}")
    assert max(dev_q, dev_e) <= 4 * SPLIT_BCE_GRAD_MEASURED


@pytest.mark.gpu
def test_range_fallback(dev):
    """A candidate element of 1e5 is outside the fp16 range: the wrapper answers the finite fp32 state, added to
    the state that was handed in."""
    from besskge import _native as nat

    name, W, nq, n_neg = "DistMult", 64, 512, 8192 + 37
    query, table = problem(name, torch.float32, W, nq, n_neg, seed=8, scale=0.4)
    table[4321, 7] = 1e5
    d = make_desc(name, 0, torch.float32, W)
    base = torch.rand(nq, 2, generator=torch.Generator().manual_seed(9)) * 100
    got = nat.neg_score_shared_bce(d, query.to(dev), nat.RowSource(table.to(dev)), state_ab=base.to(dev).clone())
    check_ab(got, ref_scores(name, 0, query.double(), table.double()), merge_depth("tile", n_neg, 1 << 20), W,
             "range fallback", base=base.double())


@pytest.mark.gpu
def test_other_scorers_are_refused(dev):
    from besskge import _native as nat

    d = nat.ModelDesc()
    d.scorer, d.norm_p, d.dtype, d.width, d.rel_width = nat.BOXE, 1, nat.F32, 16, 4 * 8 + 2
    d.reserved[0] = 3
    lib = nat.load()
    out = torch.full((4, 16), 7.0, device=dev)
    o = out.data_ptr()
    assert lib.bess_neg_score_shared_fwd_bce(ctypes.byref(d), 0, 1, 0, 0, 1, o, 0, 0, 0) == -2  # BESS_EUNSUPPORTED
    assert lib.bess_label_score_sums(ctypes.byref(d), 0, 1, 0, 0, 1, 0, 0, o, 0) == -2
    assert lib.bess_neg_score_shared_bwd_bce(ctypes.byref(d), 0, 1, 0, 0, 1, 0.0, 1.0, 0, 0, 0, o, o, 0, 0, 0) == -2
    assert bool((out == 7.0).all())
