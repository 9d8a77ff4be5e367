"""`bess_neg_score_shared_fwd_lse` / `bess_neg_score_shared_bwd_softmax` (csrc/neg_shared.hip, the log-sum-exp
epilogue of csrc/gemm_split.hip) against float64 on the CPU, autograd supplying the gradients.

Tolerance of the log-sum-exp: absolute `(L + W) * 2^-24 * max(1, max_j |s|)`.
  * A score is a chain of W fp32 operations on terms of magnitude <= max|s| (the split-fp16 product is more
    accurate than that chain: 3-4e-7 of max|out|, DESIGN "split-fp16"), so a score is off by at most
    W * 2^-24 * max|s|, and a common shift of all scores of a row shifts its log-sum-exp by as much.
  * The sum of exponentials is a merge tree: every level multiplies by an `exp` of relative error <= 2^-24 (times
    the magnitude of its argument, which is <= 17 for every term that is not below 2^-24 of the largest) and
    adds once.  A relative error r of the sum is an absolute error r of its logarithm, so L levels add
    L * 2^-24 * max(1, .).  `merge_depth` counts the levels of the tree that is implemented:
      tile path   per lane ceil(cols / 64) sequential terms, 6 butterfly levels over the wave's 64 lanes, then one
                  merge into the state per chunk (a chain as long as the number of chunks);
      epilogue    1 (a lane's two columns) + 5 butterfly levels over the 32 lanes of a row, then per chunk of the
                  split product: ceil(slabs / 64) sequential merges per lane + 6 butterfly levels + 1 into the state.

Gradients: the fp32 paths hold the project's shared-negative tolerance (rtol 1e-4, atol 1e-5).  Where the scores
behind the coefficients come out of the split-fp16 product the deviation cannot be derived from first principles:
`SPLIT_GRAD_MEASURED` is the largest deviation from float64, relative to the row's largest |gradient element|,
measured on the MI355X over the cases of `test_fused_epilogue_gradients`; the test holds 4 x that."""

import ctypes
import math

import pytest
import torch

F64 = torch.float64
SPLIT_CHUNK = 65536
#: largest |gradient - float64| / max |row of the float64 gradient| measured on the MI355X (see the module docstring)
SPLIT_GRAD_MEASURED = 4.75e-6  # (d_query, DistMult fp32 table, 512 x 8229; the split backward at 2048 x 2048: 8.8e-7)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda", 0)


def make_desc(name, p, dtype, W, fp32_math=False):
    from besskge import _native as nat

    d = nat.ModelDesc()
    d.scorer = {"TransE": nat.TRANSE, "RotatE": nat.ROTATE, "DistMult": nat.DISTMULT, "ComplEx": nat.COMPLEX}[name]
    d.norm_p = p if name in ("TransE", "RotatE") else 0
    d.dtype = nat.F32 if dtype == torch.float32 else nat.F16
    d.width = W
    d.rel_width = W // 2 if name == "RotatE" else W
    if fp32_math:
        d.reserved[0] = nat.FLAG_FP32_MATH
    return d


def ref_scores(name, p, q, e):
    """float64 scores [nq, n] of query rows q against candidate rows e"""
    if name in ("TransE", "RotatE"):
        return -torch.cdist(q, e, p=float(p))
    return q @ e.T


def problem(name, dtype, W, nq, n_rows, seed, scale=0.5, qscale=1.0):
    g = torch.Generator().manual_seed(seed)
    table = (torch.randn(n_rows, W, generator=g) * scale).to(dtype)
    query = (torch.randn(nq, W, generator=g) * scale * qscale).float()
    return query, table


def merge_depth(path, n_neg, cols=None):
    if path == "tile":
        return math.ceil(min(cols, n_neg) / 64) + 6 + math.ceil(n_neg / cols)
    chunks = math.ceil(n_neg / SPLIT_CHUNK)
    slabs = math.ceil(min(n_neg, SPLIT_CHUNK) / 64)
    return 1 + 5 + chunks * (math.ceil(slabs / 64) + 6 + 1)


def lse_tolerance(depth, W, scores):
    return (depth + W) * 2.0 ** -24 * max(1.0, float(scores.abs().max()))


def lse_of(state):
    return (state[:, 0].double() + torch.log(state[:, 1].double())).cpu()


def check_lse(state, scores, depth, W, what):
    want = torch.logsumexp(scores, dim=1)
    got = lse_of(state)
    tol = lse_tolerance(depth, W, scores)
    err = float((got - want).abs().max())
    print(f"{what}: lse max |err| {err:.3e}  tolerance {tol:.3e}")
    assert torch.isfinite(got).all()
    assert err <= tol, (what, err, tol)
    return want


def reference_grads(name, p, query, rows, coef):
    q = query.double().clone().requires_grad_(True)
    e = rows.double().clone().requires_grad_(True)
    (coef.double() * torch.logsumexp(ref_scores(name, p, q, e), dim=1)).sum().backward()
    return q.grad, e.grad


def grad_deviation(got, want):
    """largest |got - want| relative to the row's largest |want|"""
    scale = want.abs().amax(dim=1, keepdim=True).clamp_min(1e-30)
    return float(((got.double().cpu() - want).abs() / scale).max())


TILE_CASES = [("DistMult", 0, torch.float32, 20), ("ComplEx", 0, torch.float16, 32), ("TransE", 1, torch.float32, 24),
              ("TransE", 2, torch.float32, 24), ("RotatE", 1, torch.float16, 16)]


@pytest.mark.gpu
@pytest.mark.parametrize("indexed", [False, True])
@pytest.mark.parametrize("name,p,dtype,W", TILE_CASES)
def test_tile_path(dev, name, p, dtype, W, indexed):
    """A workspace of exactly 64 columns: chunks of 64 + 64 + ... + a ragged 13, forward and backward."""
    from besskge import _native as nat

    nq, n_neg = 70, 333
    query, table = problem(name, dtype, W, nq, 400 if indexed else n_neg, seed=W + p)
    idx = torch.randperm(400, generator=torch.Generator().manual_seed(1))[:n_neg].to(torch.int32) if indexed else None
    rows = table[idx.long()] if indexed else table
    d = make_desc(name, p, dtype, W)
    neg = nat.RowSource(table.to(dev), idx.to(dev) if indexed else None)
    scores = ref_scores(name, p, query.double(), rows.double())
    state = nat.neg_score_shared_lse(d, query.to(dev), neg, workspace_bytes=nq * 64 * 4)
    lse = check_lse(state, scores, merge_depth("tile", n_neg, 64), W, f"{name} p={p} {dtype} tile")
    coef = torch.rand(nq, generator=torch.Generator().manual_seed(2)) + 0.5
    fixed = (nq * W * 4 + 255) // 256 * 256
    dq, dn = nat.neg_score_shared_bwd_softmax(d, query.to(dev), neg, lse.float().to(dev), coef.to(dev),
                                              workspace_bytes=fixed + 2 * nq * 64 * 4)
    want_q, want_e = reference_grads(name, p, query, rows, coef)
    torch.testing.assert_close(dq.cpu().double(), want_q, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(dn.cpu().double(), want_e, rtol=1e-4, atol=1e-5)
    # the default workspace (one chunk) gives the same function
    dq1, dn1 = nat.neg_score_shared_bwd_softmax(d, query.to(dev), neg, lse.float().to(dev), coef.to(dev))
    torch.testing.assert_close(dq1.cpu().double(), want_q, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(dn1.cpu().double(), want_e, rtol=1e-4, atol=1e-5)


FUSED_CASES = [("DistMult", torch.float32), ("DistMult", torch.float16), ("ComplEx", torch.float32),
               ("ComplEx", torch.float16)]


@pytest.fixture(scope="module")
def fused_problems():
    """(query, table, float64 scores) of the fused cases, computed once"""
    out = {}
    for name, dtype in FUSED_CASES:
        query, table = problem(name, dtype, 64, 512, 8192 + 37, seed=len(out) + 10, scale=0.4)
        out[(name, dtype)] = (query, table, ref_scores(name, 0, query.double(), table.double()))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,dtype", FUSED_CASES)
def test_fused_epilogue(dev, fused_problems, name, dtype):
    """512 x 8229: 4 x 65 = 260 tiles of 128 x 128, just above the threshold of the split-fp16 product, ragged last
    tiles on both axes; reproducible bit for bit; accumulates over calls."""
    from besskge import _native as nat

    W, nq, n_neg = 64, 512, 8192 + 37
    query, table, scores = fused_problems[(name, dtype)]
    d = make_desc(name, 0, dtype, W)
    assert nat.load().bess_neg_score_shared_workspace(ctypes.byref(d), nq, n_neg) > 0  # the split product's shape
    q, t = query.to(dev), table.to(dev)
    state = nat.neg_score_shared_lse(d, q, nat.RowSource(t))
    check_lse(state, scores, merge_depth("fused", n_neg), W, f"{name} {dtype} fused")
    again = nat.neg_score_shared_lse(d, q, nat.RowSource(t))
    assert torch.equal(state, again), "state_ml must be bitwise reproducible"
    # the same candidates in two calls (the second one indexed): the state accumulates
    cut = 4096 + 64
    two = nat.neg_score_shared_lse(d, q, nat.RowSource(t[:cut]))
    rest = torch.arange(cut, n_neg, dtype=torch.int32, device=dev)
    two = nat.neg_score_shared_lse(d, q, nat.RowSource(t, rest), state_ml=two)
    # (either half alone has too few tiles for the split product: two tile-path calls, one chunk each)
    depth = merge_depth("tile", cut, 8192) + merge_depth("tile", n_neg - cut, 8192)
    check_lse(two, scores, depth, W, f"{name} {dtype} two calls")


@pytest.mark.gpu
@pytest.mark.parametrize("name,dtype", FUSED_CASES)
def test_fused_epilogue_gradients(dev, fused_problems, name, dtype):
    """The backward at the fused shape: its coefficients come from scores of the split-fp16 product."""
    from besskge import _native as nat

    W = 64
    query, table, scores = fused_problems[(name, dtype)]
    d = make_desc(name, 0, dtype, W)
    lse = torch.logsumexp(scores, dim=1)
    coef = torch.rand(query.shape[0], generator=torch.Generator().manual_seed(3)) + 0.5
    dq, dn = nat.neg_score_shared_bwd_softmax(d, query.to(dev), nat.RowSource(table.to(dev)), lse.float().to(dev),
                                              coef.to(dev))
    want_q, want_e = reference_grads(name, 0, query, table, coef)
    dev_q, dev_e = grad_deviation(dq, want_q), grad_deviation(dn, want_e)
    print(f"{name} {dtype}: gradient deviation d_query {dev_q:.3e}  d_neg {dev_e:.3e}")
    assert max(dev_q, dev_e) <= 4 * SPLIT_GRAD_MEASURED


@pytest.mark.gpu
def test_split_product_backward(dev):
    """2048 x 2048, W = 64: both products of the backward run on the matrix cores (split-fp16, k split 8)."""
    from besskge import _native as nat

    name, W, n = "ComplEx", 64, 2048
    query, table = problem(name, torch.float32, W, n, n, seed=5, scale=0.4)
    d = make_desc(name, 0, torch.float32, W)
    assert nat.load().bess_neg_score_shared_bwd_workspace(ctypes.byref(d), n, n) > 0
    scores = ref_scores(name, 0, query.double(), table.double())
    state = nat.neg_score_shared_lse(d, query.to(dev), nat.RowSource(table.to(dev)))
    lse = check_lse(state, scores, merge_depth("fused", n), W, "ComplEx 2048 x 2048")
    coef = torch.rand(n, generator=torch.Generator().manual_seed(4)) + 0.5
    dq, dn = nat.neg_score_shared_bwd_softmax(d, query.to(dev), nat.RowSource(table.to(dev)), lse.float().to(dev),
                                              coef.to(dev))
    want_q, want_e = reference_grads(name, 0, query, table, coef)
    dev_q, dev_e = grad_deviation(dq, want_q), grad_deviation(dn, want_e)
    print(f"split backward: gradient deviation d_query {dev_q:.3e}  d_neg {dev_e:.3e}")
    assert max(dev_q, dev_e) <= 4 * SPLIT_GRAD_MEASURED


@pytest.mark.gpu
def test_across_split_chunk(dev):
    """65,736 candidates: two passes of the split product (65,536 + 200), one set of partials."""
    from besskge import _native as nat

    name, W, nq, n_neg = "DistMult", 32, 128, SPLIT_CHUNK + 200
    query, table = problem(name, torch.float32, W, nq, n_neg, seed=6)
    d = make_desc(name, 0, torch.float32, W)
    assert nat.load().bess_neg_score_shared_workspace(ctypes.byref(d), nq, n_neg) > 0
    state = nat.neg_score_shared_lse(d, query.to(dev), nat.RowSource(table.to(dev)))
    check_lse(state, ref_scores(name, 0, query.double(), table.double()), merge_depth("fused", n_neg), W,
              "DistMult across SPLIT_CHUNK")


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["fused", "tile"])
def test_online_max(dev, path):
    """Scores of a row span about +-200: exp(score) overflows fp32, the running maximum keeps the sums finite."""
    from besskge import _native as nat

    name, W, nq, n_neg = "DistMult", 64, 512, 8192 + 37
    query, table = problem(name, torch.float32, W, nq, n_neg, seed=7, scale=1.0, qscale=6.0)
    scores = ref_scores(name, 0, query.double(), table.double())
    spread = float(scores.amax(dim=1).median())
    assert 100.0 < spread < 400.0, spread
    d = make_desc(name, 0, torch.float32, W)
    ws = None if path == "fused" else nq * 1024 * 4
    state = nat.neg_score_shared_lse(d, query.to(dev), nat.RowSource(table.to(dev)), workspace_bytes=ws)
    check_lse(state, scores, merge_depth(path, n_neg, 1024), W, f"online max, {path}")


@pytest.mark.gpu
def test_range_fallback(dev):
    """An operand outside the fp16 range: the library answers NaN states, the wrapper repeats the call in fp32
    arithmetic - the result of asking for BESS_FLAG_FP32_MATH from the start, and no NaN escapes."""
    from besskge import _native as nat

    name, W, nq, n_neg = "DistMult", 64, 512, 8192 + 37
    query, table = problem(name, torch.float32, W, nq, n_neg, seed=8, scale=0.4)
    table[4321, 7] = 7e4
    d, exact = make_desc(name, 0, torch.float32, W), make_desc(name, 0, torch.float32, W, fp32_math=True)
    q, t = query.to(dev), table.to(dev)
    # the library itself: every state of the call is NaN
    raw = torch.empty((nq, 2), dtype=torch.float32, device=dev)
    raw[:, 0], raw[:, 1] = float("-inf"), 0.0
    nbytes = int(nat.load().bess_neg_score_shared_fwd_lse_workspace(ctypes.byref(d), nq, n_neg))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    nat._launch("bess_neg_score_shared_fwd_lse", dev, ctypes.byref(d), q.data_ptr(), nq, t.data_ptr(), 0, n_neg,
                raw.data_ptr(), ws.data_ptr(), nbytes)
    assert bool(torch.isnan(raw).all())
    got = nat.neg_score_shared_lse(d, q, nat.RowSource(t))
    want = nat.neg_score_shared_lse(exact, q, nat.RowSource(t))
    assert not bool(torch.isnan(got).any())
    assert torch.equal(got, want)
    check_lse(got, ref_scores(name, 0, query.double(), table.double()), merge_depth("tile", n_neg, 1 << 20), W,
              "range fallback")


@pytest.mark.gpu
def test_edge_sizes(dev):
    from besskge import _native as nat

    for name, p in (("TransE", 1), ("DistMult", 0)):
        W = 8
        d = make_desc(name, p, torch.float32, W)
        query, table = problem(name, torch.float32, W, 1, 1, seed=9)
        state = nat.neg_score_shared_lse(d, query.to(dev), nat.RowSource(table.to(dev)))
        scores = ref_scores(name, p, query.double(), table.double())
        check_lse(state, scores, merge_depth("tile", 1, 64), W, f"{name} 1 x 1")
        dq, dn = nat.neg_score_shared_bwd_softmax(d, query.to(dev), nat.RowSource(table.to(dev)),
                                                  lse_of(state).float().to(dev), torch.ones(1, device=dev))
        want_q, want_e = reference_grads(name, p, query, table, torch.ones(1))
        torch.testing.assert_close(dq.cpu().double(), want_q, rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(dn.cpu().double(), want_e, rtol=1e-4, atol=1e-5)
        # zero sizes: OK, nothing is touched
        lib = nat.load()
        assert lib.bess_neg_score_shared_fwd_lse(ctypes.byref(d), 0, 0, 0, 0, 5, 0, 0, 0, 0) == 0
        assert lib.bess_neg_score_shared_fwd_lse(ctypes.byref(d), 0, 5, 0, 0, 0, 0, 0, 0, 0) == 0
        assert lib.bess_neg_score_shared_bwd_softmax(ctypes.byref(d), 0, 0, 0, 0, 5, 0, 0, 0, 0, 0, 0, 0) == 0
        assert lib.bess_neg_score_shared_bwd_softmax(ctypes.byref(d), 0, 5, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == 0
        empty = nat.neg_score_shared_lse(d, query.to(dev), nat.RowSource(table.to(dev)[:0]))
        assert empty[0, 0] == float("-inf") and empty[0, 1] == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("name,p", [("TransE", 1), ("TransE", 2), ("ComplEx", 0)])
def test_zero_coefficients_and_accumulation(dev, name, p):
    """coef[q] == 0 gives exact zero rows of d_query - whatever the row's lse, -inf included, never NaN - and a
    d_query handed in is added to."""
    from besskge import _native as nat

    W, nq, n_neg = 16, 37, 150
    query, table = problem(name, torch.float32, W, nq, n_neg, seed=11)
    d = make_desc(name, p, torch.float32, W)
    scores = ref_scores(name, p, query.double(), table.double())
    lse = torch.logsumexp(scores, dim=1).float()
    coef = torch.rand(nq, generator=torch.Generator().manual_seed(12)) + 0.5
    coef[::3] = 0.0
    lse[0] = float("-inf")  # (coef[0] == 0)
    neg = nat.RowSource(table.to(dev))
    fixed = (nq * W * 4 + 255) // 256 * 256
    dq, dn = nat.neg_score_shared_bwd_softmax(d, query.to(dev), neg, lse.to(dev), coef.to(dev),
                                              workspace_bytes=fixed + 2 * nq * 64 * 4)
    assert bool((dq[::3] == 0).all()) and not bool(torch.isnan(dq).any()) and not bool(torch.isnan(dn).any())
    want_q, want_e = reference_grads(name, p, query, table, coef)
    torch.testing.assert_close(dq.cpu().double(), want_q, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(dn.cpu().double(), want_e, rtol=1e-4, atol=1e-5)
    filled = torch.randn(nq, W, generator=torch.Generator().manual_seed(13))
    dq2, _ = nat.neg_score_shared_bwd_softmax(d, query.to(dev), neg, lse.to(dev), coef.to(dev),
                                              d_query=filled.to(dev).clone(), workspace_bytes=fixed + 2 * nq * 64 * 4)
    torch.testing.assert_close(dq2.cpu().double(), filled.double() + want_q, rtol=1e-4, atol=1e-5)


def test_other_scorers_are_refused():
    from besskge import _native as nat

    d = nat.ModelDesc()
    d.scorer, d.norm_p, d.dtype, d.width, d.rel_width = nat.BOXE, 1, nat.F32, 16, 4 * 8 + 2
    d.reserved[0] = 3
    lib = nat.load()
    assert lib.bess_neg_score_shared_fwd_lse(ctypes.byref(d), 0, 1, 0, 0, 1, 0, 0, 0, 0) == -2  # BESS_EUNSUPPORTED
    assert lib.bess_neg_score_shared_bwd_softmax(ctypes.byref(d), 0, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0) == -2
