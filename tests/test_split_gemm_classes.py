"""csrc/gemm_split.hip: the two split-fp16 matrix-core kernels (128 x 128 tiles, 256 x 128 tiles) share one
wave-tile epilogue - stores, pruned stores, counts.  Every epilogue is anchored here in BOTH kernels, for fp32
and fp16 tables (B_LO true / false) and for indexed and dense candidates: the stored scores against a float64
product, the counts and the pruned blocks against the stored scores of the same kernel, bit for bit.

One candidate count serves both kernels; the number of query rows alone picks the kernel (`launch_product`:
the 256 x 128 kernel runs when its tiles fill the chip, the 128 x 128 kernel otherwise).  The module checks
that arithmetic against the device it runs on before any case, so that another chip fails loudly instead of
testing one kernel twice."""

import ctypes
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

N_CAND = 16347  # 128 column tiles of 128; ragged last tile (91 columns) and ragged last 64-block (27)
WIDTH = 40      # two k slices of 32, the second one padded with zeros
ROWS_128 = 250  # 2 x 128 row tiles -> 256 tiles of 128 x 128, 128 tiles of 256 x 128: the 128 x 128 kernel
ROWS_256 = 300  # 2 x 128 tiles of 256 x 128 = 256: the 256 x 128 kernel
N_TABLE = 2 * N_CAND + 11  # rows for two candidate windows of N_CAND


def _ceil_div(a, b):
    return (a + b - 1) // b


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def kernel_of_rows(dev):
    """{row count: kernel} as `launch_product` picks it on this device; asserts the two intended classes."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    tx = _ceil_div(N_CAND, 128)
    picked = {}
    for rows in (ROWS_128, ROWS_256):
        t4, t8 = tx * _ceil_div(rows, 128), tx * _ceil_div(rows, 256)
        assert t4 >= 256, "the shape must be given to the split path at all"
        picked[rows] = "w8" if t8 >= cus else "f16"
    assert picked[ROWS_128] == "f16", f"{ROWS_128} rows must take the 128 x 128 kernel (t8 < {cus} compute units)"
    assert picked[ROWS_256] == "w8", f"{ROWS_256} rows must take the 256 x 128 kernel (t8 >= {cus} compute units)"
    return picked


@pytest.fixture(scope="module", params=[(rows, dtype, indexed) for rows in (ROWS_128, ROWS_256)
                                        for dtype in (torch.float32, torch.float16) for indexed in (True, False)],
                ids=lambda p: f"{p[0]}rows-{'f32' if p[1] == torch.float32 else 'f16'}-{'indexed' if p[2] else 'dense'}")
def case(request, dev, kernel_of_rows):
    """Inputs of one class and the score matrix its kernel stores (EPI = 0): computed once, never modified."""
    from besskge import _native as nat

    rows, dtype, indexed = request.param
    gen = torch.Generator().manual_seed(rows + int(indexed) + (7 if dtype == torch.float16 else 0))
    c = SimpleNamespace(nat=nat, rows=rows, dtype=dtype, indexed=indexed)
    c.table = (torch.randn(N_TABLE, WIDTH, generator=gen) * 0.3).to(dtype).to(dev)
    c.q = (torch.randn(rows, WIDTH, generator=gen) * 0.3).to(dev)
    c.d = nat.make_desc(nat.DISTMULT, 0, c.table, WIDTH)
    assert nat.load().bess_neg_score_shared_workspace(ctypes.byref(c.d), rows, N_CAND) > 0, "shape must take the split path"
    if indexed:
        perm = torch.randperm(N_TABLE, generator=gen).to(torch.int32).to(dev)
        c.idx = [perm[:N_CAND].contiguous(), perm[N_CAND:2 * N_CAND].contiguous()]
        c.windows = [nat.RowSource(c.table, i) for i in c.idx]
        c.cand = [c.table[i.long()] for i in c.idx]
    else:
        c.cand = [c.table[:N_CAND], c.table[N_CAND:2 * N_CAND]]
        c.windows = [nat.RowSource(r) for r in c.cand]
    c.stored = nat.neg_score_shared_fwd(c.d, c.q, c.windows[0])
    torch.cuda.synchronize()
    return c


def test_stored_scores_match_the_float64_product(case):
    """EPI = 0, full-tile and guarded stores: within 2e-6 of max|ref| of the float64 product (the bound of
    test_split_fp16_gemm_matches_float64_product; values are O(0.3))."""
    ref = case.q.double() @ case.cand[0].double().T
    assert case.stored.shape == ref.shape
    err = float((case.stored.double() - ref).abs().max())
    bound = 2e-6 * float(ref.abs().max())
    print(f"max error {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def _want_counts(sc, thr, excl):
    keep = torch.ones_like(sc, dtype=torch.bool)
    r = torch.arange(sc.shape[0], device=sc.device)
    keep[r[excl >= 0], excl[excl >= 0].long()] = False
    return torch.stack([((sc > thr[:, None]) & keep).sum(-1), ((sc == thr[:, None]) & keep).sum(-1)], dim=1)


def test_counts_equal_the_counts_of_the_stored_scores(case):
    """EPI = 2: per row the number of candidates above / equal to the row's threshold, the excluded column left
    out - exactly what counting the stored matrix of the same kernel gives; excluded columns at the edges of the
    matrix and of an interior 64-block, thresholds at +-inf and at a tie, fp16-rounded comparison, and a second
    window of candidates added to the same counters."""
    nat, sc, nq, dev = case.nat, case.stored, case.rows, case.stored.device
    gen = torch.Generator().manual_seed(nq)
    excl = torch.randint(0, N_CAND, (nq,), generator=gen).to(torch.int32)
    excl[::7] = -1
    excl[5], excl[6] = 0, N_CAND - 1  # first and last column
    excl[8], excl[9] = 64, 127        # first and last column of an interior 64-block
    excl = excl.to(dev)
    r = torch.arange(nq, device=dev)
    # thresholds: the score of the excluded candidate, or (no exclusion) of column 17 - a tie with that column
    thr = torch.where(excl >= 0, sc[r, excl.clamp(min=0).long()], sc[r, 17])
    thr[3] = float("inf")
    thr[4] = -float("inf")
    thr = thr.contiguous()
    counts = nat.neg_score_shared_counts(case.d, case.q, case.windows[0], thr, excl)
    want = _want_counts(sc, thr, excl)
    assert torch.equal(counts.long(), want)
    assert int(want[excl < 0][:, 1].min()) >= 1  # (rows without an exclusion tie with their column 17)
    assert int(want[3].sum()) == 0 and int(want[4, 0]) == N_CAND - 1
    # a half-precision model ranks fp16 scores: many ties
    sc16, thr16 = sc.half().float(), thr.half().float().contiguous()
    c16 = nat.neg_score_shared_counts(case.d, case.q, case.windows[0], thr16, excl, round_f16=True)
    want16 = _want_counts(sc16, thr16, excl)
    assert torch.equal(c16.long(), want16)
    assert int(want16[:, 1].sum()) > int(want[:, 1].sum())
    # a second window of candidates goes into the same counters (its own exclusions, the same thresholds)
    sc_b = nat.neg_score_shared_fwd(case.d, case.q, case.windows[1])
    ex_b = torch.randint(0, N_CAND, (nq,), generator=gen).to(torch.int32)
    ex_b[1::3] = -1
    ex_b = ex_b.to(dev)
    for round_f16, first, th, mat in ((False, counts, thr, sc_b), (True, c16, thr16, sc_b.half().float())):
        both = nat.neg_score_shared_counts(case.d, case.q, case.windows[1], th, ex_b, counts=first.clone(),
                                           round_f16=round_f16)
        assert torch.equal(both.long(), first.long() + _want_counts(mat, th, ex_b))


def test_pruned_stores_write_exactly_the_blocks_that_matter(case):
    """EPI = 1: a (row, 64-column block) is flagged iff a stored score in it is strictly above the row's
    threshold (the row's 10th-largest stored score; one row at -inf: every block; one at +inf: none), and every
    flagged block holds the stored scores bit for bit."""
    nat, sc, nq, dev = case.nat, case.stored, case.rows, case.stored.device
    thr = sc.topk(10, dim=1).values[:, -1].contiguous()
    thr[2] = -float("inf")
    thr[11] = float("inf")
    got, flags = nat.neg_score_shared_fwd_pruned(case.d, case.q, case.windows[0], thr)
    torch.cuda.synchronize()
    nb = _ceil_div(N_CAND, 64)
    pad = torch.full((nq, nb * 64), -float("inf"), device=dev)
    pad[:, :N_CAND] = sc
    hit = (pad.reshape(nq, nb, 64) > thr[:, None, None]).any(dim=2)
    flagged = flags[:, :nb].bool()
    assert torch.equal(flagged, hit)
    assert bool(hit[2].all()) and not bool(hit[11].any())
    assert 9 * (nq - 2) >= int(hit.sum()) - nb >= nq - 2  # (at most 9 blocks per ordinary row, at least one)
    written = flagged[:, torch.arange(nb * 64, device=dev) // 64][:, :N_CAND]
    assert torch.equal(got[written], sc[written])
