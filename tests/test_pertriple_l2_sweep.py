"""The row-ordered per-triple forward (K5s, csrc/neg_pertriple.hip) against the plain one.

bess_neg_score_pertriple_fwd takes K5s when desc.reserved[1] holds the row count of the table and the pairs use each
row several times over; with reserved[1] = 0 it takes the plain kernel.  The two must give the same scores bit for
bit, on every shape: the GPU tests score the same operands both ways and compare with torch.equal."""

import ctypes

import pytest
import torch

from besskge import _native as nat


def make_desc(scorer, p, table):
    W = int(table.shape[1])
    return nat.make_desc(scorer, p, table, W // 2 if scorer == nat.ROTATE else W)


def desc_for(scorer, p, table, rows):
    d = make_desc(scorer, p, table)
    d.reserved[1] = rows
    return d


def sweep(scorer, p, table, rows, nq, n_neg):
    return nat.pertriple_sweep(desc_for(scorer, p, table, rows), nq, n_neg)


def test_dispatch_choice_needs_no_gpu():
    f32 = torch.empty((0, 512), dtype=torch.float32)
    assert sweep(nat.COMPLEX, 0, f32, 93_773, 4096, 256)  # the headline: ~11 uses per row
    assert not sweep(nat.COMPLEX, 0, f32, 0, 4096, 256)  # row count unknown
    assert not sweep(nat.COMPLEX, 0, f32, 4096 * 256, 4096, 256)  # a receive buffer: every row once
    assert not sweep(nat.COMPLEX, 0, f32, 4_000_000, 4096, 256)  # a table 4x larger than the pairs
    assert sweep(nat.DISTMULT, 0, f32, 1000, 4000, 1)  # exactly 4 uses per row
    assert not sweep(nat.DISTMULT, 0, f32, 1001, 4000, 1)
    assert sweep(nat.TRANSE, 1, f32, 100, 1, 1000) and sweep(nat.ROTATE, 2, f32, 100, 1, 1000)
    assert sweep(nat.TRANSE, 3, torch.empty((0, 2048), dtype=torch.float16), 100, 64, 64)  # one f16 window
    assert not sweep(nat.TRANSE, 1, torch.empty((0, 2056), dtype=torch.float16), 100, 64, 64)  # two windows
    assert not sweep(nat.DISTMULT, 0, torch.empty((0, 1028), dtype=torch.float32), 100, 64, 64)  # W % 4: 256 per window
    d = desc_for(nat.COMPLEX, 0, f32, 93_773)
    out = ctypes.c_int32(7)
    assert nat.load().bess_neg_pertriple_sweep(ctypes.byref(d), 4096, 0, ctypes.byref(out)) == 0 and out.value == 0


def test_row_count_is_set_only_for_the_plain_scorers():
    table = torch.empty((321, 64), dtype=torch.float32)
    d = make_desc(nat.DISTMULT, 0, table)
    c = nat.with_row_count(d, table)
    assert c.reserved[1] == 321 and d.reserved[1] == 0  # a copy: the caller's descriptor is left alone
    d.scorer = nat.AFFINE
    d.reserved[1] = 5
    assert nat.with_row_count(d, table).reserved[1] == 5


def score(desc, rows, query, table, idx, n_neg, ld=None):
    """bess_neg_score_pertriple_fwd with desc.reserved[1] = rows; out [nq, ld] pre-filled with NaN."""
    d = nat.copy_desc(desc)
    d.reserved[1] = rows
    nq = query.shape[0]
    ld = n_neg if ld is None else ld
    out = torch.full((nq, ld), float("nan"), dtype=torch.float32, device=query.device)
    nat._launch("bess_neg_score_pertriple_fwd", query.device, ctypes.byref(d), query.data_ptr(), nq, table.data_ptr(),
                idx.data_ptr(), n_neg, out.data_ptr(), ld)
    torch.cuda.synchronize()
    return out


def both_paths(scorer, p, rows, W, nq, n_neg, dtype=torch.float32, idx=None, ld=None, seed=0):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(seed)
    table = (torch.randn((rows, W), generator=g) * 0.3).to(dtype).to(dev)
    query = (torch.randn((nq, W), generator=g) * 0.3).to(dev)
    if idx is None:
        idx = torch.randint(0, rows, (nq * n_neg,), generator=g, dtype=torch.int32)
    idx = idx.to(torch.int32).to(dev).contiguous()
    desc = make_desc(scorer, p, table)
    assert nat.pertriple_sweep(nat.with_row_count(desc, table), nq, n_neg), "the case must take the row-ordered kernel"
    plain = score(desc, 0, query, table, idx, n_neg, ld)
    swept = score(desc, rows, query, table, idx, n_neg, ld)
    assert torch.isfinite(plain[:, :n_neg]).all()
    assert torch.equal(plain[:, :n_neg], swept[:, :n_neg])
    if ld is not None and ld > n_neg:
        assert torch.isnan(swept[:, n_neg:]).all(), "columns past n_neg written"
    return desc, query, table, idx, plain


@pytest.mark.gpu
def test_c2_shape_bitwise_and_through_the_binding():
    desc, query, table, idx, plain = both_paths(nat.COMPLEX, 0, 93_773, 512, 4096, 256)
    public = nat.neg_score_pertriple_fwd(desc, query, nat.RowSource(table, idx), 256)
    assert torch.equal(public, plain)


@pytest.mark.gpu
@pytest.mark.parametrize("scorer,p,W", [(nat.DISTMULT, 0, 256), (nat.TRANSE, 1, 256), (nat.ROTATE, 2, 512),
                                        (nat.TRANSE, 3, 128), (nat.TRANSE, 2, 37), (nat.DISTMULT, 0, 1024)])
def test_scorers(scorer, p, W):
    both_paths(scorer, p, 20_000, W, 512, 256)


@pytest.mark.gpu
@pytest.mark.parametrize("scorer,p,W", [(nat.COMPLEX, 0, 512), (nat.TRANSE, 1, 200), (nat.ROTATE, 2, 100),
                                        (nat.TRANSE, 3, 2048)])
def test_f16_tables(scorer, p, W):
    both_paths(scorer, p, 10_000, W, 384, 256, dtype=torch.float16)


@pytest.mark.gpu
@pytest.mark.parametrize("nq,n_neg,rows", [(4096, 1, 1000), (64, 257, 4000), (40, 1000, 10_000), (1, 1000, 250),
                                           (7, 300, 500), (33, 2500, 5000)])
def test_odd_sizes(nq, n_neg, rows):
    both_paths(nat.COMPLEX, 0, rows, 512, nq, n_neg)


@pytest.mark.gpu
def test_every_negative_on_one_row():
    both_paths(nat.DISTMULT, 0, 5000, 256, 256, 256, idx=torch.full((256 * 256,), 1234, dtype=torch.int32))


@pytest.mark.gpu
def test_negatives_inside_a_500_row_range():
    g = torch.Generator().manual_seed(3)
    idx = torch.randint(40_000, 40_500, (2048 * 256,), generator=g, dtype=torch.int32)
    both_paths(nat.COMPLEX, 0, 93_773, 512, 2048, 256, idx=idx)


@pytest.mark.gpu
def test_duplicates_and_a_hot_row():
    g = torch.Generator().manual_seed(4)
    idx = torch.randint(0, 3000, (1000 * 64,), generator=g, dtype=torch.int32)
    idx[::3] = 17
    both_paths(nat.TRANSE, 1, 3000, 256, 1000, 64, idx=idx)


@pytest.mark.gpu
def test_table_past_2_to_the_17_rows():
    both_paths(nat.DISTMULT, 0, 140_000, 64, 4096, 256)


@pytest.mark.gpu
def test_leading_dimension_past_n_neg():
    both_paths(nat.COMPLEX, 0, 15_000, 512, 300, 256, ld=301)
    both_paths(nat.TRANSE, 1, 1500, 128, 70, 100, ld=160)
