#!/usr/bin/env python3
"""The plain per-triple forward against its row-ordered form (K5s) on the same operands: S = 4096 ComplEx d = 256
fp32 queries x 256 negatives, the table's row count withheld (desc.reserved[1] = 0: k_neg_pertriple_fwd) or given
(k_neg_pertriple_fwd_sweep).  Uniform ids over tables of 2 to 11 uses per row, and skewed ids on the C2 table: a
share of all ids on one hot row, all ids inside a 500-row range, ids from a small range per query block
(type-based sampling).  Prints one line per case: us per launch of each path (HIP events, 20 launches)."""
import ctypes
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "bess-kge_amd"), REPO]
import torch  # noqa: E402

from besskge import _native as nat  # noqa: E402

dev = torch.device("cuda", 0)
W, S, N = 512, 4096, 256


def time_launch(d, q, table, idx, out, reps=20):
    args = (ctypes.byref(d), q.data_ptr(), S, table.data_ptr(), idx.data_ptr(), N, out.data_ptr(), N)
    for _ in range(3):
        nat._launch("bess_neg_score_pertriple_fwd", dev, *args)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        nat._launch("bess_neg_score_pertriple_fwd", dev, *args)
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / reps


def case(name, rows, idx_fn):
    torch.manual_seed(0)
    table = torch.randn(rows, W, device=dev) * 0.1
    q = torch.randn(S, W, device=dev)
    idx = idx_fn(rows).to(torch.int32).contiguous()
    d = nat.make_desc(nat.COMPLEX, 0, table, W)
    known = nat.with_row_count(d, table)
    out0 = torch.empty(S, N, device=dev)
    out1 = torch.empty(S, N, device=dev)
    t0 = time_launch(d, q, table, idx, out0)
    t1 = time_launch(known, q, table, idx, out1)
    same = torch.equal(out0, out1)
    taken = nat.pertriple_sweep(known, S, N)
    print(f"{name:34s} rows {rows:>9,d} uses/row {S * N / rows:5.1f}  plain {t0:7.1f} us  "
          f"{'sweep' if taken else '(plain)':7s} {t1:7.1f} us  x{t0 / t1:4.2f}  equal {same}", flush=True)
    del table, q, idx


def uniform(rows):
    return torch.randint(rows, (S * N,), device=dev)


def hot(share):
    def f(rows):
        idx = uniform(rows)
        idx[torch.rand(S * N, device=dev) < share] = 7
        return idx
    return f


def block_range(width):
    """each query's ids inside one range of `width` rows, a different range per 32 queries"""
    def f(rows):
        lo = torch.randint(rows - width, (S // 32, 1), device=dev).repeat_interleave(32, 0)
        return (lo + torch.randint(width, (S, N), device=dev)).reshape(-1)
    return f


C2 = 93_773
for reuse in (2, 4, 6, 8):
    case(f"uniform, {reuse} uses per row", S * N // reuse, uniform)
case("uniform, C2 table", C2, uniform)
for share in (0.01, 0.1, 0.3, 1.0):
    case(f"C2 table, {share:.0%} on one row", C2, hot(share))
case("C2 table, all inside 500 rows", C2, lambda rows: torch.randint(40_000, 40_500, (S * N,), device=dev))
case("C2 table, 2,000-row range per block", C2, block_range(2000))
