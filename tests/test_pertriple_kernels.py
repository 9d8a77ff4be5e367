"""The plain per-triple kernels (K5: `bess_neg_score_pertriple_fwd` / `_bwd`, csrc/neg_pertriple.hip), the segmented
reduction that hangs off them (`bess_neg_pertriple_grad_segments`, csrc/segments.hip) and the query / positive-score
kernels of csrc/prepare.hip against float64 - other tests use these kernels AS their reference (the row-ordered and the
fused forward, the segment tests, the small step, the optimisers), so they are anchored here, in every class the host
dispatch (`dispatch_row_class<NativeRows>` of csrc/common.h, called by `run` and `grad_segments_impl`) selects:

  0. the reference itself, on the CPU (no device): the K5 rule of include/besskge_hip.h in float64 with closed-form
     gradients == `oracle.kge._reduce` and its float64 autograd; the (VEC, IT, window) class of every width; the
     `items_per_query` of every shape;
  1. plain forward and backward == float64;
  2. `bess_neg_pertriple_grad_segments` == float64 `index_add` of the reference's row gradients;
  3. `bess_query_fwd/_bwd`, `bess_score_triple_fwd/_bwd`, `bess_query_triple_fwd/_bwd` == `oracle.kge` in float64.

Class table of 1 and 2 (a 16-lane group keeps IT x 16 chunks of VEC scalars of a row; IT = the next of 1, 2, 4, 8, 16
>= ceil(chunks / 16)).  Every width but the two "full" ones leaves the last group of 16 chunks partly filled; the IT 4
and IT 8 widths have 3 and 7 groups, so a whole register iteration is empty (50 and 49 fill 4 groups, the last partly):

  dtype, VEC | IT 1 | IT 2 | IT 4   | IT 8 | IT 16 | IT 16, full
  f32, 4     |  60  | 100  | 132    | 388  | 1020  | 1024
  f32, 1     |   6  |  30  | 50, 34 | 102  |  254  |
  f16, 8     | 120  | 200  | 264    | 776  | 2040  | 2048
  f16, 2     |   6  |  50  |  66    | 194  |  510  |
  f16, 1     |   7  |  31  | 49, 33 | 101  |  255  |

  column windows: f32 2000 = 1024 + 976, 257 = 256 + 1, 513 = 256 + 256 + 1; f16 2056 = 2048 + 8, 514 = 512 + 2,
  257 = 256 + 1 (DOT and L1 are scored; p = 2 and p = 3 are refused, BESS_EUNSUPPORTED, and write nothing).

Every width runs DOT (DistMult), L1 (TransE p = 1) and L2 with p = 2 and p = 3 (TransE); RotatE and ComplEx
descriptors run at two even widths each (`COMPLEX_CASES`).  Every (width, reduction) runs, over a table of 97 rows and
5 queries,
  - n_neg = 37: nb = 8, 5 items per query, the last of 5 negatives (a `valid[u]` tail for both unroll factors),
    d_query cleared and added with atomics;  n_neg = 7: one item, d_query stored plainly;
  - the regimes "normal" (randn * 0.3), "ties" (a third of the columns of a query equal one of its negatives' values;
    negative 0 equals the query row - distance 0 -, negative 1 differs from it in one column) and "repeats" (12
    distinct rows and one hot row; a fifth of d_out exactly 0);
  - ld_out = ld_dout = n_neg + 3 with NaN padding, every output pre-filled with NaN;
  - the calls with d_neg = NULL, with d_query = NULL (DOT also on a table poisoned with NaN) and with
    BESS_FLAG_DNEG_BY_ROW on a permutation list over a table of n_query * n_neg + 50 rows (regime "perm").
`test_items_of_256_negatives` runs W = 8 (f32, f16) at 4096 x 259: nb = 256, two items.

Segments (2): the same widths, reductions and regimes over `SegmentIndex` of the 5 x 37 references.  The host code's
concurrency `n_conc` (windows side by side in one launch) takes two values:
  n_conc = 1: every width of the class table (the query matrix is below the 4 MiB of an L2), f32 768 at 4096 queries
              (three L2 windows one after the other), every p != 1 distance (never windowed);
  n_conc = 2: f32 512 and f16 512 at 4096 queries, DOT and L1 (`test_segments_l2_windows`).
`test_segments_hot_row` gives one row 520 references (> SEGMENT_CAP: the long-segment kernels) at f32 388 (IT 8) and
f16 264 (IT 4).

Tolerances are the project's: rtol 1e-4, atol max(1e-5, 2e-6 max|want|) (`close(..., scale=2e-6)` of test_hip_parity).
Each case also evaluates the same rule in fp32 torch on its own inputs; where that restatement is itself outside the
bound (more than 1 unit of it) the quantity is ill-conditioned in fp32 there and the case's bound becomes 4 x the
restatement's error (`check`, the `close64` rule of test_mask_loss_rank_kernels.py).  d_neg of DOT and of L1 is
compared exactly: one fp32 product of two floats, resp. +-g or 0.  Measured errors: DESIGN.md, section 14."""

import ctypes
import functools

import pytest
import torch

from besskge import _native as nat
from oracle import kge

gpu = pytest.mark.gpu
F32, F16 = torch.float32, torch.float16
RTOL, ATOL, SCALE = 1e-4, 1e-5, 2e-6
EUNSUPPORTED = -2  # BESS_EUNSUPPORTED

ITS = (1, 2, 4, 8, 16)
CLASS_WIDTHS = {  # (dtype, VEC) -> {IT: widths}
    (F32, 4): {1: [60], 2: [100], 4: [132], 8: [388], 16: [1020, 1024]},
    (F32, 1): {1: [6], 2: [30], 4: [50, 34], 8: [102], 16: [254]},
    (F16, 8): {1: [120], 2: [200], 4: [264], 8: [776], 16: [2040, 2048]},
    (F16, 2): {1: [6], 2: [50], 4: [66], 8: [194], 16: [510]},
    (F16, 1): {1: [7], 2: [31], 4: [49, 33], 8: [101], 16: [255]},
}
FULL_WIDTHS = {(F32, 1024), (F16, 2048)}
WINDOW_WIDTHS = {(F32, 2000): [1024, 976], (F32, 257): [256, 1], (F32, 513): [256, 256, 1],
                 (F16, 2056): [2048, 8], (F16, 514): [512, 2], (F16, 257): [256, 1]}
WIDTHS = [(dt, W) for (dt, _), its in CLASS_WIDTHS.items() for ws in its.values() for W in ws] + list(WINDOW_WIDTHS)
# name -> (oracle scorer, native scorer, p)
REDS = {"dot": (kge.DISTMULT, nat.DISTMULT, 1), "l1": (kge.TRANSE, nat.TRANSE, 1), "l2": (kge.TRANSE, nat.TRANSE, 2),
        "l3": (kge.TRANSE, nat.TRANSE, 3)}
COMPLEX_REDS = {"rotate_l1": (kge.ROTATE, nat.ROTATE, 1), "rotate_l2": (kge.ROTATE, nat.ROTATE, 2),
                "complex": (kge.COMPLEX, nat.COMPLEX, 1)}
COMPLEX_CASES = [(F32, 100, "rotate_l2"), (F16, 50, "rotate_l1"), (F32, 132, "complex"), (F16, 200, "complex")]
REGIMES = ["normal", "ties", "repeats", "perm"]
ROWS, NQ, N_NEGS = 97, 5, (37, 7)
BIG_NQ, BIG_NNEG = 4096, 259  # nb = 256, two items per query

MEASURED = {}  # (part, quantity, regime) -> [fp32 restatement, kernel]: largest error in units of the bound


def tname(dtype):
    return "f32" if dtype == F32 else "f16"


def wid(case):
    return "-".join(tname(x) if isinstance(x, torch.dtype) else str(x) for x in case)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda", 0)


# ============================================================================================ 0. the reference
def dispatch_class(dtype, W):
    """[(VEC, IT, columns)] of the column windows of a row of W scalars, as include/besskge_hip.h states the register
    layout: the widest vector that divides W (f32 4 | 1, f16 8 | 2 | 1), windows of 16 x 16 chunks = 256 VEC scalars,
    IT = the next of {1, 2, 4, 8, 16} >= ceil(chunks / 16)."""
    if dtype == F32:
        vec = 4 if W % 4 == 0 else 1
    else:
        vec = 8 if W % 8 == 0 else (2 if W % 2 == 0 else 1)
    out = []
    for col0 in range(0, W, 256 * vec):
        cols = min(256 * vec, W - col0)
        groups = -(-(cols // vec) // 16)
        out.append((vec, next(i for i in ITS if i >= groups), cols))
    return out


def rule(red, q, rows, g, dtype=torch.float64):
    """The K5 rule and its gradients in closed form: q [S, W] f32, rows [S, N, W] (table dtype), g [S, N] f32 ->
    (scores [S, N], d_query [S, W], d_neg [S, N, W]) computed in `dtype` from the exactly converted inputs."""
    p = REDS.get(red, COMPLEX_REDS.get(red))[2]
    q = q.to(dtype)[:, None, :]
    e = rows.to(dtype)
    g = g.to(dtype)[:, :, None]
    if red in ("dot", "complex"):
        return (q * e).sum(-1), (g * e).sum(1), g * q.expand_as(e)
    delta = q - e
    if p == 1:
        dqe = -g * torch.sign(delta)  # sgn(0) = 0
        return -delta.abs().sum(-1), dqe.sum(1), -dqe
    norm = delta.abs().pow(p).sum(-1).pow(1.0 / p)
    inv = torch.where(norm > 0, norm.pow(1 - p), torch.zeros_like(norm))  # 0 at distance 0, as lp_inv
    dqe = -g * torch.sign(delta) * delta.abs().pow(p - 1) * inv[..., None]
    return -norm, dqe.sum(1), -dqe


@functools.lru_cache(maxsize=64)
def inputs(dtype, W, regime, n_neg, nq=NQ):
    """(query [nq, W] f32, table [rows, W] dtype, idx [nq, n_neg] int32, g [nq, n_neg] f32) on the CPU; fixed seed,
    never written to."""
    gen = torch.Generator().manual_seed(100_000 * REGIMES.index(regime) + 10 * W + n_neg + (5 if dtype == F16 else 0))
    rows = nq * n_neg + 50 if regime == "perm" else ROWS
    table = (torch.randn(rows, W, generator=gen) * 0.3).to(dtype)
    query = torch.randn(nq, W, generator=gen) * 0.3
    g = torch.randn(nq, n_neg, generator=gen)
    if regime == "perm":
        idx = torch.randperm(rows, generator=gen)[: nq * n_neg].reshape(nq, n_neg)
    elif regime == "repeats":
        idx = torch.randint(0, 12, (nq, n_neg), generator=gen)
        idx.view(-1)[::3] = 17  # one hot row
        g.view(-1)[::5] = 0.0
    elif regime == "ties":
        assert nq <= 8
        idx = torch.randint(0, 80, (nq, n_neg), generator=gen)
        tied = torch.arange(W) % 3 == 0
        pick = torch.randint(2, n_neg, (nq, W), generator=gen)  # the negative whose value the query takes
        vals = table.float()[idx.gather(1, pick), torch.arange(W)[None, :].expand(nq, W)]
        query = torch.where(tied[None, :], vals, query)
        query = query.to(dtype).float()  # f16 tables: the query takes the f16 value
        for s in range(nq):
            table[80 + s] = query[s].to(dtype)  # distance 0
            table[88 + s] = query[s].to(dtype)  # one column differs
            table[88 + s, W // 2] = (query[s, W // 2] + 0.5).to(dtype)
            idx[s, 0], idx[s, 1] = 80 + s, 88 + s
    else:
        idx = torch.randint(0, rows, (nq, n_neg), generator=gen)
    return query, table, idx.to(torch.int32), g


@functools.lru_cache(maxsize=8)
def references(dtype, W, regime, n_neg, red, nq=NQ):
    """((scores, d_query, d_neg) in float64, the same from the fp32 restatement); d_neg [nq * n_neg, W]."""
    query, table, idx, g = inputs(dtype, W, regime, n_neg, nq)
    rows = table[idx.long()]
    out = []
    for dt in (torch.float64, torch.float32):
        s, dq, dn = rule(red, query, rows, g, dt)
        out.append((s, dq, dn.reshape(nq * n_neg, W)))
    return tuple(out)


def units(x, ref):
    """max |x - ref| / (atol + rtol |ref|) with the project's atol = max(1e-5, 2e-6 max|ref|): <= 1 passes."""
    ref = ref.double()
    atol = max(ATOL, SCALE * float(ref.abs().max()))
    return float(((x.detach().double().cpu() - ref).abs() / (atol + RTOL * ref.abs())).max())


def check(part, quantity, regime, what, got, ref64, ref32):
    """`got` against float64 at the project's bound - or, where the fp32 restatement of the rule is itself outside it
    on these inputs, at 4 x the restatement's error.  The bound never depends on `got`."""
    assert got.shape == ref64.shape, f"{what}: shape {tuple(got.shape)}"
    assert bool(torch.isfinite(ref64).all())
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    e32, ek = units(ref32, ref64), units(got, ref64)
    rec = MEASURED.setdefault((part, quantity, regime), [0.0, 0.0])
    rec[0], rec[1] = max(rec[0], e32), max(rec[1], ek)
    factor = 1.0 if e32 <= 1.0 else 4.0 * e32
    if factor > 1.0 or ek > 1.0:
        print(f"{what}: kernel at {ek:.3g} x, fp32 restatement at {e32:.3g} x of the bound")
    assert ek <= factor, f"{what}: kernel at {ek:.3g} x the bound, fp32 restatement at {e32:.3g} x"


def make_desc(red, table):
    _, scorer, p = REDS.get(red, COMPLEX_REDS.get(red))
    W = int(table.shape[1])
    return nat.make_desc(scorer, p, table, W // 2 if scorer == nat.ROTATE else W)


def items_of(desc, nq, n_neg):
    out = ctypes.c_int32(-1)
    assert nat.load().bess_neg_pertriple_items(ctypes.byref(desc), nq, n_neg, ctypes.byref(out)) == 0
    return out.value


@pytest.mark.parametrize("red", list(REDS) + list(COMPLEX_REDS))
def test_rule_forward_equals_the_oracle(red):
    name, _, p = REDS.get(red, COMPLEX_REDS.get(red))
    for dtype, W in [(F32, 100), (F16, 50), (F32, 6)]:
        for regime in ("normal", "ties"):
            query, table, idx, g = inputs(dtype, W, regime, 37)
            rows = table[idx.long()]
            want = kge._reduce(name, p, query.double()[:, None, :], rows.double())
            got = rule(red, query, rows, g)[0]
            torch.testing.assert_close(got, want, rtol=1e-13, atol=1e-14)
            assert float(got.abs().max()) > 0


@pytest.mark.parametrize("red", list(REDS) + list(COMPLEX_REDS))
def test_rule_gradients_equal_float64_autograd(red):
    """On inputs without ties and without zero distances ("normal", "repeats") - at a tie the subgradient autograd
    picks is a convention, the closed form states the kernels' one."""
    name, _, p = REDS.get(red, COMPLEX_REDS.get(red))
    for dtype, W, regime in [(F32, 100, "normal"), (F16, 50, "repeats"), (F32, 6, "normal")]:
        query, table, idx, g = inputs(dtype, W, regime, 37)
        q = query.double().requires_grad_(True)
        rows = table[idx.long()].double().requires_grad_(True)
        assert float((q[:, None, :] - rows).detach().abs().min()) > 0
        kge._reduce(name, p, q[:, None, :], rows).backward(g.double())
        _, dq, dn = rule(red, query, table[idx.long()], g)
        torch.testing.assert_close(dq, q.grad, rtol=1e-12, atol=1e-13)
        torch.testing.assert_close(dn, rows.grad, rtol=1e-12, atol=1e-13)
        assert float(dn.abs().max()) > 0


def test_ties_regime_has_its_ties():
    for dtype in (F32, F16):
        query, table, idx, g = inputs(dtype, 50, "ties", 37)
        delta = query[:, None, :] - table[idx.long()].float()
        assert bool((delta[:, 0] == 0).all()), "negative 0 is the query row"
        assert bool(((delta[:, 1] != 0).sum(-1) == 1).all()), "negative 1 differs in one column"
        assert bool(((delta[:, 2:] == 0).sum(1)[:, ::3] >= 1).all()), "a third of the columns tie with a negative"
    query, table, idx, g = inputs(F32, 50, "repeats", 37)
    assert int((g == 0).sum()) >= NQ * 37 // 5 and int((idx == 17).sum()) >= NQ * 37 // 3


def test_class_of_every_width():
    """The widths of the table are in the (VEC, IT) class the docstring puts them in, with the last group of 16
    chunks partly filled (but for the two full widths) and 3 / 7 groups at IT 4 / 8."""
    seen = set()
    for (dtype, vec), its in CLASS_WIDTHS.items():
        for it, widths in its.items():
            groups = set()
            for W in widths:
                assert dispatch_class(dtype, W) == [(vec, it, W)]
                nch = W // vec
                assert W % vec == 0 and nch <= 256
                assert (nch % 16 == 0) == ((dtype, W) in FULL_WIDTHS)
                groups.add(-(-nch // 16))
            # (IT 4 of the VEC 1 classes: 50 and 49 scalars fill 4 groups, 34 and 33 leave the fourth empty)
            assert groups == {1: {1}, 2: {2}, 4: {3, 4} if vec == 1 else {3}, 8: {7}, 16: {16}}[it]
            seen.add((dtype, vec, it))
    assert len(seen) == 25  # every (T, VEC, IT) by_it can take
    for (dtype, W), windows in WINDOW_WIDTHS.items():
        assert [c for _, _, c in dispatch_class(dtype, W)] == windows
    # the header's limits: f32 1024 (W % 4 == 0) else 256; f16 2048 (W % 8 == 0), 512 (W % 2 == 0), else 256
    for dtype, W, n in [(F32, 1024, 1), (F32, 1028, 2), (F32, 255, 1), (F32, 258, 2), (F16, 2048, 1), (F16, 2056, 2),
                        (F16, 510, 1), (F16, 514, 2), (F16, 255, 1), (F16, 257, 2)]:
        assert len(dispatch_class(dtype, W)) == n


def test_items_per_query_of_every_shape():
    """Host arithmetic: 5 x 37 -> nb = 8, 5 items (the last of 5 negatives); 5 x 7 -> one item; 4096 x 259 at W = 8
    -> two items, i.e. nb = 256 (nb is a power of two <= 256)."""
    for dtype, W in WIDTHS:
        desc = nat.make_desc(nat.TRANSE, 1, torch.empty((0, W), dtype=dtype), W)
        assert items_of(desc, NQ, 37) == 5 and items_of(desc, NQ, 7) == 1
    for dtype in (F32, F16):
        desc = nat.make_desc(nat.TRANSE, 1, torch.empty((0, 8), dtype=dtype), 8)
        assert items_of(desc, BIG_NQ, BIG_NNEG) == 2 and items_of(desc, BIG_NQ, 512) == 2


# ============================================================================================ 1. forward, backward
def nan(*shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def padded(x, ld, dev):
    out = nan(x.shape[0], ld, dev=dev)
    out[:, : x.shape[1]] = x.to(dev)
    return out


def status(name, dev, *args):
    """Return code of an entry point (for the calls that must be refused); `nat._launch` raises instead."""
    return getattr(nat.load(), name)(*args, nat._stream(dev))


def forward(dev, desc, query, table, idx, n_neg, ld, launch=nat._launch):
    out = nan(query.shape[0], ld, dev=dev)
    rc = launch("bess_neg_score_pertriple_fwd", dev, ctypes.byref(desc), query.data_ptr(), query.shape[0],
                table.data_ptr(), idx.data_ptr(), n_neg, out.data_ptr(), ld)
    torch.cuda.synchronize()
    return rc, out


def backward(dev, desc, query, table, idx, n_neg, d_out, ld, want_dq=True, want_dn=True, dn_rows=None,
             launch=nat._launch):
    """bess_neg_score_pertriple_bwd on NaN-filled outputs; d_out [nq, ld] padded."""
    nq, W = query.shape
    dq = nan(nq, W, dev=dev) if want_dq else None
    dn = nan(dn_rows if dn_rows else nq * n_neg, W, dev=dev) if want_dn else None
    rc = launch("bess_neg_score_pertriple_bwd", dev, ctypes.byref(desc), query.data_ptr(), nq, table.data_ptr(),
                idx.data_ptr(), n_neg, d_out.data_ptr(), ld, dq.data_ptr() if want_dq else None,
                dn.data_ptr() if want_dn else None)
    torch.cuda.synchronize()
    return rc, dq, dn


def check_d_neg(red, regime, what, dn, ref64, ref32):
    if red in ("dot", "complex", "l1", "rotate_l1"):  # one fp32 product of two floats | +-g or 0: exact
        assert torch.equal(dn.cpu(), ref64[2].float()), f"{what}: d_neg differs from the exact value"
    else:
        check(1, "d_neg", regime, what + " d_neg", dn, ref64[2], ref32[2])


def pertriple_against_float64(dev, dtype, W, red, regime, n_neg, nq=NQ):
    query, table, idx, g = inputs(dtype, W, regime, n_neg, nq)
    ref64, ref32 = references(dtype, W, regime, n_neg, red, nq)
    what = f"{tname(dtype)} W={W} {red} {regime} {nq}x{n_neg}"
    q, t, i = query.to(dev), table.to(dev), idx.reshape(-1).contiguous().to(dev)
    desc = make_desc(red, table)  # reserved[1] = 0: the plain forward
    ld = n_neg + 3
    go = padded(g, ld, dev)
    wide_lp = len(dispatch_class(dtype, W)) > 1 and red in ("l2", "l3")
    if wide_lp:  # refused, and nothing written
        rc, out = forward(dev, desc, q, t, i, n_neg, ld, launch=status)
        assert rc == EUNSUPPORTED and bool(torch.isnan(out).all())
        rc, dq, dn = backward(dev, desc, q, t, i, n_neg, go, ld, launch=status)
        assert rc == EUNSUPPORTED and bool(torch.isnan(dq).all()) and bool(torch.isnan(dn).all()), what
        return
    _, out = forward(dev, desc, q, t, i, n_neg, ld)
    assert bool(torch.isnan(out[:, n_neg:]).all()), f"{what}: columns past n_neg written"
    check(1, "scores", regime, what + " scores", out[:, :n_neg], ref64[0], ref32[0])
    if regime == "perm":  # d_neg stored at row neg_idx[k] of a row-space matrix; rows not named stay as they were
        by_row = nat.copy_desc(desc)
        by_row.reserved[0] |= nat.FLAG_DNEG_BY_ROW
        _, dq, dn = backward(dev, by_row, q, t, i, n_neg, go, ld, dn_rows=table.shape[0])
        named = torch.zeros(table.shape[0], dtype=torch.bool, device=dev)
        named[i.long()] = True
        assert bool(torch.isnan(dn[~named]).all()), f"{what}: a row that the list does not name was written"
        check(1, "d_query", regime, what + " d_query (by row)", dq, ref64[1], ref32[1])
        check_d_neg(red, regime, what + " (by row)", dn[i.long()], ref64, ref32)
    _, dq, dn = backward(dev, desc, q, t, i, n_neg, go, ld)
    check(1, "d_query", regime, what + " d_query", dq, ref64[1], ref32[1])
    check_d_neg(red, regime, what, dn, ref64, ref32)
    zero = (g == 0).reshape(-1)
    if bool(zero.any()):
        assert float(dn.cpu()[zero].abs().max()) == 0.0, f"{what}: d_neg rows of d_out == 0 are not zeros"
    _, dq_only, none = backward(dev, desc, q, t, i, n_neg, go, ld, want_dn=False)
    assert none is None
    check(1, "d_query", regime, what + " d_query (d_neg = NULL)", dq_only, ref64[1], ref32[1])
    _, none, dn_only = backward(dev, desc, q, t, i, n_neg, go, ld, want_dq=False)
    assert none is None and torch.equal(dn_only, dn), f"{what}: d_neg of the call with d_query = NULL differs"
    if red in ("dot", "complex"):  # the header: the candidate rows are not read at all
        poison = torch.full_like(t, float("nan"))
        _, _, dn_p = backward(dev, desc, q, poison, i, n_neg, go, ld, want_dq=False)
        assert torch.equal(dn_p, dn), f"{what}: d_neg with d_query = NULL depends on the candidate rows"


@gpu
@pytest.mark.parametrize("red", list(REDS))
@pytest.mark.parametrize("case", WIDTHS, ids=wid)
def test_forward_and_backward_equal_float64(dev, case, red):
    dtype, W = case
    for regime in REGIMES:
        for n_neg in N_NEGS:
            desc = make_desc(red, torch.empty((0, W), dtype=dtype))
            assert items_of(desc, NQ, n_neg) == (5 if n_neg == 37 else 1)
            pertriple_against_float64(dev, dtype, W, red, regime, n_neg)


@gpu
@pytest.mark.parametrize("case", COMPLEX_CASES, ids=wid)
def test_complex_scorers_equal_float64(dev, case):
    """RotatE (rel_width = W / 2, sign -1) and ComplEx (sign +1) descriptors: the same reductions."""
    dtype, W, red = case
    for regime in REGIMES:
        pertriple_against_float64(dev, dtype, W, red, regime, 37)
    bad = nat.make_desc(nat.ROTATE, 1, torch.empty((0, W), dtype=dtype), W)  # check_desc: RotatE relations are W / 2 wide
    out = ctypes.c_int32(0)
    assert nat.load().bess_neg_pertriple_sweep(ctypes.byref(bad), 4, 4, ctypes.byref(out)) == -1


@gpu
@pytest.mark.parametrize("dtype", [F32, F16], ids=tname)
def test_items_of_256_negatives(dev, dtype):
    """W = 8 at 4096 queries x 259 negatives: nb stays 256, two items per query (256 + 3 negatives)."""
    for red in REDS:
        desc = make_desc(red, torch.empty((0, 8), dtype=dtype))
        assert items_of(desc, BIG_NQ, BIG_NNEG) == 2
        pertriple_against_float64(dev, dtype, 8, red, "normal", BIG_NNEG, nq=BIG_NQ)


# ============================================================================================ 2. segments
def segments(dev, desc, query, table, n_neg, d_out, ld, seg, launch=nat._launch):
    """bess_neg_pertriple_grad_segments into a NaN-filled [max_seg, W]; d_out [nq, ld] padded."""
    W = int(table.shape[1])
    grad = nan(seg.max_seg, W, dev=dev)
    if seg.long_grad is None or seg.long_grad.shape[1] != W:
        seg.long_grad = torch.zeros((seg.long_cap, W), dtype=torch.float32, device=dev)
    rc = launch("bess_neg_pertriple_grad_segments", dev, ctypes.byref(desc), query.data_ptr(), query.shape[0],
                table.data_ptr(), n_neg, d_out.data_ptr(), ld, seg.refs.data_ptr(), seg.seg_rows.data_ptr(),
                seg.seg_offsets.data_ptr(), seg.n_seg.data_ptr(), seg.max_seg, grad.data_ptr(), 0.0,
                seg.long_segs.data_ptr(), seg.long_cap, seg.long_grad.data_ptr(), seg.long_count.data_ptr())
    torch.cuda.synchronize()
    return rc, grad


def segments_against_float64(dev, dtype, W, red, regime, n_neg, nq=NQ, query=None, table=None, idx=None, g=None,
                             atomic_rows=0):
    """grad_seg == zeros(M, W, float64).index_add_(0, idx, d_neg64) at the unique rows; two runs bitwise identical
    (but for the `atomic_rows` rows with more than SEGMENT_CAP references, summed with float atomics)."""
    if query is None:
        query, table, idx, g = inputs(dtype, W, regime, n_neg, nq)
        ref64, ref32 = references(dtype, W, regime, n_neg, red, nq)
        dn64, dn32 = ref64[2], ref32[2]
    else:
        dn64, dn32 = (rule(red, query, table[idx.long()], g, dt)[2].reshape(nq * n_neg, W)
                      for dt in (torch.float64, torch.float32))
    what = f"{tname(dtype)} W={W} {red} {regime} {nq}x{n_neg} segments"
    M = table.shape[0]
    flat = idx.reshape(-1).long()
    q, t, i = query.to(dev), table.to(dev), idx.reshape(-1).contiguous().to(dev)
    desc = make_desc(red, table)
    ld = n_neg + 3
    go = padded(g, ld, dev)
    seg = nat.SegmentIndex(i, M)
    uniq, counts = torch.unique(flat, return_counts=True)
    n_seg = int(seg.n_seg.item())
    assert n_seg == uniq.numel() and torch.equal(seg.seg_rows[:n_seg].cpu().long(), uniq)
    assert int((counts > nat.SEGMENT_CAP).sum()) == atomic_rows
    if len(dispatch_class(dtype, W)) > 1 and red in ("l2", "l3"):
        rc, grad = segments(dev, desc, q, t, n_neg, go, ld, seg, launch=status)
        assert rc == EUNSUPPORTED and bool(torch.isnan(grad).all()), what
        return
    _, g1 = segments(dev, desc, q, t, n_neg, go, ld, seg)
    _, g2 = segments(dev, desc, q, t, n_neg, go, ld, nat.SegmentIndex(i, M))
    assert bool(torch.isnan(g1[n_seg:]).all()), f"{what}: rows past n_seg written"
    short = (counts <= nat.SEGMENT_CAP).to(dev)
    assert torch.equal(g1[:n_seg][short], g2[:n_seg][short]), f"{what}: two runs differ"
    want64 = torch.zeros(M, W, dtype=torch.float64).index_add_(0, flat, dn64)[uniq]
    want32 = torch.zeros(M, W, dtype=torch.float32).index_add_(0, flat, dn32)[uniq]
    check(2, "grad_seg", regime, what, g1[:n_seg], want64, want32)
    check(2, "grad_seg", regime, what + " (second run)", g2[:n_seg], want64, want32)


@gpu
@pytest.mark.parametrize("red", list(REDS))
@pytest.mark.parametrize("case", WIDTHS, ids=wid)
def test_segments_equal_float64_index_add(dev, case, red):
    dtype, W = case
    for regime in ("normal", "ties", "repeats"):
        segments_against_float64(dev, dtype, W, red, regime, 37)


@gpu
@pytest.mark.parametrize("case", COMPLEX_CASES, ids=wid)
def test_segments_of_the_complex_scorers(dev, case):
    dtype, W, red = case
    segments_against_float64(dev, dtype, W, red, "ties", 37)


@gpu
@pytest.mark.parametrize("case", [(F32, 388), (F16, 264)], ids=wid)
def test_segments_hot_row(dev, case):
    """One row with 520 of 16 x 37 references (three slices of the long-segment kernels) at IT 8 / IT 4; the other rows
    stay on the per-row pass."""
    dtype, W = case
    nq, n_neg = 16, 37
    assert dispatch_class(dtype, W)[0][1] >= 4
    gen = torch.Generator().manual_seed(W)
    table = (torch.randn(ROWS, W, generator=gen) * 0.3).to(dtype)
    query = torch.randn(nq, W, generator=gen) * 0.3
    g = torch.randn(nq, n_neg, generator=gen)
    idx = torch.randint(0, ROWS, (nq * n_neg,), generator=gen)
    idx[torch.randperm(nq * n_neg, generator=gen)[:520]] = 41
    idx = idx.reshape(nq, n_neg).to(torch.int32)
    assert int((idx == 41).sum()) > 2 * nat.SEGMENT_CAP
    for red in REDS:
        segments_against_float64(dev, dtype, W, red, "hot", n_neg, nq=nq, query=query, table=table, idx=idx, g=g,
                                 atomic_rows=1)


@gpu
@pytest.mark.parametrize("case", [(F32, 512, 2), (F16, 512, 2), (F32, 768, 1)], ids=wid)
def test_segments_l2_windows(dev, case):
    """4096 queries: the query matrix is more than an L2 (4 MiB), so DOT and L1 are reduced in column windows of at most
    4 MiB of queries - two of them side by side in one launch (n_conc = 2: W = 512), or one after the other (n_conc = 1:
    W = 768, three windows of 256); the p = 2 distance takes the whole row."""
    dtype, W, n_conc = case
    nq, n_neg = 4096, 2
    unit = 16 * dispatch_class(dtype, W)[0][0]
    fit = (4 << 20) // (nq * 4)
    assert nq * W * 4 > (4 << 20) and fit >= unit
    win = fit // unit * unit
    assert (n_conc == 2) == (2 * win == W and W % (2 * unit) == 0)  # the host code's rule (csrc/segments.hip)
    gen = torch.Generator().manual_seed(W + n_conc)
    table = (torch.randn(ROWS, W, generator=gen) * 0.3).to(dtype)
    query = torch.randn(nq, W, generator=gen) * 0.3
    g = torch.randn(nq, n_neg, generator=gen)
    idx = torch.randint(0, ROWS, (nq, n_neg), generator=gen).to(torch.int32)
    for red in ("dot", "l1", "l2"):
        segments_against_float64(dev, dtype, W, red, "windows", n_neg, nq=nq, query=query, table=table, idx=idx, g=g)


# ============================================================================================ 3. csrc/prepare.hip
PREP_SCORERS = [("TransE", 1), ("TransE", 2), ("RotatE", 1), ("RotatE", 2), ("DistMult", 0), ("ComplEx", 0)]
PREP_D = [3, 50, 128, 1000]
N_TRIPLE, N_REL, N_ENT = 9, 4, 23
SIDES = {"t": nat.CORRUPT_TAIL, "h": nat.CORRUPT_HEAD}


@functools.lru_cache(maxsize=None)
def prepare_inputs(name, p, dtype, d):
    """9 triples over 4 relations (each used at least twice) and 23 entities; smooth values; for p = 1 every component of
    query - tail is at least 0.02 away from 0.  Never written to."""
    gen = torch.Generator().manual_seed(1000 * d + 10 * p + len(name) + (5 if dtype == F16 else 0))
    W, Wr = kge.entity_width(name, d), kge.relation_width(name, d)
    ent = (torch.randn(N_ENT, W, generator=gen) * 0.5).to(dtype)
    rel = (torch.randn(N_REL, Wr, generator=gen) * 0.5).to(dtype)
    perm = torch.randperm(N_ENT, generator=gen)
    hidx, tidx = perm[:N_TRIPLE].to(torch.int32), perm[N_TRIPLE: 2 * N_TRIPLE].to(torch.int32)  # distinct rows
    rid = torch.tensor([0, 1, 2, 3, 0, 1, 2, 3, 1], dtype=torch.int32)
    if p == 1:
        x = kge.query(name, "t", ent[hidx.long()].double(), rel[rid.long()].double()) - ent[tidx.long()].double()
        push = torch.where(x.abs() < 0.05, torch.where(x < 0, -0.1, 0.1), 0.0)
        ent[tidx.long()] = (ent[tidx.long()].double() - push).to(dtype)
        x = kge.query(name, "t", ent[hidx.long()].double(), rel[rid.long()].double()) - ent[tidx.long()].double()
        assert float(x.abs().min()) > 0.02
    d_out = torch.randn(N_TRIPLE, generator=gen)
    d_query = torch.randn(N_TRIPLE, W, generator=gen)
    d_rel0 = torch.randn(N_REL, Wr, generator=gen)
    return ent, rel, hidx, tidx, rid, d_out, d_query, d_rel0


@functools.lru_cache(maxsize=None)
def prepare_references(name, p, dtype, d, ftype):
    """Every output of the six entry points from `oracle.kge` evaluated in `ftype` (float64: the reference; float32:
    the restatement whose error sizes the ill-conditioned cases), gradients by autograd."""
    ent, rel, hidx, tidx, rid, d_out, d_query, d_rel0 = prepare_inputs(name, p, dtype, d)
    h = ent[hidx.long()].to(ftype).requires_grad_(True)
    t = ent[tidx.long()].to(ftype).requires_grad_(True)
    R = rel.to(ftype).requires_grad_(True)
    score = kge.score_triple(name, p, h, R, rid, t)
    out = {"score": score.detach()}
    ls = (score * d_out.to(ftype)).sum()
    gh, gt, gr = torch.autograd.grad(ls, (h, t, R), retain_graph=True)
    out["score_bwd"] = (gh, gt, d_rel0.to(ftype) + gr)
    for side in SIDES:
        x = h if side == "t" else t
        qy = kge.query(name, side, x, R[rid.long()])
        out["query", side] = qy.detach()
        lq = (qy * d_query.to(ftype)).sum()
        gx, gr = torch.autograd.grad(lq, (x, R), retain_graph=True)
        out["query_bwd", side] = (gx, d_rel0.to(ftype) + gr)
        gh, gt, gr = torch.autograd.grad(ls + lq, (h, t, R), retain_graph=True)  # the two gradients summed
        out["query_triple_bwd", side] = (gh, gt, d_rel0.to(ftype) + gr)
    return out


@gpu
@pytest.mark.parametrize("d", PREP_D)
@pytest.mark.parametrize("dtype", [F32, F16], ids=tname)
@pytest.mark.parametrize("name,p", PREP_SCORERS)
def test_query_and_positive_score_kernels_equal_float64(dev, name, p, dtype, d):
    ent, rel, hidx, tidx, rid, d_out, d_query, d_rel0 = prepare_inputs(name, p, dtype, d)
    r64 = prepare_references(name, p, dtype, d, torch.float64)
    r32 = prepare_references(name, p, dtype, d, torch.float32)
    W, Wr = kge.entity_width(name, d), kge.relation_width(name, d)
    desc = nat.make_desc(dict(TransE=0, RotatE=1, DistMult=2, ComplEx=3)[name], max(p, 1), ent, Wr)
    E, R, hi, ti, ri = ent.to(dev), rel.to(dev), hidx.to(dev), tidx.to(dev), rid.to(dev)
    go, gq = d_out.to(dev), d_query.to(dev)
    sources = {"indexed": (nat.RowSource(E, hi), nat.RowSource(E, ti)),
               "direct": (nat.RowSource(E[hi.long()].contiguous()), nat.RowSource(E[ti.long()].contiguous()))}

    def ok(quantity, what, got, key, part=None):
        w64, w32 = (r64[key], r32[key]) if part is None else (r64[key][part], r32[key][part])
        check(3, quantity, "smooth", f"{name} p={p} {tname(dtype)} d={d} {what}", got, w64.detach(), w32.detach())

    for how, (head, tail) in sources.items():
        ok("score", f"{how} score_triple_fwd", nat.score_triple_fwd(desc, head, tail, R, ri), "score")
        d_rel = d_rel0.to(dev).clone()  # non-zero on entry: the call accumulates
        dh, dt = nat.score_triple_bwd(desc, head, tail, R, ri, go, d_rel)
        for part, got in enumerate((dh, dt, d_rel)):
            ok("score_bwd", f"{how} score_triple_bwd[{part}]", got, "score_bwd", part)
        for side, code in SIDES.items():
            x = head if side == "t" else tail
            ok("query", f"{how} {side} query_fwd", nat.query_fwd(desc, code, x, R, ri), ("query", side))
            d_rel = d_rel0.to(dev).clone()
            dx = nat.query_bwd(desc, code, x, R, ri, gq, d_rel)
            for part, got in enumerate((dx, d_rel)):
                ok("query_bwd", f"{how} {side} query_bwd[{part}]", got, ("query_bwd", side), part)
            qy, sc = nat.query_triple_fwd(desc, code, head, tail, R, ri)
            ok("query", f"{how} {side} query_triple_fwd query", qy, ("query", side))
            ok("score", f"{how} {side} query_triple_fwd score", sc, "score")
            d_rel = d_rel0.to(dev).clone()
            dh, dt = nat.query_triple_bwd(desc, code, head, tail, R, ri, go, gq, d_rel)
            for part, got in enumerate((dh, dt, d_rel)):
                ok("query_triple_bwd", f"{how} {side} query_triple_bwd[{part}]", got, ("query_triple_bwd", side), part)
