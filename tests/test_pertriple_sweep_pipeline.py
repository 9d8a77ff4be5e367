"""The software-pipelined sweep of the row-ordered per-triple forward (K5s, `sweep_share` of csrc/neg_pertriple.hip).

A wave of K5s walks its part of a workgroup's share (n = about an eighth of the block's pairs, sorted by row) in steps
of 16 * UNROLL entries, 4 * UNROLL of them its own; the rows of step i + 1 are in flight while step i is scored, in two
register sets that take turns, two steps per trip of the loop and one or two steps after it.  Lanes past the end of a
row that does not fill the register layout (W < IT * 16 * VEC) load its last chunk and score zeros, and p-norms other
than 1 and 2 keep the loop that is not pipelined.  What can go wrong is decided by n against the step, by the row class
(table type, VEC, IT -> UNROLL = 4, 2, 1 for IT * VEC <= 16, <= 32, more) and by whether the row fills the layout, so
the cases are:

  share lengths, for one class of every UNROLL: 8 queries x n negatives make one block whose eight shares all have
      exactly n entries - n below the first entry of some waves (they run no step), one step, two steps, three steps
      and that +- 1, four steps + 1; 1 x 4 and 1 x 7 pairs on a table of one row (empty shares beside shares of one);
  blocks: a last query block with fewer queries than the others and n_neg that is no multiple of the chunk;
  rows: ids that name row 0 and the table's last row, every id on the last row, every id on row 0;
  classes: every (table type, VEC, IT) with a partly filled last group, and the full width of every class that has
      one (f32 VEC 4, f16 VEC 8: a full row of a narrower vector is a row of the wider one), each with DOT, p = 1, 2, 3;
  a leading dimension past n_neg.

Every case asserts that the sizes take K5s, scores the same operands with desc.reserved[1] = rows (K5s) and = 0 (K5)
into NaN-filled outputs, compares the two with torch.equal and K5s with the float64 rule at the bounds of
test_pertriple_kernels.py (`check`).  `test_every_shape_takes_the_sweep` states the dispatch condition
n_query * n_neg >= 4 * rows for all of them without a device."""

import ctypes

import pytest
import torch

from besskge import _native as nat
from test_pertriple_kernels import CLASS_WIDTHS, F16, F32, REDS, check, dispatch_class, make_desc, rule, tname

gpu = pytest.mark.gpu
ALL_REDS = ("dot", "l1", "l2", "l3")

# (table type, W) of one class per UNROLL, full rows: f32 VEC 4 with IT 1 (UNROLL 4), IT 8 (2: the headline's), IT 16 (1)
UNROLL_CLASSES = {4: (F32, 64), 2: (F32, 512), 1: (F32, 1024)}


def share_lengths(unroll):
    step = 16 * unroll
    return [unroll + 1, 5 * unroll, 9 * unroll + 1, step, step + 1, 2 * step, 3 * step - 1, 3 * step, 3 * step + 1,
            4 * step + 1]


def rows_for(nq, n_neg):
    return max(1, nq * n_neg // 4)


# name -> (dtype, W, nq, n_neg, rows, reds, ids, ld)
CASES = {}
for _u, (_dt, _W) in UNROLL_CLASSES.items():
    for _n in share_lengths(_u):
        CASES[f"share-u{_u}-n{_n}"] = (_dt, _W, 8, _n, rows_for(8, _n), ALL_REDS, "ends", None)
    CASES[f"share-u{_u}-empty-1x4"] = (_dt, _W, 1, 4, 1, ("dot", "l2"), "uniform", None)
    CASES[f"share-u{_u}-empty-1x7"] = (_dt, _W, 1, 7, 1, ("l1", "l3"), "uniform", None)
CASES["blocks-f32-64"] = (F32, 64, 40, 300, 1000, ALL_REDS, "ends", None)  # qb 32: blocks of 32 and 8; kc 256: 256 + 44
CASES["blocks-f32-512"] = (F32, 512, 33, 257, 2000, ("dot", "l2"), "ends", None)  # 32 + 1 queries, 256 + 1 negatives
CASES["blocks-f16-1024"] = (F16, 1024, 17, 515, 2000, ("dot", "l1"), "ends", None)  # qb 16: 16 + 1; kc 512: 512 + 3
CASES["one-row-last"] = (F32, 512, 16, 128, 500, ALL_REDS, "last", None)
CASES["one-row-first"] = (F16, 200, 16, 100, 400, ALL_REDS, "first", None)
CASES["ld-f32-512"] = (F32, 512, 8, 100, 200, ("dot", "l1"), "ends", 107)
CASES["ld-f16-66"] = (F16, 66, 24, 150, 900, ("l2", "l3"), "ends", 151)
for (_dt, _vec), _its in CLASS_WIDTHS.items():
    for _it, _ws in _its.items():
        CASES[f"class-{tname(_dt)}-v{_vec}-it{_it}-partial"] = (_dt, _ws[0], 8, 200, 97, ALL_REDS, "ends", None)
        if _vec == (4 if _dt == F32 else 8):
            CASES[f"class-{tname(_dt)}-v{_vec}-it{_it}-full"] = (_dt, 16 * _it * _vec, 8, 200, 97, ALL_REDS, "ends", None)


def operands(name):
    dtype, W, nq, n_neg, rows, _, ids, _ = CASES[name]
    gen = torch.Generator().manual_seed(sorted(CASES).index(name))
    table = (torch.randn(rows, W, generator=gen) * 0.3).to(dtype)
    query = torch.randn(nq, W, generator=gen) * 0.3
    idx = torch.randint(0, rows, (nq, n_neg), generator=gen, dtype=torch.int32)
    if ids == "ends":  # row 0 and the last row, at both ends of the list and in its middle
        flat = idx.view(-1)
        flat[0], flat[-1] = rows - 1, 0
        flat[flat.numel() // 2] = rows - 1
        flat[flat.numel() // 3] = 0
    elif ids == "last":
        idx.fill_(rows - 1)
    elif ids == "first":
        idx.fill_(0)
    return query, table, idx


def scores(red, query, gathered, dtype):
    """The forward part of test_pertriple_kernels.rule (which also builds the gradients, [S, N, W] each)."""
    p = REDS[red][2]
    q, e = query.to(dtype)[:, None, :], gathered.to(dtype)
    if red == "dot":
        return (q * e).sum(-1)
    delta = (q - e).abs()
    return -delta.sum(-1) if p == 1 else -delta.pow(p).sum(-1).pow(1.0 / p)


def test_scores_restate_the_rule():
    query, table, idx = operands("class-f16-v2-it2-partial")
    gathered = table[idx.long()]
    for red in ALL_REDS:
        for dt in (torch.float64, torch.float32):
            assert torch.equal(scores(red, query, gathered, dt), rule(red, query, gathered, torch.zeros(idx.shape), dt)[0])


def test_cases_cover_their_classes():
    for name, (dtype, W, *_rest) in CASES.items():
        if not name.startswith("class-"):
            continue
        _, t, v, it, kind = name.split("-")
        (vec, its, cols), = dispatch_class(dtype, W)
        assert (tname(dtype), f"v{vec}", f"it{its}") == (t, v, it), name
        assert (cols == its * 16 * vec) == (kind == "full"), name
    for unroll, (dtype, W) in UNROLL_CLASSES.items():
        (vec, its, cols), = dispatch_class(dtype, W)
        epl = its * vec
        assert unroll == (4 if epl <= 16 else 2 if epl <= 32 else 1) and cols == its * 16 * vec


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_shape_takes_the_sweep(name):
    dtype, W, nq, n_neg, rows, reds, _, ld = CASES[name]
    assert nq * n_neg >= 4 * rows and (ld is None or ld > n_neg)
    for red in reds:
        d = make_desc(red, torch.empty((0, W), dtype=dtype))
        d.reserved[1] = rows
        assert nat.pertriple_sweep(d, nq, n_neg), f"{name} {red}"


def launch(dev, desc, rows, query, table, idx, n_neg, ld):
    d = nat.copy_desc(desc)
    d.reserved[1] = rows
    nq = query.shape[0]
    out = torch.full((nq, ld), float("nan"), dtype=torch.float32, device=dev)
    nat._launch("bess_neg_score_pertriple_fwd", dev, ctypes.byref(d), query.data_ptr(), nq, table.data_ptr(),
                idx.data_ptr(), n_neg, out.data_ptr(), ld)
    torch.cuda.synchronize()
    return out


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_pipelined_sweep_equals_plain_and_float64(name):
    dtype, W, nq, n_neg, rows, reds, _, ld = CASES[name]
    dev = torch.device("cuda", 0)
    query, table, idx = operands(name)
    gathered = table[idx.long()]
    ld = n_neg if ld is None else ld
    q_d, t_d, i_d = query.to(dev), table.to(dev), idx.to(dev).contiguous()
    for red in reds:
        desc = make_desc(red, table)
        known = nat.copy_desc(desc)
        known.reserved[1] = rows
        assert nat.pertriple_sweep(known, nq, n_neg), "the case must take the row-ordered kernel"
        plain = launch(dev, desc, 0, q_d, t_d, i_d, n_neg, ld)
        swept = launch(dev, desc, rows, q_d, t_d, i_d, n_neg, ld)
        what = f"{name} {red}"
        assert not torch.isnan(swept[:, :n_neg]).any(), f"{what}: a score was not written"
        assert torch.isnan(swept[:, n_neg:]).all() and torch.isnan(plain[:, n_neg:]).all(), f"{what}: stray store"
        assert torch.equal(plain[:, :n_neg], swept[:, :n_neg]), what
        ref64, ref32 = scores(red, query, gathered, torch.float64), scores(red, query, gathered, torch.float32)
        check("sweep", "scores", name, what, swept[:, :n_neg].cpu(), ref64, ref32)
