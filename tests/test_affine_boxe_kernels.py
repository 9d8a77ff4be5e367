"""The shared-candidate kernels of the affine scorers (csrc/affine.hip: `k_normalize_rows`, `k_normalize_rows_bwd`,
`k_aff_shared_fwd` in its dense, counting and diagonal forms, `k_aff_shared_bwd` on both sides) and BoxE's kernels
(csrc/boxe.hip: `k_box_fwd` storing and counting, `k_box_bwd`, shared and per-triple) against float64, through the
`_native` wrappers on query matrices made directly ([S, (n_part + 1) d] = [U | V | R], [S, 6 d] = [S_0 | C_0 | H_0 | S_1
| C_1 | H_1]), in every class their host code selects.  The other tests of these kernels prove them consistent with
each other (test_fused_ranks_scorers.py) or compare small shapes with the fp32 oracle; here every case states the class
it is meant to reach and asserts it with a restatement of the planner, so a change of a planner fails the case instead
of silently testing less.

  0. on the CPU (no device): the rules of the headers of affine.hip / boxe.hip in torch float64 (`hat_rule`,
     `affine_rule`, `boxe_rule`; gradients by float64 autograd, written so that sgn(0) = 0 and the gradient at zero
     norm is 0) == `oracle.kge.score_candidates` for every member of AFFINE_VARIANTS / BOXE_VARIANTS on queries built by
     the scorers' `_uvr` / `_boxes`; the planners (`bwd_plan`, `table_tiles`, `nat.affine_count_chunk_rows`,
     `negatives_per_item`) at every shape below; the conditions of the regimes (gaps of the count thresholds, share of
     all-inside slots, no |dist - H| < 1e-5, the ties and the exact elements);
  1. `normalize_rows` / `normalize_rows_bwd`: f32 and f16, n_part 1 | 2, d 6 | 64 | 70 | 260, 13 rows, indexed and
     dense, normalize off (bit for bit), a zero row, an fp32 row of norm 1e-13 (clamped: linear) and one of 1e-11;
  2. dense forward: n_part 1 | 2, p 1 | 2 | 3, d 6 | 20 | 70 | 256 at 130 x 197 and 769 x 65, normalised or not, both
     table types;
  3. backward, both `XQ` sides by kernel name: 70 x 100 (split 1 | 1), 150 x 333 at d 20 | 70 | 132 (query side 4
     slices of 96, the last 45; candidate side 2 of 80, the last 70; 1, 2 and 3 column tiles); regimes "normal" (randn * 0.5), "apart" (the same with no |delta| below 1e-6, where fp32 may take the other sign at
     p = 1 and the restatement's error would size the bound), "ties"
     (delta == 0 in a third of the columns, one query at distance 0) and "exact" (integers, p = 1: `torch.equal`);
     d_query and d_neg start as NaN (`nan_outputs`), so a missing clear shows;
  4. table form: counts at tiles 1 (130 x 197), 2 (1,093 x 15,589) and 8 (4,101 x 16,037, last group of 3), two
     candidate chunks (70 x 8,293, two parts of 512 fp32: 8,192 rows a chunk; `excl` on the chunk's edges), exact
     counts of `>` and `==` on integer scores with `round_f16` too, and pairs == float64;
  5. BoxE, (tanh, per_dim) x p 1 | 2 | 3 x f32 | f16: storing form, backward (shared: atomic d_neg and d_query;
     per-triple) at nb 8 (5 x 9, 70 x 130), 16 (130 x 1,030) and 64 (130 x 4,100, last item of 4); counts at the same
     shapes and at nb 256 (130 x 16,133), all 24 combinations at each; regimes "normal", "inside" (a quarter to three quarters of the slots all-inside),
     "exact" (dyadic boxes, p = 1, no tanh: `torch.equal`) and a query whose candidates sit on the centre (zero norm).

Counts are compared for equality: each row's threshold is the midpoint of a gap between two adjacent float64 scores
that is wider than twice a band of 4 x the fp32 restatement's largest error on those inputs, so no fp32 evaluation
within that band can move a candidate across it.  Everything else goes through `check` of test_pertriple_kernels.py:
rtol 1e-4, atol max(1e-5, 2e-6 max|ref|), or 4 x the fp32 restatement's own error where that is outside the bound.  No
bound depends on a kernel's output.  Large references are evaluated by torch in float64 on the device when there is
one.  Classes, shapes and measured errors: DESIGN.md, section 26."""

import contextlib
import functools

import pytest
import torch

from besskge import _native as nat
from besskge._native import RowSource
from oracle import kge

from test_affine_boxe_row_classes import affine_desc, boxe_desc
from test_pertriple_kernels import MEASURED, check
from test_tile_dispatch_classes import kernel_launched, launched

gpu = pytest.mark.gpu
F16, F32, F64 = torch.float16, torch.float32, torch.float64
NORM_EPS = 1e-12
PS = (1, 2, 3)
BOX_SETTINGS = [(True, True), (True, False), (False, True), (False, False)]  # (tanh, per_dim)


def tname(dtype):
    return "f32" if dtype == F32 else "f16"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda", 0)


def ref_dev():
    """Where torch evaluates the float64 references: the device when there is one (the large shapes), else the CPU."""
    return torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")


def cdiv(a, b):
    return -(-a // b)


# ======================================================================================== 0. rules and planners
def safe_root(s, p):
    """s^(1/p) for s >= 0 with gradient 0 (not inf) at s == 0: the kernels' `lp_inv` convention."""
    pos = s > 0
    return torch.where(pos, s, torch.ones_like(s)).pow(1.0 / p) * pos.to(s.dtype)


def lp_norm(x, p):
    """||x||_p over the last dimension; autograd gives sgn(0) = 0 and 0 at zero norm."""
    if p == 1:
        return x.abs().sum(-1)
    return safe_root(x.abs().pow(p).sum(-1), p)


def hat_rule(rows, n_part, normalize, dtype=F64):
    """hat = e / max(||e_part||, 1e-12) per part: (hat [n, W], inv [n, n_part]) in `dtype`."""
    n, W = rows.shape
    x = rows.to(dtype).reshape(n, n_part, W // n_part)
    if not normalize:
        return x.reshape(n, W), torch.ones(n, n_part, dtype=dtype, device=rows.device)
    inv = 1.0 / safe_root((x * x).sum(-1), 2).clamp(min=NORM_EPS)
    return (x * inv[..., None]).reshape(n, W), inv


def affine_rule(q, hat, n_part, p):
    """score = -||U c1 + V c2 + R||_p: q [S, (n_part + 1) d] against hat [N, n_part d] -> [S, N]."""
    S, d = q.shape[0], hat.shape[1] // n_part
    u, c = q.reshape(S, n_part + 1, d), hat.reshape(-1, n_part, d)
    delta = u[:, None, n_part, :]
    for k in range(n_part):
        delta = delta + u[:, None, k, :] * c[None, :, k, :]
    return -lp_norm(delta, p)


def boxe_rule(q, rows, tanh, per_dim, p, parts=False):
    """The BoxE rule of boxe.hip's header: q [S, 6 d] against rows [N, 2 d] (shared) or [S, N, 2 d] -> [S, N].
    parts: (dist - H, all-inside flag per slot) instead."""
    S, d = q.shape[0], q.shape[1] // 6
    qq = q.reshape(S, 1, 2, 3, d)
    e = rows.reshape(1, -1, 2, d) if rows.dim() == 2 else rows.reshape(S, -1, 2, d)
    xp = e + qq[:, :, :, 0]
    if tanh:
        xp = torch.tanh(xp)
    dist, H = (xp - qq[:, :, :, 1]).abs(), qq[:, :, :, 2]
    inside = dist <= H
    if parts:
        return dist - H, inside.all(-1)
    if not per_dim:
        inside = inside.all(-1, keepdim=True)
    B = 1.0 + 2.0 * H
    A = 1.0 / B
    f = torch.where(inside, dist * A, dist * B - H * (B - A))
    return -lp_norm(f, p).sum(-1)


def reference(rule, q, rows, g, dtype, budget=1 << 24):
    """rule(q block, rows) over blocks of queries in `dtype` on `ref_dev()`: (scores, d_query, d_rows) on the CPU
    (gradients None without g).  rows: the exactly converted table rows; `rule` normalises them itself."""
    dv = ref_dev()
    qd = q.to(dv).to(dtype)
    rd = rows.detach().to(dv).to(dtype).clone().requires_grad_(g is not None)
    gd = None if g is None else g.to(dv).to(dtype)
    step = max(1, budget // max(1, rd.numel() // (rd.shape[0] if rd.dim() == 3 else 1)))
    out, dq = [], []
    for a0 in range(0, qd.shape[0], step):
        qb = qd[a0:a0 + step].clone().requires_grad_(g is not None)
        rb = rd[a0:a0 + step] if rd.dim() == 3 else rd
        with torch.set_grad_enabled(g is not None):
            s = rule(qb, rb)
        if g is not None:
            s.backward(gd[a0:a0 + step])
            dq.append(qb.grad)
        out.append(s.detach())
    if g is None:
        return torch.cat(out).cpu(), None, None
    return torch.cat(out).cpu(), torch.cat(dq).cpu(), rd.grad.cpu()


def affine_fn(n_part, normalize, p):
    return lambda q, rows: affine_rule(q, hat_rule(rows, n_part, normalize, q.dtype)[0], n_part, p)


def boxe_fn(tanh, per_dim, p):
    return lambda q, rows: boxe_rule(q, rows, tanh, per_dim, p)


def both(rule, q, rows, g=None):
    """(float64 reference, fp32 restatement) of a rule on the same inputs."""
    return reference(rule, q, rows, g, F64), reference(rule, q, rows, g, F32)


def bwd_plan(nx, ny, d):
    """`aff_bwd_launch`: (split, chunk) of the reduction over ny for nx gradient rows."""
    tiles, split = cdiv(d, 64) * cdiv(nx, 64), 1
    while tiles * split < 1024 and cdiv(ny, split * 2) >= 4 * 16:
        split *= 2
    chunk = cdiv(cdiv(ny, split), 16) * 16
    return cdiv(ny, chunk), chunk


def table_tiles(S, N):
    """`aff_table_launch`: column tiles per workgroup of the counting form."""
    col_tiles, row_tiles, tiles = cdiv(N, 64), cdiv(S, 64), 1
    while tiles < 8 and row_tiles * cdiv(col_tiles, tiles * 2) >= 256 * 8:
        tiles *= 2
    return tiles


def negatives_per_item(n_query, n_neg, nb=64):
    """common.h `negatives_per_item` without row_bytes (BoxE: nb = 64 storing and backward, 256 counting)."""
    while nb > 8 and n_query * cdiv(n_neg, nb) < 256 * 16 * 2:
        nb >>= 1
    return nb


def test_planner_restatements():
    assert bwd_plan(70, 100, 20) == (1, 112) and bwd_plan(100, 70, 20) == (1, 80)
    for d in (20, 70, 132):
        assert bwd_plan(150, 333, d) == (4, 96) and 333 - 3 * 96 == 45  # whole 16-row stages but in the last slice: 45 = 2 x 16 + 13
        assert bwd_plan(333, 150, d) == (2, 80) and 150 - 80 == 70  # ... and 70 = 4 x 16 + 6
    assert table_tiles(130, 197) == 1 and table_tiles(70, 8293) == 1
    assert table_tiles(1093, 15589) == 2 and cdiv(15589, 64) == 244
    assert table_tiles(4101, 16037) == 8 and cdiv(16037, 64) == 251 and 251 % 8 == 3  # the last workgroup breaks early
    assert table_tiles(300, 39963) == 1  # the largest case of the other tests
    assert [negatives_per_item(*s) for s in ((5, 9), (70, 130), (130, 1030), (130, 4100))] == [8, 8, 16, 64]
    assert 4100 % 64 == 4
    assert negatives_per_item(130, 16133, 256) == 256 and 16133 % 256 == 5
    assert [negatives_per_item(s, n, 256) for s, n in ((70, 130), (130, 1030), (130, 4100))] == [8, 16, 64]


def scorer_on_cpu(name, p, dd, n_rel):
    from test_hip_parity import make_scorer

    W, Wr = kge.entity_width(name, dd), kge.relation_width(name, dd)
    return make_scorer(name, p, True, n_rel, dd, torch.zeros(1, 4, W), torch.zeros(n_rel, Wr), torch.device("cpu"))


@pytest.mark.parametrize("name", list(kge.AFFINE_VARIANTS))
def test_affine_rule_equals_the_oracle(name):
    dd, S, N, n_rel = 10, 7, 11, 3
    cfg = kge.AFFINE_VARIANTS[name]
    gen = torch.Generator().manual_seed(len(name) + dd)
    W, Wr = kge.entity_width(name, dd), kge.relation_width(name, dd)
    n_part = W // dd
    ent, cand, rel = (torch.randn(n, w, generator=gen, dtype=F64) for n, w in ((S, W), (N, W), (n_rel, Wr)))
    rid = torch.randint(n_rel, (S,), generator=gen)
    for p in PS:
        fn = scorer_on_cpu(name, p, dd, n_rel)
        for side, code in (("t", nat.CORRUPT_TAIL), ("h", nat.CORRUPT_HEAD)):
            kept = list(torch.split(hat_rule(ent, n_part, cfg["normalize"])[0], dd, dim=-1))
            q = torch.cat(fn._uvr(code, kept, rel[rid]), dim=-1)
            assert q.dtype == F64 and q.shape == (S, (n_part + 1) * dd)
            got = affine_rule(q, hat_rule(cand, n_part, cfg["normalize"])[0], n_part, p)
            want = kge.score_candidates(name, p, True, side, ent, rel, rid, cand[None])
            torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("name", list(kge.BOXE_VARIANTS))
def test_boxe_rule_equals_the_oracle(name):
    dd, S, N, n_rel = 6, 7, 11, 3
    tanh, per_dim = kge.BOXE_VARIANTS[name]
    gen = torch.Generator().manual_seed(len(name) + dd)
    ent, cand, rel = (torch.randn(n, w, generator=gen, dtype=F64) * 0.7 for n, w in ((S, 2 * dd), (N, 2 * dd), (n_rel, 4 * dd + 2)))
    rid = torch.randint(n_rel, (S,), generator=gen)
    for p in PS:
        fn = scorer_on_cpu(name, p, dd, n_rel)
        center, half = fn._boxes(rel[rid])
        kept = ent.reshape(-1, 2, dd)
        for side, box in (("t", (1, 0)), ("h", (0, 1))):  # as BoxE._query_torch, in float64
            q = torch.cat([kept[:, 1], center[:, box[0]], half[:, box[0]], kept[:, 0], center[:, box[1]], half[:, box[1]]], -1)
            got = boxe_rule(q, cand, tanh, per_dim, p)
            want = kge.score_candidates(name, p, True, side, ent, rel, rid, cand[None])
            torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-13)
            per = boxe_rule(q, cand[None].expand(S, N, 2 * dd).contiguous(), tanh, per_dim, p)
            torch.testing.assert_close(per, got, rtol=0, atol=0)


def test_hand_set_gradient_rules():
    """sgn(0) = 0 and gradient 0 at zero norm come out of autograd on the restatements; the clamped normalisation is
    linear (gradient inv * d_hat)."""
    q = torch.tensor([[1.0, 1.0, -2.0, -3.0]], dtype=F64, requires_grad=True)  # U = (1, 1), R = (-2, -3)
    rows = torch.tensor([[2.0, 3.0], [2.0, 5.0]], dtype=F64, requires_grad=True)
    for p in PS:
        q.grad = rows.grad = None
        s = affine_rule(q, rows, 1, p)
        assert s.tolist() == [[0.0, -2.0]]
        s.sum().backward()
        assert bool(torch.isfinite(q.grad).all()) and rows.grad[0].tolist() == [0.0, 0.0]
        torch.testing.assert_close(rows.grad[1], torch.tensor([0.0, -1.0], dtype=F64))
        torch.testing.assert_close(q.grad, torch.tensor([[0.0, -5.0, 0.0, -1.0]], dtype=F64))
    x = torch.tensor([[0.0, 0.0, 3e-13, 4e-13]], dtype=F64, requires_grad=True)
    hat, inv = hat_rule(x, 2, True)
    assert inv.tolist() == [[1e12, 1e12]]
    (hat * torch.tensor([[1.0, 2.0, 3.0, 4.0]], dtype=F64)).sum().backward()
    torch.testing.assert_close(x.grad, torch.tensor([[1e12, 2e12, 3e12, 4e12]], dtype=F64))


# ------------------------------------------------------------------------------------------------ inputs, affine
# S, N, d -> (split, chunk) of the query side and of the candidate side (`bwd_plan`)
BWD_SHAPES = {(70, 100, 20): ((1, 112), (1, 80)), (150, 333, 20): ((4, 96), (2, 80)), (150, 333, 70): ((4, 96), (2, 80)),
              (150, 333, 132): ((4, 96), (2, 80))}
DELTA_MARGIN = 1e-6  # ~10 x the rounding error of an fp32 delta of these inputs: below it fp32 may take the other sign


def near_zero_deltas(q, rows, n_part):
    """[S, d] bool: the columns of a query with a candidate whose |delta| < DELTA_MARGIN, normalised or not (float64)."""
    dv = ref_dev()
    qd, S, d = q.to(dv).double(), q.shape[0], q.shape[1] // (n_part + 1)
    bad = torch.zeros(S, d, dtype=torch.bool, device=dv)
    for normalize in (False, True):
        c = hat_rule(rows.to(dv), n_part, normalize)[0].reshape(-1, n_part, d)
        for a0 in range(0, S, 32):
            u = qd[a0:a0 + 32].reshape(-1, n_part + 1, d)
            delta = u[:, None, n_part] + (u[:, None, :n_part] * c[None]).sum(2)
            bad[a0:a0 + 32] |= (delta.abs() < DELTA_MARGIN).any(1)
    return bad.cpu()


@functools.lru_cache(maxsize=16)
def affine_inputs(S, N, d, n_part, dtype, regime="normal"):
    """(q [S, (n_part + 1) d] f32, table [N + 50, n_part d], idx [N] int32 (distinct rows), g [S, N]) on the CPU."""
    gen = torch.Generator().manual_seed(S * 1009 + N * 13 + d * 7 + n_part + (3 if dtype == F16 else 0) + len(regime))
    M = N + 50
    idx = torch.randperm(M, generator=gen)[:N]
    if regime == "exact":
        table = torch.randint(-2, 3, (M, n_part * d), generator=gen).to(dtype)
        q = torch.randint(-2, 3, (S, (n_part + 1) * d), generator=gen).float()
        g = torch.randint(-3, 4, (S, N), generator=gen).float()
        return q, table, idx.to(torch.int32), g
    table = (torch.randn(M, n_part * d, generator=gen) * 0.5).to(dtype)
    q = torch.randn(S, (n_part + 1) * d, generator=gen) * 0.5
    g = torch.randn(S, N, generator=gen)
    if regime == "apart":  # "normal", with R redrawn where a |delta| is below DELTA_MARGIN: p = 1 needs its sign
        for _ in range(20):
            bad = near_zero_deltas(q, table[idx], n_part)
            if not bool(bad.any()):
                break
            q[:, n_part * d:] = torch.where(bad, torch.randn(S, d, generator=gen) * 0.5, q[:, n_part * d:])
        else:
            raise AssertionError("deltas near zero after 20 redraws")
    if regime == "ties":
        assert n_part == 1
        rows = table[idx].float()
        tied = (torch.arange(d) % 3 == 0)[None, :]
        pick = torch.randint(N, (S, d), generator=gen)
        q[:, :d] = torch.where(tied, torch.ones(S, d), q[:, :d])
        q[:, d:] = torch.where(tied, -rows[pick, torch.arange(d)[None, :].expand(S, d)], q[:, d:])
        q[0, :d], q[0, d:] = 1.0, -rows[5]  # distance 0 to candidate 5
    return q, table, idx.to(torch.int32), g


def test_ties_and_exact_regimes_have_their_elements():
    for dtype in (F32, F16):
        for (S, N, d) in BWD_SHAPES:
            for n_part in (1, 2):
                q, table, idx, _ = affine_inputs(S, N, d, n_part, dtype, "apart")
                assert not bool(near_zero_deltas(q, table[idx.long()], n_part).any())
        q, table, idx, _ = affine_inputs(150, 333, 20, 1, dtype, "ties")
        rows = table[idx.long()].double()
        delta = q[:, None, :20].double() * rows[None] + q[:, None, 20:].double()
        assert bool((delta[0, 5] == 0).all()) and bool(((delta == 0).sum(1)[:, ::3] >= 1).all())
        assert int((delta[1:] == 0).sum()) < 2 * 149 * 7 + 20  # ... and nowhere else but by chance
        q, table, idx, g = affine_inputs(150, 333, 20, 2, dtype, "exact")
        s = affine_rule(q.double(), table[idx.long()].double(), 2, 1)
        assert bool((s == s.round()).all()) and float(s.abs().max()) < 2048


# =============================================================================================== 1. normalisation
def normalize_case(dtype, n_part, d):
    """13 rows: generic ones, row 3 zero, (fp32) row 5 of norm ~1e-13 and row 7 of norm ~1e-11 in every part."""
    gen = torch.Generator().manual_seed(d * 31 + n_part + (1 if dtype == F16 else 0))
    n, M = 13, 40
    table = torch.randn(M, n_part * d, generator=gen)
    idx = torch.randperm(M, generator=gen)[:n]
    table[idx[3]] = 0.0
    if dtype == F32:
        table[idx[5]] *= 1e-13 / d ** 0.5
        table[idx[7]] *= 1e-11 / d ** 0.5
    return table.to(dtype), idx.to(torch.int32), torch.randn(n, n_part * d, generator=gen)


def test_normalize_case_has_its_rows():
    for d in (6, 64, 70, 260):
        table, idx, _ = normalize_case(F32, 2, d)
        nrm = table[idx.long()].double().reshape(13, 2, d).norm(dim=-1)
        assert bool((nrm[3] == 0).all()) and bool((nrm[5] < 5e-13).all()) and bool((nrm[5] > 1e-14).all())
        assert bool((nrm[7] > 2e-12).all()) and bool((nrm[7] < 1e-10).all())
        assert bool((nrm[[0, 1, 2, 4, 6, 8, 9, 10, 11, 12]] > 0.1).all())


@gpu
@pytest.mark.parametrize("d", [6, 64, 70, 260])
@pytest.mark.parametrize("n_part", [1, 2])
@pytest.mark.parametrize("dtype", [F32, F16], ids=tname)
def test_normalize_rows_and_backward(dev, dtype, n_part, d):
    table, idx, d_hat = normalize_case(dtype, n_part, d)
    rows = table[idx.long()]
    groups = {"generic": [0, 1, 2, 4, 6, 8, 9, 10, 11, 12], "zero": [3]}
    if dtype == F32:
        groups.update(clamped=[5], tiny=[7])
    for form, src in (("indexed", RowSource(table.to(dev), idx.to(dev))), ("dense", RowSource(rows.to(dev)))):
        hat, inv = nat.normalize_rows(src, n_part, False)
        assert torch.equal(hat.cpu(), rows.float()) and bool((inv == 1).all()), "normalize off: the converted row"
        hat, inv = nat.normalize_rows(src, n_part, True)
        d_rows = nat.normalize_rows_bwd(hat, inv, d_hat.to(dev))
        want = []
        for dt in (F64, F32):
            x = rows.detach().to(dt).clone().requires_grad_(True)
            h, i = hat_rule(x, n_part, True, dt)
            h.backward(d_hat.to(dt))
            want.append((h.detach(), i.detach(), x.grad))
        for name, sel in groups.items():  # by group: the gradients of the tiny rows are ~1e12 times the others'
            for k, (quantity, got) in enumerate((("hat", hat), ("inv", inv), ("d_rows", d_rows))):
                check("26.1 normalize", quantity, name, f"{form} {name} {quantity}", got[sel], want[0][k][sel], want[1][k][sel])
        assert bool((hat[3] == 0).all()) and bool((inv[3] == 1.0 / NORM_EPS).all()), "zero row"
        assert torch.equal(d_rows[3].cpu(), (inv[3].repeat_interleave(d) * d_hat.to(dev)[3]).cpu()), "zero row: inv * d_hat"
        if dtype == F32:
            assert bool((inv[5] == 1.0 / NORM_EPS).all()) and bool((inv[7] < 1.0 / NORM_EPS).all())
            assert torch.equal(d_rows[5].cpu(), (inv[5].repeat_interleave(d) * d_hat.to(dev)[5]).cpu()), "clamped: linear"


# ============================================================================================== 2. dense forward
AFFINE_COMBOS = [(n_part, p, normalize, dtype) for n_part in (1, 2) for p in PS for normalize in (True, False)
                 for dtype in (F32, F16)]


@gpu
@pytest.mark.parametrize("d", [6, 20, 70, 256])
@pytest.mark.parametrize("S,N", [(130, 197), (769, 65)])
def test_affine_dense_forward(dev, S, N, d):
    for n_part, p, normalize, dtype in AFFINE_COMBOS:
        q, table, idx, _ = affine_inputs(S, N, d, n_part, dtype)
        tb = table.to(dev)
        out = nat.neg_score_shared_fwd(affine_desc(tb, d, n_part, normalize, p), q.to(dev), RowSource(tb, idx.to(dev)))
        (s64, _, _), (s32, _, _) = both(affine_fn(n_part, normalize, p), q, table[idx.long()])
        what = f"{S}x{N} d={d} parts={n_part} p={p} norm={normalize} {tname(dtype)}"
        check("26.2 dense forward", "scores", f"p={p}", what, out, s64, s32)


# ==================================================================================================== 3. backward


class _NanEmpty:
    """`torch`, but `empty` / `empty_like` of a floating type come back filled with NaN."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def _fill(t):
        return t.fill_(float("nan")) if t.is_floating_point() else t

    def empty(self, *args, **kw):
        return self._fill(torch.empty(*args, **kw))

    def empty_like(self, *args, **kw):
        return self._fill(torch.empty_like(*args, **kw))


@contextlib.contextmanager
def nan_outputs():
    """Inside, every tensor the `_native` wrappers allocate (d_query, d_neg, their temporaries) starts as NaN: a
    gradient that is added to without having been cleared cannot pass by what the allocator happened to hand out."""
    assert nat.torch is torch
    nat.torch = _NanEmpty()
    try:
        yield
    finally:
        nat.torch = torch


def run_affine_backward(dev, S, N, d, n_part, p, normalize, dtype, regime):
    q, table, idx, g = affine_inputs(S, N, d, n_part, dtype, regime)
    tb, qd = table.to(dev), q.to(dev)
    desc, src = affine_desc(tb, d, n_part, normalize, p), RowSource(tb, idx.to(dev))
    out = nat.neg_score_shared_fwd(desc, qd, src)
    with nan_outputs():
        dq, dn = nat.neg_score_shared_bwd(desc, qd, src, out, g.to(dev))
    r64, r32 = both(affine_fn(n_part, normalize, p), q, table[idx.long()], g)
    what = f"{regime} {S}x{N} d={d} parts={n_part} p={p} norm={normalize} {tname(dtype)}"
    if regime == "exact":
        for name, got, want in zip(("scores", "d_query", "d_neg"), (out, dq, dn), r64):
            assert torch.equal(got.cpu(), want.float()), f"{what}: {name} not exact"
        return
    for name, got, w64, w32 in zip(("scores", "d_query", "d_neg"), (out, dq, dn), r64, r32):
        check("26.3 backward", name, f"{regime} p={p}", f"{what} {name}", got, w64, w32)


@gpu
@pytest.mark.parametrize("S,N,d", list(BWD_SHAPES))
def test_affine_shared_backward(dev, S, N, d):
    assert (bwd_plan(S, N, d), bwd_plan(N, S, d)) == BWD_SHAPES[(S, N, d)]

    def run():
        for n_part, p, normalize, dtype in AFFINE_COMBOS:
            run_affine_backward(dev, S, N, d, n_part, p, normalize, dtype, "apart")
            # the same draw as it comes (randn * 0.5): where an fp32 sign differs at p = 1, `check`'s 4 x rule sizes the bound
            run_affine_backward(dev, S, N, d, n_part, p, normalize, dtype, "normal")
        for dtype in (F32, F16):
            for p in PS:
                run_affine_backward(dev, S, N, d, 1, p, False, dtype, "ties")
            for n_part in (1, 2):
                run_affine_backward(dev, S, N, d, n_part, 1, False, dtype, "exact")

    _, names = launched(run)
    for n_part in (1, 2):
        for pc in (1, 2):
            for xq in (True, False):
                assert kernel_launched(names, "k_aff_shared_bwd", n_part, pc, xq), (n_part, pc, xq)


# =================================================================================================== 4. table form
def gap_thresholds(score_rows, S, N, excl_of, n_edge=0):
    """Per query row: a threshold (f32) in the widest gap between adjacent float64 scores of the middle half of the
    sorted row, the number of candidates above it (without the excluded one), and the condition that makes the
    count exact: both neighbours further from the threshold than a band of 4 x the fp32 restatement's largest error.
    The first n_edge rows look for their gap below their excluded candidate (ranks r / 4 .. r of the sorted row, r the
    candidate's), so that leaving it out changes the count: `ex_above` says for every row whether it does.
    score_rows(a0, a1, dtype) -> [a1 - a0, N] on ref_dev(); excl_of(a0, s64 block) -> int64 [rows] positions (-1: none)."""
    thr, want, margin, excl, exa, err = [], [], [], [], [], 0.0
    step = max(1, (1 << 22) // N)
    for a0 in range(0, S, step):
        a1 = min(S, a0 + step)
        s64 = score_rows(a0, a1, F64)
        err = max(err, float((score_rows(a0, a1, F32).double() - s64).abs().max()))
        srt = torch.sort(s64, dim=1).values
        ex = excl_of(a0, s64).to(s64.device)
        rows = torch.arange(a0, a1, device=s64.device)
        w_hi = torch.full_like(rows, 3 * N // 4)
        edge = (rows < n_edge) & (ex >= 0)
        rank = (s64 < s64.gather(1, ex.clamp(min=0)[:, None])).sum(1)  # sorted position of the excluded candidate
        w_hi = torch.where(edge, torch.minimum(w_hi, rank), w_hi)
        w_lo = torch.where(edge, w_hi // 4, torch.full_like(rows, N // 4))
        assert bool((w_hi - w_lo >= min(16, N // 4)).all()), "an excluded edge candidate among the lowest scores"
        pos = torch.arange(N - 1, device=s64.device)[None, :]
        gaps = (srt[:, 1:] - srt[:, :-1]).masked_fill((pos < w_lo[:, None]) | (pos >= w_hi[:, None]), -1.0)
        lo_i = torch.argmax(gaps, dim=1)
        lo, hi = srt.gather(1, lo_i[:, None])[:, 0], srt.gather(1, lo_i[:, None] + 1)[:, 0]
        t = ((lo + hi) / 2).float()
        above = s64 > t.double()[:, None]
        ex_above = torch.where(ex >= 0, above.gather(1, ex.clamp(min=0)[:, None])[:, 0], torch.zeros_like(ex, dtype=torch.bool))
        thr.append(t.cpu())
        want.append((above.sum(1) - ex_above.long()).cpu())
        margin.append(torch.minimum(hi - t.double(), t.double() - lo).cpu())
        excl.append(ex.cpu())
        exa.append(ex_above.cpu())
    return dict(thr=torch.cat(thr), want=torch.cat(want), margin=torch.cat(margin), excl=torch.cat(excl).to(torch.int32),
                ex_above=torch.cat(exa), band=4.0 * err)


def mixed_excl(N, edges=()):
    """row i: position `edges[i]` for the first rows, then -1 | the best candidate (above any threshold) | i % N."""
    def excl_of(a0, s64):
        i = torch.arange(a0, a0 + s64.shape[0], device=s64.device)
        ex = torch.where(i % 3 == 0, torch.full_like(i, -1), torch.where(i % 3 == 1, s64.argmax(1), i * 7919 % N))
        for k, e in enumerate(edges):
            if a0 <= k < a0 + s64.shape[0]:
                ex[k - a0] = e
        return ex
    return excl_of


# name -> (S, N, d, n_part, p, normalize, dtype, indexed, tiles, chunks)
COUNT_CASES = {
    "tiles2-f16": (1093, 15589, 8, 1, 1, True, F16, True, 2, 1),
    "tiles2-f32": (1093, 15589, 8, 2, 3, False, F32, False, 2, 1),
    "tiles8-f32": (4101, 16037, 8, 2, 2, True, F32, True, 8, 1),
    "tiles8-f16": (4101, 16037, 8, 1, 1, False, F16, False, 8, 1),
    "chunks-indexed": (70, 8293, 512, 2, 1, True, F32, True, 1, 2),
    "chunks-dense": (70, 8293, 512, 2, 2, True, F32, False, 1, 2),
    "chunks-plain": (70, 8293, 512, 2, 1, False, F32, False, 1, 2),
}
COUNT_CASES.update({f"tiles1-{n_part}-{p}-{int(nm)}-{tname(dt)}": (130, 197, 8, n_part, p, nm, dt, n_part == 1, 1, 1)
                    for n_part, p, nm, dt in AFFINE_COMBOS})
CHUNK_EDGES = (0, 8191, 8192, 8292, 4000, 8200)  # `excl` in both chunks and on the first and last column of each


@functools.lru_cache(maxsize=None)
def count_case(name):
    S, N, d, n_part, p, normalize, dtype, indexed, tiles, chunks = COUNT_CASES[name]
    q, table, idx, _ = affine_inputs(S, N, d, n_part, dtype)
    rows = table[idx.long()]
    dv = ref_dev()
    qd, rd = q.to(dv), rows.to(dv)

    def score_rows(a0, a1, dt):
        out = [affine_rule(qd[b0:min(a1, b0 + 8)].to(dt), hat_rule(rd, n_part, normalize, dt)[0], n_part, p)
               for b0 in range(a0, a1, 8)] if N * d * n_part > (1 << 21) else \
              [affine_rule(qd[a0:a1].to(dt), hat_rule(rd, n_part, normalize, dt)[0], n_part, p)]
        return torch.cat(out)

    with torch.no_grad():
        edges = CHUNK_EDGES if chunks > 1 else ()
        ref = gap_thresholds(score_rows, S, N, mixed_excl(N, edges), len(edges))
    ref.update(q=q, table=table, idx=idx)
    return ref


@pytest.mark.parametrize("name", list(COUNT_CASES))
def test_count_thresholds_sit_in_wide_gaps(name):
    S, N, d, n_part, p, normalize, dtype, indexed, tiles, chunks = COUNT_CASES[name]
    assert table_tiles(S, min(N, nat.affine_count_chunk_rows(affine_desc(torch.empty(1, n_part * d, dtype=dtype), d, n_part,
                                                                         normalize, p)))) == tiles
    ref = count_case(name)
    assert ref["band"] > 0 and bool((ref["margin"] > ref["band"]).all()), (ref["band"], float(ref["margin"].min()))
    assert int(ref["want"].min()) > N // 8 and int(ref["want"].max()) < N  # neither trivial
    assert bool(ref["ex_above"][1::3].all()), "the best candidate is above its row's threshold"
    if chunks > 1:  # an excluded position tests `col0` only where leaving it out changes the count
        assert ref["excl"][:len(CHUNK_EDGES)].tolist() == list(CHUNK_EDGES) and bool(ref["ex_above"][:len(CHUNK_EDGES)].all())


def affine_counts(dev, case, S, N, d, n_part, p, normalize, dtype, indexed, thr, excl, round_f16=False):
    tb = (case["table"] if indexed else case["table"][case["idx"].long()]).to(dev)
    src = RowSource(tb, case["idx"].to(dev)) if indexed else RowSource(tb)
    desc = affine_desc(tb, d, n_part, normalize, p)
    counts, names = launched(lambda: nat.neg_score_shared_counts(desc, case["q"].to(dev), src, thr.to(dev), excl.to(dev),
                                                                 round_f16=round_f16))
    assert kernel_launched(names, "k_aff_shared_fwd", n_part, min(p, 2), dtype, True, True, False), names
    return desc, counts.cpu(), names


@gpu
@pytest.mark.parametrize("name", list(COUNT_CASES))
def test_affine_counts(dev, name):
    S, N, d, n_part, p, normalize, dtype, indexed, tiles, chunks = COUNT_CASES[name]
    ref = count_case(name)
    desc, counts, names = affine_counts(dev, ref, S, N, d, n_part, p, normalize, dtype, indexed, ref["thr"], ref["excl"])
    assert cdiv(N, nat.affine_count_chunk_rows(desc)) == chunks
    assert sum("k_aff_shared_fwd" in n for n in names) == chunks
    assert table_tiles(S, min(N, nat.affine_count_chunk_rows(desc))) == tiles
    bad = (counts[:, 0].long() != ref["want"]).nonzero().flatten().tolist()
    assert not bad, (name, bad[:8], counts[bad[:8], 0].tolist(), ref["want"][bad[:8]].tolist(), ref["excl"][bad[:8]].tolist())
    assert int(counts[:, 1].abs().sum()) == 0, "a score equal to a threshold chosen inside a gap"


@gpu
@pytest.mark.parametrize("S,N,n_part,dtype,indexed", [(130, 197, 1, F32, True), (1093, 15589, 2, F16, False),
                                                      (1093, 15589, 1, F32, True)], ids=str)
def test_affine_counts_exact(dev, S, N, n_part, dtype, indexed):
    """Integer scores (p = 1, not normalised), thresholds that ARE scores of candidates: `>` and `==` counted exactly,
    the excluded position left out, with and without rounding to fp16 (integers below 2048)."""
    d = 8
    q, table, idx, _ = affine_inputs(S, N, d, n_part, dtype, "exact")
    rows = table[idx.long()]
    dv = ref_dev()
    s = torch.cat([affine_rule(q[a0:a0 + 256].to(dv).double(), rows.to(dv).double(), n_part, 1) for a0 in range(0, S, 256)])
    assert bool((s == s.round()).all()) and float(s.abs().max()) < 2048
    i = torch.arange(S, device=dv)
    target = (i * 31) % N
    thr = s.gather(1, target[:, None])[:, 0]
    excl = torch.where(i % 2 == 0, target, torch.where(i % 4 == 1, torch.full_like(i, -1), (target + 1) % N))
    keep = torch.ones_like(s, dtype=torch.bool)
    keep[i[excl >= 0], excl[excl >= 0]] = False
    want = torch.stack([((s > thr[:, None]) & keep).sum(1), ((s == thr[:, None]) & keep).sum(1)], 1).cpu()
    assert int(want[:, 1].max()) > 1
    case = dict(q=q, table=table, idx=idx)
    for round_f16 in (False, True):
        _, counts, _ = affine_counts(dev, case, S, N, d, n_part, 1, False, dtype, indexed, thr.float().cpu(),
                                     excl.to(torch.int32).cpu(), round_f16)
        assert torch.equal(counts.long(), want), (round_f16, (counts.long() != want).nonzero()[:8].tolist())


@gpu
@pytest.mark.parametrize("n,d", [(130, 8), (769, 70)])
def test_affine_pairs(dev, n, d):
    for n_part, p, normalize, dtype in AFFINE_COMBOS:
        q, table, idx, _ = affine_inputs(n, n, d, n_part, dtype)
        tb = table.to(dev)
        desc = affine_desc(tb, d, n_part, normalize, p)
        out, names = launched(lambda: nat.neg_score_shared_pairs(desc, q.to(dev), RowSource(tb, idx.to(dev)), n, 4 * n))
        assert kernel_launched(names, "k_aff_shared_fwd", n_part, min(p, 2), dtype, True, False, True), names
        rows = table[idx.long()]
        want = []
        for dt in (F64, F32):
            hat = hat_rule(rows, n_part, normalize, dt)[0].reshape(n, n_part, d)
            u = q.to(dt).reshape(n, n_part + 1, d)
            want.append(-lp_norm(u[:, n_part] + (u[:, :n_part] * hat).sum(1), p))
        what = f"pairs {n} d={d} parts={n_part} p={p} norm={normalize} {tname(dtype)}"
        check("26.4 pairs", "scores", f"p={p}", what, out, want[0], want[1])


# ========================================================================================================= 5. BoxE
BOX_M = 97
# regime, S, N, d (the class of each shape: test_planner_restatements)
BOX_CASES = [("normal", 5, 9, 6), ("normal", 5, 9, 40), ("normal", 5, 9, 100), ("normal", 70, 130, 6),
             ("inside", 5, 9, 6), ("inside", 70, 130, 6), ("inside", 70, 130, 40), ("inside", 70, 130, 100),
             ("normal", 130, 1030, 6), ("inside", 130, 4100, 6), ("exact", 70, 130, 6), ("exact", 70, 130, 40)]
BOX_COUNT_CASES = [("normal", 5, 9, 6), ("inside", 5, 9, 6), ("inside", 70, 130, 6), ("normal", 130, 1030, 6),
                   ("inside", 130, 4100, 6), ("normal", 130, 16133, 6), ("inside", 130, 16133, 6)]
BOX_COMBOS = [(tanh, per_dim, p, dtype) for tanh, per_dim in BOX_SETTINGS for p in PS for dtype in (F32, F16)]
INSIDE_H = {6: 0.85, 40: 1.22, 100: 1.4}  # half widths of the "inside" regime, in front of (0.75 .. 1.25)
BOX_MARGIN = 1e-5


def box_offenders(q, rows, pairs):
    """[S, 2, d] bool: the half widths with a candidate whose |dist - H| < BOX_MARGIN, with or without tanh.
    pairs: rows [S, n, 2 d] per query, else [n, 2 d] shared."""
    out = []
    for a0 in range(0, q.shape[0], 16):
        near = [boxe_rule(q[a0:a0 + 16], rows[a0:a0 + 16] if pairs else rows, tanh, True, 1, parts=True)[0].abs() < BOX_MARGIN
                for tanh in (True, False)]
        out.append((near[0] | near[1]).any(1))
    return torch.cat(out)


@functools.lru_cache(maxsize=8)
def boxe_inputs(regime, S, N, d, dtype):
    """(q [S, 6 d], table [BOX_M, 2 d], idx [N] shared candidates, pidx [S * N] per-triple negatives, g [S, N]).
    "normal" / "inside": half widths are redrawn until no element of either candidate list is within BOX_MARGIN of
    its box's edge (the inside decision of the settings without per_dim is a step)."""
    gen = torch.Generator().manual_seed(S * 131 + N * 7 + d + (2 if dtype == F16 else 0) + len(regime))
    idx = torch.randint(BOX_M, (N,), generator=gen)
    pidx = torch.randint(BOX_M, (S * N,), generator=gen)
    if regime == "exact":
        table = torch.randint(-3, 4, (BOX_M, 2 * d), generator=gen).to(dtype)
        q = torch.randint(-3, 4, (S, 2, 3, d), generator=gen).float()
        q[:, :, 1, 1::2] += 0.5  # centres on half-integers in the odd columns
        q[:, :, 2] = torch.tensor([0.5, 1.5, 3.5])[torch.randint(3, (S, 2, d), generator=gen)]
        return q.reshape(S, 6 * d), table, idx.to(torch.int32), pidx.to(torch.int32), \
            torch.randint(-3, 4, (S, N), generator=gen).float()
    scale = 0.7 if regime == "normal" else 0.3
    table = (torch.randn(BOX_M, 2 * d, generator=gen) * scale).to(dtype)
    q = torch.randn(S, 2, 3, d, generator=gen) * (1.0 if regime == "normal" else 0.3)

    def draw_h():
        if regime == "normal":
            return torch.randn(S, 2, d, generator=gen).abs()
        return INSIDE_H[d] * (0.75 + 0.5 * torch.rand(S, 2, d, generator=gen))

    q[:, :, 2] = draw_h()
    dv = ref_dev()
    shared = table[idx].to(dv).double()
    pairs = table[pidx].reshape(S, N, 2 * d).to(dv).double() if N <= 4100 else None  # (larger lists: counting only)
    for _ in range(50):
        qd = q.reshape(S, 6 * d).to(dv).double()
        bad = box_offenders(qd, shared, False)
        if pairs is not None:
            bad = bad | box_offenders(qd, pairs, True)
        bad = bad.cpu()
        if not bool(bad.any()):
            break
        q[:, :, 2] = torch.where(bad, draw_h(), q[:, :, 2])
    else:
        raise AssertionError("no margin to the box edges after 50 redraws")
    return q.reshape(S, 6 * d), table, idx.to(torch.int32), pidx.to(torch.int32), torch.randn(S, N, generator=gen)


@pytest.mark.parametrize("regime,S,N,d", [c for c in BOX_CASES if c[2] <= 1030] + [("inside", 130, 4100, 6)]
                         + [c for c in BOX_COUNT_CASES if c[2] > 4100])
def test_boxe_regimes_hold_their_conditions(regime, S, N, d):
    for dtype in (F32, F16):
        q, table, idx, pidx, g = boxe_inputs(regime, S, N, d, dtype)
        dv = ref_dev()
        qd = q.to(dv).double()
        lists = [(table[idx.long()], False)]
        if N <= 4100:  # (longer lists are counted only: shared candidates)
            lists.append((table[pidx.long()].reshape(S, N, 2 * d), True))
        for rows, pairs in lists:
            rows = rows.to(dv).double()
            for tanh in (True, False) if regime != "exact" else (False,):
                diff, all_in = boxe_rule(qd, rows, tanh, True, 1, parts=True)
                share = float(all_in.double().mean())
                if regime == "exact":
                    assert int((diff == 0).sum()) >= 10, "dist == H exactly"
                    e = rows.reshape(1, -1, 2, d) if rows.dim() == 2 else rows.reshape(S, -1, 2, d)
                    assert int((e + qd.reshape(S, 1, 2, 3, d)[:, :, :, 0] == qd.reshape(S, 1, 2, 3, d)[:, :, :, 1]).sum()) >= 10
                    s = boxe_rule(qd, rows, False, False, 1)
                    assert bool((s * 16 == (s * 16).round()).all()) and float(s.abs().max()) < 2 ** 15  # exact in f32
                    continue
                assert float(diff.abs().min()) >= BOX_MARGIN
                if regime == "inside":
                    assert 0.25 <= share <= 0.75, (tanh, pairs, share)
                elif d >= 6 and S * N > 100:
                    assert share < 0.01, share


def run_boxe(dev, regime, S, N, d, tanh, per_dim, p, dtype):
    q, table, idx, pidx, g = boxe_inputs(regime, S, N, d, dtype)
    tb, qd, gd = table.to(dev), q.to(dev), g.to(dev)
    desc = boxe_desc(tb, tanh, per_dim, p)
    rule = boxe_fn(tanh, per_dim, p)
    what = f"{regime} {S}x{N} d={d} tanh={tanh} per_dim={per_dim} p={p} {tname(dtype)}"
    for form, src, rows in (("shared", RowSource(tb, idx.to(dev)), table[idx.long()]),
                            ("pertriple", RowSource(tb, pidx.to(dev)), table[pidx.long()].reshape(S, N, 2 * d))):
        if form == "shared":
            out = nat.neg_score_shared_fwd(desc, qd, src)
            with nan_outputs():
                dq, dn = nat.neg_score_shared_bwd(desc, qd, src, out, gd)
        else:
            out = nat.neg_score_pertriple_fwd(desc, qd, src, N)
            with nan_outputs():
                dq, dn = nat.neg_score_pertriple_bwd(desc, qd, src, N, gd)
        r64, r32 = both(rule, q, rows, g)
        for name, got, w64, w32 in zip(("scores", "d_query", "d_neg"), (out, dq, dn.reshape(r64[2].shape)), r64, r32):
            if regime == "exact":
                assert torch.equal(got.cpu(), w64.float()), f"{what} {form}: {name} not exact"
            else:
                check(f"26.5 BoxE {form}", name, f"{regime} p={p}", f"{what} {form} {name}", got, w64, w32)


@gpu
@pytest.mark.parametrize("regime,S,N,d", BOX_CASES)
def test_boxe_forward_and_backward(dev, regime, S, N, d):
    assert negatives_per_item(S, N) == {9: 8, 130: 8, 1030: 16, 4100: 64}[N]
    assert cdiv(N, negatives_per_item(S, N)) > 1  # d_query through atomics
    for tanh, per_dim in BOX_SETTINGS if regime != "exact" else [(False, True), (False, False)]:
        for p in PS if regime != "exact" else (1,):
            for dtype in (F32, F16):
                run_boxe(dev, regime, S, N, d, tanh, per_dim, p, dtype)


@gpu
@pytest.mark.parametrize("per_dim", [True, False])
@pytest.mark.parametrize("p", [2, 3])
def test_boxe_zero_norm(dev, per_dim, p):
    """Query 0's candidates all sit on both centres (no tanh: e + s == c bit for bit): f = 0 in every dimension, score
    0, gradient 0 (`lp_inv`); the other queries are ordinary."""
    S, N, d = 5, 9, 6
    q, table, idx, pidx, g = boxe_inputs("normal", S, N, d, F32)
    q, pidx, table = q.clone().reshape(S, 2, 3, d), pidx.clone(), table.clone()
    pidx[:N] = 11
    table[11], q[0, :, 0] = (table[11] * 256).round() / 256, (q[0, :, 0] * 256).round() / 256  # e + s is exact in fp32
    q[0, :, 1] = table[11].reshape(2, d) + q[0, :, 0]
    q = q.reshape(S, 6 * d)
    assert not bool(box_offenders(q.double(), table[pidx.long()].reshape(S, N, 2 * d).double(), True).any())
    rows = table[pidx.long()].reshape(S, N, 2 * d)
    tb = table.to(dev)
    desc, src = boxe_desc(tb, False, per_dim, p), RowSource(tb, pidx.to(dev))
    out = nat.neg_score_pertriple_fwd(desc, q.to(dev), src, N)
    dq, dn = nat.neg_score_pertriple_bwd(desc, q.to(dev), src, N, g.to(dev))
    r64, r32 = both(boxe_fn(False, per_dim, p), q, rows, g)
    assert bool((r64[0][0] == 0).all()) and bool((r64[1][0] == 0).all()) and bool((r64[2][0] == 0).all())
    assert bool((out[0] == 0).all()) and bool((dq[0] == 0).all()) and bool((dn[:N] == 0).all())
    for name, got, w64, w32 in zip(("scores", "d_query", "d_neg"), (out, dq, dn.reshape(S, N, 2 * d)), r64, r32):
        check("26.5 BoxE pertriple", name, f"zero norm p={p}", f"zero norm per_dim={per_dim} p={p} {name}", got, w64, w32)


@functools.lru_cache(maxsize=None)
def boxe_count_case(regime, S, N, d, dtype, tanh, per_dim, p):
    q, table, idx, _, _ = boxe_inputs(regime, S, N, d, dtype)
    dv = ref_dev()
    qd, rd = q.to(dv), table[idx.long()].to(dv)
    with torch.no_grad():
        return gap_thresholds(lambda a0, a1, dt: boxe_rule(qd[a0:a1].to(dt), rd.to(dt), tanh, per_dim, p), S, N, mixed_excl(N))


@pytest.mark.parametrize("tanh,per_dim,p,dtype", BOX_COMBOS, ids=lambda v: tname(v) if isinstance(v, torch.dtype) else str(v))
@pytest.mark.parametrize("k", range(len(BOX_COUNT_CASES)))
def test_boxe_count_thresholds_sit_in_wide_gaps(k, tanh, per_dim, p, dtype):
    regime, S, N, d = BOX_COUNT_CASES[k]
    ref = boxe_count_case(regime, S, N, d, dtype, tanh, per_dim, p)
    assert ref["band"] > 0 and bool((ref["margin"] > ref["band"]).all()), (ref["band"], float(ref["margin"].min()))
    assert bool(ref["ex_above"][1::3].all()), "the best candidate is above its row's threshold"


@gpu
@pytest.mark.parametrize("k", range(len(BOX_COUNT_CASES)))
def test_boxe_counts(dev, k):
    """All 24 (tanh, per_dim, p, table type) combinations at every shape of BOX_COUNT_CASES."""
    regime, S, N, d = BOX_COUNT_CASES[k]
    assert negatives_per_item(S, N, 256) == {9: 8, 130: 8, 1030: 16, 4100: 64, 16133: 256}[N]
    for tanh, per_dim, p, dtype in BOX_COMBOS:
        ref = boxe_count_case(regime, S, N, d, dtype, tanh, per_dim, p)
        q, table, idx, _, _ = boxe_inputs(regime, S, N, d, dtype)
        tb = table.to(dev)
        counts = nat.neg_score_shared_counts(boxe_desc(tb, tanh, per_dim, p), q.to(dev), RowSource(tb, idx.to(dev)),
                                             ref["thr"].to(dev), ref["excl"].to(dev)).cpu()
        bad = (counts[:, 0].long() != ref["want"]).nonzero().flatten().tolist()
        assert not bad, ((tanh, per_dim, p, dtype), bad[:8], counts[bad[:8], 0].tolist(), ref["want"][bad[:8]].tolist())
        assert int(counts[:, 1].abs().sum()) == 0


@gpu
def test_measured_errors_table(dev):
    """Prints (run with -s) the largest errors of this file's cases in units of their bound: DESIGN.md section 26."""
    mine = {k: v for k, v in MEASURED.items() if str(k[0]).startswith("26.")}
    for (part, quantity, regime), (e32, ek) in sorted(mine.items()):
        print(f"{part:22s} {quantity:8s} {regime:16s} fp32 restatement {e32:9.3g}   kernel {ek:9.3g}")
    assert all(ek <= max(1.0, 4.0 * e32) for e32, ek in mine.values())
