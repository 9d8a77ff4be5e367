"""The affine scorers' and BoxE's row kernels in every (VEC, IT) class their host dispatch selects
(csrc/common.h `dispatch_row_class<PartRows>`: VEC = 4 when the part width divides by 4, else 1; IT = the next of
1, 2, 4, 8 >= ceil(chunks / 16), for both table types), through the `_native` wrappers, so that every case is certain
to reach `affine_pertriple`, `boxe_negatives` with per-triple candidates, `affine_grad_segments` and
`boxe_grad_segments`:

  part width dd |  40 | 100 | 200 | 260           |  6 | 18 | 50 | 70
  VEC, IT       | 4,1 | 4,2 | 4,4 | 4,8 (5 of 8)  | 1,1| 1,2| 1,4| 1,8
  refused ("too wide", BESS_EUNSUPPORTED, outputs untouched): dd = 130 (VEC 1, 9 iterations), 516 (VEC 4, 9)

Every class runs the four settings the other tests pair up - affine (n_part, normalize, p) and BoxE (tanh, per_dim, p)
- over a table of 64 rows, 5 queries and 9 negatives; the long-segment launches run on 30 x 9 references that all
point at one row (270 > SEGMENT_CAP).

  - per-triple forward and backward == `oracle.kge.score_candidates` and its autograd, on the same fp16-rounded inputs
    held in fp32 (the query is built by the scorer's torch formulas, its gradient taken back through them);
  - grad-segments and its fused-SGD form == float64 `index_add` of the backward kernel's d_neg rows.

Tolerances are those of the tests of the same quantities in test_hip_parity.py: `test_scoring_vs_oracle` (scores) and
`test_scoring_gradients_vs_oracle` (fp32 gradients), `test_boxe_wide_embeddings_vs_oracle` (fp16 gradients),
`test_affine_grad_segments_match_scatter_of_row_gradients` and `test_boxe_grad_segments_match_scatter_of_row_gradients`."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from besskge import _native as nat  # noqa: E402
from besskge._native import RowSource  # noqa: E402
from oracle import kge  # noqa: E402

from test_hip_parity import close, make_scorer  # noqa: E402

F32, F16 = torch.float32, torch.float16
PART_WIDTHS = [40, 100, 200, 260, 6, 18, 50, 70]
TOO_WIDE = [130, 516]
M, S, N, N_REL = 64, 5, 9, 3
S_HOT = 30  # 30 x 9 = 270 references on one row: more than SEGMENT_CAP

# (n_part, normalize, p) -> the member of the family with these settings (oracle.kge.AFFINE_VARIANTS)
AFFINE_SETTINGS = [(1, True, 1, "TripleRE"), (1, False, 2, "TripleREv2"), (2, True, 2, "TranS"), (2, False, 1, "TranSnn")]
# (tanh, per_dim, p) -> oracle.kge.BOXE_VARIANTS
BOXE_SETTINGS = [(True, True, 1, "BoxE"), (True, False, 2, "BoxEall"), (False, True, 2, "BoxEpd"), (False, False, 1, "BoxEnt")]

classes = pytest.mark.parametrize("dd", PART_WIDTHS)
dtypes = pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda", 0)


def affine_desc(table, dd, n_part, normalize, p):
    desc = nat.make_desc(nat.AFFINE, p, table, dd)
    desc.reserved[0], desc.reserved[1] = n_part, int(normalize)
    return desc


def boxe_desc(table, tanh, per_dim, p):
    desc = nat.make_desc(nat.BOXE, p, table, int(table.shape[1]))
    desc.reserved[0] = int(tanh) | (int(per_dim) << 1)
    return desc


def affine_cases(dd, dtype, dev, gen, n_query=S):
    """(desc, query, table) of the four settings, random queries"""
    for n_part, normalize, p, _ in AFFINE_SETTINGS:
        table = torch.randn(M, n_part * dd, generator=gen).to(dtype).to(dev)
        q = torch.randn(n_query, (n_part + 1) * dd, generator=gen).to(dev)
        yield affine_desc(table, dd, n_part, normalize, p), q, table


def boxe_cases(dd, dtype, dev, gen, n_query=S):
    for tanh, per_dim, p, _ in BOXE_SETTINGS:
        table = (torch.randn(M, 2 * dd, generator=gen) * 0.7).to(dtype).to(dev)
        q = torch.randn(n_query, 6 * dd, generator=gen)
        q[:, 2 * dd:3 * dd].abs_()  # half widths H_0, H_1 are positive
        q[:, 5 * dd:].abs_()
        yield boxe_desc(table, tanh, per_dim, p), q.to(dev), table


def check_pertriple_vs_oracle(dev, name, p, desc_of, dd, dtype, gen):
    """Scores, d_neg and (through the scorer's query formulas) the gradients of the kept entity and of the relation
    table, against the oracle's autograd."""
    W, Wr = kge.entity_width(name, dd), kge.relation_width(name, dd)
    rel = torch.randn(N_REL, Wr, generator=gen).to(dtype).float()
    h = torch.randn(S, W, generator=gen).to(dtype).float()
    table = torch.randn(M, W, generator=gen).to(dtype)
    rid = torch.randint(N_REL, (S,), generator=gen)
    idx = torch.randint(M, (S * N,), generator=gen, dtype=torch.int32)
    go = torch.randn(S, N, generator=gen)

    ho, ro = (x.clone().requires_grad_(True) for x in (h, rel))
    no = table.float()[idx.long()].reshape(S, N, W).clone().requires_grad_(True)
    so = kge.score_candidates(name, p, False, "t", ho, ro, rid, no)
    (so * go).sum().backward()

    fn = make_scorer(name, p, False, N_REL, dd, torch.zeros(1, 4, W), rel, dev)
    fn.relation_embedding.requires_grad_(True)
    hd = h.clone().to(dev).requires_grad_(True)
    q = fn._query_torch(nat.CORRUPT_TAIL, hd, fn.relation_embedding, rid.to(dev)).contiguous()
    src = RowSource(table.to(dev), idx.to(dev))
    desc = desc_of(src.base)
    qd = q.detach().contiguous()
    sc = nat.neg_score_pertriple_fwd(desc, qd, src, N)
    dq, dn = nat.neg_score_pertriple_bwd(desc, qd, src, N, go.to(dev))
    q.backward(dq)

    close(sc, so, scale=2e-6)
    tol = dict(scale=2e-6) if dtype == F32 else dict(rtol=2e-2, scale=4e-3)
    close(dn.reshape(S, N, W), no.grad, **tol)
    close(hd.grad, ho.grad, **tol)
    close(fn.relation_embedding.grad, ro.grad, **tol)


@classes
@dtypes
def test_affine_pertriple_vs_oracle(dev, dd, dtype):
    gen = torch.Generator().manual_seed(1000 + dd)
    for n_part, normalize, p, name in AFFINE_SETTINGS:
        assert kge.AFFINE_VARIANTS[name]["normalize"] == normalize and kge.entity_width(name, dd) == n_part * dd
        check_pertriple_vs_oracle(dev, name, p, lambda t: affine_desc(t, dd, n_part, normalize, p), dd, dtype, gen)


@classes
@dtypes
def test_boxe_pertriple_vs_oracle(dev, dd, dtype):
    gen = torch.Generator().manual_seed(2000 + dd)
    for tanh, per_dim, p, name in BOXE_SETTINGS:
        assert kge.BOXE_VARIANTS[name] == (tanh, per_dim)
        check_pertriple_vs_oracle(dev, name, p, lambda t: boxe_desc(t, tanh, per_dim, p), dd, dtype, gen)


def check_segments_vs_scatter(desc, q, table, idx, go, n_long, fp16_tol):
    """grad_seg rows and the fused SGD step == index_add (float64) of the backward kernel's d_neg rows"""
    W, n_neg = int(table.shape[1]), int(go.shape[1])
    _, dn = nat.neg_score_pertriple_bwd(desc, q, RowSource(table, idx), n_neg, go)
    seg = nat.SegmentIndex(idx, M, width=W)
    n_seg = int(seg.n_seg.item())
    assert int(seg.long_segs[0].item()) == n_long
    uniq = torch.unique(idx.cpu().long())
    want = torch.zeros(M, W, dtype=torch.float64).index_add_(0, idx.cpu().long(), dn.cpu().double())
    g1 = nat.neg_pertriple_grad_segments(desc, q, table, n_neg, go, seg)
    close(g1[:n_seg], want[uniq].float(), rtol=1e-4, atol=1e-5, scale=4e-6)
    t2 = table.clone()
    nat.neg_pertriple_grad_segments(desc, q, t2, n_neg, go, seg, fused_sgd_lr=0.5)
    tol = fp16_tol if table.dtype == F16 else 1e-5
    close(t2, table.float().cpu() - 0.5 * want.float(), rtol=tol, atol=tol, scale=4e-6)


@classes
@dtypes
@pytest.mark.parametrize("hot", [False, True], ids=["rows", "long"])
def test_affine_grad_segments_match_scatter(dev, dd, dtype, hot):
    gen = torch.Generator().manual_seed(3000 + dd)
    n_query = S_HOT if hot else S
    for desc, q, table in affine_cases(dd, dtype, dev, gen, n_query):
        idx = torch.randint(M, (n_query * N,), generator=gen, dtype=torch.int32)
        if hot:
            idx[:] = 5
        go = torch.randn(n_query, N, generator=gen) * (0.1 if hot else 1.0)
        check_segments_vs_scatter(desc, q, table, idx.to(dev), go.to(dev), int(hot), fp16_tol=2e-3)


@classes
@dtypes
@pytest.mark.parametrize("hot", [False, True], ids=["rows", "long"])
def test_boxe_grad_segments_match_scatter(dev, dd, dtype, hot):
    gen = torch.Generator().manual_seed(4000 + dd)
    n_query = S_HOT if hot else S
    for desc, q, table in boxe_cases(dd, dtype, dev, gen, n_query):
        idx = torch.randint(M, (n_query * N,), generator=gen, dtype=torch.int32)
        if hot:
            idx[:] = 5
        go = torch.randn(n_query, N, generator=gen) * 0.1
        check_segments_vs_scatter(desc, q, table, idx.to(dev), go.to(dev), int(hot), fp16_tol=4e-3)


@pytest.mark.parametrize("dd", TOO_WIDE)
@dtypes
@pytest.mark.parametrize("family", ["affine", "boxe"])
def test_parts_wider_than_the_largest_class_are_refused(dev, family, dd, dtype):
    """Nine 16-chunk iterations have no class: every entry point raises "too wide" and writes nothing."""
    gen = torch.Generator().manual_seed(5000 + dd)
    desc, q, table = next((affine_cases if family == "affine" else boxe_cases)(dd, dtype, dev, gen))
    idx = torch.randint(M, (S * N,), generator=gen, dtype=torch.int32).to(dev)
    go = torch.randn(S, N, generator=gen).to(dev)
    out = torch.full((S, N), float("nan"), device=dev)
    with pytest.raises(RuntimeError, match="too wide"):
        nat.neg_score_pertriple_fwd(desc, q, RowSource(table, idx), N, out=out)
    assert bool(torch.isnan(out).all())
    with pytest.raises(RuntimeError, match="too wide"):
        nat.neg_score_pertriple_bwd(desc, q, RowSource(table, idx), N, go)
    seg = nat.SegmentIndex(idx, M, width=int(table.shape[1]))
    with pytest.raises(RuntimeError, match="too wide"):
        nat.neg_pertriple_grad_segments(desc, q, table, N, go, seg)
    t2 = table.clone()
    with pytest.raises(RuntimeError, match="too wide"):
        nat.neg_pertriple_grad_segments(desc, q, t2, N, go, seg, fused_sgd_lr=0.5)
    assert torch.equal(t2, table)
