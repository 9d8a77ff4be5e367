"""The operand checks and buffer helpers of the binding (`besskge/_native.py`) are written once and called by the
wrappers.  Three things are held here:

1. the helpers themselves, on CPU tensors (only `_same_device` cares where a tensor lives);
2. a table of malformed calls, one row at least for every check that lives in a helper: the exception type and the
   FULL message of each row were recorded from the wrappers as they were before the helpers existed (the file was
   run against that commit first), so a consolidated check that words, orders or types its refusal differently
   fails here.  Every row raises before anything is launched;
3. one correct call per consolidated wrapper pair, at the same tiny shapes, against plain torch / a Python set.
"""

import numpy as np
import pytest
import torch

from besskge import _native as nat

gpu = pytest.mark.gpu


# ===================================================================================== 1. the helpers, device-free
def test_ptr_of_none_is_null():
    t = torch.zeros(3)
    assert nat._ptr(None) == 0
    assert nat._ptr(t) == t.data_ptr() != 0


def test_matrix_check_accepts_and_describes():
    m = torch.zeros(3, 8, dtype=torch.bool)
    assert nat._mat(None, torch.bool, "never") == (0, 0, 0)
    assert nat._mat(m, torch.bool, "never") == (m.data_ptr(), 3, 8)
    assert nat._mat(m, (torch.bool, torch.uint8), "never", rows=(1, 3), cols=8) == (m.data_ptr(), 3, 8)
    assert nat._mat(m[:1], torch.bool, "never", rows=(1, 3), cols=8) == (m.data_ptr(), 1, 8)


@pytest.mark.parametrize("what,make,kw", [
    ("wrong dtype", lambda: torch.zeros(3, 8, dtype=torch.uint8), {}),
    ("dtype outside the tuple", lambda: torch.zeros(3, 8, dtype=torch.int32), {"dtype": (torch.bool, torch.uint8)}),
    ("1-D", lambda: torch.zeros(8, dtype=torch.bool), {}),
    ("3-D", lambda: torch.zeros(1, 3, 8, dtype=torch.bool), {}),
    ("a transposed view", lambda: torch.zeros(8, 3, dtype=torch.bool).t(), {}),
    ("rows outside the set", lambda: torch.zeros(2, 8, dtype=torch.bool), {"rows": (1, 3)}),
    ("wrong columns", lambda: torch.zeros(3, 7, dtype=torch.bool), {"cols": 8}),
])
def test_matrix_check_refuses(what, make, kw):
    t, kw = make(), dict(kw)
    dtype = kw.pop("dtype", torch.bool)
    with pytest.raises(ValueError) as e:
        nat._mat(t, dtype, "the caller's text", **kw)
    assert str(e.value) == "the caller's text", what
    with pytest.raises(ValueError) as e:  # the prefix is joined only here, on the failure branch
        nat._mat(t, dtype, "the caller's text", who="wrapper", **kw)
    assert str(e.value) == "wrapper: the caller's text", what


def r4(n):
    return (n + 3) // 4 * 4


@pytest.mark.parametrize("n", [1, 3, 4, 5])
def test_carve_layout_of_the_row_vectors(n):
    """`pertriple_tail` (row terms | d_pos | loss) and `regularize_triples` (row terms | penalty): the offsets and
    totals of the layouts the wrappers computed by hand (n4 = n rounded up to 4 floats)."""
    n4 = r4(n)
    assert nat._carve_offsets((n, n, 1)) == [0, n4, 2 * n4, 2 * n4 + 4]
    assert nat._carve_offsets((n, 1)) == [0, n4, n4 + 4]


@pytest.mark.parametrize("nq,ld", [(1, 1), (3, 5), (4, 4)])
def test_carve_layout_of_the_shared_forward_loss(nq, ld):
    """scores | score gradients | row terms | d_pos | loss, as `neg_score_shared_fwd_loss` laid them out."""
    mat, nq4 = r4(nq * ld), r4(nq)
    lengths = (nq * ld, nq * ld, nq, nq, 1)
    offs = nat._carve_offsets(lengths)
    assert offs == [0, mat, 2 * mat, 2 * mat + nq4, 2 * mat + 2 * nq4, 2 * mat + 2 * nq4 + 4]
    check_pieces(lengths, offs)


def check_pieces(lengths, offs):
    assert len(offs) == len(lengths) + 1
    for k, n in enumerate(lengths):
        assert offs[k] % 4 == 0  # 16-byte boundary
        assert offs[k] + n <= offs[k + 1]  # no overlap with the next piece, the last one inside the total


@pytest.mark.parametrize("lengths", [(1, 1, 1), (3, 3, 1), (4, 4, 1), (5, 5, 1), (0, 1), (7,), ()])
def test_carve_pieces_are_aligned_and_disjoint(lengths):
    check_pieces(lengths, nat._carve_offsets(lengths))


# ============================================================================================ 2. malformed calls
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda", 0)


R, L, KK = 3, 8, 4          # top-k: rows, candidates, list length
NQ, NC, W = 3, 6, 8         # scoring: queries, shared candidates, row width
NPT = 4                     # negatives per triple of the per-triple forward
N_ENT, N_REL = 12, 3        # the known-triple graph
KNOWN = np.array([[0, 0, 1], [0, 0, 5], [0, 0, 7], [2, 1, 5], [3, 1, 5], [4, 2, 4], [9, 0, 0]], dtype=np.int64)

TOPK_FLAG_RULE = {
    "topk_update": "topk_update: flagged tiles take ids from id_base and no mask",
    "topk_update_excl": "topk_update_excl: flagged tiles take one shared row of ids (or id_base) and no mask",
}
MASK_2D = "negative_mask must be a contiguous 2-D bool tensor"
DQ_MASK = "neg_score_pertriple_fwd_dq: `mask` must be a contiguous 2-D bool / uint8 tensor"
SIDE = "`side` must be contiguous uint8 / bool with 3 entries"
SIDE_INDEX2 = "a `side` vector needs the index of both sides (`index2`)"
L2G = "`local_to_global` must be a contiguous int32 [n_shard, rows per shard] tensor"
KEPT_SHARD = "`kept_shard` needs `local_to_global`"


def z(dev, *shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype, device=dev)


def topk_rows(fn):
    """(id, exception, message, keyword changes) for one of the two top-k wrappers."""
    lists = f"{fn}: best lists must be [rows, kk] (f32 scores, int32 ids)"
    scores = f"{fn}: scores must be float32 [rows, L] with contiguous rows"
    ids = f"{fn}: ids must be a contiguous int32 [1 | rows, L] tensor"
    mask = f"{fn}: mask must be a contiguous bool [1 | rows, L] tensor"
    flags = f"{fn}: flags must be a contiguous uint8 [rows, 4 * ceil(L / 256)] tensor"
    i32, u8, b = torch.int32, torch.uint8, torch.bool
    rows = [
        ("scores-f64", ValueError, scores, lambda d: dict(scores=z(d, R, L, dtype=torch.float64))),
        ("scores-1d", ValueError, scores, lambda d: dict(scores=z(d, L))),
        ("scores-strided-columns", ValueError, scores, lambda d: dict(scores=z(d, L, R).t())),
        ("best-score-f64", ValueError, "`best_score` must be contiguous float32, got torch.float64",
         lambda d: dict(best_score=z(d, R, KK, dtype=torch.float64))),
        ("best-score-1d", ValueError, lists, lambda d: dict(best_score=z(d, KK), best_id=z(d, KK, dtype=i32))),
        ("best-score-rows", ValueError, lists, lambda d: dict(best_score=z(d, 2, KK), best_id=z(d, 2, KK, dtype=i32))),
        ("best-id-shape", ValueError, lists, lambda d: dict(best_id=z(d, R, KK + 1, dtype=i32))),
        ("best-id-int64", ValueError, lists, lambda d: dict(best_id=z(d, R, KK, dtype=torch.int64))),
        ("best-id-not-contiguous", ValueError, lists, lambda d: dict(best_id=z(d, KK, R, dtype=i32).t())),
        ("ids-int64", ValueError, ids, lambda d: dict(ids=z(d, R, L, dtype=torch.int64))),
        ("ids-1d", ValueError, ids, lambda d: dict(ids=z(d, L, dtype=i32))),
        ("ids-columns", ValueError, ids, lambda d: dict(ids=z(d, R, L - 1, dtype=i32))),
        ("ids-rows", ValueError, ids, lambda d: dict(ids=z(d, 2, L, dtype=i32))),
        ("ids-not-contiguous", ValueError, ids, lambda d: dict(ids=z(d, L, R, dtype=i32).t())),
        ("mask-uint8", ValueError, mask, lambda d: dict(mask=z(d, R, L, dtype=u8))),
        ("mask-1d", ValueError, mask, lambda d: dict(mask=z(d, L, dtype=b))),
        ("mask-columns", ValueError, mask, lambda d: dict(mask=z(d, R, L + 1, dtype=b))),
        ("mask-rows", ValueError, mask, lambda d: dict(mask=z(d, 2, L, dtype=b))),
        ("mask-not-contiguous", ValueError, mask, lambda d: dict(mask=z(d, L, R, dtype=b).t())),
        ("flags-with-mask", ValueError, TOPK_FLAG_RULE[fn],
         lambda d: dict(flags=z(d, R, 4, dtype=u8), mask=z(d, 1, L, dtype=b))),
        ("flags-with-row-ids", ValueError, TOPK_FLAG_RULE[fn],
         lambda d: dict(flags=z(d, R, 4, dtype=u8), ids=z(d, R, L, dtype=i32))),
        ("flags-bool", ValueError, flags, lambda d: dict(flags=z(d, R, 4, dtype=b))),
        ("flags-1d", ValueError, flags, lambda d: dict(flags=z(d, 4, dtype=u8))),
        ("flags-rows", ValueError, flags, lambda d: dict(flags=z(d, 2, 4, dtype=u8))),
        ("flags-not-contiguous", ValueError, flags, lambda d: dict(flags=z(d, 4, R, dtype=u8).t())),
        ("flags-columns-not-4", ValueError, flags, lambda d: dict(flags=z(d, R, 3, dtype=u8))),
        ("flags-too-few", ValueError, flags, lambda d: dict(scores=z(d, R, 260), flags=z(d, R, 4, dtype=u8))),
        ("on-the-cpu", RuntimeError, "besskge: `mask` is on cpu; the BESS hot path runs on HIP devices only (there is no "
         "CPU fallback)", lambda d: dict(mask=torch.zeros(R, L, dtype=b))),
    ]
    if fn == "topk_update":
        rows.append(("flags-with-shared-ids", ValueError, TOPK_FLAG_RULE[fn],
                     lambda d: dict(flags=z(d, R, 4, dtype=u8), ids=z(d, 1, L, dtype=i32))))
    else:
        excl = f"{fn}: excl_ptr / excl_ids must be contiguous 1-D int32 tensors"
        together = f"{fn}: excl_ptr and excl_ids go together"
        rows += [
            ("excl-ptr-alone", ValueError, together, lambda d: dict(excl_ptr=z(d, R + 1, dtype=i32))),
            ("excl-ids-alone", ValueError, together, lambda d: dict(excl_ids=z(d, 2, dtype=i32))),
            ("excl-ptr-int64", ValueError, excl,
             lambda d: dict(excl_ptr=z(d, R + 1, dtype=torch.int64), excl_ids=z(d, 2, dtype=i32))),
            ("excl-ids-2d", ValueError, excl,
             lambda d: dict(excl_ptr=z(d, R + 1, dtype=i32), excl_ids=z(d, 1, 2, dtype=i32))),
            ("excl-ptr-length", ValueError, f"{fn}: excl_ptr has 3 entries, expected rows + 1 = 4",
             lambda d: dict(excl_ptr=z(d, R, dtype=i32), excl_ids=z(d, 2, dtype=i32))),
        ]
    return [pytest.param(fn, exc, msg, change, id=f"{fn}-{name}") for name, exc, msg, change in rows]


@gpu
@pytest.mark.parametrize("fn,exc,msg,change", topk_rows("topk_update") + topk_rows("topk_update_excl"))
def test_topk_wrappers_refuse(dev, fn, exc, msg, change):
    kw = dict(scores=z(dev, R, L), best_score=z(dev, R, KK), best_id=z(dev, R, KK, dtype=torch.int32))
    kw.update(change(dev))
    with pytest.raises(exc) as e:
        getattr(nat, fn)(**kw)
    assert str(e.value) == msg


def bad_masks(dev, rows, cols, wrong_dtype):
    """(more than one row: a transposed [cols, 1] matrix IS contiguous)"""
    strided = z(dev, cols, rows, dtype=torch.bool).t()
    assert rows > 1 and not strided.is_contiguous()
    return [("dtype", z(dev, rows, cols, dtype=wrong_dtype)), ("1d", z(dev, cols, dtype=torch.bool)),
            ("3d", z(dev, 1, rows, cols, dtype=torch.bool)), ("not-contiguous", strided)]


def scoring_operands(dev):
    table = z(dev, NC, W)
    d = nat.make_desc(nat.TRANSE, 1, table, W)
    return d, z(dev, NQ, W), nat.RowSource(table)


@gpu
def test_mask_scores_refuses(dev):
    for what, mask in bad_masks(dev, NQ, NC, torch.uint8):
        with pytest.raises(ValueError) as e:
            nat.mask_scores(z(dev, NQ, NC), 0, False, 0, mask)
        assert str(e.value) == MASK_2D, what
    with pytest.raises(ValueError) as e:
        nat.mask_scores(z(dev, NC), 0, False, 0, None)
    assert str(e.value) == "negative_score must be 2-D"


@gpu
@pytest.mark.parametrize("with_loss", [False, True], ids=["neg_score_shared_fwd", "neg_score_shared_fwd_loss"])
def test_shared_forwards_refuse_a_bad_kill_mask(dev, with_loss):
    d, query, neg = scoring_operands(dev)
    for what, mask in bad_masks(dev, NQ, NC, torch.uint8):
        with pytest.raises(ValueError) as e:
            if with_loss:
                nat.neg_score_shared_fwd_loss(d, nat.LossDesc(), query, neg, z(dev, NQ), z(dev, 1), kill=(0, False, 0, mask))
            else:
                nat.neg_score_shared_fwd(d, query, neg, kill=(0, False, 0, mask))
        assert str(e.value) == MASK_2D, what
    with pytest.raises(RuntimeError) as e:
        cpu_mask = torch.zeros(1, NC, dtype=torch.bool)
        if with_loss:
            nat.neg_score_shared_fwd_loss(d, nat.LossDesc(), query, neg, z(dev, NQ), z(dev, 1), kill=(0, False, 0, cpu_mask))
        else:
            nat.neg_score_shared_fwd(d, query, neg, kill=(0, False, 0, cpu_mask))
    assert str(e.value) == ("besskge: `negative_mask` is on cpu; the BESS hot path runs on HIP devices only (there is no "
                            "CPU fallback)")


@gpu
def test_fused_pertriple_forward_refuses(dev):
    table = z(dev, NC, W)
    d = nat.make_desc(nat.DISTMULT, 0, table, W)
    neg = nat.RowSource(table, z(dev, NQ * NPT, dtype=torch.int32))
    query, l = z(dev, NQ, W), nat.LossDesc()
    cases = [
        ("`weight` must be contiguous float32, got torch.float64",
         dict(pos=z(dev, NQ), weight=z(dev, 1, dtype=torch.float64))),
        ("triple weights must have 1 or n_query entries", dict(pos=z(dev, NQ), weight=z(dev, 2))),
        ("`pos` must be contiguous float32, got torch.float64", dict(pos=z(dev, NQ, dtype=torch.float64), weight=z(dev, 1))),
        ("`pos` must have n_query entries", dict(pos=z(dev, NQ - 1), weight=z(dev, NQ))),
    ]
    cases += [(DQ_MASK, dict(pos=None, weight=z(dev, 1), mask=m)) for _, m in bad_masks(dev, NQ, NPT, torch.int32)]
    for msg, kw in cases:
        with pytest.raises(ValueError) as e:
            nat.neg_score_pertriple_fwd_dq(d, l, query, neg, NPT, **kw)
        assert str(e.value) == msg


@pytest.fixture(scope="module")
def graph(dev):
    from besskge.negative_filter import SIDE_HEAD, SIDE_TAIL, KnownTripleFilter

    flt = KnownTripleFilter([KNOWN], N_ENT, N_REL, device=dev)
    return flt.index[SIDE_TAIL], flt.index[SIDE_HEAD]


def known_rows(dev):
    kept = torch.tensor([0, 5, 4], dtype=torch.int32, device=dev)
    rel = torch.tensor([0, 1, 2], dtype=torch.int32, device=dev)
    side = torch.tensor([0, 1, 0], dtype=torch.uint8, device=dev)  # row 1: which heads complete (?, 1, 5)
    return kept, rel, side


@gpu
@pytest.mark.parametrize("fn", ["known_triple_mask", "known_completions"])
def test_known_triple_wrappers_refuse(dev, graph, fn):
    tails, heads = graph
    kept, rel, side = known_rows(dev)
    i32 = torch.int32

    def call(**kw):
        if fn == "known_triple_mask":
            cand, mask = z(dev, 3, 4, dtype=i32), z(dev, 3, 4, dtype=torch.uint8)
            return nat.known_triple_mask(tails, kept, rel, cand, mask, N_REL, **kw)
        return nat.known_completions(tails, kept, rel, N_REL, counts=z(dev, 3, dtype=i32), **kw)

    cases = [
        (SIDE, dict(index2=heads, side=z(dev, 3, dtype=i32))),
        (SIDE, dict(index2=heads, side=z(dev, 2, dtype=torch.uint8))),
        (SIDE, dict(index2=heads, side=z(dev, 3, 2, dtype=torch.uint8)[:, 0])),
        (SIDE_INDEX2, dict(side=side)),
        (L2G, dict(local_to_global=z(dev, 2, 6, dtype=torch.int64))),
        (L2G, dict(local_to_global=z(dev, 12, dtype=i32))),
        (L2G, dict(local_to_global=z(dev, 6, 2, dtype=i32).t())),
        (KEPT_SHARD, dict(kept_shard=z(dev, 3, dtype=i32))),
        ("`kept_shard` has 2 elements, expected 3",
         dict(kept_shard=z(dev, 2, dtype=i32), local_to_global=z(dev, 2, 6, dtype=i32))),
        ("`index2 offsets` has 3 elements, expected 4",
         dict(index2=(z(dev, 3, dtype=torch.int64), z(dev, 3, dtype=torch.int64), z(dev, 3, dtype=i32)))),
    ]
    if fn == "known_triple_mask":
        cover = "`local_to_global` does not cover the candidates' shards"
        cases += [(cover, dict(local_to_global=z(dev, 2, 6, dtype=i32), cand_shard=2)),
                  (cover, dict(local_to_global=z(dev, 1, 6, dtype=i32), cols_per_block=2, block_stride=2))]
    for msg, kw in cases:
        with pytest.raises(ValueError) as e:
            call(**kw)
        assert str(e.value) == msg


# ================================================================================================ 3. correct calls
def distinct_scores(gen):
    """[R, L] scores without ties: every row a permutation of 0 .. L - 1, plus the row number / 10."""
    return torch.stack([torch.randperm(L, generator=gen).float() + r / 10 for r in range(R)])


@gpu
def test_topk_update_accepts_ids_and_a_mask(dev):
    gen = torch.Generator().manual_seed(1)
    sc = distinct_scores(gen)
    ids = (100 + torch.randperm(L, generator=gen)).to(torch.int32)[None, :]
    mask = torch.ones(R, L, dtype=torch.bool)
    mask[0, sc[0].argmax()] = False   # the best candidate of row 0 is masked out
    mask[2, :3] = False
    bs = torch.full((R, KK), -50000.0, device=dev)
    bi = torch.full((R, KK), -1, dtype=torch.int32, device=dev)
    nat.topk_update(sc.to(dev), bs, bi, ids=ids.to(dev), mask=mask.to(dev))
    want = torch.topk(torch.where(mask, sc, sc - 50000.0), KK, dim=1)
    assert float(want.values.min()) > -40000  # (every row keeps KK unmasked candidates)
    assert torch.equal(bs.cpu(), want.values)
    assert torch.equal(bi.cpu(), ids.expand(R, L).gather(1, want.indices))


@gpu
def test_topk_update_excl_accepts_row_ids_and_exclusions(dev):
    gen = torch.Generator().manual_seed(2)
    sc = distinct_scores(gen)
    ids = torch.stack([100 + torch.randperm(L, generator=gen) for _ in range(R)]).to(torch.int32)
    excluded = torch.zeros(R, L, dtype=torch.bool)
    excluded[0, sc[0].argmax()] = True
    excluded[2, 1::2] = True
    lists = [sorted(ids[r][excluded[r]].tolist()) for r in range(R)]
    ptr = torch.tensor(np.cumsum([0] + [len(x) for x in lists]), dtype=torch.int32, device=dev)
    flat = torch.tensor([i for x in lists for i in x], dtype=torch.int32, device=dev)
    bs = torch.full((R, KK), -torch.inf, device=dev)
    bi = torch.full((R, KK), nat.TOPK_ID_NONE, dtype=torch.int32, device=dev)
    nat.topk_update_excl(sc.to(dev), bs, bi, ids=ids.to(dev), excl_ptr=ptr, excl_ids=flat)
    want = torch.topk(torch.where(excluded, torch.full_like(sc, -torch.inf), sc), KK, dim=1)
    assert bool(torch.isfinite(want.values).all())
    assert torch.equal(bs.cpu(), want.values)
    assert torch.equal(bi.cpu(), ids.gather(1, want.indices))


def is_known(kept, rel, side, cand):
    return ((cand, rel, kept) if side else (kept, rel, cand)) in {tuple(int(x) for x in t) for t in KNOWN}


@gpu
def test_known_triple_mask_accepts_two_sided_rows(dev, graph):
    tails, heads = graph
    kept, rel, side = known_rows(dev)
    cand = torch.tensor([[1, 2, 5, 7], [2, 3, 4, 5], [4, 0, 11, 4]], dtype=torch.int32)
    mask = torch.full((3, 4), 7, dtype=torch.uint8, device=dev)
    nat.known_triple_mask(tails, kept, rel, cand.to(dev), mask, N_REL, index2=heads, side=side)
    want = [[not is_known(int(kept[i]), int(rel[i]), int(side[i]), int(c)) for c in cand[i]] for i in range(3)]
    assert want == [[False, True, False, False], [False, False, True, True], [False, True, True, False]]
    assert mask.cpu().tolist() == [[int(x) for x in row] for row in want]


@gpu
def test_known_completions_counts_two_sided_rows(dev, graph):
    tails, heads = graph
    kept, rel, side = known_rows(dev)
    counts = torch.full((3,), -1, dtype=torch.int32, device=dev)
    skip = torch.tensor([5, -1, -1], dtype=torch.int32, device=dev)  # row 0: tail 5 is not counted
    got = nat.known_completions(tails, kept, rel, N_REL, index2=heads, side=side, skip=skip, counts=counts)
    assert got is counts
    want = [sum(is_known(int(kept[i]), int(rel[i]), int(side[i]), c) and c != int(skip[i]) for c in range(N_ENT))
            for i in range(3)]
    assert want == [2, 2, 1]
    assert counts.cpu().tolist() == want


@gpu
def test_shared_forward_accepts_a_kill_mask(dev):
    """Small integers: the L1 scores and the score of a killed cell (+ BAD_NEGATIVE_SCORE) are exact in fp16 and
    fp32 in any order of summation, so the comparison is for equality."""
    gen = torch.Generator().manual_seed(3)
    table = torch.randint(-3, 4, (NC, W), generator=gen).float()
    query = torch.randint(-3, 4, (NQ, W), generator=gen).float()
    mask = torch.tensor([[True, False, True, False]])  # over the last four candidates of every row
    d = nat.make_desc(nat.TRANSE, 1, table, W)
    got = nat.neg_score_shared_fwd(d, query.to(dev), nat.RowSource(table.to(dev)), kill=(0, False, 0, mask.to(dev)))
    want = -(query[:, None, :] - table[None, :, :]).abs().sum(-1)
    want[:, NC - 4:] += torch.where(mask, 0.0, nat.BAD_NEGATIVE_SCORE)
    assert tuple(got.shape) == (NQ, NC)
    assert torch.equal(got.cpu(), want)
