"""The fused forms a training step launches - `k_neg_pertriple_fwd<..., FUSE = true>` behind
`bess_neg_score_pertriple_fwd_dq` / `_fwd_dq_masked` / `_fwd_partials` (csrc/neg_pertriple.hip), `k_pertriple_tail`,
`k_query_triple_bwd_parts` and `k_query_triple_fwd_jobs` (csrc/prepare.hip) and the table form of `k_aff_shared_fwd` at
p = 2 (csrc/affine.hip) - against float64, in every class their host code selects.  The other tests compare them with
the separate launches they replace (which tests/test_pertriple_kernels.py, test_mask_loss_rank_kernels.py and
test_row_update_kernels.py anchor); this file anchors the fused forms themselves.

  0. the reference, on the CPU (no device): the header's per-item partials (m_i, l_i, acc_i) and their combination
     C_q / L sum_i exp(m_i - m) acc_i, written in float64, == `rule` + `oracle.kge.loss_value` + float64 autograd;
     the step's tail as one float64 autograd chain from the tables == `prepare_references`; the class of every case;
  1. the fused forward in every (T, VEC, IT, RED) class of test_pertriple_kernels.py's table, 5 queries x 37 and x 7
     negatives over 97 rows, all five (kind, adversarial) losses, in the regimes
       normal     randn * 0.3
       ties       section 14's: a third of a query's columns equal a negative's, negative 0 is the query
       saturated  amplitude 6: scores of +-1e3, a one-hot softmax
       exact      tables and queries in {-2 .. 2}, integer margin and positives: DOT, L1 and p = 2 scores are exact
                  (== float64 rounded once), three negatives sit exactly on the margin loss's hinge (step 0 there;
                  p = 3 goes through powf: within the bound, and no negative on the hinge)
       masked     `_fwd_dq_masked`, mask rows 1 and n_query, 14 of 37 columns (mask_from = 23: inside an item, not a
                  multiple of 4), one query's mask row all zero
     plus 5 x 1028 negatives (129 items of 8: the item loops of `combine_dq_row` stride over 64 lanes), the refusals
     and the partials of two shards;
  2. `bess_pertriple_tail` in its 16 (T, SCORER, CH) classes, 4 / 8 / 16 waves per workgroup, hand-made partials at
     W = 4096 (2 waves), refusals;
  3. `bess_query_triple_bwd_parts` in its 8 classes, both sides, W = 6, 128, 260 and 4096, on hand-made slabs;
  4. `bess_query_triple_fwd_jobs` in its 8 classes, both sides, with copy / fill jobs checked word for word;
  5. the affine table form at p = 2 (the cases added to test_fused_ranks_scorers.py): kernel names, scores == float64.

Bounds: the project's rtol 1e-4, atol max(1e-5, 2e-6 max|want|) through `check` of test_pertriple_kernels.py (4 x the
fp32 restatement's error where that is itself outside the bound); the losses and the gradients of the scores keep
section 13's (`LOSS_TOL`, `GRAD_TOL`, `close64`).  The restatement of the fused d_query sums a row's terms in two orders
(`fused_restatement`): d_query depends on the scores through exp(beta s), and on long L1 rows with a peaked softmax one
ulp of a score - what two fp32 summation orders differ by - is worth more than the bound (DESIGN.md section 21 lists
the cases).  Exact: `out` against the plain forward, the scores of the exact
regime, job results, untouched outputs, counters.  Every case asserts its kernel by name where the class is one of
DESIGN.md section 18's open ones.  Measured errors: DESIGN.md, section 21."""

import ctypes
import functools

import numpy as np
import pytest
import torch

from besskge import _native as nat
from oracle import kge
from test_mask_loss_rank_kernels import GRAD_TOL, LOSS_TOL, VARIANTS, close64, error_in_tolerances
from test_pertriple_kernels import (CLASS_WIDTHS, COMPLEX_CASES, COMPLEX_REDS, EUNSUPPORTED, F16, F32, MEASURED, NQ, REDS,
                                    ROWS, SIDES, WINDOW_WIDTHS, check, dispatch_class, forward, inputs, items_of,
                                    make_desc, nan, prepare_inputs, prepare_references, rule, status, tname, units)
from test_tile_dispatch_classes import kernel_launched, launched

gpu = pytest.mark.gpu
EINVAL = -1  # BESS_EINVAL
MARGIN, BETA, LOSS_SCALE, N_ENTITY = 2.0, float(np.float32(0.7)), 3.0, 5000
BAD = kge.BAD_NEGATIVE_SCORE
KIND_CODE = dict(logsigmoid=nat.LOSS_LOGSIGMOID, margin=nat.LOSS_MARGIN, ssce=nat.LOSS_SSCE)
SCORER_CODE = dict(TransE=nat.TRANSE, RotatE=nat.ROTATE, DistMult=nat.DISTMULT, ComplEx=nat.COMPLEX)
N_NEG, N_ONE_ITEM, MASK_COLS = 37, 7, 14
MANY = 1028  # 129 items of 8 negatives
PAD = 8      # floats behind the partials that must stay NaN


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda", 0)


def loss_desc(variant, n_neg):
    kind, adv = VARIANTS[variant]
    l = nat.LossDesc()
    l.kind, l.adversarial, l.margin, l.adversarial_scale, l.loss_scale = KIND_CODE[kind], int(adv), MARGIN, BETA, LOSS_SCALE
    l.ssce_shift = float(np.log(N_ENTITY - 1) - np.log(n_neg))
    return l


def loss_value(variant, pos, neg, w):
    kind, adv = VARIANTS[variant]
    return kge.loss_value(kind, pos, neg, w, margin=MARGIN, adversarial=adv, adversarial_scale=BETA, loss_scale=LOSS_SCALE,
                          n_entity=N_ENTITY)


# ============================================================================================ 0. the reference
def loss_chain(variant, pos, neg, w, dtype):
    """(loss, d_pos, d_neg) of `oracle.kge.loss_value` with autograd in `dtype`; w [S]."""
    po, no = (x.detach().to(dtype, copy=True).requires_grad_(True) for x in (pos, neg))
    loss = loss_value(variant, po, no, w.to(dtype))
    d_pos, d_neg = torch.autograd.grad(loss, (po, no))
    return loss.detach(), d_pos, d_neg


def fused_reference(red, query, rows, pos, w, variant, dtype, kill=None):
    """The fused forward stated in `dtype`: (scores [S, N] with BESS_BAD_NEGATIVE_SCORE added where `kill`, d_query)."""
    s = rule(red, query, rows, torch.zeros(rows.shape[:2]), dtype)[0]
    if kill is not None:
        s = torch.where(kill, s + BAD, s)
    g = loss_chain(variant, pos, s, w, dtype)[2]
    return s, rule(red, query, rows, g, dtype)[1]


def sequential_scores(red, query, rows):
    """The rule's scores in fp32 with the W terms of a row added one after the other.  `rule` in fp32 adds them pairwise
    (torch.sum) and the kernels in the order of the register layout: three roundings of one sum, an ulp or so apart."""
    p = (REDS.get(red) or COMPLEX_REDS[red])[2]
    q, e = query.float()[:, None, :], rows.float()
    dot = red in ("dot", "complex")
    x = q * e if dot else ((q - e).abs() if p == 1 else (q - e).abs().pow(p))
    x = x.permute(2, 0, 1).contiguous()
    acc = torch.zeros(x.shape[1:])
    for j in range(x.shape[0]):
        acc = acc + x[j]
    return acc if dot else -(acc if p == 1 else acc.pow(1.0 / p))


def fused_restatement(red, query, rows, pos, w, variant, kill, dq64, s_seq):
    """The fp32 restatement of the fused d_query whose error sizes the ill-conditioned cases: d_query depends on the
    scores through exp(beta s), so where a softmax weight is large and the row's terms cancel, one ulp of a score (all
    that two fp32 summation orders of a long row agree to) moves an element by more than the bound.  The scores are
    summed pairwise and one term after the other; the restatement further from float64 is the one that counts."""
    cands = [fused_reference(red, query, rows, pos, w, variant, torch.float32, kill)[1]]
    s = s_seq if kill is None else torch.where(kill, s_seq + BAD, s_seq)
    cands.append(rule(red, query, rows, loss_chain(variant, pos, s, w, torch.float32)[2], torch.float32)[1])
    return max(cands, key=lambda dq: units(dq, dq64))


def partials64(red, query, rows, pos, variant, nb, kill=None, dtype=torch.float64):
    """state_ml [S, items, 2] = (m_i, l_i) and state_acc [S, items, W] as include/besskge_hip.h states them: item i holds
    the negatives [i nb, (i + 1) nb); z = beta (s + shift), m_i = max z, l_i = sum exp(z - m_i),
    acc_i = sum exp(z - m_i) g(s) ds/dq with g = sigmoid(s + margin) | [s - pos + margin > 0] | 1."""
    kind, adv = VARIANTS[variant]
    s = rule(red, query, rows, torch.zeros(rows.shape[:2]), dtype)[0]
    if kill is not None:
        s = torch.where(kill, s + BAD, s)
    beta = 1.0 if kind == "ssce" else (BETA if adv else 0.0)
    shift = float(np.log(N_ENTITY - 1) - np.log(s.shape[1])) if kind == "ssce" else 0.0
    z = beta * (s + shift)
    if kind == "logsigmoid":
        gs = torch.sigmoid(s + MARGIN)
    elif kind == "margin":
        gs = (s - pos.to(dtype)[:, None] + MARGIN > 0).to(dtype)
    else:
        gs = torch.ones_like(s)
    ml, acc = [], []
    for k0 in range(0, s.shape[1], nb):
        zi = z[:, k0: k0 + nb]
        m = zi.max(1).values
        e = torch.exp(zi - m[:, None])
        ml.append(torch.stack([m, e.sum(1)], dim=1))
        acc.append(rule(red, query, rows[:, k0: k0 + nb], e * gs[:, k0: k0 + nb], dtype)[1])
    return torch.stack(ml, dim=1), torch.stack(acc, dim=1)


def combine64(ml, acc, pos, w, variant, norm=None):
    """d_query [S, W] = C_q / L sum_i exp(m_i - m) acc_i in float64; m and L over the items (and the positive: ssce), or
    from `norm` [S, 2] = (m, L / C_q); an item with m_i = -inf holds nothing."""
    kind, _ = VARIANTS[variant]
    ml, acc = ml.double(), acc.double()
    mi, li = ml[..., 0], ml[..., 1]
    if norm is not None:
        m, l_over_c = norm[:, 0].double(), norm[:, 1].double()
        scale = torch.where((l_over_c > 0) & (l_over_c < float("inf")), 1.0 / l_over_c, torch.zeros_like(l_over_c))
    else:
        m = mi.max(1).values
        if kind == "ssce":
            m = torch.maximum(m, pos.double())
    f = torch.where(mi == -float("inf"), torch.zeros_like(mi), torch.exp(mi - m[:, None]))
    if norm is None:
        L = (torch.where(mi == -float("inf"), torch.zeros_like(li), li) * f).sum(1)
        if kind == "ssce":
            L = L + torch.exp(pos.double() - m)
        scale = (0.5 if kind == "logsigmoid" else 1.0) * LOSS_SCALE * w.double() / L
    return scale[:, None] * (f[:, :, None] * acc).sum(1)


def triple_grads(name, p, side, ent, rel, hidx, tidx, rid, d_out, d_query, ftype):
    """(d_head [S, W], d_tail [S, W], d_rel_table) of sum(pos d_out) + sum(query d_query): `oracle.kge` in `ftype` on leaf
    copies of the gathered rows - what bess_query_triple_bwd computes."""
    h = ent[hidx.long()].to(ftype).requires_grad_(True)
    t = ent[tidx.long()].to(ftype).requires_grad_(True)
    R = rel.to(ftype).requires_grad_(True)
    pos = kge.score_triple(name, p, h, R, rid, t)
    qy = kge.query(name, side, h if side == "t" else t, R[rid.long()])
    return torch.autograd.grad((pos * d_out.to(ftype)).sum() + (qy * d_query.to(ftype)).sum(), (h, t, R))


def tail_chain(name, p, side, ent, rel, hidx, tidx, rid, nidx, w, variant, ftype):
    """The step from the tables to the gradients in one autograd graph of `ftype`: head, tail and relation rows as
    leaves, positive score, query, negative scores (the negatives' rows are constants: their share is K5's), loss."""
    h = ent[hidx.long()].to(ftype).requires_grad_(True)
    t = ent[tidx.long()].to(ftype).requires_grad_(True)
    R = rel.to(ftype).requires_grad_(True)
    pos = kge.score_triple(name, p, h, R, rid, t)
    qy = kge.query(name, side, h if side == "t" else t, R[rid.long()])
    neg = kge._reduce(name, p, qy[:, None, :], ent[nidx.long()].to(ftype))
    loss = loss_value(variant, pos, neg, w.to(ftype))
    d_pos, d_neg, d_query, dh, dt, dR = torch.autograd.grad(loss, (pos, neg, qy, h, t, R))
    return dict(pos=pos.detach(), query=qy.detach(), neg=neg.detach(), loss=loss.detach(), d_pos=d_pos, d_neg=d_neg,
                d_query=d_query, d_head=dh, d_tail=dt, d_rel=dR)


@functools.lru_cache(maxsize=16)
def fused_inputs(dtype, W, regime, n_neg, red, nq=NQ):
    """(query, table, idx, pos, w, masks) on the CPU, never written to.  pos - margin sits in the middle of the widest
    gap of the middle half of each query's sorted float64 scores (the margin loss's step is then the same in every
    precision); in the exact regime it equals three negatives' score to the bit."""
    gen = torch.Generator().manual_seed(7 * W + n_neg + len(regime) + len(red) + (5 if dtype == F16 else 0))
    if regime == "saturated":
        table = (torch.randn(ROWS, W, generator=gen) * 6).to(dtype)
        query = torch.randn(nq, W, generator=gen) * 6
        idx = torch.randint(0, ROWS, (nq, n_neg), generator=gen).to(torch.int32)
    elif regime == "exact":
        table = torch.randint(-2, 3, (ROWS, W), generator=gen).to(dtype)
        query = torch.randint(-2, 3, (nq, W), generator=gen).float()
        idx = torch.randint(0, ROWS, (nq, n_neg), generator=gen).to(torch.int32)
        idx[:, 5], idx[:, n_neg - 1] = idx[:, 3], idx[:, 3]
    else:
        query, table, idx, _ = inputs(dtype, W, "ties" if regime == "ties" else "normal", n_neg, nq)
    s = rule(red, query, table[idx.long()], torch.zeros(nq, n_neg))[0]
    if regime == "exact" and red != "l3":
        pos = (s[:, 3].round() + MARGIN).float()
    else:  # (p = 3 goes through powf: a perfect cube's root is an integer in neither precision, no hinge is put on it)
        srt = s.sort(1).values
        lo, hi = n_neg // 4, 3 * n_neg // 4
        gap = srt[:, lo + 1: hi + 1] - srt[:, lo:hi]
        at = gap.argmax(1) + lo
        rows = torch.arange(nq)
        pos = (0.5 * (srt[rows, at] + srt[rows, at + 1]) + MARGIN).float()
    w = torch.rand(nq, generator=gen) + 0.5
    masks = None
    if regime == "masked":
        one = torch.rand(1, MASK_COLS, generator=gen) > 0.3
        per_query = torch.rand(nq, MASK_COLS, generator=gen) > 0.3
        per_query[2] = False
        masks = (one, per_query)
    return query, table, idx, pos, w, masks


def kill_of(mask, nq, n_neg):
    """[nq, n_neg] bool: the columns a mask over the last columns masks out."""
    kill = torch.zeros(nq, n_neg, dtype=torch.bool)
    kill[:, n_neg - mask.shape[1]:] = ~mask.expand(nq, mask.shape[1])
    return kill


@pytest.mark.parametrize("one_weight", [False, True])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_partial_form_equals_the_float64_reference(variant, one_weight):
    """CPU check 1: items of 8, both weight forms, all five losses; with and without a mask."""
    for dtype, W, red, regime in [(F32, 100, "l1", "normal"), (F16, 50, "dot", "ties"), (F32, 6, "l2", "masked"),
                                  (F32, 30, "dot", "exact"), (F16, 66, "l3", "saturated")]:
        query, table, idx, pos, w, masks = fused_inputs(dtype, W, regime, N_NEG, red)
        w = (w[:1] if one_weight else w).expand(NQ)
        rows = table[idx.long()]
        kill = kill_of(masks[1], NQ, N_NEG) if masks else None
        s, want = fused_reference(red, query, rows, pos, w, variant, torch.float64, kill)
        ml, acc = partials64(red, query, rows, pos, variant, 8, kill)
        assert ml.shape == (NQ, 5, 2) and acc.shape == (NQ, 5, W)
        got = combine64(ml, acc, pos, w, variant)
        torch.testing.assert_close(got, want, rtol=1e-11, atol=1e-13 * max(1.0, float(want.abs().max())))
        assert float(want.abs().max()) > 0 or (variant == "logsigmoid" and regime == "saturated")
        if regime == "exact" and variant.startswith("margin"):  # on the hinge: no gradient, as relu
            g = loss_chain(variant, pos, s, w, torch.float64)[2]
            assert bool((s[:, 3] - pos.double() + MARGIN == 0).all()) and bool((g[:, [3, 5, N_NEG - 1]] == 0).all())


TAIL_CPU_CASES = [("TransE", 1, F32, 50, "t"), ("RotatE", 2, F16, 50, "h"), ("DistMult", 0, F32, 128, "h"),
                  ("ComplEx", 0, F16, 3, "t")]


@pytest.mark.parametrize("name,p,dtype,d,side", TAIL_CPU_CASES)
def test_tail_chain_equals_the_prepare_references(name, p, dtype, d, side):
    """CPU check 2: `triple_grads` == `prepare_references` of test_pertriple_kernels.py on its inputs; the one-graph
    chain == loss gradients fed to `triple_grads`."""
    ent, rel, hidx, tidx, rid, d_out, d_query, d_rel0 = prepare_inputs(name, p, dtype, d)
    ref = prepare_references(name, p, dtype, d, torch.float64)
    dh, dt, dr = triple_grads(name, p, side, ent, rel, hidx, tidx, rid, d_out, d_query, torch.float64)
    wh, wt, wr = ref["query_triple_bwd", side]
    for got, want in ((dh, wh), (dt, wt), (d_rel0.double() + dr, wr)):
        torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-13)
    gen = torch.Generator().manual_seed(d)
    nidx = torch.randint(0, ent.shape[0], (len(hidx), 8), generator=gen)
    w = torch.rand(len(hidx), generator=gen) + 0.5
    for variant in VARIANTS:
        c = tail_chain(name, p, side, ent, rel, hidx, tidx, rid, nidx, w, variant, torch.float64)
        torch.testing.assert_close(c["pos"], ref["score"], rtol=1e-12, atol=1e-13)
        torch.testing.assert_close(c["query"], ref["query", side], rtol=1e-12, atol=1e-13)
        loss, d_pos, d_neg = loss_chain(variant, c["pos"], c["neg"], w, torch.float64)
        torch.testing.assert_close(c["loss"], loss, rtol=1e-13, atol=0)
        torch.testing.assert_close(c["d_pos"], d_pos, rtol=1e-12, atol=1e-14)
        torch.testing.assert_close(c["d_neg"], d_neg, rtol=1e-12, atol=1e-14)
        parts = triple_grads(name, p, side, ent, rel, hidx, tidx, rid, c["d_pos"], c["d_query"], torch.float64)
        for got, want in zip((c["d_head"], c["d_tail"], c["d_rel"]), parts):
            torch.testing.assert_close(got, want, rtol=1e-11, atol=1e-13)


# name, p, dtype, S, n_neg, W, side, loss, one triple at distance 0
TAIL_CASES = [
    ("TransE", 1, F32, 9, 8, 6, "t", "logsigmoid_adv", False),
    ("TransE", 2, F32, 9, 1028, 128, "h", "margin", True),
    ("RotatE", 1, F32, 9, 1024, 128, "t", "ssce", False),
    ("RotatE", 2, F32, 9, 3072, 6, "h", "margin_adv", True),
    ("DistMult", 0, F32, 1027, 8, 128, "t", "logsigmoid", False),
    ("DistMult", 0, F32, 9, 1028, 6, "h", "ssce", False),
    ("ComplEx", 0, F32, 9, 8, 1024, "t", "margin_adv", False),
    ("ComplEx", 0, F32, 9, 1028, 128, "h", "logsigmoid", False),
    ("TransE", 1, F16, 9, 1024, 128, "h", "logsigmoid", False),
    ("TransE", 2, F16, 9, 3072, 6, "t", "ssce", True),
    ("RotatE", 1, F16, 9, 8, 2048, "t", "margin", False),
    ("RotatE", 2, F16, 9, 1028, 128, "h", "logsigmoid_adv", True),
    ("DistMult", 0, F16, 9, 8, 6, "h", "margin_adv", False),
    ("DistMult", 0, F16, 9, 1028, 128, "t", "logsigmoid_adv", False),
    ("ComplEx", 0, F16, 1027, 8, 128, "h", "ssce", False),
    ("ComplEx", 0, F16, 9, 1028, 6, "t", "margin", False),
    # more than 1024 triples of rows that no longer fit 16 to a workgroup's 32 KB: 8 and 4 waves
    ("DistMult", 0, F32, 1027, 8, 1024, "t", "ssce", False),
    ("DistMult", 0, F16, 1027, 8, 2048, "h", "logsigmoid", False),
]
PARTS_W = (6, 128, 260, 4096)
JOBS_D = (3, 50, 128)
AFFINE_P2 = [("PairRE", 2, F16, False, 128, 1), ("PairRE", 2, F32, True, 64, 1), ("TranS", 2, F16, True, 64, 2)]


def tail_waves(S, W):
    """`tail_waves` of csrc/prepare.hip: 16 waves from 1025 triples, else 4; halved while their rows exceed 32 KB."""
    nw = 16 if S > 1024 else 4
    while nw > 1 and nw * W * 4 > (32 << 10):
        nw //= 2
    return nw


def tail_class(name, dtype, S, n_neg, W):
    return (dtype, SCORER_CODE[name], 4 if n_neg <= 1024 else 12), tail_waves(S, W)


FUSED_CASES = [(dt, W, red) for (dt, _), its in CLASS_WIDTHS.items() for ws in its.values() for W in ws for red in REDS] \
    + list(COMPLEX_CASES)
PARTIAL_WIDTHS = [(dt, its[it][0]) for (dt, vec), its in CLASS_WIDTHS.items() if vec in (4, 8) for it in (1, 2, 4, 8, 16)]


def test_classes_of_the_cases():
    """CPU check 3: the class each case below selects (DESIGN.md section 21 prints this)."""
    fused = {}
    for dtype, W, red in FUSED_CASES:
        (vec, it, cols), = dispatch_class(dtype, W)
        kind = "dot" if red in ("dot", "complex") else ("l1" if red in ("l1", "rotate_l1") else "lp")
        fused.setdefault((tname(dtype), vec, it, kind), []).append(W)
        desc = make_desc(red, torch.empty((0, W), dtype=dtype))
        assert items_of(desc, NQ, N_NEG) == 5 and items_of(desc, NQ, N_ONE_ITEM) == 1
    assert len(fused) == 25 * 3, "every (T, VEC, IT) x (DOT, L1, L2) instantiation of the fused forward"
    for dtype, W in [(F32, 60), (F16, 264)]:
        desc = make_desc("l1", torch.empty((0, W), dtype=dtype))
        assert items_of(desc, NQ, MANY) == 129 > 64
    for (dtype, W), windows in WINDOW_WIDTHS.items():
        assert len(dispatch_class(dtype, W)) == len(windows) > 1
    assert sorted({dispatch_class(dt, W)[0][1] for dt, W in PARTIAL_WIDTHS}) == [1, 2, 4, 8, 16] and len(PARTIAL_WIDTHS) == 10
    tails = {}
    for name, p, dtype, S, n_neg, W, side, variant, zero in TAIL_CASES:
        cls, nw = tail_class(name, dtype, S, n_neg, W)
        tails.setdefault(cls, []).append((S, n_neg, W, nw))
        assert not zero or (p == 2 and name in ("TransE", "RotatE"))
    assert len(tails) == 16, "every (T, SCORER, CH) instantiation of k_pertriple_tail"
    assert {nw for v in tails.values() for *_, nw in v} == {4, 8, 16} and tail_waves(9, 4096) == 2
    assert {(s, sd) for s, *_, sd, _, _ in TAIL_CASES} == {(s, sd) for s in SCORER_CODE for sd in "th"}
    for text in sorted(f"fused {k}: W = {v}" for k, v in fused.items()) + \
            sorted(f"tail <{tname(k[0])}, {k[1]}, {k[2]}>: (S, n_neg, W, waves) = {v}" for k, v in tails.items()):
        print(text)


# ============================================================================================ 1. fused forward
def fused(dev, desc, l, q, t, i, n_neg, pos, w, items, *, want_dq=True, mask=None, mask_shape=None, entry="dq",
          launch=nat._launch):
    """A fused call on NaN-filled outputs: (rc, out [nq, n_neg + 3], d_query, state_ml, state_acc); the partials have
    PAD more floats than `items` need."""
    nq, W = q.shape
    ld = n_neg + 3
    out, dq = nan(nq, ld, dev=dev), nan(nq, W, dev=dev)
    ml, acc = nan(nq * items * 2 + PAD, dev=dev), nan(nq * items * W + PAD, dev=dev)
    head = (ctypes.byref(desc), ctypes.byref(l), q.data_ptr(), nq, t.data_ptr(), i.data_ptr(), n_neg)
    if entry == "partials":
        rc = launch("bess_neg_score_pertriple_fwd_partials", dev, *head, out.data_ptr(), ld, ml.data_ptr(), acc.data_ptr())
    elif mask is None:
        rc = launch("bess_neg_score_pertriple_fwd_dq", dev, *head, pos.data_ptr(), w.data_ptr(), w.numel(), out.data_ptr(),
                    ld, dq.data_ptr() if want_dq else None, ml.data_ptr(), acc.data_ptr())
    else:
        mrows, mcols = mask_shape or mask.shape
        rc = launch("bess_neg_score_pertriple_fwd_dq_masked", dev, *head, pos.data_ptr(), w.data_ptr(), w.numel(),
                    mask.data_ptr(), mrows, mcols, out.data_ptr(), ld, dq.data_ptr() if want_dq else None, ml.data_ptr(),
                    acc.data_ptr())
    torch.cuda.synchronize()
    return rc, out, dq, ml, acc


def all_nan(*tensors):
    return all(bool(torch.isnan(x).all()) for x in tensors)


def fused_against_float64(dev, dtype, W, red, regime, n_neg, one_weight, nq=NQ):
    query, table, idx, pos, w, masks = fused_inputs(dtype, W, regime, n_neg, red, nq)
    w = w[:1] if one_weight else w
    w_rows = w.expand(nq)
    rows = table[idx.long()]
    q, t, i = query.to(dev), table.to(dev), idx.reshape(-1).contiguous().to(dev)
    pos_d, w_d = pos.to(dev), w.contiguous().to(dev)
    desc = make_desc(red, table)
    items = items_of(desc, nq, n_neg)
    assert items == -(-n_neg // 8)
    exact = regime == "exact" and red in ("dot", "l1", "l2", "rotate_l1", "rotate_l2", "complex")
    what0 = f"{tname(dtype)} W={W} {red} {regime} {nq}x{n_neg}"
    _, plain = forward(dev, desc, q, t, i, n_neg, n_neg + 3)
    plain = plain[:, :n_neg].cpu()
    zero = torch.zeros(nq, n_neg)
    s64, s32 = (rule(red, query, rows, zero, dt)[0] for dt in (torch.float64, torch.float32))
    s_seq = sequential_scores(red, query, rows)
    if exact:
        assert torch.equal(plain, s64.float()), f"{what0}: scores differ from the exact value"
    else:
        check("fused", "scores", regime, what0 + " scores", plain, s64, s32)
    for mask in (masks or (None,)):
        kill = kill_of(mask, nq, n_neg) if mask is not None else None
        want_out = plain if kill is None else torch.where(kill, plain + BAD, plain)
        mask_d = mask.to(torch.uint8).contiguous().to(dev) if mask is not None else None
        for variant in VARIANTS:
            what = f"{what0} {variant}" + (f" mask rows {mask.shape[0]}" if mask is not None else "")
            l = loss_desc(variant, n_neg)
            _, dq64 = fused_reference(red, query, rows, pos, w_rows, variant, torch.float64, kill)
            dq32 = fused_restatement(red, query, rows, pos, w_rows, variant, kill, dq64, s_seq)
            _, out, dq, ml, acc = fused(dev, desc, l, q, t, i, n_neg, pos_d, w_d, items, mask=mask_d)
            assert all_nan(out[:, n_neg:], ml[nq * items * 2:], acc[nq * items * W:]), f"{what}: padding written"
            assert torch.equal(out[:, :n_neg].cpu(), want_out), f"{what}: scores differ from the plain forward's"
            check("fused", "d_query", regime, what + " d_query", dq, dq64, dq32)
            # d_query = NULL: the partials are left; combined in float64 on the host they give the same row
            _, out2, dq2, ml2, acc2 = fused(dev, desc, l, q, t, i, n_neg, pos_d, w_d, items, want_dq=False, mask=mask_d)
            assert all_nan(dq2, ml2[nq * items * 2:], acc2[nq * items * W:]) and torch.equal(out2[:, :n_neg], out[:, :n_neg])
            host = combine64(ml2[: nq * items * 2].view(nq, items, 2).cpu(), acc2[: nq * items * W].view(nq, items, W).cpu(),
                             pos, w_rows, variant)
            check("fused", "d_query (partials)", regime, what + " d_query from the partials", host, dq64, dq32)
            if mask is not None and mask.shape[0] == nq:  # the query whose mask row is all zero
                assert bool((out[2, n_neg - MASK_COLS: n_neg] < -40000).all())


@gpu
@pytest.mark.parametrize("case", list(enumerate(FUSED_CASES)), ids=lambda c: f"{tname(c[1][0])}-{c[1][1]}-{c[1][2]}")
def test_fused_forward_equals_float64(dev, case):
    n, (dtype, W, red) = case
    for regime in ("normal", "ties", "saturated", "exact", "masked"):
        for n_neg in ((N_NEG, N_ONE_ITEM) if regime in ("normal", "exact") else (N_NEG,)):
            fused_against_float64(dev, dtype, W, red, regime, n_neg, one_weight=n % 2 == 0)


@gpu
@pytest.mark.parametrize("case", [(F32, 60, "l1"), (F16, 264, "dot"), (F32, 60, "l2")],
                         ids=lambda c: f"{tname(c[0])}-{c[1]}-{c[2]}")
def test_fused_forward_of_more_than_64_items(dev, case):
    """5 x 1028 negatives: 129 items of 8, so the strided item loops of `combine_dq_row` run three rounds, the last
    one with one item."""
    dtype, W, red = case
    assert items_of(make_desc(red, torch.empty((0, W), dtype=dtype)), NQ, MANY) == 129
    fused_against_float64(dev, dtype, W, red, "normal", MANY, one_weight=False)


@gpu
def test_fused_forward_refusals(dev):
    """BESS_EUNSUPPORTED, and all four NaN-filled outputs untouched: rows wider than a group's registers, the margin loss
    through `_fwd_partials`, a mask with more columns than scores, mask rows that are neither 1 nor n_query."""
    for (dtype, W) in WINDOW_WIDTHS:
        query, table, idx, _ = inputs(dtype, W, "normal", N_NEG)
        q, t, i = query.to(dev), table.to(dev), idx.reshape(-1).contiguous().to(dev)
        pos, w = torch.zeros(NQ, device=dev), torch.ones(1, device=dev)
        for red in ("dot", "l1"):
            desc = make_desc(red, table)
            for entry, variant in (("dq", "logsigmoid_adv"), ("dq", "margin"), ("partials", "ssce")):
                rc, *outs = fused(dev, desc, loss_desc(variant, N_NEG), q, t, i, N_NEG, pos, w, 5, entry=entry, launch=status)
                assert rc == EUNSUPPORTED and all_nan(*outs), (tname(dtype), W, red, entry)
    query, table, idx, _ = inputs(F32, 60, "normal", N_NEG)
    q, t, i = query.to(dev), table.to(dev), idx.reshape(-1).contiguous().to(dev)
    pos, w = torch.zeros(NQ, device=dev), torch.ones(1, device=dev)
    desc = make_desc("l1", table)
    for variant in ("margin", "margin_adv"):
        rc, *outs = fused(dev, desc, loss_desc(variant, N_NEG), q, t, i, N_NEG, pos, w, 5, entry="partials", launch=status)
        assert rc == EUNSUPPORTED and all_nan(*outs), variant
    mask = torch.ones(NQ, N_NEG + 3, dtype=torch.uint8, device=dev)
    for shape in ((1, N_NEG + 1), (NQ, N_NEG + 3), (2, MASK_COLS), (NQ - 1, MASK_COLS), (NQ + 1, MASK_COLS)):
        rc, *outs = fused(dev, desc, loss_desc("logsigmoid", N_NEG), q, t, i, N_NEG, pos, w, 5, mask=mask, mask_shape=shape,
                          launch=status)
        assert rc == EUNSUPPORTED and all_nan(*outs), shape
    # (the same mask in a shape the pass takes is applied)
    rc, out, *_ = fused(dev, desc, loss_desc("logsigmoid", N_NEG), q, t, i, N_NEG, pos, w, 5, mask=mask,
                        mask_shape=(1, MASK_COLS), launch=status)
    assert rc == 0 and not bool(torch.isnan(out[:, :N_NEG]).any())


@gpu
@pytest.mark.parametrize("case", list(enumerate(PARTIAL_WIDTHS)), ids=lambda c: f"{tname(c[1][0])}-{c[1][1]}")
def test_partials_of_two_shards_sum_to_the_float64_gradient(dev, case):
    """Each query's 37 negatives split 23 / 14 over two `_fwd_partials` calls, `norm` from the loss kernel over the
    concatenated scores (anchored in section 13): the two `bess_combine_dq_partials` rows add up to the float64
    d_query.  A norm[:, 1] of 0, +inf or NaN gives a row of zeros."""
    n, (dtype, W) = case
    red = list(REDS)[n % 4]
    query, table, idx, pos, w, _ = fused_inputs(dtype, W, "normal", N_NEG, red)
    rows = table[idx.long()]
    q, t, pos_d, w_d = query.to(dev), table.to(dev), pos.to(dev), w.to(dev)
    desc = make_desc(red, table)
    for variant in ("logsigmoid_adv", "logsigmoid", "ssce"):
        what = f"{tname(dtype)} W={W} {red} {variant} two shards"
        l = loss_desc(variant, N_NEG)
        _, dq64 = fused_reference(red, query, rows, pos, w, variant, torch.float64)
        _, dq32 = fused_reference(red, query, rows, pos, w, variant, torch.float32)
        shards = []
        for lo, hi in ((0, 23), (23, N_NEG)):
            i = idx[:, lo:hi].reshape(-1).contiguous().to(dev)
            items = items_of(desc, NQ, hi - lo)
            rc, out, dq, ml, acc = fused(dev, desc, l, q, t, i, hi - lo, None, None, items, entry="partials")
            assert all_nan(dq, out[:, hi - lo:], ml[NQ * items * 2:], acc[NQ * items * W:])
            shards.append((out[:, : hi - lo], ml[: NQ * items * 2].view(NQ, items, 2).contiguous(),
                           acc[: NQ * items * W].view(NQ, items, W).contiguous()))
        sc = torch.cat([shards[0][0], shards[1][0]], dim=1).contiguous()
        _, plain = forward(dev, desc, q, t, idx.reshape(-1).contiguous().to(dev), N_NEG, N_NEG)
        assert torch.equal(sc, plain)
        norm = nat.loss_fwd_bwd(l, pos_d, sc, w_d, True, want_norm=True)[3]
        got = sum(nat.combine_dq_partials((ml, acc), norm) for _, ml, acc in shards)
        check("fused", "d_query (two shards)", "normal", what, got, dq64, dq32)
        host = sum(combine64(ml.cpu(), acc.cpu(), pos, w, variant, norm.cpu()) for _, ml, acc in shards)
        check("fused", "d_query (two shards)", "normal", what + " (host)", host, dq64, dq32)
        bad = norm.clone()
        bad[0, 1], bad[1, 1], bad[2, 1] = 0.0, float("inf"), float("nan")
        got = nat.combine_dq_partials(shards[0][1:], bad)
        assert bool((got[:3] == 0).all()) and torch.equal(got[3:], nat.combine_dq_partials(shards[0][1:], norm)[3:]), what


# ============================================================================================ 2. bess_pertriple_tail
@functools.lru_cache(maxsize=4)
def tail_inputs(name, p, dtype, S, n_neg, W, zero):
    gen = torch.Generator().manual_seed(S + 3 * n_neg + W + p + (5 if dtype == F16 else 0))
    M, R = 61, 5
    Wr = W // 2 if name == "RotatE" else W
    ent = (torch.randn(M, W, generator=gen) * 0.3).to(dtype)
    rel = (torch.randn(R, Wr, generator=gen) * 0.5).to(dtype)
    hidx = torch.randint(2, M, (S,), generator=gen).to(torch.int32)
    tidx = torch.randint(2, M, (S,), generator=gen).to(torch.int32)
    rid = torch.randint(0, R - 1, (S,), generator=gen).to(torch.int32)
    nidx = torch.randint(0, M, (S, n_neg), generator=gen).to(torch.int32)
    if zero:  # triple 0: query of the head == the tail row exactly (rows 0, 1 and the last relation are its own)
        hidx[0], tidx[0], rid[0] = 0, 1, R - 1
        if name == "TransE":
            ent[0] = ((ent[0].float() * 64).round() / 64).to(dtype)
            rel[R - 1] = ((rel[R - 1].float() * 64).round() / 64).to(dtype)
            ent[1] = (ent[0].float() + rel[R - 1].float()).to(dtype)
            assert torch.equal(ent[1].double(), ent[0].double() + rel[R - 1].double())
        else:
            rel[R - 1] = 0
            ent[1] = ent[0]
    w = torch.rand(S, generator=gen) + 0.5
    return ent, rel, hidx, tidx, rid, nidx, w


def check_tol(part, quantity, regime, what, got, ref64, ref32, tol):
    """`close64` of test_mask_loss_rank_kernels.py with the fp32 restatement's error of this case."""
    e32 = error_in_tolerances(ref32.detach(), ref64.detach(), **tol)
    rec = MEASURED.setdefault((part, quantity, regime), [0.0, 0.0])
    rec[0], rec[1] = max(rec[0], e32), max(rec[1], error_in_tolerances(got.detach().cpu(), ref64.detach(), **tol))
    close64(what, got.detach(), ref64.detach(), e32, **tol)


def launch_tail(dev, desc, l, side, E, hi, ti, R, ri, ml, acc, items, pos, neg, n_neg, ld_neg, w, d_rel, *, weight_len=None,
                launch=nat._launch):
    """bess_pertriple_tail on NaN-filled outputs and a zeroed counter; ld_dneg = n_neg + 4."""
    S, W = hi.numel(), desc.width
    o = dict(row_loss=nan(S, dev=dev), loss=nan(1, dev=dev), d_pos=nan(S, dev=dev), d_neg=nan(S, n_neg + 4, dev=dev),
             d_query=nan(S, W, dev=dev), d_head=nan(S, W, dev=dev), d_tail=nan(S, W, dev=dev))
    counter = torch.zeros(nat.TICKET_INTS, dtype=torch.int32, device=dev)
    rc = launch("bess_pertriple_tail", dev, ctypes.byref(desc), ctypes.byref(l), side, E.data_ptr(), hi.data_ptr(),
                E.data_ptr(), ti.data_ptr(), R.data_ptr(), ri.data_ptr(), S, ml.data_ptr(), acc.data_ptr(), items,
                pos.data_ptr(), neg.data_ptr(), n_neg, ld_neg, w.data_ptr(), w.numel() if weight_len is None else weight_len,
                o["row_loss"].data_ptr(), o["loss"].data_ptr(), o["d_pos"].data_ptr(), o["d_neg"].data_ptr(), n_neg + 4,
                o["d_query"].data_ptr(), o["d_head"].data_ptr(), o["d_tail"].data_ptr(), d_rel.data_ptr(), counter.data_ptr())
    torch.cuda.synchronize()
    return rc, o, counter


def check_tail_outputs(dev, what, o, counter, d_rel, d_rel0, r64, r32, n_neg):
    regime = "tail"
    check_tol("tail", "loss", regime, what + " loss", o["loss"].reshape(()), r64["loss"], r32["loss"], LOSS_TOL)
    row_sum = o["row_loss"].double().sum().cpu()
    assert abs(float(row_sum) - float(o["loss"])) <= LOSS_TOL["atol"] + LOSS_TOL["rtol"] * abs(float(row_sum)), what
    check_tol("tail", "d_pos", regime, what + " d_pos", o["d_pos"], r64["d_pos"], r32["d_pos"], GRAD_TOL)
    assert all_nan(o["d_neg"][:, n_neg:]), f"{what}: padding of d_neg written"
    check_tol("tail", "d_neg", regime, what + " d_neg", o["d_neg"][:, :n_neg], r64["d_neg"], r32["d_neg"], GRAD_TOL)
    for name in ("d_query", "d_head", "d_tail"):
        check("tail", name, regime, f"{what} {name}", o[name], r64[name], r32[name])
    check("tail", "d_rel_table", regime, what + " d_rel_table", d_rel, d_rel0.double() + r64["d_rel"],
          d_rel0 + r32["d_rel"])
    assert int(counter.abs().sum()) == 0, f"{what}: the counter is not left zero"


@gpu
@pytest.mark.parametrize("case", TAIL_CASES, ids=lambda c: f"{c[0]}{c[1]}-{tname(c[2])}-{c[3]}x{c[4]}x{c[5]}-{c[6]}-{c[7]}")
def test_pertriple_tail_equals_the_float64_chain(dev, case):
    name, p, dtype, S, n_neg, W, side, variant, zero = case
    ent, rel, hidx, tidx, rid, nidx, w = tail_inputs(name, p, dtype, S, n_neg, W, zero)
    if (n_neg // 4 + W) % 2 == 0:
        w = w[:1]
    w_rows = w.expand(S)
    r64, r32 = (tail_chain(name, p, side, ent, rel, hidx, tidx, rid, nidx, w_rows, variant, ft)
                for ft in (torch.float64, torch.float32))
    what = f"{name} p={p} {tname(dtype)} {S}x{n_neg}x{W} {side} {variant}"
    if zero:
        assert float(r64["pos"][0]) == 0.0 and float(r64["pos"][1:].abs().min()) > 0
    desc = nat.make_desc(SCORER_CODE[name], max(p, 1), ent, rel.shape[1])
    E, R, hi, ti, ri = ent.to(dev), rel.to(dev), hidx.to(dev), tidx.to(dev), rid.to(dev)
    ni, w_d = nidx.reshape(-1).contiguous().to(dev), w.contiguous().to(dev)
    l = loss_desc(variant, n_neg)
    q, pos = nat.query_triple_fwd(desc, SIDES[side], nat.RowSource(E, hi), nat.RowSource(E, ti), R, ri)
    out, (ml, acc) = nat.neg_score_pertriple_fwd_dq(desc, l, q, nat.RowSource(E, ni), n_neg, pos, w_d, defer=True)
    check("tail", "scores", "tail", what + " pos", pos, r64["pos"], r32["pos"])
    check("tail", "scores", "tail", what + " neg", out, r64["neg"], r32["neg"])
    gen = torch.Generator().manual_seed(W)
    d_rel0 = torch.randn(rel.shape, generator=gen) * 0.1
    d_rel = d_rel0.to(dev)
    items = int(ml.shape[1])
    args = (dev, desc, l, SIDES[side], E, hi, ti, R, ri, ml, acc, items, pos, out, n_neg, n_neg, w_d)
    (rc, o, counter), names = launched(lambda: launch_tail(*args, d_rel))
    (dt, code, ch), nw = tail_class(name, dtype, S, n_neg, W)
    assert kernel_launched(names, "k_pertriple_tail", dt, code, ch), names
    check_tail_outputs(dev, what, o, counter, d_rel.cpu(), d_rel0, r64, r32, n_neg)
    _, o2, counter2 = launch_tail(*args, d_rel0.to(dev))
    assert torch.equal(o2["loss"], o["loss"]) and torch.equal(o2["d_head"], o["d_head"]) and int(counter2.abs().sum()) == 0


@gpu
@pytest.mark.parametrize("name,p,dtype,variant", [("TransE", 1, F32, "ssce"), ("ComplEx", 0, F16, "logsigmoid_adv"),
                                                  ("RotatE", 2, F16, "margin"), ("DistMult", 0, F32, "logsigmoid")])
def test_pertriple_tail_on_rows_of_4096_from_hand_made_partials(dev, name, p, dtype, variant):
    """W = 4096: two waves per workgroup; the fused forward refuses such rows, the tail does not.  Three items of random
    m_i, positive l_i and random acc_i, one of them empty (m_i = -inf), against `combine64` and the float64 chain."""
    S, n_neg, W, items, side = 9, 8, 4096, 3, "t"
    ent, rel, hidx, tidx, rid, nidx, w = tail_inputs(name, p, dtype, S, n_neg, W, False)
    gen = torch.Generator().manual_seed(p + len(name))
    ml = torch.stack([torch.randn(S, items, generator=gen), torch.rand(S, items, generator=gen) + 0.1], dim=2)
    acc = torch.randn(S, items, W, generator=gen) * 0.1
    ml[torch.arange(S), torch.arange(S) % items, 0] = -float("inf")
    neg = torch.randn(S, n_neg, generator=gen)
    desc = nat.make_desc(SCORER_CODE[name], max(p, 1), ent, rel.shape[1])
    E, R, hi, ti, ri = ent.to(dev), rel.to(dev), hidx.to(dev), tidx.to(dev), rid.to(dev)
    q, pos = nat.query_triple_fwd(desc, SIDES[side], nat.RowSource(E, hi), nat.RowSource(E, ti), R, ri)
    pos_c = pos.cpu()
    d_rel0 = torch.randn(rel.shape, generator=gen) * 0.1
    refs = []
    for ft in (torch.float64, torch.float32):
        loss, d_pos, d_neg = loss_chain(variant, pos_c, neg, w, ft)
        dq = combine64(ml, acc, pos_c, w, variant).to(ft)
        dh, dt, dr = triple_grads(name, p, side, ent, rel, hidx, tidx, rid, d_pos, dq, ft)
        refs.append(dict(loss=loss, d_pos=d_pos, d_neg=d_neg, d_query=dq, d_head=dh, d_tail=dt, d_rel=dr))
    d_rel = d_rel0.to(dev)
    rc, o, counter = launch_tail(dev, desc, loss_desc(variant, n_neg), SIDES[side], E, hi, ti, R, ri, ml.to(dev), acc.to(dev),
                                 items, pos, neg.to(dev), n_neg, n_neg, w.to(dev), d_rel)
    assert tail_waves(S, W) == 2
    check_tail_outputs(dev, f"{name} p={p} {tname(dtype)} W=4096 {variant}", o, counter, d_rel.cpu(), d_rel0, *refs, n_neg)
    fused_desc = nat.make_desc(SCORER_CODE[name], 1, ent, rel.shape[1])
    rc, *outs = fused(dev, fused_desc, loss_desc(variant, n_neg), q, E, nidx.reshape(-1).contiguous().to(dev), n_neg, pos,
                      w.to(dev), 1, launch=status)
    assert rc == EUNSUPPORTED and all_nan(*outs)


@gpu
def test_pertriple_tail_refusals(dev):
    """n_neg = 6 (not a multiple of 4) and 3076 (more than 3072): BESS_EUNSUPPORTED; a leading dimension that is no
    multiple of 4 and weight_len = 2: BESS_EINVAL.  Every output stays NaN, d_rel_table and the counter as they were."""
    name, p, dtype, S, W = "TransE", 1, F32, 9, 6
    ent, rel, hidx, tidx, rid, _, w = tail_inputs(name, p, dtype, S, 8, W, False)
    desc = nat.make_desc(SCORER_CODE[name], 1, ent, W)
    E, R, hi, ti, ri = ent.to(dev), rel.to(dev), hidx.to(dev), tidx.to(dev), rid.to(dev)
    pos, w_d = torch.zeros(S, device=dev), w.to(dev)
    ml, acc = torch.ones(S, 1, 2, device=dev), torch.ones(S, 1, W, device=dev)
    for n_neg, ld_neg, weight_len, want in ((6, 8, S, EUNSUPPORTED), (3076, 3076, S, EUNSUPPORTED), (8, 9, S, EINVAL),
                                            (8, 8, 2, EINVAL), (8, 8, S, 0)):
        neg = torch.zeros(S, ld_neg, device=dev)
        d_rel = torch.full(rel.shape, 0.25, device=dev)
        rc, o, counter = launch_tail(dev, desc, loss_desc("logsigmoid", 8), nat.CORRUPT_TAIL, E, hi, ti, R, ri, ml, acc, 1,
                                     pos, neg, n_neg, ld_neg, w_d, d_rel, weight_len=weight_len, launch=status)
        assert rc == want, (n_neg, ld_neg, weight_len, rc)
        assert int(counter.abs().sum()) == 0
        if want:
            assert all_nan(*o.values()) and bool((d_rel == 0.25).all()), (n_neg, ld_neg, weight_len)
        else:
            assert bool(torch.isfinite(o["loss"]).all()) and not bool((d_rel == 0.25).all())


# ============================================================================================ 3. query_triple_bwd_parts
@functools.lru_cache(maxsize=4)
def parts_inputs(name, dtype, W):
    """S = 9 triples and N = 21 candidates over M = 50 rows with overlapping id lists; slabs with a fifth exact zeros."""
    gen = torch.Generator().manual_seed(W + len(name) + (5 if dtype == F16 else 0))
    S, N, M, R = 9, 21, 50, 4
    Wr = W // 2 if name == "RotatE" else W
    ent = (torch.randn(M, W, generator=gen) * 0.5).to(dtype)
    rel = (torch.randn(R, Wr, generator=gen) * 0.5).to(dtype)
    hidx = torch.randint(0, M, (S,), generator=gen).to(torch.int32)
    tidx = torch.randint(0, M, (S,), generator=gen).to(torch.int32)
    tidx[3] = hidx[5]                       # a head that is a tail
    rid = torch.tensor([0, 1, 2, 3, 0, 1, 2, 3, 1], dtype=torch.int32)
    nidx = torch.randint(0, M, (N,), generator=gen).to(torch.int32)
    nidx[4] = hidx[0]                       # a candidate that is a head
    nidx[7], nidx[11], nidx[20] = 33, 33, 33  # a candidate named three times

    def slabs(n, rows):
        x = torch.randn(n, rows, W, generator=gen) * 0.1
        return torch.where(torch.rand(n, rows, W, generator=gen) < 0.2, torch.zeros(()), x)

    dq = {n: slabs(n, S) for n in (1, 3)}
    de = {n: slabs(n, N) for n in (1, 2)}
    d_out = torch.randn(S, generator=gen)
    acc0 = torch.randn(M, W, generator=gen) * 0.1
    d_rel0 = torch.randn(R, Wr, generator=gen) * 0.1
    return ent, rel, hidx, tidx, rid, nidx, dq, de, d_out, acc0, d_rel0


def launch_parts(dev, desc, side, E, hi, ti, R, ri, d_out, dq, de, ni, acc, d_rel, launch=nat._launch):
    rc = launch("bess_query_triple_bwd_parts", dev, ctypes.byref(desc), side, E.data_ptr(),
                hi.data_ptr() if hi is not None else None, E.data_ptr(), ti.data_ptr(), R.data_ptr(), ri.data_ptr(),
                ri.numel(), d_out.data_ptr(), dq.data_ptr(), dq.shape[0], de.data_ptr(), de.shape[0], de.shape[1],
                ni.data_ptr(), acc.data_ptr(), acc.data_ptr(), acc.data_ptr(), d_rel.data_ptr())
    torch.cuda.synchronize()
    return rc


@gpu
@pytest.mark.parametrize("dtype", [F32, F16], ids=tname)
@pytest.mark.parametrize("name", list(SCORER_CODE))
def test_query_triple_bwd_parts_equals_float64(dev, name, dtype):
    """Accumulators (one matrix for heads, tails and candidates, as a step has it) and d_rel_table, non-zero on entry,
    against zeros(M, W, float64).index_add_ of the float64 `query_triple_bwd` rows and of the summed candidate slabs."""
    for W in PARTS_W:
        p = (1 if W in (6, 260) else 2) if name in ("TransE", "RotatE") else 0
        ent, rel, hidx, tidx, rid, nidx, dqs, des, d_out, acc0, d_rel0 = parts_inputs(name, dtype, W)
        desc = nat.make_desc(SCORER_CODE[name], max(p, 1), ent, rel.shape[1])
        E, R, hi, ti, ri, ni = (x.to(dev) for x in (ent, rel, hidx, tidx, rid, nidx))
        go = d_out.to(dev)
        for side, n_dq, n_de in (("t", 1, 2), ("h", 3, 1), ("t", 3, 2), ("h", 1, 1)):
            what = f"{name} p={p} {tname(dtype)} W={W} {side} parts {n_dq}/{n_de}"
            dq, de = dqs[n_dq], des[n_de]
            want = []
            for ft in (torch.float64, torch.float32):
                dh, dt, dr = triple_grads(name, p, side, ent, rel, hidx, tidx, rid, d_out, dq.to(ft).sum(0), ft)
                acc = acc0.to(ft).clone()
                acc.index_add_(0, hidx.long(), dh).index_add_(0, tidx.long(), dt).index_add_(0, nidx.long(), de.to(ft).sum(0))
                want.append((acc, d_rel0.to(ft) + dr))
            acc, d_rel = acc0.to(dev), d_rel0.to(dev)
            run = lambda: launch_parts(dev, desc, SIDES[side], E, hi, ti, R, ri, go, dq.to(dev), de.to(dev), ni, acc, d_rel)
            _, names = launched(run)
            assert kernel_launched(names, "k_query_triple_bwd_parts", dtype, SCORER_CODE[name]), names
            check("parts", "accumulators", "parts", what + " accumulators", acc, want[0][0], want[1][0])
            check("parts", "d_rel_table", "parts", what + " d_rel_table", d_rel, want[0][1], want[1][1])


@gpu
def test_query_triple_bwd_parts_refusals(dev):
    """Rows of 4097 scalars and direct rows (head_idx = NULL): refused, the accumulators untouched."""
    for name, W in (("TransE", 4097), ("DistMult", 4097), ("TransE", 128)):
        gen = torch.Generator().manual_seed(W)
        S, N, M = 9, 21, 50
        ent = torch.randn(M, W, generator=gen)
        desc = nat.make_desc(SCORER_CODE[name], 1, ent, W)
        E, R = ent.to(dev), torch.randn(4, W, generator=gen).to(dev)
        hi = torch.arange(S, dtype=torch.int32, device=dev)
        ri = torch.zeros(S, dtype=torch.int32, device=dev)
        ni = torch.arange(N, dtype=torch.int32, device=dev)
        acc0, d_rel0 = torch.randn(M, W, generator=gen), torch.randn(4, W, generator=gen)
        acc, d_rel = acc0.to(dev), d_rel0.to(dev)
        rc = launch_parts(dev, desc, nat.CORRUPT_TAIL, E, hi if W == 4097 else None, hi, R, ri, torch.ones(S, device=dev),
                          torch.ones(1, S, W, device=dev), torch.ones(1, N, W, device=dev), ni, acc, d_rel, launch=status)
        assert rc == EINVAL and torch.equal(acc.cpu(), acc0) and torch.equal(d_rel.cpu(), d_rel0), (name, W)


# ============================================================================================ 4. query_triple_fwd_jobs
SENTINEL = 0x5A5A5A5A
BIG_JOB = 8 * 256 * 256 + 5  # words: more than 256 job workgroups of 8 words per thread take in one round


@gpu
@pytest.mark.parametrize("dtype", [F32, F16], ids=tname)
@pytest.mark.parametrize("name,p", [("TransE", 1), ("RotatE", 2), ("DistMult", 0), ("ComplEx", 0)])
def test_query_triple_fwd_jobs_equals_the_plain_launch_and_does_its_jobs(dev, name, p, dtype):
    gen = torch.Generator().manual_seed(3)
    lengths = [100, 33, 17, BIG_JOB, 1]
    gap = 3
    starts = np.cumsum([gap] + [n + gap for n in lengths[:-1]])
    total = int(starts[-1]) + lengths[-1] + gap
    src = torch.randint(-2**31, 2**31 - 1, (100,), generator=gen, dtype=torch.int64).to(torch.int32).to(dev)
    one = torch.tensor([41], dtype=torch.int32, device=dev)
    values = [(src, 0), (None, 0), (None, 0xFFFFFFFF), (None, 0x01020304), (one, 1)]
    for d in JOBS_D:
        ent, rel, hidx, tidx, rid, *_ = prepare_inputs(name, p, dtype, d)
        r64, r32 = (prepare_references(name, p, dtype, d, ft) for ft in (torch.float64, torch.float32))
        desc = nat.make_desc(SCORER_CODE[name], max(p, 1), ent, rel.shape[1])
        E, R, hi, ti, ri = ent.to(dev), rel.to(dev), hidx.to(dev), tidx.to(dev), rid.to(dev)
        head, tail = nat.RowSource(E, hi), nat.RowSource(E, ti)
        for side, code in SIDES.items():
            what = f"{name} p={p} {tname(dtype)} d={d} {side} jobs"
            buf = torch.full((total,), SENTINEL, dtype=torch.int32, device=dev)
            jobs = [(buf[s: s + n], v[0], v[1]) for s, n, v in zip(starts, lengths, values)]
            (q, sc), names = launched(lambda: nat.query_triple_fwd(desc, code, head, tail, R, ri, jobs=jobs))
            assert kernel_launched(names, "k_query_triple_fwd_jobs", dtype, SCORER_CODE[name]), names
            q0, sc0 = nat.query_triple_fwd(desc, code, head, tail, R, ri)
            assert torch.equal(q, q0) and torch.equal(sc, sc0), what
            check("jobs", "query", "smooth", what + " query", q, r64["query", side], r32["query", side])
            check("jobs", "score", "smooth", what + " score", sc, r64["score"], r32["score"])
            want = torch.full((total,), SENTINEL, dtype=torch.int32)
            for s, n, fill in zip(starts, lengths, (src.cpu(), 0, -1, 0x01020304, 42)):
                want[s: s + n] = fill
            assert torch.equal(buf.cpu(), want), f"{what}: a job's words or a sentinel next to them differ"
    # jobs only
    buf = torch.full((total,), SENTINEL, dtype=torch.int32, device=dev)
    jobs = [(buf[s: s + n], v[0], v[1]) for s, n, v in zip(starts, lengths, values)]
    dst, srcs, val, words = nat._job_arrays(jobs, "test")
    nat._launch("bess_query_triple_fwd_jobs", dev, ctypes.byref(desc), nat.CORRUPT_TAIL, E.data_ptr(), None, E.data_ptr(), None,
                R.data_ptr(), ri.data_ptr(), 0, None, None, len(jobs), dst, srcs, val, words)
    torch.cuda.synchronize()
    assert torch.equal(buf.cpu(), want)


# ============================================================================================ 5. affine table form, p = 2
@gpu
@pytest.mark.parametrize("name,p,dtype,indexed,d,n_part", AFFINE_P2, ids=lambda x: tname(x) if isinstance(x, torch.dtype) else str(x))
def test_affine_table_form_at_p2_launches_its_classes_and_equals_float64(dev, name, p, dtype, indexed, d, n_part):
    """The cases test_fused_ranks_scorers.py gained: the count and the pair form of `k_aff_shared_fwd` on a raw table at
    p = 2 are launched (by kernel name), and the stored score matrix of 64 queries x 300 candidates == `oracle.kge`."""
    from test_fused_ranks_scorers import CASES
    from test_hip_parity import make_scorer, widths

    assert (name, p, dtype, indexed, d) in CASES
    gen = torch.Generator().manual_seed(d + n_part)
    nq, n_cand, n_ent, n_rel = 64, 300, 350, 11
    ew, rw = widths(name, d)
    ent = torch.randn(1, n_ent, ew, generator=gen) * 0.3
    rel = torch.randn(n_rel, rw, generator=gen) * 0.3
    fn = make_scorer(name, p, True, n_rel, d, ent, rel, dev, dtype=dtype)
    desc, table = fn.kernel_desc(), fn.entity_embedding.data[0]
    known = torch.randint(0, n_ent, (nq,), generator=gen).to(torch.int32)
    rid = torch.randint(0, n_rel, (nq,), generator=gen).to(torch.int32)
    q = fn.query_fwd(nat.CORRUPT_TAIL, nat.RowSource(table, known.to(dev)), rid.to(dev))[0]
    idx = torch.randperm(n_ent, generator=gen)[:n_cand].to(torch.int32)
    src = nat.RowSource(table, idx.to(dev)) if indexed else nat.RowSource(table[:n_cand])
    sc = nat.neg_score_shared_fwd(desc, q, src)
    tab, rl = table.cpu(), fn.relation_embedding.data.cpu()
    cand = tab[idx.long()] if indexed else tab[:n_cand]
    want = [kge.score_candidates(name, p, True, "t", tab[known.long()].to(ft), rl.to(ft), rid, cand.to(ft)[None])
            for ft in (torch.float64, torch.float32)]
    check("affine", "scores", "p2", f"{name} p={p} {tname(dtype)} score matrix", sc, *want)
    thr = sc[:, 17].contiguous()
    excl = torch.full((nq,), -1, dtype=torch.int32, device=dev)
    counts, names = launched(lambda: nat.neg_score_shared_counts(desc, q, src, thr, excl))
    assert kernel_launched(names, "k_aff_shared_fwd", n_part, 2, dtype, True, True, False), names
    assert torch.equal(counts[:, 0].long(), (sc > thr[:, None]).sum(-1))
    cols = torch.randint(0, n_cand, (nq,), generator=gen).to(torch.int32).to(dev)
    rows = idx.to(dev)[cols.long()] if indexed else cols
    pairs, names = launched(lambda: nat.neg_score_shared_pairs(desc, q, nat.RowSource(table, rows), nq, n_cand))
    assert kernel_launched(names, "k_aff_shared_fwd", n_part, 2, dtype, True, False, True), names
    assert torch.equal(pairs, sc[torch.arange(nq, device=dev), cols.long()])
