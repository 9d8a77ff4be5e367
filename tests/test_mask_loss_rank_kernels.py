"""K7 (`bess_mask_scores`), K8 (`bess_loss_fwd_bwd*`, loss_rows.h) and the two rank kernels of csrc/loss.hip against
plain references - other tests use these kernels AS their reference, so they are anchored here:

  0. the references themselves, on the CPU (no device): the K7 rule of include/besskge_hip.h restated element by
     element == `oracle.kge.apply_masks`; the float64 loss oracle == the fp32 one; the rank restatements == brute force;
  1. `mask_scores` == the rule, bit for bit;
  2. loss, d_pos, d_neg and row_norm == the float64 oracle, over every row class `loss_chunks` tells apart, both
     weight forms, four memory layouts and four value regimes;
  3. the one-launch form's grid sizes and ticket counters;
  4. the rank kernels == integer counts.

Tolerances of 2 and 3 are `test_loss_vs_oracle`'s.  Where the fp32 CPU oracle itself misses one of them against
float64 in a value regime, the quantity is ill-conditioned in fp32 there and the regime's bound becomes 4 x the fp32
oracle's largest error (`oracle_error`, `close64`; what it measures: DESIGN.md, "Float64 anchors of the mask, loss
and rank kernels")."""

import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

from oracle import kge

from test_rank_counting_host import reference_ranks

BAD = kge.BAD_NEGATIVE_SCORE
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda", 0)


# ================================================================================================ K7: the rule
def rule_kill(S, N, diag_step, ht, ppp, mask):
    """include/besskge_hip.h, K7, element by element: kill[s, j] of an [S, N] score matrix."""
    s = torch.arange(S)[:, None]
    j = torch.arange(N)[None, :]
    blk = s // ppp if ppp > 0 else torch.zeros_like(s)
    p = s - blk * ppp if ppp > 0 else torch.zeros_like(s)
    cut = ppp // 2
    kill = torch.zeros(S, N, dtype=torch.bool)
    if diag_step > 0:
        qpos = blk * cut + p % cut if ht else s
        kill = j == diag_step * qpos
    if mask is not None:
        rows, cols = mask.shape
        mrow = torch.zeros_like(s) if rows == 1 else ((p >= cut).long() if rows == 2 else s)
        mj = j - (N - cols)
        inside = (mj >= 0).expand(S, N)
        real = mask[mrow.expand(S, N), mj.clamp(min=0).expand(S, N)]
        kill = torch.where(inside, ~real, kill.expand(S, N))  # the mask overrides the diagonal on its columns
    return kill.expand(S, N).clone()


def rule_mask(scores, diag_step, ht, ppp, mask):
    kill = rule_kill(scores.shape[0], scores.shape[1], diag_step, ht, ppp, mask)
    return torch.where(kill, scores + torch.tensor(BAD, dtype=scores.dtype), scores), kill


def kill_args(spec, n, ppp, K, mask2d):
    """(diag_step, ht, ppp, mask) of a micro-batch, as `BessKGE._kill_spec` forms them; None: K7 does not run."""
    flat_ht = spec.flat and spec.scheme == "ht"
    if spec.augment:
        return (1 if spec.flat else 1 + n * K), spec.scheme == "ht", ppp, mask2d
    if mask2d is not None:
        return 0, False, ppp if flat_ht else 0, mask2d
    return None


def integer_scores(S, N, gen):
    """Small integers + 0.5: adding -50000 is exact, and an element killed twice or not at all is visible."""
    return torch.randint(-8, 9, (S, N), generator=gen).float() + 0.5


# flat 'ht' negatives come with a 2-row mask (heads, tails) and no other; every other format with 1 or S rows
SPEC_CASES = [(flat, scheme, augment, rows)
              for flat, scheme, augment in itertools.product([False, True], ["h", "t", "ht"], [False, True])
              for rows in ([None, 2] if flat and scheme == "ht" else [None, 1, "S"])]


@pytest.mark.parametrize("flat,scheme,augment,mask_rows", SPEC_CASES)
def test_mask_rule_equals_the_oracle(flat, scheme, augment, mask_rows):
    n, ppp, K, L = 4, 6, 3, 7
    S, N = n * ppp, 37
    gen = torch.Generator().manual_seed(11)
    scores = integer_scores(S, N, gen)
    negative_mask = None
    if mask_rows is not None:
        negative_mask = torch.rand(S if mask_rows == "S" else mask_rows, n, L, generator=gen) > 0.4
    spec = kge.StepSpec("TransE", 1, True, scheme, flat, augment=augment)
    want = kge.apply_masks(spec, scores.clone(), n, ppp, K, negative_mask)
    args = kill_args(spec, n, ppp, K, None if negative_mask is None else negative_mask.reshape(negative_mask.shape[0], -1))
    got = scores if args is None else rule_mask(scores, *args)[0]
    assert torch.equal(got, want)
    if augment or negative_mask is not None:
        assert not torch.equal(got, scores)


# ================================================================================================ K8: references
MARGIN, BETA, LOSS_SCALE, N_ENTITY = 2.5, float(np.float32(0.3)), 1.5, 5000
VARIANTS = {  # name -> (kind, adversarial)
    "logsigmoid_adv": ("logsigmoid", True),
    "logsigmoid": ("logsigmoid", False),
    "margin_adv": ("margin", True),
    "margin": ("margin", False),
    "ssce": ("ssce", False),
}
ROW_LENGTHS = [5, 1024, 1028, 3072, 3076, 6144, 6148]  # CH = 0, 4, 12, 12, 24, 24, streamed (-1)
REGIMES = ["normal", "saturated", "killed", "ties"]
S_ROWS = 6  # two workgroups of four waves, the second half empty
KILLED_ROW, CONST_ROW, TIE_ROW = 4, 1, 3
LOSS_TOL = dict(rtol=2e-5, atol=1e-4)
GRAD_TOL = dict(rtol=1e-4, atol=1e-6)


@functools.lru_cache(maxsize=None)
def loss_inputs(N, regime, S=S_ROWS):
    """(pos [S], neg [S, N], w [S]) fp32, fixed seed; never written to."""
    gen = torch.Generator().manual_seed(1000 * REGIMES.index(regime) + N + 7 * S)
    amp = 60.0 if regime == "saturated" else 4.0
    while True:
        pos = torch.randn(S, generator=gen) * amp
        neg = torch.randn(S, N, generator=gen) * amp
        w = torch.rand(S, generator=gen) + 0.5
        # (saturated scores are drawn again while a positive beats all its negatives by the margin - that row of the
        # margin loss is all zeros, gradients included, and checks nothing - or fewer than 90 % of the logistic
        # gradients are saturated (`logistic_saturation`).  Either happens to rows of 5 scores only.)
        top = 0.5 * LOSS_SCALE * w.double()[:, None] / N
        g = top * torch.sigmoid(neg.double() + MARGIN)
        saturated = float(((g <= 1e-6) | (top - g <= 1e-6)).double().mean())
        if regime != "saturated" or (bool((neg - pos[:, None] + MARGIN > 1.0).any(dim=1).all()) and saturated >= 0.9):
            break
    if regime == "killed":  # what K7 leaves: padding columns, and one triple all of whose negatives are padding
        dead = torch.rand(N, generator=gen) < 0.3
        kill = dead[None, :].expand(S, N).clone()
        kill[KILLED_ROW] = True
        neg = torch.where(kill, neg + BAD, neg)
    if regime == "ties":
        neg[CONST_ROW] = 0.75
        pos[TIE_ROW] = 1.5
        neg[TIE_ROW, ::3] = 1.5 - MARGIN  # relu'(0) = 0: no gradient there
    return pos, neg, w


def oracle_loss(variant, pos, neg, w, dtype):
    """(loss, d_pos, d_neg) of `oracle.kge.loss_value` with autograd, in `dtype`."""
    kind, adv = VARIANTS[variant]
    po, no = (x.detach().to(dtype, copy=True).requires_grad_(True) for x in (pos, neg))
    loss = kge.loss_value(kind, po, no, w.to(dtype), margin=MARGIN, adversarial=adv, adversarial_scale=BETA,
                          loss_scale=LOSS_SCALE, n_entity=N_ENTITY)
    loss.backward()
    return loss.detach(), po.grad, no.grad


def rule_row_norm(variant, pos, neg, w, dtype):
    """(m, L / C) per row from the definition (loss_rows.h / besskge_hip.h: bess_loss_fwd_bwd_norm), in `dtype`."""
    kind, adv = VARIANTS[variant]
    p, x, w = pos.to(dtype), neg.to(dtype), w.to(dtype)
    if kind == "ssce":
        z = x + float(np.log(N_ENTITY - 1) - np.log(x.shape[1]))
        m = torch.maximum(z.max(-1).values, p)
        L = torch.exp(z - m[:, None]).sum(-1) + torch.exp(p - m)
    elif adv:
        m = (BETA * x).max(-1).values
        L = torch.exp(BETA * x - m[:, None]).sum(-1)
    else:
        m = torch.zeros_like(p)
        L = torch.full_like(p, x.shape[1])
    C = (0.5 if kind == "logsigmoid" else 1.0) * LOSS_SCALE * w
    return torch.stack([m, L / C], dim=1)


@functools.lru_cache(maxsize=None)
def loss_references(variant, N, regime, one_weight, S=S_ROWS):
    """{name: (float64 reference, fp32 oracle)} of one case; computed once, never written to."""
    pos, neg, w = loss_inputs(N, regime, S)
    if one_weight:
        w = w[:1]
    w_rows = w.expand(S)
    r64, r32 = oracle_loss(variant, pos, neg, w_rows, torch.float64), oracle_loss(variant, pos, neg, w_rows, torch.float32)
    out = dict(zip(("loss", "d_pos", "d_neg"), zip(r64, r32)))
    out["row_norm"] = (rule_row_norm(variant, pos, neg, w_rows, torch.float64),
                       rule_row_norm(variant, pos, neg, w_rows, torch.float32))
    return out


def error_in_tolerances(x, ref, rtol, atol):
    """max |x - ref| / (atol + rtol |ref|): <= 1 is `assert_close`'s pass."""
    return float(((x.double() - ref).abs() / (atol + rtol * ref.abs())).max())


def tolerance_of(name):
    return LOSS_TOL if name == "loss" else GRAD_TOL


@functools.lru_cache(maxsize=None)
def oracle_error(variant, regime, name):
    """Largest error of the fp32 CPU oracle against float64, in tolerances, over the cases of one value regime."""
    return max(error_in_tolerances(*reversed(loss_references(variant, N, regime, one_weight)[name]), **tolerance_of(name))
               for N in ROW_LENGTHS for one_weight in (False, True))


def close64(what, got, ref, e_oracle, rtol, atol):
    """`got` against the float64 `ref` at (rtol, atol) - or, where the fp32 CPU oracle is itself outside them
    (`e_oracle` > 1, in tolerances: the quantity is ill-conditioned in fp32 in that regime), at 4 x the oracle's error
    (a different summation order over up to 6148 terms).  The bound never depends on `got`."""
    assert bool(torch.isfinite(ref).all()) and got.shape == ref.shape
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    e_kernel = error_in_tolerances(got.cpu(), ref, rtol, atol)
    factor = 1.0 if e_oracle <= 1.0 else 4.0 * e_oracle
    if factor > 1.0 or e_kernel > 1.0:
        print(f"{what}: kernel at {e_kernel:.3g} x, fp32 oracle at up to {e_oracle:.3g} x of rtol={rtol} atol={atol}")
    assert e_kernel <= factor, f"{what}: kernel at {e_kernel:.3g} x the tolerance, fp32 oracle at {e_oracle:.3g} x"


def logistic_saturation(variant, N):
    """Share of the log-sigmoid loss's negative-score gradients (float64) within 1e-6 of 0 or of their maximum, the
    gradient at sigmoid = 1: (1/2) loss_scale w a[s, j], a = the negative's weight."""
    pos, neg, w = loss_inputs(N, "saturated")
    d_neg = loss_references(variant, N, "saturated", False)["d_neg"][0]
    a = kge.negative_weights(neg.double(), VARIANTS[variant][1], BETA)
    top = 0.5 * LOSS_SCALE * w.double()[:, None] * a
    return float(((d_neg.abs() <= 1e-6) | ((top - d_neg).abs() <= 1e-6)).double().mean())


@pytest.mark.parametrize("N", ROW_LENGTHS)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_float64_oracle_agrees_with_fp32_on_normal_scores(variant, N):
    for one_weight in (False, True):
        ref = loss_references(variant, N, "normal", one_weight)
        for name, (r64, r32) in ref.items():
            assert r64.dtype == torch.float64 and r32.dtype == torch.float32
            torch.testing.assert_close(r32.double(), r64, **tolerance_of(name))


@pytest.mark.parametrize("N", ROW_LENGTHS)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_regimes_are_what_they_claim(variant, N):
    """The guards of the GPU comparison, on the references: no case can pass because everything in it is zero."""
    kind, adv = VARIANTS[variant]
    d_neg = loss_references(variant, N, "saturated", False)["d_neg"][0]
    assert bool((d_neg != 0).any(dim=1).all())
    assert bool((d_neg.abs() > GRAD_TOL["atol"]).any(dim=1).all())  # ... and not below the absolute tolerance
    if kind == "logsigmoid":
        assert logistic_saturation(variant, N) >= 0.9
    pos, neg, w = loss_inputs(N, "killed")
    assert bool((neg[KILLED_ROW] < BAD / 2).all()) and not bool((neg[0] < BAD / 2).all())
    one_row = oracle_loss(variant, pos[KILLED_ROW:KILLED_ROW + 1], neg[KILLED_ROW:KILLED_ROW + 1],
                          w[KILLED_ROW:KILLED_ROW + 1], torch.float64)[0]
    assert bool(torch.isfinite(one_row))
    pos, neg, w = loss_inputs(N, "ties")
    assert bool((neg[CONST_ROW] == neg[CONST_ROW, 0]).all())
    assert bool((neg[TIE_ROW, ::3] - pos[TIE_ROW] + MARGIN == 0).all())
    if kind == "margin":
        tie_grad = loss_references(variant, N, "ties", False)["d_neg"][0][TIE_ROW, ::3]
        assert bool((tie_grad == 0).all())


# ================================================================================================ ranks: the rules
MODES = ["optimistic", "pessimistic", "average"]


def rule_ranks_from_scores(pos, cand, mode, worst_inf):
    """`Evaluation.ranks_from_scores` with integer counts (NaN positives count as -inf)."""
    p = torch.nan_to_num(pos.clone(), nan=-torch.inf)[:, None]  # (as the method does, in place, to its argument)
    n = cand.shape[1]
    gt = (cand > p).sum(-1)
    ge = (cand >= p).sum(-1)
    if mode == "optimistic":
        twice_better, worst = 2 * gt, gt == n
    elif mode == "pessimistic":
        twice_better, worst = 2 * ge, ge == n
    else:
        twice_better, worst = gt + ge, (gt == n) | (ge == n)
    rank = 1.0 + twice_better.double() / 2
    if worst_inf:
        rank[worst] = torch.inf
    return rank.float()


def rule_ranks_from_indices(truth, cand, worst_inf):
    """`Evaluation.ranks_from_indices`: 1-based position of the first occurrence of the truth, else n + 1 (or inf)."""
    hit = cand == truth[:, None]
    first = hit.long().argmax(dim=1) + 1
    rank = torch.where(hit.any(dim=1), first.float(), torch.tensor(float(cand.shape[1] + 1)))
    if worst_inf:
        rank[~hit.any(dim=1)] = torch.inf
    return rank


SCORE_VALUES = torch.tensor([-1.0, -0.5, 0.0, 0.5, 1.0, 1.5])
SCORE_KINDS = ["nan_positive", "inf_positive", "neg_inf_candidate", "beaten_by_all", "beaten_by_none"]


def rank_score_case(n_row, n_cand, first_kind):
    """Scores of six values (ties in every lane); row r < 5 is of kind SCORE_KINDS[(first_kind + r) % 5]."""
    gen = torch.Generator().manual_seed(100 * n_row + n_cand)
    pos = SCORE_VALUES[torch.randint(0, 6, (n_row,), generator=gen)]
    cand = SCORE_VALUES[torch.randint(0, 6, (n_row, n_cand), generator=gen)]
    for r in range(min(n_row, len(SCORE_KINDS))):
        kind = SCORE_KINDS[(first_kind + r) % len(SCORE_KINDS)]
        if kind == "nan_positive":
            pos[r] = float("nan")
            cand[r, n_cand // 2] = -torch.inf  # equal to the NaN positive: '>=' counts it
        elif kind == "inf_positive":
            pos[r] = torch.inf
        elif kind == "neg_inf_candidate":
            cand[r, n_cand - 1] = -torch.inf
        elif kind == "beaten_by_all":
            pos[r] = -2.0
        else:
            pos[r] = 2.0
    return pos, cand


def rank_index_case(n_row, n_cand, first_kind):
    """Ordered ids above 2^31; row r is of kind (first_kind + r) % 4: truth absent / present twice / at the last
    position / behind an id that differs from it in bit 32 only."""
    gen = torch.Generator().manual_seed(10 * n_row + n_cand)
    cand = torch.randint(2**31, 2**40, (n_row, n_cand), generator=gen, dtype=torch.int64) * 2  # even: truths are odd
    truth = torch.randint(2**31, 2**40, (n_row,), generator=gen, dtype=torch.int64) * 2 + 1
    for r in range(n_row):
        kind = (first_kind + r) % 4
        at = int(torch.randint(0, n_cand, (1,), generator=gen))
        if kind == 1:
            cand[r, at] = truth[r]
            cand[r, (at + n_cand // 2) % n_cand] = truth[r]
        elif kind == 2:
            cand[r, n_cand - 1] = truth[r]
        elif kind == 3:
            cand[r, at] = truth[r]
            if at > 0:
                cand[r, at - 1] = truth[r] ^ (1 << 32)
    return truth, cand


def test_rank_rules_equal_brute_force():
    for n_cand, first_kind in itertools.product([1, 5, 65], range(5)):
        pos, cand = rank_score_case(9, n_cand, first_kind)
        assert bool(torch.isnan(pos).any()) and bool((pos == torch.inf).any()) and bool((cand == -torch.inf).any())
        for mode, worst_inf in itertools.product(MODES, [False, True]):
            got = rule_ranks_from_scores(pos, cand, mode, worst_inf)
            assert torch.equal(got, reference_ranks(pos, cand, mode, worst_inf))
            for r in range(9):
                p = -float("inf") if bool(torch.isnan(pos[r])) else float(pos[r])
                gt = sum(1 for c in cand[r].tolist() if c > p)
                ge = sum(1 for c in cand[r].tolist() if c >= p)
                better = dict(optimistic=gt, pessimistic=ge, average=(gt + ge) / 2)[mode]
                worst = dict(optimistic=gt == n_cand, pessimistic=ge == n_cand, average=ge == n_cand)[mode]
                assert float(got[r]) == (float("inf") if worst_inf and worst else 1 + better)
            if n_cand > 1:
                assert len(set(got.tolist())) > 2
    for n_cand, first_kind, worst_inf in itertools.product([1, 10], range(4), [False, True]):
        truth, cand = rank_index_case(9, n_cand, first_kind)
        got = rule_ranks_from_indices(truth, cand, worst_inf)
        for r in range(9):
            row = cand[r].tolist()
            t = int(truth[r])
            want = row.index(t) + 1 if t in row else (float("inf") if worst_inf else n_cand + 1)
            assert float(got[r]) == want
        assert bool((got > n_cand).any()) and bool((got <= n_cand).any())


# ================================================================================================ 1. K7 on the device
def mask_case(S, N, diag_step, ht, ppp, mask_rows, mask_cols, seed=5):
    gen = torch.Generator().manual_seed(seed)
    scores = integer_scores(S, N, gen)
    mask = None
    if mask_rows is not None:
        rows = S if mask_rows == "S" else mask_rows
        mask = torch.rand(rows, mask_cols, generator=gen) > 0.4
        if diag_step > 0:
            # the override, both ways: the first two diagonal elements under the mask are one real negative (not
            # killed although on the diagonal) and one padding negative (killed once, not twice)
            diag = rule_kill(S, N, diag_step, ht, ppp, None)
            diag[:, : N - mask_cols] = False
            under = diag.nonzero().tolist()
            if under:  # (in two different columns: rows of an 'ht' block share theirs)
                (s0, j0), (s1, j1) = under[0], next(x for x in under if x[1] != under[0][1])
                cut = ppp // 2
                mrow = (lambda s: 0) if rows == 1 else ((lambda s: int(s % ppp >= cut)) if rows == 2 else (lambda s: s))
                mask[mrow(s0), j0 - (N - mask_cols)] = True
                mask[mrow(s1), j1 - (N - mask_cols)] = False
    return scores, mask


def run_mask(dev, scores, diag_step, ht, ppp, mask):
    from besskge import _native as nat

    got = scores.to(dev)
    nat.mask_scores(got, diag_step, ht, ppp, None if mask is None else mask.to(dev))
    return got.cpu()


def check_mask(dev, S, N, diag_step, ht, ppp, mask_rows, mask_cols):
    scores, mask = mask_case(S, N, diag_step, ht, ppp, mask_rows, mask_cols)
    want, kill = rule_mask(scores, diag_step, ht, ppp, mask)
    got = run_mask(dev, scores, diag_step, ht, ppp, mask)
    assert int((got != scores).sum()) == int(kill.sum())
    assert torch.equal(got, want)
    return kill


@gpu
@pytest.mark.parametrize("mask_rows,mask_cols", [(None, 37)] + list(itertools.product([1, 2, "S"], [37, 28])))
@pytest.mark.parametrize("diag_step", [0, 1, 5])
@pytest.mark.parametrize("ht", [False, True])
def test_mask_scores_equals_the_rule(dev, ht, diag_step, mask_rows, mask_cols):
    S, N, ppp = 24, 37, 6
    # (`ppp` as BessKGE passes it: 0 where neither 'ht' nor a 2-row mask needs the blocks)
    kill = check_mask(dev, S, N, diag_step, ht, ppp if (ht or mask_rows == 2 or diag_step > 0) else 0, mask_rows, mask_cols)
    if diag_step == 5:  # some diagonal positions fall off the row
        assert int(rule_kill(S, N, 5, ht, ppp, None).sum()) < S
    if diag_step > 0 or mask_rows is not None:
        assert bool(kill.any()) and not bool(kill.all())


@gpu
def test_mask_scores_grid_stride_loop(dev):
    S, N = 520, 2051
    assert S * N > 4096 * 256  # more elements than the largest grid has threads
    kill = check_mask(dev, S, N, 3, True, 8, 2, 1000)
    assert bool(kill[S - 8:, N - 1000:].any()) and bool(kill[:, : N - 1000].any())


@gpu
@pytest.mark.parametrize("S,N", [(0, 37), (24, 0)])
def test_mask_scores_empty(dev, S, N):
    scores = torch.zeros(S, N)
    mask = torch.zeros(1, max(N, 1), dtype=torch.bool)
    assert run_mask(dev, scores, 1, False, 0, mask).shape == (S, N)
    torch.cuda.synchronize()


@gpu
def test_mask_scores_rejections(dev):
    scores = integer_scores(24, 37, torch.Generator().manual_seed(0))
    with pytest.raises(RuntimeError, match="mask_rows 3 not 1, 2 or n_triple"):
        run_mask(dev, scores, 0, False, 6, torch.ones(3, 37, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="even block size"):
        run_mask(dev, scores, 1, True, 3, None)


# ================================================================================================ 2. K8 on the device
LAYOUTS = {  # name -> (ld_neg - N, ld_dneg - N, first float of neg in its buffer)
    "dense": (0, 0, 0),
    "padded_vector": (4, 4, 0),    # 16-byte rows still
    "odd_ld": (1, 3, 0),           # rows not 16-byte aligned: streamed (CH = 0) at any N
    "misaligned": (0, 0, 1),       # the same through the base pointer
}
SENTINEL = 12345.0


def loss_desc(variant, N):
    from besskge import _native as nat

    kind, adv = VARIANTS[variant]
    l = nat.LossDesc()
    l.kind = dict(logsigmoid=0, margin=1, ssce=2)[kind]
    l.adversarial, l.margin, l.adversarial_scale, l.loss_scale = int(adv), MARGIN, BETA, LOSS_SCALE
    l.ssce_shift = float(np.log(N_ENTITY - 1) - np.log(N))
    return l


def launch_loss_norm(dev, l, pos, neg, w, layout, grad):
    """`bess_loss_fwd_bwd_norm` with free leading dimensions.  Returns (loss, d_pos, d_neg buffer [S, ld_dneg], row_norm)
    on the CPU; padding of `neg` is NaN (reading it shows), the d_neg buffer is pre-filled with SENTINEL."""
    from besskge import _native as nat

    S, N = neg.shape
    pad_n, pad_d, first = LAYOUTS[layout]
    ld_n, ld_d = N + pad_n, N + pad_d
    nbuf = torch.full((first + S * ld_n,), float("nan"), device=dev)
    nview = nbuf[first:].view(S, ld_n)
    nview[:, :N] = neg.to(dev)
    assert (nview.data_ptr() % 16 == 0) == (first == 0)
    pos_d, w_d = pos.to(dev), w.to(dev)
    row_loss = torch.full((S,), SENTINEL, device=dev)
    loss = torch.full((1,), SENTINEL, device=dev)
    norm = torch.full((S, 2), SENTINEL, device=dev)
    dp = torch.full((S,), SENTINEL, device=dev) if grad else None
    dn = torch.full((S, ld_d), SENTINEL, device=dev) if grad else None
    nat._launch("bess_loss_fwd_bwd_norm", dev, ctypes.byref(l), pos_d.data_ptr(), nview.data_ptr(), S, N, ld_n,
                w_d.data_ptr(), w_d.numel(), row_loss.data_ptr(), loss.data_ptr(), dp.data_ptr() if grad else 0,
                dn.data_ptr() if grad else 0, ld_d, norm.data_ptr())
    return loss.cpu().reshape(()), dp.cpu() if grad else None, dn.cpu() if grad else None, norm.cpu()


@gpu
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("N", ROW_LENGTHS)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_loss_kernels_equal_the_float64_oracle(dev, variant, N, regime):
    pos, neg, w = loss_inputs(N, regime)
    l = loss_desc(variant, N)
    for one_weight, layout in itertools.product([False, True], LAYOUTS):
        what = f"{variant} N={N} {regime} {'one weight' if one_weight else 'weights'} {layout}"
        ref = loss_references(variant, N, regime, one_weight)
        wt = w[:1] if one_weight else w
        loss, dp, dnbuf, norm = launch_loss_norm(dev, l, pos, neg, wt, layout, True)
        dn = dnbuf[:, :N]
        for name, got in (("loss", loss), ("d_pos", dp), ("d_neg", dn), ("row_norm", norm)):
            close64(f"{what}: {name}", got, ref[name][0], oracle_error(variant, regime, name), **tolerance_of(name))
        assert bool((dnbuf[:, N:] == SENTINEL).all()), f"{what}: wrote to the padding of d_neg"
        if regime == "saturated":
            assert bool((dn != 0).any(dim=1).all())
        if regime == "ties" and VARIANTS[variant][0] == "margin":
            assert bool((dn[TIE_ROW, ::3] == 0).all())
        # GRAD = false: the same loss, bit for bit
        loss0, _, _, norm0 = launch_loss_norm(dev, l, pos, neg, wt, layout, False)
        assert torch.equal(loss0, loss) and torch.equal(norm0, norm), what


# ================================================================================================ 3. grids and tickets
def one_launch_case(dev, S, grad=True):
    from besskge import _native as nat

    N, variant = 8, "logsigmoid_adv"
    pos, neg, w = loss_inputs(N, "normal", S)
    ref = loss_references(variant, N, "normal", False, S)
    args = (loss_desc(variant, N), pos.to(dev), neg.to(dev), w.to(dev))
    loss, dp, dn = nat.loss_fwd_bwd(*args, True)
    again = nat.loss_fwd_bwd(*args, False)[0]
    what = f"one launch, S={S}"
    for name, got in (("loss", loss), ("d_pos", dp), ("d_neg", dn)):
        r64, r32 = ref[name]
        close64(f"{what}: {name}", got, r64, error_in_tolerances(r32, r64, **tolerance_of(name)), **tolerance_of(name))
    assert torch.equal(loss, again), f"{what}: not reproducible"


@gpu
def test_one_launch_loss_over_grid_sizes_on_one_stream(dev):
    """15, 16, 17, 1, 256 and 16 workgroups one after the other: a ticket counter that one call leaves non-zero
    breaks the next."""
    for S in (60, 64, 65, 4, 1024, 61):
        one_launch_case(dev, S)


@gpu
def test_loss_of_more_rows_than_one_launch_takes(dev):
    S = 16388
    assert S > 4 * 4096  # summed by a second launch; the counters stay untouched
    one_launch_case(dev, S)
    one_launch_case(dev, 64)


# ================================================================================================ 4. ranks on the device
@gpu
@pytest.mark.parametrize("n_cand", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("n_row", [1, 5, 9])
def test_ranks_from_scores_equal_integer_counts(dev, n_row, n_cand):
    from besskge import _native as nat

    for first_kind in range(len(SCORE_KINDS) if n_row < len(SCORE_KINDS) else 1):
        pos, cand = rank_score_case(n_row, n_cand, first_kind)
        cand_d = cand.to(dev)
        for mode, worst_inf in itertools.product(range(3), [False, True]):
            want = rule_ranks_from_scores(pos, cand, MODES[mode], worst_inf)
            # the positive as it is (NaN: the kernel's own rule) and as `Evaluation.ranks_from_scores` hands it on
            for p in (pos, torch.nan_to_num(pos.clone(), nan=-torch.inf)):
                got = nat.ranks_from_scores(p.to(dev), cand_d, mode, worst_inf).cpu()
                assert torch.equal(got, want), (SCORE_KINDS[first_kind], MODES[mode], worst_inf)


@gpu
@pytest.mark.parametrize("n_cand", [1, 10, 100])
@pytest.mark.parametrize("n_row", [1, 257])
def test_ranks_from_indices_equal_first_position(dev, n_row, n_cand):
    from besskge import _native as nat

    for first_kind in range(4 if n_row < 4 else 1):
        truth, cand = rank_index_case(n_row, n_cand, first_kind)
        assert int(cand.min()) > 2**31 and int(truth.min()) > 2**31
        for worst_inf in (False, True):
            want = rule_ranks_from_indices(truth, cand, worst_inf)
            got = nat.ranks_from_indices(truth.to(dev), cand.to(dev), worst_inf).cpu()
            assert torch.equal(got, want), (first_kind, worst_inf)
