"""`bess_regularize_triples` and the regularised training step, against torch autograd in float64 on the CPU.

The oracle gathers the rows, takes `abs().pow(p)` or `(re^2 + im^2).pow(p / 2)`, weights, sums, and lets `backward()`
produce the gradients; nothing of the kernel's gradient formula is written here.  The one convention that is: where a
modulus is exactly 0 autograd's chain rule gives inf * 0 = NaN for p < 2; the specified value there is 0.

Tolerances (fp32 unit roundoff u = 2^-24; inputs convert exactly from f16 / f32 to float64):
  gradient elements, p in {1, 2, 3}: 2e-6 relative + 1e-30 (at most eight roundings per element); where the kernel adds
      into pre-filled rows, one more rounding of the sum at the magnitude of the stored element.
  p = 2.5: 4 x the largest relative deviation measured on an MI355X over the cases below (P25_MEASURED).
  penalty: L * u relative, L = the longest chain of dependent additions of the summation implemented (`chain_length`),
      all terms being non-negative.
  relation gradient under colliding atomics: 1e-5 of the row's float64 sum of absolute contributions; the row is
      pre-filled like d_tail, so each of the n atomics on it also rounds at the magnitude of what was there: + n u |before|.
"""

import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
#: largest |got - want| / |want| of a p = 2.5 gradient element over the kernel cases of this file, on an MI355X
#: (ROCm 7 `powf`; printed by the test with `pytest -s`); the test holds 4 x that
P25_MEASURED = 2.81e-7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------------- 1. the kernel
def phi(x, p, modulus):
    if modulus:
        d = x.shape[-1] // 2
        return (x[..., :d] ** 2 + x[..., d:] ** 2).pow(p / 2).sum(-1)
    return x.abs().pow(p).sum(-1)


def chain_length(S, unit):
    """Longest chain of dependent fp32 additions behind penalty[0]: a lane adds the terms of head and tail of its
    chunks (at most 8 scalars per pass, ceil(unit / (64 * vec)) passes: <= unit / 64 + 8 scalars, two adds each), the
    wave's butterfly has 6 levels, the triple's term one add; the last workgroup's threads add ceil(S / 256) terms
    each, then a tree of 8 levels.  Eight more for the roundings inside one term (squares, sqrt / powf, the scales)."""
    return 2 * (unit // 64 + 8) + 6 + 1 + math.ceil(S / 256) + 8 + 8


def kernel_case(dev, dtype, W, mode, p, S, per_triple_weight, collide=False, relation_coef=0.07, seed=0):
    """Runs the kernel (gradient call and value-only call) and the float64 oracle on the same operands."""
    from besskge import _native as nat

    gen = torch.Generator().manual_seed(seed + 7 * W + S)
    mod_e, mod_r = mode in ("moduli", "rotate"), mode == "moduli"
    Wr = W // 2 if mode == "rotate" else W
    M, n_rel = 23, 5
    ent = (torch.rand(M, W, generator=gen) * 2 - 1).to(dtype)
    rel = (torch.rand(n_rel, Wr, generator=gen) * 2 - 1).to(dtype)
    ent[3] = 0  # a row that is exactly zero
    ent[4, 1] = 0  # a coordinate that is exactly zero
    if mod_e:
        ent[4, 1 + W // 2] = 0  # ... and its modulus
    rel[1, 0] = 0
    if mod_r:
        rel[1, Wr // 2] = 0
    h_idx = torch.randint(M, (S,), generator=gen, dtype=torch.int32)
    t_idx = torch.randint(M, (S,), generator=gen, dtype=torch.int32)
    r_idx = torch.randint(n_rel, (S,), generator=gen, dtype=torch.int32)
    h_idx[0], t_idx[0], r_idx[0] = 3, 4, 1
    if collide:  # every triple on the same head row and the same relation: all atomics meet on one row
        h_idx[:] = 4
        r_idx[:] = 1
    weight = torch.rand(S if per_triple_weight else 1, generator=gen) + 0.5
    e_coef, scale = 0.05, 2.0
    before_t = (torch.randn(S, W, generator=gen) * 0.1)
    before_r = (torch.randn(n_rel, Wr, generator=gen) * 0.1)
    loss0, factor = 3.25, 0.5

    # --- float64 oracle
    h = ent.double()[h_idx.long()].requires_grad_(True)
    t = ent.double()[t_idx.long()].requires_grad_(True)
    r = rel.double()[r_idx.long()].requires_grad_(True)
    c = scale * weight.double().expand(S)
    terms = c * (e_coef * (phi(h, p, mod_e) + phi(t, p, mod_e)) + relation_coef * phi(r, p, mod_r))
    terms.sum().backward()
    want = dict(penalty=float(terms.detach().sum()))
    for name, leaf, modulus in (("dh", h, mod_e), ("dt", t, mod_e), ("dr", r, mod_r)):
        g = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)
        x = leaf.detach()
        d = x.shape[-1] // 2
        zero = (torch.cat([x[:, :d] ** 2 + x[:, d:] ** 2] * 2, dim=1) == 0) if modulus else (x == 0)
        assert not bool(torch.isnan(g)[~zero].any())  # autograd's inf * 0 only at exact zeros ...
        want[name] = torch.where(zero, torch.zeros_like(g), g)  # ... where the gradient is 0
    want["d_rel"] = torch.zeros(n_rel, Wr, dtype=torch.float64).index_add_(0, r_idx.long(), want["dr"])
    want["d_rel_abs"] = torch.zeros(n_rel, Wr, dtype=torch.float64).index_add_(0, r_idx.long(), want["dr"].abs())

    # --- the kernel
    ent_d, rel_d = ent.to(dev), rel.to(dev)
    head, tail = nat.RowSource(ent_d, h_idx.to(dev)), nat.RowSource(ent_d, t_idx.to(dev))
    dh = torch.zeros(S, W, device=dev)  # adds into zeros: the gradient itself
    dt = before_t.to(dev)  # adds into what a backward has left
    drel = before_r.to(dev) if relation_coef > 0 else None
    loss = torch.full((), loss0, device=dev)
    args = (head, tail, rel_d if relation_coef > 0 else None, r_idx.to(dev) if relation_coef > 0 else None,
            weight.to(dev), p, e_coef, relation_coef, scale, (1 if mod_e else 0) | (2 if mod_r else 0))
    pen = nat.regularize_triples(*args, dh, dt, drel, loss=loss, loss_factor=factor)
    pen2 = nat.regularize_triples(*args, dh.clone(), dt.clone(), drel.clone() if drel is not None else None)
    value = nat.regularize_triples(*args)  # value only
    torch.cuda.synchronize()
    got = dict(penalty=pen.cpu(), penalty_again=pen2.cpu(), value=value.cpu(), dh=dh.cpu().double(),
               dt_after=dt.cpu().double(), dt=dt.cpu().double() - before_t.double(), loss=float(loss),
               d_rel=(drel.cpu().double() - before_r.double()) if drel is not None else None)
    want.update(n_adds=torch.bincount(r_idx.long(), minlength=n_rel).double()[:, None], before_r=before_r.double())
    want.update(loss=loss0 + factor * want["penalty"], unit=max(W // (2 if mod_e else 1), Wr // (2 if mod_r else 1)))
    return got, want


def check_kernel_case(got, want, p, S, rel_tol):
    """`rel_tol`: relative bound on a gradient element.  Returns the largest relative deviation seen."""
    worst = 0.0
    for name, extra in (("dh", None), ("dt", got["dt_after"])):
        g, w = got[name], want[name]
        assert bool(torch.isfinite(g).all()), f"{name}: not finite"
        tol = rel_tol * w.abs() + 1e-30
        if extra is not None:
            tol = tol + U * extra.abs()  # the rounding of (what was there + gradient), at the stored element
        else:
            rel = ((g - w).abs() / w.abs().clamp(min=1e-30))[w != 0]
            worst = max(worst, float(rel.max()) if rel.numel() else 0.0)
        bad = (g - w).abs() > tol
        assert not bool(bad.any()), f"{name}: {int(bad.sum())} elements off, worst {float(((g - w).abs() - tol).max()):.3e}"
        assert bool((g[w == 0] == 0).all()) or extra is not None, f"{name}: non-zero gradient at a zero"
    if got["d_rel"] is not None:
        g, w = got["d_rel"], want["d_rel"]
        # (the kernel adds into what the backward left in the row: each of the row's atomics also rounds at the
        # magnitude of what was there)
        tol = max(1e-5, rel_tol) * want["d_rel_abs"] + want["n_adds"] * U * want["before_r"].abs() + 1e-30
        assert bool(torch.isfinite(g).all()) and not bool(((g - w).abs() > tol).any()), "d_rel_table"
    L = chain_length(S, want["unit"]) + (0 if p in (1.0, 2.0, 3.0) else 8)  # (powf: a few units in the last place)
    assert abs(float(got["penalty"]) - want["penalty"]) <= L * U * want["penalty"], (float(got["penalty"]), want["penalty"])
    assert torch.equal(got["penalty"], got["penalty_again"]), "the penalty is not bitwise reproducible"
    # (the value-only call is another instantiation of the kernel: the same bound, not the same bits)
    assert abs(float(got["value"]) - want["penalty"]) <= L * U * want["penalty"], (float(got["value"]), want["penalty"])
    assert abs(got["loss"] - want["loss"]) <= 4 * U * abs(want["loss"]) + L * U * want["penalty"]
    return worst


@pytest.mark.parametrize("p", [1.0, 2.0, 3.0, 2.5])
@pytest.mark.parametrize("mode", ["coordinates", "moduli", "rotate"])
@pytest.mark.parametrize("W", [6, 64, 100, 512, 2000])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_kernel_against_float64(dev, dtype, W, mode, p, capsys):
    worst = 0.0
    rel_tol = 2e-6 if p != 2.5 else 4 * P25_MEASURED
    for S, per_triple in ((1, False), (3, True), (257, False), (257, True)):
        got, want = kernel_case(dev, dtype, W, mode, p, S, per_triple)
        worst = max(worst, check_kernel_case(got, want, p, S, rel_tol))
    with capsys.disabled():
        if p == 2.5:
            print(f"\n[p=2.5 {dtype} W={W} {mode}] largest relative deviation of a gradient element: {worst:.3e}")


@pytest.mark.parametrize("p", [1.0, 3.0, 2.5])
@pytest.mark.parametrize("mode", ["coordinates", "moduli", "rotate"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_kernel_with_every_triple_on_one_row(dev, dtype, mode, p):
    rel_tol = 2e-6 if p != 2.5 else 4 * P25_MEASURED
    for W, S in ((100, 257), (6, 3)):
        got, want = kernel_case(dev, dtype, W, mode, p, S, True, collide=True)
        check_kernel_case(got, want, p, S, rel_tol)


@pytest.mark.parametrize("mode", ["coordinates", "moduli"])
def test_kernel_without_a_relation_term(dev, mode):
    """relation_coef = 0: no relation rows, no d_rel_table (NULL)."""
    for dtype in (torch.float32, torch.float16):
        got, want = kernel_case(dev, dtype, 100, mode, 3.0, 257, True, relation_coef=0.0)
        assert got["d_rel"] is None
        check_kernel_case(got, want, 3.0, 257, 2e-6)


def test_wrapper_refuses_mismatched_operands(dev):
    from besskge import _native as nat

    ent = torch.rand(10, 8, device=dev)
    idx = torch.zeros(4, dtype=torch.int32, device=dev)
    w = torch.ones(1, device=dev)
    src = nat.RowSource(ent, idx)
    with pytest.raises(RuntimeError, match="d_head and d_tail"):
        nat.regularize_triples(src, src, None, None, w, 3.0, 0.1, 0.0, d_head=torch.zeros(4, 8, device=dev))
    with pytest.raises(RuntimeError, match="odd width"):
        nat.regularize_triples(nat.RowSource(ent[:, :7].contiguous(), idx), nat.RowSource(ent[:, :7].contiguous(), idx),
                               None, None, w, 3.0, 0.1, 0.0, flags=1)
    with pytest.raises(ValueError):
        nat.regularize_triples(src, src, None, None, w, 3.0, 0.1, 0.0, d_head=torch.zeros(4, 7, device=dev),
                               d_tail=torch.zeros(4, 8, device=dev))
    with pytest.raises(RuntimeError, match="weight_len"):
        nat.regularize_triples(src, src, None, None, torch.ones(3, device=dev), 3.0, 0.1, 0.0)


# ------------------------------------------------------------------------------------- 2. the training step
def make_model(dev, scorer, n, per_triple, scheme, dtype, reg, loss_scale=1.0, d=16, ppp=8, K=8, score_moving=False,
               seed=0):
    """(model, batch of one micro-batch per replica, initial tables in float64)."""
    from besskge import scoring
    from besskge.bess import EmbeddingMovingBessKGE, ScoreMovingBessKGE
    from besskge.loss import LogSigmoidLoss
    from besskge.negative_sampler import RandomShardedNegativeSampler
    from besskge.sharding import Sharding

    M, n_rel = 40, 5
    sharding = Sharding.create(M * n, n, seed=0)
    torch.manual_seed(seed)
    if scorer in ("TransE", "RotatE", "PairRE"):
        fn = getattr(scoring, scorer)(not per_triple, 1, sharding, n_rel, d, device=dev, dtype=dtype)
    else:
        fn = getattr(scoring, scorer)(not per_triple, sharding, n_rel, d, device=dev, dtype=dtype)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():  # uniform in [-1, 1]
        fn.entity_embedding.copy_((torch.rand(fn.entity_embedding.shape, generator=gen) * 2 - 1).to(dtype))
        fn.relation_embedding.copy_((torch.rand(fn.relation_embedding.shape, generator=gen) * 2 - 1).to(dtype))
    ns = RandomShardedNegativeSampler(K, sharding, 0, scheme, local_sampling=False, flat_negative_format=not per_triple)
    cls = ScoreMovingBessKGE if score_moving else EmbeddingMovingBessKGE
    model = cls(negative_sampler=ns, score_fn=fn, regularizer=reg,
                loss_fn=LogSigmoidLoss(margin=2.0, negative_adversarial_sampling=False, loss_scale=loss_scale))
    return model


def make_batch(n, per_triple, scheme, ppp=8, K=8, micro=1, seed=0, weight=False):
    rng = np.random.default_rng(seed)
    S = n * ppp
    B = S if per_triple else (2 if scheme == "ht" else 1)
    rows = micro * n
    b = dict(head=rng.integers(40, size=(rows, n, ppp)), relation=rng.integers(5, size=(rows, n, ppp)),
             tail=rng.integers(40, size=(rows, n, ppp)), negative=rng.integers(40, size=(rows, n, B, K)))
    b = {k: torch.from_numpy(v.astype(np.int32)) for k, v in b.items()}
    if weight:
        b["triple_weight"] = torch.from_numpy(rng.random(size=(rows, S)).astype(np.float32) + 0.5)
    return b


def penalty_oracle(E, R, batch, n, reg, flags, loss_scale, row0=0, grad_scale=1.0):
    """float64 penalty of the micro-batches in rows row0 .. row0 + n of `batch` (one per replica) at tables E [n, M, W],
    R: (penalty per replica, d penalty / d E, d penalty / d R).  Replica r's triple (j, q) has head E[r, head[r, j, q]],
    tail E[j, tail[j, r, q]] (it arrives through the exchange) and relation R[relation[r, j, q]]."""
    E = E.clone().requires_grad_(True)
    R = R.clone().requires_grad_(True)
    pens = []
    for r in range(n):
        h = E[r][batch["head"][row0 + r].long().reshape(-1)]
        t = torch.stack([E[j][batch["tail"][row0 + j][r].long()] for j in range(n)]).reshape(h.shape)
        rr = R[batch["relation"][row0 + r].long().reshape(-1)]
        w = batch["triple_weight"][row0 + r].double() if "triple_weight" in batch else torch.ones(1, dtype=torch.float64)
        c = loss_scale * w
        pens.append((c * (reg.entity_coef * (phi(h, reg.p, flags & 1) + phi(t, reg.p, flags & 1))
                          + reg.relation_coef * phi(rr, reg.p, flags & 2))).sum())
    (grad_scale * sum(pens)).backward()
    return torch.stack([x.detach() for x in pens]), E.grad, R.grad


def f16_ulp(x):
    """One unit in the last place of the fp16 numbers `x` (float64 tensor of stored fp16 values)."""
    return 2.0 ** (torch.floor(torch.log2(x.abs().clamp(min=2.0 ** -14))) - 10)


def assert_tables_differ_by(model_a, model_b, dE, dR, dtype, lr=1.0):
    """(E_A - E_B) / lr and (R_A - R_B) / lr equal the penalty's gradient: rtol 1e-4, atol 2e-5 (fp32 tables); for
    fp16 tables one fp16 ulp of the stored element more (both steps round once)."""
    for name, a, b, want in (("entity", model_a.score_fn.entity_embedding, model_b.score_fn.entity_embedding, dE),
                             ("relation", model_a.score_fn.relation_embedding, model_b.score_fn.relation_embedding, dR)):
        a, b = a.detach().cpu().double(), b.detach().cpu().double()
        got = (a - b) / lr
        tol = 2e-5 + 1e-4 * want.abs()
        if dtype == torch.float16:
            tol = tol + torch.maximum(f16_ulp(a), f16_ulp(b)) / lr
        bad = (got - want.reshape(got.shape)).abs() > tol
        assert bool(torch.isfinite(got).all()) and not bool(bad.any()), \
            f"{name}: {int(bad.sum())} off, worst {float(((got - want.reshape(got.shape)).abs() - tol).max()):.3e}"
        assert bool((want != 0).any())


LAYOUTS = {
    # name: scorer, n, per-triple negatives, scheme, dtype, extra
    "em1-complex-pertriple-tail": ("ComplEx", 1, True, "t", torch.float32, {}),
    "em1-complex-pertriple-separate": ("ComplEx", 1, True, "t", torch.float32, dict(pertriple_tail=False)),
    "em1-complex-pertriple-d50": ("ComplEx", 1, True, "t", torch.float32, dict(d=50)),
    "em1-transe-flat": ("TransE", 1, False, "t", torch.float32, {}),
    "em1-transe-flat-d50": ("TransE", 1, False, "h", torch.float32, dict(d=50)),
    "em1-rotate-ht-pertriple": ("RotatE", 1, True, "ht", torch.float32, {}),
    "em1-rotate-ht-flat": ("RotatE", 1, False, "ht", torch.float32, {}),
    "em1-pairre-flat": ("PairRE", 1, False, "t", torch.float32, {}),
    "em1-distmult-pertriple": ("DistMult", 1, True, "h", torch.float32, {}),
    "em2-complex-pertriple": ("ComplEx", 2, True, "t", torch.float32, {}),
    "em2-transe-flat": ("TransE", 2, False, "t", torch.float32, {}),
    "em3-complex-pertriple": ("ComplEx", 3, True, "h", torch.float32, {}),
    "em3-transe-flat": ("TransE", 3, False, "t", torch.float32, dict(d=50)),
    "sm2-complex-pertriple": ("ComplEx", 2, True, "t", torch.float32, dict(score_moving=True)),
    "sm2-transe-pertriple": ("TransE", 2, True, "t", torch.float32, dict(score_moving=True)),
    "em1-transe-flat-f16": ("TransE", 1, False, "t", torch.float16, {}),
    "em2-complex-pertriple-f16": ("ComplEx", 2, True, "t", torch.float16, {}),
    "em1-complex-weighted": ("ComplEx", 1, True, "t", torch.float32, dict(weight=True)),
    "em1-transe-loss-scale-64": ("TransE", 1, False, "t", torch.float32, dict(loss_scale=64.0)),
    "em1-transe-l1-coordinates": ("TransE", 1, False, "t", torch.float32, dict(p=1.0)),
    "em1-complex-sgdm": ("ComplEx", 1, True, "t", torch.float32, dict(opt="sgdm")),
    "em1-transe-flat-f16-sgdm": ("TransE", 1, False, "t", torch.float16, dict(opt="sgdm")),
    "em1-complex-dense-sgd": ("ComplEx", 1, True, "t", torch.float32, dict(opt="dense")),
}


def step_pair(dev, layout, options=None, micro=1):
    """Models A (coefficient 0) and B (0.05) of a layout stepped once on the same batch."""
    from besskge import runtime
    from besskge.regularizer import EmbeddingRegularizer

    scorer, n, per_triple, scheme, dtype, extra = LAYOUTS[layout]
    extra = dict(extra)
    p = extra.pop("p", 3.0)
    opt_name = extra.pop("opt", "sgd")
    tail_launch = extra.pop("pertriple_tail", True)
    weight = extra.pop("weight", False)
    batch = make_batch(n, per_triple, scheme, micro=micro, weight=weight)
    res = []
    for coef in (0.0, 0.05):
        reg = EmbeddingRegularizer(p, coef)
        model = make_model(dev, scorer, n, per_triple, scheme, dtype, reg, **extra)
        model.pertriple_tail = tail_launch
        E0 = model.score_fn.entity_embedding.detach().cpu().double()
        R0 = model.score_fn.relation_embedding.detach().cpu().double()
        # (replica_reduction: the relation table takes the sum over replicas whatever the accumulation's reduction)
        opt = dict(sgd=runtime.SGD(lr=1.0, replica_reduction="sum"),
                   sgdm=runtime.SGD(lr=1.0, momentum=0.9, replica_reduction="sum"),
                   dense=runtime.SGD(lr=1.0, dense=True, replica_reduction="sum"))[opt_name]
        runner = runtime.training_model(model, options or runtime.Options(), opt, device=dev)
        out = runner(**batch)
        torch.cuda.synchronize()
        res.append((model, {k: v.cpu() for k, v in out.items()}, reg))
    return res, batch, E0, R0, n, dtype, float(extra.get("loss_scale", 1.0))


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_training_step_adds_exactly_the_penalty_gradient(dev, layout):
    (a, b), batch, E0, R0, n, dtype, loss_scale = step_pair(dev, layout)
    (model_a, out_a, _), (model_b, out_b, reg) = a, b
    pens, dE, dR = penalty_oracle(E0, R0, batch, n, reg, model_b._regularizer_flags, loss_scale)
    assert_tables_differ_by(model_a, model_b, dE, dR, dtype)
    assert bool((out_a["regularization"] == 0).all())
    torch.testing.assert_close(out_b["regularization"].double(), pens, rtol=1e-5, atol=0)
    torch.testing.assert_close((out_b["loss"] - out_b["regularization"]).double(), out_a["loss"].double(), rtol=1e-6, atol=0)


def test_forward_reports_the_same_two_values(dev):
    """`forward_replicas` (no gradient): loss = fit + penalty and the penalty, through the value-only launch."""
    from besskge.regularizer import EmbeddingRegularizer

    outs = []
    batch = make_batch(1, True, "t")
    for reg in (None, EmbeddingRegularizer.n3(0.05)):
        model = make_model(dev, "ComplEx", 1, True, "t", torch.float32, reg)
        E0 = model.score_fn.entity_embedding.detach().cpu().double()
        R0 = model.score_fn.relation_embedding.detach().cpu().double()
        with torch.no_grad():
            outs.append(model.forward(**{k: v.to(dev) for k, v in batch.items()}))
    torch.cuda.synchronize()
    assert "regularization" not in outs[0]
    pens, _, _ = penalty_oracle(E0, R0, batch, 1, EmbeddingRegularizer.n3(0.05), 3, 1.0)
    torch.testing.assert_close(outs[1]["regularization"].cpu().double().reshape(1), pens, rtol=1e-5, atol=0)
    torch.testing.assert_close((outs[1]["loss"] - outs[1]["regularization"]).cpu(), outs[0]["loss"].cpu(), rtol=1e-6, atol=0)


# ------------------------------------------------------------------------------------ 3. gradient accumulation
@pytest.mark.parametrize("reduction", ["sum", "mean"])
@pytest.mark.parametrize("layout", ["em1-complex-pertriple-tail", "em2-transe-flat"])
def test_gradient_accumulation(dev, layout, reduction):
    """Two micro-batches, one update: the A / B difference is the sum (mean: half the sum) of both micro-batches'
    penalty gradients at the initial tables; the values handed back are the micro-batches' own, unscaled."""
    from besskge import runtime

    options = runtime.Options(gradient_accumulation=2, accumulation_reduction=reduction)
    (a, b), batch, E0, R0, n, dtype, _ = step_pair(dev, layout, options, micro=2)
    (model_a, out_a, _), (model_b, out_b, reg) = a, b
    scale = 0.5 if reduction == "mean" else 1.0
    dE = dR = 0
    for m in range(2):
        pens, gE, gR = penalty_oracle(E0, R0, batch, n, reg, model_b._regularizer_flags, 1.0, row0=m * n, grad_scale=scale)
        dE, dR = dE + gE, dR + gR
    assert_tables_differ_by(model_a, model_b, dE, dR, dtype)
    # (the runner hands back the last micro-batch's outputs)
    torch.testing.assert_close(out_b["regularization"].double(), pens, rtol=1e-5, atol=0)
    torch.testing.assert_close((out_b["loss"] - out_b["regularization"]).double(), out_a["loss"].double(), rtol=1e-6, atol=0)


# ------------------------------------------------------------------------------------------ 4. hipGraph replay
@pytest.mark.parametrize("layout", ["em1-complex-pertriple-tail", "em1-transe-flat-f16"])
def test_graph_replay_recomputes_the_penalty(dev, layout):
    from besskge import runtime
    from besskge.regularizer import EmbeddingRegularizer

    scorer, n, per_triple, scheme, dtype, _ = LAYOUTS[layout]
    batches = [make_batch(n, per_triple, scheme, seed=s) for s in range(3)]
    reg = EmbeddingRegularizer.n3(0.05)
    tables, pens, want = {}, {}, []
    for graphs in (False, True):
        model = make_model(dev, scorer, n, per_triple, scheme, dtype, reg)
        runner = runtime.training_model(model, runtime.Options(use_graphs=graphs, keep_graph=graphs),
                                        runtime.SGD(lr=0.05), device=dev)
        tables[graphs], pens[graphs] = [], []
        for b in batches:
            if graphs:
                E = model.score_fn.entity_embedding.detach().cpu().double()
                R = model.score_fn.relation_embedding.detach().cpu().double()
                want.append(penalty_oracle(E, R, b, n, reg, model._regularizer_flags, 1.0)[0])
            out = runner(**b)
            torch.cuda.synchronize()
            pens[graphs].append(out["regularization"].cpu().double())
            tables[graphs].append((model.score_fn.entity_embedding.detach().cpu().float(),
                                   model.score_fn.relation_embedding.detach().cpu().float()))
        if graphs:
            (counts,) = runner.graph_node_counts().values()
            assert counts.get("kernel", 0) > 0 and "memset" not in counts, counts
    for (e0, r0), (e1, r1) in zip(tables[False], tables[True]):
        # (what the eager / recorded comparisons of these routes use: fp32 atomics differ in their last bits; an fp16
        # element may round to the neighbouring value)
        tol = dict(rtol=1e-4, atol=2e-5) if dtype == torch.float32 else dict(rtol=2e-3, atol=1e-4)
        torch.testing.assert_close(e1, e0, **tol)
        torch.testing.assert_close(r1, r0, **tol)
    for call in range(3):  # recomputed at every replay from the tables as they are, not frozen at capture
        torch.testing.assert_close(pens[True][call], want[call], rtol=1e-5, atol=0)
    assert float(pens[True][1]) != float(pens[True][0]) and float(pens[True][2]) != float(pens[True][1])


# ------------------------------------------------------------------------------- 5. no regulariser, no change
def launches(dev, build, batch, opt):
    """Entry points one training step of `build()` issues, in order (the launch path's own recording hook)."""
    from besskge import _native as nat
    from besskge import runtime

    model = build()
    runner = runtime.training_model(model, runtime.Options(), opt, device=dev)
    runner(**batch)  # (static maps, counters: a first step may differ)
    nat.start_kernel_timing(list(nat.SIGNATURES))
    try:
        runner(**batch)
        names = [entry[0] for entry in nat.kernel_timing_log()]
    finally:
        nat.stop_kernel_timing()
    return names


@pytest.mark.parametrize("layout", ["em1-complex-pertriple-tail", "em1-transe-flat", "em1-rotate-ht-pertriple",
                                    "em1-pairre-flat", "em2-complex-pertriple", "sm2-transe-pertriple",
                                    "em1-transe-flat-f16"])
def test_without_a_regulariser_the_step_launches_what_it_did(dev, layout):
    from besskge import runtime
    from besskge.bess import EmbeddingMovingBessKGE, ScoreMovingBessKGE
    from besskge.regularizer import EmbeddingRegularizer

    scorer, n, per_triple, scheme, dtype, extra = LAYOUTS[layout]
    batch = make_batch(n, per_triple, scheme)
    opt = runtime.SGD(lr=0.01)

    def positional():  # as a model was built before the keyword existed
        m = make_model(dev, scorer, n, per_triple, scheme, dtype, None, **extra)
        cls = ScoreMovingBessKGE if extra.get("score_moving") else EmbeddingMovingBessKGE
        return cls(m.negative_sampler, m.score_fn, m.loss_fn, None, False, False)

    plain = launches(dev, lambda: make_model(dev, scorer, n, per_triple, scheme, dtype, None, **extra), batch, opt)
    assert "bess_regularize_triples" not in plain
    assert plain == launches(dev, positional, batch, opt)
    with_reg = launches(dev, lambda: make_model(dev, scorer, n, per_triple, scheme, dtype, EmbeddingRegularizer.n3(0.01),
                                                **extra), batch, opt)
    assert "bess_direct_update" not in plain  # (that route: the test below)
    assert with_reg.count("bess_regularize_triples") == n  # one per replica step
    assert [x for x in with_reg if x != "bess_regularize_triples"] == plain


def test_a_regulariser_replaces_the_direct_update_by_the_coalescing_path(dev):
    """The C4 notebook micro-batch (TransE fp16, S = 512, K = 32, augmentation, sampled softmax, SGD) takes the direct
    update, which has no dh / dt: with a regulariser the step launches what it launches with
    `direct_update_max_bytes = 0`, plus the regulariser's one launch."""
    from besskge import runtime
    from besskge.bess import EmbeddingMovingBessKGE
    from besskge.loss import SampledSoftmaxCrossEntropyLoss
    from besskge.negative_sampler import RandomShardedNegativeSampler
    from besskge.regularizer import EmbeddingRegularizer
    from besskge.scoring import TransE
    from besskge.sharding import Sharding

    S, K, M = 512, 32, 20_000
    sharding = Sharding.create(M, 1, seed=0)
    rng = np.random.default_rng(0)
    batch = dict(head=rng.integers(M, size=(1, 1, S)), relation=rng.integers(50, size=(1, 1, S)),
                 tail=rng.integers(M, size=(1, 1, S)), negative=rng.integers(M, size=(1, 1, 1, K)))
    batch = {k: torch.from_numpy(v.astype(np.int32)) for k, v in batch.items()}

    def build(reg=None, direct=True):
        def make():
            torch.manual_seed(0)
            fn = TransE(True, 1, sharding, 50, 256, device=dev, dtype=torch.float16)
            ns = RandomShardedNegativeSampler(K, sharding, 0, "t", local_sampling=False, flat_negative_format=True)
            m = EmbeddingMovingBessKGE(negative_sampler=ns, score_fn=fn, augment_negative=True,
                                       loss_fn=SampledSoftmaxCrossEntropyLoss(n_entity=M), regularizer=reg)
            if not direct:
                m.direct_update_max_bytes = 0
            return m
        return make

    opt = runtime.SGD(lr=1e-3)
    plain = launches(dev, build(), batch, opt)
    assert "bess_direct_update" in plain and "bess_regularize_triples" not in plain
    coalescing = launches(dev, build(direct=False), batch, opt)
    assert "bess_direct_update" not in coalescing
    with_reg = launches(dev, build(EmbeddingRegularizer.n3(0.01)), batch, opt)
    assert with_reg.count("bess_regularize_triples") == 1
    assert [x for x in with_reg if x != "bess_regularize_triples"] == coalescing


# --------------------------------------------------------------------------------- 6. refusals at the model level
def test_model_level_refusals(dev):
    from besskge.bess import EmbeddingMovingBessKGE
    from besskge.regularizer import EmbeddingRegularizer

    m = make_model(dev, "TransE", 1, False, "t", torch.float32, None)
    with pytest.raises(ValueError, match="loss_fn"):
        EmbeddingMovingBessKGE(negative_sampler=m.negative_sampler, score_fn=m.score_fn, return_scores=True,
                               regularizer=EmbeddingRegularizer.n3(0.1))
    with pytest.raises(ValueError, match="TransE"):
        make_model(dev, "TransE", 1, False, "t", torch.float32, EmbeddingRegularizer(3.0, 0.1, complex_modulus=True))


# ------------------------------------------------------------------------------------------------ 7. the example
def test_example_with_n3():
    cmd = [sys.executable, os.path.join(REPO, "examples", "train_and_evaluate.py"), "--scorer", "ComplEx",
           "--regularizer", "n3", "--reg-coef", "1e-3", "--steps", "30"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    losses = [float(line.split("loss")[1]) for line in res.stdout.splitlines() if line.startswith("step")]
    assert losses and all(math.isfinite(x) for x in losses), res.stdout[-2000:]
