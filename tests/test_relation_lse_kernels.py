"""`bess_relation_lse_fwd / _bwd` (csrc/relation_lse.hip) against float64 + autograd on the CPU.

Bounds (u = 2^-24; "abs" = the same float64 computation on the operands' absolute values).
  s     a score is W exact products added by one chain of fp32 fused multiply-adds, its left operand g(h, t) rounded
        at most twice (ComplEx: a product and a fused multiply-add): e_s = (W + 2) u s_abs.
  lse   log-sum-exp moves by at most the largest error of its scores; the sum l of a row goes through
        depth = ceil(n_rel / 64) + 6 merges (a lane's tiles, five lane exchanges, the two waves), each three roundings,
        and the result is rounded once: e_lse = max_r e_s + (3 depth + 4 LSE_EXP_LOG_MEASURED) u (1 + |lse|).  What
        the device's exp / log add cannot be derived: every case prints how far |lse - want| goes beyond the derived
        part, in units of u (1 + |lse|).  On the MI355X it never did (largest value over all cases: -24, i.e. 24
        units below it), so LSE_EXP_LOG_MEASURED is held at one unit - the 1 ulp of v_exp_f32 / v_log_f32 - and 4x
        covers another seed.
  P     P = coef (exp(s - lse) - [r = r_i]):  e_P = |coef| p (e_s + e_lse + 4 LSE_EXP_LOG_MEASURED u) + 2 u |P|.
  d_g   n_rel products:  e_g = e_P |rel| + (n_rel + 1) u |P| |rel|;  d_head, d_tail chain it with a row (<= 3
        roundings) and are added to what the buffer held (1):  g_abs(e_g, |t|) + 3 u g_abs(dg_abs, |t|) + u (|prior| + |sum|).
  d_rel S products in at most 8 shares merged in order, g rounded twice, added to the prior content:
        e_P^T g_abs + (S + 12) u |P|^T g_abs + u (|prior| + |sum|)."""

import functools

import pytest
import torch

from besskge import _native as nat
from besskge._native import RowSource

U = 2.0 ** -24
LSE_EXP_LOG_MEASURED = 1.0  # in units of u (1 + |lse|); see the module docstring and DESIGN section 36
SHAPES = [(1, 4, 1), (33, 6, 3), (65, 36, 64), (70, 72, 65), (130, 264, 130),
          (5, 520, 3)]  # 520: the first widths past the resident g image (512) and past one backward window
CASES = [(s, "plain") for s in SHAPES] + [((70, 72, 65), m) for m in ("scaled", "pad4", "pad3")]
N_ENT = 23


def g64(h, t, cplx, absolute=False):
    if not cplx:
        return h * t
    d = h.shape[1] // 2
    h1, h2, t1, t2 = h[:, :d], h[:, d:], t[:, :d], t[:, d:]
    return torch.cat([h1 * t1 + h2 * t2, h1 * t2 + h2 * t1 if absolute else h1 * t2 - h2 * t1], dim=1)


@functools.lru_cache(maxsize=None)
def case(cplx, half, S, W, n_rel, mode):
    gen = torch.Generator().manual_seed(7 * S + W + n_rel + cplx)
    dt = torch.float16 if half else torch.float32
    table, tails, rel = (torch.randn(s, generator=gen).to(dt) for s in ((N_ENT, W), (S, W), (n_rel, W)))
    hidx = torch.randint(0, N_ENT, (S,), generator=gen).to(torch.int32)  # (S > N_ENT: rows repeat)
    ridx = torch.randint(0, n_rel, (S,), generator=gen).to(torch.int32)
    ridx[-1] = n_rel - 1
    coef = torch.rand(S, generator=gen) + 0.5
    coef[::3] = 0.0
    prior = [torch.randn(s, generator=gen) for s in ((S, W), (S, W), (n_rel, W))]
    if mode == "scaled":  # scores over about +-200: the running maximum moves
        s0 = g64(table[hidx.long()].double(), tails.double(), cplx) @ rel.double().T
        rel = (rel.double() * 200.0 / s0.abs().max()).to(dt)
    h, t, r = (x.double().requires_grad_() for x in (table[hidx.long()], tails, rel))
    s = g64(h, t, cplx) @ r.T
    lse = torch.logsumexp(s, dim=1)
    c64 = coef.double()
    grads = torch.autograd.grad((c64 * (lse - s[torch.arange(S), ridx.long()])).sum(), [h, t, r])
    want = [lse.detach()] + [p.double() + g for p, g in zip(prior, grads)]
    # the bounds of the module docstring
    h, t, r, s = h.detach(), t.detach(), r.detach(), s.detach()
    g_abs = g64(h.abs(), t.abs(), cplx, True)
    e_s = (W + 2) * U * (g_abs @ r.abs().T)
    k = 4 * LSE_EXP_LOG_MEASURED * U
    e_lse = e_s.max(dim=1).values + (3 * ((n_rel + 63) // 64 + 6) * U + k) * (1 + lse.detach().abs())
    p = torch.exp(s - lse.detach()[:, None])
    P_abs = c64[:, None] * (p + torch.nn.functional.one_hot(ridx.long(), n_rel))
    e_P = c64[:, None] * p * (e_s + e_lse[:, None] + k) + 2 * U * P_abs
    e_g, dg_abs = e_P @ r.abs() + (n_rel + 1) * U * (P_abs @ r.abs()), P_abs @ r.abs()
    bounds = [e_lse]
    for other, pr, w in ((t, prior[0], want[1]), (h, prior[1], want[2])):
        bounds.append(g64(e_g, other.abs(), cplx, True) + 3 * U * g64(dg_abs, other.abs(), cplx, True)
                      + U * (pr.abs() + w.abs()))
    bounds.append(e_P.T @ g_abs + (S + 12) * U * (P_abs.T @ g_abs) + U * (prior[2].abs() + want[3].abs()))
    return (table, hidx, tails, rel, ridx, coef, prior), want, bounds


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda", 0)


def padded(t, pad):  # `t` as a view of the leading columns of a buffer `pad` columns wider (filled with NaN)
    if not pad:
        return t.clone()
    buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=t.dtype, device=t.device)
    buf[:, : t.shape[1]] = t
    return buf[:, : t.shape[1]]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,mode", CASES)
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("cplx", [False, True])
def test_relation_softmax_against_float64(dev, cplx, half, shape, mode):
    (S, W, n_rel), pad = shape, int(mode[3:]) if mode.startswith("pad") else 0
    ops, want, bounds = case(cplx, half, S, W, n_rel, mode)
    *on_dev, prior = ops
    table, hidx, tails, rel, ridx, coef = (x.to(dev) for x in on_dev)
    table, tails, rel = (padded(x, pad) for x in (table, tails, rel))
    desc = nat.make_desc(nat.COMPLEX if cplx else nat.DISTMULT, 0, table, W)
    head, tail = RowSource(table, hidx), RowSource(tails, None)

    def run():
        lse = nat.relation_lse_fwd(desc, head, tail, rel)
        grads = [padded(p.to(dev), pad) for p in prior]
        nat.relation_lse_bwd(desc, head, tail, rel, ridx, lse, coef, *grads)
        return [lse, *grads]

    got, again = run(), run()
    for name, g, g2, w, b in zip(("lse", "d_head", "d_tail", "d_rel"), got, again, want, bounds):
        err = (g.double().cpu() - w).abs()
        print(f"{name} {shape} {mode}: largest error {float(err.max()):.3e}, error / bound {float((err / b.clamp_min(1e-300)).max()):.3e}"
              + (f", beyond the derived part, in u (1 + |lse|): {float(((err - b) / (U * (1 + w.abs()))).max() + 4 * LSE_EXP_LOG_MEASURED):.2f}"
                 if name == "lse" else ""))
        assert bool((err <= b).all()), name
        assert torch.equal(g, g2), f"{name} differs between two runs"
    # no term, no change - exactly: rows with coef == 0, and every relation when no row has a term
    off = (coef == 0).cpu()
    for g, p in zip(got[1:3], prior[:2]):
        assert torch.equal(g.cpu()[off], p[off])
    if bool(off.all()):
        assert torch.equal(got[3].cpu(), prior[2])
