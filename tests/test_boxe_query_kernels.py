"""`bess_boxe_query_fwd / _bwd` (csrc/boxe_query.hip) against the scorer's own `_query_torch` / `_triple_torch` and
autograd in float64 on the CPU (fp16 tables: their values upcast), with the same functions in float32 as the yardstick
of `check` (tests/test_pertriple_kernels.py: the project's bound, or 4 x the restatement's error where that is itself
outside it).

1200 triples over 6 relations: relation 0 has 1000 of them (cut into shares), relations 1-3 share 199, relation 4 has
one, relation 5 none (its d_rel row must stay what it was).  Every triple reads a row of its own through a permutation
index, so every element is free to move: an element whose distance is within MARGIN of its half width or of zero is
moved (`settle`), and the decisions `dist <= half` are then asserted equal in float64 and float32.  24 triples of
relation 0 are planted a quarter of the half width from the centre in every dimension (exactly at the centre the sign
of `point - centre`, which the p = 1 gradient carries, is rounding): the slots that are entirely inside.  Widths:
|w| >= 0.05 with both signs, but a zero column in one box of relations 1 and 2 and -3e-7 (below eps) in relation 3;
sizes +-(0.2 .. 0.8) with both signs in every row."""

import functools

import pytest
import torch

from besskge import _native as nat
from besskge.scoring import BoxE
from besskge.sharding import Sharding

from test_affine_boxe_row_classes import BOXE_SETTINGS
from test_pertriple_kernels import MEASURED, check  # noqa: F401  (MEASURED: the errors DESIGN.md quotes)

pytestmark = pytest.mark.gpu
F32, F16 = torch.float32, torch.float16
S, N_REL, N_PLANT, MARGIN = 1200, 6, 24, 1e-4
CLASSES = [(F32, 6), (F16, 40), (F32, 64), (F32, 512), (F16, 128)]
SIDES = {"t": nat.CORRUPT_TAIL, "h": nat.CORRUPT_HEAD}
CASES = [(tanh, per_dim, p, side, dtype, d) for tanh, per_dim, p, _ in BOXE_SETTINGS for side in SIDES
         for dtype, d in CLASSES] + [(True, True, 3, "t", F32, 64)]


def slots(fn, side, ent, oth, rel, ridx):
    """(point - centre, half width) [S, 2 slots, d] of the triples, from the scorer's own query"""
    d = fn.embedding_size
    q = fn._query_torch(SIDES[side], ent, rel, ridx).view(-1, 2, 3, d)
    x = oth.view(-1, 2, d) + q[:, :, 0]
    return (torch.tanh(x) if fn.apply_tanh else x) - q[:, :, 1], q[:, :, 2]


def settle(fn, side, ent, oth, rel, ridx, dtype):
    """move the elements of `oth` that sit within MARGIN of a kink; False if some are left after 20 rounds"""
    for _ in range(20):
        diff, half = slots(fn, side, ent.double(), oth.double(), rel.double(), ridx)
        near = ((diff.abs() - half).abs() < MARGIN) | (diff.abs() < MARGIN)
        if not near.any():
            return True
        oth.view(-1, 2, fn.embedding_size)[near] += torch.tensor(0.03, dtype=dtype)
    return False


@functools.lru_cache(maxsize=None)
def case(tanh, per_dim, p, side, dtype, d):
    fn = BoxE(False, p, Sharding.create(8, 1, seed=0), N_REL, d, apply_tanh=tanh, dist_func_per_dim=per_dim)
    gen = torch.Generator().manual_seed(1000 * d + 10 * p + 2 * tanh + per_dim)
    rel = torch.randn(N_REL, 4 * d + 2, generator=gen) * 0.4
    w = rel[:, 2 * d: 4 * d]
    w.copy_(torch.sign(w) * (w.abs() + 0.05))
    w[1, 1], w[2, d + 2 % d], w[3, 3 % d] = 0.0, 0.0, -3e-7
    rel[:, 4 * d:] = torch.tensor([[0.5, -0.7], [-0.3, 0.4], [0.8, -0.2], [-0.6, 0.3], [0.2, -0.5], [-0.4, 0.6]])
    rel = rel.to(dtype)
    ridx = torch.cat([torch.zeros(1000), torch.randint(1, 4, (199,), generator=gen), torch.full((1,), 4)])
    ridx = ridx[torch.randperm(S, generator=gen)].to(torch.int32)
    ent, oth = ((torch.randn(S, 2 * d, generator=gen) * 0.4).to(dtype) for _ in range(2))
    plant = torch.nonzero(ridx == 0).reshape(-1)[:N_PLANT]
    diff, half = slots(fn, side, ent[plant].double(), torch.zeros(N_PLANT, 2 * d, dtype=torch.float64), rel.double(),
                       ridx[plant])  # with other = 0: point = the kept part, so centre = point - diff
    centre = (torch.tanh(ent[plant].double().view(-1, 2, d).flip(1)) if tanh else ent[plant].double().view(-1, 2, d).flip(1)) - diff
    target = centre + 0.25 * half * torch.where(torch.rand(half.shape, generator=gen) < 0.5, -1.0, 1.0)
    target = torch.atanh(target) if tanh else target
    oth[plant] = (target - ent[plant].double().view(-1, 2, d).flip(1)).flatten(1).to(dtype)
    assert settle(fn, side, ent, oth, rel, ridx, dtype), "elements stay within the margin of a kink"
    # the decisions, on the float64 reference, and their float32 twins
    d64, h64 = slots(fn, side, ent.double(), oth.double(), rel.double(), ridx)
    d32, h32 = slots(fn, side, ent.float(), oth.float(), rel.float(), ridx)
    inside = d64.abs() <= h64
    assert torch.equal(inside, d32.abs() <= h32)
    assert 0.1 <= float(inside.double().mean()) <= 0.9, float(inside.double().mean())
    assert per_dim or int(inside.all(-1).sum()) >= 16
    raw = rel.double()[:, 2 * d: 4 * d]
    assert bool((raw > 0).any() and (raw < 0).any() and (raw.abs() < fn.eps).any())
    assert torch.equal(raw.abs() > fn.eps, rel.float()[:, 2 * d: 4 * d].abs() > fn.eps)
    assert bool((rel[:, 4 * d:] > 0).any(1).all() and (rel[:, 4 * d:] < 0).any(1).all())
    perm_e, perm_o = (torch.randperm(S, generator=gen).to(torch.int32) for _ in range(2))
    tab_e, tab_o = torch.empty_like(ent), torch.empty_like(oth)
    tab_e[perm_e.long()], tab_o[perm_o.long()] = ent, oth
    dq, dpos, d_rel0 = torch.randn(S, 6 * d, generator=gen), torch.randn(S, generator=gen), torch.randn(N_REL, 4 * d + 2, generator=gen)
    refs = [reference(fn, side, ent, oth, rel, ridx, dq, dpos, d_rel0, ft) for ft in (torch.float64, torch.float32)]
    return fn, (tab_e, perm_e, tab_o, perm_o, rel, ridx, dq, dpos, d_rel0), refs


def reference(fn, side, ent, oth, rel, ridx, dq, dpos, d_rel0, ft):
    """q, pos and the gradients of the three calls the routes make (query, triple, both) evaluated in `ft`"""
    ent, oth, rel = (t.to(ft).requires_grad_() for t in (ent, oth, rel))
    q = fn._query_torch(SIDES[side], ent, rel, ridx)
    pos = fn._triple_torch(*((ent, rel, ridx, oth) if side == "t" else (oth, rel, ridx, ent)))
    lq, lp = (q * dq.to(ft)).sum(), (pos * dpos.to(ft)).sum()
    out = {"q": q.detach(), "pos": pos.detach()}
    for name, loss in (("query", lq), ("triple", lp), ("both", lq + lp)):
        ge, go, gr = torch.autograd.grad(loss, [ent, oth, rel], retain_graph=True, allow_unused=True)
        out[name] = (ge, go, d_rel0.to(ft) + gr)
    return out


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda", 0)


@pytest.mark.parametrize("tanh, per_dim, p, side, dtype, d", CASES,
                         ids=lambda v: {F32: "f32", F16: "f16"}.get(v, str(v)))
def test_forward_and_backward_equal_float64(dev, tanh, per_dim, p, side, dtype, d):
    fn, inputs, (r64, r32) = case(tanh, per_dim, p, side, dtype, d)
    tab_e, perm_e, tab_o, perm_o, rel, ridx, dq, dpos, d_rel0 = (t.to(dev) for t in inputs)
    desc = nat.make_desc(nat.BOXE, p, tab_e, 4 * d + 2)
    desc.reserved[0] = int(tanh) | (int(per_dim) << 1)
    ent, oth = nat.RowSource(tab_e, perm_e), nat.RowSource(tab_o, perm_o)
    regime = f"{'f32' if dtype == F32 else 'f16'}-{d}"

    def ok(quantity, got, key, part=None):
        w64, w32 = (r64[key], r32[key]) if part is None else (r64[key][part], r32[key][part])
        check("boxe_query", quantity, regime, f"{quantity} {key}", got, w64, w32)

    q, pos = nat.boxe_query_fwd(desc, SIDES[side], fn.eps, ent, rel, ridx, other=oth)
    ok("q", q, "q")
    ok("pos", pos, "pos")
    assert torch.equal(nat.boxe_query_fwd(desc, SIDES[side], fn.eps, ent, rel, ridx)[0], q)  # without the other rows
    assert torch.equal(nat.boxe_query_fwd(desc, SIDES[side], fn.eps, ent, rel, ridx, other=oth, want_query=False)[1], pos)
    for key, g_q, g_pos in (("query", dq, None), ("triple", None, dpos), ("both", dq, dpos)):
        def run():
            d_rel = d_rel0.clone()  # non-zero on entry: the call adds
            de, do = nat.boxe_query_bwd(desc, SIDES[side], fn.eps, ent, rel, ridx, g_q, d_rel,
                                        other=None if g_pos is None else oth, d_pos=g_pos)
            return de, do, d_rel
        de, do, d_rel = run()
        ok("d_ent", de, key, 0)
        if g_pos is not None:
            ok("d_other", do, key, 1)
        ok("d_rel", d_rel, key, 2)
        assert torch.equal(d_rel[5], d_rel0[5])  # the relation no triple names
        assert torch.equal(run()[2], d_rel)  # two calls: the same bits
