"""HAKE without a device: descriptor checks, the query width, the constructor, and the [U | R | Q_p] algebra of the
query against the triple score, in float64."""
import ctypes

import pytest
import torch

from besskge import _native as nat
from besskge import scoring
from besskge.sharding import Sharding

D, N_REL, N_ENT = 6, 4, 20


def check_desc(width, rel_width):
    """(return code, message) of a call that stops after check_desc (no queries: nothing is launched)"""
    lib = nat.load()
    d = nat.ModelDesc()
    d.scorer, d.norm_p, d.dtype, d.width, d.rel_width = nat.HAKE, 2, nat.F32, width, rel_width
    rc = lib.bess_neg_score_pertriple_fwd(ctypes.byref(d), 0, 0, 0, 0, 0, 0, 0, 0)
    buf = ctypes.create_string_buffer(256)
    lib.bess_last_error(buf, 256)
    return rc, buf.value.decode()


@pytest.mark.parametrize("width,rel_width,ok", [(12, 18, True), (11, 18, False), (12, 12, False), (12, 17, False)])
def test_check_desc(width, rel_width, ok):
    rc, msg = check_desc(width, rel_width)
    assert (rc == 0) == ok and (ok or "HAKE" in msg)


def test_query_width():
    d = nat.ModelDesc()
    d.scorer, d.width = nat.HAKE, 2 * D
    assert nat.query_width(d) == 3 * D


def make(**kw):
    torch.manual_seed(0)
    return scoring.HAKE(True, Sharding.create(N_ENT, 1, seed=0), N_REL, D, **kw)


def test_constructor_and_descriptor():
    with pytest.raises(ValueError, match="modulus_weight"):
        make(modulus_weight=-1.0)
    fn = make(phase_weight=0.25, phase_scale=2.0)
    assert fn.entity_embedding.shape[-1] == 2 * D and fn.relation_embedding.shape[-1] == 3 * D
    d = fn.kernel_desc()
    assert (d.scorer, d.norm_p, d.width, d.rel_width, d.reserved[0]) == (nat.HAKE, 2, 2 * D, 3 * D, 0)
    assert [torch.tensor(int(b), dtype=torch.int32).view(torch.float32).item() for b in d.reserved[1:3]] == [0.25, 2.0]
    fn.fp32_math = True
    assert fn.kernel_desc().reserved[0] == nat.FLAG_FP32_MATH
    # the weights live in the buffers: a loaded state dict changes what the kernels and the torch hooks use
    fn.load_state_dict(make(phase_weight=0.75).state_dict())
    assert fn._weights == (1.0, 0.75, 1.0)
    with pytest.raises(ValueError, match="embedding_size"):
        scoring.HAKE(True, Sharding.create(N_ENT, 1, seed=0), N_REL, 258)


@pytest.mark.parametrize("side", [nat.CORRUPT_HEAD, nat.CORRUPT_TAIL])
def test_query_algebra(side):
    """-(||U c_m + R|| + l_p sum |sin((Q_p - s c_p) / 2)|) of the query == the triple's score, float64 throughout"""
    fn = make(modulus_weight=0.75, phase_weight=0.25, phase_scale=1.5)  # (the buffers are float32: exact values)
    gen = torch.Generator().manual_seed(1)
    rel = torch.randn(N_REL, 3 * D, generator=gen, dtype=torch.float64) * 2  # (biases on both sides of their clamps)
    h, t = (torch.randn(9, 2 * D, generator=gen, dtype=torch.float64) for _ in range(2))
    rid = torch.randint(N_REL, (9,), generator=gen)
    kept, cand = (h, t) if side == nat.CORRUPT_TAIL else (t, h)
    q = fn._query_torch(side, kept, rel, rid)
    assert q.dtype == torch.float64 and q.shape == (9, 3 * D)
    u, r, qp = q.chunk(3, dim=-1)
    cp, cm = cand.chunk(2, dim=-1)
    got = -(torch.norm(u * cm + r, dim=-1) + 0.25 * torch.sin((qp - 1.5 * cp) / 2).abs().sum(-1))
    torch.testing.assert_close(got, fn._triple_torch(h, rel, rid, t), rtol=1e-13, atol=1e-13)
