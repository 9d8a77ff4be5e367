"""`bess_conve_query_fwd / _bwd` and `bess_conve_stats_fwd / _bwd` (csrc/conve.hip) against float64 `conv2d` +
autograd on the CPU.

The ReLU kink.  The backward is discontinuous at z = 0, so the inputs are built for fp32 to compute z exactly and never
get zero: entries of x and K are integers / 16 (K's non-zero), a_c is 0.5, 1 or 2, b_c an odd multiple of 2^-10, m is 0 or 2 (or
absent).  z is then an odd multiple of 2^-10 in any order of summation (asserted on the float64 reference), and every
ReLU decision equals the reference's; dy and Wfc are `randn`.

Bounds, u = 2^-24: |got - want| <= n u sum |terms|, n the number of roundings a term can meet on its way into the
output, the sum of absolute terms being the same float64 graph (the reference's ReLU decisions kept as a gate) on the
operands' absolute values.  KK = Cin kh kw, n_ct = ceil(Ho Wo / 128); forming an element of A or of the masked
gradient costs KK + 2 roundings (the conv's chain, the affine, the mask).

  y        F + KK + 2: the MFMA chain over f.
  d_Wfc    S + KK + 2: the MFMA chain over the rows.
  d_x      d + KK + Cout n_ct + 3: the MFMA chain over d, the mask (the recomputed conv enters only through the ReLU
           decision, which is exact), a gather of <= KK taps per (channel, block of 128 output pixels), the product
           with a_c, one addition per (channel, block) into the resident image.
  d_K, d_a, d_b
           d + KK + 16 n_ct + ceil(S / 32) + 12: the MFMA chain, the mask (and conv), 16 columns per thread and
           block, the wave's butterfly (6), four waves (3), the tile-ordered merge, the product with a_c.

Statistics (the terms of M2 and of its gradients are those of sum (|conv| + |mean|)^2: the subtraction's operands):
  mean     KK + ceil(8 Ho Wo / 256) + ceil(ceil(S / 8) / 64) + 17: conv, a thread's chain over its elements of 8 rows,
           butterfly and waves (9), the strided merge and its butterfly (6), 1 / N and the product with it (2).
  M2       2 (the mean's n + 1) + the same reduction depth: each factor of a square carries conv's and the mean's error.
  d_x      3 KK + Cout + 6: d_conv (conv, the mean, two products), KK taps per channel, Cout additions.
  d_K      2 KK + ceil(8 Ho Wo / 256) + ceil(S / 8) + 15: d_conv, the thread's chain, butterfly, waves, the merge."""

import functools
import math

import pytest
import torch

from besskge import _native as nat
from besskge import ops

from test_one_vs_all import dev  # noqa: F401

U = 2.0 ** -24
# (S, Cin, H2, W, Cout, kh, kw, d, mask, padded)
SHAPES = [
    (1, 1, 4, 3, 1, 3, 3, 1, False, False),        # minimal
    (33, 1, 8, 5, 3, 3, 3, 20, True, False),       # partial tiles everywhere
    (70, 2, 6, 6, 5, 2, 3, 36, True, False),       # two input channels, non-square filter
    (257, 1, 4, 8, 4, 3, 3, 72, False, False),     # many row tiles
    (40, 1, 2, 130, 2, 1, 1, 264, True, False),    # 1 x 1 filter, d above 256, wide image
    (130, 1, 20, 20, 32, 3, 3, 200, True, False),  # the paper's
    (3, 1, 2, 249, 1, 1, 1, 4, False, False),      # 163,540 of 163,840 bytes of LDS: the largest two-row image
    (70, 2, 6, 6, 5, 2, 3, 36, True, True),        # padded leading dimensions, odd pointers: the scalar-load kernels
]
PAST_LIMIT = (3, 1, 2, 250, 1, 1, 1, 4)


def query64(x, K, a, b, m, Wfc, dy, gate=None):
    """(y, d_Wfc, d_x, d_K, d_a, d_b, z) in float64; `gate` replaces the ReLU's own decisions"""
    leaves = [t.double().requires_grad_() for t in (Wfc, x, K, a, b)]
    w, x, K, a, b = leaves
    z = a.view(1, -1, 1, 1) * torch.nn.functional.conv2d(x, K) + b.view(1, -1, 1, 1)
    act = z * ((z > 0) if gate is None else gate)
    if m is not None:
        act = act * m.double()[:, :, None, None]
    y = act.flatten(1) @ w.T
    return [y.detach(), *torch.autograd.grad(y, leaves, dy.double()), z.detach()]


def stats64(x, K, d_mean, d_M2, sign=1.0):
    """(mean, M2, d_x, d_K) in float64; sign = -1 on absolute operands: the subtraction's terms add"""
    x, K = (t.double().requires_grad_() for t in (x, K))
    conv = torch.nn.functional.conv2d(x, K)
    mean = conv.mean(dim=(0, 2, 3))
    M2 = ((conv - sign * mean.view(1, -1, 1, 1)) ** 2).sum(dim=(0, 2, 3))
    return [mean.detach(), M2.detach(), *torch.autograd.grad([mean, M2], [x, K], [d_mean.double(), d_M2.double()])]


@functools.lru_cache(maxsize=None)
def case(S, Cin, H2, W, Cout, kh, kw, d, mask):
    gen = torch.Generator().manual_seed(S + 10 * H2 + 100 * W + d)
    Ho, Wo, KK = H2 - kh + 1, W - kw + 1, Cin * kh * kw
    F = Cout * Ho * Wo
    x = torch.randint(-8, 9, (S, Cin, H2, W), generator=gen) / 16.0
    K = torch.randint(1, 9, (Cout, Cin, kh, kw), generator=gen) * (2 * torch.randint(2, (Cout, Cin, kh, kw), generator=gen) - 1) / 16.0
    a = torch.tensor([0.5, 1.0, 2.0])[torch.randint(3, (Cout,), generator=gen)]
    b = (2 * torch.randint(-64, 64, (Cout,), generator=gen) + 1) / 1024.0
    m = 2.0 * torch.randint(2, (S, Cout), generator=gen) if mask else None
    Wfc, dy = torch.randn(d, F, generator=gen), torch.randn(S, d, generator=gen)
    d_mean, d_M2 = torch.randn(Cout, generator=gen), torch.randn(Cout, generator=gen)
    want = query64(x, K, a, b, m, Wfc, dy)
    z = want.pop()
    assert bool(((z * 1024) % 2 == 1).all()), "z must be an odd multiple of 2^-10"
    terms = query64(x.abs(), K.abs(), a.abs(), b.abs(), m, Wfc.abs(), dy.abs(), gate=z > 0)[:-1]
    n_ct, tiles = math.ceil(Ho * Wo / 128), math.ceil(S / 32)
    small = d + KK + 16 * n_ct + tiles + 12
    n = [F + KK + 2, S + KK + 2, d + KK + Cout * n_ct + 3, small, small, small]
    chain, n_mean = math.ceil(8 * Ho * Wo / 256), KK + math.ceil(8 * Ho * Wo / 256) + math.ceil(math.ceil(S / 8) / 64) + 17
    n_st = [n_mean, 2 * (n_mean + 1) + n_mean - KK, 3 * KK + Cout + 6, 2 * KK + chain + math.ceil(S / 8) + 15]
    st_terms = stats64(x.abs(), K.abs(), d_mean.abs(), d_M2.abs(), sign=-1.0)
    return ((x, K, a, b, m, Wfc, dy), want, [k * U * t for k, t in zip(n, terms)],
            (d_mean, d_M2), stats64(x, K, d_mean, d_M2), [k * U * t for k, t in zip(n_st, st_terms)])


def padded(t, dev):
    """`t` on the device as a view of a wider buffer, one float past its 16-byte aligned start"""
    if t is None:
        return None
    rows = t.reshape(t.shape[0], -1)
    buf = torch.zeros(rows.shape[0], rows.shape[1] + 3, device=dev)
    buf[:, 1:1 + rows.shape[1]] = rows.to(dev)
    return buf[:, 1:1 + rows.shape[1]].unflatten(1, t.shape[1:])


def check(names, got, again, want, bound, shape):
    for name, g, g2, w, b in zip(names, got, again, want, bound):
        err = (g.double().cpu() - w).abs()
        ratio = float((err / b.clamp_min(1e-300)).max())
        print(f"{name} {shape}: largest error {float(err.max()):.3e}, largest error / bound {ratio:.3e}")
        assert bool((err <= b).all()), name
        assert torch.equal(g, g2), f"{name} differs between two runs"


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_query_and_stats_against_float64(dev, shape):
    ops_cpu, want, bound, d_stats, want_st, bound_st = case(*shape[:9])
    move = (lambda t: padded(t, dev)) if shape[9] else (lambda t: None if t is None else t.to(dev))
    x, K, a, b, m, Wfc, dy = (move(t) if i in (0, 4, 5, 6) else t.to(dev) for i, t in enumerate(ops_cpu))
    run = lambda: [nat.conve_query_fwd(x, K, a, b, m, Wfc), *nat.conve_query_bwd(x, K, a, b, m, Wfc, dy)]  # noqa: E731
    got = run()
    check(("y", "d_Wfc", "d_x", "d_K", "d_a", "d_b"), got, run(), want, bound, shape)
    # a NULL output skips its product and leaves the others as they were
    for keep in range(5):
        only = nat.conve_query_bwd(x, K, a, b, m, Wfc, dy, want=[i == keep for i in range(5)])
        assert [o is None for o in only] == [i != keep for i in range(5)]
        assert torch.equal(only[keep], got[1 + keep])
    d_mean, d_M2 = (t.to(dev) for t in d_stats)
    def run_stats():
        mean, M2 = nat.conve_stats_fwd(x, K)
        return [mean, M2, *nat.conve_stats_bwd(x, K, mean, d_mean, d_M2)]
    got = run_stats()
    check(("mean", "M2", "stats d_x", "stats d_K"), got, run_stats(), want_st, bound_st, shape)
    assert torch.equal(nat.conve_stats_bwd(x, K, got[0], d_mean, d_M2, want=(False, True))[1], got[3])


@pytest.mark.gpu
def test_empty_batch_and_the_image_limit(dev):
    x, K, a, b, m, Wfc, dy = (None if t is None else t.to(dev) for t in case(*SHAPES[1][:9])[0])
    grads = nat.conve_query_bwd(x[:0], K, a, b, None, Wfc, dy[:0])
    assert grads[1].shape[0] == 0 and all(not bool(g.any()) for g in (grads[0], *grads[2:]))
    assert nat.conve_query_fwd(x[:0], K, a, b, None, Wfc).shape == (0, Wfc.shape[0])
    S, Cin, H2, W, Cout, kh, kw, d = PAST_LIMIT
    with pytest.raises(RuntimeError, match="bytes of LDS"):
        nat.conve_query_fwd(torch.zeros(S, Cin, H2, W, device=dev), torch.zeros(Cout, Cin, kh, kw, device=dev),
                            torch.ones(Cout, device=dev), torch.ones(Cout, device=dev), None,
                            torch.zeros(d, Cout * (H2 - kh + 1) * (W - kw + 1), device=dev))


@pytest.mark.gpu
def test_masked_channels_contribute_nothing(dev):
    """Rows whose mask of a channel is 0: that channel's block of Wfc does not reach y, and its G does not reach d_x."""
    x, K, a, b, m, Wfc, dy = (t.to(dev) for t in case(*SHAPES[2][:9])[0])
    hw = Wfc.shape[1] // K.shape[0]
    other = Wfc.clone()
    other[:, :hw] = torch.randn_like(other[:, :hw])  # channel 0's weights replaced
    off = m[:, 0] == 0
    assert bool(off.any()) and bool((~off).any())
    y0, y1 = nat.conve_query_fwd(x, K, a, b, m, Wfc), nat.conve_query_fwd(x, K, a, b, m, other)
    assert torch.equal(y0[off], y1[off]) and not torch.equal(y0[~off], y1[~off])
    only_c0 = torch.zeros_like(m)
    only_c0[:, 0] = m[:, 0]
    d_x = nat.conve_query_bwd(x, K, a, b, only_c0, Wfc, dy, want=(False, True, False, False, False))[1]
    assert not bool(d_x[off].any()) and bool(d_x[~off].any())


@pytest.mark.gpu
def test_no_feature_map_is_allocated(dev):
    """Forward + backward of both ops at (512, the paper's shape) grow the peak allocation by less than ONE [S, F]
    fp32 buffer (21.2 MB) beyond their returned outputs."""
    S, F = 512, 32 * 18 * 18
    gen = torch.Generator().manual_seed(0)
    x, K, Wfc, dy = (torch.randn(s, generator=gen).to(dev).requires_grad_(g) for s, g in
                     (((S, 1, 20, 20), True), ((32, 1, 3, 3), True), ((200, F), True), ((S, 200), False)))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    mean, M2 = ops.ConvEChannelStats.apply(x, K)
    a, b = torch.rsqrt(M2 / (S * 324) + 1e-5), -mean
    mask = torch.nn.functional.dropout(torch.ones(S, 32, device=dev), 0.2)
    y = ops.ConvEQuery.apply(x, K, a, b, mask, Wfc)
    grads = torch.autograd.grad(y, [x, K, Wfc], dy)
    torch.cuda.synchronize()
    returned = sum(t.numel() * 4 for t in (mean, M2, y, *grads))
    grown = torch.cuda.max_memory_allocated(dev) - before - returned
    print(f"peak allocation beyond the outputs: {grown} bytes; [S, F] fp32: {S * F * 4}")
    assert grown < S * F * 4
