"""The small kernels of a step with their loads in flight: the fixed-order row sum of the
one-launch loss and of `k_pertriple_tail` (`strided_sum_agent`, csrc/common.h), and the register path of the query /
positive-score kernels (`fwd_rows_in_registers`, csrc/prepare.hip).

  1. Row sum.  The loss a launch returns equals, bit for bit, the order the kernels state applied to the `row_loss` the
     same launch returned: thread t of T adds the terms t, t + T, t + 2 T, ... in that order, then a halving tree over
     the T threads (T = 256 for `k_loss_rows`, 1024 for `k_sum_rows` behind more than 4 * 4096 rows, the workgroup's
     size for `k_pertriple_tail`).  The numpy restatement of that order is itself checked against a plain loop, on
     the CPU.  Sizes: one thread, one workgroup, the 256 / 4096 edges (one term more or less per thread, one group of
     16 loads more), the largest one-launch grid, and the two-launch path once.
  2. Query / triple.  `query_triple_fwd` == `query_fwd` + `score_triple_fwd` bit for bit, and both against float64
     under the project's bound (rtol 1e-4, atol max(1e-5, 2e-6 max|want|): `close` of test_hip_parity.py, as
     `test_scoring_vs_oracle` calls it).  Widths: below one trip (2), one trip exact (64), ragged (66, 510), the
     edges of the 4 / 8 / 16 trip classes (128 .. 1024), and 1026 for the loops that wider rows keep."""

import ctypes

import numpy as np
import pytest
import torch

from besskge import _native as nat
from test_fused_step_kernels import loss_desc
from test_hip_parity import close

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda", 0)


# ================================================================================================ 1. the row sum
def strided_tree_sum(terms, threads):
    """float32: thread t adds terms[t], terms[t + threads], ... in ascending order onto 0, then the halving tree."""
    terms = np.asarray(terms, dtype=np.float32)
    acc = np.zeros(threads, dtype=np.float32)
    for j in range(0, len(terms), threads):
        chunk = terms[j:j + threads]
        acc[:len(chunk)] = acc[:len(chunk)] + chunk
    h = threads // 2
    while h > 0:
        acc[:h] = acc[:h] + acc[h:2 * h]
        h //= 2
    return acc[0]


def strided_tree_sum_loop(terms, threads):
    """The same order, one scalar addition at a time."""
    part = []
    for t in range(threads):
        a = np.float32(0)
        for i in range(t, len(terms), threads):
            a = np.float32(a + np.float32(terms[i]))
        part.append(a)
    h = threads // 2
    while h > 0:
        for t in range(h):
            part[t] = np.float32(part[t] + part[t + h])
        h //= 2
    return part[0]


@pytest.mark.parametrize("n,threads", [(1, 256), (5, 256), (255, 256), (257, 256), (4097, 256), (4097, 1024), (700, 64)])
def test_restatement_of_the_sum_order_equals_a_plain_loop(n, threads):
    terms = (np.random.default_rng(n + threads).standard_normal(n) * 3 + 1).astype(np.float32)
    a, b = strided_tree_sum(terms, threads), strided_tree_sum_loop(terms, threads)
    assert a.dtype == np.float32 and a.tobytes() == b.tobytes()
    assert abs(float(a) - float(terms.astype(np.float64).sum())) <= 1e-6 * float(np.abs(terms).sum())


def launch_loss(dev, l, pos, neg, w, counter):
    S, N = neg.shape
    row_loss = torch.full((S,), float("nan"), device=dev)
    loss = torch.full((1,), float("nan"), device=dev)
    nat._launch("bess_loss_fwd_bwd_one_launch", dev, ctypes.byref(l), pos.data_ptr(), neg.data_ptr(), S, N, N, w.data_ptr(),
                w.numel(), row_loss.data_ptr(), loss.data_ptr(), None, None, 0, None, counter.data_ptr())
    torch.cuda.synchronize()
    return loss.cpu().numpy()[0], row_loss.cpu().numpy()


def check_loss_sum(dev, S, N, threads):
    gen = torch.Generator().manual_seed(7 * S + N)
    pos = torch.randn(S, generator=gen).to(dev)
    neg = torch.randn(S, N, generator=gen).to(dev)
    w = (torch.rand(S, generator=gen) + 0.5).to(dev)
    l = loss_desc("logsigmoid_adv", N)
    counter = torch.zeros(nat.TICKET_INTS, dtype=torch.int32, device=dev)
    loss, rows = launch_loss(dev, l, pos, neg, w, counter)
    assert np.isfinite(rows).all() and len(np.unique(rows)) > S // 2
    want = strided_tree_sum(rows, threads)
    assert loss.tobytes() == want.tobytes(), f"S={S} N={N}: loss {loss!r}, its row terms in the stated order {want!r}"
    assert int(counter.abs().sum()) == 0, f"S={S} N={N}: the counter is not left zero"
    again, rows2 = launch_loss(dev, l, pos, neg, w, counter)
    assert again.tobytes() == loss.tobytes() and np.array_equal(rows, rows2) and int(counter.abs().sum()) == 0


@gpu
@pytest.mark.parametrize("N", [4, 256])
def test_one_launch_loss_is_its_row_terms_in_the_stated_order(dev, N):
    for S in (1, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 16384):
        check_loss_sum(dev, S, N, 256)


@gpu
def test_loss_of_16385_rows_is_summed_by_the_second_launch(dev):
    check_loss_sum(dev, 16385, 4, 1024)


@gpu
@pytest.mark.parametrize("S", [5, 256, 4097])
def test_pertriple_tail_loss_is_its_row_terms_in_the_stated_order(dev, S):
    W, N, M, R = 64, 8, 61, 5
    gen = torch.Generator().manual_seed(S)
    E = (torch.randn(M, W, generator=gen) * 0.3).to(dev)
    Rt = (torch.randn(R, W, generator=gen) * 0.5).to(dev)
    hi, ti = (torch.randint(0, M, (S,), generator=gen).to(torch.int32).to(dev) for _ in range(2))
    ri = torch.randint(0, R, (S,), generator=gen).to(torch.int32).to(dev)
    ni = torch.randint(0, M, (S * N,), generator=gen).to(torch.int32).to(dev)
    w = (torch.rand(S, generator=gen) + 0.5).to(dev)
    desc = nat.make_desc(nat.COMPLEX, 1, E, W)
    l = loss_desc("logsigmoid_adv", N)
    assert nat.pertriple_tail_supported(desc, N)
    q, pos = nat.query_triple_fwd(desc, nat.CORRUPT_TAIL, nat.RowSource(E, hi), nat.RowSource(E, ti), Rt, ri)
    out, (ml, acc) = nat.neg_score_pertriple_fwd_dq(desc, l, q, nat.RowSource(E, ni), N, pos, w, defer=True)
    counter = torch.zeros(nat.TICKET_INTS, dtype=torch.int32, device=dev)
    threads = 64 * (16 if S > 1024 else 4)  # tail_waves (csrc/prepare.hip) at rows of 64 floats

    def launch():
        o = {k: torch.full(shape, float("nan"), device=dev) for k, shape in
             dict(row_loss=(S,), loss=(1,), d_pos=(S,), d_neg=(S, N), d_head=(S, W), d_tail=(S, W)).items()}
        d_rel = torch.zeros(R, W, device=dev)
        nat._launch("bess_pertriple_tail", dev, ctypes.byref(desc), ctypes.byref(l), nat.CORRUPT_TAIL, E.data_ptr(),
                    hi.data_ptr(), E.data_ptr(), ti.data_ptr(), Rt.data_ptr(), ri.data_ptr(), S, ml.data_ptr(), acc.data_ptr(),
                    int(ml.shape[1]), pos.data_ptr(), out.data_ptr(), N, N, w.data_ptr(), S, o["row_loss"].data_ptr(),
                    o["loss"].data_ptr(), o["d_pos"].data_ptr(), o["d_neg"].data_ptr(), N, None, o["d_head"].data_ptr(),
                    o["d_tail"].data_ptr(), d_rel.data_ptr(), counter.data_ptr())
        torch.cuda.synchronize()
        return o["loss"].cpu().numpy()[0], o["row_loss"].cpu().numpy()

    loss, rows = launch()
    assert np.isfinite(rows).all()
    want = strided_tree_sum(rows, threads)
    assert loss.tobytes() == want.tobytes(), f"S={S}: loss {loss!r}, its row terms in the stated order {want!r}"
    assert int(counter.abs().sum()) == 0
    again, rows2 = launch()
    assert again.tobytes() == loss.tobytes() and np.array_equal(rows, rows2) and int(counter.abs().sum()) == 0


# ================================================================================================ 2. query / triple
SCORERS = [("TransE", 1), ("TransE", 2), ("RotatE", 1), ("RotatE", 2), ("DistMult", 1), ("ComplEx", 1)]
CODE = dict(TransE=nat.TRANSE, RotatE=nat.ROTATE, DistMult=nat.DISTMULT, ComplEx=nat.COMPLEX)
SIZES = (1, 3, 4, 5, 257)
WIDTHS = (2, 64, 66, 128, 510, 512, 1024, 1026)  # 1026: above the register path


def reference64(name, p, tail_side, h, r, t):
    """(query rows, positive scores) in float64; complex rows are [re(d) | im(d)], RotatE's relation row d phases."""
    h, r, t = h.double(), r.double(), t.double()
    x = h if tail_side else t  # the query is built from the head for tail corruption
    if name == "TransE":
        d = h + r - t
        return (x + r if tail_side else x - r), -(d.abs().sum(-1) if p == 1 else d.abs().pow(p).sum(-1).pow(1.0 / p))
    if name == "DistMult":
        return x * r, (h * r * t).sum(-1)
    d = h.shape[-1] // 2
    rr, ri = (torch.cos(r), torch.sin(r)) if name == "RotatE" else (r[:, :d], r[:, d:])
    mul = lambda ar, ai, br, bi: (ar * br - ai * bi, ar * bi + ai * br)  # noqa: E731
    qr, qi = mul(x[:, :d], x[:, d:], rr, ri if tail_side else -ri)  # heads: the conjugate relation times the tail
    sr, si = mul(h[:, :d], h[:, d:], rr, ri)
    if name == "ComplEx":
        score = (sr * t[:, :d] + si * t[:, d:]).sum(-1)
    else:
        diff = torch.cat([sr - t[:, :d], si - t[:, d:]], dim=-1).abs()
        score = -(diff.sum(-1) if p == 1 else diff.pow(p).sum(-1).pow(1.0 / p))
    return torch.cat([qr, qi], dim=-1), score


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("name,p", SCORERS, ids=[f"{n}{p}" for n, p in SCORERS])
def test_query_and_positive_score_in_every_width_class(dev, name, p, dtype):
    M, n_rel = 50, 6
    for W in WIDTHS:
        Wr = W // 2 if name == "RotatE" else W
        gen = torch.Generator().manual_seed(W + p)
        table = torch.randn(M, W, generator=gen).to(dtype)
        rel = torch.randn(n_rel, Wr, generator=gen).to(dtype)
        desc = nat.make_desc(CODE[name], p, table, Wr)
        tab_d, rel_d = table.to(dev), rel.to(dev)
        for n in SIZES:
            hidx, tidx = (torch.randint(0, M, (n,), generator=gen) for _ in range(2))
            hidx[0], hidx[-1], tidx[-1], tidx[0] = 0, M - 1, 0, M - 1  # the first and the last row of the table
            if n >= 3:
                hidx[1], tidx[1] = hidx[0], tidx[2]  # repeated rows
            ridx = torch.randint(0, n_rel, (n,), generator=gen)
            listed = n % 2 == 1  # else: tails that came through an exchange, rows without an index list
            other = torch.randn(n, W, generator=gen).to(dtype)
            h, t, r = table[hidx], (table[tidx] if listed else other), rel[ridx]
            head = nat.RowSource(tab_d, hidx.to(torch.int32).to(dev))
            tail = nat.RowSource(tab_d, tidx.to(torch.int32).to(dev)) if listed else nat.RowSource(other.to(dev), None)
            ri = ridx.to(torch.int32).to(dev)
            for side in (nat.CORRUPT_HEAD, nat.CORRUPT_TAIL):
                what = f"{name} p={p} {dtype} W={W} n={n} side={side}"
                q, pos = nat.query_triple_fwd(desc, side, head, tail, rel_d, ri)
                q1 = nat.query_fwd(desc, side, head if side == nat.CORRUPT_TAIL else tail, rel_d, ri)
                pos1 = nat.score_triple_fwd(desc, head, tail, rel_d, ri)
                assert torch.equal(q, q1), what + ": query rows of the fused and the single launch differ"
                assert torch.equal(pos, pos1), what + ": positive scores of the fused and the single launch differ"
                q64, pos64 = reference64(name, p, side == nat.CORRUPT_TAIL, h, r, t)
                try:
                    close(q, q64.float(), scale=2e-6)
                    close(pos, pos64.float(), scale=2e-6)
                except AssertionError as e:
                    raise AssertionError(f"{what}: {e}") from None
