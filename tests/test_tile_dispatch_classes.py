"""Instantiations of the shared-negative tile kernels and of the top-k kernel that no other test selects (DESIGN.md
section 18 has the table of all of them with the test that launches each): the 64-row forward tile on ragged widths,
the backward tile with scalar loads (W % 4 != 0) in all four pairs of tile heights and with 16-byte loads in the mixed
pairs, the both-products kernel with eight waves on an fp32 table, the partial-sum kernel on an fp16 table without the
rounded query, and the one-wave-per-row top-k with scalar loads and lists of more than 64.  Every case reads the
launched kernel's name from the profiler's kernel list, as tests/test_small_step.py does, and compares with a float64
restatement built 64 query rows at a time; bounds as in
test_hip_parity.py::test_shared_distance_backward_tile_variants, relative to max|reference|: 2e-6 for scores, 1e-5 for
gradients, 2e-5 for gradients at p = 2 (which divide by the fp32 forward score)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

F32, F16 = torch.float32, torch.float16


def kernel_launched(names, kernel, *args):
    """Is kernel<args...> among the profiler's names?  (It demangles what its demangler knows; names with _Float16
    arrive mangled: both spellings are looked for.)  args: torch dtypes, bools and ints."""
    text = {F32: "float", F16: "_Float16", True: "true", False: "false"}
    code = {F32: "f", F16: "DF16_", True: "Lb1E", False: "Lb0E"}
    plain = f"{kernel}<{', '.join(text[a] if type(a) is not int else str(a) for a in args)}>("
    mangled = f"{len(kernel)}{kernel}I{''.join(code[a] if type(a) is not int else f'Li{a}E' for a in args)}EEv"
    return any(plain in n or mangled in n for n in names)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda", 0)


def launched(fn):
    """fn() and the names of the kernels it launched."""
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    return out, [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def distance_case(S, N, W, dtype, dev):
    g = torch.Generator().manual_seed(S * 7 + N + W)
    M = 2000
    table = (torch.randn(M, W, generator=g) * 0.5).to(dtype).to(dev)
    q = (torch.randn(S, W, generator=g) * 0.5).half().float().to(dev)  # fp16-exact queries: any rounding mode agrees
    idx = torch.randint(M, (N,), generator=g, dtype=torch.int32).to(dev)
    go = (torch.softmax(torch.randn(S, N, generator=g) * 2, -1) * torch.rand(S, 1, generator=g)).to(dev)
    return table, q, idx, go


def distance_reference(q, rows, go, p):
    """-||q - e||_p and, with `go`, its gradients (sgn(0) = 0; the p = 2 gradient is 0 at zero distance) in float64."""
    S, W = q.shape
    qd, rows = q.double(), rows.double()
    want_out = torch.zeros(S, rows.shape[0], dtype=torch.float64, device=q.device)
    want_q, want_n = torch.zeros_like(qd), torch.zeros_like(rows)
    for a0 in range(0, S, 64):  # [64, N, W] float64 at a time
        diff = qd[a0:a0 + 64, None, :] - rows[None, :, :]
        if p == 1:
            coef = torch.sign(diff)
            want_out[a0:a0 + 64] = -diff.abs().sum(-1)
        else:
            nrm = diff.norm(dim=-1, keepdim=True)
            coef = torch.where(nrm > 0, diff / nrm.clamp(min=1e-300), torch.zeros_like(diff))
            want_out[a0:a0 + 64] = -nrm[..., 0]
        if go is not None:
            t = go[a0:a0 + 64].double()[:, :, None] * coef
            want_q[a0:a0 + 64] = -t.sum(1)
            want_n += t.sum(0)
    return want_out, want_q, want_n


def rel_err(got, want):
    return float((got.double() - want).abs().max()) / float(want.abs().max())


@pytest.mark.parametrize("W", [20, 6])  # stages of 16 with a ragged last one: 16-byte loads (W % 4 == 0) and scalar loads
@pytest.mark.parametrize("p,dtype", [(1, torch.float32), (2, torch.float32), (1, torch.float16), (2, torch.float16)])
def test_forward_64_row_tile_on_ragged_widths(dev, p, dtype, W):
    """k_neg_shared_fwd<T, RED, ALIGNED = false, MI = 4>: 13 x 16 = 208 tiles of 64 x 64 (192 and more take the 64-row
    tile), ragged in rows, columns and width."""
    from besskge import _native as nat

    S, N = 769, 961
    table, q, idx, _ = distance_case(S, N, W, dtype, dev)
    d = nat.make_desc(nat.TRANSE, p, table, W)
    out, names = launched(lambda: nat.neg_score_shared_fwd(d, q, nat.RowSource(table, idx)))
    assert kernel_launched(names, "k_neg_shared_fwd", dtype, p, False, 4), names
    want_out, _, _ = distance_reference(q, table[idx.long()], None, p)
    err = rel_err(out, want_out)
    print(f"scores: {err:.3e}")
    assert err <= 2e-6


BWD_CASES = [  # S, N, W, p, table type -> kernel, template arguments behind the table type
    # scalar loads (W % 4 != 0; the second column tile has 6 columns): <RED, VEC4, ROUND16, MI of d_query, MI of d_neg>
    *[(S, N, 70, p, t, "k_neg_shared_bwd", (p, False, False, mia, mib))
      for S, N, mia, mib in ((70, 130, 2, 2),       # 32-row tiles on both sides
                             (1024, 1030, 4, 4),    # 64-row tiles on both sides, the reduction split 16 ways
                             (773, 1291, 4, 2), (1291, 773, 2, 4))  # one product fills the chip with 64-row tiles
      for p in (1, 2) for t in (F32, F16)],
    # the mixed tile heights with 16-byte loads: behind the packed-fp16 forward (ROUND16), at p = 2, and at a width
    # the packed forward does not take (68 % 32 != 0)
    (773, 1291, 128, 1, F16, "k_neg_shared_bwd", (1, True, True, 4, 2)),
    (773, 1291, 128, 2, F16, "k_neg_shared_bwd", (2, True, False, 4, 2)),
    (1291, 773, 68, 1, F16, "k_neg_shared_bwd", (1, True, False, 2, 4)),
    # both products from one evaluation of the sign, eight waves per workgroup (N >= 2048), fp32 table
    (256, 2048, 64, 1, F32, "k_l1_bwd_both", (False, 8)),
]


@pytest.mark.parametrize("S,N,W,p,dtype,kernel,args", BWD_CASES)
def test_backward_classes(dev, S, N, W, p, dtype, kernel, args):
    """bess_neg_score_shared_bwd of the distance scorers in the classes of BWD_CASES."""
    from besskge import _native as nat

    table, q, idx, go = distance_case(S, N, W, dtype, dev)
    d = nat.make_desc(nat.TRANSE, p, table, W)
    src = nat.RowSource(table, idx)
    out = nat.neg_score_shared_fwd(d, q, src)
    (dq, dn), names = launched(lambda: nat.neg_score_shared_bwd(d, q, src, out, go))
    assert kernel_launched(names, kernel, dtype, *args), names
    want_out, want_q, want_n = distance_reference(q, table[idx.long()], go, p)
    errs = rel_err(out, want_out), rel_err(dq, want_q), rel_err(dn, want_n)
    print("scores %.3e, d_query %.3e, d_neg %.3e" % errs)
    tol = 2e-5 if p == 2 else 1e-5
    assert errs[0] <= 2e-6 and errs[1] <= tol and errs[2] <= tol


def test_partial_sums_on_an_fp16_table_without_the_rounded_query(dev):
    """k_l1_bwd_parts<_Float16, ROUND16 = false>: BESS_FLAG_FP32_MATH keeps the forward off the packed-fp16 kernel, so
    the backward differentiates the unrounded query (queries that fp16 cannot hold exactly tell the two apart)."""
    from besskge import _native as nat

    S, N, W = 256, 288, 64
    table, _, idx, go = distance_case(S, N, W, F16, dev)
    q = (torch.randn(S, W, generator=torch.Generator().manual_seed(5)) * 0.5).to(dev)
    d = nat.make_desc(nat.TRANSE, 1, table, W)
    d.reserved[0] |= nat.FLAG_FP32_MATH
    src = nat.RowSource(table, idx)
    assert nat.shared_bwd_parts_plan(d, S, N)[0] > 0
    out = nat.neg_score_shared_fwd(d, q, src)
    (dqp, dep), names = launched(lambda: nat.neg_score_shared_bwd_parts(d, q, src, go))
    assert kernel_launched(names, "k_l1_bwd_parts", F16, False), names
    want_out, want_q, want_n = distance_reference(q, table[idx.long()], go, 1)
    errs = rel_err(out, want_out), rel_err(dqp.sum(0), want_q), rel_err(dep.sum(0), want_n)
    print("scores %.3e, d_query %.3e, d_neg %.3e" % errs)
    assert errs[0] <= 2e-6 and errs[1] <= 1e-5 and errs[2] <= 1e-5


def test_topk_one_wave_per_row_scalar_loads_long_lists(dev):
    """k_topk_update<WPR = 1, VEC = false, TWO = true, ORD = false>: more than 6144 rows, an odd leading dimension,
    lists of 65.  Scores are small integers (many ties): the lists are the stable descending sort's, exactly."""
    from besskge import _native as nat

    rows, L, kk = 6150, 77, 65
    gen = torch.Generator().manual_seed(rows + L)
    bs = torch.full((rows, kk), -50000.0, device=dev)
    bi = torch.full((rows, kk), -1, dtype=torch.int32, device=dev)
    cols, names = [], []
    for w in range(2):
        sc = torch.randint(0, 40, (rows, L), generator=gen).float()
        cols.append(sc)
        view = sc.to(dev)
        names += launched(lambda: nat.topk_update(view, bs, bi, id_base=w * L))[1]
    assert kernel_launched(names, "k_topk_update", 1, False, True, False), names
    allc = torch.cat(cols, dim=1).double()
    order = torch.sort(allc, dim=1, descending=True, stable=True).indices[:, :kk]
    assert torch.equal(bi.cpu().long(), order)
    assert torch.equal(bs.cpu().double(), torch.take_along_dim(allc, order, dim=1))
