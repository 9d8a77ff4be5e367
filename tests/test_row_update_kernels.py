"""The half of csrc/segments.hip that writes the tables - the generic coalescing step (`bess_segment_sum_rows`,
`bess_coalesced_update`), the row-sparse optimisers (`bess_apply_segments_opt`, `bess_direct_update`, the optimiser
branch of `seg_finish` reached through `bess_neg_pertriple_step_segments`) and their helpers (`bess_assign_state_rows`,
`bess_map_extra_rows`) - against float64, in every class these kernels branch on.  Other tests compare these kernels
with each other (test_small_step.py: the direct update with the indexed one) or with float32 formulas at one shape
(test_optimizers.py); they are anchored here:

  0. the reference itself, on the CPU (no device): `update_rule`, the lazy optimiser step that include/besskge_hip.h
     and `opt_step` state, in float64 == torch.optim in float64 (SGD with momentum and weight decay, Adagrad with weight
     decay, SparseAdam), to 1e-12 over three steps.  `torch.optim.Adam` and `AdamW` add eps to sqrt(v / bias2), this
     rule (like SparseAdam) to sqrt(v): they are NOT the anchor; the decoupled-decay line `p -= lr wd p` is checked by
     its closed form (the AdamW result == the Adam result - lr wd p).  The float32 restatement of the rule stays inside
     the bound on every "normal" case below, and the class functions put every width where the table says;
  1. sums: `bess_segment_sum_rows` and `bess_coalesced_update(sum_out)` == a float32 sum in reference order, bit for
     bit (the header of segments.hip promises this), and == float64 `index_add_` within the bound;
  2. updates: every entry point, over several steps with changing row sets, == `update_rule` in float64 started from
     the device's own table and state after the step before (each step is judged alone); rows not touched by a step
     are bit-equal to before, in the table and in both state tables.

Class table of the sum kernels and of `bess_direct_update` (one wave per row; float4 path: lane l takes columns
4 l .. 4 l + 3, then + 256; scalar path (W & 3 != 0): lane l takes column l, then + 64):

  path   | W    | column passes
  float4 | 4    | 1 (one lane)          scalar | 1, 3, 63 | 1
  float4 | 252  | 1 (63 lanes)          scalar | 65       | 2
  float4 | 256  | 1 (full)              scalar | 130      | 3
  float4 | 260  | 2 (the last: 1 lane)  scalar | 257      | 5
  float4 | 516  | 3 (the last: 1 lane)

  index: 300 references over 97 rows, segments of 1, 2, 3, 4, 5, 8, 9 and 37 references (the four-in-flight loop with
  its clamped tail at every length mod 4), the last reference the only one of its row; 1, 3 and 8 lists (one of one
  row, an empty one in the middle), cut anywhere, so that segments cross `first[]` inside a group of four;
  grid-stride: 17 000 unique rows at W = 4 (> 4096 workgroups x 4 waves; the device-wide radix index);
  `bess_apply_segments_opt` (flat element loop): W = 1, 48, 257, and 1100 segments x 1024 (> 4096 x 256 elements);
  the `axpy` job: 1, 1023, 1025 and 300 001 elements (> 256 workgroups x 1024: its own stride loop).

Class table of the fused step (`seg_finish` with an optimiser; `dispatch_class` of test_pertriple_kernels.py): one
width per (dtype, VEC, IT) class, the two full widths, every windowed width - DOT (row loaded after the reduction),
L1 (before it) at every width with Adam + decay, L2 (p = 2) at one width per dtype, the other optimisers at f32 132
and f16 264:

  dtype, VEC | IT 1 | IT 2 | IT 4 | IT 8 | IT 16 | full | windows
  f32, 4     |  60  | 100  | 132  | 388  | 1020  | 1024 | 2000 = 1024 + 976
  f32, 1     |   6  |  30  |  50  | 102  |  254  |      | 257 = 256 + 1, 513 = 256 + 256 + 1
  f16, 8     | 120  | 200  | 264  | 776  | 2040  | 2048 | 2056 = 2048 + 8
  f16, 2     |   6  |  50  |  66  | 194  |  510  |      | 514 = 512 + 2
  f16, 1     |   7  |  31  |  49  | 101  |  255  |      | 257 = 256 + 1

  5 queries x 37 negatives over 97 rows; extras through `bess_map_extra_rows` (some on segments, some orphans that go
  through `bess_apply_segments_opt(keep)`, some segments without one); one hot row of 520 references (> SEGMENT_CAP:
  the long tier's `seg_finish`) at f32 388 and f16 264; 4096 queries at f32 512 and f16 512 (n_conc = 2: windows side
  by side, state and xsum shifted inside the kernel) and at f32 768 (three windows one after the other).

Bounds are the project's: rtol 1e-4, atol max(1e-5, 2e-6 max|want|), for f16 tables plus half an f16 ulp of the
float64 value (the kernel rounds once, from its f32 result).  Every case also evaluates the rule in float32 with its
sums taken in REVERSED reference order (the restatement); where that is itself more than one unit outside, the case's
bound becomes 4 x the restatement's error and the case is printed (`check`, the rule of test_pertriple_kernels.py).
Part 0 asserts that no "normal" case needs that.  Measured errors: DESIGN.md, section 16."""

import ctypes
import functools

import numpy as np
import pytest
import torch

import test_pertriple_kernels as ptk
from besskge import _native as nat

gpu = pytest.mark.gpu
F32, F16 = torch.float32, torch.float16
F64 = torch.float64
RTOL, ATOL, SCALE = ptk.RTOL, ptk.ATOL, ptk.SCALE
tname = ptk.tname

ROWS = 97
NEVER = list(range(87, 97))      # rows no step touches
ONLY13 = list(range(77, 87))     # rows that steps 1 and 3 touch and step 2 does not
LENGTHS = (1, 2, 3, 4, 5, 8, 9)
COUNTS = [37] + list(LENGTHS) * 8 + [3, 2, 1]  # 299 references on 60 rows; one more reference closes the list
SPLITS = {1: [300], 3: [100, 1, 199], 8: [60, 1, 50, 0, 70, 40, 30, 49]}
SUM_WIDTHS = {"float4": [4, 252, 256, 260, 516], "scalar": [1, 3, 63, 65, 130, 257]}
SUM_PASSES = {4: 1, 252: 1, 256: 1, 260: 2, 516: 3, 1: 1, 3: 1, 63: 1, 65: 2, 130: 3, 257: 5}
ALL_SUM_WIDTHS = SUM_WIDTHS["float4"] + SUM_WIDTHS["scalar"]
APPLY_WIDTHS = [1, 48, 257]
DIRECT_WIDTHS = [4, 256, 260, 3, 130]
AXPY_SIZES = [1, 1023, 1025, 300_001]
# a power of two: alpha g is exact, and T(float(t) + alpha g) is the table type's nearest to the exact sum, whether
# the kernel forms it with an FMA or not (for f16 the compiler emits one mixed-precision FMA that rounds the exact sum
# once, straight to f16 - as in the dense axpy of csrc/rows.hip)
AXPY_ALPHA = -0.0625
BIG_ROWS = 17_000     # unique rows of the grid-stride case of the wave-per-row kernels
BIG_APPLY = (1100, 1024)

# (the hyper-parameters are used as their float32 values.  Adam's eps is 1e-4: with 1e-8 its step lr g / (|g| + eps')
# jumps from -lr to +lr within |g| < 1e-6, so that on a few of the 10^5 elements of a case the ORDER of a float32 sum
# decides the step - the float32 restatement is then itself 70 x outside the bound, e.g. at f16 2048 DOT)
OPTS = {
    "sgd": dict(kind=nat.OPT_SGD, lr=0.05, momentum=0.0, weight_decay=0.0, beta1=0.0, beta2=0.0, eps=0.0),
    "sgdm": dict(kind=nat.OPT_SGD, lr=0.05, momentum=0.9, weight_decay=0.01, beta1=0.0, beta2=0.0, eps=0.0),
    "adagrad": dict(kind=nat.OPT_ADAGRAD, lr=0.05, momentum=0.0, weight_decay=0.01, beta1=0.0, beta2=0.0, eps=1e-10),
    "adam": dict(kind=nat.OPT_ADAM, lr=0.01, momentum=0.0, weight_decay=0.0, beta1=0.9, beta2=0.999, eps=1e-4),
    "adamw": dict(kind=nat.OPT_ADAM, lr=0.01, momentum=0.0, weight_decay=0.01, beta1=0.9, beta2=0.99, eps=1e-4),
}
N_STATE = {"sgd": 0, "sgdm": 1, "adagrad": 1, "adam": 2, "adamw": 2}

# the fused step: one width per class, the full widths, the windowed widths
FUSED_WIDTHS = ([(dt, ws[0]) for (dt, _), its in ptk.CLASS_WIDTHS.items() for ws in its.values()]
                + sorted(ptk.FULL_WIDTHS, key=str) + list(ptk.WINDOW_WIDTHS))
FUSED_ALL_OPTS = [(F32, 132), (F16, 264)]
FUSED_L2 = [(F32, 100), (F16, 200)]
NQ, N_NEG, N_EXTRA = 5, 37, 40
HOT = [(F32, 388), (F16, 264)]
L2_WINDOWS = [(F32, 512, 2), (F16, 512, 2), (F32, 768, 1)]

MEASURED = {}  # (entry point, optimiser, dtype) -> [fp32 restatement, kernel]: largest error in units of the bound
WIDENED = []   # the cases that used the widened bound


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda", 0)


# ============================================================================================ 0. the reference
def update_rule(kind, hp, step, p, g, s1, s2, dtype=F64):
    """One lazy optimiser step on the touched rows, as include/besskge_hip.h and `opt_step` state it: (p, s1, s2) after
    the step, computed in `dtype` from the exactly converted inputs, the hyper-parameters taken as their float32 values.
    `kind` is a key of OPTS, or None with `hp` given."""
    hp = OPTS[kind] if hp is None else hp
    c = {k: torch.tensor(float(np.float32(v)), dtype=dtype) for k, v in hp.items() if k != "kind"}
    p, g, s1, s2 = (x.to(dtype).clone() for x in (p, g, s1, s2))
    if hp["kind"] == nat.OPT_SGD:
        g = g + c["weight_decay"] * p
        if hp["momentum"] != 0.0:
            s1 = c["momentum"] * s1 + g
            g = s1
        p = p - c["lr"] * g
    elif hp["kind"] == nat.OPT_ADAGRAD:
        g = g + c["weight_decay"] * p
        s1 = s1 + g * g
        p = p - c["lr"] * g / (s1.sqrt() + c["eps"])
    else:
        p = p - c["lr"] * c["weight_decay"] * p
        s1 = c["beta1"] * s1 + (1 - c["beta1"]) * g
        s2 = c["beta2"] * s2 + (1 - c["beta2"]) * g * g
        t = torch.tensor(float(step), dtype=dtype)
        bias1, bias2 = 1 - c["beta1"] ** t, 1 - c["beta2"] ** t
        p = p - c["lr"] * bias2.sqrt() / bias1 * s1 / (s2.sqrt() + c["eps"])
    return p, s1, s2


def sum_class(W):
    """(path, column passes) of a row of W floats in the wave-per-row kernels."""
    return ("float4", -(-W // 256)) if W % 4 == 0 else ("scalar", -(-W // 64))


def wave_rounds(n_seg, max_seg):
    """Grid-stride rounds of the wave-per-row kernels: min(ceil(max_seg / 4), 4096) workgroups of 4 waves."""
    return -(-n_seg // (4 * min(-(-max_seg // 4), 4096)))


def element_rounds(n_seg, max_seg, W):
    """Grid-stride rounds of `k_apply_segments_opt`: min(ceil(max_seg W / 256), 4096) workgroups of 256 elements."""
    return -(-n_seg * W // (256 * min(-(-max_seg * W // 256), 4096)))


def axpy_class(n):
    """(workgroups, stride rounds) of the axpy job: min(ceil(n / 1024), 256) workgroups of 256 threads - four rounds at
    most until the workgroup count saturates."""
    blocks = min(-(-n // 1024), 256)
    return blocks, -(-n // (256 * blocks))


def half_ulp16(x):
    """Half an f16 ulp at |x| (float64): 2^(e - 11) for 2^e <= |x| < 2^(e + 1), the subnormal spacing below 2^-14."""
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** -14))  # |x| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(x), e - 12)


def units(x, ref, slack=None):
    """max |x - ref| / (atol + rtol |ref| [+ slack]) with the project's atol = max(1e-5, 2e-6 max|ref|)."""
    ref = ref.double()
    if ref.numel() == 0:
        return 0.0
    bound = max(ATOL, SCALE * float(ref.abs().max())) + RTOL * ref.abs()
    if slack is not None:
        bound = bound + slack
    return float(((x.detach().double().cpu() - ref).abs() / bound).max())


def check(key, what, got, ref64, ref32, slack=None):
    """`got` against float64 at the project's bound - or, where the float32 restatement is itself outside it on these
    inputs, at 4 x the restatement's error.  The bound never depends on `got`.  `key` = (entry point, optimiser,
    dtype) of MEASURED."""
    assert got.shape == ref64.shape, f"{what}: shape {tuple(got.shape)}"
    assert bool(torch.isfinite(ref64).all())
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    e32, ek = units(ref32, ref64, slack), units(got, ref64, slack)
    rec = MEASURED.setdefault(key, [0.0, 0.0])
    rec[0], rec[1] = max(rec[0], e32), max(rec[1], ek)
    factor = 1.0 if e32 <= 1.0 else 4.0 * e32
    if factor > 1.0:
        WIDENED.append(what)
    if factor > 1.0 or ek > 1.0:
        print(f"{what}: kernel at {ek:.3g} x, fp32 restatement at {e32:.3g} x of the bound")
    assert ek <= factor, f"{what}: kernel at {ek:.3g} x the bound, fp32 restatement at {e32:.3g} x"


@functools.lru_cache(maxsize=None)
def ref_list(step, rows=ROWS):
    """The 300 references of step 1, 2 or 3 (int64): segments of 37 and of 1, 2, 3, 4, 5, 8, 9 references in a random
    order, then one reference to a row of its own.  NEVER rows are in no step, ONLY13 rows in steps 1 and 3."""
    gen = torch.Generator().manual_seed(7000 + step)
    pool = [r for r in range(rows) if r not in NEVER and r not in ONLY13]
    pool = torch.tensor(pool)[torch.randperm(len(pool), generator=gen)]
    if step != 2:
        pool = torch.cat([torch.tensor(ONLY13), pool])
        head = torch.randperm(len(COUNTS), generator=gen)  # the ONLY13 rows get any of the lengths
        pool = torch.cat([pool[: len(COUNTS)][head], pool[len(COUNTS):]])
    body = torch.repeat_interleave(pool[: len(COUNTS)], torch.tensor(COUNTS))
    body = body[torch.randperm(body.numel(), generator=gen)]
    return torch.cat([body, pool[len(COUNTS): len(COUNTS) + 1]])


@functools.lru_cache(maxsize=None)
def big_list():
    """20 000 references to BIG_ROWS unique rows of a table of BIG_ROWS + 1."""
    gen = torch.Generator().manual_seed(17)
    idx = torch.cat([torch.arange(BIG_ROWS), torch.randint(0, BIG_ROWS, (3000,), generator=gen)])
    return idx[torch.randperm(idx.numel(), generator=gen)]


def list_gradients(W, step, n=300, scale=1.0):
    gen = torch.Generator().manual_seed(100 * W + step)
    return torch.randn(n, W, generator=gen) * scale


def sums_of(idx, src, M, dtype=F64):
    """(unique rows, their summed gradient rows): float64 `index_add_`; in float32 in REVERSED reference order."""
    rows = torch.unique(idx)
    if dtype == F64:
        return rows, torch.zeros(M, src.shape[1], dtype=F64).index_add_(0, idx, src.double())[rows]
    out = torch.zeros(M, src.shape[1], dtype=F32)
    out.index_add_(0, idx.flip(0), src.flip(0).contiguous())
    return rows, out[rows]


def sum_in_reference_order(src, refs, offsets, n_seg):
    """out[s] = ((src[refs[r0]] + src[refs[r0 + 1]]) + ...) in float32: the order the kernels promise."""
    off = offsets[:n_seg].long()
    lens = offsets[1: n_seg + 1].long() - off
    out = torch.zeros(n_seg, src.shape[1], dtype=F32)
    for k in range(int(lens.max())):
        m = lens > k
        out[m] = out[m] + src[refs[off[m] + k].long()]
    return out


def table_of(dtype, rows, W, seed=0):
    gen = torch.Generator().manual_seed(31 * W + seed + (5 if dtype == F16 else 0))
    return (torch.randn(rows, W, generator=gen) * 0.3).to(dtype)


def zero_state(rows, W):
    return [torch.zeros(rows, W), torch.zeros(rows, W)]


def carried_state(rows, W, seed=0):
    """A state a few steps old: first moments / velocities of either sign, second moments / squared sums > 0."""
    gen = torch.Generator().manual_seed(977 * W + seed)
    return [torch.randn(rows, W, generator=gen) * 0.1, torch.rand(rows, W, generator=gen) * 0.05 + 1e-3]


def expected(opt, dtype, step, before, rows, g64, g32, slots=None):
    """What one step makes of the touched `rows`: ((p, s1, s2) in float64, the float32 restatement with p rounded once
    to the table's type, the state rows of `rows` (-1: none)).  `before` = (table, state1, state2) on the CPU."""
    tb, s1b, s2b = before
    srow = rows if slots is None else slots[rows].long()
    has = srow >= 0
    ins = []
    for k, s in enumerate((s1b, s2b)):
        x = torch.zeros(rows.numel(), tb.shape[1])
        if k < N_STATE[opt]:
            x[has] = s[srow[has]]
        ins.append(x)
    w64 = update_rule(opt, None, step, tb[rows], g64, ins[0], ins[1], F64)
    w32 = update_rule(opt, None, step, tb[rows], g32, ins[0], ins[1], F32)
    w32 = (w32[0].to(dtype).float(), w32[1], w32[2])
    return w64, w32, srow


def judge(entry, opt, dtype, what, step, before, after, rows, g64, g32, slots=None):
    """One step of one entry point: the touched rows and their state against `update_rule`, everything else bit-equal
    to `before`.  A row without a state row (slots[row] == -1) is stepped from zero state and keeps none."""
    key = (entry, opt, tname(dtype))
    w64, w32, srow = expected(opt, dtype, step, before, rows, g64, g32, slots)
    has = srow >= 0
    slack = half_ulp16(w64[0]) if dtype == F16 else None
    check(key, f"{what} table", after[0][rows], w64[0], w32[0], slack)
    for k in range(2):
        owned = torch.zeros(before[1 + k].shape[0], dtype=torch.bool)
        if k < N_STATE[opt]:
            check(key, f"{what} state{k + 1}", after[1 + k][srow[has]], w64[1 + k][has], w32[1 + k][has])
            owned[srow[has]] = True
        assert torch.equal(after[1 + k][~owned], before[1 + k][~owned]), f"{what}: a state{k + 1} row of no touched row moved"
    rest = torch.ones(before[0].shape[0], dtype=torch.bool)
    rest[rows] = False
    assert torch.equal(after[0][rest], before[0][rest]), f"{what}: an untouched table row moved"
    return w32


def opt_desc(opt, step, step_ptr=None, slot_map=None):
    hp = OPTS[opt]
    o = nat.OptDesc()
    o.kind, o.step = hp["kind"], step
    o.lr, o.momentum, o.weight_decay = hp["lr"], hp["momentum"], hp["weight_decay"]
    o.beta1, o.beta2, o.eps = hp["beta1"], hp["beta2"], hp["eps"]
    o.step_ptr = step_ptr.data_ptr() if step_ptr is not None else 0
    o.slot_map = slot_map.data_ptr() if slot_map is not None else 0
    return o


def keep_of(n, step):
    """int32 [n] with about a fifth of the entries 0."""
    gen = torch.Generator().manual_seed(500 + step)
    return (torch.rand(n, generator=gen) >= 0.2).to(torch.int32)


# ---- the fused step's inputs
@functools.lru_cache(maxsize=16)
def fused_inputs(dtype, W, step, shape="small"):
    """(query [nq, W] f32, idx [nq, n_neg] int64, d_out [nq, n_neg] f32, extra ids [n] int64, extra gradients [n, W]) of
    one step; never written to.  small: 5 x 37 over the rows of `ref_list`'s pools; hot: 16 x 37 with 520 references on
    row 41; win: 4096 x 2."""
    gen = torch.Generator().manual_seed(10_000 * step + 10 * W + (5 if dtype == F16 else 0) + len(shape))
    nq, n_neg = dict(small=(NQ, N_NEG), hot=(16, 37), win=(4096, 2))[shape]
    pool = [r for r in range(ROWS) if r not in NEVER and (step != 2 or r not in ONLY13)]
    pool = torch.tensor(pool)
    idx = pool[torch.randint(0, len(pool) - 12, (nq * n_neg,), generator=gen)]  # the pool's last 12 rows: extras only
    if shape == "hot":
        idx[torch.randperm(nq * n_neg, generator=gen)[:520]] = 41
    if step != 2:
        idx[:5] = torch.tensor(ONLY13[:5])
    xidx = pool[torch.randint(len(pool) - 30, len(pool), (N_EXTRA,), generator=gen)]  # 18 rows shared with idx, 12 not
    xidx[0] = 41 if shape == "hot" else int(idx[7])
    if step != 2:
        xidx[1:4] = torch.tensor(ONLY13[5:8])  # orphans of steps 1 and 3
    query = torch.randn(nq, W, generator=gen) * 0.3
    d_out = torch.randn(nq, n_neg, generator=gen)
    xgrad = torch.randn(N_EXTRA, W, generator=gen)
    return query, idx.reshape(nq, n_neg), d_out, xidx, xgrad


def fused_gradient(red, table, query, idx, d_out, xidx, xgrad, dtype):
    """(touched rows, their gradient): `index_add_` of the K5 rule's row gradients plus the extras - in float64, or in
    float32 in reversed reference order."""
    M, W = table.shape
    flat = idx.reshape(-1)
    dn = ptk.rule(red, query, table[flat].reshape(*idx.shape, W), d_out, dtype)[2].reshape(-1, W)
    rows = torch.unique(torch.cat([flat, xidx]))
    out = torch.zeros(M, W, dtype=dtype)
    if dtype == F64:
        out.index_add_(0, flat, dn).index_add_(0, xidx, xgrad.double())
    else:
        out.index_add_(0, flat.flip(0), dn.flip(0).contiguous()).index_add_(0, xidx.flip(0), xgrad.flip(0).contiguous())
    return rows, out[rows]


# ---- CPU tests
def _dense_torch(opt_cls, opt, **kw):
    hp = {k: float(np.float32(v)) for k, v in OPTS[opt].items() if k != "kind"}
    gen = torch.Generator().manual_seed(1)
    p0 = torch.randn(13, 7, generator=gen)
    param = torch.nn.Parameter(p0.double().clone())
    tor = opt_cls([param], lr=hp["lr"], **{k: hp[v] for k, v in kw.items()})
    p, s1, s2 = p0.double(), torch.zeros(13, 7, dtype=F64), torch.zeros(13, 7, dtype=F64)
    for step in range(1, 4):
        g = torch.randn(13, 7, generator=gen)
        param.grad = g.double().clone()
        tor.step()
        p, s1, s2 = update_rule(opt, None, step, p, g, s1, s2)
        torch.testing.assert_close(p, param.detach(), rtol=1e-12, atol=1e-12)
    assert float((p - p0.double()).abs().min()) > 0
    return tor, param, s1


def test_update_rule_equals_torch_optim_sgd_and_adagrad_in_float64():
    """Every row touched in every step, where lazy and dense coincide."""
    tor, param, s1 = _dense_torch(torch.optim.SGD, "sgdm", momentum="momentum", weight_decay="weight_decay")
    torch.testing.assert_close(s1, tor.state[param]["momentum_buffer"], rtol=1e-12, atol=1e-12)
    tor, param, s1 = _dense_torch(torch.optim.Adagrad, "adagrad", weight_decay="weight_decay", eps="eps")
    torch.testing.assert_close(s1, tor.state[param]["sum"], rtol=1e-12, atol=1e-12)


def test_update_rule_equals_sparse_adam_in_float64():
    """Lazy Adam: rows come and go over three steps; the decoupled decay by its closed form."""
    hp = {k: float(np.float32(v)) for k, v in OPTS["adam"].items() if k != "kind"}
    gen = torch.Generator().manual_seed(2)
    p0 = torch.randn(13, 7, generator=gen)
    param = torch.nn.Parameter(p0.double().clone())
    tor = torch.optim.SparseAdam([param], lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"])
    p, s1, s2 = p0.double(), torch.zeros(13, 7, dtype=F64), torch.zeros(13, 7, dtype=F64)
    for step, rows in ((1, [0, 3, 4, 9]), (2, [3, 5, 9, 12]), (3, [0, 3, 11])):
        rows = torch.tensor(rows)
        g = torch.randn(rows.numel(), 7, generator=gen)
        param.grad = torch.sparse_coo_tensor(rows[None], g.double(), (13, 7))
        tor.step()
        p[rows], s1[rows], s2[rows] = update_rule("adam", None, step, p[rows], g, s1[rows], s2[rows])
        torch.testing.assert_close(p, param.detach(), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(s1, tor.state[param]["exp_avg"], rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(s2, tor.state[param]["exp_avg_sq"], rtol=1e-12, atol=1e-12)
    assert torch.equal(p[[1, 2, 6, 7, 8, 10]], p0.double()[[1, 2, 6, 7, 8, 10]])
    # AdamW: the moments do not see the decay, the parameter loses lr wd p first
    s1c, s2c = carried_state(13, 7)
    g = torch.randn(13, 7, generator=gen)
    plain = update_rule(None, dict(OPTS["adamw"], weight_decay=0.0), 5, p0, g, s1c, s2c)
    decay = update_rule("adamw", None, 5, p0, g, s1c, s2c)
    lr, wd = (float(np.float32(OPTS["adamw"][k])) for k in ("lr", "weight_decay"))
    torch.testing.assert_close(decay[0], plain[0] - lr * wd * p0.double(), rtol=1e-12, atol=1e-14)
    assert torch.equal(decay[1], plain[1]) and torch.equal(decay[2], plain[2])


def test_class_of_every_width():
    for path, widths in SUM_WIDTHS.items():
        for W in widths:
            assert sum_class(W) == (path, SUM_PASSES[W])
    assert {sum_class(W)[1] for W in SUM_WIDTHS["float4"]} == {1, 2, 3}
    assert {sum_class(W)[1] for W in SUM_WIDTHS["scalar"]} == {1, 2, 3, 5}
    assert all(sum_class(W) == (("float4" if W % 4 == 0 else "scalar"), SUM_PASSES[W]) for W in DIRECT_WIDTHS)
    assert {sum_class(W)[0] for W in DIRECT_WIDTHS} == {"float4", "scalar"}
    # grid-stride rounds: one everywhere but in the cases built for two
    for step in (1, 2, 3):
        idx = ref_list(step)
        counts = torch.unique(idx, return_counts=True)[1]
        assert idx.numel() == 300 and set(counts.tolist()) == set(LENGTHS) | {37}
        assert int((idx == idx[-1]).sum()) == 1 and not set(idx.tolist()) & set(NEVER)
        assert set(ONLY13) <= set(idx.tolist()) if step != 2 else not set(idx.tolist()) & set(ONLY13)
        assert wave_rounds(counts.numel(), min(300, ROWS)) == 1
        assert all(element_rounds(counts.numel(), min(300, ROWS), W) == 1 for W in APPLY_WIDTHS)
    assert sum(COUNTS) == 299 and all(sum(s) == 300 for s in SPLITS.values()) and max(SPLITS) == nat.MAX_ROW_LISTS
    assert 1 in SPLITS[8] and 0 in SPLITS[8][1:-1]
    big = big_list()
    assert big.numel() > nat.SMALL_INDEX_MAX and torch.unique(big).numel() == BIG_ROWS
    assert wave_rounds(BIG_ROWS, BIG_ROWS + 1) == 2
    assert element_rounds(BIG_APPLY[0], BIG_APPLY[0], BIG_APPLY[1]) == 2
    assert [axpy_class(n) for n in AXPY_SIZES] == [(1, 1), (1, 4), (2, 3), (256, 5)]
    # the fused step: (VEC, IT, windows) of every width
    seen = set()
    for (dtype, vec), its in ptk.CLASS_WIDTHS.items():
        for it, widths in its.items():
            assert (dtype, widths[0]) in FUSED_WIDTHS and ptk.dispatch_class(dtype, widths[0]) == [(vec, it, widths[0])]
            seen.add((dtype, vec, it))
    assert len(seen) == 25
    for dtype, W in ptk.FULL_WIDTHS:
        assert (dtype, W) in FUSED_WIDTHS and ptk.dispatch_class(dtype, W)[0][1] == 16
    for (dtype, W), windows in ptk.WINDOW_WIDTHS.items():
        assert (dtype, W) in FUSED_WIDTHS and [c for _, _, c in ptk.dispatch_class(dtype, W)] == windows
    assert len(FUSED_WIDTHS) == 25 + 2 + 6
    for case in FUSED_ALL_OPTS + FUSED_L2 + HOT:
        assert case in FUSED_WIDTHS and len(ptk.dispatch_class(*case)) == 1
    for dtype, W, n_conc in L2_WINDOWS:  # the host code's rule (csrc/segments.hip), as test_segments_l2_windows
        unit = 16 * ptk.dispatch_class(dtype, W)[0][0]
        win = (4 << 20) // (4096 * 4) // unit * unit
        assert 4096 * W * 4 > (4 << 20) and (n_conc == 2) == (2 * win == W and W % (2 * unit) == 0)
    for step in (1, 2, 3):
        for shape in ("small", "hot"):
            _, idx, _, xidx, _ = fused_inputs(F32, 6, step, shape)
            both, segs, extras = set(idx.reshape(-1).tolist()) & set(xidx.tolist()), set(idx.reshape(-1).tolist()), set(xidx.tolist())
            assert both and extras - segs and segs - extras and not (segs | extras) & set(NEVER)
            assert bool(set(ONLY13) & segs) == (step != 2) and bool(set(ONLY13) & (extras - segs)) == (step != 2)
            assert (int((idx == 41).sum()) > 2 * nat.SEGMENT_CAP) == (shape == "hot")


def _simulate(opt, dtype, M, W, steps):
    """Three steps carried by the float32 restatement in place of the device: the restatement's largest error in units
    of the bound.  `steps`: [(rows, g64, g32) or a function of the table -> that]."""
    state = (table_of(dtype, M, W), *zero_state(M, W))
    worst = 0.0
    for t, step in enumerate(steps, start=1):
        rows, g64, g32 = step(state[0]) if callable(step) else step
        w64, w32, _ = expected(opt, dtype, t, state, rows, g64, g32)
        slack = half_ulp16(w64[0]) if dtype == F16 else None
        worst = max([worst, units(w32[0], w64[0], slack)] + [units(w32[k], w64[k]) for k in (1, 2)])
        state = tuple(x.clone() for x in state)
        state[0][rows] = w32[0].to(dtype)
        state[1][rows], state[2][rows] = w32[1], w32[2]
    return worst


@pytest.mark.parametrize("opt", list(OPTS))
def test_restatement_is_inside_the_bound_on_the_list_cases(opt):
    """The condition that keeps the widening rule from hiding a failure: on the "normal" inputs of the GPU tests the
    float32 restatement (sums in reversed order) is within one unit of the bound, for every width and optimiser."""
    for dtype in (F32, F16):
        for W in sorted(set(ALL_SUM_WIDTHS + APPLY_WIDTHS + DIRECT_WIDTHS)):
            steps = []
            for t in (1, 2, 3):
                idx, src = ref_list(t), list_gradients(W, t)
                rows, g64 = sums_of(idx, src, ROWS)
                steps.append((rows, g64, sums_of(idx, src, ROWS, F32)[1]))
                assert units(steps[-1][2], g64) <= 1.0
            assert not torch.equal(steps[0][2], torch.zeros(ROWS, W).index_add_(0, ref_list(1), list_gradients(W, 1))[steps[0][0]]) \
                or W < 4, "the restatement sums in another order than the kernels"
            e = _simulate(opt, dtype, ROWS, W, steps)
            assert e <= 1.0, f"{opt} {tname(dtype)} W={W}: restatement at {e:.3g} x the bound"


def _fused_steps(red, dtype, W, shape):
    def step(t):
        def gradient(table):
            ins = fused_inputs(dtype, W, t, shape)
            rows, g64 = fused_gradient(red, table, *ins, F64)
            return rows, g64, fused_gradient(red, table, *ins, F32)[1]
        return gradient
    return [step(t) for t in (1, 2, 3)]


@pytest.mark.parametrize("case", FUSED_WIDTHS, ids=ptk.wid)
def test_restatement_is_inside_the_bound_on_the_fused_cases(case):
    dtype, W = case
    for red in ["dot", "l1"] + (["l2"] if case in FUSED_L2 else []):
        for opt in (list(OPTS) if case in FUSED_ALL_OPTS else ["adamw"]):
            e = _simulate(opt, dtype, ROWS, W, _fused_steps(red, dtype, W, "small"))
            assert e <= 1.0, f"{opt} {tname(dtype)} W={W} {red}: restatement at {e:.3g} x the bound"
    if case in HOT:
        for red in ("dot", "l1", "l2"):
            e = _simulate("adamw", dtype, ROWS, W, _fused_steps(red, dtype, W, "hot"))
            assert e <= 1.0, f"adamw {tname(dtype)} W={W} {red} hot row: restatement at {e:.3g} x the bound"


@pytest.mark.parametrize("case", L2_WINDOWS, ids=ptk.wid)
def test_restatement_is_inside_the_bound_on_the_window_cases(case):
    dtype, W, _ = case
    for red in ("dot", "l1"):
        e = _simulate("adamw", dtype, ROWS, W, _fused_steps(red, dtype, W, "win"))
        assert e <= 1.0, f"adamw {tname(dtype)} W={W} {red} 4096 queries: restatement at {e:.3g} x the bound"


# ============================================================================================ 1. sums
def nan(*shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def split(x, sizes):
    return list(torch.split(x, sizes))


def sum_rows(dev, src, seg):
    """bess_segment_sum_rows into a NaN-filled [max_seg, W]."""
    out = nan(seg.max_seg, src.shape[1], dev=dev)
    nat._launch("bess_segment_sum_rows", dev, int(src.shape[1]), src.data_ptr(), seg.refs.data_ptr(),
                seg.seg_offsets.data_ptr(), seg.n_seg.data_ptr(), seg.max_seg, out.data_ptr())
    return out


def coalesced_sums(dev, W, seg, grads):
    """bess_coalesced_update with sum_out: a NaN-filled [max_seg, W]; o, table and state NULL, as the header allows."""
    out = nan(seg.max_seg, W, dev=dev)
    ptrs = (nat._vp * len(grads))(*[g.data_ptr() if g.numel() else None for g in grads])
    rows = (nat._i64 * len(grads))(*[int(g.shape[0]) for g in grads])
    nat._launch("bess_coalesced_update", dev, None, nat.F32, W, None, len(grads), ptrs, rows, seg.refs.data_ptr(),
                seg.seg_rows.data_ptr(), seg.seg_offsets.data_ptr(), seg.n_seg.data_ptr(), seg.max_seg, None, None,
                None, out.data_ptr())
    return out


def sums_against_float64(dev, W, idx, src, M, splits, what):
    seg = nat.SegmentIndex(idx.to(torch.int32).to(dev), M)
    n_seg = int(seg.n_seg.item())
    rows, want64 = sums_of(idx, src, M)
    want32 = sums_of(idx, src, M, F32)[1]
    assert n_seg == rows.numel() and torch.equal(seg.seg_rows[:n_seg].cpu().long(), rows)
    ordered = sum_in_reference_order(src, seg.refs.cpu(), seg.seg_offsets.cpu(), n_seg)
    d_src = src.to(dev)
    outs = [("segment_sum_rows", sum_rows(dev, d_src, seg))]
    for sizes in splits:
        outs.append((f"coalesced_update of {len(sizes)} lists", coalesced_sums(dev, W, seg, split(d_src, sizes))))
    torch.cuda.synchronize()
    for name, out in outs:
        assert bool(torch.isnan(out[n_seg:]).all()), f"{what} {name}: rows past n_seg written"
        got = out[:n_seg].cpu()
        check(("sums", "-", "f32"), f"{what} {name}", got, want64, want32)
        assert torch.equal(got, ordered), f"{what} {name}: not the float32 sum in reference order"
    return seg


@gpu
@pytest.mark.parametrize("W", ALL_SUM_WIDTHS)
def test_sums_equal_float64_and_the_ordered_float32_sum(dev, W):
    for step in (1, 2):
        sums_against_float64(dev, W, ref_list(step), list_gradients(W, step), ROWS, list(SPLITS.values()),
                             f"sums W={W} index {step}")


@gpu
def test_sums_grid_stride_over_17000_rows(dev):
    idx = big_list()
    n = idx.numel()
    seg = sums_against_float64(dev, 4, idx, list_gradients(4, 0, n), BIG_ROWS + 1, [[n], [n // 2, 0, n - n // 2]],
                               "sums W=4 17000 rows")
    assert wave_rounds(int(seg.n_seg.item()), seg.max_seg) == 2


@gpu
def test_sums_of_cancelling_rows_and_of_a_single_reference(dev):
    """+x and -x on one row: exactly 0 in any order; an index of one reference has one segment."""
    for W in (4, 3):
        x = list_gradients(W, 9, 3)
        src = torch.cat([x[:1], x[1:2], -x[:1], x[2:]])
        idx = torch.tensor([5, 2, 5, 2])
        seg = sums_against_float64(dev, W, idx, src, ROWS, [[4], [1, 3]], f"sums W={W} +x -x")
        assert int(seg.n_seg.item()) == 2
        assert float(sum_rows(dev, src.to(dev), seg)[1].abs().max()) == 0.0  # row 5
        seg = sums_against_float64(dev, W, idx[:1], src[:1], ROWS, [[1]], f"sums W={W} one reference")
        assert int(seg.n_seg.item()) == 1 and seg.max_seg == 1


# ============================================================================================ 2. updates
def guarded(rows, W, dev, fill):
    """A [rows, W] f32 state table with one row of 12345 in front of it and one behind (a write for state row -1 or
    `rows` lands there, in bounds): (the whole buffer, the table as a view of it)."""
    buf = torch.full((rows + 2, W), 12345.0, dtype=torch.float32, device=dev)
    buf[1: rows + 1] = fill.to(dev)
    return buf, buf[1: rows + 1]


def guards_intact(buf):
    return float(buf[0].min()) == 12345.0 == float(buf[0].max()) and float(buf[-1].min()) == 12345.0 == float(buf[-1].max())


def snapshot(*tensors):
    torch.cuda.synchronize()
    return tuple(t.cpu().clone() for t in tensors)


class Run:
    """Table and state of one (entry point, optimiser, dtype, W) on the device, judged step by step."""

    def __init__(self, dev, entry, opt, dtype, M, W, state=None, slots=None, state_rows=None):
        self.dev, self.entry, self.opt, self.dtype, self.M, self.W = dev, entry, opt, dtype, M, W
        self.table = table_of(dtype, M, W).to(dev)
        n = M if state_rows is None else state_rows
        state = zero_state(n, W) if state is None else state
        (self.buf1, self.s1), (self.buf2, self.s2) = (guarded(n, W, dev, s) for s in state)
        self.slot_map = slots  # int32 [M] on the device, or None
        self.before = snapshot(self.table, self.s1, self.s2)

    def desc(self, step, step_ptr=None):
        return opt_desc(self.opt, step, step_ptr, self.slot_map)

    def judge(self, what, step, rows, g64, g32):
        after = snapshot(self.table, self.s1, self.s2)
        slots = self.slot_map.cpu() if self.slot_map is not None else None
        w32 = judge(self.entry, self.opt, self.dtype, f"{self.entry} {self.opt} {tname(self.dtype)} W={self.W} {what}", step,
                    self.before, after, rows, g64, g32, slots)
        assert guards_intact(self.buf1) and guards_intact(self.buf2), f"{what}: a state row outside the table was written"
        self.before = after
        return after, w32


def list_step(run, step, n_lists, use_keep=True, entry=None, idx=None, src=None, step_ptr=None, rule_step=None):
    """One step of apply_segments_opt (its gradient rows: the float32 sums in reference order, exact inputs of the
    kernel) or of coalesced_update (n_lists lists) on the 300 references of `step`."""
    dev, W, M = run.dev, run.W, run.M
    idx = ref_list(step) if idx is None else idx
    src = list_gradients(W, step, idx.numel()) if src is None else src
    seg = nat.SegmentIndex(idx.to(torch.int32).to(dev), M)
    n_seg = int(seg.n_seg.item())
    rows, g64 = sums_of(idx, src, M)
    g32 = sums_of(idx, src, M, F32)[1]
    assert torch.equal(seg.seg_rows[:n_seg].cpu().long(), rows)
    keep = torch.ones(seg.max_seg, dtype=torch.int32)
    if use_keep:
        keep[:n_seg] = keep_of(n_seg, step)
        assert 0 < int(keep[:n_seg].sum()) < n_seg
    kept = keep[:n_seg].bool()
    o = run.desc(step, step_ptr)
    if (entry or run.entry) == "apply_segments_opt":
        gseg = nan(seg.max_seg, W, dev=dev)
        ordered = sum_in_reference_order(src, seg.refs.cpu(), seg.seg_offsets.cpu(), n_seg)
        gseg[:n_seg] = ordered.to(dev)
        nat.apply_segments_opt(o, run.table, seg, gseg, run.s1, run.s2, keep=keep.to(dev) if use_keep else None)
        g64, g32 = ordered.double(), ordered  # the kernel's input is this gradient, exactly
    else:
        grads = split(src.to(dev), SPLITS[n_lists] if idx.numel() == 300 else [idx.numel()])
        nat.coalesced_update(o, run.table, seg, grads, run.s1, run.s2, keep=keep.to(dev) if use_keep else None)
    return run.judge(f"step {step}", rule_step or step, rows[kept], g64[kept], g32[kept])


@gpu
@pytest.mark.parametrize("dtype", [F32, F16], ids=tname)
@pytest.mark.parametrize("W", APPLY_WIDTHS)
def test_apply_segments_opt_equals_the_rule(dev, W, dtype):
    for opt in OPTS:
        run = Run(dev, "apply_segments_opt", opt, dtype, ROWS, W)
        for step in (1, 2, 3):
            list_step(run, step, 1)


@gpu
@pytest.mark.parametrize("dtype", [F32, F16], ids=tname)
def test_apply_segments_opt_grid_stride(dev, dtype):
    """1100 segments x 1024 columns: more than the 4096 x 256 elements of one round of the flat loop."""
    n, W = BIG_APPLY
    gen = torch.Generator().manual_seed(11)
    idx = torch.randperm(n + 50, generator=gen)[:n]
    run = Run(dev, "apply_segments_opt", "adamw", dtype, n + 50, W, state=carried_state(n + 50, W))
    after, _ = list_step(run, 2, 1, idx=idx, src=list_gradients(W, 5, n))
    assert element_rounds(n, n, W) == 2


@gpu
@pytest.mark.parametrize("dtype", [F32, F16], ids=tname)
@pytest.mark.parametrize("W", ALL_SUM_WIDTHS)
def test_coalesced_update_equals_the_rule(dev, W, dtype):
    """Steps 1, 2, 3 through 1, 3 and 8 lists."""
    for opt in OPTS:
        run = Run(dev, "coalesced_update", opt, dtype, ROWS, W)
        for step, n_lists in ((1, 1), (2, 3), (3, 8)):
            list_step(run, step, n_lists)


@gpu
def test_coalesced_update_grid_stride_over_17000_rows(dev):
    idx = big_list()
    run = Run(dev, "coalesced_update", "adamw", F32, BIG_ROWS + 1, 4, state=carried_state(BIG_ROWS + 1, 4))
    list_step(run, 2, 1, idx=idx, src=list_gradients(4, 0, idx.numel()))


def axpy_operands(dev, dtype, n):
    gen = torch.Generator().manual_seed(n)
    t2 = torch.randn(n, generator=gen).to(dtype)
    g2 = torch.randn(n, generator=gen)
    # T(t + alpha g) of the exact sum (exact in float64: alpha g is, and the operands are at most 2^49 apart), rounded
    # ONCE - by numpy, whose float64 -> float16 conversion is direct; torch's goes through float32, which rounds an
    # exact value just off an f16 tie onto it and then to even (16 of the 300 001 elements here)
    exact = (t2.double() + AXPY_ALPHA * g2.double()).numpy()
    want = torch.from_numpy(exact.astype(np.float16 if dtype == F16 else np.float32))
    return t2, g2, want, t2.to(dev), g2.to(dev)


@gpu
@pytest.mark.parametrize("dtype", [F32, F16], ids=tname)
@pytest.mark.parametrize("n", AXPY_SIZES)
def test_axpy_job_of_both_updates(dev, n, dtype):
    """`table2 += alpha grad2` in the last workgroups of bess_coalesced_update_axpy and bess_direct_update:
    T(float(t) + alpha g) exactly - the exact sum, rounded once -, the main update unchanged by the job."""
    W = 4
    idx, src = ref_list(1), list_gradients(W, 1)
    rows, g64 = sums_of(idx, src, ROWS)
    g32 = sums_of(idx, src, ROWS, F32)[1]
    t2, g2, want, d_t2, d_g2 = axpy_operands(dev, dtype, n)
    run = Run(dev, "coalesced_update", "sgdm", dtype, ROWS, W)
    seg = nat.SegmentIndex(idx.to(torch.int32).to(dev), ROWS)
    nat.coalesced_update(run.desc(1), run.table, seg, split(src.to(dev), SPLITS[3]), run.s1, run.s2,
                         axpy=(d_t2, d_g2, AXPY_ALPHA))
    run.judge(f"with axpy of {n}", 1, rows, g64, g32)
    assert torch.equal(d_t2.cpu(), want), "coalesced_update: axpy result"
    d_t2 = t2.to(dev)
    run = Run(dev, "direct_update", "sgdm", dtype, ROWS, W)
    scratch = nat.DirectAccumulator(run.table)
    scratch.acc.index_add_(0, idx.to(dev), src.to(dev))
    nat.step_prologue([scratch.increment_job()])
    nat.direct_update(run.desc(1), run.table, [idx.to(torch.int32).to(dev)], scratch, run.s1, run.s2,
                      axpy=(d_t2, d_g2, AXPY_ALPHA))
    run.judge(f"with axpy of {n}", 1, rows, g64, g32)
    assert torch.equal(d_t2.cpu(), want), "direct_update: axpy result"


@gpu
@pytest.mark.parametrize("dtype", [F32, F16], ids=tname)
@pytest.mark.parametrize("W", DIRECT_WIDTHS)
def test_direct_update_equals_the_rule(dev, W, dtype):
    """The accumulator is filled by torch's `index_add_` on the device: `k_direct_update` is the only native kernel in
    the path.  Two steps on one DirectAccumulator, through 1, 3 or 8 id lists with duplicates inside and across them."""
    for n_opt, opt in enumerate(OPTS):
        run = Run(dev, "direct_update", opt, dtype, ROWS, W)
        scratch = nat.DirectAccumulator(run.table)
        claim = torch.zeros(ROWS, dtype=torch.int32)
        for step in (1, 2):
            idx, src = ref_list(step), list_gradients(W, step)
            rows, g64 = sums_of(idx, src, ROWS)
            g32 = sums_of(idx, src, ROWS, F32)[1]
            lists = split(idx.to(torch.int32).to(dev), SPLITS[(1, 3, 8)[(n_opt + step) % 3]])
            scratch.acc.index_add_(0, idx.to(dev), src.to(dev))
            nat.step_prologue([scratch.increment_job()])
            nat.direct_update(run.desc(step), run.table, lists, scratch, run.s1, run.s2)
            run.judge(f"step {step}", step, rows, g64, g32)
            assert int(scratch.generation) == step + 1
            assert float(scratch.acc.abs().max()) == 0.0, "acc is not left zero"
            claim[rows] = step + 1
            assert torch.equal(scratch.claim.cpu(), claim), "claim: the generation on the touched rows, and only there"
    o = run.desc(3)
    o.slot_map = scratch.claim.data_ptr()
    with pytest.raises(RuntimeError, match="paged"):
        nat.direct_update(o, run.table, lists, scratch, run.s1, run.s2)


# ---- the fused step
def fused_step(run, red, step, shape="small", step_ptr=None, rule_step=None, assign=None, inputs=None):
    """One step of bess_neg_pertriple_step_segments with extras (`bess_map_extra_rows`), the orphan extras through
    bess_apply_segments_opt(keep).  `assign` = (counter, capacity): paged state, slots handed out first."""
    dev, W, M, dtype = run.dev, run.W, run.M, run.dtype
    query, idx, d_out, xidx, xgrad = inputs or fused_inputs(dtype, W, step, shape)
    nq, n_neg = idx.shape
    table = run.before[0]
    rows, g64 = fused_gradient(red, table, query, idx, d_out, xidx, xgrad, F64)
    g32 = fused_gradient(red, table, query, idx, d_out, xidx, xgrad, F32)[1]
    desc = ptk.make_desc(red, run.table)
    seg = nat.SegmentIndex(idx.reshape(-1).to(torch.int32).to(dev), M, width=W)
    xseg = nat.SegmentIndex(xidx.to(torch.int32).to(dev), M)
    xsum = nat.segment_sum_rows(xgrad.to(dev), xseg)
    xmap, keep = nat.map_extra_rows(seg, xseg)
    n, nx = int(seg.n_seg.item()), int(xseg.n_seg.item())
    srows, xrows = seg.seg_rows[:n].cpu().tolist(), xseg.seg_rows[:nx].cpu().tolist()
    assert srows == sorted(set(idx.reshape(-1).tolist())) and xrows == sorted(set(xidx.tolist()))
    assert xmap[:n].cpu().tolist() == [xrows.index(r) if r in xrows else -1 for r in srows], "xmap"
    assert keep[:nx].cpu().tolist() == [0 if r in srows else 1 for r in xrows], "keep"
    assert 0 < int(keep[:nx].sum()) < nx and int((xmap[:n] >= 0).sum()) < n
    assert int(seg.long_segs[0].item()) == (1 if shape == "hot" else 0)
    if assign is not None:
        nat.assign_state_rows(seg, run.slot_map, assign[0], assign[1])
        nat.assign_state_rows(xseg, run.slot_map, assign[0], assign[1], keep=keep)
    o = run.desc(step, step_ptr)
    nat.neg_pertriple_step_segments(desc, query.to(dev), run.table, n_neg, d_out.to(dev), seg, o, run.s1, run.s2, xmap, xsum)
    nat.apply_segments_opt(o, run.table, xseg, xsum, run.s1, run.s2, keep=keep)
    return run.judge(f"{red} {shape} step {step}", rule_step or step, rows, g64, g32)


@gpu
@pytest.mark.parametrize("case", FUSED_WIDTHS, ids=ptk.wid)
def test_fused_step_equals_the_rule(dev, case):
    dtype, W = case
    windows = len(ptk.dispatch_class(dtype, W))
    reds = ["dot", "l1"] + (["l2"] if case in FUSED_L2 else [])
    for red in reds:
        for opt in (list(OPTS) if case in FUSED_ALL_OPTS else ["adamw"]):
            run = Run(dev, "step_segments", opt, dtype, ROWS, W)
            for step in (1, 2, 3):
                fused_step(run, red, step)
    if windows > 1:  # the p = 2 norm needs the whole row: refused, nothing written
        run = Run(dev, "step_segments", "adamw", dtype, ROWS, W)
        query, idx, d_out, _, _ = fused_inputs(dtype, W, 1)
        seg = nat.SegmentIndex(idx.reshape(-1).to(torch.int32).to(dev), ROWS, width=W)
        with pytest.raises(RuntimeError):
            nat.neg_pertriple_step_segments(ptk.make_desc("l2", run.table), query.to(dev), run.table, N_NEG,
                                            d_out.to(dev), seg, run.desc(1), run.s1, run.s2)
        assert all(torch.equal(a, b) for a, b in zip(snapshot(run.table, run.s1, run.s2), run.before))


@gpu
@pytest.mark.parametrize("case", HOT, ids=ptk.wid)
def test_fused_step_hot_row(dev, case):
    """520 references on row 41 (> SEGMENT_CAP): the long tier's `seg_finish` with an optimiser and an extra."""
    dtype, W = case
    for red in ("dot", "l1", "l2"):
        run = Run(dev, "step_segments", "adamw", dtype, ROWS, W)
        for step in (1, 2, 3):
            fused_step(run, red, step, "hot")


@gpu
@pytest.mark.parametrize("case", L2_WINDOWS, ids=ptk.wid)
def test_fused_step_l2_windows(dev, case):
    """4096 queries: two windows side by side in one launch (n_conc = 2: state, xsum and table shifted inside the
    kernel), or three one after the other (shifted by the host)."""
    dtype, W, n_conc = case
    for red in ("dot", "l1"):
        run = Run(dev, "step_segments", "adamw", dtype, ROWS, W)
        for step in (1, 2, 3):
            fused_step(run, red, step, "win")


# ---- device-side step count
@gpu
@pytest.mark.parametrize("count", [1, 2, 1000])
def test_step_count_on_the_device(dev, count):
    """o.step_ptr -> an int32 on the device, o.step = 0: the bias corrections are those of that count."""
    ptr = torch.full((1,), count, dtype=torch.int32, device=dev)
    for dtype, W in ((F32, 48), (F16, 257)):
        for entry in ("apply_segments_opt", "coalesced_update"):
            run = Run(dev, entry, "adamw", dtype, ROWS, W, state=carried_state(ROWS, W))
            o = run.desc(0, ptr)
            assert o.step == 0 and o.step_ptr == ptr.data_ptr()
            list_step(run, 0, 3, step_ptr=ptr, rule_step=count, idx=ref_list(1), src=list_gradients(W, 1))
    for dtype, W, shape in ((F32, 132, "small"), (F16, 264, "hot"), (F32, 257, "small")):
        run = Run(dev, "step_segments", "adamw", dtype, ROWS, W, state=carried_state(ROWS, W))
        fused_step(run, "dot", 0, shape, step_ptr=ptr, rule_step=count, inputs=fused_inputs(dtype, W, 1, shape))


# ---- paged state
@gpu
def test_assign_state_rows(dev):
    idx = ref_list(1)
    seg = nat.SegmentIndex(idx.to(torch.int32).to(dev), ROWS)
    n = int(seg.n_seg.item())
    rows = seg.seg_rows[:n].cpu().long()
    # room for everyone: distinct slots in [0, capacity); owners keep theirs; keep == 0 rows get none
    slot_map = torch.full((ROWS,), -1, dtype=torch.int32, device=dev)
    slot_map[rows[:3]] = torch.tensor([70, 71, 72], dtype=torch.int32, device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    keep = torch.ones(seg.max_seg, dtype=torch.int32)
    keep[[1, 5, 6]] = 0
    nat.assign_state_rows(seg, slot_map, counter, 64, keep=keep.to(dev))
    got = slot_map.cpu()
    assert got[rows[:3]].tolist() == [70, 71, 72]
    assert got[rows[5]] == -1 and got[rows[6]] == -1
    fresh = got[rows[3:]][keep[3:n].bool()]
    assert sorted(fresh.tolist()) == list(range(n - 5)) and int(counter) == n - 5
    untouched = torch.ones(ROWS, dtype=torch.bool)
    untouched[rows] = False
    assert bool((got[untouched] == -1).all())
    nat.assign_state_rows(seg, slot_map, counter, 64, keep=keep.to(dev))
    assert torch.equal(slot_map.cpu(), got) and int(counter) == n - 5
    # more rows than slots: exactly `capacity` owners, the rest at -1, counter > capacity; a second call changes nothing
    for capacity in (40, n - 1):
        slot_map = torch.full((ROWS,), -1, dtype=torch.int32, device=dev)
        counter = torch.zeros(1, dtype=torch.int32, device=dev)
        nat.assign_state_rows(seg, slot_map, counter, capacity)
        got, count = slot_map.cpu(), int(counter)
        assert sorted(got[got >= 0].tolist()) == list(range(capacity)) and bool((got[untouched] == -1).all())
        assert capacity < count <= n
        nat.assign_state_rows(seg, slot_map, counter, capacity)
        assert torch.equal(slot_map.cpu(), got) and int(counter) == count


@gpu
@pytest.mark.parametrize("capacity", [90, 40])
@pytest.mark.parametrize("dtype", [F32, F16], ids=tname)
def test_updates_with_paged_state(dev, dtype, capacity):
    """slot_map: the state of row r lands in state row slot_map[r]; state rows of nobody are bit-equal to before; a row
    at -1 (capacity 40: the pool is exhausted in step 1) is stepped exactly as from zero state, and no state row - the
    guard row in front of the pool included - changes on its account."""
    for entry, W in (("apply_segments_opt", 48), ("coalesced_update", 260), ("coalesced_update", 65),
                     ("step_segments", 132 if dtype == F32 else 264), ("step_segments", 257)):
        for opt in ("adamw", "sgdm"):
            slot_map = torch.full((ROWS,), -1, dtype=torch.int32, device=dev)
            counter = torch.zeros(1, dtype=torch.int32, device=dev)
            run = Run(dev, entry, opt, dtype, ROWS, W, state=carried_state(capacity, W), slots=slot_map,
                      state_rows=capacity)
            for step in (1, 2, 3):
                if entry == "step_segments":
                    fused_step(run, "l1", step, assign=(counter, capacity))
                else:
                    seg = nat.SegmentIndex(ref_list(step).to(torch.int32).to(dev), ROWS)
                    nat.assign_state_rows(seg, slot_map, counter, capacity)
                    list_step(run, step, 3, use_keep=False)
            owners = int((slot_map >= 0).sum())
            assert (int(counter) > capacity) == (capacity == 40)
            assert (owners == capacity) == (capacity == 40)


# ---- edges
@gpu
@pytest.mark.parametrize("opt", ["adam", "adagrad"])
def test_a_cancelling_row_takes_the_step_of_a_zero_gradient(dev, opt):
    """+x and -x on one row sum to exactly 0 in any order; a d_out that is 0 for every reference of a row gives it the
    gradient 0: the new row is finite and the rule's at g = 0 (from zero state: the row itself)."""
    for dtype, W in ((F32, 4), (F16, 65)):
        x = list_gradients(W, 9, 3)
        src, idx = torch.cat([x[:1], x[1:2], -x[:1], x[2:]]), torch.tensor([5, 2, 5, 2])
        for entry in ("coalesced_update", "direct_update"):
            run = Run(dev, entry, opt, dtype, ROWS, W)
            if entry == "direct_update":
                scratch = nat.DirectAccumulator(run.table)
                scratch.acc.index_add_(0, idx.to(dev), src.to(dev))
                nat.step_prologue([scratch.increment_job()])
                nat.direct_update(run.desc(1), run.table, [idx.to(torch.int32).to(dev)], scratch, run.s1, run.s2)
                rows, g64 = sums_of(idx, src, ROWS)
                after, _ = run.judge("+x -x", 1, rows, g64, sums_of(idx, src, ROWS, F32)[1])
            else:
                after, _ = list_step(run, 1, 1, use_keep=False, idx=idx, src=src)
            if OPTS[opt]["weight_decay"] == 0.0:
                assert torch.equal(after[0][5], table_of(dtype, ROWS, W)[5])
    dtype, W = F32, 132
    query, idx, d_out, xidx, xgrad = fused_inputs(dtype, W, 1)
    d_out = d_out.clone()
    lone = next(r for r in idx.reshape(-1).tolist() if r not in xidx.tolist())  # a row without an extra
    d_out[idx == lone] = 0.0
    run = Run(dev, "step_segments", opt, dtype, ROWS, W)
    after, _ = fused_step(run, "dot", 1, inputs=(query, idx, d_out, xidx, xgrad))
    assert bool(torch.isfinite(after[0][lone]).all())
    if OPTS[opt]["weight_decay"] == 0.0:
        assert torch.equal(after[0][lone], table_of(dtype, ROWS, W)[lone])


@gpu
@pytest.mark.parametrize("entry", ["direct_update", "step_segments"])
def test_f16_rows_are_rounded_once(dev, entry):
    """Plain SGD on an f16 table, gradients that are small multiples of 2^-10 (their f32 sums are exact in any order):
    the new row is the f16 nearest to the f32 result, i.e. within ONE f16 ulp of the float64 value - on the row of 37
    references a rounding per contribution would be several away."""
    W = 264
    gen = torch.Generator().manual_seed(4)
    run = Run(dev, entry, "sgd", F16, ROWS, W)
    if entry == "direct_update":
        idx = ref_list(1)
        src = torch.randint(-32, 33, (300, W), generator=gen).float() / 1024
        scratch = nat.DirectAccumulator(run.table)
        scratch.acc.index_add_(0, idx.to(dev), src.to(dev))
        nat.step_prologue([scratch.increment_job()])
        nat.direct_update(run.desc(1), run.table, split(idx.to(torch.int32).to(dev), SPLITS[8]), scratch, run.s1, run.s2)
        rows, g64 = sums_of(idx, src, ROWS)
        g32 = sums_of(idx, src, ROWS, F32)[1]
        after, w32 = run.judge("exact sums", 1, rows, g64, g32)
    else:
        query, idx, d_out, xidx, xgrad = fused_inputs(F16, W, 1)
        query = torch.randint(-32, 33, query.shape, generator=gen).float() / 32
        d_out = torch.randint(-32, 33, d_out.shape, generator=gen).float() / 32
        xgrad = torch.randint(-32, 33, xgrad.shape, generator=gen).float() / 1024
        rows, g64 = fused_gradient("dot", run.before[0], query, idx, d_out, xidx, xgrad, F64)
        g32 = fused_gradient("dot", run.before[0], query, idx, d_out, xidx, xgrad, F32)[1]
        after, w32 = fused_step(run, "dot", 1, inputs=(query, idx, d_out, xidx, xgrad))
    assert torch.equal(g32.double(), g64), "the sums of these inputs are exact in float32"
    before = table_of(F16, ROWS, W)
    want64 = update_rule("sgd", None, 1, before[rows], g64, torch.zeros_like(g64), torch.zeros_like(g64))[0]
    off = (after[0][rows].double() - want64).abs() / (2 * half_ulp16(want64))
    assert float(off.max()) <= 1.0, f"{entry}: {float(off.max()):.3g} f16 ulp from the float64 value"
    assert float(off.max()) > 0.0  # (the f16 rounding is there to be seen)


@gpu
def test_print_measured_errors(dev):
    """Last: the largest error per (entry point, optimiser, dtype), in units of the bound - DESIGN.md, section 16."""
    print("\nentry point | optimiser | dtype | fp32 restatement | kernel")
    for (entry, opt, dt), (e32, ek) in sorted(MEASURED.items()):
        print(f"{entry} | {opt} | {dt} | {e32:.3g} | {ek:.3g}")
    print("cases that used the widened bound:", WIDENED or "none")
    assert all(ek <= max(1.0, 4.0 * e32) for e32, ek in MEASURED.values())
