#!/usr/bin/env python3
"""HAKE's candidate kernels against the same computation written in torch on the device, d = 256,
S = 4096, fp32 and fp16 tables; in the style of profiles/bench_boxe_query.py:

  per-triple  256 negatives per query: forward, backward (d_query and d_neg)
  shared      all 93,773 entities: forward (scores), counts (ranks, nothing stored), backward; the kernels' tile form,
              their row form (zero index stride: `BESS_FLAG_FP32_MATH`) and torch, chunked over the queries so that its
              [chunk, N, d] intermediates fit

"torch" is the formula written as plain broadcast torch ops, not a tuned implementation.  The routes of one
measurement alternate inside every repeat; a timed window holds as many calls as fill about `--window-ms` (sized on
the warm-up), and the figure is the window over its calls.  Medians and [min, max] of `--repeats` windows after
`--warmup`; one JSON line per measurement, all of them written to `--out`."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "bess-kge_amd"), REPO]
import torch  # noqa: E402

from besskge import _native as nat  # noqa: E402
from besskge.scoring import HAKE  # noqa: E402
from besskge.sharding import Sharding  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--queries", type=int, default=4096)
ap.add_argument("--entities", type=int, default=93_773)
ap.add_argument("--negatives", type=int, default=256)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--window-ms", type=float, default=50.0)
ap.add_argument("--torch-chunk", type=int, default=16, help="queries per chunk of the torch route over all entities")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_hake.json"))
args = ap.parse_args()

assert torch.cuda.is_available(), "this measurement needs a HIP device"
dev = torch.device("cuda", 0)
S, d, M, K = args.queries, args.size, args.entities, args.negatives
LP, PS = 0.5, 1.0
results = []


def alternate(runs):
    times = {label: [] for label, _ in runs}
    calls = {label: 1 for label, _ in runs}
    for it in range(args.warmup + args.repeats):
        for label, run in runs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls[label]):
                run()
            b.record()
            torch.cuda.synchronize()
            ms = a.elapsed_time(b) / calls[label]
            if it >= args.warmup:
                times[label].append(ms)
            elif it == args.warmup - 1:
                calls[label] = max(1, min(256, int(args.window_ms / max(ms, 1e-3))))
    return times


def measure(runs, **tags):
    for label, v in alternate(runs).items():
        res = dict(tags, route=label, S=S, d=d, ms=round(statistics.median(v), 4),
                   ms_min_max=[round(min(v), 4), round(max(v), 4)], device=torch.cuda.get_device_name(0),
                   repeats=args.repeats)
        print(json.dumps(res), flush=True)
        results.append(res)


def torch_scores(q, rows):
    """q [s, 3 d] f32 against rows [s, n, 2 d] or [n, 2 d] of the table type -> [s, n]"""
    u, r, qp = q.unsqueeze(1).chunk(3, dim=-1)
    cp, cm = rows.float().chunk(2, dim=-1)
    return -(torch.norm(u * cm + r, dim=-1) + LP * torch.sin((qp - PS * cp) / 2).abs().sum(-1))


def torch_chunks(q, table, idx, n, chunk, g=None, thr=None):
    """forward (g, thr None), counts (thr) or backward (g) of all S queries, `chunk` queries at a time"""
    dq, dt = torch.zeros_like(q), torch.zeros(table.shape, dtype=torch.float32, device=dev)
    for s0 in range(0, S, chunk):
        qc = q[s0: s0 + chunk].clone().requires_grad_(g is not None)
        rows = table[idx[s0: s0 + chunk].long()] if idx is not None else table
        if g is not None:
            rows = rows.float().requires_grad_(True)
        sc = torch_scores(qc, rows)
        if thr is not None:
            (sc > thr[s0: s0 + chunk, None]).sum(1)
        if g is not None:
            gq, gr = torch.autograd.grad(sc, [qc, rows], g[s0: s0 + chunk])
            dq[s0: s0 + chunk] = gq
            if idx is None:
                dt += gr
    return dq, dt


gen = torch.Generator().manual_seed(1)
q = torch.cat([torch.randn(S, 2 * d, generator=gen), (torch.rand(S, d, generator=gen) * 2 - 1) * 3.14], -1).to(dev)
own = torch.randint(M, (S, K), generator=gen, dtype=torch.int32).to(dev)
g_own, g_all = torch.randn(S, K, generator=gen).to(dev), torch.randn(S, M, generator=gen).to(dev)
thr = torch.full((S,), -float(d) / 3, device=dev)
excl = torch.full((S,), -1, dtype=torch.int32, device=dev)

for dtype in (torch.float32, torch.float16):
    tag = "f32" if dtype == torch.float32 else "f16"
    torch.manual_seed(0)
    fn = HAKE(True, Sharding.create(M, 1, seed=0), 8, d, phase_weight=LP, phase_scale=PS, device=dev, dtype=dtype)
    table = fn.entity_embedding.data[0]
    table[:, d:] = torch.randn(M, d, device=dev).to(dtype)  # moduli of order 1
    desc = nat.copy_desc(fn.kernel_desc())
    fn.fp32_math = True
    rows_desc = nat.copy_desc(fn.kernel_desc())
    src_own, src_all = nat.RowSource(table, own.reshape(-1)), nat.RowSource(table, None)

    out = nat.neg_score_pertriple_fwd(desc, q, src_own, K)
    print(json.dumps(dict(part="agreement", table=tag, pertriple=float(
        (out[:64] - torch_scores(q[:64], table[own[:64].long()])).abs().max()))), flush=True)
    measure([("hip", lambda: nat.neg_score_pertriple_fwd(desc, q, src_own, K)),
             ("torch", lambda: torch_scores(q, table[own.long()]) if K * S * d * 4 * 6 < 8e9
              else torch_chunks(q, table, own, K, 512))],
            part="per-triple forward", table=tag, negatives=K)
    measure([("hip", lambda: nat.neg_score_pertriple_bwd(desc, q, src_own, K, g_own)),
             ("torch", lambda: torch_chunks(q, table, own, K, 512, g=g_own))],
            part="per-triple backward", table=tag, negatives=K)

    scores = nat.neg_score_shared_fwd(desc, q, src_all)
    measure([("hip tile", lambda: nat.neg_score_shared_fwd(desc, q, src_all)),
             ("hip rows", lambda: nat.neg_score_shared_fwd(rows_desc, q, src_all)),
             ("torch", lambda: torch_chunks(q, table, None, M, args.torch_chunk))],
            part="shared forward", table=tag, entities=M)
    measure([("hip tile", lambda: nat.neg_score_shared_counts(desc, q, src_all, thr, excl)),
             ("hip rows", lambda: nat.neg_score_shared_counts(rows_desc, q, src_all, thr, excl)),
             ("torch", lambda: torch_chunks(q, table, None, M, args.torch_chunk, thr=thr))],
            part="shared counts", table=tag, entities=M)
    measure([("hip tile", lambda: nat.neg_score_shared_bwd(desc, q, src_all, scores, g_all)),
             ("hip rows", lambda: nat.neg_score_shared_bwd(rows_desc, q, src_all, scores, g_all)),
             ("torch", lambda: torch_chunks(q, table, None, M, args.torch_chunk, g=g_all))],
            part="shared backward", table=tag, entities=M)
    del scores

with open(args.out, "w") as fh:
    json.dump(results, fh, indent=1)
