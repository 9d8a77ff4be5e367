#!/usr/bin/env python3
"""BoxE's S-row work on its two routes, d = 256, S = 4096, fp32 and fp16 tables; in the style of
profiles/bench_conve_query.py:

  forward   the hooks `query_fwd` + `triple_fwd` of one step ("torch": gathers, torch ops, an autograd graph; "native":
            csrc/boxe_query.hip), the two routes alternating in one process
  backward  `query_bwd` + `triple_bwd` for fixed dq and d_pos (the torch route's forward runs outside the timed region
            on every repeat: its graph is consumed)
  step      one `EmbeddingMovingBessKGE` training step (plain SGD, per-triple negatives of the own shard, one shard);
            host time included: eager; with the number of native calls of a step on each route

Medians and [min, max] of `--repeats` event pairs after `--warmup`.  Prints one JSON line per measurement and writes
them to `--out`."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "bess-kge_amd"), REPO]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from besskge import _native as nat  # noqa: E402
from besskge import runtime  # noqa: E402
from besskge.bess import EmbeddingMovingBessKGE  # noqa: E402
from besskge.loss import LogSigmoidLoss  # noqa: E402
from besskge.negative_sampler import RandomShardedNegativeSampler  # noqa: E402
from besskge.scoring import BoxE  # noqa: E402
from besskge.sharding import Sharding  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--queries", type=int, default=4096)
ap.add_argument("--entities", type=int, default=50_000)
ap.add_argument("--relations", type=int, default=51)
ap.add_argument("--negatives", type=int, default=16)
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_boxe_query.json"))
args = ap.parse_args()

assert torch.cuda.is_available(), "this measurement needs a HIP device"
dev = torch.device("cuda", 0)
S, d, M = args.queries, 256, args.entities
ROUTES = ("torch", "native")
results = []


def alternate(runs):
    """{label: [ms]}: every run is (label, prepare | None, timed); the labels take turns inside every repeat"""
    times = {label: [] for label, _, _ in runs}
    for it in range(args.warmup + args.repeats):
        for label, prepare, run in runs:
            state = prepare() if prepare else None
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run(state)
            b.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                times[label].append(a.elapsed_time(b))
    return times


def measure(runs, **tags):
    for label, v in alternate(runs).items():
        res = dict(tags, route=label, S=S, d=d, ms=round(statistics.median(v), 4),
                   ms_min_max=[round(min(v), 4), round(max(v), 4)], device=torch.cuda.get_device_name(0),
                   repeats=args.repeats)
        print(json.dumps(res), flush=True)
        results.append(res)


def make(route, dtype):
    torch.manual_seed(0)
    return BoxE(False, 2, Sharding.create(M, 1, seed=0), args.relations, d, query_route=route, device=dev, dtype=dtype)


rng = np.random.default_rng(0)
hidx, tidx, ridx = (torch.from_numpy(rng.integers(hi, size=S).astype(np.int32)).to(dev)
                    for hi in (M, M, args.relations))
gen = torch.Generator().manual_seed(1)
dq, d_pos = torch.randn(S, 6 * d, generator=gen).to(dev), torch.randn(S, generator=gen).to(dev)

for dtype in (torch.float32, torch.float16):
    tag = "f32" if dtype == torch.float32 else "f16"
    fns = {route: make(route, dtype) for route in ROUTES}

    def sources(fn):
        table = fn.entity_embedding.data[0]
        return nat.RowSource(table, hidx), nat.RowSource(table, tidx)

    def forward(fn):
        head, tail = sources(fn)
        with torch.enable_grad():
            q, qctx = fn.query_fwd(nat.CORRUPT_HEAD, tail, ridx)
            pos, tctx = fn.triple_fwd(head, tail, ridx)
        return q, pos, qctx, tctx

    def backward(fn, state):
        head, tail = sources(fn)
        d_rel = torch.zeros(fn.relation_embedding.shape, dtype=torch.float32, device=dev)
        fn.query_bwd(nat.CORRUPT_HEAD, tail, ridx, state[2], dq, d_rel)
        fn.triple_bwd(head, tail, ridx, state[3], d_pos, d_rel)

    out = {route: forward(fn) for route, fn in fns.items()}
    print(json.dumps(dict(part="agreement", table=tag,
                          q=float((out["torch"][0] - out["native"][0]).abs().max()),
                          pos=float((out["torch"][1] - out["native"][1]).abs().max()))), flush=True)
    measure([(route, None, lambda _, fn=fn: forward(fn)) for route, fn in fns.items()], part="forward", table=tag)
    measure([(route, lambda fn=fn: forward(fn), lambda st, fn=fn: backward(fn, st)) for route, fn in fns.items()],
            part="backward", table=tag)

    batch = {k: torch.from_numpy(rng.integers(hi, size=s).astype(np.int32)).to(dev)
             for k, hi, s in (("head", M, (1, 1, S)), ("relation", args.relations, (1, 1, S)), ("tail", M, (1, 1, S)),
                              ("negative", M, (1, 1, S, args.negatives)))}
    runners = []
    for route in ROUTES:
        fn = make(route, dtype)
        ns = RandomShardedNegativeSampler(args.negatives, fn.sharding, 0, "h", local_sampling=False,
                                          flat_negative_format=False)
        model = EmbeddingMovingBessKGE(ns, fn, LogSigmoidLoss(1.0, True, 0.5))
        runner = runtime.training_model(model, runtime.Options(device_iterations=1), runtime.SGD(lr=1e-3), device=dev)
        runner(**batch)
        nat.start_kernel_timing(list(nat.SIGNATURES))
        runner(**batch)
        calls = [entry[0] for entry in nat.kernel_timing_log()]
        nat.stop_kernel_timing()
        print(json.dumps(dict(part="step calls", table=tag, route=route, native_calls=len(calls),
                              gather_rows=calls.count("bess_gather_rows"))), flush=True)
        results.append(dict(part="step calls", table=tag, route=route, native_calls=len(calls),
                            gather_rows=calls.count("bess_gather_rows")))
        runners.append((route, None, lambda _, runner=runner: runner(**batch)))
    measure(runners, part="EmbeddingMoving step", issue="eager (host time included)", table=tag, M=M,
            n_rel=args.relations, negatives=args.negatives)

with open(args.out, "w") as fh:
    json.dump(results, fh, indent=1)
