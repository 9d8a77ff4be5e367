#!/usr/bin/env python3
"""ConvE's query network on its two routes, paper's shape (d = 200 as 20 x 20 stacked image, 32
channels, 3 x 3), train mode with batch-norm, dropouts 0, S = 4096; in the style of profiles/bench_relation_query.py:

  query    `_net` forward, and forward + backward for a fixed dq, "torch" (MIOpen / rocBLAS modules) against "fused"
           (csrc/conve.hip), the two alternating in one process; peak allocation of one call beside the times
  step     one `KvsAllBessKGE` training step (plain SGD, label smoothing 0.1, 93,773 entities, one shard, 474
           relations) on both routes; host time included: eager

Medians of `--repeats` event pairs after `--warmup`.  Prints one JSON line per measurement and writes them to `--out`.
FLOP of the query: 2 S F (d + Cin kh kw) forward, three times that forward + backward."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "bess-kge_amd"), REPO]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from besskge import runtime  # noqa: E402
from besskge.k_vs_all import KvsAllBessKGE  # noqa: E402
from besskge.loss import AllEntitiesBCELoss  # noqa: E402
from besskge.negative_sampler import PlaceholderNegativeSampler  # noqa: E402
from besskge.scoring import ConvE  # noqa: E402
from besskge.sharding import Sharding  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--queries", type=int, default=4096)
ap.add_argument("--entities", type=int, default=93_773)
ap.add_argument("--relations", type=int, default=474)
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_conve_query.json"))
args = ap.parse_args()

assert torch.cuda.is_available(), "this measurement needs a HIP device"
dev = torch.device("cuda", 0)
S, d, F, KK = args.queries, 200, 32 * 18 * 18, 9
results = []


def alternate(runs):
    times = {label: [] for label, _ in runs}
    for it in range(args.warmup + args.repeats):
        for label, run in runs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run()
            b.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                times[label].append(a.elapsed_time(b))
    return times


def peak_of(run):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    out = run()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated(dev) - base


def measure(runs, flop=None, **tags):
    times = alternate(runs)
    for label, run in runs:
        v = times[label]
        res = dict(tags, route=label, S=S, ms=round(statistics.median(v), 3), ms_min_max=[round(min(v), 3), round(max(v), 3)],
                   peak_bytes=peak_of(run), device=torch.cuda.get_device_name(0), repeats=args.repeats)
        if flop:
            res["tflops"] = round(flop / statistics.median(v) / 1e9, 2)
        print(json.dumps(res), flush=True)
        results.append(res)


def make(route, sharding):
    torch.manual_seed(0)
    return ConvE(True, sharding, args.relations, d, 10, 20, inverse_relations=False, input_dropout=0.0,
                 feature_map_dropout=0.0, hidden_dropout=0.0, query_route=route, device=dev).to(dev).train()


small = Sharding.create(1000, 1, seed=0)
nets = {route: make(route, small) for route in ("torch", "fused")}
gen = torch.Generator().manual_seed(1)
head, rel, dq = (torch.randn(s, generator=gen).to(dev) for s in ((S, d + 1), (S, d), (S, d)))
with torch.no_grad():
    q = {route: fn._net(head, rel) for route, fn in nets.items()}
print(json.dumps(dict(part="agreement", largest_deviation=float((q["torch"] - q["fused"]).abs().max()),
                      largest_value=float(q["torch"].abs().max()))), flush=True)


def forward(fn):
    with torch.no_grad():
        return fn._net(head, rel)


def forward_backward(fn):
    h, r = head.clone().requires_grad_(), rel.clone().requires_grad_()
    return torch.autograd.grad(fn._net(h, r), [h, r] + fn.dense_parameters(), dq, allow_unused=True)


flop = 2.0 * S * F * (d + KK)
measure([(route, lambda fn=fn: forward(fn)) for route, fn in nets.items()], flop=flop, part="query forward")
measure([(route, lambda fn=fn: forward_backward(fn)) for route, fn in nets.items()], flop=3 * flop, part="query forward + backward")

Mn = args.entities
rng = np.random.default_rng(0)
sharding = Sharding.create(Mn, 1, seed=0)
batch_np = {k: rng.integers(hi, size=S) for k, hi in (("head", Mn), ("relation", args.relations), ("tail", Mn))}
l2g = sharding.shard_and_idx_to_entity[0]
known = np.stack([l2g[batch_np["head"]], batch_np["relation"], l2g[batch_np["tail"]]], axis=1).astype(np.int64)
batch = {k: torch.from_numpy(v.astype(np.int32).reshape(1, 1, S)).to(dev) for k, v in batch_np.items()}
runners = []
for route in ("torch", "fused"):
    model = KvsAllBessKGE(PlaceholderNegativeSampler("t"), make(route, sharding),
                          AllEntitiesBCELoss(Mn, label_smoothing=0.1, loss_scale=1.0 / Mn), [known])
    runner = runtime.training_model(model, runtime.Options(device_iterations=1), runtime.SGD(lr=1e-3), device=dev)
    runner(**batch)
    runners.append((route, lambda runner=runner: runner(**batch)))
measure(runners, part="KvsAll step", issue="eager (host time included)", M=Mn, n_rel=args.relations, label_smoothing=0.1)

with open(args.out, "w") as fh:
    json.dump(results, fh, indent=1)
