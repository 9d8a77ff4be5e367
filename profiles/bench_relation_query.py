#!/usr/bin/env python3
"""The relation-grouped query product at the paper's entity width: S = 4096 rows, de = 200, with
(a) 474 relations drawn uniformly, (b) 22 relations, (c) every row in one relation.

  kernels  `relation_query_fwd / _bwd` alone (RESCAL's query; segment index prebuilt and, separately, the index build),
           and the whole TuckER query at dr = 200 and 30 on three routes, forward and forward + backward through
           autograd down to the relation table and the core: "relation" (`rel_table @ core` + `ops.RelationQuery`),
           "outer" (`ops.TuckerQuery` on gathered relation rows) and torch (`rel @ core` per triple + `bmm`, the route
           of profiles/bench_tucker.py); launched alternately in one process; milliseconds and peak allocation
  step     one `KvsAllBessKGE` training step (plain SGD, label smoothing 0.1, 93,773 entities, one shard, 474
           relations) of TuckER de = dr = 200 on both routes and of RESCAL de = 200; host time included: eager

Medians of `--repeats` event pairs after `--warmup`.  Prints one JSON line per measurement and writes them to `--out`."""
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
from besskge import ops, runtime  # noqa: E402
from besskge.k_vs_all import KvsAllBessKGE  # noqa: E402
from besskge.loss import AllEntitiesBCELoss  # noqa: E402
from besskge.negative_sampler import PlaceholderNegativeSampler  # noqa: E402
from besskge.scoring import RESCAL, TuckER  # noqa: E402
from besskge.sharding import Sharding  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--queries", type=int, default=4096)
ap.add_argument("--de", type=int, default=200)
ap.add_argument("--dr", type=int, nargs="+", default=[200, 30])
ap.add_argument("--entities", type=int, default=93_773)
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_relation_query.json"))
args = ap.parse_args()

assert torch.cuda.is_available(), "this measurement needs a HIP device"
dev = torch.device("cuda", 0)
S, de = args.queries, args.de
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


def measure(runs, **tags):
    times = alternate(runs)
    for label, run in runs:
        v = times[label]
        res = dict(tags, call=label, S=S, de=de, ms=round(statistics.median(v), 3),
                   ms_min_max=[round(min(v), 3), round(max(v), 3)], peak_bytes=peak_of(run),
                   device=torch.cuda.get_device_name(0), repeats=args.repeats)
        print(json.dumps(res), flush=True)
        results.append(res)


torch.manual_seed(0)
SETTINGS = [("a: 474 uniform", 474, lambda: torch.randint(474, (S,))), ("b: 22 uniform", 22, lambda: torch.randint(22, (S,))),
            ("c: one relation", 1, lambda: torch.zeros(S, dtype=torch.long))]
for setting, n_rel, draw in SETTINGS:
    rid = draw().to(dev)
    rid32 = rid.to(torch.int32)
    x, dq, M = (torch.randn(s, device=dev) for s in ((S, de), (S, de), (n_rel, de * de)))
    seg = nat.SegmentIndex(rid32, n_rel)
    measure([("index", lambda: nat.SegmentIndex(rid32, n_rel)),
             ("fwd", lambda: nat.relation_query_fwd(x, M, seg, False)),
             ("bwd", lambda: nat.relation_query_bwd(x, M, seg, False, dq)),
             ("bwd_d_x", lambda: nat.relation_query_bwd(x, M, seg, False, dq, want=(True, False))),
             ("bwd_d_M", lambda: nat.relation_query_bwd(x, M, seg, False, dq, want=(False, True)))],
            part="kernels", setting=setting, n_rel=n_rel)
    del M
    for dr in args.dr:
        gx, gR, gcore = (torch.randn(s, device=dev).requires_grad_() for s in ((S, de), (n_rel, dr), (dr * de, de)))
        routes = {
            "relation": lambda: ops.RelationQuery.apply(gx, gR @ gcore.view(dr, de * de), rid, False),
            "outer": lambda: ops.TuckerQuery.apply(gx, gR[rid], gcore, False),
            "torch": lambda: torch.bmm(gx.unsqueeze(1), (gR[rid] @ gcore.view(dr, -1)).view(S, de, de)).squeeze(1),
        }
        runs = []
        for name, fwd in routes.items():
            runs += [(f"{name}_fwd", fwd),
                     (f"{name}_fwd_bwd", lambda fwd=fwd: torch.autograd.grad(fwd(), [gx, gR, gcore], dq))]
        want = routes["torch"]().detach()
        dev_rel = {k: float((routes[k]().detach() - want).abs().max() / want.abs().max()) for k in ("relation", "outer")}
        measure(runs, part="tucker_query", setting=setting, n_rel=n_rel, dr=dr, fwd_deviation_from_torch=dev_rel)
        del gx, gR, gcore, want

# whole KvsAll steps
Mn, n_rel = args.entities, 474
rng = np.random.default_rng(0)
sharding = Sharding.create(Mn, 1, seed=0)
batch_np = {k: rng.integers(hi, size=S) for k, hi in (("head", Mn), ("relation", n_rel), ("tail", Mn))}
l2g = sharding.shard_and_idx_to_entity[0]
known = np.stack([l2g[batch_np["head"]], batch_np["relation"], l2g[batch_np["tail"]]], axis=1).astype(np.int64)
batch = {k: torch.from_numpy(v.astype(np.int32).reshape(1, 1, S)).to(dev) for k, v in batch_np.items()}
MODELS = [("TuckER outer", lambda: TuckER(True, sharding, n_rel, de, args.dr[0], device=dev)),
          ("TuckER relation", lambda: TuckER(True, sharding, n_rel, de, args.dr[0], query_route="relation", device=dev)),
          ("RESCAL", lambda: RESCAL(True, sharding, n_rel, de, device=dev))]
for name, make in MODELS:
    model = KvsAllBessKGE(PlaceholderNegativeSampler("t"), make(), AllEntitiesBCELoss(Mn, label_smoothing=0.1, loss_scale=1.0 / Mn),
                          [known])
    runner = runtime.training_model(model, runtime.Options(device_iterations=1), runtime.SGD(lr=1e-3), device=dev)
    runner(**batch)
    measure([("step", lambda: runner(**batch))], part="step", model=name, issue="eager (host time included)", M=Mn,
            n_rel=n_rel, dr=args.dr[0], label_smoothing=0.1)
    del model, runner

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(results, f, indent=1)
    f.write("\n")
