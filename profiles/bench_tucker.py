#!/usr/bin/env python3
"""TuckER's query product at the paper's entity width: S = 4096 rows, de = 200, dr = 30 and 200.

  kernels  `bess_tucker_query_fwd` and `bess_tucker_query_bwd` (all three gradients) beside the route every public
           implementation takes - `(rel @ core.view(dr, -1)).view(S, de, de)` then `bmm`, and its autograd -
           launched alternately in one process; milliseconds, fp32 TFLOP/s (2 S dr de^2 per product: one forward,
           three backward) and the peak allocation of one call of each
  step     one `KvsAllBessKGE` training step of the scorer (plain SGD, label smoothing 0.1, 93,773 entities, one
           shard, the batch's own triples as labels), host time included: the step is eager

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
from besskge import runtime  # noqa: E402
from besskge.k_vs_all import KvsAllBessKGE  # noqa: E402
from besskge.loss import AllEntitiesBCELoss  # noqa: E402
from besskge.negative_sampler import PlaceholderNegativeSampler  # noqa: E402
from besskge.scoring import TuckER  # noqa: E402
from besskge.sharding import Sharding  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--queries", type=int, default=4096)
ap.add_argument("--de", type=int, default=200)
ap.add_argument("--dr", type=int, nargs="+", default=[30, 200])
ap.add_argument("--entities", type=int, default=93_773)
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_tucker.json"))
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


def emit(res):
    res.update(device=torch.cuda.get_device_name(0), repeats=args.repeats)
    print(json.dumps(res), flush=True)
    results.append(res)


torch.manual_seed(0)
for dr in args.dr:
    x, rel, core, dq = (torch.randn(s, device=dev) for s in ((S, de), (S, dr), (dr * de, de), (S, de)))
    tx, trel, tcore = (t.clone().requires_grad_() for t in (x, rel, core))

    def torch_fwd():
        return torch.bmm(tx.unsqueeze(1), (trel @ tcore.view(dr, -1)).view(S, de, de)).squeeze(1)

    def torch_bwd():  # (autograd needs the graph of its forward: the two are timed together)
        return torch.autograd.grad(torch_fwd(), [tx, trel, tcore], dq)

    runs = [("fwd", lambda: nat.tucker_query_fwd(x, rel, core, False)),
            ("bwd", lambda: nat.tucker_query_bwd(x, rel, core, False, dq)),
            ("torch_fwd", torch_fwd), ("torch_fwd_bwd", torch_bwd)]
    got, want = runs[0][1](), torch_fwd().detach()
    deviation = float((got - want).abs().max() / want.abs().max())
    times = alternate(runs)
    flop = 2.0 * S * dr * de * de
    for (label, run), products in zip(runs, (1, 3, 1, 4)):
        v = times[label]
        ms = statistics.median(v)
        emit(dict(part="kernels", call=label, S=S, de=de, dr=dr, ms=round(ms, 3), ms_min_max=[round(min(v), 3), round(max(v), 3)],
                  fp32_tflops=round(products * flop / ms / 1e9, 1), peak_bytes=peak_of(run),
                  fwd_deviation_from_torch_relative_to_largest=deviation))
    del tx, trel, tcore

# the whole KvsAll step of the scorer
M, dr = args.entities, args.dr[0]
rng = np.random.default_rng(0)
sharding = Sharding.create(M, 1, seed=0)
fn = TuckER(True, sharding, 51, de, dr, device=dev)
batch_np = {k: rng.integers(hi, size=S) for k, hi in (("head", M), ("relation", 51), ("tail", M))}
l2g = sharding.shard_and_idx_to_entity[0]
known = np.stack([l2g[batch_np["head"]], batch_np["relation"], l2g[batch_np["tail"]]], axis=1).astype(np.int64)
model = KvsAllBessKGE(PlaceholderNegativeSampler("t"), fn, AllEntitiesBCELoss(M, label_smoothing=0.1, loss_scale=1.0 / M),
                      [known])
runner = runtime.training_model(model, runtime.Options(device_iterations=1), runtime.SGD(lr=1e-3), device=dev)
batch = {k: torch.from_numpy(v.astype(np.int32).reshape(1, 1, S)).to(dev) for k, v in batch_np.items()}
runner(**batch)
torch.cuda.synchronize()
torch.cuda.reset_peak_memory_stats(dev)
base = torch.cuda.memory_allocated(dev)
v = alternate([("step", lambda: runner(**batch))])["step"]
emit(dict(part="step", issue="eager (host time included)", S=S, M=M, de=de, dr=dr, label_smoothing=0.1,
          ms=round(statistics.median(v), 3), ms_min_max=[round(min(v), 3), round(max(v), 3)], resident_bytes=base,
          peak_bytes_over_resident=torch.cuda.max_memory_allocated(dev) - base))

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(results, f, indent=1)
    f.write("\n")
