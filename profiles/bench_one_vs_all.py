#!/usr/bin/env python3
"""1vsAll training at BASELINE config 2's shape: ComplEx d = 256 fp32 (W = 512), 93,773
entities, S = 4096 queries, one shard.

  kernels  `bess_neg_score_shared_fwd_lse`, `bess_neg_score_shared_bwd_softmax` and - the yardstick of the forward:
           the same split-fp16 product with the counting epilogue - `bess_neg_score_shared_fwd_counts`, launched
           alternately in one process; flops = 2 S M W per product (one in the forward; the recomputed scores and the
           two gradient products in the backward: three)
  step     one `OneVsAllBessKGE` training step (plain SGD), host time included: the step is eager
  memory   peak allocated bytes over a step, beside the 2 x S x M x 4 bytes of a score matrix and its gradient

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
from besskge.loss import SampledSoftmaxCrossEntropyLoss  # noqa: E402
from besskge.negative_sampler import PlaceholderNegativeSampler  # noqa: E402
from besskge.one_vs_all import OneVsAllBessKGE  # noqa: E402
from besskge.scoring import ComplEx  # noqa: E402
from besskge.sharding import Sharding  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--entities", type=int, default=93_773)
ap.add_argument("--queries", type=int, default=4096)
ap.add_argument("--d", type=int, default=256)
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_one_vs_all.json"))
args = ap.parse_args()

assert torch.cuda.is_available(), "this measurement needs a HIP device"
dev = torch.device("cuda", 0)
M, S, d = args.entities, args.queries, args.d
W = 2 * d
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


def emit(res):
    res.update(device=torch.cuda.get_device_name(0), repeats=args.repeats)
    print(json.dumps(res), flush=True)
    results.append(res)


torch.manual_seed(0)
sharding = Sharding.create(M, 1, seed=0)
fn = ComplEx(True, sharding, 51, d, device=dev)
desc = fn.kernel_desc()
table = fn.entity_embedding.data[0]
gen = torch.Generator().manual_seed(1)
known = torch.randint(M, (S,), generator=gen, dtype=torch.int32).to(dev)
rid = torch.randint(51, (S,), generator=gen, dtype=torch.int32).to(dev)
query = fn.query_fwd(nat.CORRUPT_TAIL, nat.RowSource(table, known), rid)[0]
cand = nat.RowSource(table)
state = nat.neg_score_shared_lse(desc, query, cand)
lse = (state[:, 0] + torch.log(state[:, 1])).contiguous()
coef = torch.ones(S, device=dev)
thr = torch.zeros(S, device=dev)
excl = torch.full((S,), -1, dtype=torch.int32, device=dev)

times = alternate([
    ("fwd_lse", lambda: nat.neg_score_shared_lse(desc, query, cand)),
    ("fwd_counts", lambda: nat.neg_score_shared_counts(desc, query, cand, thr, excl)),
    ("bwd_softmax", lambda: nat.neg_score_shared_bwd_softmax(desc, query, cand, lse, coef)),
])
flop = 2.0 * S * M * W
for label, v in times.items():
    ms = statistics.median(v)
    emit(dict(part="kernels", call=label, S=S, M=M, W=W, ms=round(ms, 3), ms_min_max=[round(min(v), 3), round(max(v), 3)],
              tflops=round((3 if label == "bwd_softmax" else 1) * flop / ms / 1e9, 1)))

model = OneVsAllBessKGE(PlaceholderNegativeSampler("t"), fn, SampledSoftmaxCrossEntropyLoss(M))
runner = runtime.training_model(model, runtime.Options(device_iterations=1), runtime.SGD(lr=1e-3), device=dev)
rng = np.random.default_rng(0)
batch = {k: torch.from_numpy(rng.integers(hi, size=(1, 1, S)).astype(np.int32)).to(dev)
         for k, hi in (("head", M), ("relation", 51), ("tail", M))}
runner(**batch)
torch.cuda.synchronize()
torch.cuda.reset_peak_memory_stats(dev)
base = torch.cuda.memory_allocated(dev)
v = alternate([("step", lambda: runner(**batch))])["step"]
peak = torch.cuda.max_memory_allocated(dev)
emit(dict(part="step", issue="eager (host time included)", S=S, M=M, W=W, ms=round(statistics.median(v), 3),
          ms_min_max=[round(min(v), 3), round(max(v), 3)], resident_bytes=base, peak_bytes_over_resident=peak - base,
          score_matrix_and_gradient_bytes=2 * S * M * 4))

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(results, f, indent=1)
    f.write("\n")
