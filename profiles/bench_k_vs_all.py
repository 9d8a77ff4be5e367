#!/usr/bin/env python3
"""KvsAll training at BASELINE config 2's shape: ComplEx d = 256 fp32 (W = 512), 93,773
entities, S = 4096 queries, one shard.

  kernels  `bess_neg_score_shared_fwd_bce`, `bess_label_score_sums`, `bess_neg_score_shared_bwd_bce` and their
           yardsticks as they stand - `bess_neg_score_shared_fwd_counts`, `bess_neg_score_shared_fwd_lse`,
           `bess_neg_score_shared_bwd_softmax` - launched alternately in one process
  labels   a synthetic filter: every query has Poisson(3) known completions beside its own, 32 queries have 256 and
           one hub query has `--hub` (2048); the distribution is written into the JSON
  step     one `KvsAllBessKGE` training step (plain SGD), host time included: the step is eager
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
from besskge.k_vs_all import KvsAllBessKGE  # noqa: E402
from besskge.loss import AllEntitiesBCELoss  # noqa: E402
from besskge.negative_sampler import PlaceholderNegativeSampler  # noqa: E402
from besskge.scoring import ComplEx  # noqa: E402
from besskge.sharding import Sharding  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--entities", type=int, default=93_773)
ap.add_argument("--queries", type=int, default=4096)
ap.add_argument("--d", type=int, default=256)
ap.add_argument("--hub", type=int, default=2048)
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_k_vs_all.json"))
args = ap.parse_args()

assert torch.cuda.is_available(), "this measurement needs a HIP device"
dev = torch.device("cuda", 0)
M, S, d = args.entities, args.queries, args.d
W = 2 * d
EPS = 0.1
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
rng = np.random.default_rng(0)
sharding = Sharding.create(M, 1, seed=0)
fn = ComplEx(True, sharding, 51, d, device=dev)
desc = fn.kernel_desc()
table = fn.entity_embedding.data[0]
batch_np = {k: rng.integers(hi, size=S) for k, hi in (("head", M), ("relation", 51), ("tail", M))}
# the filter: the batch's triples and the extra completions of their queries (local row == global id on one shard
# only up to the sharding's permutation: the batch holds local rows, the filter global ids)
l2g = sharding.shard_and_idx_to_entity[0]
lengths = rng.poisson(3.0, size=S)
lengths[rng.choice(S, 32, replace=False)] = 256
lengths[0] = args.hub
heads = np.repeat(l2g[batch_np["head"]], lengths)
rels = np.repeat(batch_np["relation"], lengths)
known = np.concatenate([np.stack([l2g[batch_np["head"]], batch_np["relation"], l2g[batch_np["tail"]]], axis=1),
                        np.stack([heads, rels, rng.integers(M, size=heads.shape[0])], axis=1)]).astype(np.int64)
loss_fn = AllEntitiesBCELoss(M, label_smoothing=EPS, loss_scale=1.0 / M)
model = KvsAllBessKGE(PlaceholderNegativeSampler("t"), fn, loss_fn, [known])
runner = runtime.training_model(model, runtime.Options(device_iterations=1), runtime.SGD(lr=1e-3), device=dev)
batch = {k: torch.from_numpy(v.astype(np.int32).reshape(1, 1, S)).to(dev) for k, v in batch_np.items()}

# the kernels on the step's own queries and labels
head, rid = batch["head"].reshape(-1), batch["relation"].reshape(-1)
query = fn.query_fwd(nat.CORRUPT_TAIL, nat.RowSource(table, head), rid)[0]
cand = nat.RowSource(table)
step = type("Step", (), dict(table=table, sm_head=batch["head"].reshape(1, S), local_tail=batch["tail"].reshape(1, S),
                             ppp=S))()
ptr, col = model._query_labels([step], [batch["relation"].reshape(1, 1, S)])[0]
row_len = (ptr[1:] - ptr[:-1]).cpu().numpy()
state = nat.neg_score_shared_lse(desc, query, cand)
lse = (state[:, 0] + torch.log(state[:, 1])).contiguous()
coef = torch.ones(S, device=dev)
thr = torch.zeros(S, device=dev)
excl = torch.full((S,), -1, dtype=torch.int32, device=dev)
smooth, pw = loss_fn.smooth, loss_fn.positive_weight

times = alternate([
    ("fwd_counts", lambda: nat.neg_score_shared_counts(desc, query, cand, thr, excl)),
    ("fwd_lse", lambda: nat.neg_score_shared_lse(desc, query, cand)),
    ("fwd_bce", lambda: nat.neg_score_shared_bce(desc, query, cand)),
    ("label_score_sums", lambda: nat.label_score_sums(desc, query, cand, ptr, col, validate=False)),
    ("bwd_softmax", lambda: nat.neg_score_shared_bwd_softmax(desc, query, cand, lse, coef)),
    ("bwd_bce", lambda: nat.neg_score_shared_bwd_bce(desc, query, cand, smooth, pw, ptr, col, coef, validate=False)),
])
labels = dict(total=int(row_len.sum()), mean=round(float(row_len.mean()), 2), median=float(np.median(row_len)),
              p99=float(np.percentile(row_len, 99)), longest=int(row_len.max()), rows_of_256_or_more=int((row_len >= 256).sum()))
for label, v in times.items():
    emit(dict(part="kernels", call=label, S=S, M=M, W=W, ms=round(statistics.median(v), 3),
              ms_min_max=[round(min(v), 3), round(max(v), 3)], label_lists=labels))
# what the longest list costs: the same call without the hub row's labels
short_ptr = ptr.clone()
short_ptr[1:] -= int(row_len[0])
short_col = col[int(row_len[0]):].contiguous()
v = alternate([("no_hub", lambda: nat.label_score_sums(desc, query, cand, short_ptr, short_col, validate=False))])["no_hub"]
emit(dict(part="kernels", call="label_score_sums without the longest list", ms=round(statistics.median(v), 3),
          ms_min_max=[round(min(v), 3), round(max(v), 3)], longest_left=int(np.sort(row_len)[-2])))

runner(**batch)
torch.cuda.synchronize()
torch.cuda.reset_peak_memory_stats(dev)
base = torch.cuda.memory_allocated(dev)
v = alternate([("step", lambda: runner(**batch))])["step"]
peak = torch.cuda.max_memory_allocated(dev)
emit(dict(part="step", issue="eager (host time included)", S=S, M=M, W=W, label_smoothing=EPS,
          ms=round(statistics.median(v), 3), ms_min_max=[round(min(v), 3), round(max(v), 3)], resident_bytes=base,
          peak_bytes_over_resident=peak - base, score_matrix_and_gradient_bytes=2 * S * M * 4))

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(results, f, indent=1)
    f.write("\n")
