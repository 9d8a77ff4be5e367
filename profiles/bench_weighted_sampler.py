#!/usr/bin/env python3
"""Degree-weighted negative sampling: `bess_sample_negatives_weighted` against the uniform `bess_sample_negatives`,
in one process and at the same shapes.

  c2_pertriple   1 shard of 93,773 rows, B = 4096 triples x K = 256 negatives (BASELINE configs[1])
  c4_flat_k32    8 shards of 312,576 rows as one rank sees them (source shard 0 only), B = 1, K = 32
  c4_flat_k2048  the same, K = 2048
  synthetic      1 shard of 62.5 M rows (500 MB of running sums), B = 8192, K = 64

Weights: floor(zipf(1.6) ** 0.75 * 1024) from `default_rng(0)`.  Both kernels draw from the same generator state; the
two are launched alternately, `--inner` launches between a pair of HIP events, medians of `--repeats` pairs after
`--warmup`.  The first 4096 rows of every weighted draw are checked against numpy.  Prints one JSON line per shape and
writes them to `--out`."""
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
from besskge.device_sampler import Pcg64Stream  # noqa: E402

SHAPES = {  # name: (n_shard, rows per shard, B, K)
    "c2_pertriple": (1, 93_773, 4096, 256),
    "c4_flat_k32": (8, 312_576, 1, 32),
    "c4_flat_k2048": (8, 312_576, 1, 2048),
    "synthetic": (1, 62_500_000, 8192, 64),
}

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", nargs="*", default=list(SHAPES), choices=list(SHAPES))
ap.add_argument("--repeats", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--inner", type=int, default=10)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_weighted_sampler.json"))
args = ap.parse_args()

assert torch.cuda.is_available(), "this measurement needs a HIP device"
dev = torch.device("cuda", 0)
results = []
for name in args.shapes:
    n_shard, rows, B, K = SHAPES[name]
    rng = np.random.default_rng(0)
    weights = np.floor(rng.zipf(1.6, size=rows).astype(np.float64) ** 0.75 * 1024).astype(np.int64)
    cum_host = np.cumsum(weights)[None, :]  # the rank's own shard: one row of running sums
    assert 0 < int(cum_host[0, -1]) < 1 << 62
    cum = torch.from_numpy(cum_host).to(dev)
    counts = torch.full((n_shard,), rows, dtype=torch.int32, device=dev)
    stream = Pcg64Stream.from_generator(np.random.default_rng(1))
    table = torch.from_numpy(stream.jump_table().view(np.int64)).to(dev)
    gen = stream.native()

    def uniform():
        return nat.sample_negatives(gen, table, 1, n_shard, 0, 1, B, K, counts)

    def weighted():
        return nat.sample_negatives_weighted(gen, table, 1, n_shard, 0, 1, B, K, cum, counts)

    got = weighted().reshape(-1)[:4096].cpu().numpy()
    raw = np.random.default_rng(1).integers(1 << 63, size=got.shape[0])
    assert np.array_equal(got, np.searchsorted(cum_host[0], raw % cum_host[0, -1], side="right")), name
    times = {"uniform": [], "weighted": []}
    for it in range(args.warmup + args.repeats):
        for label, run in (("uniform", uniform), ("weighted", weighted)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.inner):
                run()
            b.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                times[label].append(a.elapsed_time(b) * 1e3 / args.inner)  # us per launch
    us = {k: statistics.median(v) for k, v in times.items()}
    n_out = n_shard * B * K
    res = dict(shape=name, n_shard=n_shard, rows_per_shard=rows, B=B, K=K, draws=n_out,
               search_levels=int(rows).bit_length(), running_sums_mib=round(cum.numel() * 8 / 2 ** 20, 1),
               uniform_us=round(us["uniform"], 2), weighted_us=round(us["weighted"], 2),
               ratio=round(us["weighted"] / us["uniform"], 2),
               uniform_us_min_max=[round(min(times["uniform"]), 2), round(max(times["uniform"]), 2)],
               weighted_us_min_max=[round(min(times["weighted"]), 2), round(max(times["weighted"]), 2)],
               weighted_draws_per_s=round(n_out / us["weighted"] * 1e6), inner=args.inner, repeats=args.repeats,
               device=torch.cuda.get_device_name(0))
    print(json.dumps(res), flush=True)
    results.append(res)
    del cum
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(results, f, indent=1)
    f.write("\n")
