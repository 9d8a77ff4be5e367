#!/usr/bin/env python3
"""Filtered evaluation: what it costs to make one sampler batch's filter (`rank_filter` + counts per kept triple).

  host    the path of `AllScoresPipeline(filter_triples=[...])`: `utils.get_entity_filter` (queries x filter
          triples) + `rank_filter_pairs` on the host, and the copy of the result to the device;
  device  the path of `device_filter=True`: a count pass and a fill pass of `bess_known_completions` over the
          `KnownTripleFilter` index in HBM, the uploads of the batch's index tensors and the one host read included.

Both through `AllScoresPipeline._filter_pairs`, on the same batch; the two results must be equal.  YAGO3-10 shape,
synthetic (`default_rng(0)`): 5000 queries, 123,182 entities, 37 relations, 1,079,040 filter triples,
h_shard, one shard.  Medians of repeated runs after warm-up; host path: wall clock ending in a device synchronise,
device path: the same and HIP events round the call.  The peak resident memory is read after the host runs (the
device runs come first: they do not raise it).  Prints one JSON line."""
import argparse
import json
import os
import resource
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "bess-kge_amd"), REPO]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from besskge.batch_sampler import RigidShardedBatchSampler  # noqa: E402
from besskge.dataset import KGDataset  # noqa: E402
from besskge.metric import Evaluation  # noqa: E402
from besskge.negative_sampler import PlaceholderNegativeSampler  # noqa: E402
from besskge.pipeline import AllScoresPipeline  # noqa: E402
from besskge.scoring import TransE  # noqa: E402
from besskge.sharding import PartitionedTripleSet, Sharding  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--queries", type=int, default=5000)
ap.add_argument("--entities", type=int, default=123_182)
ap.add_argument("--relations", type=int, default=37)
ap.add_argument("--filter-triples", type=int, default=1_079_040)
ap.add_argument("--host-repeats", type=int, default=3)
ap.add_argument("--device-repeats", type=int, default=50)
args = ap.parse_args()

assert torch.cuda.is_available(), "this measurement needs a HIP device"
dev = torch.device("cuda", 0)
rng = np.random.default_rng(0)
nt = args.filter_triples
known = np.stack([rng.integers(args.entities, size=nt), rng.integers(args.relations, size=nt),
                  rng.integers(args.entities, size=nt)], axis=1)
queries = known[rng.choice(nt, size=args.queries, replace=False)]  # (a filtered evaluation's filter holds its queries)
sharding = Sharding.create(args.entities, 1, seed=1234)
ds = KGDataset(n_entity=args.entities, n_relation_type=args.relations, triples={"test": queries},
               original_triple_ids={"test": np.arange(args.queries)})
pts = PartitionedTripleSet.create_from_dataset(ds, "test", sharding, partition_mode="h_shard")
torch.manual_seed(0)
fn = TransE(True, 1, sharding, args.relations, 16).to(dev).half().eval()  # (never scored here: the filter alone is timed)


def pipeline(**kw):
    bs = RigidShardedBatchSampler(pts, PlaceholderNegativeSampler("t"), shard_bs=args.queries, batches_per_step=1,
                                  seed=1234, return_triple_idx=True)
    return AllScoresPipeline(bs, "t", fn, evaluation=Evaluation(["mrr"]), filter_triples=[known], device=dev, **kw)


def wall(run, repeats, warmup):
    out = []
    for it in range(warmup + repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = run()
        torch.cuda.synchronize()
        if it >= warmup:
            out.append(time.perf_counter() - t0)
    return res, out


host = pipeline()
t0 = time.perf_counter()
device = pipeline(device_filter=True)
torch.cuda.synchronize()
build_s = time.perf_counter() - t0  # (index build + upload, once per pipeline; the rest of the constructor is small)
batch = dict(next(iter(host.dl)))
mask, truth, triple_id = batch.pop("triple_mask"), batch.pop("tail"), batch.pop("triple_idx")

got, device_wall = wall(lambda: device._filter_pairs(truth, mask, None, batch), args.device_repeats, 5)
events = []
for _ in range(args.device_repeats):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    device._filter_pairs(truth, mask, None, batch)
    b.record()
    torch.cuda.synchronize()
    events.append(a.elapsed_time(b) * 1e-3)
rss_before_host = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss


def host_path():
    filt, per_kept = host._filter_pairs(truth, mask, triple_id)
    return filt.to(dev), per_kept.to(dev)


want, host_wall = wall(host_path, args.host_repeats, 1)
rss_after_host = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "the two paths disagree"
ms = lambda xs: round(statistics.median(xs) * 1e3, 3)  # noqa: E731
print(json.dumps(dict(
    shape=dict(queries=args.queries, entities=args.entities, relations=args.relations, filter_triples=nt),
    rank_filter_shape=list(want[0].shape), filtered_pairs=int(want[1].sum()),
    host_ms=ms(host_wall), host_ms_all=[round(x * 1e3, 1) for x in host_wall],
    host_peak_rss_gib=round(rss_after_host / 2 ** 20, 2), rss_before_host_gib=round(rss_before_host / 2 ** 20, 2),
    device_wall_ms=ms(device_wall), device_events_ms=ms(events),
    device_wall_ms_min_max=[round(min(device_wall) * 1e3, 3), round(max(device_wall) * 1e3, 3)],
    index_build_s=round(build_s, 3), index_mib=round(device.known_filter.nbytes / 2 ** 20, 1),
    device=torch.cuda.get_device_name(0))), flush=True)
