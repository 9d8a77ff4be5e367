#!/usr/bin/env python3
"""Cost of filtered negative sampling: the known-triple kernel alone, timed with HIP events, at
  * BASELINE config 2's shape - 4096 rows x 256 per-triple candidates, a 93,773-entity shard, an index of 1 M random
    triples over 51 relations (shard-local ids translated in the kernel, as the sampler calls it), and
  * a wikikg2-shaped point - 2.5 M entities, 535 relations, 16 M triples with skewed tails (hub entities), one flat
    candidate row of 1024 shared by 4096 rows, both sides;
against the bytes the call must move (4 B per candidate read, 1 B per mask byte written, the rows' operands and the
index lines touched), and the config-2 sampler call and training step with and without the filter.

    python profiles/bench_filter.py [--skip-wikikg2] [--skip-step] [--out FILE.json]
"""
import argparse
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "bess-kge_amd"), REPO]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import besskge  # noqa: E402,F401
from besskge import runtime  # noqa: E402
from besskge.batch_sampler import RandomShardedBatchSampler  # noqa: E402
from besskge.bess import EmbeddingMovingBessKGE  # noqa: E402
from besskge.dataset import KGDataset  # noqa: E402
from besskge.device_sampler import DeviceBatchSampler  # noqa: E402
from besskge.embedding import init_KGE_normal  # noqa: E402
from besskge.loss import LogSigmoidLoss  # noqa: E402
from besskge.negative_filter import SIDE_HEAD, SIDE_TAIL, KnownTripleFilter  # noqa: E402
from besskge.negative_sampler import RandomShardedNegativeSampler  # noqa: E402
from besskge.scoring import ComplEx  # noqa: E402
from besskge.sharding import PartitionedTripleSet, Sharding  # noqa: E402

LINE = 128  # bytes of an L2 line: what a touched index entry costs at least


def time_us(fn, warmup=10, reps=200):
    """Microseconds per call: `reps` calls between one pair of HIP events, after a warm-up."""
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / reps


def index_traffic(flt, side, kept_global, relation):
    """Bytes of index lines one call touches: per row the lines of its binary search over the keys (counted once
    per row - rows share the top levels in cache, so this is an upper bound on what leaves L2), one line of offsets,
    and the lines of its completion list where the pair exists."""
    keys, off, _ = flt.index_host[side]
    key = kept_global.astype(np.int64) * flt.n_relation_type + relation
    at = np.minimum(np.searchsorted(keys, key), keys.shape[0] - 1)
    found = keys[at] == key
    length = np.where(found, off[at + 1] - off[at], 0)
    steps = math.ceil(math.log2(max(2, keys.shape[0])))
    lines = key.shape[0] * steps + int(found.sum()) + int(np.ceil(length * 4 / LINE).sum())
    return lines * LINE, float(found.mean()), float(length.mean()), int(length.max())


def report(name, us, rows, cols, cand_bytes, index_bytes, extra):
    must = cand_bytes + rows * cols + rows * 9
    out = dict(case=name, rows=rows, cols=cols, us=round(us, 2), bytes_streamed=must, index_bytes_touched=index_bytes,
               GBps_streamed=round(must / us / 1e3, 1), GBps_with_index=round((must + index_bytes) / us / 1e3, 1),
               G_probes_per_s=round(rows * cols / us / 1e3, 2), **extra)
    print(json.dumps(out), flush=True)
    return out


def config2(dev, results, skip_step):
    n_ent, n_rel, n_known, S, K, D = 93_773, 51, 1_000_000, 4096, 256, 256
    rng = np.random.default_rng(0)
    triples = np.stack([rng.integers(n_ent, size=n_known), rng.integers(n_rel, size=n_known),
                        rng.integers(n_ent, size=n_known)], axis=1)
    sharding = Sharding.create(n_ent, 1, seed=1234)
    flt = KnownTripleFilter([triples], n_ent, n_rel, device=dev)
    l2g = torch.from_numpy(sharding.shard_and_idx_to_entity.astype(np.int32)).to(dev)
    kept = rng.integers(n_ent, size=S).astype(np.int32)  # local rows of shard 0
    rel = rng.integers(n_rel, size=S).astype(np.int32)
    cand = torch.from_numpy(rng.integers(n_ent, size=(S, K)).astype(np.int32)).to(dev)
    kept_d, rel_d = torch.from_numpy(kept).to(dev), torch.from_numpy(rel).to(dev)
    shard0 = torch.zeros(S, dtype=torch.int32, device=dev)
    mask = torch.empty((S, K), dtype=torch.bool, device=dev)
    kept_global = sharding.shard_and_idx_to_entity[0][kept]
    for side, name in ((SIDE_TAIL, "t"), (SIDE_HEAD, "h")):
        us = time_us(lambda: flt.mask(kept_d, rel_d, side, cand, out=mask, local_to_global=l2g, kept_shard=shard0,
                                      cols_per_shard=K))
        ib, found, mean_len, max_len = index_traffic(flt, side, kept_global, rel)
        known = 1.0 - float(mask.double().mean())
        # (the translation reads 4 B of the local-to-global table per candidate on top of the candidate itself)
        results.append(report(f"config2 {S}x{K} side {name}", us, S, K, 8 * S * K, ib,
                              dict(index_MB=round(flt.nbytes / 2 ** 20, 1), pairs_found=round(found, 3),
                                   mean_list=round(mean_len, 2), max_list=max_len, known_share=round(known, 8))))
    if skip_step:
        return
    # ---- the sampler call and the training step, with and without the filter
    n_train = 4_762_678
    train = np.stack([rng.integers(n_ent, size=n_train), rng.integers(n_rel, size=n_train),
                      rng.integers(n_ent, size=n_train)], axis=1)
    ds = KGDataset(n_entity=n_ent, n_relation_type=n_rel, triples={"train": train},
                   original_triple_ids={"train": np.arange(n_train)})
    pts = PartitionedTripleSet.create_from_dataset(ds, "train", sharding, partition_mode="ht_shardpair")

    def make(**kw):
        ns = RandomShardedNegativeSampler(K, sharding, 1234, "t", local_sampling=False, flat_negative_format=False)
        return DeviceBatchSampler(RandomShardedBatchSampler(pts, ns, S, 1, seed=1234), dev, **kw)

    plain, filtered = make(), make(filter_triples=flt)
    t_plain, t_filt = time_us(plain.sample, 5, 100), time_us(filtered.sample, 5, 100)
    torch.manual_seed(0)
    fn = ComplEx(False, sharding, n_rel, D, [init_KGE_normal], [init_KGE_normal])
    model = EmbeddingMovingBessKGE(negative_sampler=plain.host.negative_sampler, score_fn=fn,
                                   loss_fn=LogSigmoidLoss(margin=12.0, negative_adversarial_sampling=True))
    runner = runtime.training_model(model, runtime.Options(device_iterations=1), runtime.SGD(lr=1e-3), device=dev)
    b_plain = {k: v.flatten(end_dim=1) for k, v in plain.sample().items()}
    b_filt = {k: v.flatten(end_dim=1) for k, v in filtered.sample().items()}
    step = {}
    for _ in range(2):  # alternate the two versions; keep the second round
        step["plain"] = time_us(lambda: runner(**b_plain), 5, 100)
        step["masked"] = time_us(lambda: runner(**b_filt), 5, 100)
    both = {}
    for name, smp in (("plain", plain), ("masked", filtered)):
        both[name] = time_us(lambda: runner(**{k: v.flatten(end_dim=1) for k, v in smp.sample().items()}), 5, 100)
    out = dict(case="config2 sampler call and training step (ComplEx d=256 fp32, SGD)",
               sample_us=round(t_plain, 1), sample_filtered_us=round(t_filt, 1),
               step_us=round(step["plain"], 1), step_masked_us=round(step["masked"], 1),
               step_ratio=round(step["masked"] / step["plain"], 4),
               sample_and_step_us=round(both["plain"], 1), sample_and_step_filtered_us=round(both["masked"], 1),
               sample_and_step_ratio=round(both["masked"] / both["plain"], 4),
               known_share=round(1.0 - float(b_filt["negative_mask"].double().mean()), 8))
    print(json.dumps(out), flush=True)
    results.append(out)


def wikikg2(dev, results):
    n_ent, n_rel, n_known, S, C = 2_500_000, 535, 16_000_000, 4096, 1024
    rng = np.random.default_rng(1)
    tails = (n_ent * rng.random(n_known) ** 4).astype(np.int64)  # skewed: a few hub tails with thousands of heads
    triples = np.stack([rng.integers(n_ent, size=n_known), rng.integers(n_rel, size=n_known), tails], axis=1)
    flt = KnownTripleFilter([triples], n_ent, n_rel, device=dev)
    pick = rng.integers(n_known, size=S)  # queries are known triples: their pairs exist
    cand = torch.from_numpy(rng.integers(n_ent, size=(1, C)).astype(np.int32)).to(dev)
    mask = torch.empty((S, C), dtype=torch.bool, device=dev)
    for side, name, col in ((SIDE_TAIL, "t", 0), (SIDE_HEAD, "h", 2)):
        kept, rel = triples[pick, col].astype(np.int32), triples[pick, 1].astype(np.int32)
        kept_d, rel_d = torch.from_numpy(kept).to(dev), torch.from_numpy(rel).to(dev)
        us = time_us(lambda: flt.mask(kept_d, rel_d, side, cand, out=mask))
        ib, found, mean_len, max_len = index_traffic(flt, side, kept, rel)
        known = 1.0 - float(mask.double().mean())
        results.append(report(f"wikikg2-shaped {S}x{C} flat, side {name}", us, S, C, 4 * C, ib,
                              dict(index_MB=round(flt.nbytes / 2 ** 20, 1), distinct_triples=flt.n_triple,
                                   pairs_found=round(found, 3), mean_list=round(mean_len, 2), max_list=max_len,
                                   known_share=round(known, 8))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-wikikg2", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_filter.py measures on a HIP device; none found")
    dev = torch.device("cuda", 0)
    results = []
    config2(dev, results, args.skip_step)
    if not args.skip_wikikg2:
        wikikg2(dev, results)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
