"""Filtered top-10 of 5000 queries against all 123,182 entities of one shard (YAGO3-10): the lists kept while the
shard is scored (`AllScoresBESS.topk_replicas`: pruned score tiles + `bess_topk_update_excl`) against the matrix
path of `AllScoresPipeline(fused_topk=False)` - the device work of `pipeline.py: forward`: the window loop of
`AllScoresBESS`, the `[queries, n_entity]` fp32 matrix, -inf at the filtered completions, one `topk_merge`.
ComplEx d = 128 fp32, TransE d = 256 fp16, PairRE d = 256 fp16.  The filter leaves out 8 of every query's 20 best
entities (filtered completions are true triples: they score high); the hub run gives query 0 its 5000 best
entities as exclusions on top.  Timed with HIP events around 5 repetitions after 2 warm-up runs; peak allocation
(`torch.cuda.max_memory_allocated`) of one run of each path on top of what the model and the batch hold.

    python profiles/bench_topk_filtered.py            (needs the GPU)
"""

import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "bess-kge_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

from besskge.bess import AllScoresBESS  # noqa: E402
from besskge.collectives import SingleProcessGroup  # noqa: E402
from besskge.negative_sampler import PlaceholderNegativeSampler  # noqa: E402
from besskge.query import topk_merge  # noqa: E402
from besskge.scoring import ComplEx, PairRE, TransE  # noqa: E402
from besskge.sharding import Sharding  # noqa: E402

dev = torch.device("cuda", 0)
K = 10


def timed(f, reps=5, warmup=2):
    """(milliseconds per call by HIP events, peak bytes allocated by one call, last result)"""
    for _ in range(warmup):
        out = f()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = f()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        out = f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, peak, out


def run(label, make, n_entity, n_rel, ew, rw, n_query, dtype, window):
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    sharding = Sharding.create(n_entity, 1, seed=0)
    ent = torch.randn(1, sharding.max_entity_per_shard, ew) * 0.3
    rel = torch.randn(n_rel, rw) * 0.3
    fn = make(sharding, n_rel, ent, rel).to(dev)
    if dtype == torch.float16:
        fn = fn.half()
    mod = AllScoresBESS(PlaceholderNegativeSampler("t"), fn, window_size=window)
    mod.attach(SingleProcessGroup(1))
    batch = dict(head=torch.from_numpy(rng.integers(n_entity, size=(1, n_query)).astype(np.int32)).to(dev),
                 relation=torch.from_numpy(rng.integers(n_rel, size=(1, n_query)).astype(np.int32)).to(dev))
    kk = torch.full((1, 1), K, dtype=torch.int32)
    # column order of the assembled scores -> global entity id (pipeline.py: _first)
    M = sharding.max_entity_per_shard
    cols = np.concatenate([sharding.shard_and_idx_to_entity[:, np.minimum(i * window + np.arange(window), M - 1)].flatten()
                           for i in range(mod.n_step)])
    first = torch.from_numpy(np.unique(cols, return_index=True)[1]).to(dev)
    col_ent = torch.from_numpy(cols.astype(np.int64)).to(dev)

    def pairs_for(hub):
        top = mod.topk_replicas([dict(batch, topk_k=torch.full((1, 1), 20, dtype=torch.int32))])[0]["topk_global_id"]
        q = torch.arange(n_query, device=dev)[:, None].expand(n_query, 8)
        p = torch.stack([q.reshape(-1), top[:, ::2][:, :8].reshape(-1).long()], dim=1)
        if hub:
            sc = mod.forward_replicas([dict(batch, step=torch.zeros((1, 1), dtype=torch.int32))])[0]  # window 0
            best = col_ent[torch.topk(sc[0].float(), 5000).indices].long()  # the hub's 5000 best of that window
            p = torch.cat([p, torch.stack([torch.zeros_like(best), best], dim=1)])
        p = torch.unique(p, dim=0)
        return p

    for hub in (False, True):
        p = pairs_for(hub)
        filt = p.to(torch.int32)[None]  # [1, P, 2]: (query position, global entity id)
        b = dict(batch, topk_k=kk, rank_filter=filt)

        def lists():
            return mod.topk_replicas([b])[0]["topk_global_id"]

        def matrix():
            parts = [mod.forward_replicas([dict(batch, step=torch.full((1, 1), i, dtype=torch.int32))])[0]
                     for i in range(mod.n_step)]
            sc = torch.concat(parts, dim=-1)[:, first][:, :n_entity].float()
            sc[p[:, 0], p[:, 1]] = -torch.inf
            top_s = torch.full((n_query, K), -torch.inf, dtype=torch.float32, device=dev)
            top_i = torch.zeros((n_query, K), dtype=torch.int32, device=dev)
            topk_merge(sc.contiguous(), top_s, top_i)
            return top_i

        tm, pm, rm = timed(matrix)
        tl, pl, rl = timed(lists)
        agree = float((rl == rm).float().mean())
        g = n_query * n_entity / 1e6
        what = "hub row of %d exclusions" % int((p[:, 0] == 0).sum()) if hub else "%d filtered pairs" % len(p)
        print(f"{label:28s} {what:28s} lists {tl:8.2f} ms ({g / tl:6.1f} G scores/s) peak {pl / 2**20:8.1f} MiB | "
              f"score matrix {tm:8.2f} ms ({g / tm:6.1f} G scores/s) peak {pm / 2**20:8.1f} MiB | "
              f"ids equal {agree:.4f}", flush=True)


if __name__ == "__main__":
    print(torch.cuda.get_device_name(0), flush=True)
    N, R, Q = 123_182, 37, 5000
    cx = lambda sh, n_rel, ent, rel: ComplEx(True, sh, n_rel, 128, ent, rel)  # noqa: E731
    te = lambda sh, n_rel, ent, rel: TransE(True, 1, sh, n_rel, 256, ent, rel)  # noqa: E731
    pair = lambda sh, n_rel, ent, rel: PairRE(True, 1, sh, n_rel, 256, ent, rel, normalize_entities=True)  # noqa: E731
    # (one window per shard: the matrix path at its fastest, and the kernel the all-entity pass takes)
    run("ComplEx d=128 fp32", cx, N, R, 256, 256, Q, torch.float32, N)
    run("TransE d=256 fp16", te, N, R, 256, 256, Q, torch.float16, N)
    run("PairRE d=256 fp16", pair, N, R, 256, 512, Q, torch.float16, N)
