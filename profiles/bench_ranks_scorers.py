"""Full ranks of PairRE (normalised; fp16 and fp32 table) and BoxE queries against all entities of one shard:
counted in the scoring kernel (`AllScoresBESS.rank_counts_replicas`) against the score-matrix path the library
had before (all entities scored into a matrix in 1 GiB tiles + `nat.ranks_from_scores`, as
`profiles/bench_topk.py: run_ranks` does for the four native scorers).  Shapes of that script's ranks row: 5000
queries x 123,182 entities (YAGO3-10), d = 256 for PairRE, d = 128 for BoxE.  Timed with HIP events around 5
repetitions after 2 warm-up runs; peak allocation (`torch.cuda.max_memory_allocated`) of one run of each path
on top of what the model and the batch hold.

    python profiles/bench_ranks_scorers.py            (needs the GPU)
"""

import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "bess-kge_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

from besskge import _native as nat  # noqa: E402
from besskge._native import RowSource  # noqa: E402
from besskge.bess import AllScoresBESS  # noqa: E402
from besskge.collectives import SingleProcessGroup  # noqa: E402
from besskge.negative_sampler import PlaceholderNegativeSampler  # noqa: E402
from besskge.scoring import BoxE, PairRE  # noqa: E402
from besskge.sharding import Sharding  # noqa: E402

dev = torch.device("cuda", 0)


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


def run(label, make, n_entity, n_rel, ew, rw, n_query, dtype):
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    sharding = Sharding.create(n_entity, 1, seed=0)
    ent = torch.randn(1, sharding.max_entity_per_shard, ew) * 0.3
    rel = torch.randn(n_rel, rw) * 0.3
    fn = make(sharding, n_rel, ent, rel).to(dev)
    if dtype == torch.float16:
        fn = fn.half()
    mod = AllScoresBESS(PlaceholderNegativeSampler("t"), fn, window_size=1000)
    mod.attach(SingleProcessGroup(1))
    batch = dict(head=torch.from_numpy(rng.integers(n_entity, size=(1, n_query)).astype(np.int32)).to(dev),
                 relation=torch.from_numpy(rng.integers(n_rel, size=(1, n_query)).astype(np.int32)).to(dev))
    truth = torch.from_numpy(rng.integers(n_entity, size=(1, n_query)).astype(np.int32)).to(dev)
    b = dict(batch, rank_truth=truth)
    half = dtype == torch.float16

    def counted():
        return mod.rank_counts_replicas([b])[0]

    def matrix():
        q = mod._gather_queries([batch])[0]
        table = mod._local_table(0)
        desc = fn.kernel_desc()
        rows = sharding.entity_to_idx[truth.reshape(-1).cpu().numpy()]
        rows_t = torch.from_numpy(np.ascontiguousarray(rows)).to(device=dev, dtype=torch.int64)
        ranks = []
        tile = max(64, (1 << 30) // 4 // n_entity)  # 1 GiB score tiles
        for q0 in range(0, n_query, tile):
            qq = q[q0:q0 + tile]
            sc = nat.neg_score_shared_fwd(desc, qq, RowSource(table[:n_entity]))
            if half:  # (scores leave AllScoresBESS in the model's dtype)
                sc = sc.half().float()
            r = torch.arange(qq.shape[0], device=dev)
            pos = sc[r, rows_t[q0:q0 + tile]].clone()
            sc[r, rows_t[q0:q0 + tile]] = -torch.inf
            ranks.append(nat.ranks_from_scores(pos, sc, 2, False))
        return torch.cat(ranks)

    tm, pm, rm = timed(matrix)
    tc, pc, rc = timed(counted)
    c = rc["counts"].float()
    agree = float(((1 + c[:, 0] + 0.5 * c[:, 1]) == rm).float().mean())
    g = n_query * n_entity / 1e6
    print(f"{label:34s} counted {tc:8.2f} ms ({g / tc:6.1f} G scores/s) peak {pc / 2**20:8.1f} MiB | "
          f"score matrix {tm:8.2f} ms ({g / tm:6.1f} G scores/s) peak {pm / 2**20:8.1f} MiB | ranks equal {agree:.4f}",
          flush=True)


if __name__ == "__main__":
    print(torch.cuda.get_device_name(0), flush=True)
    N, R, Q = 123_182, 37, 5000
    pair = lambda sh, n_rel, ent, rel: PairRE(True, 1, sh, n_rel, 256, ent, rel, normalize_entities=True)  # noqa: E731
    box = lambda sh, n_rel, ent, rel: BoxE(True, 1, sh, n_rel, 128, ent, rel, apply_tanh=True,  # noqa: E731
                                           dist_func_per_dim=True)
    run("YAGO3-10 PairRE d=256 fp16", pair, N, R, 256, 512, Q, torch.float16)
    run("YAGO3-10 PairRE d=256 fp32", pair, N, R, 256, 512, Q, torch.float32)
    run("YAGO3-10 BoxE d=128 fp32", box, N, R, 256, 4 * 128 + 2, Q, torch.float32)
