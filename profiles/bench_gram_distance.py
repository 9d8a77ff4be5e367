"""TransE p = 2 over all entities: the direct tile kernels against the distance route of the split-fp16 product
(`distance_route="gram"`, BESS_FLAG_GRAM_L2), alternating in one process.

    python profiles/bench_gram_distance.py [--reps 15] -> profiles/bench_gram_distance.json

d = 256, 93,773 entities, S = 4096 queries, fp32 and fp16 tables; `neg_score_shared_lse`, `neg_score_shared_counts`
and `neg_score_shared_bwd_softmax`.  Every figure is the median of `reps` event pairs with [min, max]; a ratio counts
only where the two ranges do not overlap."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "bess-kge_amd"))
from besskge import _native as nat  # noqa: E402

W, N_ENTITY, S = 256, 93773, 4096


def desc(dtype, gram):
    d = nat.ModelDesc()
    d.scorer, d.norm_p, d.width, d.rel_width = nat.TRANSE, 2, W, W
    d.dtype = nat.F32 if dtype == torch.float32 else nat.F16
    if gram:
        d.reserved[0] |= nat.FLAG_GRAM_L2
    return d


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    query = (torch.randn(S, W, generator=g) * 0.5).to(dev)
    thr = torch.full((S,), -11.0, device=dev)
    excl = torch.full((S,), -1, dtype=torch.int32, device=dev)
    coef = torch.ones(S, device=dev)
    result = {"W": W, "n_entity": N_ENTITY, "S": S, "reps": args.reps, "cases": []}
    for dtype in (torch.float32, torch.float16):
        neg = nat.RowSource((torch.randn(N_ENTITY, W, generator=g) * 0.5).to(dtype).to(dev))
        lse = {}
        for gram in (False, True):
            st = nat.neg_score_shared_lse(desc(dtype, gram), query, neg)
            lse[gram] = (st[:, 0] + torch.log(st[:, 1])).contiguous()
        calls = {
            "neg_score_shared_lse": lambda gr: nat.neg_score_shared_lse(desc(dtype, gr), query, neg),
            "neg_score_shared_counts": lambda gr: nat.neg_score_shared_counts(desc(dtype, gr), query, neg, thr, excl),
            "neg_score_shared_bwd_softmax": lambda gr: nat.neg_score_shared_bwd_softmax(desc(dtype, gr), query, neg,
                                                                                        lse[gr], coef),
        }
        for name, call in calls.items():
            ms = {False: [], True: []}
            for gram in (False, True):  # warm-up
                call(gram)
            for _ in range(args.reps):
                for gram in (False, True):
                    ms[gram].append(timed(lambda: call(gram)))
            stat = {("gram" if k else "direct"): {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
                    for k, v in ms.items()}
            stat.update(call=name, dtype=str(dtype), speedup=stat["direct"]["median_ms"] / stat["gram"]["median_ms"],
                        ranges_overlap=not (stat["gram"]["max_ms"] < stat["direct"]["min_ms"]
                                            or stat["direct"]["max_ms"] < stat["gram"]["min_ms"]))
            print(json.dumps(stat))
            result["cases"].append(stat)
    out = os.path.join(os.environ.get("BENCH_OUT_DIR", os.path.dirname(os.path.abspath(__file__))),
                       "bench_gram_distance.json")
    with open(out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
