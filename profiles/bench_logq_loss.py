#!/usr/bin/env python3
"""Sampled softmax over weighted negatives: what the log-proposal costs.

  loss     `bess_loss_fwd_bwd_logq` against `bess_loss_fwd_bwd_one_launch` (same scores, forward + gradients), launched
           alternately in one process: 512 x 640, 4096 x 2048, 4096 x 256 (one log-proposal row for all triples - the
           flat format - and one per triple)
  gather   `bess_gather_negative_logq` at the shapes of section 23 (`bench_weighted_sampler.py`), as one rank runs it
  step     the C4 training step (TransE d = 256 fp16, flat negatives, augmentation, sampled softmax, SGD; S = 512,
           K = 32 - the notebook's - and S = 4096, K = 256) with the correction (two-pass route: scores, K7, loss) and
           without (the shared-negative scoring call finishes the loss itself), alternately

`--inner` launches (steps) between a pair of HIP events, medians of `--repeats` pairs after `--warmup`.  The launches
of `loss` and `gather` are replayed from a hipGraph (the host cannot issue them as fast as they run); the steps are
eager, host time included.  Prints one JSON line per measurement and writes them to `--out`."""
import argparse
import json
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "bess-kge_amd"), REPO]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from besskge import _native as nat  # noqa: E402
from besskge import runtime  # noqa: E402
from besskge.bess import EmbeddingMovingBessKGE  # noqa: E402
from besskge.loss import SampledSoftmaxCrossEntropyLoss  # noqa: E402
from besskge.negative_sampler import WeightedShardedNegativeSampler  # noqa: E402
from besskge.scoring import TransE  # noqa: E402
from besskge.sharding import Sharding  # noqa: E402

LOSS_SHAPES = [(512, 640), (4096, 2048), (4096, 256)]
GATHER_SHAPES = {  # name: (n_shard, rows per shard, B, K): bench_weighted_sampler.py
    "c2_pertriple": (1, 93_773, 4096, 256),
    "c4_flat_k32": (8, 312_576, 1, 32),
    "c4_flat_k2048": (8, 312_576, 1, 2048),
    "synthetic": (1, 62_500_000, 8192, 64),
}
STEP_SHAPES = [(512, 32), (4096, 256)]

ap = argparse.ArgumentParser()
ap.add_argument("--parts", nargs="*", default=["loss", "gather", "step"], choices=["loss", "gather", "step"])
ap.add_argument("--repeats", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--inner", type=int, default=10)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_logq_loss.json"))
args = ap.parse_args()

assert torch.cuda.is_available(), "this measurement needs a HIP device"
dev = torch.device("cuda", 0)
results = []


def alternate(runs, graph=False):
    """{label: [us per launch]} of `runs` = [(label, callable)], launched alternately.  `graph`: the `inner` launches
    are recorded once into a hipGraph and replayed between the events - issued from Python a call costs ~18 us of host
    time, more than these kernels take, and the events would time the host."""
    times = {label: [] for label, _ in runs}
    replays = {}
    if graph:
        for label, run in runs:
            run()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(args.inner):
                    run()
            replays[label] = g
    for it in range(args.warmup + args.repeats):
        for label, run in runs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            if graph:
                replays[label].replay()
            else:
                for _ in range(args.inner):
                    run()
            b.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                times[label].append(a.elapsed_time(b) * 1e3 / args.inner)
    return times


def summary(times):
    out = {}
    for label, v in times.items():
        out[f"{label}_us"] = round(statistics.median(v), 2)
        out[f"{label}_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
    return out


def emit(res):
    res.update(inner=args.inner, repeats=args.repeats, device=torch.cuda.get_device_name(0))
    print(json.dumps(res), flush=True)
    results.append(res)


if "loss" in args.parts:
    n_entity = 2_500_604
    plain_fn = SampledSoftmaxCrossEntropyLoss(n_entity)
    logq_fn = SampledSoftmaxCrossEntropyLoss(n_entity, proposal_correction=True)
    for S, N in LOSS_SHAPES:
        gen = torch.Generator().manual_seed(S + N)
        pos = (torch.randn(S, generator=gen) * 4).to(dev)
        neg = (torch.randn(S, N, generator=gen) * 4).to(dev)
        w = torch.ones(1, device=dev)
        for rows in (1, S):
            logq = (-(torch.rand(rows, N, generator=gen) * 9 + 3)).to(dev)
            ld_plain, ld_logq = plain_fn.kernel_desc(N), logq_fn.kernel_desc(N)

            def plain():
                return nat.loss_fwd_bwd(ld_plain, pos, neg, w, True)

            def corrected():
                return nat.loss_fwd_bwd(ld_logq, pos, neg, w, True, logq=logq, lead_logq=logq_fn.lead_logq)

            # a uniform proposal makes the two the same loss: the new call is checked against the old before it is timed
            flat = torch.full_like(logq, -math.log(n_entity - 1))
            same = nat.loss_fwd_bwd(ld_logq, pos, neg, w, True, logq=flat, lead_logq=logq_fn.lead_logq)
            torch.testing.assert_close(same[0], plain()[0], rtol=2e-5, atol=1e-4)
            torch.testing.assert_close(same[2], plain()[2], rtol=1e-4, atol=1e-6)
            t = alternate([("one_launch", plain), ("logq", corrected)], graph=True)
            s = summary(t)
            # bytes the call moves at least: scores read once, gradients written once (+ the log-proposals)
            emit(dict(part="loss", n_triple=S, n_neg=N, logq_rows=rows, issue="graph replay", **s,
                      ratio=round(s["logq_us"] / s["one_launch_us"], 3),
                      logq_gb_per_s=round((2 * S * N + rows * N) * 4 / s["logq_us"] / 1e3, 1),
                      one_launch_gb_per_s=round(2 * S * N * 4 / s["one_launch_us"] / 1e3, 1)))

if "gather" in args.parts:
    for name, (n_shard, rows, B, K) in GATHER_SHAPES.items():
        rng = np.random.default_rng(0)
        table = torch.from_numpy(-rng.random((n_shard, rows), dtype=np.float32) * 9 - 3).to(dev)
        neg = torch.from_numpy(rng.integers(rows, size=(1, n_shard, n_shard, B, K)).astype(np.int32)).to(dev)

        def gather():
            return nat.gather_negative_logq(neg, table, 0, 0, 1, False)

        got = gather()[0, 0].cpu()  # [B, n_shard, K] = table[j, neg[0, j, 0, b, k]]
        want = torch.stack([table[j].cpu()[neg[0, j, 0].cpu().long()] for j in range(n_shard)], dim=1)
        assert torch.equal(got, want), name
        s = summary(alternate([("gather", gather)], graph=True))
        n_out = B * n_shard * K
        emit(dict(part="gather", shape=name, issue="graph replay", n_shard=n_shard, rows_per_shard=rows, B=B, K=K,
                  values=n_out, table_mib=round(table.numel() * 4 / 2 ** 20, 1), **s,
                  values_per_s=round(n_out / s["gather_us"] * 1e6)))
        del table, neg
        torch.cuda.empty_cache()

if "step" in args.parts:
    n_ent, n_rel, d = 312_576, 535, 256
    sharding = Sharding.create(n_ent, 1, seed=0)
    rng = np.random.default_rng(0)
    weights = np.floor(rng.zipf(1.6, size=n_ent).astype(np.float64) ** 0.75 * 1024).astype(np.int64)
    for S, K in STEP_SHAPES:
        ns = WeightedShardedNegativeSampler(weights, K, sharding, 0, "t", False, flat_negative_format=True,
                                            return_logq=True)
        drawn = ns(np.zeros((1, 1, S), dtype=np.int64))
        batch = dict(head=rng.integers(n_ent, size=(1, 1, S)), relation=rng.integers(n_rel, size=(1, 1, S)),
                     tail=rng.integers(n_ent, size=(1, 1, S)), negative=drawn["negative_entities"][0])
        batch = {k: torch.from_numpy(v.astype(np.int32)).to(dev) for k, v in batch.items()}
        logq = torch.from_numpy(drawn["negative_logq"][0]).to(dev)
        runners = {}
        for corrected in (False, True):
            torch.manual_seed(0)
            fn = TransE(True, 1, sharding, n_rel, d, device=dev, dtype=torch.float16)
            model = EmbeddingMovingBessKGE(
                negative_sampler=ns, score_fn=fn, augment_negative=True,
                loss_fn=SampledSoftmaxCrossEntropyLoss(n_entity=2_500_604, proposal_correction=corrected))
            runner = runtime.training_model(model, runtime.Options(), runtime.SGD(lr=1e-3), device=dev)
            b = dict(batch, negative_logq=logq) if corrected else batch
            runners["corrected" if corrected else "fused"] = (runner, b)

        def run_of(key):
            runner, b = runners[key]
            return lambda: runner(**b)

        nat.start_kernel_timing(["bess_loss_fwd_bwd_logq", "bess_neg_score_shared_fwd_loss"])
        for key in runners:
            run_of(key)()
        torch.cuda.synchronize()
        calls = sorted(nat.stop_kernel_timing())
        assert calls == ["bess_loss_fwd_bwd_logq", "bess_neg_score_shared_fwd_loss"], calls
        s = summary(alternate([("fused", run_of("fused")), ("corrected", run_of("corrected"))]))
        emit(dict(part="step", S=S, K=K, n_neg=S + K, **s, ratio=round(s["corrected_us"] / s["fused_us"], 3),
                  note="eager steps, host time included: events around `inner` whole steps"))

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(results, f, indent=1)
    f.write("\n")
