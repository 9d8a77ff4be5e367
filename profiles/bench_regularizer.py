#!/usr/bin/env python3
"""Embedding regulariser: what the one launch of `bess_regularize_triples` costs.

  kernel   the launch alone (N3: p = 3; gradient form, the rows' gradients added in place), replayed from a hipGraph:
             c2        ComplEx d = 256 fp32 (W = Wr = 512, moduli), S = 4096
             c4        TransE d = 256 fp16 (W = Wr = 256, coordinates), S = 512 - the notebook micro-batch
             s65536    ComplEx d = 256 fp16 (moduli), S = 65,536
           bytes = S * (2 W + Wr) * sz read + 2 * S * W * 8 read-modify-write, over the median time
  step     the C2 training step (ComplEx d = 256 fp32, per-triple negatives S = 4096, K = 256, log-sigmoid, SGD) and the
           C4 one (TransE d = 256 fp16, flat negatives S = 512, K = 32, augmentation, sampled softmax, SGD) with
           `EmbeddingRegularizer.n3(1e-3)` and without, eager (host time included) and replayed from a hipGraph
           (`Options.use_graphs`), the variants alternating in one process

`--inner` launches (steps) between a pair of HIP events, medians of `--repeats` pairs after `--warmup`.  Prints one JSON
line per measurement and writes them to `--out`."""
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
from besskge.bess import EmbeddingMovingBessKGE  # noqa: E402
from besskge.loss import LogSigmoidLoss, SampledSoftmaxCrossEntropyLoss  # noqa: E402
from besskge.negative_sampler import RandomShardedNegativeSampler  # noqa: E402
from besskge.regularizer import EmbeddingRegularizer  # noqa: E402
from besskge.scoring import ComplEx, TransE  # noqa: E402
from besskge.sharding import Sharding  # noqa: E402

KERNEL_SHAPES = {  # name: (dtype, W, Wr, flags, S, rows of the shard)
    "c2": (torch.float32, 512, 512, 3, 4096, 93_773),
    "c4": (torch.float16, 256, 256, 0, 512, 312_576),
    "s65536": (torch.float16, 512, 512, 3, 65_536, 312_576),
}

ap = argparse.ArgumentParser()
ap.add_argument("--parts", nargs="*", default=["kernel", "step"], choices=["kernel", "step"])
ap.add_argument("--repeats", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--inner", type=int, default=10)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_regularizer.json"))
args = ap.parse_args()

assert torch.cuda.is_available(), "this measurement needs a HIP device"
dev = torch.device("cuda", 0)
results = []


def alternate(runs, graph=False):
    """{label: [us per launch]} of `runs` = [(label, callable)], launched alternately.  `graph`: the `inner` launches
    are recorded once into a hipGraph and replayed between the events (the host cannot issue them as fast as they run)."""
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


kernel_us = {}
if "kernel" in args.parts:
    for name, (dtype, W, Wr, flags, S, rows) in KERNEL_SHAPES.items():
        gen = torch.Generator().manual_seed(S)
        table = (torch.rand(rows, W, generator=gen) * 2 - 1).to(dtype).to(dev)
        rel = (torch.rand(51, Wr, generator=gen) * 2 - 1).to(dtype).to(dev)
        head = nat.RowSource(table, torch.randint(rows, (S,), generator=gen, dtype=torch.int32).to(dev))
        tail = nat.RowSource(table, torch.randint(rows, (S,), generator=gen, dtype=torch.int32).to(dev))
        r_idx = torch.randint(51, (S,), generator=gen, dtype=torch.int32).to(dev)
        w = torch.ones(1, device=dev)
        dh, dt = torch.zeros(S, W, device=dev), torch.zeros(S, W, device=dev)
        d_rel = torch.zeros(51, Wr, device=dev)
        loss = torch.zeros((), device=dev)

        def launch():
            return nat.regularize_triples(head, tail, rel, r_idx, w, 3.0, 1e-3, 1e-3, 1.0, flags, dh, dt, d_rel, loss=loss)

        s = summary(alternate([("regularize", launch)], graph=True))
        sz = table.element_size()
        moved = S * (2 * W + Wr) * sz + 2 * S * W * 8
        kernel_us[name] = s["regularize_us"]
        emit(dict(part="kernel", shape=name, issue="graph replay", dtype=str(dtype), W=W, Wr=Wr, flags=flags, S=S,
                  bytes=moved, **s, gb_per_s=round(moved / s["regularize_us"] / 1e3, 1)))
        del table, dh, dt
        torch.cuda.empty_cache()

if "step" in args.parts:
    STEPS = {
        "c2": dict(scorer="ComplEx", rows=93_773, S=4096, K=256, flat=False, dtype=torch.float32),
        "c4": dict(scorer="TransE", rows=312_576, S=512, K=32, flat=True, dtype=torch.float16),
    }
    for name, c in STEPS.items():
        S, K, rows = c["S"], c["K"], c["rows"]
        sharding = Sharding.create(rows, 1, seed=0)
        rng = np.random.default_rng(0)
        batch = dict(head=rng.integers(rows, size=(1, 1, S)), relation=rng.integers(51, size=(1, 1, S)),
                     tail=rng.integers(rows, size=(1, 1, S)),
                     negative=rng.integers(rows, size=(1, 1, 1 if c["flat"] else S, K)))
        batch = {k: torch.from_numpy(v.astype(np.int32)).to(dev) for k, v in batch.items()}
        for graphs in (False, True):
            runners = {}
            for label, reg in (("plain", None), ("n3", EmbeddingRegularizer.n3(1e-3))):
                torch.manual_seed(0)
                ns = RandomShardedNegativeSampler(K, sharding, 0, "t", local_sampling=False, flat_negative_format=c["flat"])
                if c["scorer"] == "ComplEx":
                    fn = ComplEx(False, sharding, 51, 256, device=dev, dtype=c["dtype"])
                    model = EmbeddingMovingBessKGE(negative_sampler=ns, score_fn=fn, regularizer=reg,
                                                   loss_fn=LogSigmoidLoss(margin=6.0, negative_adversarial_sampling=True))
                else:
                    fn = TransE(True, 1, sharding, 51, 256, device=dev, dtype=c["dtype"])
                    model = EmbeddingMovingBessKGE(negative_sampler=ns, score_fn=fn, augment_negative=True, regularizer=reg,
                                                   loss_fn=SampledSoftmaxCrossEntropyLoss(n_entity=2_500_604))
                runners[label] = runtime.training_model(model, runtime.Options(use_graphs=graphs), runtime.SGD(lr=1e-3),
                                                        device=dev)

            def run_of(label):
                runner = runners[label]
                return lambda: runner(**batch)

            if not graphs:  # (the regularised step does launch the kernel; events inside a capture cannot be read)
                nat.start_kernel_timing(["bess_regularize_triples"])
                for label in runners:
                    run_of(label)()
                torch.cuda.synchronize()
                assert len(nat.stop_kernel_timing().get("bess_regularize_triples", [])) == 1
            s = summary(alternate([("plain", run_of("plain")), ("n3", run_of("n3"))]))
            res = dict(part="step", shape=name, issue="graph replay" if graphs else "eager (host time included)", S=S, K=K,
                       **s, ratio=round(s["n3_us"] / s["plain_us"], 3), added_us=round(s["n3_us"] - s["plain_us"], 2))
            if name in kernel_us:
                res["kernel_share_of_step"] = round(kernel_us[name] / s["n3_us"], 4)
            emit(res)
            del runners
            torch.cuda.empty_cache()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(results, f, indent=1)
    f.write("\n")
