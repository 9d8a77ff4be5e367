#!/usr/bin/env python3
"""Relation prediction: ComplEx d = 256 fp32 (W = 512), S = 4096 triples, R in {51, 237, 535}.

  fused    `bess_relation_lse_fwd` and `bess_relation_lse_bwd`
  forced   the route the library offered before them, launched alternately with the fused calls in one process:
           g(h, t) by torch ops, `nat.neg_score_shared_lse` / `nat.neg_score_shared_bwd_softmax` with the relation
           table as the candidates, the positive's term and the chain rule back to the rows by torch ops
  step     one `OneVsAllBessKGE` step (plain SGD, eager, host time included) at BASELINE config 2's shape with
           relation_prediction_weight 0 and 0.5, alternately

Medians of `--repeats` event pairs after `--warmup`, with [min, max].  One JSON line per measurement, all to `--out`."""
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
ap.add_argument("--relations", type=int, nargs="+", default=[51, 237, 535])
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_relation_prediction.json"))
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


def emit(res, v):
    res.update(ms=round(statistics.median(v), 3), ms_min_max=[round(min(v), 3), round(max(v), 3)],
               device=torch.cuda.get_device_name(0), repeats=args.repeats)
    print(json.dumps(res), flush=True)
    results.append(res)


def g_of(h, t):
    h1, h2, t1, t2 = h[:, :d], h[:, d:], t[:, :d], t[:, d:]
    return torch.cat([h1 * t1 + h2 * t2, h1 * t2 - h2 * t1], dim=1)


torch.manual_seed(0)
sharding = Sharding.create(M, 1, seed=0)
gen = torch.Generator().manual_seed(1)
hidx = torch.randint(M, (S,), generator=gen, dtype=torch.int32).to(dev)
tails = (torch.rand(S, W, generator=gen) * 2 - 1).to(dev)
coef = torch.ones(S, device=dev)
for R in args.relations:
    fn = ComplEx(True, sharding, R, d, device=dev)
    desc, table, rel = fn.kernel_desc(), fn.entity_embedding.data[0], fn.relation_embedding.data
    dot = nat.make_desc(nat.DISTMULT, 0, rel, W)  # an identity query against the relation rows
    rid = torch.randint(R, (S,), generator=gen, dtype=torch.int32).to(dev)
    head, tail = nat.RowSource(table, hidx), nat.RowSource(tails)
    lse = nat.relation_lse_fwd(desc, head, tail, rel)
    dh, dt, dr = torch.zeros(S, W, device=dev), torch.zeros(S, W, device=dev), torch.zeros(R, W, device=dev)
    ones = torch.ones(S, W, device=dev)

    def forced_fwd():
        state = nat.neg_score_shared_lse(dot, g_of(table[hidx.long()], tails), nat.RowSource(rel))
        return state[:, 0] + torch.log(state[:, 1])

    def forced_bwd():
        h = table[hidx.long()].requires_grad_(True)
        t = tails.clone().requires_grad_(True)
        g = g_of(h, t)
        dg, d_rel = nat.neg_score_shared_bwd_softmax(dot, g.detach(), nat.RowSource(rel), lse, coef)
        dg = dg - coef[:, None] * rel[rid.long()]  # the positive's term
        d_rel.index_add_(0, rid.long(), -coef[:, None] * g.detach())
        gh, gt = torch.autograd.grad(g, [h, t], dg)
        dh.add_(gh), dt.add_(gt), dr.add_(d_rel)

    times = alternate([
        ("fused_fwd", lambda: nat.relation_lse_fwd(desc, head, tail, rel)),
        ("forced_fwd", forced_fwd),
        ("fused_bwd", lambda: nat.relation_lse_bwd(desc, head, tail, rel, rid, lse, coef, dh, dt, dr)),
        ("forced_bwd", forced_bwd),
    ])
    for label, v in times.items():
        emit(dict(part="kernels", call=label, S=S, R=R, W=W), v)

fn = ComplEx(True, sharding, 51, d, device=dev)
rng = np.random.default_rng(0)
batch = {k: torch.from_numpy(rng.integers(hi, size=(1, 1, S)).astype(np.int32)).to(dev)
         for k, hi in (("head", M), ("relation", 51), ("tail", M))}
runners = []
for weight in (0.0, 0.5):
    model = OneVsAllBessKGE(PlaceholderNegativeSampler("t"), fn, SampledSoftmaxCrossEntropyLoss(M),
                            relation_prediction_weight=weight)
    runners.append((f"step_weight_{weight}", runtime.training_model(model, runtime.Options(device_iterations=1),
                                                                    runtime.SGD(lr=1e-3), device=dev)))
for label, v in alternate([(label, lambda r=r: r(**batch)) for label, r in runners]).items():
    emit(dict(part="step", call=label, issue="eager (host time included)", S=S, M=M, R=51, W=W), v)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(results, f, indent=1)
    f.write("\n")
