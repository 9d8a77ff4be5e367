"""What a training step has decided (fused forward, loss in the scoring call, prologue launch, indices built
ahead, direct update, per-triple tail) travels in one per-step object (`besskge.bess._StepContext`), not through
the module's instance dict.  Two properties of that:

1. the step issues the same native calls in the same order as before the context existed: the ordered entry-point
   names of two consecutive weight updates, per configuration, equal the lists recorded at the parent commit
   (`tests/golden/step_calls.json`, written by `python tests/test_step_context.py --write --parent <commit id>`
   from a checkout of that commit with only this file added);
2. a step that raises leaves nothing behind on the model.
"""

import argparse
import json
import os

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (run as a script: puts the repository and the package on the path)
from test_oracle import load_bess_case

pytestmark = pytest.mark.gpu

CALLS_FILE = os.path.join(conftest.GOLDEN_DIR, "step_calls.json")
KEYS = ("head", "relation", "tail", "negative", "negative_mask")

GOLDEN_CASES = [
    "tr_EM_ComplEx0_ht_pt_n2",   # fused forward over received rows; two groups; C8
    "tr_EM_DistMult0_ht_pt_n2",
    "tr_EM_TransE1_ht_pt_n2",    # two-pass
    "tr_SM_ComplEx0_t_pt_n2",    # ScoreMoving: partials
    "tr_SM_ht_pt_n2",            # two groups per shard
    "tr_SM_ht_flat_n2",          # no partials
]
C4, ONE_SHARD = "c4_notebook", "one_shard_complex"
ONE_SHARD_HT, ONE_SHARD_F16 = ONE_SHARD + "_ht", ONE_SHARD + "_f16"
SYNTHETIC = (C4, ONE_SHARD, ONE_SHARD_HT, ONE_SHARD_F16)
# the routes of the shard update that the cases above leave out
ROUTE_CASES = [
    "tr_EM_ComplEx0_h_pt_n1",    # the "h" side
    "tr_EM_InterHT1_h_pt_n1",    # affine: segments that are no native scorer's - padded into one more row list
    "tr_EM_InterHT1_ht_pt_n2",   # ... two groups per shard
    "tr_EM_BoxE1_h_pt_n1",
    "tr_EM_ConvE0_t_flat_n1",    # the scorer's dense parameters
    "tr_EM_loc_aug_ht_flat_n4",  # augmentation, the planned concatenation, four shards
    ONE_SHARD_HT,                # two deferred groups on one fp32 table
]
COALESCE_FROM = 16  # `coalesce_sgd_from` of the "sgdcoalesce" configuration: below every update list of its case
OPTIMISERS = {
    "sgd": lambda rt: rt.SGD(lr=0.05),
    "adam": lambda rt: rt.Adam(lr=0.01),
    "adagrad": lambda rt: rt.Adagrad(lr=0.05),
    "sgdmomentum": lambda rt: rt.SGD(lr=0.05, momentum=0.9),
    "adampaged": lambda rt: rt.Adam(lr=0.01, state_rows=1024),  # (fewer than ONE_SHARD's 3000 rows)
    "sgddense": lambda rt: rt.SGD(lr=0.05, dense=True),
    "adamdense": lambda rt: rt.Adam(lr=0.01, dense=True),
    "sgdcoalesce": lambda rt: rt.SGD(lr=0.05),  # plain SGD's long-list coalescing (COALESCE_FROM)
}
# (case, optimiser, micro-batches per update, reduction)
CONFIGS = [(case, opt, 1, "sum") for case in GOLDEN_CASES + [C4, ONE_SHARD] for opt in ("sgd", "adam")]
CONFIGS += [(case, opt, 2, red) for case in (GOLDEN_CASES[0], GOLDEN_CASES[3], ONE_SHARD) for opt in ("sgd", "adam")
            for red in ("sum", "mean")]
CONFIGS += [(case, opt, 1, "sum") for case in ROUTE_CASES for opt in ("sgd", "adam")]
CONFIGS += [(ONE_SHARD, opt, 1, "sum") for opt in ("adagrad", "sgdmomentum", "adampaged", "sgddense", "adamdense")]
CONFIGS += [(C4, "sgddense", 1, "sum"), (C4, "adamdense", 1, "sum"),
            (ONE_SHARD_F16, "sgd", 1, "sum"),  # plain SGD on an f16 shard coalesces
            (GOLDEN_CASES[0], "sgdcoalesce", 1, "sum")]


def config_id(cfg):
    case, opt, accum, red = cfg
    return f"{case}-{opt}" + (f"-acc{accum}{red}" if accum > 1 else "")


def _synthetic(case, dev, micro):
    """(model, batch of `micro` micro-batches) of the one-shard shapes that are no golden case."""
    from besskge.bess import EmbeddingMovingBessKGE
    from besskge.loss import LogSigmoidLoss, SampledSoftmaxCrossEntropyLoss
    from besskge.negative_sampler import RandomShardedNegativeSampler
    from besskge.scoring import ComplEx, TransE
    from besskge.sharding import Sharding

    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    if case == C4:
        # `test_small_step.py::test_training_step_dispatch_count_c4_notebook_shape`: prologue launch (or its jobs
        # riding in the query launch), loss in the scoring call, the small lists' update without an index
        S, K, M, n_rel = 512, 32, 20_000, 50
        sharding = Sharding.create(M, 1, seed=0)
        fn = TransE(True, 1, sharding, n_rel, 256, device=dev, dtype=torch.float16)
        ns = RandomShardedNegativeSampler(K, sharding, 0, "t", local_sampling=False, flat_negative_format=True)
        model = EmbeddingMovingBessKGE(negative_sampler=ns, score_fn=fn, augment_negative=True,
                                       loss_fn=SampledSoftmaxCrossEntropyLoss(n_entity=M))
        neg_shape = (micro, 1, 1, K)
    else:
        # `test_small_step.py::test_training_step_through_the_pertriple_tail_equals_the_separate_launches`, fp32
        # ComplEx: per-triple negatives of the own shard (`pertriple_tail`, segmented update).  Its "ht" variant has
        # two such groups on the one table, its f16 variant a shard on which plain SGD coalesces
        S, K, M, n_rel = 192, 64, 3000, 9
        sharding = Sharding.create(M, 1, seed=0)
        fn = ComplEx(False, sharding, n_rel, 32, device=dev,
                     dtype=torch.float16 if case == ONE_SHARD_F16 else torch.float32)
        ns = RandomShardedNegativeSampler(K, sharding, 0, "ht" if case == ONE_SHARD_HT else "t", local_sampling=False,
                                          flat_negative_format=False)
        model = EmbeddingMovingBessKGE(negative_sampler=ns, score_fn=fn,
                                       loss_fn=LogSigmoidLoss(margin=4.0, negative_adversarial_sampling=True))
        neg_shape = (micro, 1, S, K)
    batch = dict(head=rng.integers(M, size=(micro, 1, S)), relation=rng.integers(n_rel, size=(micro, 1, S)),
                 tail=rng.integers(M, size=(micro, 1, S)), negative=rng.integers(M, size=neg_shape))
    return model, {k: torch.from_numpy(v.astype(np.int32)).to(dev) for k, v in batch.items()}


def build(cfg, dev):
    """(model, runner, the batch of one weight update) of a configuration, from scratch."""
    from besskge import runtime
    from test_hip_parity import build_model

    case, opt_name, accum, red = cfg
    if case in SYNTHETIC:
        model, batch = _synthetic(case, dev, accum)
    else:
        c = load_bess_case(case)
        model = build_model(c, dev)
        batch = {k: torch.stack([c["batch"][k][it] for it in range(accum)]).flatten(end_dim=1)
                 for k in KEYS if k in c["batch"]}
    opt = OPTIMISERS[opt_name](runtime)
    if opt_name == "sgdcoalesce":
        model.coalesce_sgd_from = COALESCE_FROM
    options = runtime.Options(device_iterations=1, gradient_accumulation=accum, accumulation_reduction=red)
    return model, runtime.training_model(model, options, opt, device=dev), batch


def logged(fn):
    """(result of fn(), entry-point names of the native calls it issued, in order)."""
    from besskge import _native as nat

    nat.start_kernel_timing(list(nat.SIGNATURES))
    try:
        out = fn()
        names = [entry[0] for entry in nat.kernel_timing_log()]
    finally:
        nat.stop_kernel_timing()
    return out, names


def two_updates(cfg, dev):
    """Two consecutive weight updates of a fresh model: (their native calls, entity table, relation table)."""
    model, runner, batch = build(cfg, dev)
    _, names = logged(lambda: [runner(**batch) for _ in range(2)])
    torch.cuda.synchronize()
    return names, model.score_fn.entity_embedding.detach().clone(), model.score_fn.relation_embedding.detach().clone()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def recorded():
    with open(CALLS_FILE) as f:
        return json.load(f)


@pytest.mark.parametrize("cfg", CONFIGS, ids=config_id)
def test_step_issues_the_recorded_calls_in_the_recorded_order(dev, recorded, cfg):
    """Same launches in the same order as the parent commit; and, where the parent's update is reproducible, the same
    bits from two fresh models.  `recorded["bit_identical"]` names those configurations: the ones whose tables were
    equal between three fresh models in every run of the parent (five runs of the writer; the file holds the lists
    of the first and the configurations that every run named - a single run names a few more, another few each
    time).  They are four: Adam on the 16-triple one-shard cases of InterHT, BoxE and ConvE, and plain SGD on the f16
    copy of the one-shard ComplEx step.  For all others the bit-for-bit assertion is dropped: every step sums the
    relation gradient - a few relations, many triples each - with fp32 atomics, whose order is not fixed; plain SGD
    on an fp32 shard adds every row contribution with an atomic too, the direct update and the dense step add
    gradient rows into their accumulator with atomics, and on two shards the gradients of the rows that came
    through the all-to-all are summed into the receive layout with atomics whatever the optimiser."""
    key = config_id(cfg)
    names, ent, rel = two_updates(cfg, dev)
    want = recorded["calls"][key]
    assert names == want
    if key in recorded["bit_identical"]:
        _, ent2, rel2 = two_updates(cfg, dev)
        assert torch.equal(ent, ent2) and torch.equal(rel, rel2)


@pytest.mark.parametrize("case", ["tr_EM_ComplEx0_ht_pt_n2", "tr_SM_ComplEx0_t_pt_n2"])
def test_a_step_that_raises_leaves_nothing_behind(dev, case):
    """`_fusable` is the first thing a training step calls, before any launch is queued.  After a step that died
    there, the model forwards and trains like a twin that never saw it.  (Before the step's state was an object of
    its own, ScoreMoving kept the training layout of its all-gathers for every later inference forward.)"""
    from test_hip_parity import close

    cfg = (case, "sgd", 1, "sum")
    c = load_bess_case(case)
    assert c["table"].dtype == torch.float32 and c["spec"].scorer == "ComplEx"
    model, runner, batch = build(cfg, dev)
    twin, twin_runner, _ = build(cfg, dev)
    lr = runner.optimizer.lr

    def broken(b):
        raise RuntimeError("no fuse description today")

    model._fusable = broken
    with pytest.raises(RuntimeError, match="no fuse description"):
        model.train_step_replicas(runner._split(batch, 0), runner.optimizer)
    del model._fusable

    outs = []
    for m, r in ((model, runner), (twin, twin_runner)):
        with torch.no_grad():
            outs.append(logged(lambda: m.forward_replicas(r._split(batch, 0))))
    (res, names), (res_twin, names_twin) = outs
    assert names == names_twin
    for a, b in zip(res, res_twin):
        for k in ("loss", "positive_score", "negative_score"):
            assert torch.equal(a[k], b[k]), k

    runner(**batch)
    twin_runner(**batch)
    for m in (model, twin):
        close(m.score_fn.entity_embedding, c["table"] - lr * c["grads"]["entity"], rtol=1e-4, atol=2e-5)
        close(m.score_fn.relation_embedding, c["rel"] - lr * c["grads"]["relation"].sum(0), rtol=1e-4, atol=2e-5)
    close(model.score_fn.entity_embedding, twin.score_fn.entity_embedding, rtol=1e-4, atol=2e-5)
    close(model.score_fn.relation_embedding, twin.score_fn.relation_embedding, rtol=1e-4, atol=2e-5)

    # caches appear once, nothing else does - on the model that saw the failed step as on its twin
    keys, fn_keys = set(twin.__dict__), set(twin.score_fn.__dict__)
    assert set(model.__dict__) == keys and set(model.score_fn.__dict__) == fn_keys
    runner(**batch)
    twin_runner(**batch)
    for m in (model, twin):
        assert set(m.__dict__) == keys and set(m.score_fn.__dict__) == fn_keys


def _write(path, parent):
    dev = torch.device("cuda", 0)
    calls, same = {}, []
    for cfg in CONFIGS:
        runs = [two_updates(cfg, dev) for _ in range(3)]
        assert all(r[0] == runs[0][0] for r in runs), config_id(cfg)
        calls[config_id(cfg)] = runs[0][0]
        if all(torch.equal(r[1], runs[0][1]) and torch.equal(r[2], runs[0][2]) for r in runs):
            same.append(config_id(cfg))
        print(config_id(cfg), len(runs[0][0]), "calls;", "bit-identical" if config_id(cfg) in same else "not bit-identical",
              flush=True)
    with open(path, "w") as f:
        json.dump(dict(parent=parent, bit_identical=same, calls=calls), f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description="record the native calls of the training steps at the current commit")
    ap.add_argument("--write", nargs="?", const=CALLS_FILE, required=True, metavar="PATH")
    ap.add_argument("--parent", required=True, help="id of the commit the lists are recorded at")
    args = ap.parse_args()
    _write(args.write, args.parent)
