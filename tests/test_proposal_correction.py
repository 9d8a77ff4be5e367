"""Sampled softmax over weighted negatives on the device: the loss kernel that lowers every score by its candidate's
log-proposal (`bess_loss_fwd_bwd_logq`) against float64 in every dispatch class, the device twin's `negative_logq`
(`bess_gather_negative_logq`) bit for bit against the host class, and the model's corrected training step - which
log-proposal goes with which score column, and the identity with the reference's loss for a uniform proposal."""

import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from besskge.batch_sampler import RandomShardedBatchSampler, RigidShardedBatchSampler
from besskge.dataset import KGDataset
from besskge.negative_sampler import WeightedShardedNegativeSampler
from besskge.sharding import PartitionedTripleSet, Sharding
from oracle import kge

N_ENTITY = 50_000  # of the loss (the kernel tests): lead_logq = -log(N_ENTITY - 1)
LOSS_SCALE = 1.5
# tolerances and rule of tests/test_mask_loss_rank_kernels.py, as they stand
LOSS_TOL = dict(rtol=2e-5, atol=1e-4)
GRAD_TOL = dict(rtol=1e-4, atol=1e-6)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda", 0)


def error_in_tolerances(x, ref, rtol, atol):
    """max |x - ref| / (atol + rtol |ref|): <= 1 is `assert_close`'s pass."""
    return float(((x.double() - ref).abs() / (atol + rtol * ref.abs())).max())


def close64(what, got, ref, e_oracle, rtol, atol):
    """`got` against the float64 `ref` at (rtol, atol) - or, where the fp32 CPU oracle is itself outside them
    (`e_oracle` > 1, in tolerances: the quantity is ill-conditioned in fp32 in that regime), at 4 x the oracle's error
    (a different summation order over up to 6148 terms).  The bound never depends on `got`."""
    assert bool(torch.isfinite(ref).all()) and got.shape == ref.shape
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    e_kernel = error_in_tolerances(got.cpu(), ref, rtol, atol)
    factor = 1.0 if e_oracle <= 1.0 else 4.0 * e_oracle
    if factor > 1.0 or e_kernel > 1.0:
        print(f"{what}: kernel at {e_kernel:.3g} x, fp32 oracle at up to {e_oracle:.3g} x of rtol={rtol} atol={atol}")
    assert e_kernel <= factor, f"{what}: kernel at {e_kernel:.3g} x the tolerance, fp32 oracle at {e_oracle:.3g} x"


# ----------------------------------------------------------------- loss kernel
def mrow(s, rows, ppp):
    """Row of the log-proposal table that triple `s` reads: the rule of `bess_mask_scores`."""
    if rows == 1:
        return 0
    if rows == 2:
        return 1 if s % ppp >= ppp // 2 else 0
    return s


# (S, N, logq_cols, logq_rows ("S": one per triple), ppp, one weight, counter, regime, logq misaligned by 4 bytes)
KERNEL_CASES = {
    "regs4_9x8": (9, 8, 8, "S", 0, False, True, "plain", False),
    "regs4_9x1024_one_row": (9, 1024, 1024, 1, 0, True, False, "plain", False),
    "regs4_8x12_ht_rows_lead4": (8, 12, 8, 2, 4, False, True, "plain", False),
    "regs12_5x1028": (5, 1028, 1028, "S", 0, True, True, "plain", False),
    "regs24_5x3076_lead1024": (5, 3076, 2052, 1, 0, False, False, "plain", False),
    "stream16_3x6148": (3, 6148, 6148, "S", 0, False, True, "plain", False),
    "stream16_3x6148_lead4_no_counter": (3, 6148, 6144, 1, 0, True, False, "plain", False),
    "bytes4_9x7_lead1": (9, 7, 6, "S", 0, False, True, "plain", False),
    "bytes4_6x12_lead6": (6, 12, 6, 1, 0, True, False, "plain", False),
    "bytes4_8x12_ht_rows_lead6": (8, 12, 6, 2, 4, False, True, "plain", False),
    "bytes4_9x8_misaligned_logq": (9, 8, 8, "S", 0, False, True, "plain", True),
    "bytes4_5x6151": (5, 6151, 6151, "S", 0, False, False, "plain", False),
    "two_launches_16388x4": (16388, 4, 4, "S", 0, False, True, "plain", False),
    "rare_negative_dominates_9x1024": (9, 1024, 1024, "S", 0, False, True, "rare", False),
}


@functools.lru_cache(maxsize=None)
def kernel_case(name):
    """Inputs (fp32, fixed seed, never written to) and {name: (float64 reference, fp32 restatement)} of one case."""
    S, N, cols, rows, ppp, one_w, _, regime, _ = KERNEL_CASES[name]
    rows = S if rows == "S" else rows
    gen = torch.Generator().manual_seed(1 + sorted(KERNEL_CASES).index(name))
    pos = torch.randn(S, generator=gen) * 4.0
    neg = torch.randn(S, N, generator=gen) * 4.0
    w = torch.rand(1 if one_w else S, generator=gen) + 0.5
    logq = -(torch.rand(rows, cols, generator=gen) * 9.0 + 3.0)  # proposals between e^-12 and e^-3
    if regime == "rare":
        # one candidate per row that the sampler almost never draws: its corrected logit is 30 above its score,
        # far above the positive - the row's loss is ~ that gap and the gradient sits on that candidate
        logq[torch.arange(rows), torch.arange(rows) * 37 % cols] = -30.0
    lead = -math.log(N_ENTITY - 1)
    full = torch.full((S, N), lead)
    for s in range(S):
        full[s, N - cols:] = logq[mrow(s, rows, ppp)]
    refs = []
    for dtype in (torch.float64, torch.float32):
        po, no = (x.detach().to(dtype, copy=True).requires_grad_(True) for x in (pos, neg))
        loss = kge.loss_value("ssce", po, no - full.to(dtype) - math.log(N_ENTITY - 1), w.expand(S).to(dtype),
                              loss_scale=LOSS_SCALE, n_entity=N_ENTITY)
        loss.backward()
        refs.append((loss.detach(), po.grad, no.grad))
    if regime == "rare":
        assert bool((refs[0][2].max(dim=1).values > 0.4 * LOSS_SCALE * w.expand(S).double()).all())
        assert float(refs[0][0]) > 20.0 * S
    return (pos, neg, w, logq), dict(zip(("loss", "d_pos", "d_neg"), zip(*refs)))


def launch_logq(dev, ld, pos, neg, w, logq, ppp, lead, counter=True, want_grad=True):
    """`bess_loss_fwd_bwd_logq` called directly (the wrapper always hands a counter over)."""
    from besskge import _native as nat

    S, N = neg.shape
    row_loss = torch.empty(S, device=dev)
    loss = torch.empty(1, device=dev)
    dp = torch.empty(S, device=dev) if want_grad else None
    dn = torch.empty(S, N, device=dev) if want_grad else None
    cnt = torch.zeros(nat.TICKET_INTS, dtype=torch.int32, device=dev) if counter else None
    nat._launch("bess_loss_fwd_bwd_logq", dev, ctypes.byref(ld), pos.data_ptr(), neg.data_ptr(), S, N, N, w.data_ptr(),
                w.numel(), row_loss.data_ptr(), loss.data_ptr(), dp.data_ptr() if want_grad else 0,
                dn.data_ptr() if want_grad else 0, N, 0, cnt.data_ptr() if counter else 0, logq.data_ptr(),
                logq.shape[0], logq.shape[1], ppp, lead)
    torch.cuda.synchronize()
    if counter:
        assert not bool(cnt.any())  # left at zero for the next call
    return loss.reshape(()), dp, dn


def corrected_loss():
    from besskge.loss import SampledSoftmaxCrossEntropyLoss

    return SampledSoftmaxCrossEntropyLoss(N_ENTITY, loss_scale=LOSS_SCALE, proposal_correction=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_logq_loss_kernel_against_float64(dev, name):
    S, N, cols, rows, ppp, one_w, counter, regime, misaligned = KERNEL_CASES[name]
    (pos, neg, w, logq), refs = kernel_case(name)
    fn = corrected_loss()
    ld = fn.kernel_desc(N)
    assert ld.ssce_shift == pytest.approx(-math.log(N)) and fn.lead_logq == pytest.approx(-math.log(N_ENTITY - 1))
    neg_d = neg.to(dev)
    if misaligned:
        store = torch.empty(logq.numel() + 1, device=dev)
        logq_d = store[1:].view(logq.shape)
        logq_d.copy_(logq)
        assert logq_d.data_ptr() % 16 == 4
    else:
        logq_d = logq.to(dev)
    loss, dp, dn = launch_logq(dev, ld, pos.to(dev), neg_d, w.to(dev), logq_d, ppp, fn.lead_logq, counter=counter)
    assert torch.equal(neg_d.cpu(), neg)  # the scores are not modified
    for what, got, tol in (("loss", loss, LOSS_TOL), ("d_pos", dp, GRAD_TOL), ("d_neg", dn, GRAD_TOL)):
        ref64, ref32 = refs[what]
        close64(f"{name}/{what}", got, ref64, error_in_tolerances(ref32, ref64, **tol), **tol)
    # the forward alone is the same number
    only, none_p, none_n = launch_logq(dev, ld, pos.to(dev), neg_d, w.to(dev), logq_d, ppp, fn.lead_logq, counter=counter,
                                       want_grad=False)
    assert none_p is None and none_n is None and torch.equal(only, loss)


@pytest.mark.gpu
def test_wrapper_loss_class_and_autograd(dev):
    """`nat.loss_fwd_bwd(..., logq=)`, `SampledSoftmaxCrossEntropyLoss.forward(..., negative_logq=)` and its autograd
    gradients are the direct call's; the class refuses a missing / unwanted / misshapen `negative_logq`."""
    from besskge import _native as nat
    from besskge.loss import LogSigmoidLoss, SampledSoftmaxCrossEntropyLoss

    name = "regs4_9x1024_one_row"
    (pos, neg, w, logq), refs = kernel_case(name)
    fn = corrected_loss()
    N = neg.shape[1]
    direct = launch_logq(dev, fn.kernel_desc(N), pos.to(dev), neg.to(dev), w.to(dev), logq.to(dev), 0, fn.lead_logq)
    via = nat.loss_fwd_bwd(fn.kernel_desc(N), pos.to(dev), neg.to(dev), w.to(dev), True, logq=logq.to(dev),
                           lead_logq=fn.lead_logq)
    for a, b in zip(direct, via):
        assert torch.equal(a, b)
    po, no = pos.to(dev).requires_grad_(True), neg.to(dev).requires_grad_(True)
    loss = fn(po, no, w.to(dev), negative_logq=logq.to(dev))
    loss.backward()
    assert torch.equal(loss.detach(), direct[0]) and torch.equal(po.grad, direct[1]) and torch.equal(no.grad, direct[2])
    with pytest.raises(ValueError, match="negative_logq"):
        fn(po, no, w.to(dev))
    with pytest.raises(ValueError, match="proposal_correction"):
        SampledSoftmaxCrossEntropyLoss(N_ENTITY)(po, no, w.to(dev), negative_logq=logq.to(dev))
    with pytest.raises(ValueError, match="proposal_correction"):
        LogSigmoidLoss(1.0, False)(po, no, w.to(dev), negative_logq=logq.to(dev))
    with pytest.raises(ValueError, match="does not match"):
        fn(po, no, w.to(dev), negative_logq=logq.to(dev)[:, :-4])
    with pytest.raises(RuntimeError):  # a kind the entry point does not take
        nat.loss_fwd_bwd(LogSigmoidLoss(1.0, False).kernel_desc(N), pos.to(dev), neg.to(dev), w.to(dev), True,
                         logq=logq.to(dev))


# -------------------------------------------------------------- device sampler
def skewed(n_entity, seed):
    """floor(zipf ** 0.75 * 1024) with a tenth of the entities at weight 0."""
    rng = np.random.default_rng(seed)
    w = np.floor(rng.zipf(1.6, size=n_entity).astype(np.float64) ** 0.75 * 1024).astype(np.int64)
    w[rng.choice(n_entity, size=n_entity // 10, replace=False)] = 0
    return w


def make(n_shard, shard_bs, scheme, flat, local, rigid, weights="skewed", n_entity=1000, n_rel=7, n_triple=4000, K=7,
         bps=2, seed=31, triples=None, return_logq=True, count=2):
    """Identical batch samplers over a weighted negative sampler (the host reference, the one handed to the twin)."""
    rng = np.random.default_rng(seed)
    if triples is None:
        triples = np.stack([rng.integers(n_entity, size=n_triple), rng.integers(n_rel, size=n_triple),
                            rng.integers(n_entity, size=n_triple)], axis=1)
    ds = KGDataset(n_entity=n_entity, n_relation_type=n_rel, triples={"train": triples},
                   original_triple_ids={"train": np.arange(triples.shape[0])})
    sharding = Sharding.create(n_entity, n_shard, seed=seed)
    pts = PartitionedTripleSet.create_from_dataset(ds, "train", sharding, partition_mode="ht_shardpair")
    w = skewed(n_entity, seed + 5) if isinstance(weights, str) else np.asarray(weights)

    def build():
        ns = WeightedShardedNegativeSampler(w, K, sharding, seed + 1, scheme, local, flat_negative_format=flat,
                                            return_logq=return_logq)
        cls = RigidShardedBatchSampler if rigid else RandomShardedBatchSampler
        return cls(partitioned_triple_set=pts, negative_sampler=ns, shard_bs=shard_bs, batches_per_step=bps, seed=seed + 2)

    return [build() for _ in range(count)]


def same(got, want, key):
    assert got.is_cuda
    g = got.cpu()
    assert g.dtype == want.dtype and tuple(g.shape) == tuple(want.shape), (key, g.dtype, want.dtype, g.shape, want.shape)
    assert torch.equal(g, want), key


@pytest.mark.gpu
@pytest.mark.parametrize("n_shard", [1, 3])
@pytest.mark.parametrize("scheme", ["h", "t", "ht"])
@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("local", [False, True])
def test_device_twin_returns_the_host_negative_logq(dev, n_shard, scheme, flat, local):
    """shard_bs 6 and 48, both batch samplers, three consecutive calls: `negative_logq` and every other key are the
    host's, bit for bit, and the stream goes back to the host where the host class left it."""
    from besskge.device_sampler import DeviceBatchSampler

    for shard_bs in (6, 48):
        for rigid in (False, True):
            host, twin = make(n_shard, shard_bs, scheme, flat, local, rigid)
            dbs = DeviceBatchSampler(twin, dev)
            order = list(host.get_dataloader_sampler(shuffle=False))
            for step in range(3):
                idx = order[step % len(order)]
                want, got = host[idx], dbs.sample(idx)
                assert set(got) == set(want) and "negative_logq" in want
                for k in want:
                    same(got[k], want[k], f"{step}/{k}")
            B = (2 if scheme == "ht" else 1) if flat else shard_bs
            assert tuple(want["negative_logq"].shape) == (2, n_shard, B, n_shard, 7)
            assert want["negative_logq"].dtype == torch.float32 and bool((want["negative_logq"] < 0).all())
            dbs.sync_host()
            assert host.negative_sampler.rng.bit_generator.state == twin.negative_sampler.rng.bit_generator.state


@pytest.mark.gpu
@pytest.mark.parametrize("local", [False, True])
@pytest.mark.parametrize("flat", [False, True])
def test_a_rank_that_draws_one_shard_of_three(dev, flat, local):
    """Every rank makes the rows of its own scoring shard - without local sampling from the blocks of all three source
    shards - and still hands back only its slice of the negatives."""
    from besskge.device_sampler import DeviceBatchSampler

    n = 3
    samplers = make(n, 48, "ht", flat, local, False, count=n + 1)
    host, ranks = samplers[0], [DeviceBatchSampler(t, dev, shards=range(r, r + 1)) for r, t in enumerate(samplers[1:])]
    for step in range(3):
        want = host[[0]]
        for r, dbs in enumerate(ranks):
            got = dbs.sample()
            assert set(got) == set(want)
            for k in want:
                same(got[k], want[k][:, r: r + 1], f"{step}/{r}/{k}")
    for dbs, twin in zip(ranks, samplers[1:]):
        dbs.sync_host()
        assert host.negative_sampler.rng.bit_generator.state == twin.negative_sampler.rng.bit_generator.state


@pytest.mark.gpu
@pytest.mark.parametrize("n_shard", [1, 2])
def test_negative_logq_together_with_the_filter(dev, n_shard):
    """`filter_triples` adds its mask and changes nothing else; also for the rank of the last shard alone."""
    from besskge.device_sampler import DeviceBatchSampler

    rng = np.random.default_rng(40)
    flat_ids = rng.choice(40 * 5 * 40, size=600, replace=False)
    h, rest = np.divmod(flat_ids, 5 * 40)
    r, t = np.divmod(rest, 40)
    triples = np.stack([h, r, t], axis=1).astype(np.int64)
    kw = dict(weights=1 + (np.arange(40) % 5) * 1000, n_entity=40, n_rel=5, triples=triples, K=6, count=4)
    host, plain, filtered, last = make(n_shard, 8 * n_shard, "ht", False, False, False, **kw)
    plain, filtered = DeviceBatchSampler(plain, dev), DeviceBatchSampler(filtered, dev, filter_triples=[triples])
    last = DeviceBatchSampler(last, dev, shards=range(n_shard - 1, n_shard), filter_triples=[triples])
    for step in range(2):
        want, a, b, c = host[[0]], plain.sample(), filtered.sample(), last.sample()
        assert set(a) == set(want) and set(b) == set(c) == set(want) | {"negative_mask"}
        for k in want:
            same(a[k], want[k], k)
            same(b[k], want[k], k)
            same(c[k], want[k][:, n_shard - 1:], k)
        assert torch.equal(b["negative_mask"][:, n_shard - 1:], c["negative_mask"]) and not bool(b["negative_mask"].all())


@pytest.mark.gpu
def test_gather_wrapper_clamps_and_refuses(dev):
    from besskge import _native as nat

    table = -torch.arange(1, 11, dtype=torch.float32, device=dev).reshape(2, 5)
    neg = torch.tensor([0, 4, 7, -3, 1, 2, 3, 4], dtype=torch.int32, device=dev).reshape(1, 2, 2, 1, 2)
    out = nat.gather_negative_logq(neg, table, 0, 0, 2, False)
    # [step, d, b, j, k] = table[j, neg[step, j, d, b, k]]; 7 and -3 are clamped to rows 4 and 0
    want = torch.tensor([[[-1., -5.], [-7., -8.]], [[-5., -1.], [-9., -10.]]]).reshape(1, 2, 1, 2, 2)
    assert torch.equal(out.cpu(), want)
    own = nat.gather_negative_logq(neg[:, 1:], table, 1, 1, 1, True)  # local: [d, b, j, k] = table[d, neg[d, j, b, k]]
    assert torch.equal(own.cpu(), torch.tensor([[-7., -8.], [-9., -10.]]).reshape(1, 1, 1, 2, 2))
    with pytest.raises(RuntimeError, match="every source shard"):
        nat.gather_negative_logq(neg[:, 1:], table, 1, 1, 1, False)
    with pytest.raises(ValueError, match="log_q"):
        nat.gather_negative_logq(neg, table[:1], 0, 0, 2, False)
    with pytest.raises(ValueError, match="negatives"):
        nat.gather_negative_logq(neg.long(), table, 0, 0, 2, False)


# ------------------------------------------------------------------------ model
D, N_REL, SHARD_BS = 32, 7, 12


def model_batch(n_shard, scheme, flat, weights, n_entity=1000, K=7):
    """One rigidly sampled micro-batch per shard (all triples real), as the runner takes it: {key: [n_shard, ...]}."""
    (bs,) = make(n_shard, SHARD_BS, scheme, flat, False, True, weights=weights, n_entity=n_entity, bps=1, K=K, count=1)
    full = bs[list(bs.get_dataloader_sampler(shuffle=False))[0]]
    assert bool(full["triple_mask"].all())
    return bs, {k: full[k][0] for k in ("head", "relation", "tail", "negative", "negative_logq")}


def build_runner(dev, bs, scorer, moving, loss, augment, opt, sharing=None):
    from besskge import runtime
    from besskge.bess import EmbeddingMovingBessKGE, ScoreMovingBessKGE
    from besskge.scoring import ComplEx, TransE

    ns = bs.negative_sampler
    sharding = ns.sharding
    gen = torch.Generator().manual_seed(5)
    W = D if scorer == "TransE" else 2 * D
    ent = 0.5 * torch.randn(sharding.n_shard, sharding.max_entity_per_shard, W, generator=gen)
    rel = 0.5 * torch.randn(N_REL, W, generator=gen)
    sharing = ns.flat_negative_format if sharing is None else sharing
    fn = TransE(sharing, 1, sharding, N_REL, D, ent, rel) if scorer == "TransE" else \
        ComplEx(sharing, sharding, N_REL, D, ent, rel)
    cls = EmbeddingMovingBessKGE if moving == "EM" else ScoreMovingBessKGE
    model = cls(ns, fn, loss, return_scores=True, augment_negative=augment)
    # Adam's first step is lr * g / (|g| + eps): it divides the fp32 rounding of a gradient sum (absolute, ~1e-7 for
    # terms below 1 - two routes that sum in different orders differ by that) by |g| + eps, so an element whose terms
    # nearly cancel moves by up to lr whatever the route did right.  With eps = 1e-3 two correct routes stay within
    # lr * 1e-7 / eps = 1e-6 of each other, below the golden test's atol of 2e-5; elements with |g| >> eps still move by lr.
    optimizer = dict(sgd=runtime.SGD(lr=0.1), adam=runtime.Adam(lr=0.01, eps=1e-3),
                     sgdm=runtime.SGD(lr=0.1, momentum=0.9))[opt]
    return model, runtime.training_model(model, runtime.Options(device_iterations=1), optimizer, device=dev)


def step(dev, runner, model, batch, timed=()):
    from besskge import _native as nat

    nat.start_kernel_timing(list(timed))
    out = runner(**{k: v.to(dev) for k, v in batch.items()})
    torch.cuda.synchronize()
    calls = {k: len(v) for k, v in nat.stop_kernel_timing().items()}
    return ({k: v.detach().float().cpu().clone() for k, v in out.items()},
            model.score_fn.entity_embedding.detach().float().cpu().clone(),
            model.score_fn.relation_embedding.detach().float().cpu().clone(), calls)


# (moving, n_shard, flat, augment): flat negatives with augmentation (EmbeddingMoving only; ScoreMoving scores flat
# negatives of n shards against n x n_shard x K candidates, which negative_logq does not cover: one shard) and per-triple
LAYOUTS = [("EM", 1, True, True), ("EM", 2, True, True), ("EM", 1, False, False), ("EM", 2, False, False),
           ("SM", 1, True, False), ("SM", 1, False, False), ("SM", 2, False, False)]
FUSED_CALLS = ["bess_neg_score_shared_fwd_loss", "bess_neg_score_pertriple_fwd_dq", "bess_neg_score_pertriple_fwd_partials",
               "bess_pertriple_tail", "bess_loss_fwd_bwd_one_launch", "bess_loss_fwd_bwd_logq"]


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["t", "ht"])
@pytest.mark.parametrize("moving,n_shard,flat,augment", LAYOUTS)
@pytest.mark.parametrize("scorer", ["TransE", "ComplEx"])
def test_returned_loss_is_the_float64_corrected_loss_of_the_returned_scores(dev, scorer, moving, n_shard, flat, augment,
                                                                            scheme):
    """Skewed weights.  The step's loss against float64 from the scores it returns (as scored: no shift, no correction)
    and the batch's `negative_logq` in its documented layout [scoring shard, B, n_shard, K] -> the last n_shard * K
    columns of the shard's score rows: pins which log-proposal goes with which column.  The step takes the two-pass
    route: one `bess_loss_fwd_bwd_logq` per replica, none of the fused forwards."""
    from besskge.loss import SampledSoftmaxCrossEntropyLoss

    n_entity = 1000
    bs, batch = model_batch(n_shard, scheme, flat, "skewed")
    loss_fn = SampledSoftmaxCrossEntropyLoss(n_entity, proposal_correction=True)
    model, runner = build_runner(dev, bs, scorer, moving, loss_fn, augment, "sgd")
    ent0 = model.score_fn.entity_embedding.detach().float().cpu().clone()
    out, ent, _, calls = step(dev, runner, model, batch, FUSED_CALLS)
    assert calls == {"bess_loss_fwd_bwd_logq": n_shard}, calls
    assert not torch.equal(ent, ent0)
    S = SHARD_BS
    pos = out["positive_score"].reshape(n_shard, S).double()
    neg = out["negative_score"].reshape(n_shard, S, -1).double()
    N = neg.shape[-1]
    lq = batch["negative_logq"].double()  # [d, B, n, K]
    cols = n_shard * 7
    assert N == cols + (0 if not augment else (S // 2 if scheme == "ht" else S))
    want = []
    for d in range(n_shard):
        rows = lq[d].reshape(lq.shape[1], cols)
        full = torch.full((S, N), -math.log(n_entity - 1), dtype=torch.float64)
        for s in range(S):
            b = 0 if rows.shape[0] == 1 else (s if rows.shape[0] == S else int(s % (S // n_shard) >= S // n_shard // 2))
            full[s, N - cols:] = rows[b]
        logits = torch.cat([pos[d][:, None], neg[d] - full - math.log(N)], dim=1)
        want.append((torch.logsumexp(logits, dim=1) - pos[d]).sum())
    got = out["loss"].reshape(n_shard).double()
    e = error_in_tolerances(got, torch.stack(want), **LOSS_TOL)
    assert e <= 1.0, (got, want, e)
    # the correction is not a small term here: without it the loss is another number
    plain = [(torch.logsumexp(torch.cat([pos[d][:, None], neg[d] + math.log(n_entity - 1) - math.log(N)], dim=1), dim=1)
              - pos[d]).sum() for d in range(n_shard)]
    assert error_in_tolerances(torch.stack(plain), torch.stack(want), **LOSS_TOL) > 100.0


@pytest.mark.gpu
@pytest.mark.parametrize("opt", ["sgd", "adam"])
@pytest.mark.parametrize("moving,n_shard,flat,augment", LAYOUTS)
@pytest.mark.parametrize("scorer", ["TransE", "ComplEx"])
def test_uniform_proposal_is_the_reference_loss(dev, scorer, moving, n_shard, flat, augment, opt):
    """All weights 1 on equal shards: every log-proposal is -log(n_entity), so the corrected logits are the
    reference's for `n_entity + 1` (shift log(n_entity) - log N).  Both losses are built with `n_entity + 1`, which the
    corrected one only reads for the augmented candidates (their uniform value is then the same number too).  One
    step of the new two-pass route against today's route - the fused calls where it takes them - on the same batch:
    loss and tables at the tolerances of the train-step golden test (tests/test_hip_parity.py) for fp32 tables."""
    from besskge.loss import SampledSoftmaxCrossEntropyLoss

    n_entity = 1000
    bs, batch = model_batch(n_shard, "t", flat, np.ones(n_entity, dtype=np.int64))
    assert len(set(bs.negative_sampler.shard_counts.tolist())) == 1
    torch.testing.assert_close(batch["negative_logq"], torch.full_like(batch["negative_logq"], -math.log(n_entity)),
                               rtol=0, atol=1e-6)
    res = []
    for corrected in (True, False):
        loss_fn = SampledSoftmaxCrossEntropyLoss(n_entity + 1, proposal_correction=corrected)
        model, runner = build_runner(dev, bs, scorer, moving, loss_fn, augment, opt)
        b = batch if corrected else {k: v for k, v in batch.items() if k != "negative_logq"}
        res.append(step(dev, runner, model, b, FUSED_CALLS))
    assert res[0][3] == {"bess_loss_fwd_bwd_logq": n_shard}, res[0][3]
    assert "bess_loss_fwd_bwd_logq" not in res[1][3]
    gen = torch.Generator().manual_seed(5)  # (the tables `build_runner` starts from)
    ent0 = 0.5 * torch.randn(res[0][1].shape, generator=gen)
    assert float((res[1][1] - ent0).abs().max()) > 100 * 2e-5  # the step moves rows by far more than the tolerance
    torch.testing.assert_close(res[0][0]["loss"], res[1][0]["loss"], rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(res[0][1], res[1][1], rtol=1e-4, atol=2e-5)
    torch.testing.assert_close(res[0][2], res[1][2], rtol=1e-4, atol=2e-5)
    # scores come back as scored; the reference's fp32 route returns them shifted (its in-place shift)
    N = res[0][0]["negative_score"].shape[-1]
    torch.testing.assert_close(res[0][0]["negative_score"] + (math.log(n_entity) - math.log(N)),
                               res[1][0]["negative_score"], rtol=1e-5, atol=1e-5)


@pytest.mark.gpu
def test_device_sampled_batch_trains_like_the_host_sampled_one(dev):
    """One corrected step (TransE, two shards in lock-step, per-triple "t") from the device twin's batch and from the
    host's: equal loss and tables, bit for bit.  SGD with momentum sums every row's contributions in a fixed order and
    every triple has a relation of its own, so the step is reproducible (tests/test_device_weighted_sampler.py)."""
    from besskge import runtime
    from besskge.bess import EmbeddingMovingBessKGE
    from besskge.device_sampler import DeviceBatchSampler
    from besskge.loss import SampledSoftmaxCrossEntropyLoss
    from besskge.scoring import TransE

    n_shard, n_rel = 2, 4000
    rng = np.random.default_rng(6)
    triples = np.stack([rng.integers(1000, size=n_rel), np.arange(n_rel), rng.integers(1000, size=n_rel)], axis=1)
    host, twin = make(n_shard, 48, "t", False, False, True, bps=1, n_rel=n_rel, triples=triples)
    sharding = host.negative_sampler.sharding
    idx = list(host.get_dataloader_sampler(shuffle=False))[0]
    from_host = {k: v.to(dev) for k, v in host[idx].items()}
    from_dev = DeviceBatchSampler(twin, dev).sample(idx)
    gen = torch.Generator().manual_seed(5)
    ent = 0.5 * torch.randn(n_shard, sharding.max_entity_per_shard, D, generator=gen)
    rel = 0.5 * torch.randn(n_rel, D, generator=gen)
    res = []
    for batch in (from_host, from_dev):
        fn = TransE(False, 1, sharding, n_rel, D, ent.clone(), rel.clone())
        model = EmbeddingMovingBessKGE(host.negative_sampler, fn,
                                       SampledSoftmaxCrossEntropyLoss(1000, proposal_correction=True))
        runner = runtime.training_model(model, runtime.Options(device_iterations=1), runtime.SGD(lr=0.1, momentum=0.9),
                                        device=dev)
        out = runner(**{k: batch[k][0] for k in ("head", "relation", "tail", "negative", "negative_logq")})
        torch.cuda.synchronize()
        res.append((out["loss"].detach().cpu().clone(), fn.entity_embedding.detach().cpu().clone(),
                    fn.relation_embedding.detach().cpu().clone()))
    assert not torch.equal(res[0][1], ent) and not torch.equal(res[0][2], rel)
    for a, b, what in zip(res[0], res[1], ("loss", "entity table", "relation table")):
        assert torch.equal(a, b), (what, float((a - b).abs().max()))


@pytest.mark.gpu
def test_the_model_refuses_what_the_correction_does_not_cover(dev):
    from besskge.loss import LogSigmoidLoss, SampledSoftmaxCrossEntropyLoss

    bs, batch = model_batch(1, "t", False, "skewed")
    on = SampledSoftmaxCrossEntropyLoss(1000, proposal_correction=True)
    model, runner = build_runner(dev, bs, "TransE", "EM", on, False, "sgd")
    table = model.score_fn.entity_embedding.detach().clone()
    with pytest.raises(ValueError, match="no `negative_logq`"):
        runner(**{k: v.to(dev) for k, v in batch.items() if k != "negative_logq"})
    with pytest.raises(ValueError, match="negative_logq has shape"):
        runner(**{k: (v[..., :-1].contiguous() if k == "negative_logq" else v).to(dev) for k, v in batch.items()})
    for off in (SampledSoftmaxCrossEntropyLoss(1000), LogSigmoidLoss(1.0, False)):
        _, plain = build_runner(dev, bs, "TransE", "EM", off, False, "sgd")
        with pytest.raises(ValueError, match="only taken by"):
            plain(**{k: v.to(dev) for k, v in batch.items()})
    _, shared = build_runner(dev, bs, "TransE", "EM", on, False, "sgd", sharing=True)
    with pytest.raises(ValueError, match="negative_sample_sharing"):
        shared(**{k: v.to(dev) for k, v in batch.items()})
    # ScoreMoving on two shards scores flat negatives against n_shard x n_shard x K candidates: not covered
    bs2, batch2 = model_batch(2, "t", True, "skewed")
    _, sm = build_runner(dev, bs2, "TransE", "SM", on, False, "sgd")
    with pytest.raises(ValueError, match="candidates per triple"):
        sm(**{k: v.to(dev) for k, v in batch2.items()})
    torch.cuda.synchronize()
    assert torch.equal(model.score_fn.entity_embedding.detach(), table)  # nothing was stepped


@pytest.mark.gpu
def test_example_trains_with_the_correction():
    """`examples/train_and_evaluate.py --negative-weights degree --loss ssce --proposal-correction`: device-sampled
    batches with `negative_logq` through the corrected step, two shards; the option is refused without its two needs."""
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    try:
        import train_and_evaluate
    finally:
        sys.path.pop(0)
    res = train_and_evaluate.main(["--steps", "120", "--n-shard", "2", "--negative-weights", "degree", "--loss", "ssce",
                                   "--proposal-correction"])
    assert res["losses"][-1] < 0.5 * res["losses"][0]
    assert res["hits@10"] > 0.2, res  # 2000 candidates: chance level is 0.005
    for argv in (["--proposal-correction"], ["--proposal-correction", "--loss", "ssce"],
                 ["--proposal-correction", "--negative-weights", "degree"]):
        with pytest.raises(SystemExit):
            train_and_evaluate.main(argv)
