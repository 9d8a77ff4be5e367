"""Host side of the filtered top-k over all entities (besskge/pipeline.py: `rank_filter_pairs` as the exclusion
pairs of `AllScoresBESS.topk_replicas`; besskge/query.py: `threshold_below`), on the CPU: the pairs against a
brute-force loop over `filter_triples`, and the pruning thresholds against the definition of "the next value
below".  The launch-path / ABI invariants with the two new entry points are those of tests/test_launch_path.py and
tests/test_abi.py; the checks here name the new entry points explicitly."""

import inspect

import numpy as np
import pytest
import torch

from besskge.pipeline import AllScoresPipeline, rank_filter_pairs
from besskge.utils import get_entity_filter


def brute_force_pairs(slots, triples, truth, extra, scheme, candidate, keep_truth):
    """{(flat slot, entity)}: entity completes (h, r, ?) / (?, r, t) of the slot's query in `extra`."""
    col, other = (0, 2) if scheme == "t" else (2, 0)
    want = set()
    for s in slots:
        a, r = int(triples[s, col]), int(triples[s, 1])
        for row in extra.tolist():
            if row[col] == a and row[1] == r:
                e = row[other]
                if keep_truth and e == int(truth[s]):
                    continue
                if candidate is not None and not bool(candidate[e]):
                    continue
                want.add((s, e))
    return want


@pytest.mark.parametrize("scheme", ["t", "h"])
@pytest.mark.parametrize("subset", [False, True])
@pytest.mark.parametrize("with_truth", [True, False])
def test_exclusion_pairs_equal_a_brute_force_loop_over_the_filter(scheme, subset, with_truth):
    rng = np.random.default_rng(11)
    gen = torch.Generator().manual_seed(11)
    n_entity, n_rel, rows, shard_bs = 150, 4, 6, 8
    n_slot = rows * shard_bs
    keep = torch.rand(n_slot, generator=gen) > 0.2  # a padded batch
    triples = torch.from_numpy(np.stack([rng.integers(n_entity, size=n_slot), rng.integers(n_rel, size=n_slot),
                                         rng.integers(n_entity, size=n_slot)], axis=1))
    truth = triples[:, 2 if scheme == "t" else 0]
    kept = triples[keep]
    extra = torch.from_numpy(np.stack([rng.integers(n_entity, size=500), rng.integers(n_rel, size=500),
                                       rng.integers(n_entity, size=500)], axis=1))
    pick = torch.from_numpy(rng.integers(len(kept), size=300))
    if scheme == "t":
        extra[:300, :2] = kept[pick][:, :2]  # many queries share (h, r) with the filter
    else:
        extra[:300, 1:] = kept[pick][:, 1:]
    extra = torch.cat([extra, kept[:12], extra[:60]])  # the test triples themselves, and duplicates
    candidate = (torch.rand(n_entity, generator=gen) > 0.3) if subset else None
    flt = get_entity_filter(kept, extra, filter_mode=scheme)
    filt, per_kept = rank_filter_pairs(flt, keep, truth if with_truth else None, rows, shard_bs, candidate)
    assert filt.dtype == torch.int32 and filt.shape[0] == rows and filt.shape[2] == 2
    got, listed = set(), 0
    for r in range(rows):
        for qi, e in filt[r].tolist():
            if qi < 0:
                assert e == -1
                continue
            assert 0 <= qi < shard_bs
            got.add((r * shard_bs + qi, e))
            listed += 1
    assert listed == len(got), "a pair is listed twice"
    kept_slots = [int(s) for s in keep.nonzero().reshape(-1)]
    want = brute_force_pairs(kept_slots, triples, truth, extra, scheme, candidate, keep_truth=with_truth)
    assert got == want
    assert torch.equal(per_kept, torch.tensor([sum(1 for s_, _ in want if s_ == k) for k in kept_slots]))
    in_filter = [s for s in kept_slots[:12]]
    if with_truth:  # the first kept triples are in the filter: their truth stays
        assert all((s, int(truth[s])) not in got for s in in_filter)
    elif not subset:  # without a ground truth nothing is protected
        assert all((s, int(truth[s])) in got for s in in_filter)


def test_pruning_thresholds_are_the_next_values_below():
    from besskge.query import threshold_below

    tau = torch.tensor([0.0, 1.0, -1.0, 3.1415927, -2.5e-7, 1e-30, 65504.0, -65504.0, 1e20, -torch.inf, torch.inf])
    thr = threshold_below(tau, half=False)
    assert torch.equal(thr, torch.nextafter(tau, torch.full_like(tau, -torch.inf)))
    assert bool((thr[:-2] < tau[:-2]).all()) and thr[-2] == -torch.inf and torch.isfinite(thr[-1])
    # fp16: every fp16 value (as the kernels round them) against the sorted list of all fp16 values
    bits = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16)
    vals = bits.view(torch.float16).float()
    vals = torch.unique(vals[torch.isfinite(vals)])  # ascending, -0.0 == 0.0 once
    thr16 = threshold_below(vals, half=True)
    assert torch.equal(thr16[1:], vals[:-1]), "not the next fp16 value below"
    assert float(thr16[0]) < -65504.0
    # every f32 score that rounds to `v` or above lies above the threshold of `v`
    x = torch.linspace(-3.0, 3.0, 200_001)
    v = x.half().float()
    assert bool((x > threshold_below(v, half=True)).all())
    edge = threshold_below(torch.tensor([-torch.inf, torch.inf]), half=True)
    assert edge[0] == -torch.inf and edge[1] == 65504.0


def test_new_entry_points_are_bound_planned_and_timed_with_their_siblings():
    from besskge import _native
    from test_launch_path import launched_names, native_tree, plan_fns

    fns, launched = plan_fns(), launched_names(native_tree())
    for name in ("bess_topk_update_excl", "bess_topk_update_flagged_excl"):
        assert name in _native.SIGNATURES and name in fns and name in launched
        assert _native.TIMING_LABELS[name] == "bess_topk_update"
    assert len(_native.SIGNATURES["bess_topk_update_excl"]) == len(_native.SIGNATURES["bess_topk_update"]) + 4
    assert hasattr(_native.load(), "bess_topk_update_excl")
    lib = _native.load()
    # argument checks before any launch: list length, exclusion arrays that do not go together
    assert lib.bess_topk_update_excl(0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 129, 0) == -1
    assert lib.bess_topk_update_excl(0, 1, 1, 1, 0, 0, 0, 0, 0, 8, 0, 0, 0, 0, 0, 10, 0) == -1
    assert lib.bess_topk_update_flagged_excl(0, 1, 1, 1, 0, 4, 0, 0, 0, 8, 0, 0, 0, 0, 10, 0) == -1
    assert lib.bess_topk_update_excl(0, 0, 5, 8, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 10, 0) == 0  # no rows: nothing to do


def test_pipeline_takes_the_fused_topk_argument():
    assert inspect.signature(AllScoresPipeline.__init__).parameters["fused_topk"].default is True
