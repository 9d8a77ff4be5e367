"""The host side of the shard update in `besskge.bess` (no GPU needed): which way a step's shard updates go, the
"ht" split of the score gradients, the merge of accumulated per-triple groups, and the index built ahead as the
row-list helper accepts or refuses it."""

import types

import pytest
import torch


# ------------------------------------------------------------------ the route
def _optimisers(dense):
    from besskge import runtime

    kw = dict(dense=True) if dense else {}
    return dict(sgd=runtime.SGD(lr=0.1, **kw), momentum=runtime.SGD(lr=0.1, momentum=0.9, **kw),
                adagrad=runtime.Adagrad(lr=0.1, **kw), adam=runtime.Adam(lr=0.1, **kw))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_route_of_every_optimiser(dtype):
    """dense: `optimizer.dense`; atomic: plain SGD (a bare learning rate, or SGD without momentum and weight decay) on
    fp32 rows; coalesced: everything else - a bare learning rate then comes back as an optimiser object."""
    from besskge.bess import BessKGE, _PlainSGD

    route = BessKGE._update_route
    plain_route = "atomic" if dtype == torch.float32 else "coalesced"
    r, opt = route(0.25, dtype)
    assert r == plain_route
    if r == "coalesced":
        assert isinstance(opt, _PlainSGD) and opt.lr == 0.25 and opt.is_plain_sgd
    else:
        assert opt == 0.25
    want = dict(sgd=plain_route, momentum="coalesced", adagrad="coalesced", adam="coalesced")
    for name, o in _optimisers(False).items():
        assert route(o, dtype) == (want[name], o), name
    for name, o in _optimisers(True).items():
        assert route(o, dtype) == ("dense", o), name
        # the small lists are planned as if the rows were stepped sparsely (`_small_plan`)
        assert route(o, dtype, dense=False) == (want[name], o), name


# ------------------------------------------------------------- the "ht" split
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("ppp", [2, 3, 4])
def test_ht_split_equals_the_two_forms_it_replaces(n, ppp):
    from besskge.bess import _split_ht

    def same(got, want):
        assert len(got) == len(want) == 2
        for a, b in zip(got, want):
            assert a.shape == b.shape and torch.equal(a, b) and a.is_contiguous() and b.is_contiguous()

    cut = ppp // 2
    # EmbeddingMoving: d_neg [n * ppp, N]
    d_neg = torch.randn(n * ppp, 5)
    dn3 = d_neg.reshape(n, ppp, -1)
    same(_split_ht(d_neg, ppp), [dn3[:, :cut].reshape(-1, dn3.shape[-1]).contiguous(),
                                 dn3[:, cut:].reshape(-1, dn3.shape[-1]).contiguous()])
    # ScoreMoving: dsc [n, n * ppp, Nl] - contiguous, and as the paired all-to-all hands it over (a column window
    # of a wider buffer, which no reshape to [n * n, ppp, Nl] can view)
    wide = torch.randn(n, n * ppp * 7 + 3)
    for dsc in (torch.randn(n, n * ppp, 7), wide[:, : n * ppp * 7].reshape(n, n * ppp, 7)):
        d4 = dsc.reshape(n, n, ppp, -1)
        same(_split_ht(dsc, ppp), [d4[:, :, :cut].reshape(n * n * cut, -1).contiguous(),
                                   d4[:, :, cut:].reshape(n * n * (ppp - cut), -1).contiguous()])


# ------------------------------------------------------ the accumulation merge
class _Group:
    """Stand-in of a per-triple `_NegGroup`: what the merge reads."""

    def __init__(self, side, n_per_query, tag):
        self.side, self.n_per_query, self.tag = side, n_per_query, tag
        self.query = torch.full((2, 3), float(tag))
        self.neg = types.SimpleNamespace(idx=torch.full((2 * n_per_query,), tag, dtype=torch.int32))


def _pending(n_micro, n_shard, n_group, n_per_query=lambda micro: 4):
    from besskge.bess import _PendingUpdate, _ReplicaStep, _ShardGrads

    steps = [_ReplicaStep() for _ in range(n_shard)]
    for s, st in enumerate(steps):
        st.table = torch.zeros(6 + s, 3)
    pending, tag = [], 0
    for m in range(n_micro):
        shards = []
        for st in steps:
            sh = _ShardGrads(st)
            for k in range(n_group):
                tag += 1
                g = _Group(k % 2, n_per_query(m), tag)
                sh.segments.append((g, torch.full((2, n_per_query(m)), float(tag))))
            shards.append(sh)
        pending.append(_PendingUpdate(shards, torch.zeros(1)))
    return pending


def _by_slot_of_record(pending):
    """The merge as `apply_accumulated` wrote it before the gradients travelled per shard, on the flat list of
    (shard, group, d_scores) it had then: [(table, [(group, d_scores) of every micro-batch])] in launch order."""
    by_slot = {}
    for p in pending:
        deferred = [(sh.step.table, g, go) for sh in p.shards for g, go in sh.segments]
        seen = {}
        for table, g, go in deferred:
            k = seen.get((table.data_ptr(), g.side), 0)
            seen[(table.data_ptr(), g.side)] = k + 1
            by_slot.setdefault((table.data_ptr(), g.side, k), []).append((table, g, go))
    out = []
    for items in by_slot.values():
        table, g0, _ = items[0]
        if len(items) > 1 and any(g.n_per_query != g0.n_per_query for _, g, _ in items):
            raise RuntimeError("accumulated micro-batches differ in negatives per triple")
        out.append((table, [(g, go) for _, g, go in items]))
    return out


@pytest.mark.parametrize("n_group", [1, 2])
@pytest.mark.parametrize("n_shard", [1, 2])
@pytest.mark.parametrize("n_micro", [1, 3])
def test_accumulation_merge_equals_the_by_slot_loop(n_micro, n_shard, n_group):
    from besskge.bess import BessKGE

    pending = _pending(n_micro, n_shard, n_group)
    merged = BessKGE._merge_segments(pending)
    assert len(merged) == n_shard
    got = [(sh.step.table, items) for sh, slots in zip(pending[0].shards, merged) for items in slots]
    want = _by_slot_of_record(pending)
    assert len(got) == len(want) == n_shard * n_group
    for (table, items), (table_w, items_w) in zip(got, want):
        assert table is table_w and len(items) == len(items_w) == n_micro
        for (g, go), (g_w, go_w) in zip(items, items_w):
            assert g is g_w and go is go_w


def test_accumulation_merge_refuses_other_negatives_per_triple():
    from besskge.bess import BessKGE

    pending = _pending(3, 2, 2, n_per_query=lambda micro: 4 if micro < 2 else 5)
    with pytest.raises(RuntimeError, match="accumulated micro-batches differ in negatives per triple"):
        _by_slot_of_record(pending)
    with pytest.raises(RuntimeError, match="accumulated micro-batches differ in negatives per triple"):
        BessKGE._merge_segments(pending)


# ------------------------------------------- the index built ahead, as matched
class _Built:
    """What stands in for `nat.SegmentIndex` here: remembers what it was built from."""

    def __init__(self, ids, n_rows, scratch=None):
        self.ids, self.n_rows, self.scratch = ids, n_rows, scratch


@pytest.fixture
def row_lists(monkeypatch):
    from besskge import bess
    from besskge.update_state import UpdateState

    monkeypatch.setattr(bess.nat, "SegmentIndex", _Built)
    me = types.SimpleNamespace(update_state=UpdateState(), _match_ahead=bess.BessKGE._match_ahead)
    return lambda *args, **kw: bess.BessKGE._row_lists(me, *args, **kw)


def _lists(lengths):
    ids = [torch.arange(n, dtype=torch.int32) for n in lengths]
    return ids, [torch.randn(n, 4) for n in lengths]


def test_row_lists_take_the_index_of_exactly_these_lists(row_lists):
    from besskge.bess import _SmallPlan

    table = torch.zeros(50, 4)
    ids, grads = _lists([3, 5, 2])
    plan = _SmallPlan()
    plan.extend(ids)
    ahead = object()
    seg, out = row_lists(table, list(zip(ids, grads)), (plan, ahead), True)
    assert seg is ahead and len(out) == 3 and all(a is b for a, b in zip(out, grads))
    # one list fewer than planned: not the index of these lists
    seg, out = row_lists(table, list(zip(ids[:2], grads[:2])), (plan, ahead), True)
    assert isinstance(seg, _Built) and torch.equal(seg.ids, torch.cat(ids[:2])) and seg.n_rows == 50


def test_row_lists_take_a_named_concatenation_in_its_parts(row_lists):
    from besskge.bess import _SmallPlan

    table = torch.zeros(50, 4)
    parts, _ = _lists([3, 5])
    joined = torch.cat(parts)
    tail_ids, tail_grads = _lists([4])
    plan = _SmallPlan()
    plan.concats[0] = (joined.data_ptr(), 2)
    plan.extend(parts + tail_ids)
    g = torch.randn(8, 4)
    ahead = object()
    seg, out = row_lists(table, [(joined, g), (tail_ids[0], tail_grads[0])], (plan, ahead), True)
    assert seg is ahead and len(out) == 3
    assert torch.equal(out[0], g[:3]) and torch.equal(out[1], g[3:]) and out[2] is tail_grads[0]


@pytest.mark.parametrize("with_scratch", [True, False])
def test_row_lists_refuse_an_unplanned_list_of_the_planned_length(row_lists, with_scratch):
    """A list that merely has the length of the next planned ones must not reuse their index: a fresh one is built
    (with the shared scratch, or - next to a group's live index - without)."""
    from besskge.bess import _SmallPlan

    table = torch.zeros(50, 4)
    parts, _ = _lists([3, 5])
    plan = _SmallPlan()
    named = torch.cat(parts)  # (alive, so that the list handed over below is another tensor at another address)
    plan.concats[0] = (named.data_ptr(), 2)
    plan.extend(parts)
    stranger = torch.arange(10, 18, dtype=torch.int32)
    assert stranger.data_ptr() != named.data_ptr() and stranger.numel() == named.numel()
    g = torch.randn(8, 4)
    seg, out = row_lists(table, [(stranger, g)], (plan, object()), with_scratch)
    assert isinstance(seg, _Built) and torch.equal(seg.ids, stranger) and len(out) == 1 and out[0] is g
    assert (seg.scratch is not None) == with_scratch
