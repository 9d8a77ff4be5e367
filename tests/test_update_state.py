"""`besskge.update_state` (no GPU needed): the per-table optimiser state - allocation, paging, snapshot / restore,
the "same layout?" test -, what moves `UpdateState.generation`, what a replica shares, and the checkpoint files
`checkpoint._save_table` / `_load_table` write and read through it."""

import json

import pytest
import torch


def _table():
    return torch.arange(40, dtype=torch.float32).reshape(10, 4)


def _paged_adam(table):
    """One paged Adam table: step 3, device-side step 5, two state rows handed out."""
    from besskge.update_state import UpdateState

    states = UpdateState()
    st = states.table_state(table, 2, 4)
    st.step, st.kind = 3, 2
    st.step_dev = torch.tensor([5], dtype=torch.int32)
    st.s[0].fill_(1.0)
    st.s[1].fill_(2.0)
    st.slot_map[7], st.slot_map[2] = 0, 1
    st.slot_counter.fill_(2)
    return states, st


def test_ensure_full_size():
    from besskge.update_state import TableState

    table = _table()
    st = TableState().ensure(table, 1, None)
    first = st.s[0].data_ptr()
    st.ensure(table, 2, None)
    assert not st.paged and len(st.s) == 2 and st.s[0].data_ptr() == first
    for t in st.s:
        assert t.dtype == torch.float32 and tuple(t.shape) == (10, 4) and float(t.abs().max()) == 0.0
    assert st.step == 0 and st.kind is None and st.step_dev is None and st.capacity is None


def test_ensure_paged():
    from besskge.update_state import TableState

    table = _table()
    st = TableState().ensure(table, 2, 4)
    assert st.paged and st.capacity == 4
    assert [tuple(t.shape) for t in st.s] == [(4, 4), (4, 4)] and all(t.dtype == torch.float32 for t in st.s)
    assert st.slot_map.dtype == torch.int32 and tuple(st.slot_map.shape) == (10,) and bool((st.slot_map == -1).all())
    assert st.slot_counter.dtype == torch.int32 and int(st.slot_counter.item()) == 0
    for rows in (10, None):
        assert not TableState().ensure(table, 2, rows).paged


def test_snapshot_and_restore():
    table = _table()
    states, st = _paged_adam(table)
    tensors = [st.s[0], st.s[1], st.slot_map, st.slot_counter, st.step_dev]
    want = [t.clone() for t in tensors]
    snap = states.snapshot()
    st.step = 9
    for t in tensors:
        t.add_(3)
    states.restore(snap)
    assert st.step == 3
    for t, w in zip(tensors, want):
        assert torch.equal(t, w)
    assert all(a is b for a, b in zip([st.s[0], st.s[1], st.slot_map, st.slot_counter, st.step_dev], tensors))
    # a table the snapshot does not know: created since, goes back to nothing
    states.restore({})
    assert st.step == 0 and all(float(t.abs().max()) == 0.0 for t in st.s)
    assert bool((st.slot_map == -1).all()) and int(st.slot_counter.item()) == 0 and int(st.step_dev.item()) == st.step


def test_same_layout():
    from besskge.update_state import TableState

    table = _table()
    full = TableState().ensure(table, 2, None)
    assert full.same_layout(2, False, None, (10, 4), False)
    assert full.same_layout(0, False, None, (10, 4), True)  # a file without optimiser history
    assert not full.same_layout(1, False, None, (10, 4), False)  # a momentum checkpoint under live Adam
    assert not full.same_layout(2, True, 4, (4, 4), False)
    paged = TableState().ensure(table, 2, 4)
    assert paged.same_layout(2, True, 4, (4, 4), False)
    assert not paged.same_layout(2, False, None, (10, 4), False)
    assert not paged.same_layout(2, True, 5, (5, 4), False)
    assert not paged.same_layout(2, True, 5, (4, 4), False)  # the capacities differ, whatever the shapes say


def test_replace_and_drop_move_the_generation():
    from besskge.update_state import TableState, UpdateState

    table = _table()
    states = UpdateState()
    states.table_state(table, 1, None)
    assert states.generation == 0
    states.replace(table, TableState())
    assert states.generation == 1
    states.drop(table)
    assert states.generation == 2 and states.get(table) is None


def test_growing_long_row_scratch_moves_the_generation():
    from besskge import _native as nat
    from besskge.update_state import UpdateState

    states = UpdateState()
    dev = torch.device("cpu")

    def request(long_cap, width=4):
        seg = nat.SegmentIndex.__new__(nat.SegmentIndex)
        seg.long_cap = long_cap
        seg._long_scratch(dev, width, states.seg_scratch)
        return seg.long_count, seg.long_grad

    count, grad = request(3)
    assert states.generation == 0 and tuple(count.shape) == (3,) and tuple(grad.shape) == (3, 4)
    for cap in (3, 2):
        again = request(cap)
        assert again[0] is count and again[1] is grad and states.generation == 0
    other, _ = request(2, width=8)  # another width: another entry, nothing replaced
    assert other is not count and states.generation == 0
    bigger, _ = request(5)
    assert tuple(bigger.shape) == (5,) and states.generation == 1
    assert request(4)[0] is bigger and states.generation == 1


def test_for_replica():
    table = _table()
    states, st = _paged_adam(table)
    states.seg_scratch["key"] = 1
    rep = states.for_replica()
    assert rep.tables is not states.tables and rep.tables == states.tables and rep.get(table) is st
    assert rep.seg_scratch is not states.seg_scratch and not rep.seg_scratch
    assert rep.direct is not states.direct and rep.dense_segments is not states.dense_segments
    rep.device_step = True
    assert states.device_step is False
    rep.table_state(torch.zeros(3, 4), 1, None)  # a replica's own tables stay its own
    assert len(states.tables) == 1


def test_checkpoint_files_and_loading(tmp_path):
    from besskge import checkpoint
    from besskge.update_state import UpdateState

    table = _table()
    states, st = _paged_adam(table)
    checkpoint._save_table(states, table, tmp_path / "t", 4096)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["t.meta.json", "t.npy", "t.slots.npy", "t.state0.npy", "t.state1.npy"]
    with open(tmp_path / "t.meta.json") as f:
        meta = json.load(f)
    # what the commit before `update_state` wrote for this state, key for key and type for type
    want = {"step": 5, "n_state": 2, "paged": True, "kind": 2, "capacity": 4, "counter": 2, "step_dev": 5}
    assert meta == want and list(meta) == list(want)
    assert all(type(meta[k]) is type(v) for k, v in want.items())

    # into live state of the same layout: in place
    live = UpdateState()
    mine = live.table_state(table, 2, 4)
    mine.kind = 2
    mine.step_dev = torch.zeros((1,), dtype=torch.int32)
    tensors = [mine.s[0], mine.s[1], mine.slot_map, mine.slot_counter, mine.step_dev]
    ptrs = [t.data_ptr() for t in tensors]
    checkpoint._load_table(live, table, tmp_path / "t", 4096)
    assert live.generation == 0 and live.get(table) is mine
    assert [t.data_ptr() for t in (mine.s[0], mine.s[1], mine.slot_map, mine.slot_counter, mine.step_dev)] == ptrs
    assert mine.step == 5 and int(mine.step_dev.item()) == 5 and int(mine.slot_counter.item()) == 2
    assert torch.equal(mine.s[0], st.s[0]) and torch.equal(mine.s[1], st.s[1]) and torch.equal(mine.slot_map, st.slot_map)

    # into live state of another layout (full-size moments): replaced
    other = UpdateState()
    old = other.table_state(table, 2, None)
    checkpoint._load_table(other, table, tmp_path / "t", 4096)
    new = other.get(table)
    assert other.generation > 0 and new is not old and new.paged and new.capacity == 4 and new.kind == 2
    assert new.true_step() == 5 and torch.equal(new.s[1], st.s[1]) and torch.equal(new.slot_map, st.slot_map)

    # a kind the live tensors do not belong to is refused
    mine.kind = 1
    with pytest.raises(ValueError, match="optimiser kind"):
        checkpoint._load_table(live, table, tmp_path / "t", 4096)
