"""What a model keeps between training steps: per-table optimiser state and the update's scratch.

`BessKGE.update_state` is the one `UpdateState` of a model.  The update methods of `BessKGE` step it, `Runner`
snapshots it around a recording, `checkpoint` saves and loads it.  Depends on torch and `_native` only."""

from typing import Any, Dict, List, Optional, Tuple

import torch

from besskge import _native as nat


class TableState:
    """Optimiser state of one table (an entity shard, the relation table, a dense parameter)."""

    __slots__ = ("step", "s", "kind", "step_dev", "slot_map", "slot_counter", "capacity")

    def __init__(self, step: int = 0, kind: Optional[int] = None) -> None:
        self.step = step  #: updates taken, as the host counts them
        self.s: List[torch.Tensor] = []  #: fp32 state tensors (momentum | Adagrad's sum | Adam's two moments)
        self.kind = kind  #: BESS_OPT_* the tensors belong to (None: not stepped yet)
        self.step_dev: Optional[torch.Tensor] = None  #: int32[1] device-side count (Adam under graphs / plans)
        self.slot_map: Optional[torch.Tensor] = None  #: paged state: int32[rows] row -> state row, -1 = none yet
        self.slot_counter: Optional[torch.Tensor] = None  #: paged state: int32[1] state rows asked for so far
        self.capacity: Optional[int] = None  #: paged state: rows of each state pool

    @property
    def paged(self) -> bool:
        return self.slot_map is not None

    def ensure(self, table: torch.Tensor, n_state: int, state_rows: Optional[int] = None) -> "TableState":
        """At least `n_state` zeroed state tensors.  `state_rows` (the optimiser's option; only for tables with more
        rows than that) decides paging on first use: pools of that many rows plus a row -> state-row map, rows get
        a state row the first time they are stepped (a 128 GB shard cannot carry Adam's two fp32 tables of its own
        size)."""
        if state_rows is not None and int(state_rows) < table.shape[0] and not self.paged and n_state > 0:
            self.capacity = int(state_rows)
            self.slot_map = torch.full((table.shape[0],), -1, dtype=torch.int32, device=table.device)
            self.slot_counter = torch.zeros((1,), dtype=torch.int32, device=table.device)
        shape = (self.capacity, table.shape[1]) if self.paged else tuple(table.shape)
        while len(self.s) < n_state:
            self.s.append(torch.zeros(shape, dtype=torch.float32, device=table.device))
        return self

    def true_step(self) -> int:
        """Optimiser steps taken so far.  Under hipGraph replay only the device-side count advances (the host
        count is restored after the capture): the larger of the two is the truth."""
        if self.step_dev is None:
            return int(self.step)
        return max(int(self.step), int(self.step_dev.item()))

    def same_layout(self, n_state: int, paged: bool, capacity: Optional[int], shape: Tuple[int, ...], fresh: bool) -> bool:
        """Can state of this description be loaded into the live tensors (recordings on them stay valid)?  `fresh`:
        a description without optimiser history - the live state starts over, whatever it holds.  Fewer state
        tensors than live - a momentum checkpoint under Adam - is NOT the same layout: zeroed moments under the
        checkpoint's step count would skip Adam's bias correction, first updates ~30x too large."""
        return (self.paged == paged and (len(self.s) == n_state or fresh)
                and all(tuple(x.shape) == tuple(shape) for x in self.s) and (not paged or self.capacity == capacity))

    def snapshot(self) -> "TableState":
        old = TableState(self.step, self.kind)
        old.s = [t.clone() for t in self.s]
        old.step_dev = self.step_dev.clone() if self.step_dev is not None else None
        if self.paged:
            old.slot_map, old.slot_counter, old.capacity = self.slot_map.clone(), self.slot_counter.clone(), self.capacity
        return old

    def restore(self, old: Optional["TableState"]) -> None:
        """Back to `snapshot()`'s values, in the live tensors.  What was created (or grew) since - `old` is None
        or shorter - goes back to what it was: zero."""
        self.step = old.step if old else 0
        for i, t in enumerate(self.s):
            if old and i < len(old.s):
                t.copy_(old.s[i])
            else:
                t.zero_()
        if self.paged:  # which row owns which state row
            if old and old.paged:
                self.slot_map.copy_(old.slot_map)
                self.slot_counter.copy_(old.slot_counter)
            else:
                self.slot_map.fill_(-1)
                self.slot_counter.zero_()
        if self.step_dev is not None:
            if old and old.step_dev is not None:
                self.step_dev.copy_(old.step_dev)
            else:
                self.step_dev.fill_(self.step)


class _SegScratch(dict):
    """`SegmentIndex`'s scratch dict.  Replacing an entry (the long-row tier grew) frees buffers that recorded
    graphs and plans hold by address: the owner's generation moves on."""

    def __init__(self, owner: "UpdateState") -> None:
        super().__init__()
        self.owner = owner

    def __setitem__(self, key: Any, value: Any) -> None:
        if key in self:
            self.owner.stale()
        super().__setitem__(key, value)


class UpdateState:
    """Everything a model's update keeps across steps."""

    def __init__(self) -> None:
        self.tables: Dict[int, TableState] = {}  #: by `table.data_ptr()`
        self.device_step = False  #: Adam's step count lives on the device (set by a Runner that records steps)
        self.generation = 0  #: moves on when a tensor a recording may hold by address was replaced
        self.seg_scratch: dict = _SegScratch(self)  #: zeroed long-row scratch shared by the step's SegmentIndex objects
        self.direct: Dict[Any, Any] = {}  #: (table pointer, shape) -> nat.DirectAccumulator
        self.dense_segments: Dict[Any, Any] = {}  #: (table pointer, rows) -> identity segments

    def get(self, table: torch.Tensor) -> Optional[TableState]:
        return self.tables.get(table.data_ptr())

    def table_state(self, table: torch.Tensor, n_state: int, state_rows: Optional[int] = None) -> TableState:
        """The (lazily allocated) state of `table` with at least `n_state` state tensors."""
        st = self.tables.get(table.data_ptr())
        if st is None:
            st = self.tables[table.data_ptr()] = TableState()
        return st.ensure(table, n_state, state_rows)

    def stale(self) -> None:
        """Tensors were replaced: recordings hold the old addresses.  Runners compare `generation` with the one
        they recorded under and record again (`Runner._call_with_graphs`, `_call_with_plans`)."""
        self.generation += 1

    def drop(self, table: torch.Tensor) -> None:
        if self.tables.pop(table.data_ptr(), None) is not None:
            self.stale()

    def replace(self, table: torch.Tensor, state: TableState) -> None:
        self.tables[table.data_ptr()] = state
        self.stale()

    def rows_used(self) -> Dict[int, Tuple[int, int]]:
        """{table pointer: (state rows asked for so far, capacity)} of the tables with paged state."""
        return {key: (int(st.slot_counter.item()), st.capacity) for key, st in self.tables.items() if st.paged}

    def direct_scratch(self, table: torch.Tensor) -> Any:
        key = (table.data_ptr(), tuple(table.shape))
        if key not in self.direct:
            self.direct[key] = nat.DirectAccumulator(table)
        return self.direct[key]

    def identity_segments(self, table: torch.Tensor) -> Any:
        key = (table.data_ptr(), int(table.shape[0]))
        if key not in self.dense_segments:
            self.dense_segments[key] = nat.identity_segments(int(table.shape[0]), table.device)
        return self.dense_segments[key]

    def snapshot(self) -> Dict[int, TableState]:
        return {key: st.snapshot() for key, st in self.tables.items()}

    def restore(self, snap: Dict[int, TableState]) -> None:
        for key, st in self.tables.items():
            st.restore(snap.get(key))

    def for_replica(self) -> "UpdateState":
        """The state a replica of the model starts from (`MultiDeviceRunner`): the per-table entries the parent has,
        and scratch, caches and `device_step` of its own - replicas run on other devices, from other threads."""
        rep = UpdateState()
        rep.tables = dict(self.tables)
        return rep
