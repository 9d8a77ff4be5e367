"""Filtered negative sampling: an exact index of the known triples.

The random samplers draw entity ids blindly; on dense graphs a drawn "negative"
is often a triple of the training set, and the loss then pushes down a fact the
model is being taught.  `KnownTripleFilter` holds the known triples in a form
that one kernel (`csrc/known_triples.hip`) can probe for the S x C sampled
(query, candidate) pairs of a step, and produces the boolean `negative_mask`
that `BessKGE.forward` and the training step already accept: a masked-out
candidate scores `BAD_NEGATIVE_SCORE` and falls out of the loss and its
gradients.  `DeviceBatchSampler(..., filter_triples=...)` makes that mask for
every sampled batch.

Filtered evaluation asks the same index the other question - "list the known
completions of this query": `completions` (two passes of
`bess_known_completions`) returns them as a CSR pair on the device, and
`AllScoresPipeline(..., filter_triples=KnownTripleFilter(...))` builds every
batch's filter from it instead of comparing all queries with all filter triples
on the host.

The index is exact - no hashing: a mask is reproducible bit for bit.  One CSR
structure per corruption side:

  * side 0 / "t" (the tail is replaced): the sorted unique 64-bit keys
    `head * n_relation_type + relation` of the (head, relation) pairs that
    occur, an offset array, and the sorted, de-duplicated tails of each pair;
  * side 1 / "h" (the head is replaced): the same over
    `tail * n_relation_type + relation` and the heads.

Memory: 4 B per distinct triple and side for the completions plus 16 B per
distinct pair for keys and offsets - about 24 B per distinct triple for both
sides together when pairs have a few completions each, 40 B at the worst (every
pair with a single completion).  Every rank of a multi-GPU job holds the whole
index.
"""

from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch
from numpy.typing import NDArray

SIDE_TAIL, SIDE_HEAD = 0, 1  # which entity of the triple the candidates replace
_SIDES = {"t": SIDE_TAIL, "h": SIDE_HEAD, SIDE_TAIL: SIDE_TAIL, SIDE_HEAD: SIDE_HEAD}


def _csr(kept: NDArray[np.int64], relation: NDArray[np.int64], completion: NDArray[np.int64], n_relation: int
         ) -> Tuple[NDArray[np.int64], NDArray[np.int64], NDArray[np.int32]]:
    """(keys, offsets, completions) of the distinct (kept, relation, completion) rows."""
    key = kept * n_relation + relation
    order = np.lexsort((completion, key))
    key, completion = key[order], completion[order]
    new_key = np.ones(key.shape[0], dtype=bool)
    new_key[1:] = key[1:] != key[:-1]
    distinct = new_key.copy()
    distinct[1:] |= completion[1:] != completion[:-1]  # duplicate triples are neighbours now
    key, completion, new_key = key[distinct], completion[distinct], new_key[distinct]
    first = np.flatnonzero(new_key)
    offsets = np.concatenate([first, [key.shape[0]]]).astype(np.int64)
    return key[first].astype(np.int64), offsets, completion.astype(np.int32)


class KnownTripleFilter:
    """Exact membership index over known (head, relation, tail) triples in global entity ids (module docstring)."""

    def __init__(self, triples: Sequence[NDArray], n_entity: int, n_relation_type: int,
                 device: Optional[Union[torch.device, str]] = None) -> None:
        """
        :param triples: list of [n, 3] integer arrays of (head, relation, tail),
            global ids (train, and whatever else must not be drawn); duplicates
            within and across the arrays collapse.
        :param n_entity: number of entities.
        :param n_relation_type: number of relation types (inverse relations
            included when the triples carry them).
        :param device: HIP device the index is uploaded to (once); None: host
            only (`mask_host`), `to(device)` uploads later.
        """
        n_entity, n_relation_type = int(n_entity), int(n_relation_type)
        if n_entity <= 0 or n_relation_type <= 0:
            raise ValueError("n_entity and n_relation_type must be positive")
        if n_entity * n_relation_type >= 2 ** 63:
            raise ValueError(f"n_entity * n_relation_type = {n_entity * n_relation_type} does not fit a 64-bit key")
        if n_entity > 2 ** 31 - 1:
            raise ValueError("entity ids are 32-bit")
        if isinstance(triples, np.ndarray):
            triples = [triples]
        parts = []
        for t in triples:
            t = np.asarray(t)
            if t.ndim != 2 or t.shape[1] != 3 or not np.issubdtype(t.dtype, np.integer):
                raise ValueError(f"triples must be integer [n, 3] arrays, got {t.dtype} {t.shape}")
            parts.append(t.astype(np.int64))
        if not parts or sum(p.shape[0] for p in parts) == 0:
            raise ValueError("no triples to filter against")
        hrt = np.concatenate(parts, axis=0)
        h, r, t = hrt[:, 0], hrt[:, 1], hrt[:, 2]
        if h.min() < 0 or t.min() < 0 or max(h.max(), t.max()) >= n_entity:
            raise ValueError(f"entity id outside [0, {n_entity})")
        if r.min() < 0 or r.max() >= n_relation_type:
            raise ValueError(f"relation id outside [0, {n_relation_type})")
        self.n_entity = n_entity
        self.n_relation_type = n_relation_type
        #: per side (SIDE_TAIL, SIDE_HEAD): (keys int64 [P], offsets int64 [P + 1], completions int32 [n_triple])
        self.index_host = (_csr(h, r, t, n_relation_type), _csr(t, r, h, n_relation_type))
        #: distinct triples
        self.n_triple = int(self.index_host[SIDE_TAIL][2].shape[0])
        self._flat_host: list = [None, None]
        self.device: Optional[torch.device] = None
        self.index: Optional[Tuple[Tuple[torch.Tensor, ...], Tuple[torch.Tensor, ...]]] = None
        if device is not None:
            self.to(device)

    def to(self, device: Union[torch.device, str]) -> "KnownTripleFilter":
        """Upload the index (int64 keys and offsets, int32 completions) to `device`."""
        device = torch.device(device)
        if self.device != device:
            self.index = tuple(tuple(torch.from_numpy(a).to(device).contiguous() for a in side)  # type: ignore
                               for side in self.index_host)
            self.device = device
        return self

    @property
    def nbytes(self) -> int:
        """Bytes of the index (both sides)."""
        return int(sum(a.nbytes for side in self.index_host for a in side))

    # ------------------------------------------------------------------ host
    def _flat(self, side: int) -> NDArray[np.int64]:
        """pair * n_entity + completion of every triple: ascending, so that membership is one searchsorted."""
        if self._flat_host[side] is None:
            keys, off, comp = self.index_host[side]
            pair = np.repeat(np.arange(keys.shape[0], dtype=np.int64), np.diff(off))
            self._flat_host[side] = pair * self.n_entity + comp
        return self._flat_host[side]

    def mask_host(self, kept: NDArray, relation: NDArray, side: Union[int, str, NDArray], candidates: NDArray
                  ) -> NDArray[np.bool_]:
        """The meaning of `mask`, in numpy: `out[i, j]` is False iff
        (kept[i], relation[i], candidates[i, j]) - read as (h, r, t) where
        side is 0 / "t" and as (t, r, h) where it is 1 / "h" - is a known
        triple.  `candidates` is [rows, columns], or [columns] / [1, columns]
        shared by all rows; `side` one value or one per row.  Ids outside
        their range are never known."""
        kept = np.asarray(kept).astype(np.int64).reshape(-1)
        relation = np.asarray(relation).astype(np.int64).reshape(-1)
        cand = np.asarray(candidates).astype(np.int64)
        cand = np.broadcast_to(cand.reshape(-1, cand.shape[-1]) if cand.ndim > 1 else cand[None, :],
                               (kept.shape[0], cand.shape[-1]))
        if isinstance(side, (int, str)):
            side = np.full(kept.shape, _SIDES[side], dtype=np.uint8)
        side = np.asarray(side).reshape(-1) != 0
        out = np.ones(cand.shape, dtype=np.bool_)
        ok = (kept >= 0) & (kept < self.n_entity) & (relation >= 0) & (relation < self.n_relation_type)
        for s in (SIDE_TAIL, SIDE_HEAD):
            rows = np.nonzero(ok & (side == bool(s)))[0]
            keys = self.index_host[s][0]
            if rows.size == 0:
                continue
            key = kept[rows] * self.n_relation_type + relation[rows]
            pair = np.minimum(np.searchsorted(keys, key), keys.shape[0] - 1)
            rows, pair = rows[keys[pair] == key], pair[keys[pair] == key]
            c = cand[rows]
            flat = self._flat(s)
            q = pair[:, None] * self.n_entity + c
            at = np.minimum(np.searchsorted(flat, q), flat.shape[0] - 1)
            out[rows] = ~((flat[at] == q) & (c >= 0) & (c < self.n_entity))
        return out

    def completions_host(self, kept: NDArray, relation: NDArray, side: Union[int, str, NDArray],
                         skip: Optional[NDArray] = None, keep_entity: Optional[NDArray] = None,
                         kept_shard: Optional[NDArray] = None, local_to_global: Optional[NDArray] = None
                         ) -> Tuple[NDArray[np.int64], NDArray[np.int32]]:
        """The meaning of `completions`, in numpy: `ids[ptr[i]:ptr[i + 1]]` are, in ascending order, the entities
        e such that (kept[i], relation[i], e) - read as (h, r, t) where side is 0 / "t" and as (t, r, h) where it
        is 1 / "h" - is a known triple, without `skip[i]` (-1: none) and, with `keep_entity` (bool [n_entity]),
        without the entities it does not mark.  With `local_to_global` ([n_shard, rows per shard]) `kept[i]` is a
        local row of shard `kept_shard[i]` where that is >= 0.  A row whose kept id is negative, or whose kept id,
        shard, local row or relation is outside its range, has no completions."""
        kept = np.asarray(kept).astype(np.int64).reshape(-1)
        relation = np.asarray(relation).astype(np.int64).reshape(-1)
        if isinstance(side, (int, str)):
            side = np.full(kept.shape, _SIDES[side], dtype=np.uint8)
        side = np.asarray(side).reshape(-1) != 0
        ok = kept >= 0
        if kept_shard is not None:
            if local_to_global is None:
                raise ValueError("`kept_shard` needs `local_to_global`")
            table = np.asarray(local_to_global)
            shard = np.asarray(kept_shard).astype(np.int64).reshape(-1)
            local = shard >= 0
            ok &= ~local | ((shard < table.shape[0]) & (kept < table.shape[1]))
            at = local & ok
            kept = np.where(at, table[np.where(at, shard, 0), np.where(at, kept, 0)].astype(np.int64), kept)
        ok &= (kept < self.n_entity) & (relation >= 0) & (relation < self.n_relation_type)
        lists = []
        for i in range(kept.shape[0]):
            keys, off, comp = self.index_host[int(side[i])]
            row = comp[:0]
            if ok[i]:
                key = kept[i] * self.n_relation_type + relation[i]
                pair = int(np.searchsorted(keys, key))
                if pair < keys.shape[0] and keys[pair] == key:
                    row = comp[off[pair]: off[pair + 1]]
            if skip is not None:
                row = row[row != int(np.asarray(skip).reshape(-1)[i])]
            if keep_entity is not None:
                row = row[np.asarray(keep_entity).reshape(-1)[row] != 0]
            lists.append(row)
        ptr = np.zeros(kept.shape[0] + 1, dtype=np.int64)
        ptr[1:] = np.cumsum([len(x) for x in lists])
        return ptr, np.concatenate(lists + [np.zeros(0, dtype=np.int32)]).astype(np.int32)

    # ---------------------------------------------------------------- device
    def _sides(self, side: Union[int, str, torch.Tensor]) -> tuple:
        """(first index, second index or None, `side` vector or None) as the kernels take them."""
        if self.index is None:
            raise RuntimeError("the index is on the host only: call to(device) first")
        if isinstance(side, torch.Tensor):
            return self.index[SIDE_TAIL], self.index[SIDE_HEAD], side
        return self.index[_SIDES[side]], None, None

    def completions(self, kept: torch.Tensor, relation: torch.Tensor, side: Union[int, str, torch.Tensor],
                    skip: Optional[torch.Tensor] = None, keep_entity: Optional[torch.Tensor] = None,
                    kept_shard: Optional[torch.Tensor] = None, local_to_global: Optional[torch.Tensor] = None
                    ) -> Tuple[torch.Tensor, torch.Tensor]:
        """`completions_host` on the device (`bess_known_completions`): a count pass, a `cumsum` and a fill pass
        over the same rows; the one host read - the total - sizes `ids`.

        :param kept: int32 [rows]; :param relation: int32 [rows]; :param side: as for `mask`.
        :param skip: int32 [rows], an entity left out of every row's list (-1: none).
        :param keep_entity: bool / uint8 [n_entity], the only entities listed.
        :param kept_shard / local_to_global: as for `mask`.
        :return: (ptr int64 [rows + 1], ids int32 [ptr[-1]]) on the device.
        """
        query = dict(skip=skip, keep_entity=keep_entity, kept_shard=kept_shard, local_to_global=local_to_global)
        counts = self.count_completions(kept, relation, side, **query)
        ptr = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=kept.device)
        torch.cumsum(counts, 0, out=ptr[1:])
        ids = torch.empty(int(ptr[-1]), dtype=torch.int32, device=kept.device)
        if ids.numel():
            self.fill_completions(kept, relation, side, ptr[:-1], ids, **query)
        return ptr, ids

    def count_completions(self, kept: torch.Tensor, relation: torch.Tensor, side: Union[int, str, torch.Tensor],
                          **query: Optional[torch.Tensor]) -> torch.Tensor:
        """The count pass of `completions` alone: int32 [rows], the length of every row's list (`query`: `skip`,
        `keep_entity`, `kept_shard`, `local_to_global`)."""
        from besskge import _native as nat

        first, second, side_t = self._sides(side)
        keep_entity = query.get("keep_entity")
        if keep_entity is not None and keep_entity.numel() != self.n_entity:
            raise ValueError(f"`keep_entity` has {keep_entity.numel()} entries, the index {self.n_entity} entities")
        counts = torch.empty(int(kept.numel()), dtype=torch.int32, device=kept.device)
        return nat.known_completions(first, kept, relation, self.n_relation_type, index2=second, side=side_t,
                                     counts=counts, **query)

    def fill_completions(self, kept: torch.Tensor, relation: torch.Tensor, side: Union[int, str, torch.Tensor],
                         dst: torch.Tensor, out: torch.Tensor, tag: Optional[torch.Tensor] = None,
                         **query: Optional[torch.Tensor]) -> torch.Tensor:
        """The fill pass of `completions` alone, for callers with a layout of their own: row i's list starts at
        entry `dst[i]` (int64 [rows]) of `out` (int32); with `tag` (int32 [rows]) an entry is the pair
        (tag[i], entity) - `out` is [entries, 2] then.  Same rows and `query` as the count pass that sized `out`;
        what `dst` leaves between the lists is not touched."""
        from besskge import _native as nat

        first, second, side_t = self._sides(side)
        return nat.known_completions(first, kept, relation, self.n_relation_type, index2=second, side=side_t, dst=dst,
                                     out=out, out_stride=1 if tag is None else 2, tag=tag, **query)

    def mask(self, kept: torch.Tensor, relation: torch.Tensor, side: Union[int, str, torch.Tensor],
             candidates: torch.Tensor, out: Optional[torch.Tensor] = None, and_into: bool = False,
             cand_row: Optional[torch.Tensor] = None, local_to_global: Optional[torch.Tensor] = None,
             kept_shard: Optional[torch.Tensor] = None, cols_per_shard: int = 0) -> torch.Tensor:
        """`mask_host` on the device, in one kernel (`bess_known_triple_mask`).

        :param kept: int32 [rows] the entity of each query that stays.
        :param relation: int32 [rows].
        :param side: 0 / "t" (tails are replaced), 1 / "h", or uint8 / bool
            [rows] for rows of both kinds.
        :param candidates: int32 [rows, columns]; [1, columns] (or [columns]):
            one row shared by all; with `cand_row` (int32 [rows]): row
            `cand_row[i]` of `candidates` serves query i.
        :param out: bool / uint8 [rows, >= columns] to write into (columns past
            `columns` are left alone); with `and_into` entries are only
            cleared, so a padding mask keeps its zeros.
        :param local_to_global: int32 [n_shard, rows per shard]
            (`Sharding.shard_and_idx_to_entity`): the candidates are shard
            local rows, column j of shard `j // cols_per_shard`; `kept[i]` is a
            local row of shard `kept_shard[i]` where that is >= 0.
        :return: bool [rows, columns] (or `out`).
        """
        from besskge import _native as nat

        first, second, side_t = self._sides(side)
        n_row = int(kept.numel())
        if candidates.dim() == 1:
            candidates = candidates[None, :]
        n_col = int(candidates.shape[-1])
        shared = candidates.shape[0] == 1 and cand_row is None and n_row != 1
        if out is None:
            if and_into:
                raise ValueError("`and_into` needs the mask to combine with (`out`)")
            out = torch.empty((n_row, n_col), dtype=torch.bool, device=kept.device)
        nat.known_triple_mask(first, kept, relation, candidates, out, self.n_relation_type, index2=second, side=side_t,
                              kept_shard=kept_shard, n_col=n_col, ld_cand=0 if shared else n_col,
                              n_cand_row=int(candidates.shape[0]), cand_row=cand_row,
                              cols_per_block=int(cols_per_shard), block_stride=int(cols_per_shard),
                              local_to_global=local_to_global, and_into=and_into)
        return out
