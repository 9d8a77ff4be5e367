"""Listing the known completions of a query (besskge/negative_filter.py: `completions`, `completions_host`;
csrc/known_triples.hip: `bess_known_completions`): the numpy statement and the two kernel passes, each checked bit
for bit against lists made from a Python `set` of (head, relation, tail) tuples, never against each other."""

import ctypes

import numpy as np
import pytest
import torch

from besskge.negative_filter import SIDE_HEAD, SIDE_TAIL, KnownTripleFilter
from besskge.sharding import Sharding

N_ENT, N_REL, N_TRIPLE = 40, 5, 600


# ---------------------------------------------------------------- the oracle
def graph40():
    """600 distinct random triples over 40 entities and 5 relations (the graph of tests/test_negative_filter.py)."""
    rng = np.random.default_rng(40)
    flat = rng.choice(N_ENT * N_REL * N_ENT, size=N_TRIPLE, replace=False)
    h, rest = np.divmod(flat, N_REL * N_ENT)
    r, t = np.divmod(rest, N_ENT)
    return np.stack([h, r, t], axis=1).astype(np.int64)


def as_set(*arrays):
    return {tuple(int(x) for x in row) for a in arrays for row in np.asarray(a)}


def brute_lists(known, kept, relation, side, skip=None, keep=None):
    """Per row the ascending list of the entities e with (kept, relation, e) - side 0 - or (e, relation, kept) -
    side 1 - in the set, without skip[i] and without the entities `keep` does not mark."""
    by_pair = ({}, {})
    for h, r, t in known:
        by_pair[0].setdefault((h, r), set()).add(t)
        by_pair[1].setdefault((t, r), set()).add(h)
    kept, relation = np.asarray(kept).reshape(-1), np.asarray(relation).reshape(-1)
    side = np.broadcast_to(np.asarray(side), kept.shape)
    out = []
    for i in range(kept.shape[0]):
        row = by_pair[int(side[i])].get((int(kept[i]), int(relation[i])), set())
        if skip is not None:
            row = row - {int(skip[i])}
        if keep is not None:
            row = {e for e in row if keep[e]}
        out.append(sorted(row))
    return out


def flat(lists):
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(x) for x in lists])
    return ptr, np.array([e for row in lists for e in row], dtype=np.int32)


# --------------------------------------------------------------------- CPU
@pytest.fixture(scope="module")
def host40():
    triples = graph40()
    flt = KnownTripleFilter([triples[:400], triples[300:]], N_ENT, N_REL)  # overlapping parts collapse
    assert flt.n_triple == N_TRIPLE
    return flt, as_set(triples)


@pytest.mark.parametrize("side", [0, 1, "mixed"])
def test_completions_host_against_a_set(host40, side):
    flt, known = host40
    rng = np.random.default_rng(3 + (7 if side == "mixed" else side))
    n = 80
    kept, rel = rng.integers(N_ENT, size=n), rng.integers(N_REL, size=n)
    sd = rng.integers(2, size=n).astype(np.uint8) if side == "mixed" else side
    lists = brute_lists(known, kept, rel, sd)
    ptr, ids = flt.completions_host(kept, rel, sd)
    want_ptr, want_ids = flat(lists)
    assert ptr.dtype == np.int64 and ids.dtype == np.int32
    assert np.array_equal(ptr, want_ptr) and np.array_equal(ids, want_ids)
    assert ptr[-1] > 100 and min(len(x) for x in lists) == 0 and max(len(x) for x in lists) >= 5
    if side != "mixed":  # "t" / "h" spelling
        ptr2, ids2 = flt.completions_host(kept, rel, "th"[side])
        assert np.array_equal(ptr2, ptr) and np.array_equal(ids2, ids)
    # skip: a member (first / last of the list), a non-member, -1
    skip = np.full(n, -1, dtype=np.int64)
    member = np.zeros(n, dtype=bool)
    for i, row in enumerate(lists):
        if i % 4 == 0 and row:
            skip[i], member[i] = row[0], True
        elif i % 4 == 1 and row:
            skip[i], member[i] = row[-1], True
        elif i % 4 == 2:
            skip[i] = next(e for e in range(N_ENT) if e not in row)
    ptr_s, ids_s = flt.completions_host(kept, rel, sd, skip=skip)
    want_ptr, want_ids = flat(brute_lists(known, kept, rel, sd, skip=skip))
    assert np.array_equal(ptr_s, want_ptr) and np.array_equal(ids_s, want_ids)
    assert member.sum() > 10 and np.array_equal(np.diff(ptr) - np.diff(ptr_s), member.astype(np.int64))
    # a subset of the entities, alone and with skip
    keep = rng.random(N_ENT) < 0.6
    for sk in (None, skip):
        ptr_k, ids_k = flt.completions_host(kept, rel, sd, skip=sk, keep_entity=keep)
        want_ptr, want_ids = flat(brute_lists(known, kept, rel, sd, skip=sk, keep=keep))
        assert np.array_equal(ptr_k, want_ptr) and np.array_equal(ids_k, want_ids)
        assert 0 < ptr_k[-1] < ptr[-1] and keep[ids_k].all()


def test_completions_host_rows_that_name_no_pair(host40):
    flt, known = host40
    some = next(iter(known))
    kept = np.array([some[0], -1, N_ENT, some[0], some[0], some[0]])
    rel = np.array([some[1], some[1], some[1], N_REL, -1, some[1]])
    ptr, ids = flt.completions_host(kept, rel, 0)
    full = brute_lists(known, [some[0]], [some[1]], 0)[0]
    assert len(full) >= 1 and some[2] in full
    assert list(np.diff(ptr)) == [len(full), 0, 0, 0, 0, len(full)]
    assert list(ids) == full + full


def test_completions_host_local_rows(host40):
    """The entity that stays as a local row of a 3-shard sharding: rows of their shard, rows that are global
    (shard -1), a padding row, a row past the table, a shard that does not exist."""
    flt, known = host40
    sharding = Sharding.create(N_ENT, 3, seed=5)
    table = sharding.shard_and_idx_to_entity
    assert table.shape == (3, 14) and (table >= N_ENT).sum() == 2  # two padding rows
    rng = np.random.default_rng(9)
    n = 60
    glob = rng.integers(N_ENT, size=n)
    rel = rng.integers(N_REL, size=n)
    sd = rng.integers(2, size=n).astype(np.uint8)
    shard = sharding.entity_to_shard[glob].astype(np.int32)
    kept = sharding.entity_to_idx[glob].astype(np.int32)
    as_global = np.arange(n) % 5 == 0
    shard[as_global], kept[as_global] = -1, glob[as_global]
    ptr, ids = flt.completions_host(kept, rel, sd, kept_shard=shard, local_to_global=table)
    want_ptr, want_ids = flat(brute_lists(known, glob, rel, sd))
    assert np.array_equal(ptr, want_ptr) and np.array_equal(ids, want_ids) and ptr[-1] > 100
    pad_shard, pad_row = (int(x[0]) for x in np.nonzero(table >= N_ENT))
    kept = np.array([pad_row, table.shape[1], 0, 0], dtype=np.int32)
    shard = np.array([pad_shard, 0, 3, 0], dtype=np.int32)
    rel = np.zeros(4, dtype=np.int32)
    ptr, ids = flt.completions_host(kept, rel, 0, kept_shard=shard, local_to_global=table)
    last = brute_lists(known, [table[0, 0]], [0], 0)[0]
    assert list(np.diff(ptr)) == [0, 0, 0, len(last)] and list(ids) == last
    with pytest.raises(ValueError, match="local_to_global"):
        flt.completions_host(kept, rel, 0, kept_shard=shard)


def last_error(lib):
    buf = ctypes.create_string_buffer(256)
    lib.bess_last_error(buf, 256)
    return buf.value.decode()


def test_entry_point_validates_before_it_launches():
    """No device needed: nothing is dereferenced before the arguments have been checked (the pointers below are
    addresses of host arrays), and an empty problem is fine with nothing else given."""
    from besskge import _native as nat

    lib = nat.load()
    assert "bess_known_completions" in nat.SIGNATURES
    keys, off = np.zeros(1, dtype=np.int64), np.array([0, 1], dtype=np.int64)
    comp, vec = np.zeros(1, dtype=np.int32), np.zeros(4, dtype=np.int32)
    wide, big = np.zeros(4, dtype=np.int64), np.zeros(64, dtype=np.int32)
    bytes_ = np.zeros(4, dtype=np.uint8)
    p = lambda a: a.ctypes.data  # noqa: E731

    def call(n_row=4, index2=False, side=0, keep=0, n_entity=0, counts=0, dst=0, out=0, n_out=0, stride=1, tag=0):
        second = (p(keys), p(off), 1, p(comp)) if index2 else (0, 0, 0, 0)
        return lib.bess_known_completions(p(keys), p(off), 1, p(comp), *second, p(vec), 0, p(vec), side, n_row, N_REL,
                                          0, 0, 0, 0, keep, n_entity, counts, dst, out, n_out, stride, tag, 0)

    assert call(counts=p(vec), dst=p(wide), out=p(big), n_out=32) == -1 and "exactly one pass" in last_error(lib)
    assert call() == -1 and "exactly one pass" in last_error(lib)
    assert call(dst=p(wide), out=p(big), n_out=16, stride=3, tag=p(vec)) == -1 and "out_stride 3" in last_error(lib)
    assert call(dst=p(wide), out=p(big), n_out=16, stride=0) == -1
    assert call(dst=p(wide), out=p(big), n_out=16, stride=2) == -1  # pairs without the tags
    assert call(dst=p(wide)) == -1 and call(out=p(big), n_out=16) == -1  # half a fill pass
    assert call(counts=p(vec), side=p(bytes_)) == -1 and "both sides" in last_error(lib)
    assert call(counts=p(vec), keep=p(bytes_), n_entity=0) == -1 and "keep_entity" in last_error(lib)
    assert call(counts=p(vec), keep=p(bytes_), n_entity=-3) == -1
    assert call(n_row=-1, counts=p(vec)) == -1
    assert lib.bess_known_completions(*([0] * 12), 0, N_REL, *([0] * 13)) == 0  # n_row == 0: every pointer NULL
    assert call(n_row=0, counts=p(vec), dst=p(wide), out=p(big), stride=3) == 0  # (checked before anything else)


def test_completions_needs_the_index_on_a_device(host40):
    flt, _ = host40
    with pytest.raises(RuntimeError, match="to\\(device\\)"):
        flt.completions(torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 0)


# --------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda", 0)


def put(x, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return t.to(device=dev, dtype=dtype or t.dtype).contiguous()


P_ENT, P_REL = 6000, 3
PLANTED = (0, 1, 63, 64, 65, 5000)  # list lengths: none, one lane, a chunk less / exactly / plus one, a hub


def planted_triples():
    """Entity 10 + j has PLANTED[j] tails under relation 0 (the hub: 5000 of the 6000 entities); read from the
    other side every tail has a short list of heads among 10 .. 15.  Some rows twice: the index de-duplicates."""
    rng = np.random.default_rng(6000)
    parts = []
    for j, length in enumerate(PLANTED):
        tails = rng.choice(P_ENT, size=length, replace=False)
        parts.append(np.stack([np.full(length, 10 + j), np.zeros(length, dtype=np.int64), tails], axis=1))
    parts.append(parts[-1][:700])
    parts.append(np.stack([rng.integers(P_ENT, size=300), np.full(300, 2), rng.integers(P_ENT, size=300)], axis=1))
    return np.concatenate(parts).astype(np.int64)


@pytest.fixture(scope="module")
def planted(dev):
    triples = planted_triples()
    flt = KnownTripleFilter([triples], P_ENT, P_REL, device=dev)
    known = as_set(triples)
    by_len = [len(x) for x in brute_lists(known, 10 + np.arange(len(PLANTED)), np.zeros(len(PLANTED)), 0)]
    assert tuple(by_len) == PLANTED
    return flt, known


def planted_rows(known, n_row, variant):
    """Rows over the planted pairs - the hub first, every length in turn, from row 12 on also (tail, relation)
    rows of the other side and rows that name no pair - with the per-call filters of `variant`."""
    rng = np.random.default_rng(n_row)
    j = (5 - np.arange(n_row)) % len(PLANTED)
    kept, rel, side = (10 + j).astype(np.int32), np.zeros(n_row, dtype=np.int32), np.zeros(n_row, dtype=np.uint8)
    for i in range(12, n_row):
        if i % 5 == 2:  # the heads of a tail
            kept[i], side[i] = rng.integers(P_ENT), 1
        elif i % 5 == 3:
            kept[i], rel[i] = ((-1, 0), (P_ENT, 0), (15, P_REL), (15, -1), (15, 1))[(i // 5) % 5]
    full = brute_lists(known, kept, rel, side)
    skip = keep = None
    if variant == "skip":
        # rows of one length come 6 apart: in turn their first, last and 64th entry, a non-member, none
        skip = np.full(n_row, -1, dtype=np.int32)
        for i, row in enumerate(full):
            kind = (i // len(PLANTED)) % 5 if n_row > 1 else 2
            if row and kind < 3:
                skip[i] = row[(0, len(row) - 1, min(63, len(row) - 1))[kind]]
            elif kind == 3:
                members = set(row)
                skip[i] = next(e for e in range(P_ENT) if e not in members)
    elif variant == "keep":
        keep = rng.random(P_ENT) < 0.7
        hub = brute_lists(known, [15], [0], 0)[0]
        keep[hub[64:192]] = False  # the hub's second and third chunk pass nothing
        keep[hub[4992:]] = False   # nor does its tail chunk
        keep[brute_lists(known, [12], [0], 0)[0]] = False  # a whole list
    return kept, rel, side, skip, keep


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["plain", "skip", "keep"])
@pytest.mark.parametrize("out_stride", [1, 2])
@pytest.mark.parametrize("n_row", [1, 5, 130])
def test_kernel_passes_on_the_planted_lists(dev, planted, n_row, out_stride, variant):
    """Count pass and fill pass against the set: lists of 0 / 1 / 63 / 64 / 65 / 5000 entries, both sides in one
    call, `dst` with gaps whose cells (and the tail of `out`) keep what they held."""
    from besskge import _native as nat

    flt, known = planted
    kept, rel, side, skip, keep = planted_rows(known, n_row, variant)
    want = brute_lists(known, kept, rel, side, skip, keep)
    want_counts = np.array([len(x) for x in want], dtype=np.int32)
    assert want_counts.max() > 3000 and (n_row < 130 or (want_counts == 0).any())
    if variant != "plain":
        plain = np.array([len(x) for x in brute_lists(known, kept, rel, side)])
        assert (want_counts < plain).any()  # the filter of this case bites
    mixed = bool(side.any())
    first = flt.index[SIDE_TAIL]
    query = dict(index2=flt.index[SIDE_HEAD] if mixed else None, side=put(side, dev) if mixed else None,
                 skip=None if skip is None else put(skip, dev),
                 keep_entity=None if keep is None else put(keep.astype(np.uint8), dev))
    counts = torch.full((n_row,), -3, dtype=torch.int32, device=dev)
    nat.known_completions(first, put(kept, dev), put(rel, dev), P_REL, counts=counts, **query)
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    gap = np.arange(n_row) % 3
    dst = np.cumsum(want_counts + gap) - want_counts  # row i starts after gap[i] untouched entries
    n_out = int(dst[-1] + want_counts[-1]) + 5
    tag = (1000 + np.arange(n_row)).astype(np.int32)
    want_out = np.full((n_out, out_stride), -7, dtype=np.int32)
    for i, row in enumerate(want):
        want_out[dst[i]: dst[i] + len(row), -1] = row
        if out_stride == 2:
            want_out[dst[i]: dst[i] + len(row), 0] = tag[i]
    out = torch.full((n_out, out_stride), -7, dtype=torch.int32, device=dev)
    nat.known_completions(first, put(kept, dev), put(rel, dev), P_REL, dst=put(dst.astype(np.int64), dev), out=out,
                          out_stride=out_stride, tag=put(tag, dev) if out_stride == 2 else None, **query)
    got = out.cpu().numpy()
    bad = np.argwhere(got != want_out)
    assert bad.shape[0] == 0, f"{bad.shape[0]} wrong of {want_out.size}, first at {bad[:5].tolist()}"


@pytest.mark.gpu
def test_fill_pass_drops_what_does_not_fit(dev, planted):
    """An `out` shorter than the lists: the entries past it are dropped, those inside it are written."""
    from besskge import _native as nat

    flt, known = planted
    kept, rel = put(np.array([14, 15], dtype=np.int32), dev), put(np.zeros(2, dtype=np.int32), dev)
    other, hub = brute_lists(known, [14, 15], [0, 0], 0)
    out = torch.full((4100,), -7, dtype=torch.int32, device=dev)
    # the 65 entries start 5 before `out` does, the hub's 5000 at entry 60 of 4000
    nat.known_completions(flt.index[SIDE_TAIL], kept, rel, P_REL, dst=put(np.array([-5, 60], dtype=np.int64), dev),
                          out=out[:4000])
    got = out.cpu().numpy()
    assert list(got[:60]) == other[5:] and list(got[60:4000]) == hub[:3940]
    assert (got[4000:] == -7).all()


@pytest.mark.gpu
@pytest.mark.parametrize("side", [0, 1, "mixed"])
def test_completions_on_the_device_equal_the_set(dev, side):
    """`KnownTripleFilter.completions` (count, cumsum, fill) over the 40-entity graph, the entity that stays given
    as local rows of a 3-shard sharding, with a skipped entity and a subset; an empty result; no rows."""
    triples = graph40()
    known = as_set(triples)
    flt = KnownTripleFilter([triples], N_ENT, N_REL, device=dev)
    sharding = Sharding.create(N_ENT, 3, seed=5)
    table = put(sharding.shard_and_idx_to_entity, dev, torch.int32)
    rng = np.random.default_rng(21 + (7 if side == "mixed" else side))
    n = 130
    glob, rel = rng.integers(N_ENT, size=n), rng.integers(N_REL, size=n).astype(np.int32)
    sd = rng.integers(2, size=n).astype(np.uint8) if side == "mixed" else np.full(n, side, dtype=np.uint8)
    shard = sharding.entity_to_shard[glob].astype(np.int32)
    kept = sharding.entity_to_idx[glob].astype(np.int32)
    shard[::5], kept[::5] = -1, glob[::5]  # (global ids among them)
    kept[7], shard[7] = table.shape[1], 0  # a row past the table
    glob[7] = -1
    skip = rng.integers(N_ENT, size=n).astype(np.int32)
    keep = rng.random(N_ENT) < 0.6
    side_arg = put(sd, dev) if side == "mixed" else side
    for sk, kp in ((None, None), (skip, None), (skip, keep)):
        ptr, ids = flt.completions(put(kept, dev), put(rel, dev), side_arg, skip=None if sk is None else put(sk, dev),
                                   keep_entity=None if kp is None else put(kp, dev), kept_shard=put(shard, dev),
                                   local_to_global=table)
        want_ptr, want_ids = flat(brute_lists(known, glob, rel, sd, sk, kp))
        assert ptr.dtype == torch.int64 and ids.dtype == torch.int32 and ptr.device == ids.device == dev
        assert np.array_equal(ptr.cpu().numpy(), want_ptr) and np.array_equal(ids.cpu().numpy(), want_ids)
        assert want_ptr[-1] > 100
        host = flt.completions_host(kept, rel, sd, skip=sk, keep_entity=kp, kept_shard=shard,
                                    local_to_global=sharding.shard_and_idx_to_entity)
        assert np.array_equal(host[0], want_ptr) and np.array_equal(host[1], want_ids)
    nobody = put(np.full(3, -1, dtype=np.int32), dev)
    ptr, ids = flt.completions(nobody, put(np.zeros(3, dtype=np.int32), dev), side_arg if side != "mixed" else 0)
    assert ptr.tolist() == [0, 0, 0, 0] and ids.numel() == 0
    ptr, ids = flt.completions(nobody[:0], nobody[:0], 0)
    assert ptr.tolist() == [0] and ids.numel() == 0
