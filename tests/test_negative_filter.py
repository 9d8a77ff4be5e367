"""Filtered negative sampling (besskge/negative_filter.py, csrc/known_triples.hip): the exact index of the known
triples, its numpy meaning (`mask_host`), the kernel and the mask `DeviceBatchSampler(..., filter_triples=...)` adds -
all checked bit for bit against a Python `set` of (head, relation, tail) tuples, never against each other."""

import ctypes

import numpy as np
import pytest
import torch

from besskge.batch_sampler import RandomShardedBatchSampler
from besskge.dataset import KGDataset
from besskge.negative_filter import SIDE_HEAD, SIDE_TAIL, KnownTripleFilter
from besskge.negative_sampler import (
    PlaceholderNegativeSampler,
    RandomShardedNegativeSampler,
    TripleBasedShardedNegativeSampler,
    TypeBasedShardedNegativeSampler,
)
from besskge.sharding import PartitionedTripleSet, Sharding

N_ENT, N_REL, N_TRIPLE = 40, 5, 600  # a random candidate is a known triple with probability 600 / 8000 = 7.5 %


# ---------------------------------------------------------------- the oracle
def graph40():
    """600 distinct random triples over 40 entities and 5 relations."""
    rng = np.random.default_rng(40)
    flat = rng.choice(N_ENT * N_REL * N_ENT, size=N_TRIPLE, replace=False)
    h, rest = np.divmod(flat, N_REL * N_ENT)
    r, t = np.divmod(rest, N_ENT)
    return np.stack([h, r, t], axis=1).astype(np.int64)


def as_set(*arrays):
    return {tuple(int(x) for x in row) for a in arrays for row in np.asarray(a)}


def brute(known, kept, relation, side, cand):
    """out[i, j] = False iff the triple with cand[i, j] in the replaced place is in the set."""
    kept, relation = np.asarray(kept).reshape(-1), np.asarray(relation).reshape(-1)
    side = np.broadcast_to(np.asarray(side), kept.shape)
    cand = np.asarray(cand)
    cand = np.broadcast_to(cand.reshape(-1, cand.shape[-1]), (kept.shape[0], cand.shape[-1]))
    out = np.ones(cand.shape, dtype=bool)
    for i in range(cand.shape[0]):
        for j in range(cand.shape[1]):
            k, r, c = int(kept[i]), int(relation[i]), int(cand[i, j])
            out[i, j] = ((c, r, k) if side[i] else (k, r, c)) not in known
    return out


RANDOM_SHAPES = [(n_row, n_col) for n_row in (1, 5, 130) for n_col in (1, 63, 64, 65, 259)]


def random_case(n_row, n_col, side):
    """Queries over the 40-entity graph; side: 0, 1 or "mixed"."""
    rng = np.random.default_rng(1000 * n_row + n_col + (7 if side == "mixed" else int(side)))
    kept = rng.integers(N_ENT, size=n_row).astype(np.int32)
    rel = rng.integers(N_REL, size=n_row).astype(np.int32)
    sd = rng.integers(2, size=n_row).astype(np.uint8) if side == "mixed" else np.full(n_row, side, dtype=np.uint8)
    cand = rng.integers(N_ENT, size=(n_row, n_col)).astype(np.int32)
    return kept, rel, sd, cand


def degenerate(n_row, n_col):
    """Too few cells to expect both mask values at 7.5 % known triples - or a single query, whose (entity, relation)
    pair may have no completion at all."""
    return n_row == 1 or n_row * n_col < 60


# --------------------------------------------------------------------- CPU
def test_index_build_against_a_set():
    a = np.array([[3, 1, 5], [3, 1, 2], [3, 1, 9], [3, 1, 2], [0, 0, 7], [6, 2, 3]])
    b = np.array([[3, 1, 9], [8, 1, 5], [3, 1, 0], [0, 0, 7]])  # repeats rows of `a`, adds two
    known = as_set(a, b)
    assert len(known) == 7
    flt = KnownTripleFilter([a, b], n_entity=10, n_relation_type=3)
    assert flt.n_triple == 7
    for side, (kept_col, comp_col) in ((SIDE_TAIL, (0, 2)), (SIDE_HEAD, (2, 0))):
        keys, off, comp = flt.index_host[side]
        assert keys.dtype == np.int64 and off.dtype == np.int64 and comp.dtype == np.int32
        want = {}
        for tr in known:
            want.setdefault(tr[kept_col] * 3 + tr[1], set()).add(tr[comp_col])
        assert list(keys) == sorted(want)  # sorted, unique
        assert off[0] == 0 and off[-1] == len(known) == comp.shape[0] and off.shape[0] == keys.shape[0] + 1
        assert np.all(np.diff(off) > 0)
        for k, lo, hi in zip(keys, off[:-1], off[1:]):
            assert list(comp[lo:hi]) == sorted(want[int(k)])  # sorted and de-duplicated
    # (3, 1) has many tails, (0, 0) one; tail 5 has heads {3, 8} under relation 1; (6, 2) exists on the tail side only
    keys_t, off_t, comp_t = flt.index_host[SIDE_TAIL]
    at = list(keys_t).index(3 * 3 + 1)
    assert list(comp_t[off_t[at]:off_t[at + 1]]) == [0, 2, 5, 9]
    at = list(keys_t).index(0)
    assert list(comp_t[off_t[at]:off_t[at + 1]]) == [7]
    keys_h = flt.index_host[SIDE_HEAD][0]
    assert 6 * 3 + 2 in keys_t and 6 * 3 + 2 not in keys_h and 3 * 3 + 2 in keys_h and 3 * 3 + 2 not in keys_t


@pytest.mark.parametrize("side", [0, 1, "mixed"])
def test_mask_host_against_brute_force(side):
    triples = graph40()
    known = as_set(triples)
    assert len(known) == N_TRIPLE
    flt = KnownTripleFilter([triples[:400], triples[300:]], N_ENT, N_REL)  # overlapping parts collapse
    assert flt.n_triple == N_TRIPLE
    kept, rel, sd, cand = random_case(50, 33, side)
    got = flt.mask_host(kept, rel, sd if side == "mixed" else side, cand)
    want = brute(known, kept, rel, sd, cand)
    assert got.dtype == np.bool_ and np.array_equal(got, want)
    assert 0.02 < 1 - want.mean() < 0.3
    # one shared candidate row, "h" / "t" spelling of the side
    if side != "mixed":
        got = flt.mask_host(kept, rel, "ht"[1 - side], cand[0])
        assert np.array_equal(got, brute(known, kept, rel, sd, cand[:1]))
    # ids outside their range are never known
    assert flt.mask_host([N_ENT, 3], [0, N_REL], 0, [[0, 1], [2, -1]]).all()


def test_random_cases_hold_both_values_on_the_oracle():
    """The seeds of the GPU cases: every non-degenerate mask has known and unknown pairs, and the share of known
    ones over all of them is near the expected 7.5 % - so a kernel that writes all ones cannot pass."""
    known = as_set(graph40())
    zeros = cells = 0
    for n_row, n_col in RANDOM_SHAPES:
        for side in (0, 1, "mixed"):
            kept, rel, sd, cand = random_case(n_row, n_col, side)
            want = brute(known, kept, rel, sd, cand)
            if not degenerate(n_row, n_col):
                assert want.any() and not want.all(), (n_row, n_col, side)
            zeros += int((~want).sum())
            cells += want.size
    assert 0.02 < zeros / cells < 0.30, zeros / cells


def test_filter_refusals():
    ok = np.array([[0, 0, 1]])
    with pytest.raises(ValueError, match="entity id outside"):
        KnownTripleFilter([ok, np.array([[0, 0, 10]])], n_entity=10, n_relation_type=2)
    with pytest.raises(ValueError, match="entity id outside"):
        KnownTripleFilter([np.array([[-1, 0, 1]])], n_entity=10, n_relation_type=2)
    with pytest.raises(ValueError, match="relation id outside"):
        KnownTripleFilter([np.array([[0, 2, 1]])], n_entity=10, n_relation_type=2)
    with pytest.raises(ValueError, match="64-bit key"):
        KnownTripleFilter([ok], n_entity=2 ** 31 - 1, n_relation_type=2 ** 33)
    KnownTripleFilter([ok], n_entity=2 ** 31 - 1, n_relation_type=2 ** 32)  # 2^63 - 2^32: fits


def _sampler(n_shard, scheme, flat=False, typed=False, placeholder=False, triple_based=False, bps=1, K=6):
    triples = graph40()
    ds = KGDataset(n_entity=N_ENT, n_relation_type=N_REL, triples={"train": triples},
                   original_triple_ids={"train": np.arange(triples.shape[0])})
    types = np.array([0, 8, 20]) if typed else None
    sharding = Sharding.create(N_ENT, n_shard, seed=5, type_offsets=types)
    pts = PartitionedTripleSet.create_from_dataset(ds, "train", sharding, partition_mode="ht_shardpair")
    if placeholder:
        ns = PlaceholderNegativeSampler(corruption_scheme=scheme, seed=3)
    elif triple_based:
        lists = np.random.default_rng(1).integers(N_ENT, size=(triples.shape[0], 4)).astype(np.int32)
        ns = TripleBasedShardedNegativeSampler(lists, lists, sharding, corruption_scheme=scheme, seed=3)
    elif typed:
        tt = np.random.default_rng(8).integers(len(types), size=(pts.triples.shape[0], 2)).astype(np.int32)
        ns = TypeBasedShardedNegativeSampler(triple_types=tt, n_negative=K, sharding=sharding, corruption_scheme=scheme,
                                             local_sampling=False, seed=3)
    else:
        ns = RandomShardedNegativeSampler(n_negative=K, sharding=sharding, seed=3, corruption_scheme=scheme,
                                          local_sampling=False, flat_negative_format=flat)
    bs = RandomShardedBatchSampler(partitioned_triple_set=pts, negative_sampler=ns, shard_bs=8 * n_shard,
                                   batches_per_step=bps, seed=11)
    assert bs.positive_per_partition == 8
    return bs, sharding, triples


def test_device_sampler_refuses_what_it_cannot_filter():
    """Construction only: the refusals come before any device work."""
    from besskge.device_sampler import DeviceBatchSampler

    cpu = torch.device("cpu")
    known = [graph40()]
    with pytest.raises(ValueError, match="PlaceholderNegativeSampler"):
        DeviceBatchSampler(_sampler(2, "t", placeholder=True)[0], cpu, filter_triples=known)
    with pytest.raises(ValueError, match="TripleBasedShardedNegativeSampler"):
        DeviceBatchSampler(_sampler(2, "t", triple_based=True)[0], cpu, filter_triples=known)
    with pytest.raises(ValueError, match="negative_sample_sharing"):
        DeviceBatchSampler(_sampler(2, "t")[0], cpu, filter_triples=known, negative_sample_sharing=True)


def test_entry_point_validates_before_it_launches():
    """No device needed: empty problems are fine with nothing else given, a NULL index is the usual error code."""
    from besskge import _native as nat

    lib = nat.load()

    def call(n_row, n_col):  # every pointer NULL
        return lib.bess_known_triple_mask(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, n_row, 5, 0, n_col, 0, 0, 0, 0, 0, -1, 0, 0, 0,
                                          0, n_col, 0, 0)

    assert call(0, 7) == 0 and call(7, 0) == 0
    assert call(3, 7) == -1
    buf = ctypes.create_string_buffer(256)
    lib.bess_last_error(buf, 256)
    assert "NULL index" in buf.value.decode()
    assert call(-1, 7) == -1


# --------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def flt40(dev):
    return KnownTripleFilter([graph40()], N_ENT, N_REL, device=dev), as_set(graph40())


def put(x, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return t.to(device=dev, dtype=dtype or t.dtype).contiguous()


def check(got, want, what=""):
    got = got.cpu().numpy().astype(bool)
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, f"{what}: {bad.shape[0]} wrong of {want.size}, first at {bad[:5].tolist()}"


@pytest.mark.gpu
@pytest.mark.parametrize("side", [0, 1, "mixed"])
@pytest.mark.parametrize("n_row, n_col", RANDOM_SHAPES)
def test_kernel_on_the_random_graph(dev, flt40, n_row, n_col, side):
    """Lane tails (1, 63, 64, 65 columns), more than one wave trip per row (259), 1 / 5 / 130 rows; leading
    dimensions larger than the column count, whose padding is left alone."""
    from besskge import _native as nat

    flt, known = flt40
    kept, rel, sd, cand = random_case(n_row, n_col, side)
    want = brute(known, kept, rel, sd, cand)
    if not degenerate(n_row, n_col):
        assert want.any() and not want.all()
    side_arg = put(sd, dev) if side == "mixed" else side
    got = flt.mask(put(kept, dev), put(rel, dev), side_arg, put(cand, dev))
    assert got.dtype == torch.bool and tuple(got.shape) == (n_row, n_col)
    check(got, want, "plain")
    # ld_cand = n_col + 3 (padding: ids that would be known or out of range), ld_mask = n_col + 5 prefilled with 7
    wide = np.full((n_row, n_col + 3), -5, dtype=np.int32)
    wide[:, :n_col] = cand
    mask = torch.full((n_row, n_col + 5), 7, dtype=torch.uint8, device=dev)
    first = flt.index[SIDE_TAIL] if side != 1 else flt.index[SIDE_HEAD]
    nat.known_triple_mask(first, put(kept, dev), put(rel, dev), put(wide, dev).reshape(-1), mask, N_REL,
                          index2=flt.index[SIDE_HEAD] if side == "mixed" else None,
                          side=put(sd, dev) if side == "mixed" else None, n_col=n_col, ld_cand=n_col + 3, n_cand_row=n_row)
    m = mask.cpu().numpy()
    assert np.all(m[:, n_col:] == 7)
    assert set(np.unique(m[:, :n_col])) <= {0, 1}
    check(mask[:, :n_col], want, "padded")


@pytest.mark.gpu
def test_kernel_share_of_known_triples_on_the_random_graph(dev, flt40):
    flt, _ = flt40
    zeros = cells = 0
    for n_row, n_col in RANDOM_SHAPES:
        for side in (0, 1, "mixed"):
            kept, rel, sd, cand = random_case(n_row, n_col, side)
            got = flt.mask(put(kept, dev), put(rel, dev), put(sd, dev) if side == "mixed" else side, put(cand, dev))
            zeros += int((~got).sum())
            cells += got.numel()
    assert 0.02 < zeros / cells < 0.30, zeros / cells


HUB_ENT, HUB_REL = 4000, 3
LIST_LENGTHS = {100: 1, 200: 63, 300: 64, 400: 65, 500: 1500}  # kept entity -> completions under relation 1


def hub_graph():
    """Completion lists of length 1, 63, 64, 65 and a hub of 1500 among 4000 entities: tails of (kept, 1) and, the
    same lists again, heads of (kept, 2).  Completions lie in [2, 3997], so on either side the keys of (0, 0) and
    (3999, 2) fall below the first and above the last pair key; (150, .) and (100, 0) are absent pairs inside."""
    rng = np.random.default_rng(12)
    rows = []
    for kept, n in LIST_LENGTHS.items():
        comp = np.sort(rng.choice(np.arange(2, HUB_ENT - 2), size=n, replace=False))
        rows += [(kept, 1, int(c)) for c in comp]
    tails = np.array(rows, dtype=np.int64)
    heads = tails[:, ::-1] + np.array([0, 1, 0])  # (c, 2, kept): the same lists for replaced heads, relation 2
    return tails, heads


def boundary_candidates(known, kept, rel, side, rng, n_col):
    """A row's candidates: first and last completion, the ids just below and above each, 0 and n_entity - 1, then
    random ids."""
    comp = sorted((t[0] if side else t[2]) for t in known if (t[2] if side else t[0]) == kept and t[1] == rel)
    forced = [0, HUB_ENT - 1]
    if comp:
        forced += [comp[0], comp[0] - 1, comp[0] + 1, comp[-1], comp[-1] - 1, comp[-1] + 1, comp[len(comp) // 2]]
    row = rng.integers(HUB_ENT, size=n_col)
    row[: len(forced)] = forced
    return row


@pytest.mark.gpu
@pytest.mark.parametrize("side", [0, 1, "mixed"])
def test_kernel_completion_lists_at_their_boundaries(dev, side):
    """Lists of 0 (pair absent: inside the key range, below the first and above the last key), 1, 63, 64, 65 (in
    registers) and 1500 completions (per-lane binary search), probed at both ends."""
    tails, heads = hub_graph()
    known = as_set(tails, heads)
    flt = KnownTripleFilter([tails, heads], HUB_ENT, HUB_REL, device=dev)
    for s in (SIDE_TAIL, SIDE_HEAD):
        keys, off, _ = flt.index_host[s]
        assert keys[0] > 0 and keys[-1] < (HUB_ENT - 1) * HUB_REL + HUB_REL - 1
        for k, n in LIST_LENGTHS.items():
            at = int(np.searchsorted(keys, k * HUB_REL + (2 if s else 1)))
            assert keys[at] == k * HUB_REL + (2 if s else 1) and off[at + 1] - off[at] == n
    rng = np.random.default_rng(3)
    n_col = 70
    queries = []  # (kept, relation, side)
    for s in ((0, 1) if side == "mixed" else (side,)):
        rel = 2 if s else 1
        queries += [(k, rel, s) for k in LIST_LENGTHS] + [(150, rel, s), (0, 0, s), (HUB_ENT - 1, HUB_REL - 1, s),
                                                           (100, 0, s)]
    kept = np.array([q[0] for q in queries], dtype=np.int32)
    rel = np.array([q[1] for q in queries], dtype=np.int32)
    sd = np.array([q[2] for q in queries], dtype=np.uint8)
    cand = np.stack([boundary_candidates(known, *q, rng, n_col) for q in queries]).astype(np.int32)
    want = brute(known, kept, rel, sd, cand)
    assert want.any() and not want.all()
    for i, q in enumerate(queries):  # every list is hit at its first, last and middle element and missed next to them
        if q[0] in LIST_LENGTHS and q[1] == (2 if q[2] else 1):
            assert not want[i, 2] and not want[i, 5] and not want[i, 8]
            assert LIST_LENGTHS[q[0]] > 1 or (want[i, 3] and want[i, 4])
        else:
            assert want[i].all()
    got = flt.mask(put(kept, dev), put(rel, dev), put(sd, dev) if side == "mixed" else side, put(cand, dev))
    check(got, want, "lists")
    assert np.array_equal(flt.mask_host(kept, rel, sd, cand), want)


@pytest.mark.gpu
@pytest.mark.parametrize("side", [0, 1])
def test_kernel_shared_candidate_rows(dev, flt40, side):
    flt, known = flt40
    kept, rel, sd, _ = random_case(130, 65, side)
    rows = np.random.default_rng(4).integers(N_ENT, size=(2, 65)).astype(np.int32)
    # one row for all (ld_cand == 0)
    got = flt.mask(put(kept, dev), put(rel, dev), side, put(rows[:1], dev))
    want = brute(known, kept, rel, sd, rows[:1])
    assert want.any() and not want.all()
    check(got, want, "one shared row")
    # two shared rows, picked per query
    pick = (np.arange(130) % 3 == 0).astype(np.int32)
    got = flt.mask(put(kept, dev), put(rel, dev), side, put(rows, dev), cand_row=put(pick, dev))
    check(got, brute(known, kept, rel, sd, rows[pick]), "cand_row")


@pytest.mark.gpu
@pytest.mark.parametrize("n_shard", [2, 3])
@pytest.mark.parametrize("side", [0, 1, "mixed"])
def test_kernel_translates_shard_local_ids(dev, flt40, n_shard, side):
    """Candidates (column j of shard j // cols_per_shard) and kept entities as local rows of shards of unequal
    size; the padding entries of the table (ids >= n_entity) are never reached by valid rows."""
    flt, known = flt40
    rng = np.random.default_rng(n_shard)
    cut = np.sort(rng.choice(np.arange(5, N_ENT - 5), size=n_shard - 1, replace=False))
    perm = rng.permutation(N_ENT)
    members = np.split(perm, cut)  # unequal shards
    counts = [len(m) for m in members]
    assert len(set(counts)) > 1
    ld = max(counts) + 2
    l2g = np.full((n_shard, ld), N_ENT + 1000, dtype=np.int32)  # padding: no entity
    for s, m in enumerate(members):
        l2g[s, : len(m)] = m
    n_row, per = 37, 21
    n_col = n_shard * per
    kept_shard = rng.integers(-1, n_shard, size=n_row).astype(np.int32)  # -1: the id is global already
    kept = np.array([rng.integers(N_ENT) if s < 0 else rng.integers(counts[s]) for s in kept_shard], dtype=np.int32)
    kept_global = np.array([k if s < 0 else l2g[s, k] for k, s in zip(kept, kept_shard)])
    rel = rng.integers(N_REL, size=n_row).astype(np.int32)
    sd = rng.integers(2, size=n_row).astype(np.uint8) if side == "mixed" else np.full(n_row, side, dtype=np.uint8)
    col_shard = np.arange(n_col) // per
    cand = np.stack([rng.integers(counts[s], size=n_row) for s in col_shard], axis=1).astype(np.int32)
    cand_global = l2g[col_shard[None, :], cand]
    assert cand_global.max() < N_ENT
    want = brute(known, kept_global, rel, sd, cand_global)
    assert want.any() and not want.all()
    got = flt.mask(put(kept, dev), put(rel, dev), put(sd, dev) if side == "mixed" else side, put(cand, dev),
                   local_to_global=put(l2g, dev), kept_shard=put(kept_shard, dev), cols_per_shard=per)
    check(got, want, "local ids")


@pytest.mark.gpu
def test_kernel_and_into_keeps_zeros(dev, flt40):
    flt, known = flt40
    kept, rel, sd, cand = random_case(130, 65, "mixed")
    want = brute(known, kept, rel, sd, cand)
    before = np.random.default_rng(9).random(want.shape) < 0.6
    mask = put(before, dev)
    out = flt.mask(put(kept, dev), put(rel, dev), put(sd, dev), put(cand, dev), out=mask, and_into=True)
    assert out is mask
    assert (before & ~want).any() and (~before & want).any()  # ones that are cleared, zeros that stay
    check(mask, before & want, "and_into")


@pytest.mark.gpu
def test_kernel_keys_beyond_32_bits(dev):
    """n_entity = 2^31 - 1, kept entity 2^31 - 2, 5 relations: the key (2^31 - 2) * 5 + 4 needs 34 bits.  The pair is
    found; its neighbours and the pair whose key equals it modulo 2^32 are other pairs."""
    big, n_ent = 2 ** 31 - 2, 2 ** 31 - 1
    assert big * 5 + 4 >= 2 ** 32
    alias, alias_rel = divmod((big * 5 + 4) % 2 ** 32, 5)  # the pair a key cut to 32 bits would be taken for
    triples = np.array([[big, 4, 7], [big, 4, big], [alias, alias_rel, 11], [3, 0, 2]], dtype=np.int64)
    known = as_set(triples)
    flt = KnownTripleFilter([triples], n_ent, 5, device=dev)
    kept = np.array([big, big, big - 1, alias, 3], dtype=np.int32)
    rel = np.array([4, 3, 4, alias_rel, 0], dtype=np.int32)
    cand = np.tile(np.array([7, 11, big, 2, 0, 8], dtype=np.int32), (5, 1))
    want = brute(known, kept, rel, 0, cand)
    assert list(want[0]) == [False, True, False, True, True, True] and want[1].all() and want[2].all()
    assert list(want[3]) == [True, False, True, True, True, True]
    check(flt.mask(put(kept, dev), put(rel, dev), 0, put(cand, dev)), want, "64-bit keys")
    assert np.array_equal(flt.mask_host(kept, rel, 0, cand), want)
    # and with the big entity as the replaced head
    want_h = brute(known, np.array([7, big], dtype=np.int32), [4, 4], 1, cand[:2])
    assert not want_h[0, 2] and not want_h[1, 2]
    check(flt.mask(put(np.array([7, big], dtype=np.int32), dev), put(rel[[0, 0]], dev), 1, put(cand[:2], dev)), want_h, "heads")


@pytest.mark.gpu
def test_kernel_empty_problems_write_nothing(dev, flt40):
    flt, _ = flt40
    mask = torch.full((4, 6), 7, dtype=torch.uint8, device=dev)
    kept, rel, _, _ = random_case(4, 1, 0)
    flt.mask(put(kept, dev), put(rel, dev), 0, torch.empty((4, 0), dtype=torch.int32, device=dev), out=mask)
    empty = torch.empty((0,), dtype=torch.int32, device=dev)
    flt.mask(empty, empty, 0, torch.empty((0, 6), dtype=torch.int32, device=dev), out=mask)
    assert bool((mask == 7).all())


# ------------------------------------------------------- sampler and step
def brute_batch_mask(batch, sharding, known, scheme, flat):
    """negative_mask [step, shard, S, shard, K] from the whole batch's own tensors and the sharding tables."""
    head, rel, tail, neg = (batch[k].cpu().numpy() for k in ("head", "relation", "tail", "negative"))
    l2g = sharding.shard_and_idx_to_entity
    n_step, n, _, per = head.shape
    K = neg.shape[-1]
    out = np.ones((n_step, n, n * per, n, K), dtype=bool)
    for s in range(n_step):
        for d in range(n):
            for j in range(n):
                for p in range(per):
                    h = int(l2g[d, head[s, d, j, p]])
                    t = int(l2g[j, tail[s, j, d, p]])
                    r = int(rel[s, d, j, p])
                    heads_replaced = scheme == "h" or (scheme == "ht" and p < per // 2)
                    b = j * per + p
                    row = (0 if heads_replaced or scheme != "ht" else 1) if flat else b
                    for src in range(n):
                        for k in range(K):
                            c = int(l2g[src, neg[s, src, d, row, k]])
                            out[s, d, b, src, k] = ((c, r, t) if heads_replaced else (h, r, c)) not in known
    return out


SAMPLER_CASES = [("random", "h", False), ("random", "t", False), ("random", "ht", False), ("random", "t", True),
                 ("typed", "ht", False)]


@pytest.mark.gpu
@pytest.mark.parametrize("n_shard", [1, 2])
@pytest.mark.parametrize("kind, scheme, flat", SAMPLER_CASES)
def test_device_sampler_adds_the_mask_and_changes_nothing_else(dev, n_shard, kind, scheme, flat):
    from besskge.device_sampler import DeviceBatchSampler

    def make(**kw):
        bs, sharding, triples = _sampler(n_shard, scheme, flat=flat, typed=kind == "typed", bps=2)
        return DeviceBatchSampler(bs, dev, **kw), sharding, triples

    plain, sharding, triples = make()
    known = as_set(triples)
    filtered, _, _ = make(filter_triples=[triples])
    for _ in range(2):  # (two calls: the streams advance the same way)
        want_batch, got = plain.sample(), filtered.sample()
        assert set(got) == set(want_batch) | {"negative_mask"}
        for k, v in want_batch.items():
            assert got[k].dtype == v.dtype and torch.equal(got[k], v), k
        mask = got["negative_mask"]
        K = want_batch["negative"].shape[-1]
        assert mask.dtype == torch.bool and tuple(mask.shape) == (2, n_shard, n_shard * 8, n_shard, K)
        want = brute_batch_mask(want_batch, sharding, known, scheme, flat)
        assert want.any() and not want.all()
        check(mask, want, "negative_mask")
    # a rank's slice: the mask rows of its own shard, everything else as without the filter
    last = [n_shard - 1]
    plain_r, _, _ = make(shards=last)
    filt_r, _, _ = make(shards=last, filter_triples=KnownTripleFilter([triples], N_ENT, N_REL))
    whole, _, _ = make()
    full = whole.sample()
    want_batch, got = plain_r.sample(), filt_r.sample()
    for k, v in want_batch.items():
        assert torch.equal(got[k], v), k
    want = brute_batch_mask(full, sharding, known, scheme, flat)[:, n_shard - 1:]
    check(got["negative_mask"], want, "own rows")


def _one_step(dev, scorer, n_shard, batch, mask):
    """One SGD step from fixed initial tables; `batch`: the sampler's tensors [1 step, shard, ...]."""
    from besskge import runtime
    from besskge.bess import EmbeddingMovingBessKGE
    from besskge.loss import LogSigmoidLoss
    from besskge.scoring import DistMult, TransE

    bs, sharding, _ = _sampler(n_shard, "t")
    gen = torch.Generator().manual_seed(21)
    ent = 0.5 * torch.randn(n_shard, sharding.max_entity_per_shard, 16, generator=gen)
    rel = 0.5 * torch.randn(N_REL, 16, generator=gen)
    if scorer == "TransE":
        fn = TransE(False, 1, sharding, N_REL, 16, ent.clone(), rel.clone())
    else:
        fn = DistMult(False, sharding, N_REL, 16, ent.clone(), rel.clone())
    model = EmbeddingMovingBessKGE(bs.negative_sampler, fn, LogSigmoidLoss(3.0, True, 0.5), return_scores=True)
    runner = runtime.training_model(model, runtime.Options(device_iterations=1), runtime.SGD(lr=0.1), device=dev)
    inputs = {k: batch[k][0] for k in ("head", "relation", "tail", "negative")}
    if mask is not None:
        inputs["negative_mask"] = mask[0]
    res = runner(**inputs)
    torch.cuda.synchronize()
    return (res["loss"].detach().cpu().clone(), res["negative_score"].detach().float().cpu().clone(),
            fn.entity_embedding.detach().cpu().clone(), fn.relation_embedding.detach().cpu().clone())


@pytest.mark.gpu
@pytest.mark.parametrize("scorer, n_shard", [("TransE", 2), ("DistMult", 1)])
def test_training_step_with_the_sampled_mask(dev, scorer, n_shard):
    """A: the filtered sampler's mask; B: the same mask made by brute force on the host; C: no filter.  The masks are
    equal bit for bit, A and B take the same code path, and so their loss and scores are equal bit for bit.  The
    updated tables are not compared that way: plain SGD adds the gradient rows into the tables (and the relation
    gradient into its buffer) with fp32 atomics, whose order is not fixed - the step does not reproduce its own tables
    (measured on an MI355X: B against a second B differs in 126 of 640 entity-table elements by up to 1.8e-7, A
    against B in 168 by up to 1.2e-7; one shard: 12 of 640 by 6e-8).  They are held to the bound of a reordered fp32
    sum instead: (m - 1) * 2^-24 * sum |addends| with m <= S * (2 + n_shard * K) contributions to a row, each addend
    below max |table| + 1 - four orders of magnitude below what a masked negative moves (lr * gradient ~ 1e-2).
    For TransE, A differs from C exactly at the masked scores.  DistMult on one shard takes the fused masked forward
    (A against B only)."""
    from besskge import _native as nat
    from besskge.device_sampler import DeviceBatchSampler

    bs, sharding, triples = _sampler(n_shard, "t")
    batch = DeviceBatchSampler(bs, dev, filter_triples=[triples]).sample()
    host_mask = brute_batch_mask(batch, sharding, as_set(triples), "t", False)
    assert host_mask.any() and not host_mask.all()
    check(batch["negative_mask"], host_mask, "the sampler's mask")
    a = _one_step(dev, scorer, n_shard, batch, batch["negative_mask"])
    b = _one_step(dev, scorer, n_shard, batch, torch.from_numpy(host_mask))
    assert torch.equal(a[0], b[0]), "loss"
    assert torch.equal(a[1], b[1]), "negative_score"
    S, K = 8 * n_shard, int(batch["negative"].shape[-1])
    for x, y, what in zip(a[2:], b[2:], ("entity table", "relation table")):
        bound = (S * (2 + n_shard * K) - 1) * 2.0 ** -24 * (float(y.abs().max()) + 1.0)
        assert float((x - y).abs().max()) <= bound, (what, float((x - y).abs().max()), bound)
    if scorer != "TransE":
        return
    c = _one_step(dev, scorer, n_shard, batch, None)
    assert not torch.equal(a[0], c[0])
    keep = torch.from_numpy(host_mask[0]).reshape(a[1].shape)
    assert torch.equal(a[1][keep], c[1][keep])
    assert torch.equal(a[1][~keep], c[1][~keep] + torch.tensor(nat.BAD_NEGATIVE_SCORE, dtype=torch.float32))
