// Filtered negative sampling: which of a step's sampled (query, candidate) pairs are known triples?
// Filtered evaluation: which entities complete a query to a known triple (k_known_completions, further down)?
//
// The index (besskge/negative_filter.py: KnownTripleFilter) is exact - one CSR structure per corruption side:
//   keys  int64 [n_pair]      sorted unique  kept * n_relation + relation  of the (kept entity, relation) pairs
//   off   int64 [n_pair + 1]  offsets into
//   comp  int32 [off[n_pair]] the sorted, de-duplicated completions of each pair (tails of (h, r) / heads of (t, r))
// A query row is (kept entity, relation, side); its candidates are a row of entity ids.  mask[i, j] = 0 iff
// (kept_i, relation_i, cand_ij) is in the index of row i's side.
//
// Work split: a wave owns one row at a time, its lanes stride the row's columns (coalesced candidate loads and
// mask stores).  Everything about the row - side, the translation of the kept entity, the 64-bit key and its
// ~log2(n_pair) step binary search over `keys` - is wave-uniform: the row index goes through readfirstlane, so the
// search runs once per row on scalar registers, not once per lane.  The common outcomes are "no such pair" (the
// row's mask is all ones, no completion is read) and a short list: up to 64 completions are loaded once, one per
// lane, and every lane compares its candidate against each of them (v_readlane with a uniform lane number).
// Longer lists - hub entities with thousands of completions - get a branch-free binary search per lane whose trip
// count is uniform (the list length is).  Candidates and kept entities may be shard-local rows: they are
// translated through the sharding's [n_shard, ld_map] table here, so no [rows, columns] tensor of global ids is
// ever made.  Ids outside the tables they index are never loaded through: such a pair is "not known".
#include "common.h"

namespace bess {

struct TripleIndex {
    const int64_t* keys;
    const int64_t* off;
    int64_t n_pair;
    const int32_t* comp;
};

struct KnownArgs {
    TripleIndex index[2];     // [side]; index[1] unused when side == NULL
    const int32_t* kept;      // [n_row]
    const int32_t* kept_shard;  // [n_row] or NULL; >= 0: kept is a local row of that shard
    const int32_t* relation;  // [n_row]
    const uint8_t* side;      // [n_row] or NULL (every row takes index[0])
    int64_t n_row, n_relation;
    const int32_t* cand;
    int64_t n_col, ld_cand, n_cand_row;
    const int32_t* cand_row;  // [n_row] or NULL
    int64_t cols_per_block, block_stride;
    int32_t cand_shard;       // >= 0: every column is a local row of that shard; < 0: of shard column / cols_per_block
    const int32_t* map;       // [n_map_shard, ld_map] or NULL
    int64_t ld_map, n_map_shard;
    uint8_t* mask;
    int64_t ld_mask;
    int32_t and_into;
};

constexpr int KNOWN_WAVES = 4;  // per workgroup

// The completion list [beg, beg + len) of row `row`'s (kept entity, relation) pair in the index of the row's side;
// len == 0 when there is no such pair or the row names none (kept < 0, a relation, shard or local row outside its
// table - nothing is loaded through such an id).  `row` is wave-uniform, so everything here is.  A: KnownArgs /
// CompletionArgs (the query description they share).
template <typename A>
__device__ __forceinline__ TripleIndex find_pair(const A& a, int64_t row, int64_t& beg, int64_t& len) {
    const int s = a.side ? (a.side[row] ? 1 : 0) : 0;
    const TripleIndex ix = a.index[s];
    int64_t kept = a.kept[row];
    bool valid = kept >= 0;
    if (a.map && a.kept_shard) {
        const int64_t sh = a.kept_shard[row];
        if (sh >= 0) {
            valid = valid && sh < a.n_map_shard && kept < a.ld_map;
            kept = valid ? static_cast<int64_t>(a.map[sh * a.ld_map + kept]) : 0;
        }
    }
    const int64_t rel = a.relation[row];
    valid = valid && rel >= 0 && rel < a.n_relation;
    const int64_t key = kept * a.n_relation + rel;
    int64_t lo = 0, hi = valid ? ix.n_pair : 0;
    while (lo < hi) {  // first pair with keys[pair] >= key
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (ix.keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    beg = 0, len = 0;
    if (valid && lo < ix.n_pair && ix.keys[lo] == key) {
        beg = ix.off[lo];
        len = ix.off[lo + 1] - beg;
    }
    return ix;
}

__global__ __launch_bounds__(64 * KNOWN_WAVES) void k_known_triple_mask(KnownArgs a) {
    const int lane = static_cast<int>(threadIdx.x) & 63;
    const int64_t wave0 = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x * KNOWN_WAVES + (threadIdx.x >> 6)));
    const int64_t n_wave = static_cast<int64_t>(gridDim.x) * KNOWN_WAVES;
    for (int64_t row = wave0; row < a.n_row; row += n_wave) {
        // ---- the row's pair: wave-uniform
        int64_t beg, len;
        const TripleIndex ix = find_pair(a, row, beg, len);
        const int64_t crow = a.cand_row ? static_cast<int64_t>(a.cand_row[row]) : row;
        const bool row_ok = a.ld_cand == 0 || (crow >= 0 && crow < a.n_cand_row);
        if (!row_ok) len = 0;  // (no such candidate row: nothing is read, nothing is known)
        const int32_t* __restrict__ crow_ptr = a.cand + (row_ok ? crow * a.ld_cand : 0);
        const int32_t* __restrict__ list = ix.comp + beg;
        uint8_t* __restrict__ mrow = a.mask + row * a.ld_mask;
        // a short list sits in the wave's registers, one completion per lane (-1 never equals a valid candidate)
        int32_t mine = -1;
        if (len > 0 && len <= 64 && lane < len) mine = list[lane];

        for (int64_t col0 = 0; col0 < a.n_col; col0 += 64) {
            const int64_t col = col0 + lane;
            const bool live = col < a.n_col && row_ok;
            bool known = false;
            if (len > 0) {
                const int64_t cc = col < a.n_col ? col : a.n_col - 1;  // (clamped: the load is unconditional)
                const int64_t blk = cc / a.cols_per_block;
                int32_t c = crow_ptr[blk * a.block_stride + (cc - blk * a.cols_per_block)];
                if (a.map) {
                    const int64_t sh = a.cand_shard >= 0 ? a.cand_shard : blk;
                    const bool ok = c >= 0 && c < a.ld_map && sh < a.n_map_shard;
                    const int32_t g = a.map[ok ? sh * a.ld_map + c : 0];
                    c = ok ? g : -2;
                }
                if (len <= 64) {
                    const int n = static_cast<int>(len);
                    for (int t = 0; t < n; ++t) known |= __builtin_amdgcn_readlane(mine, t) == c;
                } else {
                    // branch-free lower bound: the answer stays inside [base, base + n), n is uniform
                    int64_t base = 0, n = len;
                    while (n > 1) {
                        const int64_t half = n >> 1;
                        base = list[base + half - 1] < c ? base + half : base;
                        n -= half;
                    }
                    known = list[base] == c;
                }
            }
            if (live) {
                if (!a.and_into) mrow[col] = known ? 0 : 1;
                else if (known) mrow[col] = 0;  // (a byte that is 0 already stays 0, a 1 stays unless the triple is known)
            }
        }
    }
}

// Filtered evaluation asks the index the other question: not "is this candidate known?" but "list the known
// completions of this query" - one CSR row per query row, enumerated in two passes over the same rows.
struct CompletionArgs {
    TripleIndex index[2];       // [side]; index[1] unused when side == NULL
    const int32_t* kept;        // [n_row]
    const int32_t* kept_shard;  // [n_row] or NULL; >= 0: kept is a local row of that shard
    const int32_t* relation;    // [n_row]
    const uint8_t* side;        // [n_row] or NULL (every row takes index[0])
    int64_t n_row, n_relation;
    const int32_t* map;         // [n_map_shard, ld_map] or NULL
    int64_t ld_map, n_map_shard;
    const int32_t* skip;         // [n_row] or NULL: the entity left out of the row's list (-1: none)
    const uint8_t* keep_entity;  // [n_entity] or NULL: only entities with a non-zero byte pass
    int64_t n_entity;
    int32_t* counts;             // count pass: [n_row]
    const int64_t* dst;          // fill pass: [n_row] first entry of the row's list in `out`
    int32_t* out;                // [n_out, out_stride]
    int64_t n_out, out_stride;
    const int32_t* tag;          // [n_row] or NULL: with out_stride == 2, the first word of every entry of the row
};

// One wave per row, as above; its lanes stride the row's completion list in chunks of 64 (coalesced loads).  The
// trip count is wave-uniform (the list length is), so every ballot sees the whole wave.  Count: the population of
// the ballot of the passing lanes.  Fill: a passing lane's place is the running base plus its rank among the
// passing lanes of the chunk (mbcnt of the ballot) - the ascending order of the list survives without atomics or a
// sort, and a hub row of thousands of completions is a loop of chunks in one wave.
template <bool FILL>
__global__ __launch_bounds__(64 * KNOWN_WAVES) void k_known_completions(CompletionArgs a) {
    const int lane = static_cast<int>(threadIdx.x) & 63;
    const int64_t wave0 = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x * KNOWN_WAVES + (threadIdx.x >> 6)));
    const int64_t n_wave = static_cast<int64_t>(gridDim.x) * KNOWN_WAVES;
    for (int64_t row = wave0; row < a.n_row; row += n_wave) {
        int64_t beg, len;
        const TripleIndex ix = find_pair(a, row, beg, len);
        const int32_t* __restrict__ list = ix.comp + beg;
        const int32_t skip = a.skip ? a.skip[row] : -1;
        const int32_t tag = FILL && a.tag ? a.tag[row] : -1;
        int64_t base = FILL ? a.dst[row] : 0;  // entries of the row passed so far (+ where its list starts)
        for (int64_t c0 = 0; c0 < len; c0 += 64) {
            const int64_t c = c0 + lane;
            int32_t e = -1;
            bool pass = false;
            if (c < len) {
                e = list[c];
                pass = e != skip;
                if (a.keep_entity) pass = pass && e >= 0 && e < a.n_entity && a.keep_entity[e] != 0;
            }
            const uint64_t m = __ballot(pass);
            if (FILL) {
                const int64_t at = base + __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32),
                                                                    __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u));
                if (pass && at >= 0 && at < a.n_out) {  // (an entry outside `out` is dropped, never written)
                    if (a.out_stride == 2) a.out[at * 2] = tag;
                    a.out[at * a.out_stride + (a.out_stride - 1)] = e;
                }
            }
            base += __popcll(m);
        }
        if (!FILL && lane == 0) a.counts[row] = static_cast<int32_t>(base);
    }
}

static bool index_given(const int64_t* keys, const int64_t* off, int64_t n_pair, const int32_t* comp) {
    // (an index without pairs has no completions either: comp may be NULL then)
    return keys && off && n_pair >= 0 && (comp || n_pair == 0);
}

}  // namespace bess

using namespace bess;

extern "C" int bess_known_triple_mask(const int64_t* pair_keys, const int64_t* pair_off, int64_t n_pair,
                                      const int32_t* completions, const int64_t* pair_keys2,
                                      const int64_t* pair_off2, int64_t n_pair2, const int32_t* completions2,
                                      const int32_t* kept, const int32_t* kept_shard, const int32_t* relation,
                                      const uint8_t* side, int64_t n_row, int64_t n_relation, const int32_t* cand,
                                      int64_t n_col, int64_t ld_cand, int64_t n_cand_row, const int32_t* cand_row,
                                      int64_t cols_per_block, int64_t block_stride, int32_t cand_shard,
                                      const int32_t* local_to_global, int64_t ld_map, int64_t n_map_shard,
                                      uint8_t* mask, int64_t ld_mask, int32_t and_into, void* stream) {
    BESS_REQUIRE(n_row >= 0 && n_col >= 0 && n_relation > 0, "known_triple_mask: bad sizes (%lld rows, %lld columns, %lld relations)",
                 static_cast<long long>(n_row), static_cast<long long>(n_col), static_cast<long long>(n_relation));
    if (n_row == 0 || n_col == 0) return BESS_OK;
    BESS_REQUIRE(index_given(pair_keys, pair_off, n_pair, completions), "known_triple_mask: NULL index");
    BESS_REQUIRE(!side || index_given(pair_keys2, pair_off2, n_pair2, completions2),
                 "known_triple_mask: a `side` vector needs the index of both sides");
    BESS_REQUIRE(kept && relation && cand && mask, "known_triple_mask: NULL pointer");
    BESS_REQUIRE(ld_mask >= n_col, "known_triple_mask: ld_mask %lld < %lld columns", static_cast<long long>(ld_mask),
                 static_cast<long long>(n_col));
    if (cols_per_block <= 0) cols_per_block = n_col, block_stride = n_col;  // one block: a plain row
    BESS_REQUIRE(block_stride >= cols_per_block, "known_triple_mask: candidate blocks overlap");
    const int64_t n_block = ceil_div(n_col, cols_per_block);
    const int64_t row_span = (n_block - 1) * block_stride + (n_col - (n_block - 1) * cols_per_block);
    BESS_REQUIRE(ld_cand == 0 || (ld_cand > 0 && n_cand_row > 0 && (n_block > 1 || ld_cand >= row_span)),
                 "known_triple_mask: bad candidate layout (ld_cand %lld, %lld rows)", static_cast<long long>(ld_cand),
                 static_cast<long long>(n_cand_row));
    BESS_REQUIRE(cand_row || ld_cand == 0 || n_cand_row >= n_row, "known_triple_mask: %lld candidate rows for %lld rows",
                 static_cast<long long>(n_cand_row), static_cast<long long>(n_row));
    BESS_REQUIRE(!local_to_global || (ld_map > 0 && n_map_shard > 0 && (cand_shard >= 0 ? cand_shard < n_map_shard
                                                                                          : n_block <= n_map_shard)),
                 "known_triple_mask: the local-to-global table does not cover the candidates' shards");
    BESS_REQUIRE(local_to_global || !kept_shard, "known_triple_mask: kept_shard without a local-to-global table");
    KnownArgs a;
    a.index[0] = TripleIndex{pair_keys, pair_off, n_pair, completions};
    a.index[1] = side ? TripleIndex{pair_keys2, pair_off2, n_pair2, completions2} : a.index[0];
    a.kept = kept, a.kept_shard = kept_shard, a.relation = relation, a.side = side;
    a.n_row = n_row, a.n_relation = n_relation;
    a.cand = cand, a.n_col = n_col, a.ld_cand = ld_cand, a.n_cand_row = n_cand_row, a.cand_row = cand_row;
    a.cols_per_block = cols_per_block, a.block_stride = block_stride, a.cand_shard = cand_shard;
    a.map = local_to_global, a.ld_map = ld_map, a.n_map_shard = n_map_shard;
    a.mask = mask, a.ld_mask = ld_mask, a.and_into = and_into;
    const int64_t blocks = std::min<int64_t>(ceil_div(n_row, KNOWN_WAVES), 256 * 8);
    k_known_triple_mask<<<static_cast<unsigned>(blocks), 64 * KNOWN_WAVES, 0, as_stream(stream)>>>(a);
    return check_launch("known_triple_mask");
}

extern "C" int bess_known_completions(const int64_t* pair_keys, const int64_t* pair_off, int64_t n_pair,
                                      const int32_t* completions, const int64_t* pair_keys2,
                                      const int64_t* pair_off2, int64_t n_pair2, const int32_t* completions2,
                                      const int32_t* kept, const int32_t* kept_shard, const int32_t* relation,
                                      const uint8_t* side, int64_t n_row, int64_t n_relation,
                                      const int32_t* local_to_global, int64_t ld_map, int64_t n_map_shard,
                                      const int32_t* skip, const uint8_t* keep_entity, int64_t n_entity,
                                      int32_t* counts, const int64_t* dst, int32_t* out, int64_t n_out,
                                      int64_t out_stride, const int32_t* tag, void* stream) {
    BESS_REQUIRE(n_row >= 0 && n_relation > 0, "known_completions: bad sizes (%lld rows, %lld relations)",
                 static_cast<long long>(n_row), static_cast<long long>(n_relation));
    if (n_row == 0) return BESS_OK;
    const bool count_pass = counts != nullptr, fill_pass = dst != nullptr || out != nullptr;
    BESS_REQUIRE(count_pass != fill_pass, "known_completions: exactly one pass per call (`counts`, or `dst` and `out`)");
    BESS_REQUIRE(!fill_pass || (dst && out && n_out >= 0), "known_completions: the fill pass needs `dst`, `out` and n_out >= 0");
    BESS_REQUIRE(!fill_pass || out_stride == 1 || (out_stride == 2 && tag),
                 "known_completions: out_stride %lld (1, or 2 with a `tag` vector)", static_cast<long long>(out_stride));
    BESS_REQUIRE(index_given(pair_keys, pair_off, n_pair, completions), "known_completions: NULL index");
    BESS_REQUIRE(!side || index_given(pair_keys2, pair_off2, n_pair2, completions2),
                 "known_completions: a `side` vector needs the index of both sides");
    BESS_REQUIRE(kept && relation, "known_completions: NULL pointer");
    BESS_REQUIRE(!local_to_global || (ld_map > 0 && n_map_shard > 0), "known_completions: empty local-to-global table");
    BESS_REQUIRE(local_to_global || !kept_shard, "known_completions: kept_shard without a local-to-global table");
    BESS_REQUIRE(!keep_entity || n_entity > 0, "known_completions: `keep_entity` with n_entity = %lld",
                 static_cast<long long>(n_entity));
    CompletionArgs a;
    a.index[0] = TripleIndex{pair_keys, pair_off, n_pair, completions};
    a.index[1] = side ? TripleIndex{pair_keys2, pair_off2, n_pair2, completions2} : a.index[0];
    a.kept = kept, a.kept_shard = kept_shard, a.relation = relation, a.side = side;
    a.n_row = n_row, a.n_relation = n_relation;
    a.map = local_to_global, a.ld_map = ld_map, a.n_map_shard = n_map_shard;
    a.skip = skip, a.keep_entity = keep_entity, a.n_entity = n_entity;
    a.counts = counts, a.dst = dst, a.out = out, a.n_out = n_out, a.out_stride = out_stride, a.tag = tag;
    const unsigned blocks = static_cast<unsigned>(std::min<int64_t>(ceil_div(n_row, KNOWN_WAVES), 256 * 8));
    if (count_pass) k_known_completions<false><<<blocks, 64 * KNOWN_WAVES, 0, as_stream(stream)>>>(a);
    else k_known_completions<true><<<blocks, 64 * KNOWN_WAVES, 0, as_stream(stream)>>>(a);
    return check_launch("known_completions");
}
