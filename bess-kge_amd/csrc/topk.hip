// K11 on gfx950: streaming top-k of score rows (TopKQueryBessKGE, next-1).
//
// Replaces `torch.topk(torch.concat([window_scores, running_best]))` +
// `gather_indices` of the reference's sliding-window loop (bess.py:771-822) and
// the final `torch.topk` over the shards' lists (bess.py:889-894).
//
// One workgroup (four wavefronts) per query row.  A wave's list (kk <= 64 entries, sorted by
// descending score) lives in registers, entry j in lane j (65 .. 128 entries: two registers per lane).  The window is
// streamed 64 candidates at a time; a candidate enters only if it beats the
// current kk-th score tau (`__ballot(x > tau)`), so after the first few chunks
// almost every chunk costs one load, one compare and one ballot: the expected
// number of insertions over a stream of L random scores is ~kk * ln(L / kk).
// An insertion is O(1) wave operations: rank by ballot + popcount, shift by one
// lane (DPP-style __shfl_up), write the new entry.  Ties keep the earlier entry
// first (torch.topk leaves the order of equal scores unspecified); the _excl entry points order equal scores by
// ascending id instead and leave out a sparse set of (row, id) pairs (AllScoresBESS's filtered top-k).
#include "common.h"

namespace bess {

// Id of an empty list entry (and of a candidate that was taken out) under the total order: nothing sorts after
// (-inf, INT32_MAX), so it never enters a list.
constexpr int32_t ID_NONE = INT32_MAX;

// A row's running list, entry j in lane j (TWO: entry 64 + j in lane j of the second register pair).
// ORD = false: a candidate enters if its score beats the kk-th score; earlier entries win ties.
// ORD = true: the lists follow the total order (score descending, id ascending) - a candidate enters if its score
// is above the kk-th score, or equals it while its id is below the kk-th id, and is placed by the same rule: the
// result does not depend on the order in which candidates, tiles or shards' lists arrive.
template <bool TWO, bool ORD>
struct TopList {
    float bs = -INFINITY, bs1 = -INFINITY;  // (bs1, bi1): entries 64 .. 127 (TWO)
    int32_t bi = ORD ? ID_NONE : 0, bi1 = ORD ? ID_NONE : 0;
    float tau;      // the kk-th score
    int32_t tau_i;  // ... and its id (ORD)
    int kk, k0, lane;

    __device__ TopList(int kk_, int lane_) : kk(kk_), k0(TWO ? 64 : kk_), lane(lane_) {}
    __device__ void refresh() {
        tau = TWO ? __shfl(bs1, kk - 65, 64) : __shfl(bs, kk - 1, 64);
        if (ORD) tau_i = TWO ? __shfl(bi1, kk - 65, 64) : __shfl(bi, kk - 1, 64);
    }
    __device__ void load(const float* s, const int32_t* i) {
        if (lane < k0) {
            bs = s[lane];
            bi = i[lane];
        }
        if (TWO && 64 + lane < kk) {
            bs1 = s[64 + lane];
            bi1 = i[64 + lane];
        }
        refresh();
    }
    __device__ void store(float* s, int32_t* i) const {
        if (lane < k0) {
            s[lane] = bs;
            i[lane] = bi;
        }
        if (TWO && 64 + lane < kk) {
            s[64 + lane] = bs1;
            i[64 + lane] = bi1;
        }
    }
    __device__ bool enters(float x, int32_t xi) const {
        if (ORD) return x > tau || (x == tau && xi < tau_i);
        return x > tau;
    }
    // does entry (s, i) stay ahead of the newcomer (xv, iv)?
    __device__ static bool ahead(float s, int32_t i, float xv, int32_t iv) {
        if (ORD) return s > xv || (s == xv && i < iv);
        return s >= xv;  // earlier entries win ties
    }
    // candidate (xv, iv), wave-uniform, is known to enter.  O(1) wave operations: rank by ballot + popcount,
    // shift by one lane, write the new entry.
    __device__ void insert(float xv, int32_t iv) {
        const int pos0 = __popcll(__ballot(lane < k0 && ahead(bs, bi, xv, iv)));
        const float up_s = __shfl_up(bs, 1, 64);
        const int32_t up_i = __shfl_up(bi, 1, 64);
        if (TWO) {
            // the second half: shifted as a whole when the newcomer lands in the first (whose last entry
            // moves over), from the newcomer's place on when it lands here
            const int pos1 = __popcll(__ballot(64 + lane < kk && ahead(bs1, bi1, xv, iv)));
            const float last_s = __shfl(bs, 63, 64);
            const int32_t last_i = __shfl(bi, 63, 64);
            float up1_s = __shfl_up(bs1, 1, 64);
            int32_t up1_i = __shfl_up(bi1, 1, 64);
            if (lane == 0) {
                up1_s = last_s;
                up1_i = last_i;
            }
            if (64 + lane < kk) {
                if (pos0 < 64 || lane > pos1) {
                    bs1 = up1_s;
                    bi1 = up1_i;
                } else if (lane == pos1) {
                    bs1 = xv;
                    bi1 = iv;
                }
            }
        }
        if (lane < k0) {
            if (lane > pos0) {
                bs = up_s;
                bi = up_i;
            } else if (lane == pos0) {
                bs = xv;
                bi = iv;
            }
        }
        refresh();
    }
};

// A row's exclusion list (ORD kernels): ids[lo .. hi) ascending, in the id space of the candidates.  Only lanes
// whose candidate has passed the list's ballot look their id up (a binary search each), and a second ballot
// follows: a chunk that holds no such candidate costs one load, one compare and one ballot as before.
struct ExclRow {
    const int32_t* ids = nullptr;
    int32_t lo = 0, hi = 0;
    __device__ ExclRow() {}
    __device__ ExclRow(const int32_t* ptr, const int32_t* ids_, int64_t n_excl, int64_t row) {
        if (ptr) {
            ids = ids_;
            const int64_t a = ptr[row], b = ptr[row + 1];
            hi = static_cast<int32_t>(b < 0 ? 0 : (b > n_excl ? n_excl : b));
            lo = static_cast<int32_t>(a < 0 ? 0 : (a > hi ? hi : a));
        }
    }
    __device__ bool any() const { return hi > lo; }
    __device__ bool has(int32_t id) const {
        int32_t a = lo, b = hi;
        while (a < b) {
            const int32_t m = a + ((b - a) >> 1);
            if (ids[m] < id) a = m + 1;
            else b = m;
        }
        return a < hi && ids[a] == id;
    }
};

// a chunk of 64 candidates (one per lane), examined in lane order
template <bool TWO, bool ORD>
__device__ __forceinline__ void examine(TopList<TWO, ORD>& L, const ExclRow& ex, float x, int32_t xi, bool check) {
    unsigned long long m = __ballot(L.enters(x, xi));
    if (ORD && check && m && ex.any()) {  // wave-uniform
        if (((m >> L.lane) & 1ull) && ex.has(xi)) {
            x = -INFINITY;
            xi = ID_NONE;
        }
        m = __ballot(L.enters(x, xi));
    }
    while (m) {
        const int l = __ffsll(static_cast<long long>(m)) - 1;
        L.insert(__shfl(x, l, 64), __shfl(xi, l, 64));
        m &= ~(1ull << l);
        m &= __ballot(L.enters(x, xi));
    }
}

// WPR waves per query row (4 rows per workgroup, or 1 row whose four waves each stream a
// contiguous quarter of the columns - more bytes in flight when there are few rows, at the price
// of one list warm-up per wave).  With WPR = 4, wave 0 starts from the running list, waves 1-3 from
// empty lists; at the end wave 0 examines the other three lists as three more chunks, in wave
// order - quarters are in column order, so ties resolve exactly as in a single left-to-right pass.
// VEC: rows are 16-B aligned (ld % 4 == 0), a lane loads 4 consecutive columns with one instruction.
// TWO: lists of 65 .. 128 entries - entry j < 64 in lane j of the first register pair, entry 64 + j in lane j of
// the second; an insertion shifts the first into the second through lane 63 -> lane 0.
// ORD: total order, exclusion lists and fp16 rounding of the scores (bess_topk_update_excl).
template <int WPR, bool VEC, bool TWO, bool ORD>
__global__ __launch_bounds__(256) void k_topk_update(const float* __restrict__ scores, int64_t n_row,
                                                     int64_t n_col, int64_t ld, const int32_t* __restrict__ ids,
                                                     int64_t ids_rows, int32_t id_base,
                                                     const uint8_t* __restrict__ mask, int64_t mask_rows,
                                                     const int32_t* __restrict__ excl_ptr,
                                                     const int32_t* __restrict__ excl_ids, int64_t n_excl, int round16,
                                                     float* __restrict__ best_score,
                                                     int32_t* __restrict__ best_id, int kk) {
    __shared__ float l_s[3][TWO ? 128 : 64];
    __shared__ int32_t l_i[3][TWO ? 128 : 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int part = WPR == 4 ? wave : 0;  // which quarter of the columns
    const int64_t row = WPR == 4 ? static_cast<int64_t>(blockIdx.x) : blockIdx.x * 4ll + wave;
    if (row >= n_row) return;  // WPR == 1 only (whole waves; no barrier on that path)
    TopList<TWO, ORD> L(kk, lane);
    if (part == 0) L.load(best_score + row * kk, best_id + row * kk);
    else L.refresh();
    ExclRow ex;
    if (ORD) ex = ExclRow(excl_ptr, excl_ids, n_excl, row);
    const float* srow = scores + row * ld;
    const int32_t* irow = ids ? ids + (ids_rows == 1 ? 0 : row) * n_col : nullptr;
    const uint8_t* mrow = mask ? mask + (mask_rows == 1 ? 0 : row) * n_col : nullptr;
    // U groups are loaded back to back (U independent loads in flight per lane: the row is
    // streamed, not pointer-chased), then examined
    constexpr int U = VEC ? 4 : 8, PER = VEC ? 4 : 1, STEP = 64 * U * PER;
    const int64_t seg = WPR == 4 ? (n_col + 4 * STEP - 1) / (4 * STEP) * STEP : n_col;  // columns per wave
    const int64_t c_begin = part * seg, c_end = min(n_col, c_begin + seg);
    for (int64_t c0 = c_begin; c0 < c_end; c0 += STEP) {
        float xs[U][PER];
        int32_t xis[U][PER];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t j = c0 + 64 * PER * u + lane * PER;
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                xs[u][i] = -INFINITY;
                xis[u][i] = ORD ? ID_NONE : 0;
            }
            if constexpr (VEC) {
                if (j + 3 < c_end) {
                    VecLoad<float, 4>::load(srow + j, xs[u]);
                } else {  // the last, partial group of the row
#pragma unroll
                    for (int i = 0; i < PER; ++i)
                        if (j + i < c_end) xs[u][i] = srow[j + i];
                }
#pragma unroll
                for (int i = 0; i < PER; ++i) {
                    if (j + i < c_end) {
                        if (mrow && mrow[j + i] == 0) xs[u][i] += BESS_BAD_NEGATIVE_SCORE;
                        if (ORD) xs[u][i] = count_value(xs[u][i], round16);
                        xis[u][i] = irow ? irow[j + i] : id_base + static_cast<int32_t>(j + i);
                    }
                }
            } else if (j < c_end) {
                xs[u][0] = srow[j];
                if (mrow && mrow[j] == 0) xs[u][0] += BESS_BAD_NEGATIVE_SCORE;
                if (ORD) xs[u][0] = count_value(xs[u][0], round16);
                xis[u][0] = irow ? irow[j] : id_base + static_cast<int32_t>(j);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if constexpr (!VEC) {
                examine(L, ex, xs[u][0], xis[u][0], true);
            } else {
                // 256 candidates, column = 4 * lane + i: taken in column order (lowest lane first,
                // then lowest component), so that equal scores keep their left-to-right order
                auto some = [&]() {
                    return __ballot(L.enters(xs[u][0], xis[u][0]) || L.enters(xs[u][1], xis[u][1]) ||
                                    L.enters(xs[u][2], xis[u][2]) || L.enters(xs[u][3], xis[u][3]));
                };
                unsigned long long any = some();
                if (ORD && any && ex.any()) {  // wave-uniform: the lanes that passed look their candidates up
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if (L.enters(xs[u][i], xis[u][i]) && ex.has(xis[u][i])) {
                            xs[u][i] = -INFINITY;
                            xis[u][i] = ID_NONE;
                        }
                    }
                    any = some();
                }
                while (any) {
                    const int l = __ffsll(static_cast<long long>(any)) - 1;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float xv = __shfl(xs[u][i], l, 64);
                        const int32_t iv = __shfl(xis[u][i], l, 64);
                        if (L.enters(xv, iv)) L.insert(xv, iv);  // wave-uniform branch
                    }
                    any &= ~(1ull << l);
                    any &= some();
                }
            }
        }
    }
    if (WPR == 4) {
        if (wave > 0) {
            l_s[wave - 1][lane] = lane < L.k0 ? L.bs : -INFINITY;
            l_i[wave - 1][lane] = L.bi;
            if (TWO) {
                l_s[wave - 1][64 + lane] = 64 + lane < kk ? L.bs1 : -INFINITY;
                l_i[wave - 1][64 + lane] = L.bi1;
            }
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int w = 0; w < 3; ++w) {  // (entries of a list have passed their exclusion check already)
                examine(L, ex, l_s[w][lane], l_i[w][lane], false);
                if (TWO) examine(L, ex, l_s[w][64 + lane], l_i[w][64 + lane], false);
            }
        }
    }
    if (part == 0) L.store(best_score + row * kk, best_id + row * kk);
}

// The same update when the scoring kernel has pruned the tile against the rows' current k-th scores
// (bess_neg_score_shared_fwd_pruned): flags[row, b] != 0 marks the blocks of 64 columns that hold a score above
// the threshold the row had when the tile was scored - only those were written, only those are read.  One wave
// per row: a dword of flags per lane names 256 blocks (16,384 columns) per step, the flagged ones are fetched
// four at a time (four independent loads in flight) and examined in column order, so equal scores keep their
// left-to-right order exactly as in the dense pass.  After the first tiles of a long row almost nothing is
// flagged: the pass costs the flag bytes (1/256 of the scores).
// ORD (bess_topk_update_flagged_excl): as in k_topk_update; candidate ids may come from one shared row `ids`.
template <bool TWO, bool ORD>
__global__ __launch_bounds__(256) void k_topk_update_flagged(const float* __restrict__ scores, int64_t n_row,
                                                             int64_t n_col, int64_t ld,
                                                             const uint32_t* __restrict__ flags, int64_t ldf32,
                                                             const int32_t* __restrict__ ids, int32_t id_base,
                                                             const int32_t* __restrict__ excl_ptr,
                                                             const int32_t* __restrict__ excl_ids, int64_t n_excl,
                                                             int round16, float* __restrict__ best_score,
                                                             int32_t* __restrict__ best_id, int kk) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = blockIdx.x * 4ll + wave;
    if (row >= n_row) return;
    TopList<TWO, ORD> L(kk, lane);
    L.load(best_score + row * kk, best_id + row * kk);
    ExclRow ex;
    if (ORD) ex = ExclRow(excl_ptr, excl_ids, n_excl, row);
    const float* srow = scores + row * ld;
    const int64_t n_block = (n_col + 63) / 64;
    const int64_t n_word = (n_block + 3) / 4;
    const uint32_t* frow = flags + row * ldf32;
    for (int64_t w0 = 0; w0 < n_word; w0 += 64) {
        const uint32_t f = w0 + lane < n_word ? frow[w0 + lane] : 0u;
        unsigned long long m = __ballot(f != 0u);
        // flagged blocks of this step, four at a time: (lane of the word, byte in it) in column order
        int64_t blk[4];
        int n_blk = 0;
        auto flush = [&]() {
            float x[4];
            int32_t xi[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t j = blk[i < n_blk ? i : 0] * 64 + lane;
                const bool in = i < n_blk && j < n_col;
                x[i] = in ? srow[j] : -INFINITY;
                if (ORD) {
                    x[i] = count_value(x[i], round16);
                    xi[i] = in ? (ids ? ids[j] : id_base + static_cast<int32_t>(j)) : ID_NONE;
                } else {
                    xi[i] = id_base + static_cast<int32_t>(j);
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < n_blk) examine(L, ex, x[i], xi[i], true);
            n_blk = 0;
        };
        while (m) {
            const int l = __ffsll(static_cast<long long>(m)) - 1;
            m &= ~(1ull << l);
            const uint32_t fl = __shfl(f, l, 64);
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                if ((fl >> (8 * b)) & 0xffu) {  // wave-uniform
                    const int64_t block = (w0 + l) * 4 + b;
                    if (block < n_block) {
                        blk[n_blk++] = block;
                        if (n_blk == 4) flush();
                    }
                }
            }
        }
        if (n_blk) flush();
    }
    L.store(best_score + row * kk, best_id + row * kk);
}

}  // namespace bess

using namespace bess;

// what both update calls ask of their sizes, list length and exclusion lists
static int topk_check_sizes(const char* what, int64_t n_row, int64_t n_col, int64_t ld, int32_t kk, const int32_t* excl_ptr,
                            const int32_t* excl_ids, int64_t n_excl) {
    BESS_REQUIRE(n_row >= 0 && n_row < (1ll << 31) && n_col >= 0 && ld >= n_col, "%s: bad sizes", what);
    BESS_REQUIRE(kk >= 1 && kk <= 128, "%s: list length %d not in [1, 128]", what, kk);
    BESS_REQUIRE(!excl_ptr == !excl_ids && n_excl >= 0 && n_excl < (1ll << 31),
                 "%s: excl_ptr and excl_ids go together (fewer than 2^31 entries)", what);
    return BESS_OK;
}

static int topk_update_flagged(bool ord, const char* what, const float* scores, int64_t n_row, int64_t n_col, int64_t ld,
                               const uint8_t* flags, int64_t ld_flags, const int32_t* ids, int32_t id_base,
                               const int32_t* excl_ptr, const int32_t* excl_ids, int64_t n_excl, int32_t round_f16,
                               float* best_score, int32_t* best_id, int32_t kk, void* stream) {
    if (int e = topk_check_sizes(what, n_row, n_col, ld, kk, excl_ptr, excl_ids, n_excl)) return e;
    if (n_row == 0 || n_col == 0) return BESS_OK;
    BESS_REQUIRE(scores && flags && best_score && best_id, "%s: NULL pointer", what);
    BESS_REQUIRE(ld_flags % 4 == 0 && ld_flags >= (n_col + 63) / 64 && reinterpret_cast<uintptr_t>(flags) % 4 == 0,
                 "%s: flag rows must be 4-byte aligned and hold one byte per 64 columns", what);
    const unsigned grid = static_cast<unsigned>(ceil_div(n_row, 4));
    const uint32_t* f32 = reinterpret_cast<const uint32_t*>(flags);
    hipStream_t st = as_stream(stream);
    with_flag(kk > 64, [&](auto two) {
        with_flag(ord, [&](auto o) {
            k_topk_update_flagged<decltype(two)::value, decltype(o)::value><<<grid, 256, 0, st>>>(
                scores, n_row, n_col, ld, f32, ld_flags / 4, ids, id_base, excl_ptr, excl_ids, n_excl, round_f16, best_score,
                best_id, kk);
        });
    });
    return check_launch(what);
}

extern "C" int bess_topk_update_flagged(const float* scores, int64_t n_row, int64_t n_col, int64_t ld,
                                        const uint8_t* flags, int64_t ld_flags, int32_t id_base, float* best_score,
                                        int32_t* best_id, int32_t kk, void* stream) {
    return topk_update_flagged(false, "topk_update_flagged", scores, n_row, n_col, ld, flags, ld_flags, nullptr, id_base,
                               nullptr, nullptr, 0, 0, best_score, best_id, kk, stream);
}

extern "C" int bess_topk_update_flagged_excl(const float* scores, int64_t n_row, int64_t n_col, int64_t ld,
                                             const uint8_t* flags, int64_t ld_flags, const int32_t* ids,
                                             int32_t id_base, const int32_t* excl_ptr, const int32_t* excl_ids,
                                             int64_t n_excl, int32_t round_f16, float* best_score, int32_t* best_id,
                                             int32_t kk, void* stream) {
    return topk_update_flagged(true, "topk_update_flagged_excl", scores, n_row, n_col, ld, flags, ld_flags, ids, id_base,
                               excl_ptr, excl_ids, n_excl, round_f16, best_score, best_id, kk, stream);
}

static int topk_update(bool ord, const char* what, const float* scores, int64_t n_row, int64_t n_col, int64_t ld,
                       const int32_t* ids, int64_t ids_rows, int32_t id_base, const uint8_t* mask, int64_t mask_rows,
                       const int32_t* excl_ptr, const int32_t* excl_ids, int64_t n_excl, int32_t round_f16,
                       float* best_score, int32_t* best_id, int32_t kk, void* stream) {
    if (int e = topk_check_sizes(what, n_row, n_col, ld, kk, excl_ptr, excl_ids, n_excl)) return e;
    if (n_row == 0 || n_col == 0) return BESS_OK;
    BESS_REQUIRE(scores && best_score && best_id, "%s: NULL pointer", what);
    BESS_REQUIRE(!ids || ids_rows == 1 || ids_rows == n_row, "%s: ids_rows must be 1 or n_row", what);
    BESS_REQUIRE(!mask || mask_rows == 1 || mask_rows == n_row, "%s: mask_rows must be 1 or n_row", what);
    // few rows: four waves per row keep enough loads in flight; many rows: one wave per row
    // (measured crossover on 256 CUs, profiles/bench_topk.py)
    const bool wide = n_row <= 6144;
    const bool vec = ld % 4 == 0 && reinterpret_cast<uintptr_t>(scores) % 16 == 0;
    const unsigned grid = static_cast<unsigned>(wide ? n_row : ceil_div(n_row, 4));
    hipStream_t st = as_stream(stream);
    with_constant<4, 1>(wide ? 4 : 1, [&](auto wpr) {
        with_flag(vec, [&](auto v) {
            with_flag(kk > 64, [&](auto two) {
                with_flag(ord, [&](auto o) {
                    k_topk_update<decltype(wpr)::value, decltype(v)::value, decltype(two)::value, decltype(o)::value>
                        <<<grid, 256, 0, st>>>(scores, n_row, n_col, ld, ids, ids_rows, id_base, mask, mask_rows, excl_ptr,
                                               excl_ids, n_excl, round_f16, best_score, best_id, kk);
                });
            });
        });
    });
    return check_launch(what);
}

extern "C" int bess_topk_update(const float* scores, int64_t n_row, int64_t n_col, int64_t ld,
                                const int32_t* ids, int64_t ids_rows, int32_t id_base, const uint8_t* mask,
                                int64_t mask_rows, float* best_score, int32_t* best_id, int32_t kk,
                                void* stream) {
    return topk_update(false, "topk_update", scores, n_row, n_col, ld, ids, ids_rows, id_base, mask, mask_rows, nullptr,
                       nullptr, 0, 0, best_score, best_id, kk, stream);
}

extern "C" int bess_topk_update_excl(const float* scores, int64_t n_row, int64_t n_col, int64_t ld,
                                     const int32_t* ids, int64_t ids_rows, int32_t id_base, const uint8_t* mask,
                                     int64_t mask_rows, const int32_t* excl_ptr, const int32_t* excl_ids,
                                     int64_t n_excl, int32_t round_f16, float* best_score, int32_t* best_id,
                                     int32_t kk, void* stream) {
    return topk_update(true, "topk_update_excl", scores, n_row, n_col, ld, ids, ids_rows, id_base, mask, mask_rows,
                       excl_ptr, excl_ids, n_excl, round_f16, best_score, best_id, kk, stream);
}
