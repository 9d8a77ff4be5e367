// Relation prediction (Chen et al. 2021): the softmax of every triple's relation against ALL relations, for the two
// scorers that are linear in the relation row (exact fp32, v_mfma_f32_32x32x2_f32):
//
//     s[i, r]   = <rel[r], g(h_i, t_i)>      DistMult g = h * t;  ComplEx g = [h1 t1 + h2 t2 | h1 t2 - h2 t1]
//     lse[i]    = log sum_{r < n_rel} exp(s[i, r])
//     P[i, r]   = coef[i] * (exp(s[i, r] - lse[i]) - [r == rel_idx[i]])
//     d_g[i]    = sum_r P[i, r] rel[r]  ->  d_head[i] +=, d_tail[i] +=          d_rel[r] += sum_i P[i, r] g[i]
//
// The candidates are few (50 .. 1500 relations), the work is small and what counts is launches and trips through
// memory: the left operand g exists nowhere - it is formed from the two gathered rows on the way to LDS - and no
// [S, n_rel] buffer exists either: scores live in MFMA accumulators and become (m, l) states or P tiles in LDS.
//
//   k_rlse_fwd    one 64-row tile per workgroup, one launch.  RESIDENT (W <= 512): the [W][64] image of g stays in LDS
//                 for the whole kernel and only relation slices stream; wider rows re-form g per relation tile.  After
//                 each 64-relation tile every lane folds its 16 scores into 16 running (m, l) pairs in registers;
//                 the lanes' pairs are merged once at the end, in a fixed order
//   k_rlse_bwd    one launch, two kinds of workgroup that share everything but the roles of their operands:
//                 ROWS   a 64-row tile; per relation tile: scores -> P as an [r][row] image -> d_g (64 x window, up
//                        to 8 accumulator tiles) += P x rel; then d_g goes through LDS into d_head / d_tail
//                 REL    a 64-relation tile and one share of the rows; per row tile: scores -> P as a [row][r] image ->
//                        (64 relations x window) += P^T x g; the share's partial goes to the workspace
//   k_rlse_merge  d_rel += the shares' partials, in share order
//
// A window is 512 columns (DistMult) or 256 re / im pairs (ComplEx: the pair stays together, so the chain rule needs
// no second window); wider rows take further workgroups that recompute the scores.  Tile, images and staging helpers
// are mfma_tile.h's.  No float atomics: every output element has one owner and a fixed order of summation.
#include "common.h"
#include "mfma_tile.h"

namespace bess {
namespace {

constexpr int RESIDENT_MAX_W = 512;  // 16 slices of the g image beside the relation table's two buffers: 150,528 bytes
constexpr int NCT = 8;               // accumulator tiles of a backward window
constexpr int MAX_SPLIT = 8;         // shares of the rows on the relation side
static_assert((2 * B_IMG + (RESIDENT_MAX_W / TK) * TK * LD_T + 2 * TT) * 4 <= LDS_LIMIT, "the g image of RESIDENT_MAX_W must fit");

template <typename T>
struct LseArgs {
    const T *head, *tail, *rel;
    const int32_t *head_idx, *tail_idx;
    int64_t ldh, ldt, ldr, S, n_rel;
    int W;
    float* lse_out;  // forward
    // backward
    const int32_t* rel_idx;
    const float *lse, *coef;
    float *d_head, *d_tail, *parts;
    int64_t ld_dh, ld_dt;
    int we, n_win, n_split, tiles_per_split, n_row_wg;
};

struct Lane {
    int t, wm, wn, l31, lk;
};
__device__ __forceinline__ Lane this_lane() {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    return Lane{t, (wave >> 1) * 32, (wave & 1) * 32, lane & 31, lane >> 5};
}

// load4 of mfma_tile.h for either table type (fp16: one 8-byte load, converted)
template <typename T, bool VEC4>
__device__ __forceinline__ void load4t(const T* __restrict__ row, int64_t c, int64_t c_end, bool live, float (&v)[4]) {
    if constexpr (VEC4) {
        VecLoad<T, 4>::load(row + min(c, c_end - 4), v);
        live = live && c < c_end;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = live ? v[i] : 0.f;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = (live && c + i < c_end) ? to_f32(row[c + i]) : 0.f;
    }
}

// g(h, t)[c .. c + 3]; zeros where the row is not live or the column is at or past c_end (<= W).  ComplEx rows are
// [re | im] (prepare.hip); VEC4 there means W % 8 == 0: a chunk never spans the two halves.
template <typename T, bool CPLX, bool VEC4>
__device__ __forceinline__ void form_g4(const T* __restrict__ h, const T* __restrict__ t, int64_t c, int W, int64_t c_end,
                                        bool live, float (&g)[4]) {
    if constexpr (!CPLX) {
        float a[4], b[4];
        load4t<T, VEC4>(h, c, c_end, live, a);
        load4t<T, VEC4>(t, c, c_end, live, b);
#pragma unroll
        for (int i = 0; i < 4; ++i) g[i] = a[i] * b[i];
    } else if constexpr (VEC4) {
        const int64_t d = W / 2;
        const bool im = c >= d;
        const int64_t e = im ? c - d : c;
        live = live && c < c_end;
        float h1[4], h2[4], t1[4], t2[4];
        load4t<T, true>(h, e, d, live, h1);
        load4t<T, true>(h + d, e, d, live, h2);
        load4t<T, true>(t, e, d, live, t1);
        load4t<T, true>(t + d, e, d, live, t2);
#pragma unroll
        for (int i = 0; i < 4; ++i) g[i] = im ? h1[i] * t2[i] - h2[i] * t1[i] : h1[i] * t1[i] + h2[i] * t2[i];
    } else {
        const int64_t d = W / 2;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t col = c + i;
            g[i] = 0.f;
            if (live && col < c_end) {
                const bool im = col >= d;
                const int64_t e = im ? col - d : col;
                const float h1 = to_f32(h[e]), h2 = to_f32(h[d + e]), t1 = to_f32(t[e]), t2 = to_f32(t[d + e]);
                g[i] = im ? h1 * t2 - h2 * t1 : h1 * t1 + h2 * t2;
            }
        }
    }
}

template <typename T>
__device__ __forceinline__ const T* source_row(const T* base, const int32_t* idx, int64_t ld, int64_t i) {
    return base + (idx ? static_cast<int64_t>(idx[i]) : i) * ld;
}

// The head, tail (rows m0 + p * 32 + t / 8) and relation rows (n0 + p * 32 + t / 8) a thread stages for a score tile.
template <typename T>
struct ScoreRows {
    const T *h[2], *t[2], *r[2];
    bool live[2], rlive[2];
    __device__ __forceinline__ void rows(const LseArgs<T>& A, int64_t m0, int tid) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int64_t m = m0 + p * 32 + (tid >> 3), mc = min(m, A.S - 1);
            live[p] = m < A.S;
            h[p] = source_row(A.head, A.head_idx, A.ldh, mc);
            t[p] = source_row(A.tail, A.tail_idx, A.ldt, mc);
        }
    }
    __device__ __forceinline__ void relations(const LseArgs<T>& A, int64_t n0, int tid) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int64_t n = n0 + p * 32 + (tid >> 3);
            rlive[p] = n < A.n_rel;
            r[p] = A.rel + min(n, A.n_rel - 1) * A.ldr;
        }
    }
};

// ------------------------------------------------------------------------------------------------- forward
// grid ceil(S / 64).  LDS: [2][32 x 68] relation slices | the g image: RESIDENT [ceil(W / 32) * 32][65], else [2][32 x 68]
// | [64][2] (m, l) of the right-hand waves.
template <typename T, bool CPLX, bool VEC4, bool RESIDENT>
__global__ __launch_bounds__(256) void k_rlse_fwd(LseArgs<T> A) {
    extern __shared__ __attribute__((aligned(16))) float lds[];  // (all of it dynamic: the whole CU's LDS can be reserved)
    float* const Bs = lds;
    float* const Gs = lds + 2 * B_IMG;
    const Lane L = this_lane();
    const int64_t m0 = static_cast<int64_t>(blockIdx.x) * TT;
    const int W = A.W, nsl = (W + TK - 1) / TK;
    float(*const s_ml)[2] = reinterpret_cast<float(*)[2]>(Gs + (RESIDENT ? nsl * TK * LD_T : 2 * B_IMG));  // [64]: the waves' exchange
    const int n_tile = static_cast<int>((A.n_rel + TT - 1) / TT);
    const int64_t c = (L.t & 7) * 4;
    ScoreRows<T> R;
    R.rows(A, m0, L.t);
    R.relations(A, 0, L.t);
    float gv[2][4], bv[2][4];
    auto load_g = [&](int j) {
#pragma unroll
        for (int p = 0; p < 2; ++p) form_g4<T, CPLX, VEC4>(R.h[p], R.t[p], static_cast<int64_t>(j) * TK + c, W, W, R.live[p], gv[p]);
    };
    auto load_b = [&](int j) {
#pragma unroll
        for (int p = 0; p < 2; ++p) load4t<T, VEC4>(R.r[p], static_cast<int64_t>(j) * TK + c, W, R.rlive[p], bv[p]);
    };
    if (RESIDENT) {
        for (int j = 0; j < nsl; ++j) {
            load_g(j);
            store_transposed(Gs + j * TK * LD_T, gv);
        }
    } else {
        load_g(0);
        store_transposed(Gs, gv);
    }
    load_b(0);
    store_transposed(Bs, bv);
    float m[16], l[16];  // running log-sum-exp of row acc_row(r, lk) over the columns this lane has seen
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        m[r] = -INFINITY;
        l[r] = 0.f;
    }
    f32x16 acc;
    zero_acc(acc);
    __syncthreads();

    const int total = n_tile * nsl;
    int tile = 0, j = 0;
    for (int s = 0; s < total; ++s) {
        const int cur = s & 1;
        const bool more = s + 1 < total;
        const int jn = j + 1 == nsl ? 0 : j + 1, tn = j + 1 == nsl ? tile + 1 : tile;
        if (more) {  // issued ahead of this slice's MFMAs
            if (jn == 0) R.relations(A, static_cast<int64_t>(tn) * TT, L.t);
            load_b(jn);
            if (!RESIDENT) load_g(jn);
        }
        mfma_slice<LD_T, LD_T, false>(RESIDENT ? Gs + j * TK * LD_T : Gs + cur * B_IMG, Bs + cur * B_IMG, acc, L.wm, L.wn,
                                      L.l31, L.lk, 1.f);
        if (jn == 0) {  // the tile is complete; relations at or past n_rel are no candidates
            if (static_cast<int64_t>(tile) * TT + L.wn + L.l31 < A.n_rel) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float d = acc[r] - m[r], e = __expf(-fabsf(d));  // (m = -inf: d = +inf, e = 0, l = 1)
                    l[r] = d > 0.f ? l[r] * e + 1.f : l[r] + e;
                    m[r] = fmaxf(m[r], acc[r]);
                }
            }
            zero_acc(acc);
        }
        if (more) {
            store_transposed(Bs + (cur ^ 1) * B_IMG, bv);
            if (!RESIDENT) store_transposed(Gs + (cur ^ 1) * B_IMG, gv);
        }
        __syncthreads();
        tile = tn;
        j = jn;
    }
    // the 32 lanes of a row, then the two waves side by side: a fixed tree
#pragma unroll
    for (int r = 0; r < 16; ++r)
#pragma unroll
        for (int x = 1; x < 32; x <<= 1) lse_merge(m[r], l[r], __shfl_xor(m[r], x, 64), __shfl_xor(l[r], x, 64));
    if (L.wn == 32 && L.l31 == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s_ml[L.wm + acc_row(r, L.lk)][0] = m[r];
            s_ml[L.wm + acc_row(r, L.lk)][1] = l[r];
        }
    }
    __syncthreads();
    if (L.wn == 0 && L.l31 == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = L.wm + acc_row(r, L.lk);
            lse_merge(m[r], l[r], s_ml[row][0], s_ml[row][1]);
            if (m0 + row < A.S) A.lse_out[m0 + row] = m[r] + logf(l[r]);
        }
    }
}

// ------------------------------------------------------------------------------------------------- backward
// Virtual column v of a window -> (column c of the row, end of the valid columns).  DistMult: columns e0 + v.
// ComplEx: v < we is the real part of pair e0 + v, v >= we the imaginary part of pair e0 + v - we.
template <bool CPLX>
__device__ __forceinline__ void window_col(int64_t e0, int we, int W, int v, int64_t& c, int64_t& c_end) {
    if (!CPLX) {
        c = e0 + v;
        c_end = W;
    } else if (v < we) {
        c = e0 + v;
        c_end = W / 2;
    } else {
        c = W / 2 + e0 + (v - we);
        c_end = W;
    }
}

// the scores of rows R.h / R.t against the relations R.r, streamed in slices of 32 through Gs / Bs [2][32 x 68]
template <typename T, bool CPLX, bool VEC4>
__device__ __forceinline__ void score_tile(const ScoreRows<T>& R, int W, float* Gs, float* Bs, f32x16& acc, const Lane& L) {
    const int nsl = (W + TK - 1) / TK;
    const int64_t c = (L.t & 7) * 4;
    float gv[2][4], bv[2][4];
    auto load = [&](int j) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            form_g4<T, CPLX, VEC4>(R.h[p], R.t[p], static_cast<int64_t>(j) * TK + c, W, W, R.live[p], gv[p]);
            load4t<T, VEC4>(R.r[p], static_cast<int64_t>(j) * TK + c, W, R.rlive[p], bv[p]);
        }
    };
    load(0);
    store_transposed(Gs, gv);
    store_transposed(Bs, bv);
    zero_acc(acc);
    __syncthreads();
    for (int s = 0; s < nsl; ++s) {
        const int cur = s & 1;
        const bool more = s + 1 < nsl;
        if (more) load(s + 1);
        mfma_slice<LD_T, LD_T, false>(Gs + cur * B_IMG, Bs + cur * B_IMG, acc, L.wm, L.wn, L.l31, L.lk, 1.f);
        if (more) {
            store_transposed(Gs + (cur ^ 1) * B_IMG, gv);
            store_transposed(Bs + (cur ^ 1) * B_IMG, bv);
        }
        __syncthreads();
    }
}

// acc[ct] += P (the [64][65] image Ps, reduction index first) x the 64 x 64 tiles ct < nct of the right operand, whose
// slices ld(rs, ct, v) come as [reduction index][column] shares of store_direct
template <typename LOADER>
__device__ __forceinline__ void accumulate_tiles(const float* Ps, float* Bs, f32x16 (&acc)[NCT], int nct, LOADER&& ld,
                                                 const Lane& L) {
    float v[2][4];
    ld(0, 0, v);
    store_direct(Bs, v);
    __syncthreads();  // (Ps too)
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        if (ct < nct) {
#pragma unroll
            for (int rs = 0; rs < 2; ++rs) {
                const bool more = rs == 0 || ct + 1 < nct;
                if (more) ld(rs ^ 1, rs == 0 ? ct : ct + 1, v);
                mfma_slice<LD_T, LD_D, false>(Ps + rs * TK * LD_T, Bs + rs * B_IMG, acc[ct], L.wm, L.wn, L.l31, L.lk, 1.f);
                if (more) store_direct(Bs + (rs ^ 1) * B_IMG, v);
                __syncthreads();
            }
        }
    }
}

constexpr int BWD_STREAM_FLOATS = 4 * B_IMG + TT * LD_T;  // Gs [2] | Bs [2] | Ps
constexpr int BWD_ROW_FLOATS = 3 * TT;                    // behind them: lse, coef, relation id of the tile's rows
__host__ __device__ inline int bwd_image_floats(int nct) {
    const int stage = nct * TT * LD_T;  // the ROWS epilogue's d_g image takes the streams' place
    return stage > BWD_STREAM_FLOATS ? stage : BWD_STREAM_FLOATS;
}

// grid n_row_wg + (relation tiles x shares x windows)
template <typename T, bool CPLX, bool VEC4>
__global__ __launch_bounds__(256) void k_rlse_bwd(LseArgs<T> A) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* const Gs = lds;
    float* const Bs = lds + 2 * B_IMG;
    float* const Ps = lds + 4 * B_IMG;
    const Lane L = this_lane();
    const int W = A.W, we = A.we;
    const int nct = (CPLX ? 2 : 1) * (we / TT);
    float* const s_lse = lds + bwd_image_floats(nct);
    float* const s_coef = s_lse + TT;
    int* const s_rel = reinterpret_cast<int*>(s_coef + TT);
    const int64_t S = A.S, n_rel = A.n_rel, d = W / 2;
    const int row_tiles = static_cast<int>((S + TT - 1) / TT), rel_tiles = static_cast<int>((n_rel + TT - 1) / TT);
    const bool rows_role = static_cast<int>(blockIdx.x) < A.n_row_wg;
    int b = rows_role ? blockIdx.x : blockIdx.x - A.n_row_wg;
    const int64_t e0 = static_cast<int64_t>(b % A.n_win) * (CPLX ? NCT / 2 : NCT) * TT;
    b /= A.n_win;
    // ROWS: row tile b against every relation tile; REL: relation tile b / n_split against the row tiles of its share
    const int fixed = rows_role ? b : b / A.n_split;
    const int first = rows_role ? 0 : (b % A.n_split) * A.tiles_per_split;
    const int last = rows_role ? rel_tiles : min(row_tiles, first + A.tiles_per_split);

    f32x16 acc[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) zero_acc(acc[ct]);
    ScoreRows<T> R;
    for (int it = first; it < last; ++it) {
        const int64_t m0 = static_cast<int64_t>(rows_role ? fixed : it) * TT, n0 = static_cast<int64_t>(rows_role ? it : fixed) * TT;
        if (rows_role ? it == first : true) {
            R.rows(A, m0, L.t);
            if (L.t < TT) {
                const int64_t m = min(m0 + L.t, S - 1);
                s_lse[L.t] = A.lse[m];
                s_coef[L.t] = m0 + L.t < S ? A.coef[m] : 0.f;
                s_rel[L.t] = A.rel_idx[m];
            }
        }
        if (rows_role ? true : it == first) R.relations(A, n0, L.t);
        f32x16 sc;
        score_tile<T, CPLX, VEC4>(R, W, Gs, Bs, sc, L);  // (its barriers publish s_lse / s_coef / s_rel)
        const int64_t col = n0 + L.wn + L.l31;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = L.wm + acc_row(r, L.lk);
            const float co = s_coef[row];
            const float p = __expf(sc[r] - s_lse[row]) - (col == s_rel[row] ? 1.f : 0.f);
            // ROWS: [relation][row]; REL: [row][relation] - the reduction index first
            Ps[rows_role ? (L.wn + L.l31) * LD_T + row : row * LD_T + L.wn + L.l31] = (co == 0.f || col >= n_rel) ? 0.f : co * p;
        }
        if (rows_role) {
            accumulate_tiles(Ps, Bs, acc, nct, [&](int rs, int ct, float (&v)[2][4]) {
                int64_t c, c_end;
                window_col<CPLX>(e0, we, W, ct * TT + (L.t & 15) * 4, c, c_end);
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    const int64_t n = n0 + rs * TK + p * 16 + (L.t >> 4);
                    load4t<T, VEC4>(A.rel + min(n, n_rel - 1) * A.ldr, c, c_end, n < n_rel, v[p]);
                }
            }, L);
        } else {
            accumulate_tiles(Ps, Bs, acc, nct, [&](int rs, int ct, float (&v)[2][4]) {
                int64_t c, c_end;
                window_col<CPLX>(e0, we, W, ct * TT + (L.t & 15) * 4, c, c_end);
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    const int64_t m = m0 + rs * TK + p * 16 + (L.t >> 4), mc = min(m, S - 1);
                    form_g4<T, CPLX, VEC4>(source_row(A.head, A.head_idx, A.ldh, mc), source_row(A.tail, A.tail_idx, A.ldt, mc),
                                           c, W, c_end, m < S, v[p]);
                }
            }, L);
        }
    }

    if (!rows_role) {  // the share's partial of d_rel: [share][relation][column]
        const int share = b % A.n_split;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            if (ct < nct) {
                int64_t c, c_end;
                window_col<CPLX>(e0, we, W, ct * TT + L.wn + L.l31, c, c_end);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t rel = static_cast<int64_t>(fixed) * TT + L.wm + acc_row(r, L.lk);
                    if (rel < n_rel && c < c_end) A.parts[(share * n_rel + rel) * W + c] = acc[ct][r];
                }
            }
        }
        return;
    }
    // d_g of the window as a [virtual column][row] image, then the chain rule: one owner per element of d_head / d_tail
    float* const Ds = lds;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        if (ct < nct) {
#pragma unroll
            for (int r = 0; r < 16; ++r) Ds[(ct * TT + L.wn + L.l31) * LD_T + L.wm + acc_row(r, L.lk)] = acc[ct][r];
        }
    }
    __syncthreads();
    const int64_t m0 = static_cast<int64_t>(fixed) * TT;
    for (int i = L.t; i < TT * we; i += 256) {
        const int m = i / we, v = i % we;
        const int64_t row = m0 + m, e = e0 + v;
        if (row >= S || e >= (CPLX ? d : W)) continue;
        const T* const h = source_row(A.head, A.head_idx, A.ldh, row);
        const T* const t = source_row(A.tail, A.tail_idx, A.ldt, row);
        float* const dh = A.d_head + row * A.ld_dh;
        float* const dt = A.d_tail + row * A.ld_dt;
        if (!CPLX) {
            const float g = Ds[v * LD_T + m];
            dh[e] += g * to_f32(t[e]);
            dt[e] += g * to_f32(h[e]);
        } else {
            const float ga = Ds[v * LD_T + m], gb = Ds[(we + v) * LD_T + m];
            const float h1 = to_f32(h[e]), h2 = to_f32(h[d + e]), t1 = to_f32(t[e]), t2 = to_f32(t[d + e]);
            dh[e] += ga * t1 + gb * t2;
            dh[d + e] += ga * t2 - gb * t1;
            dt[e] += ga * h1 - gb * h2;
            dt[d + e] += ga * h2 + gb * h1;
        }
    }
}

// d_rel[r, c] += parts[0][r][c] + parts[1][r][c] + ... in that order
__global__ __launch_bounds__(256) void k_rlse_merge(const float* __restrict__ parts, int n_part, int64_t n_rel, int W,
                                                    float* __restrict__ d_rel, int64_t ld) {
    const int64_t n = n_rel * W;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += 256ll * gridDim.x) {
        float acc = parts[i];
        for (int p = 1; p < n_part; ++p) acc += parts[p * n + i];
        d_rel[(i / W) * ld + i % W] += acc;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------
int check_problem(const char* who, const bess_model_desc* d, int64_t S, int64_t n_rel) {
    BESS_REQUIRE(d, "%s: NULL descriptor", who);
    if (int rc = check_desc(d)) return rc;
    BESS_REQUIRE(d->scorer == BESS_DISTMULT || d->scorer == BESS_COMPLEX,
                 "%s: DistMult or ComplEx only (the score must be a dot product with the relation row)", who);
    BESS_REQUIRE(d->rel_width == d->width && d->width >= 1 && d->width <= 32768 && (d->scorer != BESS_COMPLEX || d->width % 2 == 0),
                 "%s: rel_width == width, 1 <= width <= 32768, even for ComplEx (got %d, %d)", who, d->width, d->rel_width);
    BESS_REQUIRE(S >= 0 && S < (1ll << 22) && n_rel >= 1 && n_rel < (1ll << 24), "%s: 0 <= S < 2^22 and 1 <= n_rel < 2^24", who);
    return BESS_OK;
}

// how the backward splits: the window's extent, the windows, the shares of the rows on the relation side
struct BwdPlan {
    int we, n_win, n_split, tiles_per_split;
    int64_t row_tiles, rel_tiles;
};
BwdPlan bwd_plan(const bess_model_desc* d, int64_t S, int64_t n_rel) {
    const bool cplx = d->scorer == BESS_COMPLEX;
    const int64_t units = cplx ? d->width / 2 : d->width, we_max = (cplx ? NCT / 2 : NCT) * TT;
    BwdPlan P;
    P.we = static_cast<int>(units < we_max ? ceil_div(units, TT) * TT : we_max);
    P.n_win = static_cast<int>(ceil_div(units, we_max));
    P.row_tiles = ceil_div(S, TT);
    P.rel_tiles = ceil_div(n_rel, TT);
    // shares: fill the 256 CUs beside the row tiles, at most MAX_SPLIT partials to merge
    int64_t want = (256 - P.row_tiles * P.n_win) / (P.rel_tiles * P.n_win);
    want = want < 1 ? 1 : (want > MAX_SPLIT ? MAX_SPLIT : want);
    want = want > P.row_tiles ? (P.row_tiles > 0 ? P.row_tiles : 1) : want;
    P.tiles_per_split = static_cast<int>(ceil_div(P.row_tiles > 0 ? P.row_tiles : 1, want));
    P.n_split = static_cast<int>(ceil_div(P.row_tiles > 0 ? P.row_tiles : 1, P.tiles_per_split));
    return P;
}
inline int64_t bwd_ws_bytes(const bess_model_desc* d, const BwdPlan& P, int64_t n_rel) { return P.n_split * n_rel * d->width * 4; }

struct Operands {
    const void *head, *tail, *rel;
    int64_t ldh, ldt, ldr;
};
// whole 4-scalar chunks at aligned addresses everywhere (ComplEx: in both halves of a row)
bool vec4_class(const bess_model_desc* d, const Operands& O) {
    const int64_t chunk = 4 * scalar_bytes_of(d);
    auto ok = [&](const void* p, int64_t ld) { return reinterpret_cast<uintptr_t>(p) % chunk == 0 && ld % 4 == 0; };
    return d->width % (d->scorer == BESS_COMPLEX ? 8 : 4) == 0 && ok(O.head, O.ldh) && ok(O.tail, O.ldt) && ok(O.rel, O.ldr);
}

template <typename F>
void dispatch(const bess_model_desc* d, bool vec4, F&& f) {
    with_table_type(d->dtype, [&](auto t) {
        with_flag(d->scorer == BESS_COMPLEX, [&](auto cp) { with_flag(vec4, [&](auto v4) { f(t, cp, v4); }); });
        return 0;
    });
}

#define RLSE_CHECK_ROWS(who)                                                                                           \
    if (int rc = check_problem(who, d, S, n_rel)) return rc;                                                           \
    BESS_REQUIRE(ld_head >= d->width && ld_tail >= d->width && ld_rel >= d->width, who ": bad leading dimension")

}  // namespace
}  // namespace bess

using namespace bess;

extern "C" int bess_relation_lse_fwd(const bess_model_desc* d, const void* head_base, int64_t ld_head,
                                     const int32_t* head_idx, const void* tail_base, int64_t ld_tail,
                                     const int32_t* tail_idx, const void* rel_table, int64_t ld_rel, int64_t n_rel,
                                     int64_t S, float* lse, void* stream) {
    RLSE_CHECK_ROWS("relation_lse_fwd");
    if (S == 0) return BESS_OK;
    BESS_REQUIRE(head_base && tail_base && rel_table && lse, "relation_lse_fwd: NULL pointer");
    const Operands O{head_base, tail_base, rel_table, ld_head, ld_tail, ld_rel};
    const int W = d->width;
    const bool resident = W <= RESIDENT_MAX_W;
    const size_t lds = static_cast<size_t>(2 * B_IMG + (resident ? ceil_div(W, TK) * TK * LD_T : 2 * B_IMG) + 2 * TT) * 4;
    const unsigned grid = static_cast<unsigned>(ceil_div(S, TT));
    bool reserved = true;
    dispatch(d, vec4_class(d, O), [&](auto t, auto cp, auto v4) {
        using T = decltype(t);
        LseArgs<T> A{};
        A.head = static_cast<const T*>(head_base), A.tail = static_cast<const T*>(tail_base), A.rel = static_cast<const T*>(rel_table);
        A.head_idx = head_idx, A.tail_idx = tail_idx;
        A.ldh = ld_head, A.ldt = ld_tail, A.ldr = ld_rel, A.S = S, A.n_rel = n_rel, A.W = W, A.lse_out = lse;
        with_flag(resident, [&](auto rs) {
            constexpr bool CP = decltype(cp)::value, V4 = decltype(v4)::value, RS = decltype(rs)::value;
            static std::atomic<uint64_t> done{0};
            if ((reserved = reserve_lds(k_rlse_fwd<T, CP, V4, RS>, done)))
                k_rlse_fwd<T, CP, V4, RS><<<grid, 256, lds, as_stream(stream)>>>(A);
        });
    });
    BESS_REQUIRE(reserved, "relation_lse_fwd: cannot reserve %lld bytes of LDS", static_cast<long long>(LDS_LIMIT));
    return check_launch("relation_lse_fwd");
}

extern "C" int bess_relation_lse_workspace(const bess_model_desc* d, int64_t S, int64_t n_rel, int64_t* bytes) {
    BESS_REQUIRE(bytes, "relation_lse_workspace: NULL pointer");
    if (int rc = check_problem("relation_lse_workspace", d, S, n_rel)) return rc;
    *bytes = bwd_ws_bytes(d, bwd_plan(d, S, n_rel), n_rel);
    return BESS_OK;
}

extern "C" int bess_relation_lse_bwd(const bess_model_desc* d, const void* head_base, int64_t ld_head,
                                     const int32_t* head_idx, const void* tail_base, int64_t ld_tail,
                                     const int32_t* tail_idx, const void* rel_table, int64_t ld_rel, int64_t n_rel,
                                     const int32_t* rel_idx, const float* lse, const float* coef, int64_t S,
                                     float* d_head, int64_t ld_dhead, float* d_tail, int64_t ld_dtail, float* d_rel,
                                     int64_t ld_drel, void* workspace, int64_t workspace_bytes, void* stream) {
    RLSE_CHECK_ROWS("relation_lse_bwd");
    BESS_REQUIRE(ld_dhead >= d->width && ld_dtail >= d->width && ld_drel >= d->width, "relation_lse_bwd: bad leading dimension");
    if (S == 0) return BESS_OK;  // nothing is added
    BESS_REQUIRE(head_base && tail_base && rel_table && rel_idx && lse && coef && d_head && d_tail && d_rel,
                 "relation_lse_bwd: NULL pointer");
    const BwdPlan P = bwd_plan(d, S, n_rel);
    BESS_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= bwd_ws_bytes(d, P, n_rel),
                 "relation_lse_bwd: workspace too small (bess_relation_lse_workspace) or misaligned");
    const Operands O{head_base, tail_base, rel_table, ld_head, ld_tail, ld_rel};
    const int W = d->width;
    const int nct = (d->scorer == BESS_COMPLEX ? 2 : 1) * (P.we / TT);
    const size_t lds = static_cast<size_t>(bwd_image_floats(nct) + BWD_ROW_FLOATS) * 4;
    const int n_row_wg = static_cast<int>(P.row_tiles * P.n_win);
    const unsigned grid = static_cast<unsigned>(n_row_wg + P.rel_tiles * P.n_split * P.n_win);
    hipStream_t st = as_stream(stream);
    bool reserved = true;
    dispatch(d, vec4_class(d, O), [&](auto t, auto cp, auto v4) {
        using T = decltype(t);
        constexpr bool CP = decltype(cp)::value, V4 = decltype(v4)::value;
        LseArgs<T> A{};
        A.head = static_cast<const T*>(head_base), A.tail = static_cast<const T*>(tail_base), A.rel = static_cast<const T*>(rel_table);
        A.head_idx = head_idx, A.tail_idx = tail_idx;
        A.ldh = ld_head, A.ldt = ld_tail, A.ldr = ld_rel, A.S = S, A.n_rel = n_rel, A.W = W;
        A.rel_idx = rel_idx, A.lse = lse, A.coef = coef;
        A.d_head = d_head, A.d_tail = d_tail, A.parts = static_cast<float*>(workspace), A.ld_dh = ld_dhead, A.ld_dt = ld_dtail;
        A.we = P.we, A.n_win = P.n_win, A.n_split = P.n_split, A.tiles_per_split = P.tiles_per_split, A.n_row_wg = n_row_wg;
        static std::atomic<uint64_t> done{0};
        if ((reserved = reserve_lds(k_rlse_bwd<T, CP, V4>, done))) k_rlse_bwd<T, CP, V4><<<grid, 256, lds, st>>>(A);
    });
    BESS_REQUIRE(reserved, "relation_lse_bwd: cannot reserve %lld bytes of LDS", static_cast<long long>(LDS_LIMIT));
    if (int rc = check_launch("relation_lse_bwd")) return rc;
    int64_t blocks = ceil_div(n_rel * W, 256);
    blocks = blocks > 2048 ? 2048 : blocks;
    k_rlse_merge<<<static_cast<unsigned>(blocks), 256, 0, st>>>(static_cast<const float*>(workspace), P.n_split, n_rel, W, d_rel,
                                                                ld_drel);
    return check_launch("relation_lse_merge");
}
