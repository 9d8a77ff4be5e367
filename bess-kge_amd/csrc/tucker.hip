// TuckER's query product on the CDNA4 matrix cores, and its three gradients:
//
//     q[m, n] = sum_{k, j} rel[m, k] * x[m, j] * B_k(j, n)          (exact fp32, v_mfma_f32_32x32x2_f32)
//
// with the core stored as the GEMM's right operand, core [dr * de, de]: row (k, a), column b = W[k, a, b]
// (relation, head, tail).  B_k(j, n) = W[k, j, n] for tail corruption (x = head rows) and W[k, n, j] for head
// corruption (x = tail rows, `swap_axes`): the same kernels read the core's slice along its other axis and stage it
// transposed, no transposed copy of the core is ever made.
//
// It is a GEMM [S, dr * de] x [dr * de, de] whose left operand is an outer product.  That operand exists nowhere: the
// 64 x de tile of x sits in LDS as an [a][m] image for the whole kernel and a lane forms its MFMA fragment on the read,
// lds_x[a][m] * rel[m, k] - a lane's row m never changes, so rel[m, k] is one register per k.
//
//   k_tucker_fwd       q (and d_x: the same product with dq in the place of x and the axes exchanged)
//   k_tucker_bwd_rel   d_rel[m, k] = sum_n dq[m, n] (sum_j x[m, j] B_k(j, n)): the forward's loop with the
//                      accumulators cleared per k, multiplied by dq in accumulator layout and summed over the wave's
//                      32 columns; one partial per wave column, merged in a fixed order by k_tucker_merge_parts
//   k_tucker_bwd_core  d_core[(k, a), b] = sum_m rel[m, k] u[m, a] v[m, b], (u, v) = (x, dq) or, with exchanged axes,
//                      (dq, x): one 64 x 64 tile of one k per workgroup, reduction over the rows
//
// Conventions are gemm_mfma.hip's (the tile, its LDS images and their staging helpers: mfma_tile.h), global -> register
// -> LDS staging split around the MFMA phase.  Only 64-tiles: the product has de output columns, so 128-tiles would give
// ceil(S / 128) * ceil(de / 128) workgroups - 64 at S = 4096, de = 200, a quarter of the chip.
// No atomics anywhere: every output element is written once, by one lane, in a fixed order of summation.
#include "common.h"
#include "mfma_tile.h"

namespace bess {
namespace {

constexpr int TUCKER_MAX_DE = 544;                // 17 slices of the resident x image beside the core's two buffers

inline int64_t rows_lds_bytes(int64_t de) { return (2 * B_IMG + ceil_div(de, TK) * TK * LD_T) * 4; }
static_assert((2 * B_IMG + (TUCKER_MAX_DE / TK) * TK * LD_T) * 4 <= LDS_LIMIT, "the x image of TUCKER_MAX_DE must fit");

struct RowsArgs {
    const float* x;     // [S, de]: the rows whose tile stays in LDS
    const float* rel;   // [S, dr]
    const float* core;  // [dr * de, de]
    const float* dq;    // REL: [S, de]
    float* out;         // q [S, de], or REL: partials [2 * gridDim.x][S][dr]
    int64_t ldx, ldr, lddq, ldo, S;
    int de, dr;
};

// Body of k_tucker_fwd (REL = false) and k_tucker_bwd_rel (REL = true).  grid (ceil(de / 64), ceil(S / 64)).
// LDS: [2][32 x 68] slices of the core | [ceil(de / 32) * 32][65] image of the x tile.
template <bool SWAP, bool VEC4, bool REL>
__device__ __forceinline__ void tucker_rows(const RowsArgs& A) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* const Bs = lds;
    float* const Xs = lds + 2 * B_IMG;
    constexpr int LDB = MatrixSlice<SWAP, VEC4>::LD;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int l31 = lane & 31, lk = lane >> 5;
    const int64_t m0 = static_cast<int64_t>(blockIdx.y) * TT, n0 = static_cast<int64_t>(blockIdx.x) * TT;
    const int64_t S = A.S, de = A.de;
    const int spk = (A.de + TK - 1) / TK;  // slices per k

    // the x tile, once: rows past S and columns past de are zeros
    for (int j = 0; j < spk; ++j) {
        float v[2][4];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int64_t m = m0 + p * 32 + (t >> 3);
            load4<VEC4>(A.x + min(m, S - 1) * A.ldx, j * TK + (t & 7) * 4, de, m < S, v[p]);
        }
        store_transposed(Xs + j * TK * LD_T, v);
    }
    MatrixSlice<SWAP, VEC4> cs;  // of W[k]
    cs.load(A.core, de, 0, n0);
    cs.store(Bs);
    // the lane's row of rel (clamped: the products of rows past S are never stored)
    const float* relrow = A.rel + min(m0 + wm + l31, S - 1) * A.ldr;
    float rk = REL ? 1.f : relrow[0];
    float g[16];  // REL: the tile of dq in accumulator layout
    if (REL) {
        const int64_t col = n0 + wn + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t row = m0 + wm + acc_row(r, lk);
            g[r] = (row < S && col < de) ? A.dq[row * A.lddq + col] : 0.f;
        }
    }
    f32x16 acc;
    zero_acc(acc);
    __syncthreads();

    const int n_slice = A.dr * spk;
    int k = 0, j = 0;
    for (int s = 0; s < n_slice; ++s) {
        const int cur = s & 1;
        const bool more = s + 1 < n_slice;
        const int jn = j + 1 == spk ? 0 : j + 1, kn = j + 1 == spk ? k + 1 : k;
        float rk_next = rk;
        if (more) {  // issued ahead of this slice's MFMAs
            cs.load(A.core + kn * de * de, de, static_cast<int64_t>(jn) * TK, n0);
            if (!REL && jn == 0) rk_next = relrow[kn];
        }
        mfma_slice<LD_T, LDB, !REL>(Xs + j * TK * LD_T, Bs + cur * B_IMG, acc, wm, wn, l31, lk, rk);
        if (REL && jn == 0) {
            // this k is complete: times dq, summed over the wave's 32 columns; lane r of each half keeps row r's sum
            float mine = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v = row16_allreduce_sum(acc[r] * g[r]);
                v += __shfl_xor(v, 16, 64);
                mine = l31 == r ? v : mine;
            }
            const int64_t row = m0 + wm + acc_row(l31 & 15, lk);
            const int64_t part = static_cast<int64_t>(blockIdx.x) * 2 + (wave & 1);
            if (l31 < 16 && row < S) A.out[(part * S + row) * A.dr + k] = mine;
            zero_acc(acc);
        }
        if (more) cs.store(Bs + (cur ^ 1) * B_IMG);
        __syncthreads();
        k = kn;
        j = jn;
        rk = rk_next;
    }
    if (!REL) {
        const int64_t col = n0 + wn + l31;
        if (col < de) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t row = m0 + wm + acc_row(r, lk);
                if (row < S) A.out[row * A.ldo + col] = acc[r];
            }
        }
    }
}

template <bool SWAP, bool VEC4>
__global__ __launch_bounds__(256) void k_tucker_fwd(RowsArgs A) {
    tucker_rows<SWAP, VEC4, false>(A);
}
template <bool SWAP, bool VEC4>
__global__ __launch_bounds__(256) void k_tucker_bwd_rel(RowsArgs A) {
    tucker_rows<SWAP, VEC4, true>(A);
}

// d_rel[m, k] = parts[0][m][k] + parts[1][m][k] + ... in that order
__global__ __launch_bounds__(256) void k_tucker_merge_parts(const float* __restrict__ parts, int n_part, int64_t S, int dr,
                                                            float* __restrict__ d_rel, int64_t ld) {
    const int64_t n = S * dr;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += 256ll * gridDim.x) {
        float acc = parts[i];
        for (int p = 1; p < n_part; ++p) acc += parts[p * n + i];
        d_rel[(i / dr) * ld + i % dr] = acc;
    }
}

// d_core[(k, a0 ..), b0 ..] = sum_m rel[m, k] u[m, a] v[m, b].  grid (ceil(de / 64), ceil(de / 64), dr): b tile, a tile, k.
// Both operands are "reduction index = row" images; the rows of u are scaled by rel[m, k] as they are staged.
template <bool VEC4>
__global__ __launch_bounds__(256) void k_tucker_bwd_core(const float* __restrict__ u, int64_t ldu,
                                                         const float* __restrict__ v, int64_t ldv,
                                                         const float* __restrict__ rel, int64_t ldr,
                                                         float* __restrict__ d_core, int64_t S, int de) {
    __shared__ __attribute__((aligned(16))) float As[2][B_IMG];
    __shared__ __attribute__((aligned(16))) float Vs[2][B_IMG];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int l31 = lane & 31, lk = lane >> 5;
    const int64_t b0 = static_cast<int64_t>(blockIdx.x) * TT, a0 = static_cast<int64_t>(blockIdx.y) * TT;
    const int64_t k = blockIdx.z;
    float sa[2][4], sv[2][4];
    auto load = [&](int64_t ms) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int64_t m = ms + p * 16 + (t >> 4), mr = min(m, S - 1);
            const int64_t c = (t & 15) * 4;
            const float r = rel[mr * ldr + k];
            load4<VEC4>(u + mr * ldu, a0 + c, de, m < S, sa[p]);
            load4<VEC4>(v + mr * ldv, b0 + c, de, m < S, sv[p]);
#pragma unroll
            for (int i = 0; i < 4; ++i) sa[p][i] *= r;
        }
    };
    load(0);
    store_direct(As[0], sa);
    store_direct(Vs[0], sv);
    f32x16 acc;
    zero_acc(acc);
    __syncthreads();
    const int n_slice = static_cast<int>((S + TK - 1) / TK);
    for (int s = 0; s < n_slice; ++s) {
        const int cur = s & 1;
        const bool more = s + 1 < n_slice;
        if (more) load(static_cast<int64_t>(s + 1) * TK);
        mfma_slice<LD_D, LD_D, false>(As[cur], Vs[cur], acc, wm, wn, l31, lk, 1.f);
        if (more) {
            store_direct(As[cur ^ 1], sa);
            store_direct(Vs[cur ^ 1], sv);
        }
        __syncthreads();
    }
    const int64_t col = b0 + wn + l31;
    if (col < de) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t row = a0 + wm + acc_row(r, lk);
            if (row < de) d_core[(k * de + row) * de + col] = acc[r];
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------
inline int64_t rel_parts(int64_t de) { return 2 * ceil_div(de, TT); }  // one per 32-column wave tile
inline int64_t rel_ws_bytes(int64_t S, int64_t de, int64_t dr) { return rel_parts(de) * S * dr * 4; }

int check_shape(const char* who, int64_t S, int64_t de, int64_t dr) {
    BESS_REQUIRE(S >= 0 && de >= 1 && dr >= 1, "%s: S >= 0, de >= 1 and dr >= 1 (got %lld, %lld, %lld)", who,
                 static_cast<long long>(S), static_cast<long long>(de), static_cast<long long>(dr));
    BESS_REQUIRE(S < (1ll << 22) && dr <= 65535, "%s: S < 2^22 and dr <= 65535", who);
    if (de > TUCKER_MAX_DE)
        return fail(BESS_EUNSUPPORTED, "%s: de = %lld is above %d (the 64 x de tile of the rows stays in LDS)", who,
                    static_cast<long long>(de), TUCKER_MAX_DE);
    return BESS_OK;
}

// q (REL false) or the partials of d_rel (REL true) of one product
int launch_rows(bool rel_grad, bool swap, RowsArgs A, hipStream_t st) {
    const bool vec4 = A.de % 4 == 0 && A.ldx % 4 == 0 && aligned16(A.x) && aligned16(A.core);
    const dim3 grid(static_cast<unsigned>(ceil_div(A.de, TT)), static_cast<unsigned>(ceil_div(A.S, TT)));
    const size_t lds = static_cast<size_t>(rows_lds_bytes(A.de));
    bool reserved = true;
    with_flag(rel_grad, [&](auto rg) {
        with_flag(swap, [&](auto sw) {
            with_flag(vec4, [&](auto v4) {
                constexpr bool RG = decltype(rg)::value, SW = decltype(sw)::value, V4 = decltype(v4)::value;
                if constexpr (RG) {
                    static std::atomic<uint64_t> done{0};
                    if ((reserved = reserve_lds(k_tucker_bwd_rel<SW, V4>, done))) k_tucker_bwd_rel<SW, V4><<<grid, 256, lds, st>>>(A);
                } else {
                    static std::atomic<uint64_t> done{0};
                    if ((reserved = reserve_lds(k_tucker_fwd<SW, V4>, done))) k_tucker_fwd<SW, V4><<<grid, 256, lds, st>>>(A);
                }
            });
        });
    });
    BESS_REQUIRE(reserved, "tucker_query: cannot reserve %lld bytes of LDS", static_cast<long long>(LDS_LIMIT));
    return check_launch(rel_grad ? "tucker_bwd_rel" : "tucker_fwd");
}

}  // namespace
}  // namespace bess

using namespace bess;

extern "C" int bess_tucker_query_workspace(int64_t S, int64_t de, int64_t dr, int64_t* bytes) {
    BESS_REQUIRE(bytes, "tucker_query_workspace: NULL pointer");
    if (int rc = check_shape("tucker_query_workspace", S, de, dr)) return rc;
    *bytes = rel_ws_bytes(S, de, dr);
    return BESS_OK;
}

extern "C" int bess_tucker_query_fwd(const float* x, int64_t ldx, const float* rel, int64_t ldr, const float* core,
                                     int32_t swap_axes, float* q, int64_t ldq, int64_t S, int64_t de, int64_t dr,
                                     void* workspace, int64_t workspace_bytes, void* stream) {
    if (int rc = check_shape("tucker_query_fwd", S, de, dr)) return rc;
    BESS_REQUIRE(swap_axes == 0 || swap_axes == 1, "tucker_query_fwd: swap_axes is 0 or 1");
    BESS_REQUIRE(ldx >= de && ldr >= dr && ldq >= de && workspace_bytes >= 0, "tucker_query_fwd: bad leading dimension");
    if (S == 0) return BESS_OK;
    BESS_REQUIRE(x && rel && core && q, "tucker_query_fwd: NULL pointer");
    (void)workspace;
    RowsArgs A{x, rel, core, nullptr, q, ldx, ldr, 0, ldq, S, static_cast<int>(de), static_cast<int>(dr)};
    return launch_rows(false, swap_axes != 0, A, as_stream(stream));
}

extern "C" int bess_tucker_query_bwd(const float* x, int64_t ldx, const float* rel, int64_t ldr, const float* core,
                                     int32_t swap_axes, const float* dq, int64_t lddq, float* d_x, int64_t ld_dx,
                                     float* d_rel, int64_t ld_drel, float* d_core, int64_t S, int64_t de, int64_t dr,
                                     void* workspace, int64_t workspace_bytes, void* stream) {
    if (int rc = check_shape("tucker_query_bwd", S, de, dr)) return rc;
    BESS_REQUIRE(swap_axes == 0 || swap_axes == 1, "tucker_query_bwd: swap_axes is 0 or 1");
    BESS_REQUIRE(ldx >= de && ldr >= dr && lddq >= de && (!d_x || ld_dx >= de) && (!d_rel || ld_drel >= dr),
                 "tucker_query_bwd: bad leading dimension");
    const bool swap = swap_axes != 0;
    hipStream_t st = as_stream(stream);
    if (S == 0) {  // d_core of an empty batch is zero; there are no rows
        if (d_core && hipSuccess != fill_words_async(d_core, 0u, dr * de * de, st)) return check_launch("tucker_query_bwd: fill");
        return BESS_OK;
    }
    BESS_REQUIRE(x && rel && core && dq, "tucker_query_bwd: NULL pointer");
    if (d_rel)
        BESS_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= rel_ws_bytes(S, de, dr),
                     "tucker_query_bwd: workspace too small (bess_tucker_query_workspace) or misaligned");
    const int ide = static_cast<int>(de), idr = static_cast<int>(dr);
    if (d_x) {  // the forward product of dq along the core's other axis
        RowsArgs A{dq, rel, core, nullptr, d_x, lddq, ldr, 0, ld_dx, S, ide, idr};
        if (int rc = launch_rows(false, !swap, A, st)) return rc;
    }
    if (d_rel) {
        float* parts = static_cast<float*>(workspace);
        RowsArgs A{x, rel, core, dq, parts, ldx, ldr, lddq, 0, S, ide, idr};
        if (int rc = launch_rows(true, swap, A, st)) return rc;
        int64_t blocks = ceil_div(S * dr, 256);
        blocks = blocks > 2048 ? 2048 : blocks;
        k_tucker_merge_parts<<<static_cast<unsigned>(blocks), 256, 0, st>>>(parts, static_cast<int>(rel_parts(de)), S, idr,
                                                                          d_rel, ld_drel);
        if (int rc = check_launch("tucker_merge_parts")) return rc;
    }
    if (d_core) {
        const float* u = swap ? dq : x;
        const float* v = swap ? x : dq;
        const int64_t ldu = swap ? lddq : ldx, ldv = swap ? ldx : lddq;
        const bool vec4 = de % 4 == 0 && ldu % 4 == 0 && ldv % 4 == 0 && aligned16(u) && aligned16(v);
        const unsigned tiles = static_cast<unsigned>(ceil_div(de, TT));
        const dim3 grid(tiles, tiles, static_cast<unsigned>(dr));
        with_flag(vec4, [&](auto v4) {
            k_tucker_bwd_core<decltype(v4)::value><<<grid, 256, 0, st>>>(u, ldu, v, ldv, rel, ldr, d_core, S, ide);
        });
        if (int rc = check_launch("tucker_bwd_core")) return rc;
    }
    return BESS_OK;
}
