// The 64 x 64 output tile on v_mfma_f32_32x32x2_f32 that tucker.hip and relation_query.hip share: 256 threads = 4
// waves of one 32 x 32 MFMA tile each, the reduction staged through LDS in slices of 32 as [k][m] / [k][n] images (a
// fragment read is one ds_read_b32 per lane), odd stride 65 for transposing stores and 68 for direct 16-byte stores.
// gemm_mfma.hip's conventions, restated here for kernels whose operands are gathered or formed on the way to LDS.
#pragma once

#include <atomic>

#include "common.h"

namespace bess {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TK = 32;         // reduction slice
constexpr int TT = 64;         // edge of the output tile
constexpr int LD_T = TT + 1;   // [k][m] image written by transposing stores
constexpr int LD_D = TT + 4;   // [k][m] image written by direct 16-byte stores
constexpr int B_IMG = TK * LD_D;                  // floats of one slice image (either stride)

constexpr int64_t LDS_LIMIT = 160 * 1024;         // per workgroup on gfx950

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// row[c .. c + 3], zeros where the row is not live or the column is at or past c_end.  `row` is a valid row in either
// case.  VEC4 (c_end % 4 == 0, c_end >= 4, 16-byte aligned rows): one unconditional 16-byte load at a clamped address,
// then selects - no branch that would make the loads of a slice wait for one another.
template <bool VEC4>
__device__ __forceinline__ void load4(const float* __restrict__ row, int64_t c, int64_t c_end, bool live, float (&v)[4]) {
    if (VEC4) {
        const float4 t = *reinterpret_cast<const float4*>(row + min(c, c_end - 4));
        live = live && c < c_end;
        v[0] = live ? t.x : 0.f;
        v[1] = live ? t.y : 0.f;
        v[2] = live ? t.z : 0.f;
        v[3] = live ? t.w : 0.f;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = (live && c + i < c_end) ? row[c + i] : 0.f;
    }
}

// One thread's share of a 32 x 64 slice whose rows are the reduction index (contiguous along the tile's 64 columns):
// rows p * 16 + t / 16, columns (t % 16) * 4 .. + 3; stored with one 16-byte store per pass.
__device__ __forceinline__ void store_direct(float* img, const float (&v)[2][4]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int p = 0; p < 2; ++p)
        *reinterpret_cast<float4*>(&img[(p * 16 + (t >> 4)) * LD_D + (t & 15) * 4]) =
            make_float4(v[p][0], v[p][1], v[p][2], v[p][3]);
}
// ... and of a 64 x 32 slice whose rows are the tile's 64 columns (contiguous along the reduction index):
// rows p * 32 + t / 8, reduction entries (t % 8) * 4 .. + 3; stored transposed.
__device__ __forceinline__ void store_transposed(float* img, const float (&v)[2][4]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int i = 0; i < 4; ++i) img[((t & 7) * 4 + i) * LD_T + p * 32 + (t >> 3)] = v[p][i];
}

// Slice (j0 .. j0 + 32) x (n0 .. n0 + 64) of B(j, n) = mat[j, n] (SWAP: mat[n, j]) for one row-major de x de matrix,
// through registers into a [j][n] image.
template <bool SWAP, bool VEC4>
struct MatrixSlice {
    static constexpr int LD = SWAP ? LD_T : LD_D;
    float v[2][4];
    __device__ __forceinline__ void load(const float* __restrict__ mat, int64_t de, int64_t j0, int64_t n0) {
        const int t = threadIdx.x;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            // the matrix's row r and the first of four columns: (j, n ..) as stored, (n, j ..) with exchanged axes
            const int64_t r = SWAP ? n0 + p * 32 + (t >> 3) : j0 + p * 16 + (t >> 4);
            const int64_t c = SWAP ? j0 + (t & 7) * 4 : n0 + (t & 15) * 4;
            load4<VEC4>(mat + min(r, de - 1) * de, c, de, r < de, v[p]);
        }
    }
    __device__ __forceinline__ void store(float* img) const {
        if (SWAP) store_transposed(img, v);
        else store_direct(img, v);
    }
};

// the 16 steps of one slice: acc += A(wm .., j) B(j, wn ..) from the two images; SCALE: A times `rk` on the read.
// Fragments of step kk + 2 are read while the MFMA of step kk issues (two register sets), as in gemm_mfma.hip.
template <int LDA, int LDB, bool SCALE>
__device__ __forceinline__ void mfma_slice(const float* a_img, const float* b_img, f32x16& acc, int wm, int wn, int l31,
                                           int lk, float rk) {
    float a[2], b[2];
    a[0] = a_img[lk * LDA + wm + l31];
    b[0] = b_img[lk * LDB + wn + l31];
#pragma unroll
    for (int kk = 0; kk < TK; kk += 2) {
        const int c = (kk >> 1) & 1;
        if (kk + 2 < TK) {
            a[c ^ 1] = a_img[(kk + 2 + lk) * LDA + wm + l31];
            b[c ^ 1] = b_img[(kk + 2 + lk) * LDB + wn + l31];
        }
        __builtin_amdgcn_sched_barrier(0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(SCALE ? a[c] * rk : a[c], b[c], acc, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// A kernel whose images stay resident may take all of the CU's LDS.  The attribute belongs to a (kernel, device) pair: it is set once for
// every device this process launches on (`done`: one bit per device ordinal, one word per instantiation).
template <typename K>
inline bool reserve_lds(K kernel, std::atomic<uint64_t>& done) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
    const uint64_t bit = 1ull << dev;
    if (done.load(std::memory_order_relaxed) & bit) return true;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            static_cast<int>(LDS_LIMIT)) != hipSuccess)
        return false;
    done.fetch_or(bit, std::memory_order_relaxed);
    return true;
}

__device__ __forceinline__ void zero_acc(f32x16& acc) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
}
// C/D layout of the 32 x 32 MFMA: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
__device__ __forceinline__ int acc_row(int r, int lk) { return (r & 3) + 8 * (r >> 2) + 4 * lk; }

}  // namespace
}  // namespace bess
