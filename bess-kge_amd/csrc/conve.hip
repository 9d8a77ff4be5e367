// ConvE's query network between the stacked image and the FC output, on the CDNA4 matrix cores:
//
//     conv[s, c, i, j] = sum_{ci, u, v} K[c, ci, u, v] x[s, ci, i + u, j + v]        (no bias, no padding, stride 1)
//     A[s, f] = m[s, c] max(a_c conv + b_c, 0),  f = (c Ho + i) Wo + j               (channel affine, ReLU, channel mask)
//     y[s, n] = sum_f A[s, f] Wfc[n, f]                                              (exact fp32, v_mfma_f32_32x32x2_f32)
//
// It is a GEMM [S, F] x [F, d] whose left operand costs Cin kh kw FMAs per element.  That operand exists nowhere: the
// images of a tile's rows sit in LDS and A is formed from them on the way into the MFMA, in the forward and in both
// backward GEMMs - no [S, F] feature map is written in either direction.
//
//   k_conve_fwd        y: 64 x 64 tile, the 64 images resident as a [pixel][row] image (a wave forms 8 reduction
//                      entries of a slice for its lane's row: the pixel address is wave-uniform), Wfc slices through two
//                      transposed LDS buffers; ceil(d / 64) workgroups re-form A for the same rows
//   k_conve_bwd_fc     d_Wfc[n, f] = sum_s dy[s, n] A[s, f]: 64 x 64 tile, reduction over the rows in slices of 32; a
//                      lane owns one f, so its filter taps and pixel offsets are fixed and its reads of x are contiguous
//                      across the lanes - A is re-formed from global memory (x stays in L2)
//   k_conve_bwd_act    one tile of 32 rows, channels in order: G_c = dy Wfc[:, channel block] on the MFMA (dy resident,
//                      128 columns per pass), then on the tile in LDS: z recomputed, G' = m [z > 0] G, this tile's
//                      partials of d_b = sum G', d_a = sum G' conv, d_K = sum G' patch, and d_x in gather form into an
//                      LDS image that is written once at the end.  Partials [tiles][Cout][KK + 2] are summed over the
//                      tile axis in tile order by k_conve_merge
//   k_conve_stats      per-channel sum of conv, then of (conv - mean)^2 (two passes: the second is centred), 8 rows per
//                      workgroup, partials merged in a fixed order by k_conve_merge_stats
//   k_conve_stats_bwd  d_conv = d_mean / N + 2 (conv - mean) d_M2 pushed through the conv: d_x per row, d_K partials
//
// Conventions are mfma_tile.h's.  No atomics anywhere: every output element is written once, by one lane, in a fixed
// order of summation.
#include <atomic>

#include "common.h"
#include "mfma_tile.h"

namespace bess {
namespace {

constexpr int AT = 32;                     // rows of a k_conve_bwd_act tile
constexpr int LD_R = AT + 1;               // ... and the stride of its [index][row] images
constexpr int ACT_COLS = 128;              // columns of G per pass: 4 waves side by side
constexpr int LD_G = ACT_COLS + 4;         // the Wfc slice [k][column], direct 16-byte stores
constexpr int STAT_ROWS = 8;               // rows per workgroup of the statistics kernels
static_assert(ACT_COLS * LD_R == TK * LD_G, "the G tile [column][row] takes the place of the Wfc slice");

struct Geo {
    int Cin, H2, W, Cout, kh, kw, Ho, Wo;
    int HW, P, KK, F, d;  // Ho Wo, Cin H2 W, Cin kh kw, Cout Ho Wo
};

// LDS floats of the three resident-image kernels (the limits of include/besskge_hip.h)
inline int64_t fwd_lds_floats(const Geo& g) {
    return 2 * B_IMG + 2 * TK * LD_T + static_cast<int64_t>(g.Cout) * (g.KK + 2) + static_cast<int64_t>(g.P) * LD_T;
}
inline int64_t act_lds_floats(const Geo& g) {
    return TK * LD_G + (g.KK + 2) * 4 + static_cast<int64_t>(g.Cout) * (g.KK + 2) + ceil_div(g.d, TK) * TK * LD_R +
           2 * static_cast<int64_t>(g.P) * LD_R;
}
inline int64_t stats_lds_floats(const Geo& g) {
    return static_cast<int64_t>(STAT_ROWS) * (2 * g.P + g.HW) + static_cast<int64_t>(g.Cout) * g.KK + g.KK * 4 + 4;
}

// conv[c, i, j] of one row: pixel p of the row is img[p * ld] (ld = 1: the row as stored, else an LDS image's stride);
// Kc = K[c].  One chain of fused multiply-adds in (ci, u, v) order.
__device__ __forceinline__ float conv_at(const float* img, int ld, const float* Kc, const Geo& g, int i, int j) {
    float acc = 0.f;
    int q = 0;
    for (int ci = 0; ci < g.Cin; ++ci)
        for (int u = 0; u < g.kh; ++u) {
            const float* px = img + static_cast<int64_t>((ci * g.H2 + i + u) * g.W + j) * ld;
            for (int v = 0; v < g.kw; ++v, ++q) acc = fmaf(Kc[q], px[v * ld], acc);
        }
    return acc;
}

// The images of rows m0 .. m0 + rows - 1 as img[pixel * ld + row]; rows past S are zeros.
template <bool VEC4>
__device__ __forceinline__ void load_image(float* img, int ld, int rows, const float* __restrict__ x, int64_t ldx,
                                           int64_t m0, int64_t S, int P) {
    const int t = threadIdx.x;
    if (VEC4) {
        const int P4 = P >> 2;
        for (int e = t; e < rows * P4; e += 256) {
            const int r = e / P4, p = (e - r * P4) * 4;
            const bool live = m0 + r < S;
            const float4 v = *reinterpret_cast<const float4*>(x + min(m0 + r, S - 1) * ldx + p);
            img[(p + 0) * ld + r] = live ? v.x : 0.f;
            img[(p + 1) * ld + r] = live ? v.y : 0.f;
            img[(p + 2) * ld + r] = live ? v.z : 0.f;
            img[(p + 3) * ld + r] = live ? v.w : 0.f;
        }
    } else {
        for (int e = t; e < rows * P; e += 256) {
            const int r = e / P, p = e - r * P;
            img[p * ld + r] = m0 + r < S ? x[(m0 + r) * ldx + p] : 0.f;
        }
    }
}

struct QueryArgs {
    const float *x, *K, *a, *b, *m, *Wfc, *dy;  // m may be NULL; dy: the backward kernels
    float* out;                                 // y | d_Wfc | d_x
    float* parts;                               // k_conve_bwd_act: [tiles][Cout][KK + 2]
    int64_t ldx, ldm, ldw, lddy, ldo, S;
    Geo g;
};

// grid (ceil(d / 64), ceil(S / 64)).
// LDS: [2][32 x 68] Wfc slices | [2][32 x 65] A slices | K | a | b | [P][65] image of the 64 rows.
template <bool VEC4>
__global__ __launch_bounds__(256) void k_conve_fwd(QueryArgs A) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const Geo& g = A.g;
    float* const Bs = lds;
    float* const As = Bs + 2 * B_IMG;
    float* const Ks = As + 2 * TK * LD_T;
    float* const ab = Ks + g.Cout * g.KK;
    float* const Xs = ab + 2 * g.Cout;
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int l31 = lane & 31, lk = lane >> 5;
    const int64_t m0 = static_cast<int64_t>(blockIdx.y) * TT, n0 = static_cast<int64_t>(blockIdx.x) * TT;
    const int64_t S = A.S, d = g.d, F = g.F;

    load_image<VEC4>(Xs, LD_T, TT, A.x, A.ldx, m0, S, g.P);
    for (int e = t; e < g.Cout * g.KK; e += 256) Ks[e] = A.K[e];
    for (int e = t; e < g.Cout; e += 256) {
        ab[e] = A.a[e];
        ab[g.Cout + e] = A.b[e];
    }
    float wv[2][4];
    auto load_w = [&](int64_t f0) {  // rows n0 .. + 63 of Wfc, reduction entries f0 .. + 31
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int64_t n = n0 + p * 32 + (t >> 3);
            load4<VEC4>(A.Wfc + min(n, d - 1) * A.ldw, f0 + (t & 7) * 4, F, n < d, wv[p]);
        }
    };
    // the lane's row of the mask (clamped: the products of rows past S are never stored)
    const float* mrow = A.m ? A.m + min(m0 + lane, S - 1) * A.ldm : nullptr;
    auto form = [&](int f0, float* img) {  // A[rows, f0 + wave * 8 .. + 7] as [k][m]: f is wave-uniform
        for (int r = 0; r < 8; ++r) {
            const int k = wave * 8 + r, f = f0 + k;
            float v = 0.f;
            if (f < g.F) {
                const int c = f / g.HW, pos = f - c * g.HW, i = pos / g.Wo, j = pos - i * g.Wo;
                const float conv = conv_at(Xs + lane, LD_T, Ks + c * g.KK, g, i, j);
                v = fmaxf(fmaf(ab[c], conv, ab[g.Cout + c]), 0.f);
                if (mrow) v *= mrow[c];
            }
            img[k * LD_T + lane] = v;
        }
    };
    load_w(0);
    __syncthreads();  // the image, K, a, b
    form(0, As);
    store_transposed(Bs, wv);
    f32x16 acc;
    zero_acc(acc);
    __syncthreads();

    const int n_slice = (g.F + TK - 1) / TK;
    for (int s = 0; s < n_slice; ++s) {
        const int cur = s & 1;
        const bool more = s + 1 < n_slice;
        if (more) {  // the next slice: Wfc loads issued, A formed into the other buffer, ahead of this slice's MFMAs
            load_w(static_cast<int64_t>(s + 1) * TK);
            form((s + 1) * TK, As + (cur ^ 1) * TK * LD_T);
        }
        mfma_slice<LD_T, LD_T, false>(As + cur * TK * LD_T, Bs + cur * B_IMG, acc, wm, wn, l31, lk, 1.f);
        if (more) store_transposed(Bs + (cur ^ 1) * B_IMG, wv);
        __syncthreads();
    }
    const int64_t col = n0 + wn + l31;
    if (col < d) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t row = m0 + wm + acc_row(r, lk);
            if (row < S) A.out[row * A.ldo + col] = acc[r];
        }
    }
}

// d_Wfc[n0 .., f0 ..] = sum_s dy[s, n] A[s, f].  grid (ceil(F / 64), ceil(d / 64)).  Both operands are "reduction index
// = row" images; lane l of every wave forms A[rows, f0 + l] from x as stored (VEC4: the 16-byte loads of dy).
template <bool VEC4>
__global__ __launch_bounds__(256) void k_conve_bwd_fc(QueryArgs A) {
    __shared__ __attribute__((aligned(16))) float Ds[2][B_IMG];
    __shared__ __attribute__((aligned(16))) float As[2][B_IMG];
    const Geo& g = A.g;
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int l31 = lane & 31, lk = lane >> 5;
    const int64_t f0 = static_cast<int64_t>(blockIdx.x) * TT, n0 = static_cast<int64_t>(blockIdx.y) * TT;
    const int64_t S = A.S, d = g.d;
    // the lane's column of A: its channel, output pixel, filter and affine never change
    const bool live_f = f0 + lane < g.F;
    const int f = static_cast<int>(min(f0 + lane, static_cast<int64_t>(g.F) - 1));
    const int c = f / g.HW, pos = f - c * g.HW, i = pos / g.Wo, j = pos - i * g.Wo;
    const float* Kc = A.K + c * g.KK;
    const float ac = A.a[c], bc = A.b[c];
    float dv[2][4];
    auto load_dy = [&](int64_t ms) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int64_t m = ms + p * 16 + (t >> 4);
            load4<VEC4>(A.dy + min(m, S - 1) * A.lddy, n0 + (t & 15) * 4, d, m < S, dv[p]);
        }
    };
    auto form = [&](int64_t ms, float* img) {  // A[ms + wave * 8 .. + 7, f] as [k = row][f]
        for (int r = 0; r < 8; ++r) {
            const int k = wave * 8 + r;
            const int64_t m = min(ms + k, S - 1);
            const float conv = conv_at(A.x + m * A.ldx, 1, Kc, g, i, j);
            float v = fmaxf(fmaf(ac, conv, bc), 0.f);
            if (A.m) v *= A.m[m * A.ldm + c];
            img[k * LD_D + lane] = (live_f && ms + k < S) ? v : 0.f;
        }
    };
    load_dy(0);
    form(0, As[0]);
    store_direct(Ds[0], dv);
    f32x16 acc;
    zero_acc(acc);
    __syncthreads();
    const int n_slice = static_cast<int>((S + TK - 1) / TK);
    for (int s = 0; s < n_slice; ++s) {
        const int cur = s & 1;
        const bool more = s + 1 < n_slice;
        if (more) {
            load_dy(static_cast<int64_t>(s + 1) * TK);
            form(static_cast<int64_t>(s + 1) * TK, As[cur ^ 1]);
        }
        mfma_slice<LD_D, LD_D, false>(Ds[cur], As[cur], acc, wm, wn, l31, lk, 1.f);
        if (more) store_direct(Ds[cur ^ 1], dv);
        __syncthreads();
    }
    const int64_t col = f0 + wn + l31;
    if (col < g.F) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t row = n0 + wm + acc_row(r, lk);
            if (row < d) A.out[row * A.ldo + col] = acc[r];
        }
    }
}

// grid ceil(S / 32).  LDS: [32 x 132] Wfc slice, then the G tile [128][33] in its place | [KK + 2][4] wave partials |
// K | a | b | [ceil(d / 32) * 32][33] dy | [P][33] image | [P][33] d_x.
// VEC4: the 16-byte loads of x and of Wfc (Ho Wo % 4 == 0: every channel block starts on a 16-byte boundary).
template <bool VEC4>
__global__ __launch_bounds__(256) void k_conve_bwd_act(QueryArgs A) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const Geo& g = A.g;
    const int KK = g.KK, per = KK + 2;
    const int dpad = (g.d + TK - 1) / TK * TK;
    float* const Bs = lds;  // and Gs
    float* const red = Bs + TK * LD_G;
    float* const Ks = red + per * 4;
    float* const ab = Ks + g.Cout * KK;
    float* const dYs = ab + 2 * g.Cout;
    float* const Xs = dYs + dpad * LD_R;
    float* const dXs = Xs + g.P * LD_R;
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int l31 = lane & 31, lk = lane >> 5;
    const int row = t & 31, grp = t >> 5;  // the element work: a thread keeps one row, eight groups share the columns
    const int64_t m0 = static_cast<int64_t>(blockIdx.x) * AT;
    const int64_t S = A.S, d = g.d;

    load_image<VEC4>(Xs, LD_R, AT, A.x, A.ldx, m0, S, g.P);
    for (int e = t; e < g.P * LD_R; e += 256) dXs[e] = 0.f;
    for (int e = t; e < g.Cout * KK; e += 256) Ks[e] = A.K[e];
    for (int e = t; e < g.Cout; e += 256) {
        ab[e] = A.a[e];
        ab[g.Cout + e] = A.b[e];
    }
    for (int e = t; e < AT * dpad; e += 256) {  // dy as [k][row]; zeros past S and past d
        const int r = e / dpad, k = e - r * dpad;
        dYs[k * LD_R + r] = (m0 + r < S && k < d) ? A.dy[(m0 + r) * A.lddy + k] : 0.f;
    }
    __syncthreads();
    const bool live_row = m0 + row < S;
    const float* mrow = A.m ? A.m + min(m0 + row, S - 1) * A.ldm : nullptr;
    const int n_ct = (g.HW + ACT_COLS - 1) / ACT_COLS, n_ks = dpad / TK;

    for (int c = 0; c < g.Cout; ++c) {
        for (int e = t; e < per * 4; e += 256) red[e] = 0.f;
        const float mval = live_row ? (mrow ? mrow[c] : 1.f) : 0.f;
        const float ac = ab[c], bc = ab[g.Cout + c];
        const float* Kc = Ks + c * KK;
        float da = 0.f, db = 0.f;
        for (int ct = 0; ct < n_ct; ++ct) {
            // G[rows, ct * 128 .. + 127 of channel c] = dy Wfc[:, that block]: reduction over d
            const int64_t fb = static_cast<int64_t>(c) * g.HW + ct * ACT_COLS;
            f32x16 acc;
            zero_acc(acc);
            for (int ks = 0; ks < n_ks; ++ks) {
                float wv[4][4];
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const int64_t n = ks * TK + p * 8 + (t >> 5);
                    load4<VEC4>(A.Wfc + min(n, d - 1) * A.ldw, fb + (t & 31) * 4, g.F, n < d, wv[p]);
                }
                __syncthreads();  // the slice (or the G tile) before this one has been read
#pragma unroll
                for (int p = 0; p < 4; ++p)
                    *reinterpret_cast<float4*>(&Bs[(p * 8 + (t >> 5)) * LD_G + (t & 31) * 4]) =
                        make_float4(wv[p][0], wv[p][1], wv[p][2], wv[p][3]);
                __syncthreads();
                mfma_slice<LD_R, LD_G, false>(dYs + ks * TK * LD_R, Bs, acc, 0, wave * 32, l31, lk, 1.f);
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 16; ++r) Bs[(wave * 32 + l31) * LD_R + acc_row(r, lk)] = acc[r];
            __syncthreads();
            float* const Gs = Bs;
            // the thread's 16 columns: G' = m [z > 0] G in place (zeros past the channel's end), d_a, d_b
            int base[16];  // i W + j of the column's output pixel, -1 past the end
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int col = grp + 8 * e, pos = ct * ACT_COLS + col;
                float gv = 0.f;
                base[e] = -1;
                if (pos < g.HW) {
                    const int i = pos / g.Wo, j = pos - i * g.Wo;
                    base[e] = i * g.W + j;
                    const float conv = conv_at(Xs + row, LD_R, Kc, g, i, j);
                    gv = fmaf(ac, conv, bc) > 0.f ? Gs[col * LD_R + row] * mval : 0.f;
                    db += gv;
                    da = fmaf(gv, conv, da);
                }
                Gs[col * LD_R + row] = gv;
            }
            // d_K: per tap, the thread's columns, then the wave; lane 0 keeps the wave's running sum
            int q = 0;
            for (int ci = 0; ci < g.Cin; ++ci)
                for (int u = 0; u < g.kh; ++u)
                    for (int v = 0; v < g.kw; ++v, ++q) {
                        const int off = (ci * g.H2 + u) * g.W + v;
                        float part = 0.f;
#pragma unroll
                        for (int e = 0; e < 16; ++e)
                            if (base[e] >= 0) part = fmaf(Gs[(grp + 8 * e) * LD_R + row], Xs[(off + base[e]) * LD_R + row], part);
                        part = wave_allreduce_sum(part);
                        if (lane == 0) red[q * 4 + wave] += part;
                    }
            __syncthreads();  // G' of every column
            // d_x in gather form: the pixels this block of output pixels touches, each owned by one thread
            const int i_lo = ct * ACT_COLS / g.Wo, i_hi = min(g.HW - 1, ct * ACT_COLS + ACT_COLS - 1) / g.Wo;
            const int npx = (i_hi - i_lo + g.kh) * g.W;
            for (int e = grp; e < g.Cin * npx; e += 8) {
                const int ci = e / npx, rem = e - ci * npx, y = i_lo + rem / g.W, xx = rem % g.W;
                float sum = 0.f;
                for (int u = 0; u < g.kh; ++u) {
                    const int i = y - u;
                    if (i < i_lo || i > i_hi) continue;
                    for (int v = 0; v < g.kw; ++v) {
                        const int j = xx - v, p = i * g.Wo + j - ct * ACT_COLS;
                        if (j < 0 || j >= g.Wo || p < 0 || p >= ACT_COLS) continue;
                        sum = fmaf(Kc[(ci * g.kh + u) * g.kw + v], Gs[p * LD_R + row], sum);
                    }
                }
                dXs[((ci * g.H2 + y) * g.W + xx) * LD_R + row] += ac * sum;
            }
        }
        da = wave_allreduce_sum(da);
        db = wave_allreduce_sum(db);
        if (lane == 0) {
            red[KK * 4 + wave] = da;
            red[(KK + 1) * 4 + wave] = db;
        }
        __syncthreads();
        for (int e = t; e < per; e += 256)
            A.parts[(static_cast<int64_t>(blockIdx.x) * g.Cout + c) * per + e] =
                ((red[e * 4] + red[e * 4 + 1]) + red[e * 4 + 2]) + red[e * 4 + 3];
        __syncthreads();
    }
    if (A.out) {
        for (int e = t; e < AT * g.P; e += 256) {
            const int r = e / g.P, p = e - r * g.P;
            if (m0 + r < S) A.out[(m0 + r) * A.ldo + p] = dXs[p * LD_R + r];
        }
    }
}

// out = sum over the tile axis of parts [tiles][Cout][per], in tile order: entries 0 .. KK - 1 of a channel to d_K
// (times a_c if given), entry KK to d_a, KK + 1 to d_b; a NULL target is skipped.
__global__ __launch_bounds__(256) void k_conve_merge(const float* __restrict__ parts, int64_t tiles, int Cout, int KK,
                                                     int per, const float* __restrict__ a, float* __restrict__ d_K,
                                                     float* __restrict__ d_a, float* __restrict__ d_b) {
    const int n = Cout * per;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < n; idx += 256 * gridDim.x) {
        float acc = 0.f;
        for (int64_t p = 0; p < tiles; ++p) acc += parts[p * n + idx];
        const int c = idx / per, j = idx - c * per;
        if (j < KK) {
            if (d_K) d_K[c * KK + j] = a ? a[c] * acc : acc;
        } else if (j == KK) {
            if (d_a) d_a[c] = acc;
        } else if (d_b) {
            d_b[c] = acc;
        }
    }
}

struct StatsArgs {
    const float *x, *K, *mean, *d_mean, *d_M2;
    float *parts, *d_x;
    int64_t ldx, ld_dx, S;
    float inv_n;
    Geo g;
};

// parts[workgroup][c] = sum over the workgroup's 8 rows of conv (CENTRED: of (conv - mean_c)^2).  grid ceil(S / 8).
// LDS: the rows as stored [8][P] | K | 4 wave partials.
template <bool CENTRED>
__global__ __launch_bounds__(256) void k_conve_stats(StatsArgs A) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const Geo& g = A.g;
    float* const Xs = lds;
    float* const Ks = Xs + STAT_ROWS * g.P;
    float* const red = Ks + g.Cout * g.KK;
    const int t = threadIdx.x, wave = t >> 6;
    const int64_t m0 = static_cast<int64_t>(blockIdx.x) * STAT_ROWS;
    const int rows = static_cast<int>(min(static_cast<int64_t>(STAT_ROWS), A.S - m0));
    for (int e = t; e < rows * g.P; e += 256) Xs[e] = A.x[(m0 + e / g.P) * A.ldx + e % g.P];
    for (int e = t; e < g.Cout * g.KK; e += 256) Ks[e] = A.K[e];
    __syncthreads();
    for (int c = 0; c < g.Cout; ++c) {
        const float mean = CENTRED ? A.mean[c] : 0.f;
        float acc = 0.f;
        for (int e = t; e < rows * g.HW; e += 256) {
            const int r = e / g.HW, pos = e - r * g.HW, i = pos / g.Wo, j = pos - i * g.Wo;
            const float v = conv_at(Xs + r * g.P, 1, Ks + c * g.KK, g, i, j) - mean;
            acc = CENTRED ? fmaf(v, v, acc) : acc + v;
        }
        acc = wave_allreduce_sum(acc);
        if ((t & 63) == 0) red[wave] = acc;
        __syncthreads();
        if (t == 0) A.parts[static_cast<int64_t>(blockIdx.x) * g.Cout + c] = ((red[0] + red[1]) + red[2]) + red[3];
        __syncthreads();
    }
}

// out[c] = scale * sum_p parts[p][c]: lane l adds p = l, l + 64, ... in order, then the wave's butterfly.  grid Cout.
__global__ __launch_bounds__(64) void k_conve_merge_stats(const float* __restrict__ parts, int64_t n_part, int Cout,
                                                          float scale, float* __restrict__ out) {
    float acc = 0.f;
    for (int64_t p = threadIdx.x; p < n_part; p += 64) acc += parts[p * Cout + blockIdx.x];
    acc = wave_allreduce_sum(acc);
    if (threadIdx.x == 0) out[blockIdx.x] = acc * scale;
}

// d_conv[s, c, i, j] = d_mean_c / N + 2 (conv - mean_c) d_M2_c through the conv.  grid ceil(S / 8).
// LDS: [8][P] rows | [8][P] d_x | [8][Ho Wo] d_conv of one channel | K | [KK][4] wave partials.
__global__ __launch_bounds__(256) void k_conve_stats_bwd(StatsArgs A) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const Geo& g = A.g;
    const int KK = g.KK;
    float* const Xs = lds;
    float* const dXs = Xs + STAT_ROWS * g.P;
    float* const Dc = dXs + STAT_ROWS * g.P;
    float* const Ks = Dc + STAT_ROWS * g.HW;
    float* const red = Ks + g.Cout * KK;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t m0 = static_cast<int64_t>(blockIdx.x) * STAT_ROWS;
    const int rows = static_cast<int>(min(static_cast<int64_t>(STAT_ROWS), A.S - m0));
    for (int e = t; e < rows * g.P; e += 256) {
        Xs[e] = A.x[(m0 + e / g.P) * A.ldx + e % g.P];
        dXs[e] = 0.f;
    }
    for (int e = t; e < g.Cout * KK; e += 256) Ks[e] = A.K[e];
    __syncthreads();
    for (int c = 0; c < g.Cout; ++c) {
        const float* Kc = Ks + c * KK;
        const float shift = A.d_mean[c] * A.inv_n, mean = A.mean[c], twice = 2.f * A.d_M2[c];
        for (int e = t; e < rows * g.HW; e += 256) {
            const int r = e / g.HW, pos = e - r * g.HW, i = pos / g.Wo, j = pos - i * g.Wo;
            Dc[e] = fmaf(conv_at(Xs + r * g.P, 1, Kc, g, i, j) - mean, twice, shift);
        }
        __syncthreads();
        int q = 0;
        for (int ci = 0; ci < g.Cin; ++ci)
            for (int u = 0; u < g.kh; ++u)
                for (int v = 0; v < g.kw; ++v, ++q) {
                    float part = 0.f;
                    for (int e = t; e < rows * g.HW; e += 256) {
                        const int r = e / g.HW, pos = e - r * g.HW, i = pos / g.Wo, j = pos - i * g.Wo;
                        part = fmaf(Dc[e], Xs[r * g.P + (ci * g.H2 + i + u) * g.W + j + v], part);
                    }
                    part = wave_allreduce_sum(part);
                    if (lane == 0) red[q * 4 + wave] = part;
                }
        for (int e = t; e < rows * g.P; e += 256) {  // gather: the thread owns the pixel in every channel
            const int r = e / g.P, p = e - r * g.P, ci = p / (g.H2 * g.W), y = p / g.W - ci * g.H2, xx = p % g.W;
            float sum = 0.f;
            for (int u = 0; u < g.kh; ++u) {
                const int i = y - u;
                if (i < 0 || i >= g.Ho) continue;
                for (int v = 0; v < g.kw; ++v) {
                    const int j = xx - v;
                    if (j < 0 || j >= g.Wo) continue;
                    sum = fmaf(Kc[(ci * g.kh + u) * g.kw + v], Dc[r * g.HW + i * g.Wo + j], sum);
                }
            }
            dXs[e] += sum;
        }
        __syncthreads();
        for (int e = t; e < KK; e += 256)
            A.parts[(static_cast<int64_t>(blockIdx.x) * g.Cout + c) * KK + e] =
                ((red[e * 4] + red[e * 4 + 1]) + red[e * 4 + 2]) + red[e * 4 + 3];
    }
    if (A.d_x)
        for (int e = t; e < rows * g.P; e += 256) A.d_x[(m0 + e / g.P) * A.ld_dx + e % g.P] = dXs[e];
}

// ---- host ---------------------------------------------------------------------------------------------------
int make_geo(const char* who, int64_t S, int64_t Cin, int64_t H2, int64_t W, int64_t Cout, int64_t kh, int64_t kw,
             int64_t d, bool query, Geo* g) {
    BESS_REQUIRE(S >= 0 && Cin >= 1 && H2 >= 1 && W >= 1 && Cout >= 1 && kh >= 1 && kw >= 1 && d >= 1,
                 "%s: S >= 0 and every other size >= 1", who);
    BESS_REQUIRE(kh <= H2 && kw <= W, "%s: the %lld x %lld filter does not fit the %lld x %lld image", who,
                 static_cast<long long>(kh), static_cast<long long>(kw), static_cast<long long>(H2), static_cast<long long>(W));
    const int64_t Ho = H2 - kh + 1, Wo = W - kw + 1;
    BESS_REQUIRE(S < (1ll << 22) && Cin * H2 * W < (1 << 20) && Cout < (1 << 20) && d < (1 << 20) &&
                     Cout * Ho * Wo < (1ll << 30),
                 "%s: S < 2^22, image, channels and d < 2^20, features < 2^30", who);
    *g = Geo{static_cast<int>(Cin), static_cast<int>(H2), static_cast<int>(W), static_cast<int>(Cout), static_cast<int>(kh),
             static_cast<int>(kw), static_cast<int>(Ho), static_cast<int>(Wo), static_cast<int>(Ho * Wo),
             static_cast<int>(Cin * H2 * W), static_cast<int>(Cin * kh * kw), static_cast<int>(Cout * Ho * Wo),
             static_cast<int>(d)};
    const int64_t need = query ? (fwd_lds_floats(*g) > act_lds_floats(*g) ? fwd_lds_floats(*g) : act_lds_floats(*g))
                               : stats_lds_floats(*g);
    if (need * 4 > LDS_LIMIT)
        return fail(BESS_EUNSUPPORTED, "%s: the images of a row tile and the filter need %lld bytes of LDS, above %lld", who,
                    static_cast<long long>(need * 4), static_cast<long long>(LDS_LIMIT));
    return BESS_OK;
}

inline int64_t act_parts_bytes(int64_t S, const Geo& g) { return ceil_div(S, AT) * g.Cout * (g.KK + 2) * 4; }
inline int64_t stats_parts_bytes(int64_t S, const Geo& g) { return ceil_div(S, STAT_ROWS) * g.Cout * (g.KK > 1 ? g.KK : 1) * 4; }

template <typename K, typename ARGS>
int launch_resident(const char* what, K kernel, std::atomic<uint64_t>& done, dim3 grid, int64_t lds_floats, const ARGS& A,
                    hipStream_t st) {
    BESS_REQUIRE(reserve_lds(kernel, done), "%s: cannot reserve %lld bytes of LDS", what, static_cast<long long>(LDS_LIMIT));
    kernel<<<grid, 256, static_cast<size_t>(lds_floats * 4), st>>>(A);
    return check_launch(what);
}

bool x_vec4(const QueryArgs& A) { return A.g.P % 4 == 0 && A.ldx % 4 == 0 && aligned16(A.x); }
bool w_vec4(const QueryArgs& A, int64_t block) { return block % 4 == 0 && A.ldw % 4 == 0 && aligned16(A.Wfc); }

int merge_parts(const float* parts, int64_t tiles, const Geo& g, int per, const float* a, float* d_K, float* d_a,
                float* d_b, hipStream_t st) {
    const unsigned blocks = static_cast<unsigned>(ceil_div(static_cast<int64_t>(g.Cout) * per, 256));
    k_conve_merge<<<blocks, 256, 0, st>>>(parts, tiles, g.Cout, g.KK, per, a, d_K, d_a, d_b);
    return check_launch("conve_merge");
}

}  // namespace
}  // namespace bess

using namespace bess;

extern "C" int bess_conve_query_workspace(int64_t S, int64_t Cin, int64_t H2, int64_t W, int64_t Cout, int64_t kh,
                                          int64_t kw, int64_t d, int64_t* bytes) {
    BESS_REQUIRE(bytes, "conve_query_workspace: NULL pointer");
    Geo g;
    if (int rc = make_geo("conve_query_workspace", S, Cin, H2, W, Cout, kh, kw, d, true, &g)) return rc;
    *bytes = act_parts_bytes(S, g);
    return BESS_OK;
}

extern "C" int bess_conve_query_fwd(const float* x, int64_t ldx, const float* K, const float* a, const float* b,
                                    const float* m, int64_t ldm, const float* Wfc, int64_t ldw, float* y, int64_t ldy,
                                    int64_t S, int64_t Cin, int64_t H2, int64_t W, int64_t Cout, int64_t kh, int64_t kw,
                                    int64_t d, void* stream) {
    Geo g;
    if (int rc = make_geo("conve_query_fwd", S, Cin, H2, W, Cout, kh, kw, d, true, &g)) return rc;
    BESS_REQUIRE(ldx >= g.P && ldw >= g.F && ldy >= d && (!m || ldm >= Cout), "conve_query_fwd: bad leading dimension");
    if (S == 0) return BESS_OK;
    BESS_REQUIRE(x && K && a && b && Wfc && y, "conve_query_fwd: NULL pointer");
    QueryArgs A{x, K, a, b, m, Wfc, nullptr, y, nullptr, ldx, ldm, ldw, 0, ldy, S, g};
    const dim3 grid(static_cast<unsigned>(ceil_div(d, TT)), static_cast<unsigned>(ceil_div(S, TT)));
    int rc = BESS_OK;
    with_flag(x_vec4(A) && w_vec4(A, g.F), [&](auto v4) {
        static std::atomic<uint64_t> done{0};
        rc = launch_resident("conve_fwd", k_conve_fwd<decltype(v4)::value>, done, grid, fwd_lds_floats(g), A, as_stream(stream));
    });
    return rc;
}

extern "C" int bess_conve_query_bwd(const float* x, int64_t ldx, const float* K, const float* a, const float* b,
                                    const float* m, int64_t ldm, const float* Wfc, int64_t ldw, const float* dy,
                                    int64_t lddy, float* d_Wfc, int64_t ld_dw, float* d_x, int64_t ld_dx, float* d_K,
                                    float* d_a, float* d_b, int64_t S, int64_t Cin, int64_t H2, int64_t W, int64_t Cout,
                                    int64_t kh, int64_t kw, int64_t d, void* workspace, int64_t workspace_bytes,
                                    void* stream) {
    Geo g;
    if (int rc = make_geo("conve_query_bwd", S, Cin, H2, W, Cout, kh, kw, d, true, &g)) return rc;
    BESS_REQUIRE(ldx >= g.P && ldw >= g.F && lddy >= d && (!m || ldm >= Cout) && (!d_Wfc || ld_dw >= g.F) &&
                     (!d_x || ld_dx >= g.P) && workspace_bytes >= 0,
                 "conve_query_bwd: bad leading dimension");
    hipStream_t st = as_stream(stream);
    if (S == 0) {  // the parameter gradients of an empty batch are zero; there are no rows
        hipError_t e = hipSuccess;
        if (d_Wfc)
            for (int64_t n = 0; n < d && e == hipSuccess; ++n) e = fill_words_async(d_Wfc + n * ld_dw, 0u, g.F, st);
        if (d_K && e == hipSuccess) e = fill_words_async(d_K, 0u, static_cast<int64_t>(g.Cout) * g.KK, st);
        if (d_a && e == hipSuccess) e = fill_words_async(d_a, 0u, g.Cout, st);
        if (d_b && e == hipSuccess) e = fill_words_async(d_b, 0u, g.Cout, st);
        return e == hipSuccess ? BESS_OK : check_launch("conve_query_bwd: fill");
    }
    BESS_REQUIRE(x && K && a && b && Wfc && dy, "conve_query_bwd: NULL pointer");
    QueryArgs A{x, K, a, b, m, Wfc, dy, nullptr, nullptr, ldx, ldm, ldw, lddy, 0, S, g};
    if (d_Wfc) {
        A.out = d_Wfc;
        A.ldo = ld_dw;
        const dim3 grid(static_cast<unsigned>(ceil_div(g.F, TT)), static_cast<unsigned>(ceil_div(d, TT)));
        with_flag(d % 4 == 0 && lddy % 4 == 0 && aligned16(dy),
                  [&](auto v4) { k_conve_bwd_fc<decltype(v4)::value><<<grid, 256, 0, st>>>(A); });
        if (int rc = check_launch("conve_bwd_fc")) return rc;
    }
    if (d_x || d_K || d_a || d_b) {
        BESS_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= act_parts_bytes(S, g),
                     "conve_query_bwd: workspace too small (bess_conve_query_workspace) or misaligned");
        A.out = d_x;
        A.ldo = ld_dx;
        A.parts = static_cast<float*>(workspace);
        const int64_t tiles = ceil_div(S, AT);
        int rc = BESS_OK;
        with_flag(x_vec4(A) && w_vec4(A, g.HW), [&](auto v4) {
            static std::atomic<uint64_t> done{0};
            rc = launch_resident("conve_bwd_act", k_conve_bwd_act<decltype(v4)::value>, done,
                                 dim3(static_cast<unsigned>(tiles)), act_lds_floats(g), A, st);
        });
        if (rc) return rc;
        if (d_K || d_a || d_b)
            if (int rc2 = merge_parts(A.parts, tiles, g, g.KK + 2, a, d_K, d_a, d_b, st)) return rc2;
    }
    return BESS_OK;
}

extern "C" int bess_conve_stats_workspace(int64_t S, int64_t Cin, int64_t H2, int64_t W, int64_t Cout, int64_t kh,
                                          int64_t kw, int64_t* bytes) {
    BESS_REQUIRE(bytes, "conve_stats_workspace: NULL pointer");
    Geo g;
    if (int rc = make_geo("conve_stats_workspace", S, Cin, H2, W, Cout, kh, kw, 1, false, &g)) return rc;
    *bytes = stats_parts_bytes(S, g);
    return BESS_OK;
}

extern "C" int bess_conve_stats_fwd(const float* x, int64_t ldx, const float* K, float* mean, float* M2, int64_t S,
                                    int64_t Cin, int64_t H2, int64_t W, int64_t Cout, int64_t kh, int64_t kw,
                                    void* workspace, int64_t workspace_bytes, void* stream) {
    Geo g;
    if (int rc = make_geo("conve_stats_fwd", S, Cin, H2, W, Cout, kh, kw, 1, false, &g)) return rc;
    BESS_REQUIRE(S >= 1, "conve_stats_fwd: statistics of an empty batch");
    BESS_REQUIRE(x && K && mean && M2 && ldx >= g.P, "conve_stats_fwd: NULL pointer or bad leading dimension");
    BESS_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= stats_parts_bytes(S, g),
                 "conve_stats_fwd: workspace too small (bess_conve_stats_workspace) or misaligned");
    hipStream_t st = as_stream(stream);
    StatsArgs A{x, K, mean, nullptr, nullptr, static_cast<float*>(workspace), nullptr, ldx, 0, S, 0.f, g};
    const unsigned blocks = static_cast<unsigned>(ceil_div(S, STAT_ROWS));
    const size_t lds = static_cast<size_t>(stats_lds_floats(g) * 4);
    const float inv_n = static_cast<float>(1.0 / (static_cast<double>(S) * g.HW));
    static std::atomic<uint64_t> done0{0}, done1{0};
    BESS_REQUIRE(reserve_lds(k_conve_stats<false>, done0) && reserve_lds(k_conve_stats<true>, done1),
                 "conve_stats_fwd: cannot reserve LDS");
    k_conve_stats<false><<<blocks, 256, lds, st>>>(A);
    k_conve_merge_stats<<<static_cast<unsigned>(g.Cout), 64, 0, st>>>(A.parts, blocks, g.Cout, inv_n, mean);
    k_conve_stats<true><<<blocks, 256, lds, st>>>(A);
    k_conve_merge_stats<<<static_cast<unsigned>(g.Cout), 64, 0, st>>>(A.parts, blocks, g.Cout, 1.f, M2);
    return check_launch("conve_stats");
}

extern "C" int bess_conve_stats_bwd(const float* x, int64_t ldx, const float* K, const float* mean, const float* d_mean,
                                    const float* d_M2, float* d_x, int64_t ld_dx, float* d_K, int64_t S, int64_t Cin,
                                    int64_t H2, int64_t W, int64_t Cout, int64_t kh, int64_t kw, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
    Geo g;
    if (int rc = make_geo("conve_stats_bwd", S, Cin, H2, W, Cout, kh, kw, 1, false, &g)) return rc;
    BESS_REQUIRE(ldx >= g.P && (!d_x || ld_dx >= g.P), "conve_stats_bwd: bad leading dimension");
    hipStream_t st = as_stream(stream);
    if (S == 0) {
        if (d_K && hipSuccess != fill_words_async(d_K, 0u, static_cast<int64_t>(g.Cout) * g.KK, st))
            return check_launch("conve_stats_bwd: fill");
        return BESS_OK;
    }
    BESS_REQUIRE(x && K && mean && d_mean && d_M2, "conve_stats_bwd: NULL pointer");
    if (!d_x && !d_K) return BESS_OK;
    BESS_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= stats_parts_bytes(S, g),
                 "conve_stats_bwd: workspace too small (bess_conve_stats_workspace) or misaligned");
    const float inv_n = static_cast<float>(1.0 / (static_cast<double>(S) * g.HW));
    StatsArgs A{x, K, mean, d_mean, d_M2, static_cast<float*>(workspace), d_x, ldx, ld_dx, S, inv_n, g};
    const int64_t blocks = ceil_div(S, STAT_ROWS);
    static std::atomic<uint64_t> done{0};
    if (int rc = launch_resident("conve_stats_bwd", k_conve_stats_bwd, done, dim3(static_cast<unsigned>(blocks)),
                                 stats_lds_floats(g), A, st))
        return rc;
    if (d_K) return merge_parts(A.parts, blocks, g, g.KK, nullptr, d_K, nullptr, nullptr, st);
    return BESS_OK;
}
