// HAKE negative scoring (Zhang et al. 2020, "Learning Hierarchy-Aware Knowledge Graph Embeddings").
//
// An entity row is [phase | modulus] (2 x d), a relation row [phase | modulus | bias] (3 x d).  With
// b' = max(min(b, 1), -|r_m|):
//
//     score(h, r, t) = -( l_m || h_m (|r_m| + b') - t_m (1 - b') ||_2 + l_p || sin((h_p + r_p - t_p) / 2) ||_1 )
//
// (phases enter multiplied by phase_scale).  For a query (kept entity + relation) and a candidate e = [c_p | c_m]
// the query matrix is [n_query, 3 d] = [U | R | Q_p]:
//
//     score = -( || U c_m + R ||_2 + l_p || sin((Q_p - phase_scale c_p) / 2) ||_1 )
//
// l_m >= 0 is folded into U and R (the norm is homogeneous); relation-side work is query-only and done over S rows
// by the host side.  desc.width = 2 d, desc.rel_width = 3 d, desc.reserved[1] / [2] = the float bits of l_p and
// phase_scale, desc.reserved[0] = flag bits (BESS_FLAG_FP32_MATH: shared candidates through the row form).
//
// Two forms.
//   Row form (per-triple negatives forward and backward, their segment gradient, and shared candidates when asked
//   for or when the shared backward is given no workspace):
//     the mapping of neg_pertriple.hip / boxe.hip - a 16-lane DPP row streams one candidate row, the query's three
//     vectors stay in registers.  Per element: fma + fma for the modulus; fma, mul, v_sin_f32, abs-add for the phase.
//     The hardware sine takes revolutions; the phase difference is formed first and scaled by 1 / (4 pi) after, so
//     that equal phases give an exact zero (and the gradient 0 of the kink convention).
//   Tile form (shared candidates: store, counting epilogue, pairs; the backward's two kernels further down): 64 x 64 outputs per workgroup, 4 x 4
//     per thread, K-slices of 16 through LDS.  The inner loop holds no transcendental:
//         |sin((a - b) / 2)| = |sin(a/2) cos(b/2) - cos(a/2) sin(b/2)|
//     and the stage that writes a K-slice to LDS writes l_p sin(a/2), l_p cos(a/2) of the query phases and cos(b/2),
//     -sin(b/2) of the candidate phases: two transcendentals per staged element, each used 64 times.  Per element
//     pair: fma, fma (modulus) and mul, fma, abs-add (phase); two accumulators per output.
#include <string.h>

#include <algorithm>

#include "common.h"
#include "segment_pass.h"

namespace bess {

static const char* const HAKE_TOO_WIDE =
    "HAKE: embedding size %d too wide for the row kernels (max 512; 256 when not a multiple of 4, 128 when odd)";

constexpr float HAKE_REV = 0.07957747154594767f;  // 1 / (4 pi): half an angle in radians, as revolutions

// v_sin_f32 / v_cos_f32 take revolutions (|x| <= 256: phase differences up to 512 pi); absolute error 1.3e-7
__device__ __forceinline__ float sin_rev(float x) { return __builtin_amdgcn_sinf(x); }
__device__ __forceinline__ float cos_rev(float x) { return __builtin_amdgcn_cosf(x); }

inline float float_of_bits(int32_t b) {
    float f;
    memcpy(&f, &b, sizeof f);
    return f;
}

// ---------------------------------------------------------------------------------------------------------------
// row form
// Row classes: the parts of a row are read as 4-, 2- or 1-element vectors of either table type (a part starts d
// elements into the row, so the vector must divide d)
struct HakeRows {
    using f32_vecs = Ints<4, 2, 1>;
    using f16_vecs = Ints<4, 2, 1>;
    using its = Ints<1, 2, 4, 8>;
};
inline int hake_vec_of(int dd) { return dd % 4 == 0 ? 4 : (dd % 2 == 0 ? 2 : 1); }

struct HakeArgs {
    const float* query;  // [n_query, 3 d]
    const void* base;
    const int32_t* idx;  // [n_query * n_neg] (idx_stride = n_neg) or [n_neg] (idx_stride = 0) or NULL (row k)
    int64_t idx_stride;
    int64_t n_query;
    int n_neg;
    int d;
    int nch;
    int nb, items_per_query;
    float lp;  // phase weight
    float ps;  // phase_scale
};

// the query's three vectors
template <int VEC, int IT>
struct HakeQuery {
    float u[IT][VEC], r[IT][VEC], qp[IT][VEC];
    __device__ __forceinline__ void load(const float* q, int g, int d, int nch) {
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int ch = g + 16 * it;
            load_chunk<float, VEC>(q, ch, nch, u[it]);
            load_chunk<float, VEC>(q + d, ch, nch, r[it]);
            load_chunk<float, VEC>(q + 2 * d, ch, nch, qp[it]);
        }
    }
};

// ev[0] = phase, ev[1] = modulus; chunks past the row's end are zero: m = 0 and sin(0) = 0 add nothing
template <typename T, int VEC, int IT>
__device__ __forceinline__ void hake_load_row(const T* rp, int g, int d, int nch, float (&ev)[2][IT][VEC]) {
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int it = 0; it < IT; ++it) load_chunk<T, VEC>(rp + p * d, g + 16 * it, nch, ev[p][it]);
}

// (sum of squares of the modulus difference, sum of |sin| of the half phase difference) of one row, over the 16 lanes
template <int VEC, int IT>
__device__ __forceinline__ void hake_row_sums(const HakeQuery<VEC, IT>& qv, const float (&ev)[2][IT][VEC], float ps,
                                              float& am, float& ap) {
    am = ap = 0.f;
#pragma unroll
    for (int it = 0; it < IT; ++it)
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const float m = fmaf(qv.u[it][v], ev[1][it][v], qv.r[it][v]);
            am = fmaf(m, m, am);
            ap += fabsf(sin_rev(fmaf(-ps, ev[0][it][v], qv.qp[it][v]) * HAKE_REV));
        }
    am = row16_allreduce_sum(am);
    ap = row16_allreduce_sum(ap);
}

// d total / d (modulus difference) and d total / d (phase difference) of one element, total = ||m||_2 + l_p sum |sin|;
// gm = go / ||m|| (0 at the kink), gl = go * l_p / 2.  sgn through the 2^100 pre-scale: sin == 0 gives 0.
__device__ __forceinline__ void hake_dterms(float u, float r, float qp, float cp, float cm, float ps, float gm,
                                            float gl, float& dm, float& dp) {
    dm = gm * fmaf(u, cm, r);
    const float x = fmaf(-ps, cp, qp) * HAKE_REV;
    dp = gl * sgn_prescaled(sin_rev(x) * SGN_PRESCALE) * cos_rev(x);
}

__device__ __forceinline__ int64_t ceil_div_dev(int64_t a, int64_t b) { return (a + b - 1) / b; }

__device__ __forceinline__ const int32_t* hake_idx(const HakeArgs& a, int64_t q) {
    return a.idx ? a.idx + q * a.idx_stride : nullptr;
}

// COUNT: the counting variant of the row form (CountArgs of common.h; shared candidates only), as k_box_fwd's
template <typename T, int VEC, int IT, bool COUNT>
__global__ __launch_bounds__(256) void k_hake_fwd(HakeArgs a, float* __restrict__ out, int64_t ld_out,
                                                  const float* __restrict__ thr, CountArgs cnt) {
    const int lane = threadIdx.x & 63;
    const int g = lane & 15, sub = lane >> 4;
    const int64_t item = blockIdx.x * 4ll + (threadIdx.x >> 6);
    if (item >= a.n_query * a.items_per_query) return;
    const int64_t q = COUNT ? item % a.n_query : item / a.items_per_query;
    const int k0 = static_cast<int>(COUNT ? item / a.n_query : item - q * a.items_per_query) * a.nb;
    const int k1 = min(k0 + a.nb, a.n_neg);
    float th = 0.f;
    int64_t ex = -1;
    int cg = 0, ce = 0;
    if constexpr (COUNT) {
        th = thr[q];
        ex = static_cast<int64_t>(cnt.excl[q]) - cnt.col0;
    }
    HakeQuery<VEC, IT> qv;
    qv.load(a.query + q * 3 * a.d, g, a.d, a.nch);
    const T* base = static_cast<const T*>(a.base);
    const int32_t* idx = hake_idx(a, q);
    float* orow = COUNT ? nullptr : out + q * ld_out;
    for (int kb = k0; kb < k1; kb += 4) {
        const int k = kb + sub;
        const bool valid = k < k1;
        const int ks = valid ? k : (k1 - 1);
        const int64_t row = idx ? static_cast<int64_t>(idx[ks]) : ks;
        float ev[2][IT][VEC];
        hake_load_row<T, VEC, IT>(base + row * 2 * a.d, g, a.d, a.nch, ev);
        float am, ap;
        hake_row_sums<VEC, IT>(qv, ev, a.ps, am, ap);
        const float sc = -fmaf(a.lp, ap, sqrtf(am));
        if constexpr (COUNT) {
            const float v = count_value(sc, cnt.round16);
            const bool in = valid && k != ex;
            cg += (in && v > th) ? 1 : 0;
            ce += (in && v == th) ? 1 : 0;
        } else {
            if (g == 0 && valid) orow[k] = sc;
        }
    }
    if constexpr (COUNT) {  // (the 16 lanes of a group hold the same counts)
        cg += __shfl_xor(cg, 16, 64);
        cg += __shfl_xor(cg, 32, 64);
        ce += __shfl_xor(ce, 16, 64);
        ce += __shfl_xor(ce, 32, 64);
        if (lane == 0) {
            if (cg) atomicAdd(cnt.counts + 2 * q, cg);
            if (ce) atomicAdd(cnt.counts + 2 * q + 1, ce);
        }
    }
}

// d_neg (per-triple negatives; NULL for shared candidates, whose d_neg is k_hake_bwd_cand's): DN_REF = stored at
// reference (q, k); DN_ROW = stored at row idx[k] of a matrix over the table's row space (BESS_FLAG_DNEG_BY_ROW)
enum : int { DN_REF = 0, DN_ROW = 2 };

template <typename T, int VEC, int IT>
__global__ __launch_bounds__(256) void k_hake_bwd(HakeArgs a, const float* __restrict__ d_out, int64_t ld_dout,
                                                  float* __restrict__ d_query, float* __restrict__ d_neg, int dn_mode) {
    const int lane = threadIdx.x & 63;
    const int g = lane & 15, sub = lane >> 4;
    const int64_t item = blockIdx.x * 4ll + (threadIdx.x >> 6);
    if (item >= a.n_query * a.items_per_query) return;
    const int64_t q = item / a.items_per_query;
    const int k0 = static_cast<int>(item - q * a.items_per_query) * a.nb;
    const int k1 = min(k0 + a.nb, a.n_neg);
    HakeQuery<VEC, IT> qv;
    qv.load(a.query + q * 3 * a.d, g, a.d, a.nch);
    float du[IT][VEC], dr[IT][VEC], dqp[IT][VEC];
#pragma unroll
    for (int it = 0; it < IT; ++it)
#pragma unroll
        for (int v = 0; v < VEC; ++v) du[it][v] = dr[it][v] = dqp[it][v] = 0.f;
    const T* base = static_cast<const T*>(a.base);
    const int32_t* idx = hake_idx(a, q);
    for (int kb = k0; kb < k1; kb += 4) {
        const int k = kb + sub;
        const bool valid = k < k1;
        const int ks = valid ? k : (k1 - 1);
        const int64_t row = idx ? static_cast<int64_t>(idx[ks]) : ks;
        float ev[2][IT][VEC];
        hake_load_row<T, VEC, IT>(base + row * 2 * a.d, g, a.d, a.nch, ev);
        const float go = valid ? -d_out[q * ld_dout + ks] : 0.f;  // d score / d (||m|| + l_p sum |sin|)
        float* dn = nullptr;
        if (d_neg) {
            const int64_t at = dn_mode == DN_ROW ? row : q * a.n_neg + ks;
            dn = d_neg + at * 2 * a.d;
        }
        float am, ap;
        hake_row_sums<VEC, IT>(qv, ev, a.ps, am, ap);
        const float gm = go * lp_inv(sqrtf(am), 2.f), gl = go * a.lp * 0.5f;
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int ch = g + 16 * it;
            float de[2][VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                float dm, dp;
                hake_dterms(qv.u[it][v], qv.r[it][v], qv.qp[it][v], ev[0][it][v], ev[1][it][v], a.ps, gm, gl, dm, dp);
                du[it][v] = fmaf(dm, ev[1][it][v], du[it][v]);
                dr[it][v] += dm;
                dqp[it][v] += dp;
                de[0][v] = -a.ps * dp;
                de[1][v] = dm * qv.u[it][v];
            }
            if (dn && valid && ch < a.nch) {
#pragma unroll
                for (int p = 0; p < 2; ++p)
#pragma unroll
                    for (int v = 0; v < VEC; ++v) dn[p * a.d + ch * VEC + v] = de[p][v];
            }
        }
    }
    float* dq = d_query + q * 3 * a.d;
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int ch = g + 16 * it;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            float x[3] = {du[it][v], dr[it][v], dqp[it][v]};
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                x[j] += __shfl_xor(x[j], 16, 64);
                x[j] += __shfl_xor(x[j], 32, 64);
                if (sub == 0 && ch < a.nch) {
                    float* o = dq + j * a.d + ch * VEC + v;
                    if (a.items_per_query == 1) *o = x[j];
                    else unsafeAtomicAdd(o, x[j]);
                }
            }
        }
    }
}

// d_neg of shared candidates without atomics: the roles swapped.  A 16-lane group keeps ONE candidate row and its
// gradient in registers and streams the queries of its slice (the four groups of a wave read the same query rows);
// per (query, candidate) the arithmetic is k_hake_bwd's.  One slice per candidate stores, more add.  (With d_neg
// through atomics in k_hake_bwd, S x N x 2 d of them, the backward over all entities took as long as torch's.)
template <typename T, int VEC, int IT>
__global__ __launch_bounds__(256) void k_hake_bwd_cand(HakeArgs a, const float* __restrict__ d_out, int64_t ld_dout,
                                                       float* __restrict__ d_neg, int qb, int items_per_cand) {
    const int lane = threadIdx.x & 63;
    const int g = lane & 15, sub = lane >> 4;
    const int64_t item = blockIdx.x * 4ll + (threadIdx.x >> 6);
    if (item >= ceil_div_dev(a.n_neg, 4) * items_per_cand) return;
    const int64_t cgroup = item / items_per_cand;
    const int64_t q0 = (item - cgroup * items_per_cand) * qb;
    const int64_t q1 = min(q0 + qb, a.n_query);
    const int k = static_cast<int>(cgroup) * 4 + sub;
    const bool valid = k < a.n_neg;
    const int ks = valid ? k : (a.n_neg - 1);
    const int64_t row = a.idx ? static_cast<int64_t>(a.idx[ks]) : ks;
    float ev[2][IT][VEC], acc[2][IT][VEC];
    hake_load_row<T, VEC, IT>(static_cast<const T*>(a.base) + row * 2 * a.d, g, a.d, a.nch, ev);
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int it = 0; it < IT; ++it)
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[p][it][v] = 0.f;
    for (int64_t q = q0; q < q1; ++q) {
        HakeQuery<VEC, IT> qv;
        qv.load(a.query + q * 3 * a.d, g, a.d, a.nch);
        const float go = -d_out[q * ld_dout + ks];
        float am, ap;
        hake_row_sums<VEC, IT>(qv, ev, a.ps, am, ap);
        const float gm = go * lp_inv(sqrtf(am), 2.f), gl = go * a.lp * 0.5f;
#pragma unroll
        for (int it = 0; it < IT; ++it)
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                float dm, dp;
                hake_dterms(qv.u[it][v], qv.r[it][v], qv.qp[it][v], ev[0][it][v], ev[1][it][v], a.ps, gm, gl, dm, dp);
                acc[0][it][v] = fmaf(-a.ps, dp, acc[0][it][v]);
                acc[1][it][v] = fmaf(dm, qv.u[it][v], acc[1][it][v]);
            }
    }
    float* dn = d_neg + static_cast<int64_t>(ks) * 2 * a.d;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int ch = g + 16 * it;
            if (!valid || ch >= a.nch) continue;
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                if (items_per_cand == 1) dn[p * a.d + ch * VEC + v] = acc[p][it][v];
                else unsafeAtomicAdd(dn + p * a.d + ch * VEC + v, acc[p][it][v]);
            }
        }
}

static HakeArgs hake_args(const bess_model_desc* d, const float* query, int64_t n_query, const void* neg_base,
                          const int32_t* neg_idx, int64_t idx_stride, int64_t n_neg, int nb) {
    const int dd = d->width / 2;
    const int vec = hake_vec_of(dd);
    HakeArgs a;
    a.query = query;
    a.base = neg_base;
    a.idx = neg_idx;
    a.idx_stride = idx_stride;
    a.n_query = n_query;
    a.n_neg = static_cast<int>(n_neg);
    a.d = dd;
    a.nch = dd / vec;
    a.nb = nb;
    a.items_per_query = static_cast<int>(ceil_div(n_neg, nb));
    a.lp = float_of_bits(d->reserved[1]);
    a.ps = float_of_bits(d->reserved[2]);
    return a;
}

// the row form; shared == true: idx is one list of n_neg rows for every query (or NULL = rows 0..n_neg-1), d_neg is
// [n_neg, 2d]
static int hake_rows(const bess_model_desc* d, bool fwd, bool shared, const float* query, int64_t n_query,
                     const void* neg_base, const int32_t* neg_idx, int64_t n_neg, float* out, const float* d_out,
                     int64_t ld, float* dq, float* dn, hipStream_t st, const float* thr, const CountArgs* count) {
    // (counting: a wave's candidates end in one atomic pair)
    const HakeArgs a = hake_args(d, query, n_query, neg_base, neg_idx, shared ? 0 : n_neg, n_neg,
                                 negatives_per_item(n_query, n_neg, count ? 256 : 64));
    BESS_REQUIRE(ceil_div(n_query * a.items_per_query, 4) < (1ll << 31), "HAKE: problem too large for one launch");
    BESS_REQUIRE(fwd || dq, "HAKE: the backward writes d_query (NULL)");
    const int it = static_cast<int>(ceil_div(a.nch, 16));
    const int dn_mode = (d->reserved[0] & BESS_FLAG_DNEG_BY_ROW) ? DN_ROW : DN_REF;
    // shared candidates: d_neg from the candidate-side kernel, in slices of qb queries
    const int64_t cand_groups = ceil_div(n_neg, 4);
    const int qb = negatives_per_item(cand_groups, n_query, 4096);
    const int items_per_cand = static_cast<int>(ceil_div(n_query, qb));
    BESS_REQUIRE(ceil_div(cand_groups * items_per_cand, 4) < (1ll << 31), "HAKE: problem too large for one launch");
    if (!fwd) {
        hipError_t e = hipSuccess;
        if (a.items_per_query > 1) e = fill_words_async(dq, 0u, n_query * 3 * a.d, st);
        if (e == hipSuccess && shared && dn && items_per_cand > 1) e = fill_words_async(dn, 0u, n_neg * 2 * a.d, st);
        if (e != hipSuccess) return fail(static_cast<int>(e), "memset: %s", hipGetErrorString(e));
    }
    const unsigned blocks = static_cast<unsigned>(ceil_div(a.n_query * a.items_per_query, 4));
    const CountArgs none{nullptr, nullptr, 0, 0};
    const bool ok = dispatch_row_class<HakeRows>(d->dtype, a.d / a.nch, it, [&](auto c) {
        using C = decltype(c);
        using T = typename C::T;
        if (count) k_hake_fwd<T, C::VEC, C::IT, true><<<blocks, 256, 0, st>>>(a, nullptr, 0, thr, *count);
        else if (fwd) k_hake_fwd<T, C::VEC, C::IT, false><<<blocks, 256, 0, st>>>(a, out, ld, nullptr, none);
        else {
            k_hake_bwd<T, C::VEC, C::IT><<<blocks, 256, 0, st>>>(a, d_out, ld, dq, shared ? nullptr : dn, dn_mode);
            if (shared && dn)
                k_hake_bwd_cand<T, C::VEC, C::IT><<<static_cast<unsigned>(ceil_div(cand_groups * items_per_cand, 4)), 256, 0, st>>>(
                    a, d_out, ld, dn, qb, items_per_cand);
        }
    });
    if (!ok) return fail(BESS_EUNSUPPORTED, HAKE_TOO_WIDE, a.d);
    return check_launch(fwd ? "neg_score fwd (HAKE)" : "neg_score bwd (HAKE)");
}

// ---------------------------------------------------------------------------------------------------------------
// K9 for the per-triple negatives of the own shard (HAKE counterpart of k_box_grad_segments, boxe.hip): one 16-lane
// group per unique destination row; the row is loaded once and every reference (q, k) of the segment contributes
// d score / d e recomputed from query[q] and d_out[q, k] - the arithmetic of k_hake_bwd's d_neg.  Rows with more than
// BESS_SEGMENT_CAP references go to the whole grid in slices (segment_pass.h).
struct HakeSegArgs {
    const float* query;  // [n_query, 3 d]
    const void* table;
    const float* d_out;
    int64_t ld_dout;
    const int32_t* refs;
    const int32_t* seg_rows;
    const int32_t* seg_offsets;
    const int32_t* n_seg;
    int n_neg;
    int d;
    int nch;
    const int32_t* long_segs;
    float lp, ps;
};

// acc += d score / d e over references [r0, r1) of one row (ev)
template <int VEC, int IT>
__device__ __forceinline__ void hake_seg_accumulate(const HakeSegArgs& a, int g, const float (&ev)[2][IT][VEC], int r0,
                                                    int r1, float (&acc)[2][IT][VEC]) {
    for (int r = r0; r < r1; ++r) {
        const int ref = a.refs[r];
        const int q = ref / a.n_neg;
        const int k = ref - q * a.n_neg;
        const float go = -a.d_out[q * a.ld_dout + k];
        HakeQuery<VEC, IT> qv;
        qv.load(a.query + static_cast<int64_t>(q) * 3 * a.d, g, a.d, a.nch);
        float am, ap;
        hake_row_sums<VEC, IT>(qv, ev, a.ps, am, ap);
        const float gm = go * lp_inv(sqrtf(am), 2.f), gl = go * a.lp * 0.5f;
#pragma unroll
        for (int it = 0; it < IT; ++it)
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                float dm, dp;
                hake_dterms(qv.u[it][v], qv.r[it][v], qv.qp[it][v], ev[0][it][v], ev[1][it][v], a.ps, gm, gl, dm, dp);
                acc[0][it][v] = fmaf(-a.ps, dp, acc[0][it][v]);
                acc[1][it][v] = fmaf(dm, qv.u[it][v], acc[1][it][v]);
            }
    }
}

template <typename T, int VEC, int IT>
__device__ __forceinline__ void hake_seg_store(const HakeSegArgs& a, int g, const float (&ev)[2][IT][VEC],
                                               const float (&acc)[2][IT][VEC], int64_t seg, int64_t row,
                                               float* __restrict__ grad_seg, T* table_rw, float lr) {
    const int W = 2 * a.d;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int c = g + 16 * it;
            if (c >= a.nch) continue;
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const int64_t o = p * a.d + c * VEC + v;
                if (grad_seg) grad_seg[seg * W + o] = acc[p][it][v];
                else table_rw[row * W + o] = static_cast<T>(ev[p][it][v] - lr * acc[p][it][v]);
            }
        }
}

template <int VEC, int IT>
__device__ __forceinline__ void hake_zero(float (&acc)[2][IT][VEC]) {
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int it = 0; it < IT; ++it)
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[p][it][v] = 0.f;
}

template <typename T, int VEC, int IT>
__global__ __launch_bounds__(256) void k_hake_grad_segments(HakeSegArgs a, float* __restrict__ grad_seg, T* table_rw,
                                                            float lr) {
    const int g = threadIdx.x & 15;
    const int n_seg = *a.n_seg;
    const int64_t group0 = (blockIdx.x * 256ll + threadIdx.x) >> 4;
    const int64_t n_group = (gridDim.x * 256ll) >> 4;
    const T* table = static_cast<const T*>(a.table);
    for (int64_t seg = group0; seg < n_seg; seg += n_group) {
        const int64_t row = a.seg_rows[seg];
        const int r0 = a.seg_offsets[seg], r1 = a.seg_offsets[seg + 1];
        if (a.long_segs && r1 - r0 > BESS_SEGMENT_CAP) continue;  // left to k_hake_long_segments
        float ev[2][IT][VEC], acc[2][IT][VEC];
        hake_load_row<T, VEC, IT>(table + row * 2 * a.d, g, a.d, a.nch, ev);
        hake_zero<VEC, IT>(acc);
        hake_seg_accumulate<VEC, IT>(a, g, ev, r0, r1, acc);
        hake_seg_store<T, VEC, IT>(a, g, ev, acc, seg, row, grad_seg, table_rw, lr);
    }
}

template <typename T, int VEC, int IT>
__global__ __launch_bounds__(256) void k_hake_long_segments(HakeSegArgs a, float* __restrict__ long_grad,
                                                            int32_t* __restrict__ long_cnt, int32_t capacity,
                                                            float* __restrict__ grad_seg, T* table_rw, float lr) {
    const int lane = threadIdx.x & 63, g = lane & 15;
    const int64_t group0 = (blockIdx.x * 256ll + threadIdx.x) >> 4;
    const int64_t n_group = (gridDim.x * 256ll) >> 4;
    const int n_long = min(a.long_segs[0], capacity);
    const T* table = static_cast<const T*>(a.table);
    const int W = 2 * a.d;
    for (int li = 0; li < n_long; ++li) {
        const int seg = a.long_segs[1 + li];
        const int64_t row = a.seg_rows[seg];
        const int r0 = a.seg_offsets[seg], r1 = a.seg_offsets[seg + 1];
        const int parts = (r1 - r0 + BESS_SEGMENT_CAP - 1) / BESS_SEGMENT_CAP;
        if (group0 >= parts) continue;
        float ev[2][IT][VEC];
        hake_load_row<T, VEC, IT>(table + row * W, g, a.d, a.nch, ev);
        float* sum = long_grad + static_cast<int64_t>(li) * W;
        for (int64_t pt = group0; pt < parts; pt += n_group) {
            float acc[2][IT][VEC];
            hake_zero<VEC, IT>(acc);
            const int rb = r0 + static_cast<int>(pt) * BESS_SEGMENT_CAP;
            hake_seg_accumulate<VEC, IT>(a, g, ev, rb, min(r1, rb + BESS_SEGMENT_CAP), acc);
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int it = 0; it < IT; ++it) {
                    const int c = g + 16 * it;
                    if (c < a.nch) {
#pragma unroll
                        for (int v = 0; v < VEC; ++v) atomicAdd(sum + p * a.d + c * VEC + v, acc[p][it][v]);
                    }
                }
            if ((seg_count_slice(long_cnt + li, lane, g) + 1) % parts != 0) continue;
            seg_last_slice(long_cnt + li, g);
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int it = 0; it < IT; ++it) {
                    const int c = g + 16 * it;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        acc[p][it][v] = 0.f;
                        if (c < a.nch) acc[p][it][v] = seg_take(sum + p * a.d + c * VEC + v);
                    }
                }
            hake_seg_store<T, VEC, IT>(a, g, ev, acc, seg, row, grad_seg, table_rw, lr);
        }
    }
}

int hake_grad_segments(const bess_model_desc* d, const SegRefs& r, const SegPass& ps, hipStream_t st) {
    const int dd = d->width / 2;
    const int vec = hake_vec_of(dd);
    const HakeSegArgs a{r.query, r.table, r.d_out, r.ld_dout, r.refs, r.seg_rows, r.seg_offsets, r.n_seg, r.n_neg,
                        dd, dd / vec, r.long_segs, float_of_bits(d->reserved[1]), float_of_bits(d->reserved[2])};
    const int it = static_cast<int>(ceil_div(a.nch, 16));
    return launch_segment_pass(r, ps, 1, "neg_pertriple_grad_segments (HAKE)", [&](unsigned blocks, bool long_tier) {
        const bool ok = dispatch_row_class<HakeRows>(d->dtype, vec, it, [&](auto c) {
            using C = decltype(c);
            using T = typename C::T;
            T* rw = static_cast<T*>(r.table);
            if (long_tier)
                k_hake_long_segments<T, C::VEC, C::IT><<<blocks, 256, 0, st>>>(
                    a, ps.long_grad, ps.long_count, static_cast<int32_t>(ps.long_cap), ps.grad_seg, rw, ps.fused_sgd_lr);
            else
                k_hake_grad_segments<T, C::VEC, C::IT><<<blocks, 256, 0, st>>>(a, ps.grad_seg, rw, ps.fused_sgd_lr);
        });
        return ok ? BESS_OK : fail(BESS_EUNSUPPORTED, HAKE_TOO_WIDE, a.d);
    });
}

// ---------------------------------------------------------------------------------------------------------------
// tile form: forward over shared candidates
constexpr int HKT = 16;   // K-slice
constexpr int HLDP = 68;  // padded tile row: the float4 reads of 16 consecutive threads fall on distinct banks

struct HakeTile {
    const float* Q;  // [S, 3 d]
    int64_t S;
    const int32_t* idx;  // candidate rows (NULL: rows 0 .. N-1)
    int64_t N;
    int d;
    int vec_q, vec_c;  // rows may be read as 4-element vectors
    float lp, ps_rev;
    int norm_only;  // the storing form writes ||U c_m + R||_2 instead of the score (the backward's pre-pass)
};

// This thread's share of a K-slice: 4 consecutive k (kc .. kc + 3 past k0) of one query row and one candidate row.
// Elements past d are zero in every image (sin AND cos), so they add nothing to either accumulator.
__device__ __forceinline__ void hake_fetch_q(const float* __restrict__ rp, int d, int k0, bool vec, float (&v)[3][4]) {
    const int kc = (threadIdx.x & 3) * 4;
    if (vec && k0 + kc + 3 < d) {
#pragma unroll
        for (int p = 0; p < 3; ++p) VecLoad<float, 4>::load(rp + p * d + k0, v[p]);
    } else {
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int i = 0; i < 4; ++i) v[p][i] = (k0 + kc + i < d) ? rp[p * d + k0 + i] : 0.f;
    }
}
template <typename TC>
__device__ __forceinline__ void hake_fetch_c(const TC* __restrict__ rp, int d, int k0, bool vec, float (&v)[2][4]) {
    const int kc = (threadIdx.x & 3) * 4;
    if (vec && k0 + kc + 3 < d) {
#pragma unroll
        for (int p = 0; p < 2; ++p) VecLoad<TC, 4>::load(rp + p * d + k0, v[p]);
    } else {
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int i = 0; i < 4; ++i) v[p][i] = (k0 + kc + i < d) ? to_f32(rp[p * d + k0 + i]) : 0.f;
    }
}

// COUNT: the counting epilogue of common.h's CountArgs - a workgroup walks over `tiles` consecutive column tiles and
// keeps its rows' two counters in registers (at most one atomic pair per row); nothing is stored.  DIAG: S == N, the
// workgroup of row tile y computes column tile y only and stores its diagonal: out[i] = score(query i, candidate i).
// The K loop and the expression of the score are the same code in all three, so a rank counted here equals the rank
// of the stored scores to the last bit.
template <typename TC, bool COUNT, bool DIAG>
__global__ __launch_bounds__(256) void k_hake_tile_fwd(HakeTile a, const TC* __restrict__ base, float* __restrict__ out,
                                                       int64_t ld_out, const float* __restrict__ thr, CountArgs cnt,
                                                       int tiles) {
    __shared__ __attribute__((aligned(16))) float Qs[4][HKT][HLDP];  // U, R, l_p sin(Q_p / 2), l_p cos(Q_p / 2)
    __shared__ __attribute__((aligned(16))) float Cs[3][HKT][HLDP];  // c_m, cos(s c_p / 2), -sin(s c_p / 2)
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int srow = threadIdx.x >> 2, kc = (threadIdx.x & 3) * 4;  // the row and first k this thread stages
    const int d = a.d;
    const int64_t q0 = static_cast<int64_t>(blockIdx.y) * 64;
    const float* qrow = a.Q + min(q0 + srow, a.S - 1) * 3 * d + kc;
    int cg[4] = {0, 0, 0, 0}, ce[4] = {0, 0, 0, 0};
    const int n_tile = COUNT ? tiles : 1;
    for (int tile = 0; tile < n_tile; ++tile) {
        const int64_t j0 = DIAG ? q0 : (static_cast<int64_t>(blockIdx.x) * n_tile + tile) * 64;
        if (COUNT && j0 >= a.N) break;  // (the same for the whole workgroup)
        float am[4][4], ap[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) am[i][j] = ap[i][j] = 0.f;
        const int64_t ci = min(j0 + srow, a.N - 1);
        const TC* crow = base + (a.idx ? static_cast<int64_t>(a.idx[ci]) : ci) * 2 * d + kc;
        float qv[3][4], cv[2][4];
        hake_fetch_q(qrow, d, 0, a.vec_q != 0, qv);
        hake_fetch_c<TC>(crow, d, 0, a.vec_c != 0, cv);
        for (int k0 = 0; k0 < d; k0 += HKT) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float live = (k0 + kc + i < d) ? 1.f : 0.f;
                const float xa = qv[2][i] * HAKE_REV, xb = cv[0][i] * a.ps_rev;
                Qs[0][kc + i][srow] = qv[0][i];
                Qs[1][kc + i][srow] = qv[1][i];
                Qs[2][kc + i][srow] = live * a.lp * sin_rev(xa);
                Qs[3][kc + i][srow] = live * a.lp * cos_rev(xa);
                Cs[0][kc + i][srow] = cv[1][i];
                Cs[1][kc + i][srow] = live * cos_rev(xb);
                Cs[2][kc + i][srow] = -live * sin_rev(xb);
            }
            __syncthreads();
            if (k0 + HKT < d) {
                hake_fetch_q(qrow, d, k0 + HKT, a.vec_q != 0, qv);
                hake_fetch_c<TC>(crow, d, k0 + HKT, a.vec_c != 0, cv);
            }
            // the slice's 16 terms are summed on their own and then added: chains of 16 and of d / 16 terms, not of d
            float sm[4][4], sp[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) sm[i][j] = sp[i][j] = 0.f;
#pragma unroll
            for (int k = 0; k < HKT; ++k) {
                float u[4][4], c[3][4];
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const float4 t = *reinterpret_cast<const float4*>(&Qs[p][k][ty * 4]);
                    u[p][0] = t.x; u[p][1] = t.y; u[p][2] = t.z; u[p][3] = t.w;
                }
#pragma unroll
                for (int p = 0; p < 3; ++p) {
                    const float4 t = *reinterpret_cast<const float4*>(&Cs[p][k][tx * 4]);
                    c[p][0] = t.x; c[p][1] = t.y; c[p][2] = t.z; c[p][3] = t.w;
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float m = fmaf(u[0][i], c[0][j], u[1][i]);
                        sm[i][j] = fmaf(m, m, sm[i][j]);
                        const float s = fmaf(u[3][i], c[2][j], u[2][i] * c[1][j]);
                        sp[i][j] += fabsf(s);
                    }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    am[i][j] += sm[i][j];
                    ap[i][j] += sp[i][j];
                }
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t q = q0 + ty * 4 + i;
            if constexpr (COUNT) {
                // (rows past the end count against the last row's threshold and are dropped at the atomics)
                const int64_t qc = min(q, a.S - 1);
                const float th = thr[qc];
                const int64_t ex = static_cast<int64_t>(cnt.excl[qc]) - cnt.col0;  // position in this launch's columns
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int64_t jj = j0 + tx * 4 + j;
                    const float v = count_value(-(sqrtf(am[i][j]) + ap[i][j]), cnt.round16);
                    const bool in = jj < a.N && jj != ex;
                    cg[i] += (in && v > th) ? 1 : 0;
                    ce[i] += (in && v == th) ? 1 : 0;
                }
            } else {
                if (q >= a.S) continue;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int64_t jj = j0 + tx * 4 + j;
                    const float sc = a.norm_only ? sqrtf(am[i][j]) : -(sqrtf(am[i][j]) + ap[i][j]);
                    if (DIAG) {
                        if (jj == q) out[q] = sc;
                    } else if (jj < a.N) {
                        out[q * ld_out + jj] = sc;
                    }
                }
            }
        }
    }
    if constexpr (COUNT) {
        // the 16 threads that share a ty are the 16 lanes of one DPP row (at most 64 * tiles per counter: exact in f32)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int g = static_cast<int>(row16_allreduce_sum(static_cast<float>(cg[i])));
            const int e = static_cast<int>(row16_allreduce_sum(static_cast<float>(ce[i])));
            const int64_t q = q0 + ty * 4 + i;
            if (tx == 0 && q < a.S) {
                if (g) atomicAdd(cnt.counts + 2 * q, g);
                if (e) atomicAdd(cnt.counts + 2 * q + 1, e);
            }
        }
    }
}

// the tile form's shapes: the row tiles are the grid's y
static bool hake_tile_takes(const bess_model_desc* d, int64_t S) {
    return !(d->reserved[0] & BESS_FLAG_FP32_MATH) && ceil_div(S, 64) < 65536;
}

// cnt != NULL: counts only; diag: S == N, out [S]; else out [S, ld]
static int hake_tile_fwd(const bess_model_desc* d, const float* query, int64_t S, const void* base, const int32_t* idx,
                         int64_t N, float* out, int64_t ld, const float* thr, const CountArgs* cnt, bool diag,
                         hipStream_t st, bool norm_only = false) {
    const int dd = d->width / 2;
    const float scale = float_of_bits(d->reserved[2]);
    const bool v4 = dd % 4 == 0;
    const HakeTile a{query, S, idx, N, dd, v4 && reinterpret_cast<uintptr_t>(query) % 16 == 0,
                     v4 && reinterpret_cast<uintptr_t>(base) % 16 == 0, float_of_bits(d->reserved[1]), scale * HAKE_REV,
                     norm_only ? 1 : 0};
    const int64_t col_tiles = ceil_div(N, 64), row_tiles = ceil_div(S, 64);
    const CountArgs none{nullptr, nullptr, 0, 0};
    with_table_type(d->dtype, [&](auto t) {
        using T = decltype(t);
        const T* b = static_cast<const T*>(base);
        if (cnt) {
            // column tiles per workgroup: as many as leave the chip ~8 workgroups per CU (one atomic pair per row each)
            int tiles = 1;
            while (tiles < 8 && row_tiles * ceil_div(col_tiles, tiles * 2) >= 256 * 8) tiles *= 2;
            const dim3 grid(static_cast<unsigned>(ceil_div(col_tiles, tiles)), static_cast<unsigned>(row_tiles));
            k_hake_tile_fwd<T, true, false><<<grid, 256, 0, st>>>(a, b, nullptr, 0, thr, *cnt, tiles);
        } else if (diag) {
            k_hake_tile_fwd<T, false, true><<<dim3(1, static_cast<unsigned>(row_tiles)), 256, 0, st>>>(a, b, out, 0, nullptr, none, 1);
        } else {
            const dim3 grid(static_cast<unsigned>(col_tiles), static_cast<unsigned>(row_tiles));
            k_hake_tile_fwd<T, false, false><<<grid, 256, 0, st>>>(a, b, out, ld, nullptr, none, 1);
        }
        return 0;
    });
    return check_launch(cnt ? "neg_score_shared_fwd_counts (HAKE)" : (diag ? "neg_score_shared_fwd_pairs (HAKE)" : "neg_score_shared_fwd (HAKE)"));
}

// ---------------------------------------------------------------------------------------------------------------
// tile form: backward over shared candidates, two kernels in the shape of k_aff_shared_bwd (affine.hip).
// X = the side whose gradient is produced (rows a, 64 per workgroup, 64 columns w of d: operands and sums in
// registers), Y = the other side (rows b, the reduction, K-slices of 16 through LDS).  XQ: X is the query side
// (d_query [S, 3 d]), otherwise the candidate side (the dense d_cand [N, 2 d]).  Both sides enter as (modulus operands,
// sin / cos images of the half phases), written when an operand is loaded (X: once) or staged (Y: per slice), so the
// loop holds no transcendental:
//     sin((a - b) / 2) = sa cb - ca sb,   cos((a - b) / 2) = ca cb + sa sb
// (the raw phases ride along for the sign of a sine that the images cannot tell from zero: hake_sign_exact).
// The coefficient tile in LDS holds, per (a, b), gm = -g / ||U c_m + R|| (0 at a zero norm) and gl = -g l_p / 2; the
// norms are recomputed by the forward tile kernel into the call's workspace (norm_only), never taken from the scores.
//     dm = gm (U c_m + R),  dp = gl sgn(sin) cos        XQ: dU += dm c_m, dR += dm, dQ_p += dp
//                                                       !XQ: dc_m += dm U, dc_p -= phase_scale dp
// The reduction is split over gridDim.z when the grid is small (float atomics into the zeroed target).
// Where the images leave sin((a - b) / 2) within their own error of zero, its sign comes from the phase difference
// itself (x = a - b, one fma of the raw phases: exact for close operands): x = 2 pi k + r, sin(x / 2) = (-1)^k
// sin(r / 2).  Equal phases give exactly 0, the kink convention of the row form.
constexpr float HAKE_SIGN_EPS = 4e-6f;  // > 10 x the error of the difference identity on images of 1.3e-7 error
__device__ __forceinline__ float hake_sign_exact(float x) {
    const float k = rintf(x * 0.15915494309189535f);
    const float r = fmaf(-6.283185307179586f, k, x);
    const float odd = k - 2.f * rintf(0.5f * k);  // 0 or +-1
    return sgn_prescaled(r * SGN_PRESCALE) * (odd == 0.f ? 1.f : -1.f);
}

struct HakeBwd {
    const float* Q;  // [S, 3 d]
    int64_t S;
    const int32_t* idx;
    int64_t N;
    int d;
    const float* d_out;
    int64_t ld_dout;
    const float* norm;  // [S, N]
    float lp, ps, ps_rev;
};

template <typename TC, bool XQ>
__global__ __launch_bounds__(256) void k_hake_tile_bwd(HakeBwd a, const TC* __restrict__ base, float* __restrict__ dX,
                                                       int64_t b_chunk) {
    constexpr int NVX = XQ ? 5 : 4, NVY = XQ ? 4 : 5, NACC = XQ ? 3 : 2;
    __shared__ __attribute__((aligned(16))) float Ks[2][HKT][HLDP];    // [gm | gl][b][a]
    __shared__ __attribute__((aligned(16))) float Ys[NVY][HKT][HLDP];  // [v][b][w]
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int d = a.d;
    const int64_t nx = XQ ? a.S : a.N, ny = XQ ? a.N : a.S;
    const int64_t a0 = static_cast<int64_t>(blockIdx.y) * 64;
    const int w0 = blockIdx.x * 64;
    // (modulus operands, images, raw phase) of row r of the query side: U, R, sin, cos, Q_p; of the candidate side:
    // c_m, cos, sin, c_p
    auto query_at = [&](int64_t r, int w, bool live, float (&o)[5]) {
        const float* rp = a.Q + r * 3 * d + w;
        const float x = rp[2 * d] * HAKE_REV, l = live ? 1.f : 0.f;
        o[0] = l * rp[0]; o[1] = l * rp[d]; o[2] = l * sin_rev(x); o[3] = l * cos_rev(x); o[4] = l * rp[2 * d];
    };
    auto cand_at = [&](int64_t r, int w, bool live, float (&o)[5]) {
        const TC* rp = base + (a.idx ? static_cast<int64_t>(a.idx[r]) : r) * 2 * d + w;
        const float x = to_f32(rp[0]) * a.ps_rev, l = live ? 1.f : 0.f;
        o[0] = l * to_f32(rp[d]); o[1] = l * cos_rev(x); o[2] = l * sin_rev(x); o[3] = l * to_f32(rp[0]); o[4] = 0.f;
    };
    float xv[NVX][4][4], acc[NACC][4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t r = a0 + ty * 4 + i;
            const int w = w0 + tx * 4 + j;
            float o[5];
            if (XQ) query_at(min(r, nx - 1), min(w, d - 1), r < nx && w < d, o);
            else cand_at(min(r, nx - 1), min(w, d - 1), r < nx && w < d, o);
#pragma unroll
            for (int p = 0; p < NVX; ++p) xv[p][i][j] = o[p];
#pragma unroll
            for (int p = 0; p < NACC; ++p) acc[p][i][j] = 0.f;
        }
    const int64_t b_lo = static_cast<int64_t>(blockIdx.z) * b_chunk;
    const int64_t b_hi = min(b_lo + b_chunk, ny);
    if (b_lo >= b_hi) return;
    const int yb = t >> 4, ywc = (t & 15) * 4;
    float kv[2][4], yv[4][5];
    auto fetch = [&](int64_t b0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int bb, al;  // the score gradient is contiguous in the candidates: in b for XQ, in a otherwise
            if (XQ) { bb = t & 15; al = (t >> 4) + 16 * i; }
            else { al = t & 63; bb = (t >> 6) + 4 * i; }
            const bool ok = a0 + al < nx && b0 + bb < b_hi;
            const int64_t ac = min(a0 + al, nx - 1), bc = min(b0 + bb, b_hi - 1);
            const int64_t q = XQ ? ac : bc, c = XQ ? bc : ac;
            const float g = -a.d_out[q * a.ld_dout + c];
            kv[0][i] = ok ? g * lp_inv(a.norm[q * a.N + c], 2.f) : 0.f;
            kv[1][i] = ok ? g * a.lp * 0.5f : 0.f;
        }
        const int64_t b = min(b0 + yb, b_hi - 1);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int w = w0 + ywc + i;
            if (XQ) cand_at(b, min(w, d - 1), w < d, yv[i]);
            else query_at(b, min(w, d - 1), w < d, yv[i]);
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                if (XQ) Ks[p][t & 15][(t >> 4) + 16 * i] = kv[p][i];
                else Ks[p][(t >> 6) + 4 * i][t & 63] = kv[p][i];
            }
#pragma unroll
        for (int p = 0; p < NVY; ++p)
            *reinterpret_cast<float4*>(&Ys[p][yb][ywc]) = make_float4(yv[0][p], yv[1][p], yv[2][p], yv[3][p]);
    };
    fetch(b_lo);
    for (int64_t b0 = b_lo; b0 < b_hi; b0 += HKT) {
        stash();
        __syncthreads();
        if (b0 + HKT < b_hi) fetch(b0 + HKT);
#pragma unroll 1
        for (int k = 0; k < HKT; ++k) {
            const float4 g4 = *reinterpret_cast<const float4*>(&Ks[0][k][ty * 4]);
            const float4 l4 = *reinterpret_cast<const float4*>(&Ks[1][k][ty * 4]);
            const float gm[4] = {g4.x, g4.y, g4.z, g4.w}, gl[4] = {l4.x, l4.y, l4.z, l4.w};
            float y[NVY][4];
#pragma unroll
            for (int p = 0; p < NVY; ++p) {
                const float4 t4 = *reinterpret_cast<const float4*>(&Ys[p][k][tx * 4]);
                y[p][0] = t4.x; y[p][1] = t4.y; y[p][2] = t4.z; y[p][3] = t4.w;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float U = XQ ? xv[0][i][j] : y[0][j], R = XQ ? xv[1][i][j] : y[1][j];
                    const float sa = XQ ? xv[2][i][j] : y[2][j], ca = XQ ? xv[3][i][j] : y[3][j];
                    const float cm = XQ ? y[0][j] : xv[0][i][j], cb = XQ ? y[1][j] : xv[1][i][j];
                    const float sb = XQ ? y[2][j] : xv[2][i][j];
                    const float qp = XQ ? xv[4][i][j] : y[4][j], cp = XQ ? y[3][j] : xv[3][i][j];
                    const float dm = gm[i] * fmaf(U, cm, R);
                    const float sn = fmaf(-ca, sb, sa * cb), cs = fmaf(sa, sb, ca * cb);
                    float sg = sgn_prescaled(sn * SGN_PRESCALE);
                    if (fabsf(sn) < HAKE_SIGN_EPS) sg = hake_sign_exact(fmaf(-a.ps, cp, qp));
                    const float dp = gl[i] * sg * cs;
                    if (XQ) {
                        acc[0][i][j] = fmaf(dm, cm, acc[0][i][j]);
                        acc[1][i][j] += dm;
                        acc[2][i][j] += dp;
                    } else {
                        acc[0][i][j] = fmaf(-a.ps, dp, acc[0][i][j]);
                        acc[1][i][j] = fmaf(dm, U, acc[1][i][j]);
                    }
                }
        }
        __syncthreads();
    }
    const int64_t ldx = static_cast<int64_t>(NACC) * d;
#pragma unroll
    for (int p = 0; p < NACC; ++p)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t r = a0 + ty * 4 + i;
            if (r >= nx) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int w = w0 + tx * 4 + j;
                if (w < d) {
                    float* o = dX + r * ldx + p * d + w;
                    if (gridDim.z == 1) *o = acc[p][i][j];
                    else unsafeAtomicAdd(o, acc[p][i][j]);
                }
            }
        }
}

template <typename TC, bool XQ>
static int hake_bwd_launch(const HakeBwd& a, const TC* base, float* dX, hipStream_t st) {
    const int64_t nx = XQ ? a.S : a.N, ny = XQ ? a.N : a.S;
    const int64_t tiles = ceil_div(a.d, 64) * ceil_div(nx, 64);
    int64_t split = 1;
    while (tiles * split < 1024 && ceil_div(ny, split * 2) >= 4 * HKT) split *= 2;
    const int64_t chunk = ceil_div(ceil_div(ny, split), HKT) * HKT;
    split = ceil_div(ny, chunk);
    if (split > 1) {
        hipError_t e = fill_words_async(dX, 0u, nx * (XQ ? 3 : 2) * a.d, st);
        if (e != hipSuccess) return fail(static_cast<int>(e), "memset: %s", hipGetErrorString(e));
    }
    const dim3 grid(static_cast<unsigned>(ceil_div(a.d, 64)), static_cast<unsigned>(ceil_div(nx, 64)),
                    static_cast<unsigned>(split));
    k_hake_tile_bwd<TC, XQ><<<grid, 256, 0, st>>>(a, base, dX, chunk);
    return BESS_OK;
}

// bytes of scratch the tile backward wants (the norms [S, N]); 0: the row form runs, which needs none
int64_t hake_shared_bwd_workspace(const bess_model_desc* d, int64_t S, int64_t N) {
    return hake_tile_takes(d, S) && ceil_div(N, 64) < 65536 ? S * N * 4 : 0;
}

// d_query [S, 3 d] and d_cand [N, 2 d] over shared candidates: the tile kernels through the workspace, or (no
// workspace, BESS_FLAG_FP32_MATH, more row tiles than a grid's y takes) the row form
int hake_shared_bwd(const bess_model_desc* d, const float* query, int64_t S, const void* base, const int32_t* idx,
                    int64_t N, const float* d_out, int64_t ld_dout, float* dq, float* dn, void* ws, int64_t ws_bytes,
                    hipStream_t st) {
    const int64_t want = hake_shared_bwd_workspace(d, S, N);
    if (want == 0 || !ws || ws_bytes < want || reinterpret_cast<uintptr_t>(ws) % 16 != 0)
        return hake_rows(d, false, true, query, S, base, idx, N, nullptr, d_out, ld_dout, dq, dn, st, nullptr, nullptr);
    float* norm = static_cast<float*>(ws);
    if (int e = hake_tile_fwd(d, query, S, base, idx, N, norm, N, nullptr, nullptr, false, st, true)) return e;
    const float scale = float_of_bits(d->reserved[2]);
    const HakeBwd a{query, S, idx, N, d->width / 2, d_out, ld_dout, norm, float_of_bits(d->reserved[1]), scale,
                    scale * HAKE_REV};
    const int rc = with_table_type(d->dtype, [&](auto t) {
        using T = decltype(t);
        const T* b = static_cast<const T*>(base);
        if (int e = hake_bwd_launch<T, true>(a, b, dq, st)) return e;
        return hake_bwd_launch<T, false>(a, b, dn, st);
    });
    return rc ? rc : check_launch("neg_score_shared_bwd (HAKE)");
}

int hake_negatives(const bess_model_desc* d, bool fwd, bool shared, const float* query, int64_t n_query,
                   const void* neg_base, const int32_t* neg_idx, int64_t n_neg, float* out, const float* d_out,
                   int64_t ld, float* dq, float* dn, hipStream_t st, const float* thr, const CountArgs* count) {
    BESS_REQUIRE(!count || (fwd && shared && thr), "HAKE: counting is a forward over shared candidates");
    if (fwd && shared && hake_tile_takes(d, n_query))
        return hake_tile_fwd(d, query, n_query, neg_base, neg_idx, n_neg, out, ld, thr, count, false, st);
    return hake_rows(d, fwd, shared, query, n_query, neg_base, neg_idx, n_neg, out, d_out, ld, dq, dn, st, thr, count);
}

// out[i] = score(query[i], candidate idx[i]) in the arithmetic hake_negatives' shared forward uses for these flags:
// the tile kernel's diagonal, or the row form with one candidate per query
int hake_pairs(const bess_model_desc* d, const float* query, const void* neg_base, const int32_t* neg_idx, int64_t n_pair,
               float* out, hipStream_t st) {
    BESS_REQUIRE(neg_idx, "HAKE: pair scores take one indexed candidate per query");
    if (hake_tile_takes(d, n_pair))
        return hake_tile_fwd(d, query, n_pair, neg_base, neg_idx, n_pair, out, 0, nullptr, nullptr, true, st);
    return hake_rows(d, true, false, query, n_pair, neg_base, neg_idx, 1, out, nullptr, 1, nullptr, nullptr, st, nullptr,
                     nullptr);
}

}  // namespace bess
