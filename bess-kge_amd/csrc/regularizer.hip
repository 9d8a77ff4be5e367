// Embedding regulariser of the training step on gfx950: the Lp / N3 penalty on the rows of the positive triples
// (Lacroix et al. 2018, the per-triple "weighted" form), its value and its gradient in ONE launch behind the backward.
//
//   term_i = c_i * (entity_coef * (Phi(h_i) + Phi(t_i)) + relation_coef * Phi_r(r_i)),   c_i = loss_scale * weight_i
//   Phi(x) = sum_k |x_k|^p, or over the d = W / 2 complex coordinates (x_k, x_{d+k}): sum_k (re_k^2 + im_k^2)^(p/2)
//
// One wavefront per triple, a lane per 16-byte chunk of the head and tail rows (column passes of 64 chunks: rows of
// any width).  The gradient is ADDED to the triple's rows of d_head / d_tail - the dense [n_triple, W] arrays every
// backward of the step leaves - and to the relation gradient with fp32 atomics; the update lists behind them stay what
// they were.  The relation row (a few rows, L2 resident) is read a scalar per lane, lane-contiguous, so that every
// atomic wave-instruction adds 256 contiguous bytes of one row - the shape k_query_triple_bwd issues them in.  The
// row terms are summed by the launch's last workgroup in a fixed order (bitwise reproducible), which also adds the
// penalty to the step's loss scalar.  No LDS besides that sum.
#include <math.h>

#include <algorithm>

#include "common.h"

namespace bess {

struct RegArgs {
    const void* head_base;
    const int32_t* head_idx;
    const void* tail_base;
    const int32_t* tail_idx;
    const void* rel_table;  // NULL: no relation term (relation_coef == 0)
    const int32_t* rel_idx;
    int64_t n;
    int W, Wr;
    int nch_e;   // chunks of VEC scalars per entity row (per half of the row under its modulus flag)
    int unit_r;  // scalars per relation row (per half of it under its modulus flag)
    const float* weight;
    int64_t weight_len;
    float p, entity_coef, relation_coef, loss_scale;
    float* d_head;
    float* d_tail;
    float* d_rel;
    float* row_terms;
    float* penalty;
    float* loss_inout;
    float loss_factor;
    int32_t* ticket;
};

// |x|^p and its derivative over p, sgn(x) |x|^(p-1) (0 at x == 0), of one coordinate - or, MOD, of one complex
// coordinate (re, im): m^p and m^(p-2) * (re, im), 0 at m == 0.  p is uniform over the launch: p = 1, 2, 3 are
// multiplies (and one sqrt for a modulus), every other p goes through powf (the idiom of lp_term / lp_dterm).
template <bool MOD>
__device__ __forceinline__ float reg_elem(float re, float im, float p, float& g_re, float& g_im) {
    if (MOD) {
        const float m2 = re * re + im * im;
        float term, f;
        if (p == 2.f) {
            term = m2, f = 1.f;
        } else {
            const float m = sqrtf(m2);
            if (p == 3.f) term = m2 * m, f = m;
            else if (p == 1.f) term = m, f = m > 0.f ? 1.f / m : 0.f;
            else term = powf(m, p), f = m > 0.f ? powf(m, p - 2.f) : 0.f;
        }
        g_re = f * re, g_im = f * im;
        return term;
    }
    const float a = fabsf(re);
    g_im = 0.f;
    if (p == 2.f) return g_re = re, re * re;
    if (p == 3.f) return g_re = re * a, a * a * a;
    if (p == 1.f) return g_re = sgnf(re), a;
    g_re = a > 0.f ? copysignf(powf(a, p - 1.f), re) : 0.f;
    return powf(a, p);
}

// VEC gradient scalars at p, in accesses of up to 16 bytes
template <int VEC>
__device__ __forceinline__ void load_grad(const float* __restrict__ p, float (&v)[VEC]) {
    constexpr int GV = VEC < 4 ? VEC : 4;
#pragma unroll
    for (int k = 0; k < VEC; k += GV) VecLoad<float, GV>::load(p + k, reinterpret_cast<float (&)[GV]>(v[k]));
}
template <int VEC>
__device__ __forceinline__ void store_grad(float* __restrict__ p, const float (&v)[VEC]) {
    constexpr int GV = VEC < 4 ? VEC : 4;
    typedef float vec_t __attribute__((ext_vector_type(GV)));
#pragma unroll
    for (int k = 0; k < VEC; k += GV) {
        if constexpr (GV == 1) {
            p[k] = v[k];
        } else {
            vec_t o;
#pragma unroll
            for (int j = 0; j < GV; ++j) o[j] = v[k + j];
            *reinterpret_cast<vec_t*>(p + k) = o;
        }
    }
}

// One row of the triple in one column pass: the lane's chunk (both halves of it under MOD), loaded at a clamped
// address whether the lane has a chunk in this pass or not.
template <typename T, int VEC, bool MOD>
struct RowChunk {
    float re[VEC], im[VEC];
    __device__ __forceinline__ void load(const T* __restrict__ row, int c, int nch) {
        load_chunk_clamped<T, VEC>(row, c, nch, re);
        if (MOD) load_chunk_clamped<T, VEC>(row + nch * VEC, c, nch, im);
    }
};
template <int VEC, bool MOD>
struct GradChunk {
    float re[VEC], im[VEC];
    __device__ __forceinline__ void load(const float* __restrict__ row, int c, int nch) {
        const int at = min(c, nch - 1) * VEC;
        load_grad<VEC>(row + at, re);
        if (MOD) load_grad<VEC>(row + nch * VEC + at, im);
    }
    __device__ __forceinline__ void store(float* __restrict__ row, int c, int nch) const {
        store_grad<VEC>(row + c * VEC, re);
        if (MOD) store_grad<VEC>(row + nch * VEC + c * VEC, im);
    }
};

// Phi of the lane's chunk, added to acc; with GRAD the chunk's gradient gs * dPhi is added into g
template <typename T, int VEC, bool MOD, bool GRAD>
__device__ __forceinline__ void reg_chunk(const RowChunk<T, VEC, MOD>& x, float p, float gs, float& acc,
                                          GradChunk<VEC, MOD>& g) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        float g_re, g_im;
        acc += reg_elem<MOD>(x.re[k], MOD ? x.im[k] : 0.f, p, g_re, g_im);
        if (GRAD) {
            g.re[k] += gs * g_re;
            if (MOD) g.im[k] += gs * g_im;
        }
    }
}

// ME / MR: entity / relation rows are [re(d) | im(d)] and their moduli are penalised.  GRAD: d_head / d_tail (and
// d_rel) are given.  A wave takes the triples s = wave, wave + waves of the grid, ...
template <typename T, int VEC, bool ME, bool MR, bool GRAD>
__global__ __launch_bounds__(256) void k_regularize_triples(RegArgs a) {
    __shared__ float part[256];
    __shared__ int last;
    const int lane = threadIdx.x & 63;
    const int64_t waves = 4ll * gridDim.x;
    const bool has_rel = a.rel_table != nullptr;
    // (without a relation term the relation loads read the head row's first scalar: a valid address, never used)
    const int unit_r = has_rel ? a.unit_r : 1;
    const int n_pass = max((a.nch_e + 63) >> 6, has_rel ? (a.unit_r + 64 * VEC - 1) / (64 * VEC) : 0);
    for (int64_t s = blockIdx.x * 4ll + (threadIdx.x >> 6); s < a.n; s += waves) {
        const T* h = row_ptr(static_cast<const T*>(a.head_base), a.head_idx, s, a.W);
        const T* t = row_ptr(static_cast<const T*>(a.tail_base), a.tail_idx, s, a.W);
        const int64_t rid = has_rel ? static_cast<int64_t>(a.rel_idx[s]) : 0;
        const T* r = has_rel ? static_cast<const T*>(a.rel_table) + rid * a.Wr : h;
        const float c = a.loss_scale * a.weight[a.weight_len == 1 ? 0 : s];
        const float gs_e = c * a.entity_coef * a.p, gs_r = c * a.relation_coef * a.p;
        float* dh = GRAD ? a.d_head + s * a.W : nullptr;
        float* dt = GRAD ? a.d_tail + s * a.W : nullptr;
        float* dr = GRAD && has_rel ? a.d_rel + rid * a.Wr : nullptr;
        float acc_e = 0.f, acc_r = 0.f;
        for (int pass = 0; pass < n_pass; ++pass) {
            const int ch = pass * 64 + lane;
            // every load of the pass is issued before the first use
            RowChunk<T, VEC, ME> xh, xt;
            GradChunk<VEC, ME> gh, gt;
            float r_re[VEC], r_im[VEC];
            xh.load(h, ch, a.nch_e);
            xt.load(t, ch, a.nch_e);
            const int e0 = pass * 64 * VEC + lane;  // the pass's relation scalars e0 + 64 k
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const int e = min(e0 + 64 * k, unit_r - 1);
                r_re[k] = to_f32(r[e]);
                r_im[k] = MR ? to_f32(r[unit_r + e]) : 0.f;
            }
            if (GRAD) {
                gh.load(dh, ch, a.nch_e);
                gt.load(dt, ch, a.nch_e);
            }
            const bool live_e = ch < a.nch_e;
            float pe = 0.f;
            reg_chunk<T, VEC, ME, GRAD>(xh, a.p, gs_e, pe, gh);
            reg_chunk<T, VEC, ME, GRAD>(xt, a.p, gs_e, pe, gt);
            acc_e += live_e ? pe : 0.f;
            if (GRAD && live_e) {
                gh.store(dh, ch, a.nch_e);
                gt.store(dt, ch, a.nch_e);
            }
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const int e = e0 + 64 * k;
                const bool live_r = has_rel && e < a.unit_r;
                float g_re, g_im;
                const float term = reg_elem<MR>(r_re[k], r_im[k], a.p, g_re, g_im);
                acc_r += live_r ? term : 0.f;
                if (GRAD && live_r) {
                    g_re *= gs_r, g_im *= gs_r;
                    if (g_re != 0.f) unsafeAtomicAdd(dr + e, g_re);
                    if (MR && g_im != 0.f) unsafeAtomicAdd(dr + a.unit_r + e, g_im);
                }
            }
        }
        acc_e = wave_allreduce_sum(acc_e);
        acc_r = wave_allreduce_sum(acc_r);
        if (lane == 0) store_agent(a.row_terms + s, c * (a.entity_coef * acc_e + a.relation_coef * acc_r));
    }
    // the last workgroup sums the row terms: thread i the terms i, i + 256, ... in order, then a tree over the threads
    release_to_agent();
    __syncthreads();
    if (threadIdx.x == 0) last = last_workgroup_ticket(a.ticket);
    __syncthreads();
    if (!last) return;
    part[threadIdx.x] = strided_sum_agent(a.row_terms, a.n, threadIdx.x, 256);
    __syncthreads();
    for (int hf = 128; hf > 0; hf >>= 1) {
        if (threadIdx.x < hf) part[threadIdx.x] += part[threadIdx.x + hf];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        a.penalty[0] = part[0];
        if (a.loss_inout) a.loss_inout[0] += a.loss_factor * part[0];
    }
}

// the row classes of the native family, without the iterations axis: the column passes are a run-time loop
struct PassRows : NativeRows {
    using its = Ints<1>;
};

// The widest vector of the table type's classes that divides the entity rows' unit (a half of the row under the modulus
// flag) and that every pointer is aligned for (gradient rows: accesses of min(vec, 4) floats).
static int reg_vec_of(int dtype, int unit_e, const void* const* rows, int n_rows, const float* const* grads, int n_grads) {
    const int sz = dtype == BESS_F32 ? 4 : 2;
    for (int vec : {8, 4, 2}) {
        if ((dtype == BESS_F32 && vec != 4) || (dtype == BESS_F16 && vec == 4)) continue;
        bool ok = unit_e % vec == 0;
        for (int i = 0; i < n_rows; ++i) ok = ok && reinterpret_cast<uintptr_t>(rows[i]) % (vec * sz) == 0;
        for (int i = 0; i < n_grads; ++i) ok = ok && reinterpret_cast<uintptr_t>(grads[i]) % (4 * std::min(vec, 4)) == 0;
        if (ok) return vec;
    }
    return 1;
}

}  // namespace bess

using namespace bess;

extern "C" int bess_regularize_triples(const bess_model_desc* d, const void* head_base, const int32_t* head_idx,
                                       const void* tail_base, const int32_t* tail_idx, const void* rel_table,
                                       const int32_t* rel_idx, int64_t n_triple, const float* weight, int64_t weight_len,
                                       float p, float entity_coef, float relation_coef, float loss_scale, int32_t flags,
                                       float* d_head, float* d_tail, float* d_rel_table, float* row_terms, float* penalty,
                                       float* loss_inout, float loss_factor, int32_t* ticket, void* stream) {
    BESS_REQUIRE(d, "regularize_triples: NULL descriptor");
    BESS_REQUIRE(d->dtype == BESS_F32 || d->dtype == BESS_F16, "regularize_triples: unknown dtype %d", d->dtype);
    BESS_REQUIRE(d->width > 0 && d->rel_width > 0, "regularize_triples: non-positive width %d / %d", d->width, d->rel_width);
    BESS_REQUIRE(n_triple > 0, "regularize_triples: bad sizes");
    BESS_REQUIRE(p >= 1.f && p < INFINITY, "regularize_triples: p = %g is not a finite p >= 1", static_cast<double>(p));
    BESS_REQUIRE(entity_coef >= 0.f && relation_coef >= 0.f && entity_coef < INFINITY && relation_coef < INFINITY,
                 "regularize_triples: coefficients %g / %g must be finite and >= 0", static_cast<double>(entity_coef),
                 static_cast<double>(relation_coef));
    BESS_REQUIRE((flags & ~(BESS_REG_ENTITY_MODULUS | BESS_REG_RELATION_MODULUS)) == 0, "regularize_triples: unknown flags %d",
                 flags);
    const bool mod_e = flags & BESS_REG_ENTITY_MODULUS, rel = relation_coef > 0.f;
    const bool mod_r = rel && (flags & BESS_REG_RELATION_MODULUS);
    BESS_REQUIRE(!(mod_e && d->width % 2), "regularize_triples: moduli of entity rows of odd width %d", d->width);
    BESS_REQUIRE(!((flags & BESS_REG_RELATION_MODULUS) && d->rel_width % 2),
                 "regularize_triples: moduli of relation rows of odd width %d", d->rel_width);
    BESS_REQUIRE(weight_len == 1 || weight_len == n_triple, "regularize_triples: weight_len must be 1 or n_triple");
    BESS_REQUIRE((d_head == nullptr) == (d_tail == nullptr), "regularize_triples: d_head and d_tail come together (both "
                                                             "NULL: value only)");
    const bool grad = d_head != nullptr;
    BESS_REQUIRE(head_base && tail_base && weight && row_terms && penalty && ticket, "regularize_triples: NULL pointer");
    BESS_REQUIRE(!rel || (rel_table && rel_idx), "regularize_triples: relation_coef > 0 needs the relation rows");
    BESS_REQUIRE(!(rel && grad) || d_rel_table, "regularize_triples: relation_coef > 0 needs d_rel_table");

    const int unit_e = mod_e ? d->width / 2 : d->width;
    const int unit_r = mod_r ? d->rel_width / 2 : d->rel_width;
    const void* rows[2] = {head_base, tail_base};
    const float* grads[2] = {d_head, d_tail};
    const int vec = reg_vec_of(d->dtype, unit_e, rows, 2, grads, grad ? 2 : 0);
    RegArgs a{head_base, head_idx, tail_base, tail_idx, rel ? rel_table : nullptr, rel_idx, n_triple, d->width,
              d->rel_width, unit_e / vec, unit_r, weight, weight_len, p, entity_coef, rel ? relation_coef : 0.f,
              loss_scale, d_head, d_tail, grad && rel ? d_rel_table : nullptr, row_terms, penalty, loss_inout, loss_factor,
              ticket};
    // four triples per workgroup; beyond 4096 workgroups the waves stride (one ticket per workgroup: common.h)
    const unsigned grid = static_cast<unsigned>(std::min<int64_t>(ceil_div(n_triple, 4), 4096));
    const bool known = dispatch_row_class<PassRows>(d->dtype, vec, 1, [&](auto rc) {
        using RC = decltype(rc);
        with_flag(mod_e, [&](auto me) {
            with_flag(mod_r, [&](auto mr) {
                with_flag(grad, [&](auto g) {
                    k_regularize_triples<typename RC::T, RC::VEC, decltype(me)::value, decltype(mr)::value, decltype(g)::value>
                        <<<grid, 256, 0, as_stream(stream)>>>(a);
                });
            });
        });
    });
    if (!known) return fail(BESS_EUNSUPPORTED, "regularize_triples: no row class for vec %d", vec);
    return check_launch("regularize_triples");
}
