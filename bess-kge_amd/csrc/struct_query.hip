// The structured bilinear query transform and its backward: QuatE, SimplE, CP, ANALOGY, AutoSF - and DistMult and
// ComplEx - from one term table.  Entity rows are K blocks of d columns, relation rows Kr blocks;
//
//     score(h, r, t) = sum over terms (i, j, k, c) of  c * sum_x h[i d + x] r[j d + x] t[k d + x]
//
// is bilinear in the candidate, so only the query and its gradients are new; candidates meet DistMult's kernels.
// The host turns the term list into a dense coefficient tensor C[a][j][o] over (kept-entity block, relation block,
// query block) - for head corruption with a and o exchanged, so the kernels know no side:
//
//     q[o d + x] = sum_{a, j} C[a][j][o] e[a d + x] r[j d + x]
//
// C travels by value in the kernel arguments: every coefficient is a uniform (scalar) load with a compile-time
// offset, a zero coefficient is a scalar branch around its multiply-add.  Block counts are rounded up to KB in
// {1, 2, 4, 8}; blocks that do not exist are never loaded.
//
//   k_struct_fwd        a lane owns VEC columns x of one triple and holds the K + Kr blocks of those columns in
//                       registers: one pass over the operands, the term list is register arithmetic, and the unit
//                       norm of the relation (over its Kr blocks, per column) needs no other lane.  A triple takes
//                       gs = min(d / VEC, 256) neighbouring threads, a workgroup 256 / gs triples: narrow blocks
//                       keep several triples in flight per wave.  pos = <q, other row>: partial sums per thread,
//                       a tree over the triple's threads in LDS, in a fixed order
//   k_struct_bwd_rows   the same layout: d_ent, and d_other = d_pos q, of every triple
//   k_struct_bwd_rel    one workgroup walks one relation segment of the batch (grouped by the caller's segment
//                       index): 256 / lpr triples in flight, lpr = the threads one row takes; per-thread sums in
//                       walk order, then a tree over the triples in flight in LDS.  A segment of more than
//                       SHORT_SEG triples is cut into N_SHARE shares, one workgroup each, whose partial rows go to
//                       the workspace; k_struct_merge adds them in share order.  The Jacobian of the unit norm is
//                       linear in the summed gradient and applied once per share.  No atomics: a relation's
//                       columns have one owner.
#include "common.h"

namespace bess {
namespace {

constexpr int SHORT_SEG = 32;  // segments up to this many triples: one workgroup, added into d_rel directly
constexpr int N_SHARE = 16;    // shares of a longer segment

template <int KB>
struct Coef {
    float c[KB * KB * KB];  // [a][j][o]
};
__device__ __forceinline__ bool nonzero(float c) { return (__builtin_bit_cast(uint32_t, c) << 1) != 0u; }

struct StructArgs {
    const void *ent, *other, *rel;  // rows of the table type; other NULL: no positive score
    const int32_t *ent_idx, *other_idx, *rel_idx;
    int64_t ld_ent, ld_other, ld_rel;
    float* q;  // forward
    float* pos;
    const float* dq;  // backward (either may be NULL)
    const float* d_pos;
    float *d_ent, *d_other, *d_rel;
    int64_t ldq, lddq, ld_dent, ld_dother, ld_drel;
    const int32_t *refs, *seg_rows, *seg_offsets, *n_seg;
    float* ws;
    int64_t S;
    int d, K, Kr, nch;  // nch: chunks of VEC columns per block
    int gs, rows_per_wg;  // row kernels: threads per triple, triples per workgroup
    int lpr_log2;         // relation kernel: log2 of the threads per row
    int norm;
};

template <typename T>
__device__ __forceinline__ const T* src_row(const void* base, const int32_t* idx, int64_t ld, int64_t i) {
    return static_cast<const T*>(base) + (idx ? static_cast<int64_t>(idx[i]) : i) * ld;
}

template <typename T, int VEC, int KB>
__device__ __forceinline__ void load_blocks(const T* __restrict__ row, int nb, int d, int col, float (&v)[KB][VEC]) {
#pragma unroll
    for (int b = 0; b < KB; ++b) {
        if (b < nb) {
            VecLoad<T, VEC>::load(row + static_cast<int64_t>(b) * d + col, v[b]);
        } else {
#pragma unroll
            for (int x = 0; x < VEC; ++x) v[b][x] = 0.f;
        }
    }
}

template <int VEC, int KB>
__device__ __forceinline__ void store_blocks(float* __restrict__ row, int nb, int d, int col, const float (&v)[KB][VEC]) {
    typedef float vec_t __attribute__((ext_vector_type(VEC)));
#pragma unroll
    for (int b = 0; b < KB; ++b) {
        if (b < nb) {
            if constexpr (VEC == 1) {
                row[static_cast<int64_t>(b) * d + col] = v[b][0];
            } else {
                vec_t o;
#pragma unroll
                for (int x = 0; x < VEC; ++x) o[x] = v[b][x];
                *reinterpret_cast<vec_t*>(row + static_cast<int64_t>(b) * d + col) = o;
            }
        }
    }
}

// r <- r / |r| per column, the norm over the relation's blocks; inv = 1 / |r| (correctly rounded root and quotients)
template <int VEC, int KB>
__device__ __forceinline__ void unit_norm(float (&r)[KB][VEC], float (&inv)[VEC]) {
#pragma unroll
    for (int x = 0; x < VEC; ++x) {
        float n2 = 0.f;
#pragma unroll
        for (int j = 0; j < KB; ++j) n2 = fmaf(r[j][x], r[j][x], n2);
        const float n = sqrtf(n2);
        inv[x] = 1.f / n;
#pragma unroll
        for (int j = 0; j < KB; ++j) r[j][x] = r[j][x] / n;
    }
}

// q[o] += C[a][j][o] e[a] r[j]
template <int VEC, int KB>
__device__ __forceinline__ void query_terms(const Coef<KB>& C, const float (&e)[KB][VEC], const float (&r)[KB][VEC],
                                            float (&q)[KB][VEC]) {
#pragma unroll
    for (int a = 0; a < KB; ++a)
#pragma unroll
        for (int j = 0; j < KB; ++j) {
            float p[VEC];
#pragma unroll
            for (int x = 0; x < VEC; ++x) p[x] = e[a][x] * r[j][x];
#pragma unroll
            for (int o = 0; o < KB; ++o) {
                const float cf = C.c[(a * KB + j) * KB + o];
                if (nonzero(cf)) {
#pragma unroll
                    for (int x = 0; x < VEC; ++x) q[o][x] = fmaf(cf, p[x], q[o][x]);
                }
            }
        }
}

// g[o] = dq[o] + d_pos other[o]  (either part may be absent)
template <typename T, int VEC, int KB>
__device__ __forceinline__ void load_query_grad(const StructArgs& A, int64_t s, int col, float dp, float (&g)[KB][VEC]) {
    if (A.dq) {
        load_blocks<float, VEC, KB>(A.dq + s * A.lddq, A.K, A.d, col, g);
    } else {
#pragma unroll
        for (int o = 0; o < KB; ++o)
#pragma unroll
            for (int x = 0; x < VEC; ++x) g[o][x] = 0.f;
    }
    if (A.d_pos) {
        float ot[KB][VEC];
        load_blocks<T, VEC, KB>(src_row<T>(A.other, A.other_idx, A.ld_other, s), A.K, A.d, col, ot);
#pragma unroll
        for (int o = 0; o < KB; ++o)
#pragma unroll
            for (int x = 0; x < VEC; ++x) g[o][x] = fmaf(dp, ot[o][x], g[o][x]);
    }
}

template <typename T, int VEC, int KB>
__global__ __launch_bounds__(256) void k_struct_fwd(StructArgs A, Coef<KB> C) {
    __shared__ float red[256];
    const int t = threadIdx.x, g = t / A.gs, c0 = t - g * A.gs;
    const int64_t s = static_cast<int64_t>(blockIdx.x) * A.rows_per_wg + g;
    const bool in_group = g < A.rows_per_wg, live = in_group && s < A.S;
    float part = 0.f;
    if (live) {
        const T* const erow = src_row<T>(A.ent, A.ent_idx, A.ld_ent, s);
        const T* const rrow = static_cast<const T*>(A.rel) + static_cast<int64_t>(A.rel_idx[s]) * A.ld_rel;
        const T* const orow = A.pos ? src_row<T>(A.other, A.other_idx, A.ld_other, s) : nullptr;
        float* const qrow = A.q + s * A.ldq;
        for (int c = c0; c < A.nch; c += A.gs) {
            const int col = c * VEC;
            float e[KB][VEC], r[KB][VEC], q[KB][VEC], inv[VEC];
            load_blocks<T, VEC, KB>(erow, A.K, A.d, col, e);
            load_blocks<T, VEC, KB>(rrow, A.Kr, A.d, col, r);
            if (A.norm) unit_norm<VEC, KB>(r, inv);
#pragma unroll
            for (int o = 0; o < KB; ++o)
#pragma unroll
                for (int x = 0; x < VEC; ++x) q[o][x] = 0.f;
            query_terms<VEC, KB>(C, e, r, q);
            store_blocks<VEC, KB>(qrow, A.K, A.d, col, q);
            if (orow) {
                float ot[KB][VEC];
                load_blocks<T, VEC, KB>(orow, A.K, A.d, col, ot);
#pragma unroll
                for (int o = 0; o < KB; ++o)
#pragma unroll
                    for (int x = 0; x < VEC; ++x) part = fmaf(q[o][x], ot[o][x], part);
            }
        }
    }
    if (A.pos) {  // the triple's threads, in a fixed order
        red[t] = part;
        __syncthreads();
        for (int off = 128; off >= 1; off >>= 1) {
            if (in_group && c0 < off && c0 + off < A.gs) red[t] += red[t + off];
            __syncthreads();
        }
        if (live && c0 == 0) A.pos[s] = red[t];
    }
}

template <typename T, int VEC, int KB>
__global__ __launch_bounds__(256) void k_struct_bwd_rows(StructArgs A, Coef<KB> C) {
    const int t = threadIdx.x, g = t / A.gs, c0 = t - g * A.gs;
    const int64_t s = static_cast<int64_t>(blockIdx.x) * A.rows_per_wg + g;
    if (g >= A.rows_per_wg || s >= A.S) return;
    const T* const erow = src_row<T>(A.ent, A.ent_idx, A.ld_ent, s);
    const T* const rrow = static_cast<const T*>(A.rel) + static_cast<int64_t>(A.rel_idx[s]) * A.ld_rel;
    const float dp = A.d_pos ? A.d_pos[s] : 0.f;
    for (int c = c0; c < A.nch; c += A.gs) {
        const int col = c * VEC;
        float e[KB][VEC], r[KB][VEC], gq[KB][VEC], de[KB][VEC], q[KB][VEC], inv[VEC];
        load_blocks<T, VEC, KB>(erow, A.K, A.d, col, e);
        load_blocks<T, VEC, KB>(rrow, A.Kr, A.d, col, r);
        if (A.norm) unit_norm<VEC, KB>(r, inv);
        load_query_grad<T, VEC, KB>(A, s, col, dp, gq);
#pragma unroll
        for (int o = 0; o < KB; ++o)
#pragma unroll
            for (int x = 0; x < VEC; ++x) de[o][x] = q[o][x] = 0.f;
        // d_e[a] += C[a][j][o] r[j] g[o]
#pragma unroll
        for (int j = 0; j < KB; ++j)
#pragma unroll
            for (int o = 0; o < KB; ++o) {
                float p[VEC];
#pragma unroll
                for (int x = 0; x < VEC; ++x) p[x] = r[j][x] * gq[o][x];
#pragma unroll
                for (int a = 0; a < KB; ++a) {
                    const float cf = C.c[(a * KB + j) * KB + o];
                    if (nonzero(cf)) {
#pragma unroll
                        for (int x = 0; x < VEC; ++x) de[a][x] = fmaf(cf, p[x], de[a][x]);
                    }
                }
            }
        store_blocks<VEC, KB>(A.d_ent + s * A.ld_dent, A.K, A.d, col, de);
        if (A.d_other) {
            query_terms<VEC, KB>(C, e, r, q);
#pragma unroll
            for (int o = 0; o < KB; ++o)
#pragma unroll
                for (int x = 0; x < VEC; ++x) q[o][x] *= dp;
            store_blocks<VEC, KB>(A.d_other + s * A.ld_dother, A.K, A.d, col, q);
        }
    }
}

// grid (segment bound, N_SHARE, windows of lpr chunks)
template <typename T, int VEC, int KB>
__global__ __launch_bounds__(256) void k_struct_bwd_rel(StructArgs A, Coef<KB> C) {
    __shared__ float red[KB * VEC * 256];
    const int seg = blockIdx.x, sh = blockIdx.y;
    if (seg >= *A.n_seg) return;
    const int first = A.seg_offsets[seg], L = A.seg_offsets[seg + 1] - first;
    const bool cut = L > SHORT_SEG;
    if (!cut && sh) return;
    const int r0 = cut ? static_cast<int>(static_cast<int64_t>(L) * sh / N_SHARE) : 0;
    const int r1 = cut ? static_cast<int>(static_cast<int64_t>(L) * (sh + 1) / N_SHARE) : L;
    const int t = threadIdx.x, lpr = 1 << A.lpr_log2, G = 256 >> A.lpr_log2;
    const int g = t >> A.lpr_log2, c = static_cast<int>(blockIdx.z) * lpr + (t & (lpr - 1));
    const bool live = c < A.nch;
    const int col = min(c, A.nch - 1) * VEC;  // (lanes past the row: a valid address, nothing stored)
    const int64_t rel_row = A.seg_rows[seg];
    float r[KB][VEC], acc[KB][VEC], inv[VEC];
    load_blocks<T, VEC, KB>(static_cast<const T*>(A.rel) + rel_row * A.ld_rel, A.Kr, A.d, col, r);
    if (A.norm) unit_norm<VEC, KB>(r, inv);
#pragma unroll
    for (int j = 0; j < KB; ++j)
#pragma unroll
        for (int x = 0; x < VEC; ++x) acc[j][x] = 0.f;
    for (int i = r0 + g; i < r1; i += G) {
        const int64_t s = A.refs[first + i];
        float e[KB][VEC], gq[KB][VEC];
        load_blocks<T, VEC, KB>(src_row<T>(A.ent, A.ent_idx, A.ld_ent, s), A.K, A.d, col, e);
        load_query_grad<T, VEC, KB>(A, s, col, A.d_pos ? A.d_pos[s] : 0.f, gq);
        // d_r[j] += C[a][j][o] e[a] g[o]
#pragma unroll
        for (int a = 0; a < KB; ++a)
#pragma unroll
            for (int o = 0; o < KB; ++o) {
                float p[VEC];
#pragma unroll
                for (int x = 0; x < VEC; ++x) p[x] = e[a][x] * gq[o][x];
#pragma unroll
                for (int j = 0; j < KB; ++j) {
                    const float cf = C.c[(a * KB + j) * KB + o];
                    if (nonzero(cf)) {
#pragma unroll
                        for (int x = 0; x < VEC; ++x) acc[j][x] = fmaf(cf, p[x], acc[j][x]);
                    }
                }
            }
    }
    for (int st = G >> 1; st >= 1; st >>= 1) {  // the rows in flight, pairwise in a fixed order
        if (g >= st && g < 2 * st) {
#pragma unroll
            for (int j = 0; j < KB; ++j)
#pragma unroll
                for (int x = 0; x < VEC; ++x) red[(j * VEC + x) * 256 + t] = acc[j][x];
        }
        __syncthreads();
        if (g < st) {
#pragma unroll
            for (int j = 0; j < KB; ++j)
#pragma unroll
                for (int x = 0; x < VEC; ++x) acc[j][x] += red[(j * VEC + x) * 256 + t + st * lpr];
        }
        __syncthreads();
    }
    if (g != 0 || !live) return;
    if (A.norm) {  // r^ = r / n:  d_r[j] = (d_r^[j] - r^[j] <d_r^, r^>) / n
#pragma unroll
        for (int x = 0; x < VEC; ++x) {
            float dot = 0.f;
#pragma unroll
            for (int j = 0; j < KB; ++j) dot = fmaf(acc[j][x], r[j][x], dot);
#pragma unroll
            for (int j = 0; j < KB; ++j) acc[j][x] = (acc[j][x] - r[j][x] * dot) * inv[x];
        }
    }
    const int64_t Wr = static_cast<int64_t>(A.Kr) * A.d;
    if (cut) {
        store_blocks<VEC, KB>(A.ws + (static_cast<int64_t>(first / SHORT_SEG) * N_SHARE + sh) * Wr, A.Kr, A.d, col, acc);
    } else {
        float* const out = A.d_rel + rel_row * A.ld_drel;
#pragma unroll
        for (int j = 0; j < KB; ++j)
            if (j < A.Kr) {
#pragma unroll
                for (int x = 0; x < VEC; ++x) out[static_cast<int64_t>(j) * A.d + col + x] += acc[j][x];
            }
    }
}

// d_rel[row of segment] += the shares of a cut segment, in share order.  Two cut segments start more than SHORT_SEG
// sorted rows apart: first / SHORT_SEG is a slot of its own for each.
__global__ __launch_bounds__(256) void k_struct_merge(StructArgs A) {
    const int seg = blockIdx.x;
    if (seg >= *A.n_seg) return;
    const int first = A.seg_offsets[seg];
    if (A.seg_offsets[seg + 1] - first <= SHORT_SEG) return;
    const int64_t Wr = static_cast<int64_t>(A.Kr) * A.d;
    const float* const part = A.ws + static_cast<int64_t>(first / SHORT_SEG) * N_SHARE * Wr;
    float* const out = A.d_rel + static_cast<int64_t>(A.seg_rows[seg]) * A.ld_drel;
    for (int64_t w = threadIdx.x; w < Wr; w += 256) {
        float sum = 0.f;
#pragma unroll
        for (int sh = 0; sh < N_SHARE; ++sh) sum += part[sh * Wr + w];
        out[w] += sum;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------
inline int64_t workspace_bytes_of(const bess_struct_desc* D, int64_t S) {
    return (S / SHORT_SEG + 1) * N_SHARE * static_cast<int64_t>(D->n_rel_blocks) * D->block_width * 4;
}

int check_struct_desc(const char* who, const bess_struct_desc* D, int64_t S) {
    BESS_REQUIRE(D, "%s: NULL descriptor", who);
    BESS_REQUIRE(D->dtype == BESS_F32 || D->dtype == BESS_F16, "%s: dtype is BESS_F32 or BESS_F16", who);
    BESS_REQUIRE(D->n_ent_blocks >= 1 && D->n_rel_blocks >= 1 && D->block_width >= 1 && D->n_terms >= 1 && S >= 0,
                 "%s: block counts, block width and term count are positive, S >= 0", who);
    if (D->n_ent_blocks > BESS_STRUCT_MAX_BLOCKS || D->n_rel_blocks > BESS_STRUCT_MAX_BLOCKS ||
        D->n_terms > BESS_STRUCT_MAX_TERMS)
        return fail(BESS_EUNSUPPORTED, "%s: at most %d entity / relation blocks and %d terms (got %d, %d, %d)", who,
                    BESS_STRUCT_MAX_BLOCKS, BESS_STRUCT_MAX_TERMS, D->n_ent_blocks, D->n_rel_blocks, D->n_terms);
    if (static_cast<int64_t>(D->block_width) * BESS_STRUCT_MAX_BLOCKS > (1ll << 24) || S > (1ll << 30))
        return fail(BESS_EUNSUPPORTED, "%s: rows of at most 2^24 columns (block_width <= 2^21) and S <= 2^30", who);
    for (int n = 0; n < D->n_terms; ++n) {
        BESS_REQUIRE(D->ti[n] >= 0 && D->ti[n] < D->n_ent_blocks && D->tk[n] >= 0 && D->tk[n] < D->n_ent_blocks &&
                         D->tj[n] >= 0 && D->tj[n] < D->n_rel_blocks,
                     "%s: term %d names block (%d, %d, %d) of (%d, %d, %d)", who, n, D->ti[n], D->tj[n], D->tk[n],
                     D->n_ent_blocks, D->n_rel_blocks, D->n_ent_blocks);
        BESS_REQUIRE(D->tc[n] - D->tc[n] == 0.f, "%s: the coefficient of term %d is not finite", who, n);
    }
    return BESS_OK;
}

inline bool aligned_to(const void* p, uintptr_t bytes) { return reinterpret_cast<uintptr_t>(p) % bytes == 0; }

// the launch class (table type, vector width, padded block count) and the coefficients of `side`
struct Launch {
    const bess_struct_desc* D;
    int side, kb;
    bool vec4;
    Launch(const bess_struct_desc* D_, int side_, bool vec4_) : D(D_), side(side_), vec4(vec4_) {
        const int k = D->n_ent_blocks > D->n_rel_blocks ? D->n_ent_blocks : D->n_rel_blocks;
        kb = k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : 8;
    }
    void shape(StructArgs& A) const {
        const int vec = vec4 ? 4 : 1;
        A.d = D->block_width, A.K = D->n_ent_blocks, A.Kr = D->n_rel_blocks, A.norm = D->relation_unit_norm != 0;
        A.nch = A.d / vec;
        A.gs = A.nch < 256 ? A.nch : 256;
        A.rows_per_wg = 256 / A.gs;
        A.lpr_log2 = 0;
        while ((1 << A.lpr_log2) < A.gs) ++A.lpr_log2;
    }
    // f(T{}, vec, kb, Coef<KB>): kept block a = head block i for tail corruption, tail block k for head corruption
    template <typename F>
    void run(F&& f) const {
        with_table_type(D->dtype, [&](auto t) {
            with_flag(vec4, [&](auto v4) {
                with_constant<1, 2, 4, 8>(kb, [&](auto kbc) {
                    constexpr int KB = decltype(kbc)::value;
                    Coef<KB> C{};
                    for (int n = 0; n < D->n_terms; ++n) {
                        const int a = side == BESS_CORRUPT_TAIL ? D->ti[n] : D->tk[n];
                        const int o = side == BESS_CORRUPT_TAIL ? D->tk[n] : D->ti[n];
                        if (a < KB && o < KB && D->tj[n] < KB) C.c[(a * KB + D->tj[n]) * KB + o] += D->tc[n];
                    }
                    f(t, std::integral_constant<int, decltype(v4)::value ? 4 : 1>{}, kbc, C);
                });
            });
            return 0;
        });
    }
};

}  // namespace
}  // namespace bess

using namespace bess;

extern "C" int bess_struct_query_workspace(const bess_struct_desc* desc, int64_t S, int64_t n_rel, int64_t* bytes) {
    BESS_REQUIRE(bytes && n_rel >= 1, "struct_query_workspace: NULL pointer or n_rel < 1");
    if (int rc = check_struct_desc("struct_query_workspace", desc, S)) return rc;
    *bytes = workspace_bytes_of(desc, S);
    return BESS_OK;
}

#define STRUCT_CHECK_ROWS(who)                                                                                        \
    if (int rc = check_struct_desc(who, desc, S)) return rc;                                                          \
    BESS_REQUIRE(side == BESS_CORRUPT_HEAD || side == BESS_CORRUPT_TAIL, who ": bad side");                           \
    const int64_t W = static_cast<int64_t>(desc->n_ent_blocks) * desc->block_width;                                   \
    const int64_t Wr = static_cast<int64_t>(desc->n_rel_blocks) * desc->block_width;                                  \
    BESS_REQUIRE(ld_ent >= W && ld_rel >= Wr && (!other_base || ld_other >= W), who ": bad leading dimension");      \
    const uintptr_t tab_align = desc->dtype == BESS_F32 ? 16 : 8;                                                     \
    bool vec4 = desc->block_width % 4 == 0 && ld_ent % 4 == 0 && ld_rel % 4 == 0 && aligned_to(ent_base, tab_align) && \
                aligned_to(rel_table, tab_align) &&                                                                   \
                (!other_base || (ld_other % 4 == 0 && aligned_to(other_base, tab_align)))

extern "C" int bess_struct_query_fwd(const bess_struct_desc* desc, int32_t side, const void* ent_base, int64_t ld_ent,
                                     const int32_t* ent_idx, const void* other_base, int64_t ld_other,
                                     const int32_t* other_idx, const void* rel_table, int64_t ld_rel,
                                     const int32_t* rel_idx, int64_t S, float* q, int64_t ldq, float* pos, void* stream) {
    STRUCT_CHECK_ROWS("struct_query_fwd");
    BESS_REQUIRE(ldq >= W, "struct_query_fwd: bad leading dimension");
    BESS_REQUIRE(!pos == !other_base, "struct_query_fwd: pos and the other rows come together");
    if (S == 0) return BESS_OK;
    BESS_REQUIRE(ent_base && rel_table && rel_idx && q, "struct_query_fwd: NULL pointer");
    vec4 = vec4 && ldq % 4 == 0 && aligned_to(q, 16);
    const Launch L(desc, side, vec4);
    StructArgs A{};
    L.shape(A);
    A.ent = ent_base, A.ent_idx = ent_idx, A.ld_ent = ld_ent, A.other = other_base, A.other_idx = other_idx;
    A.ld_other = ld_other, A.rel = rel_table, A.ld_rel = ld_rel, A.rel_idx = rel_idx, A.S = S;
    A.q = q, A.ldq = ldq, A.pos = pos;
    const unsigned grid = static_cast<unsigned>(ceil_div(S, A.rows_per_wg));
    L.run([&](auto t, auto vec, auto kb, auto C) {
        k_struct_fwd<decltype(t), decltype(vec)::value, decltype(kb)::value><<<grid, 256, 0, as_stream(stream)>>>(A, C);
    });
    return check_launch("struct_query_fwd");
}

extern "C" int bess_struct_query_bwd(const bess_struct_desc* desc, int32_t side, const void* ent_base, int64_t ld_ent,
                                     const int32_t* ent_idx, const void* other_base, int64_t ld_other,
                                     const int32_t* other_idx, const void* rel_table, int64_t ld_rel, int64_t n_rel,
                                     const int32_t* rel_idx, const int32_t* refs_sorted, const int32_t* seg_rows,
                                     const int32_t* seg_offsets, const int32_t* n_seg, int64_t S, const float* dq,
                                     int64_t lddq, const float* d_pos, float* d_ent, int64_t ld_dent, float* d_other,
                                     int64_t ld_dother, float* d_rel, int64_t ld_drel, void* workspace,
                                     int64_t workspace_bytes, void* stream) {
    STRUCT_CHECK_ROWS("struct_query_bwd");
    BESS_REQUIRE(n_rel >= 1 && (!dq || lddq >= W) && ld_dent >= W && (!d_other || ld_dother >= W) &&
                     (!d_rel || ld_drel >= Wr),
                 "struct_query_bwd: bad leading dimension or n_rel < 1");
    BESS_REQUIRE(!d_pos == !other_base && !d_other == !d_pos,
                 "struct_query_bwd: d_pos, the other rows and d_other come together");
    if (S == 0) return BESS_OK;
    BESS_REQUIRE(ent_base && rel_table && rel_idx && d_ent && (dq || d_pos), "struct_query_bwd: NULL pointer");
    vec4 = vec4 && (!dq || (lddq % 4 == 0 && aligned_to(dq, 16))) && ld_dent % 4 == 0 && aligned_to(d_ent, 16) &&
           (!d_other || (ld_dother % 4 == 0 && aligned_to(d_other, 16))) &&
           (!d_rel || (aligned_to(workspace, 16) && ld_drel % 4 == 0 && aligned_to(d_rel, 16)));
    const Launch L(desc, side, vec4);
    StructArgs A{};
    L.shape(A);
    A.ent = ent_base, A.ent_idx = ent_idx, A.ld_ent = ld_ent, A.other = other_base, A.other_idx = other_idx;
    A.ld_other = ld_other, A.rel = rel_table, A.ld_rel = ld_rel, A.rel_idx = rel_idx, A.S = S;
    A.dq = dq, A.lddq = lddq, A.d_pos = d_pos, A.d_ent = d_ent, A.ld_dent = ld_dent, A.d_other = d_other;
    A.ld_dother = ld_dother, A.d_rel = d_rel, A.ld_drel = ld_drel;
    A.refs = refs_sorted, A.seg_rows = seg_rows, A.seg_offsets = seg_offsets, A.n_seg = n_seg;
    A.ws = static_cast<float*>(workspace);
    hipStream_t st = as_stream(stream);
    const unsigned grid = static_cast<unsigned>(ceil_div(S, A.rows_per_wg));
    L.run([&](auto t, auto vec, auto kb, auto C) {
        k_struct_bwd_rows<decltype(t), decltype(vec)::value, decltype(kb)::value><<<grid, 256, 0, st>>>(A, C);
    });
    if (int rc = check_launch("struct_query_bwd: rows")) return rc;
    if (!d_rel) return BESS_OK;
    BESS_REQUIRE(refs_sorted && seg_rows && seg_offsets && n_seg, "struct_query_bwd: NULL segment index");
    BESS_REQUIRE(workspace && workspace_bytes >= workspace_bytes_of(desc, S),
                 "struct_query_bwd: workspace too small (bess_struct_query_workspace)");
    const unsigned max_seg = static_cast<unsigned>(S < n_rel ? S : n_rel);
    const dim3 rel_grid(max_seg, N_SHARE, static_cast<unsigned>(ceil_div(A.nch, 1 << A.lpr_log2)));
    L.run([&](auto t, auto vec, auto kb, auto C) {
        k_struct_bwd_rel<decltype(t), decltype(vec)::value, decltype(kb)::value><<<rel_grid, 256, 0, st>>>(A, C);
    });
    if (int rc = check_launch("struct_query_bwd: relations")) return rc;
    k_struct_merge<<<max_seg, 256, 0, st>>>(A);
    return check_launch("struct_query_bwd: merge");
}
