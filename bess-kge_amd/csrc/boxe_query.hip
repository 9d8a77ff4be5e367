// BoxE: the S-row side of a step - the query [S_0 | C_0 | H_0 | S_1 | C_1 | H_1] of the candidate kernels (boxe.hip),
// the positive score, and the backward of both (reference scoring.py:1149-1415; the candidate side is boxe.hip).
//
// A relation row is [head centre | tail centre | head width | tail width | head size, tail size] (4 d + 2).  Per box
// b (0 head, 1 tail), over its d columns i:
//
//     a_i  = |width_i|                      gm = exp(mean_i log max(a_i, eps))
//     w_i  = a_i / max(gm, eps) * (1 + elu(size))
//     tanh:  low = tanh(c_i - w_i / 2), up = tanh(low + w_i):  C_i = (low + up) / 2,  H_i = (up - low) / 2
//     else:  C_i = c_i,  H_i = w_i / 2
//
// An entity row is [base | bump].  Slot p of the query holds S_p = part 1 - p of the kept row and the box the
// candidate's part p meets: (tail, head) for tail corruption, (head, tail) for head corruption.  The positive score is
// the candidate arithmetic of box_math.h with the triple's other row as the one candidate.
//
// Layout.  The kernels' widths are BoxE's (d <= 512, <= 128 when d % 4 != 0), so a row part is at most 128 chunks of
// VEC = 4 | 1 columns: ONE chunk per lane.  A triple takes gs = the power of two >= d / VEC neighbouring lanes
// (1 .. 128), a workgroup of 256 threads 256 / gs triples: a narrow row keeps several triples in a wave, the widest
// one takes two waves.  A lane holds its VEC columns of both entity parts, of the other row and of the four relation
// blocks in registers; everything is elementwise but the reductions over d, which run over the triple's lanes in a
// fixed order (`group_sum`: DPP inside a 16-lane row, shuffles inside a wave, one LDS exchange between the two waves
// of a 128-lane triple) - two values at a time, one for each box or slot:
//     the sum of log widths;  the count of dimensions outside (one choice per slot);  the two p-norms.
//
//   k_boxq_fwd        q and / or pos of every triple
//   k_boxq_bwd_rows   d_ent and d_other of every triple
//   k_boxq_bwd_rel    one workgroup walks one relation segment of the batch (a share of it when the segment has more
//                     than SHORT_SEG triples), 256 / gs triples in flight.  The normalised box depends on the relation
//                     alone: it is computed once; the walk sums d loss / d C and d loss / d H over the triples - the
//                     C and H blocks of dq as they are, the d_pos part recomputed from the rows - in walk order, a
//                     tree over the triples in flight in LDS, and the Jacobian of the normalisation (tanh pair,
//                     geometric-mean scaling with its one reduction sum_i G_i a_i, elu, abs) is applied to the sum:
//                     once per segment or, by linearity, per share.  Shares go through the workspace and
//                     k_boxq_merge adds them in share order.  No atomics: a relation's columns have one owner.
#include "box_math.h"
#include "common.h"

namespace bess {
namespace {

constexpr int SHORT_SEG = 32;  // segments up to this many triples: one workgroup, added into d_rel directly
constexpr int N_SHARE = 16;    // shares of a longer segment

struct BoxQArgs {
    const void *ent, *other, *rel;  // rows of the table type; other NULL: no positive score
    const int32_t *ent_idx, *other_idx, *rel_idx;
    int64_t ld_ent, ld_other, ld_rel;
    float *q, *pos;  // forward (either may be NULL)
    const float *dq, *d_pos;  // backward (either may be NULL)
    float *d_ent, *d_other, *d_rel;
    int64_t ldq, lddq, ld_dent, ld_dother, ld_drel;
    const int32_t *refs, *seg_rows, *seg_offsets, *n_seg;
    float* ws;
    int ws_by_seg;  // a cut segment's slot of the workspace: its number, or first / SHORT_SEG
    int64_t S;
    int d, nch;        // nch: chunks of VEC columns per part
    int gs, gs_log2;   // lanes per triple
    int tail;          // tail corruption: slot 0 meets the tail box
    float eps, p;
};

template <typename T>
__device__ __forceinline__ const T* src_row(const void* base, const int32_t* idx, int64_t ld, int64_t i) {
    return static_cast<const T*>(base) + (idx ? static_cast<int64_t>(idx[i]) : i) * ld;
}

// VEC columns of a relation row: rows of 4 d + 2 scalars start on every other pair, so a chunk of four is two pairs
template <typename T, int VEC>
__device__ __forceinline__ void load_rel(const T* __restrict__ p, float (&v)[VEC]) {
    if constexpr (VEC == 4) {
        float lo[2], hi[2];
        VecLoad<T, 2>::load(p, lo);
        VecLoad<T, 2>::load(p + 2, hi);
        v[0] = lo[0], v[1] = lo[1], v[2] = hi[0], v[3] = hi[1];
    } else {
        VecLoad<T, 1>::load(p, v);
    }
}

template <int VEC>
__device__ __forceinline__ void store_f32(float* __restrict__ p, const float (&v)[VEC]) {
    if constexpr (VEC == 1) {
        p[0] = v[0];
    } else {
        typedef float vec_t __attribute__((ext_vector_type(VEC)));
        vec_t o;
#pragma unroll
        for (int x = 0; x < VEC; ++x) o[x] = v[x];
        *reinterpret_cast<vec_t*>(p) = o;
    }
}

// Sums over the gs lanes of a triple, two values at a time; every lane of the triple gets the same bits.  red: LDS,
// 2 x 8 floats; `phase` alternates between its halves, so one barrier per exchange is enough.  Called by every thread
// of the workgroup (gs is uniform).
__device__ __forceinline__ void group_sum(float (&v)[2], int gs, float* red, int& phase) {
    if (gs >= 16) {
        v[0] = row16_allreduce_sum(v[0]);
        v[1] = row16_allreduce_sum(v[1]);
    } else {
        for (int m = 1; m < gs; m <<= 1) {
            v[0] += __shfl_xor(v[0], m, 64);
            v[1] += __shfl_xor(v[1], m, 64);
        }
    }
    if (gs >= 32) {
        v[0] += __shfl_xor(v[0], 16, 64);
        v[1] += __shfl_xor(v[1], 16, 64);
    }
    if (gs >= 64) {
        v[0] += __shfl_xor(v[0], 32, 64);
        v[1] += __shfl_xor(v[1], 32, 64);
    }
    if (gs == 128) {  // the two waves of the triple, the lower one first
        const int w = threadIdx.x >> 6;
        float* buf = red + 8 * phase;
        if ((threadIdx.x & 63) == 0) buf[w] = v[0], buf[4 + w] = v[1];
        __syncthreads();
        v[0] = buf[w & 2] + buf[(w & 2) + 1];
        v[1] = buf[4 + (w & 2)] + buf[4 + (w & 2) + 1];
        phase ^= 1;
    }
}

// One lane's columns of a relation row and the scaling of its two boxes
template <int VEC>
struct BoxRel {
    float c[2][VEC], wr[2][VEC], sz[2];
    float gm[2], gmc[2], sc[2];  // geometric mean, its clamp, 1 + elu(size)

    template <typename T>
    __device__ __forceinline__ void load(const T* __restrict__ row, int d, int col) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            load_rel<T, VEC>(row + b * d + col, c[b]);
            load_rel<T, VEC>(row + (2 + b) * d + col, wr[b]);
            sz[b] = static_cast<float>(row[4 * d + b]);
        }
    }
    __device__ __forceinline__ void scale(bool live, int d, float eps, int gs, float* red, int& phase) {
        float ls[2] = {0.f, 0.f};
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int x = 0; x < VEC; ++x) ls[b] += live ? logf(fmaxf(fabsf(wr[b][x]), eps)) : 0.f;
        group_sum(ls, gs, red, phase);
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            gm[b] = expf(ls[b] / static_cast<float>(d));
            gmc[b] = fmaxf(gm[b], eps);
            sc[b] = 1.f + (sz[b] > 0.f ? sz[b] : expm1f(sz[b]));
        }
    }
    __device__ __forceinline__ float width(int b, int x) const { return fabsf(wr[b][x]) / gmc[b] * sc[b]; }
    // centre and half width of box b
    template <bool TANH>
    __device__ __forceinline__ void shape(int b, float (&C)[VEC], float (&H)[VEC]) const {
#pragma unroll
        for (int x = 0; x < VEC; ++x) {
            const float w = width(b, x);
            if (TANH) {
                const float low = tanhf(c[b][x] - 0.5f * w), up = tanhf(low + w);
                C[x] = 0.5f * (low + up);
                H[x] = 0.5f * (up - low);
            } else {
                C[x] = c[b][x];
                H[x] = 0.5f * w;
            }
        }
    }
};

// The positive score's pieces of one triple: slot p sees the other row's part p bumped by the kept row's part 1 - p
template <int VEC, int P, bool TANH, bool PERDIM>
struct BoxTriple {
    float outs[2], acc[2];
    // Cs, Hs: by slot
    __device__ __forceinline__ void reduce(const float (&e)[2][VEC], const float (&o)[2][VEC], const float (&Cs)[2][VEC],
                                           const float (&Hs)[2][VEC], bool live, float p, bool need_norm, int gs,
                                           float* red, int& phase) {
        outs[0] = outs[1] = 0.f;
        if (!PERDIM) {  // one choice per slot: inside only if every dimension is
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int x = 0; x < VEC; ++x) {
                    float xp, dist;
                    bool in;
                    box_point<TANH>(o[s][x], e[1 - s][x], Cs[s][x], Hs[s][x], xp, dist, in);
                    outs[s] += (live && !in) ? 1.f : 0.f;
                }
            group_sum(outs, gs, red, phase);
        }
        acc[0] = acc[1] = 0.f;
        if (!need_norm) return;
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int x = 0; x < VEC; ++x) {
                float xp, dist;
                bool in;
                box_point<TANH>(o[s][x], e[1 - s][x], Cs[s][x], Hs[s][x], xp, dist, in);
                if (!PERDIM) in = outs[s] == 0.f;
                const float f = box_final(dist, Hs[s][x], in);
                acc[s] += live ? ((P == 1) ? fabsf(f) : lp_term(f, p)) : 0.f;
            }
        group_sum(acc, gs, red, phase);
    }
    // gradients of slot s for d loss / d score = dp: the point before its tanh (dx), the centre, the half width
    __device__ __forceinline__ void grad(int s, const float (&e)[2][VEC], const float (&o)[2][VEC], const float (&Cs)[VEC],
                                         const float (&Hs)[VEC], float dp, float p, float (&dx)[VEC], float (&dc)[VEC],
                                         float (&dh)[VEC]) const {
        const float gp = (P == 2) ? -dp * lp_inv(lp_root(acc[s], p), p) : -dp;
#pragma unroll
        for (int x = 0; x < VEC; ++x) {
            float xp, dist;
            bool in;
            box_point<TANH>(o[s][x], e[1 - s][x], Cs[x], Hs[x], xp, dist, in);
            if (!PERDIM) in = outs[s] == 0.f;
            box_grad<TANH, P>(xp, dist, Cs[x], Hs[x], in, gp, p, dx[x], dc[x], dh[x]);
        }
    }
};

// what every kernel's thread is: lane c0 of triple slot g, its chunk's first column (lanes past the part: the last
// chunk, a valid address, and nothing stored)
struct Lane {
    int g, c0, col;
    bool live;
    __device__ __forceinline__ explicit Lane(const BoxQArgs& A, int VEC) {
        g = threadIdx.x >> A.gs_log2, c0 = threadIdx.x & (A.gs - 1);
        live = c0 < A.nch;
        col = min(c0, A.nch - 1) * VEC;
    }
};

template <typename T, int VEC>
__device__ __forceinline__ void load_parts(const T* __restrict__ row, int d, int col, float (&v)[2][VEC]) {
    VecLoad<T, VEC>::load(row + col, v[0]);
    VecLoad<T, VEC>::load(row + d + col, v[1]);
}

// centre and half width by slot from the boxes' (slot 0 meets the tail box for tail corruption)
template <int VEC, bool TANH>
__device__ __forceinline__ void slot_boxes(const BoxRel<VEC>& R, bool tail, float (&Cs)[2][VEC], float (&Hs)[2][VEC]) {
    float C[2][VEC], H[2][VEC];
    R.template shape<TANH>(0, C[0], H[0]);
    R.template shape<TANH>(1, C[1], H[1]);
#pragma unroll
    for (int x = 0; x < VEC; ++x) {
        Cs[0][x] = tail ? C[1][x] : C[0][x], Hs[0][x] = tail ? H[1][x] : H[0][x];
        Cs[1][x] = tail ? C[0][x] : C[1][x], Hs[1][x] = tail ? H[0][x] : H[1][x];
    }
}

template <typename T, int VEC, int P, bool TANH, bool PERDIM>
__global__ __launch_bounds__(256) void k_boxq_fwd(BoxQArgs A) {
    __shared__ float red[16];
    int phase = 0;
    const Lane L(A, VEC);
    const int64_t s_raw = static_cast<int64_t>(blockIdx.x) * (256 >> A.gs_log2) + L.g;
    const bool valid = s_raw < A.S;
    const int64_t s = valid ? s_raw : A.S - 1;
    BoxRel<VEC> R;
    R.load(static_cast<const T*>(A.rel) + static_cast<int64_t>(A.rel_idx[s]) * A.ld_rel, A.d, L.col);
    float e[2][VEC], Cs[2][VEC], Hs[2][VEC];
    load_parts<T, VEC>(src_row<T>(A.ent, A.ent_idx, A.ld_ent, s), A.d, L.col, e);
    R.scale(L.live, A.d, A.eps, A.gs, red, phase);
    slot_boxes<VEC, TANH>(R, A.tail != 0, Cs, Hs);
    if (A.q && valid && L.live) {
        float* const qrow = A.q + s * A.ldq + L.col;
#pragma unroll
        for (int sl = 0; sl < 2; ++sl) {
            store_f32<VEC>(qrow + (3 * sl + 0) * A.d, e[1 - sl]);
            store_f32<VEC>(qrow + (3 * sl + 1) * A.d, Cs[sl]);
            store_f32<VEC>(qrow + (3 * sl + 2) * A.d, Hs[sl]);
        }
    }
    if (A.pos) {
        float o[2][VEC];
        load_parts<T, VEC>(src_row<T>(A.other, A.other_idx, A.ld_other, s), A.d, L.col, o);
        BoxTriple<VEC, P, TANH, PERDIM> tr;
        tr.reduce(e, o, Cs, Hs, L.live, A.p, true, A.gs, red, phase);
        const float total = (P == 2) ? lp_root(tr.acc[0], A.p) + lp_root(tr.acc[1], A.p) : tr.acc[0] + tr.acc[1];
        if (valid && L.c0 == 0) A.pos[s] = -total;
    }
}

template <typename T, int VEC, int P, bool TANH, bool PERDIM>
__global__ __launch_bounds__(256) void k_boxq_bwd_rows(BoxQArgs A) {
    __shared__ float red[16];
    int phase = 0;
    const Lane L(A, VEC);
    const int64_t s_raw = static_cast<int64_t>(blockIdx.x) * (256 >> A.gs_log2) + L.g;
    const bool valid = s_raw < A.S;
    const int64_t s = valid ? s_raw : A.S - 1;
    float dS[2][VEC];  // by slot: the gradient of S_p, the kept row's part 1 - p
#pragma unroll
    for (int sl = 0; sl < 2; ++sl) {
        if (A.dq) {
            VecLoad<float, VEC>::load(A.dq + s * A.lddq + 3 * sl * A.d + L.col, dS[sl]);
        } else {
#pragma unroll
            for (int x = 0; x < VEC; ++x) dS[sl][x] = 0.f;
        }
    }
    if (A.d_pos) {
        BoxRel<VEC> R;
        R.load(static_cast<const T*>(A.rel) + static_cast<int64_t>(A.rel_idx[s]) * A.ld_rel, A.d, L.col);
        float e[2][VEC], o[2][VEC], Cs[2][VEC], Hs[2][VEC];
        load_parts<T, VEC>(src_row<T>(A.ent, A.ent_idx, A.ld_ent, s), A.d, L.col, e);
        load_parts<T, VEC>(src_row<T>(A.other, A.other_idx, A.ld_other, s), A.d, L.col, o);
        R.scale(L.live, A.d, A.eps, A.gs, red, phase);
        slot_boxes<VEC, TANH>(R, A.tail != 0, Cs, Hs);
        BoxTriple<VEC, P, TANH, PERDIM> tr;
        tr.reduce(e, o, Cs, Hs, L.live, A.p, P == 2, A.gs, red, phase);
        const float dp = A.d_pos[s];
#pragma unroll
        for (int sl = 0; sl < 2; ++sl) {
            float dx[VEC], dc[VEC], dh[VEC];
            tr.grad(sl, e, o, Cs[sl], Hs[sl], dp, A.p, dx, dc, dh);
#pragma unroll
            for (int x = 0; x < VEC; ++x) dS[sl][x] += dx[x];
            if (valid && L.live) store_f32<VEC>(A.d_other + s * A.ld_dother + sl * A.d + L.col, dx);
        }
    }
    if (valid && L.live) {
        store_f32<VEC>(A.d_ent + s * A.ld_dent + A.d + L.col, dS[0]);
        store_f32<VEC>(A.d_ent + s * A.ld_dent + L.col, dS[1]);
    }
}

// grid (segment bound, N_SHARE)
template <typename T, int VEC, int P, bool TANH, bool PERDIM>
__global__ __launch_bounds__(256) void k_boxq_bwd_rel(BoxQArgs A) {
    __shared__ float red[16];
    __shared__ float tree[4 * VEC * 256];
    int phase = 0;
    const int seg = blockIdx.x, sh = blockIdx.y;
    if (seg >= *A.n_seg) return;
    const int first = A.seg_offsets[seg], len = A.seg_offsets[seg + 1] - first;
    const bool cut = len > SHORT_SEG;
    if (!cut && sh) return;
    const int r0 = cut ? static_cast<int>(static_cast<int64_t>(len) * sh / N_SHARE) : 0;
    const int r1 = cut ? static_cast<int>(static_cast<int64_t>(len) * (sh + 1) / N_SHARE) : len;
    const Lane L(A, VEC);
    const int t = threadIdx.x, G = 256 >> A.gs_log2;
    const bool tail = A.tail != 0;
    const int64_t rel_row = A.seg_rows[seg];
    BoxRel<VEC> R;
    R.load(static_cast<const T*>(A.rel) + rel_row * A.ld_rel, A.d, L.col);
    R.scale(L.live, A.d, A.eps, A.gs, red, phase);
    float Cs[2][VEC], Hs[2][VEC];
    slot_boxes<VEC, TANH>(R, tail, Cs, Hs);
    float gc[2][VEC], gh[2][VEC];  // by slot: sums of d loss / d C_p, d loss / d H_p
#pragma unroll
    for (int sl = 0; sl < 2; ++sl)
#pragma unroll
        for (int x = 0; x < VEC; ++x) gc[sl][x] = gh[sl][x] = 0.f;
    for (int i0 = r0; i0 < r1; i0 += G) {  // (uniform trip count: the reductions hold barriers)
        const bool valid = i0 + L.g < r1;
        const int64_t s = A.refs[first + min(i0 + L.g, r1 - 1)];
        if (A.dq) {
            const float* const row = A.dq + s * A.lddq + L.col;
#pragma unroll
            for (int sl = 0; sl < 2; ++sl) {
                float dc[VEC], dh[VEC];
                VecLoad<float, VEC>::load(row + (3 * sl + 1) * A.d, dc);
                VecLoad<float, VEC>::load(row + (3 * sl + 2) * A.d, dh);
#pragma unroll
                for (int x = 0; x < VEC; ++x) {
                    gc[sl][x] += valid ? dc[x] : 0.f;
                    gh[sl][x] += valid ? dh[x] : 0.f;
                }
            }
        }
        if (A.d_pos) {
            float e[2][VEC], o[2][VEC];
            load_parts<T, VEC>(src_row<T>(A.ent, A.ent_idx, A.ld_ent, s), A.d, L.col, e);
            load_parts<T, VEC>(src_row<T>(A.other, A.other_idx, A.ld_other, s), A.d, L.col, o);
            BoxTriple<VEC, P, TANH, PERDIM> tr;
            tr.reduce(e, o, Cs, Hs, L.live, A.p, P == 2, A.gs, red, phase);
            const float dp = A.d_pos[s];
#pragma unroll
            for (int sl = 0; sl < 2; ++sl) {
                float dx[VEC], dc[VEC], dh[VEC];
                tr.grad(sl, e, o, Cs[sl], Hs[sl], dp, A.p, dx, dc, dh);
#pragma unroll
                for (int x = 0; x < VEC; ++x) {
                    gc[sl][x] += valid ? dc[x] : 0.f;
                    gh[sl][x] += valid ? dh[x] : 0.f;
                }
            }
        }
    }
    for (int st = G >> 1; st >= 1; st >>= 1) {  // the triples in flight, pairwise in a fixed order
        if (L.g >= st && L.g < 2 * st) {
#pragma unroll
            for (int sl = 0; sl < 2; ++sl)
#pragma unroll
                for (int x = 0; x < VEC; ++x) {
                    tree[((2 * sl + 0) * VEC + x) * 256 + t] = gc[sl][x];
                    tree[((2 * sl + 1) * VEC + x) * 256 + t] = gh[sl][x];
                }
        }
        __syncthreads();
        if (L.g < st) {
#pragma unroll
            for (int sl = 0; sl < 2; ++sl)
#pragma unroll
                for (int x = 0; x < VEC; ++x) {
                    gc[sl][x] += tree[((2 * sl + 0) * VEC + x) * 256 + t + st * A.gs];
                    gh[sl][x] += tree[((2 * sl + 1) * VEC + x) * 256 + t + st * A.gs];
                }
        }
        __syncthreads();
    }
    // The Jacobian of the normalisation on the summed gradients (every thread runs it: the reduction holds a
    // barrier; the triple slot 0 owns the result).  By box b: slot 1 - b for tail corruption, slot b otherwise.
    float dcen[2][VEC], dw[2][VEC], dk[2] = {0.f, 0.f};
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int x = 0; x < VEC; ++x) {
            const float GC = tail ? gc[1 - b][x] : gc[b][x], GH = tail ? gh[1 - b][x] : gh[b][x];
            const float a = fabsf(R.wr[b][x]), w = R.width(b, x);
            if (TANH) {
                const float low = tanhf(R.c[b][x] - 0.5f * w), up = tanhf(low + w);
                const float dz = 0.5f * (GC + GH) * (1.f - up * up);
                const float dy = (0.5f * (GC - GH) + dz) * (1.f - low * low);
                dcen[b][x] = dy;
                dw[b][x] = dz - 0.5f * dy;
            } else {
                dcen[b][x] = GC;
                dw[b][x] = 0.5f * GH;
            }
            dk[b] += L.live ? dw[b][x] * a : 0.f;
        }
    group_sum(dk, A.gs, red, phase);
    if (L.g != 0 || !L.live) return;
    const int64_t Wr = 4ll * A.d + 2;
    float* const out = cut ? A.ws + (static_cast<int64_t>(A.ws_by_seg ? seg : first / SHORT_SEG) * N_SHARE + sh) * Wr
                           : A.d_rel + rel_row * A.ld_drel;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        // w = a k, k = sc / gmc: d k = sum_i dw_i a_i;  a clamped value passes no gradient
        const float dgm = R.gm[b] >= A.eps ? -dk[b] * R.sc[b] / (R.gmc[b] * R.gmc[b]) : 0.f;
        const float dmean = dgm * R.gm[b] / static_cast<float>(A.d);  // d loss / d log max(a_i, eps), every i
        const float dsz = dk[b] / R.gmc[b] * (R.sz[b] > 0.f ? 1.f : expf(R.sz[b]));
#pragma unroll
        for (int x = 0; x < VEC; ++x) {
            const float a = fabsf(R.wr[b][x]);
            const float da = dw[b][x] * (R.sc[b] / R.gmc[b]) + (a >= A.eps ? dmean / a : 0.f);
            const float dwr = da * sgnf(R.wr[b][x]);
            float* const oc = out + b * A.d + L.col + x;
            float* const ow = out + (2 + b) * A.d + L.col + x;
            if (cut) *oc = dcen[b][x], *ow = dwr;
            else *oc += dcen[b][x], *ow += dwr;
        }
        if (L.c0 == 0) {
            if (cut) out[4 * A.d + b] = dsz;
            else out[4 * A.d + b] += dsz;
        }
    }
}

// d_rel[row of segment] += the shares of a cut segment, in share order
__global__ __launch_bounds__(256) void k_boxq_merge(BoxQArgs A) {
    const int seg = blockIdx.x;
    if (seg >= *A.n_seg) return;
    const int first = A.seg_offsets[seg];
    if (A.seg_offsets[seg + 1] - first <= SHORT_SEG) return;
    const int64_t Wr = 4ll * A.d + 2;
    const float* const part = A.ws + static_cast<int64_t>(A.ws_by_seg ? seg : first / SHORT_SEG) * N_SHARE * Wr;
    float* const out = A.d_rel + static_cast<int64_t>(A.seg_rows[seg]) * A.ld_drel;
    for (int64_t w = threadIdx.x; w < Wr; w += 256) {
        float sum = 0.f;
#pragma unroll
        for (int sh = 0; sh < N_SHARE; ++sh) sum += part[sh * Wr + w];
        out[w] += sum;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------
// Two cut segments start more than SHORT_SEG sorted triples apart and there are at most n_rel segments: a cut
// segment's slot is first / SHORT_SEG or its number, whichever range is smaller.
inline bool ws_by_seg(int64_t S, int64_t n_rel) { return n_rel < S / SHORT_SEG + 1; }
inline int64_t workspace_bytes_of(int d, int64_t S, int64_t n_rel) {
    const int64_t slots = ws_by_seg(S, n_rel) ? n_rel : S / SHORT_SEG + 1;
    return slots * N_SHARE * (4ll * d + 2) * 4;
}

int check_box_desc(const char* who, const bess_model_desc* D, int64_t S) {
    if (int rc = check_desc(D)) return rc;
    BESS_REQUIRE(D->scorer == BESS_BOXE, "%s: the descriptor is not BoxE's", who);
    BESS_REQUIRE(S >= 0 && S <= (1ll << 30), "%s: 0 <= S <= 2^30", who);
    const int d = D->width / 2;
    BESS_REQUIRE(D->rel_width == 4 * d + 2, "%s: rel_width %d is not 4 d + 2", who, D->rel_width);
    if (d > 512 || (d % 4 != 0 && d > 128)) return fail(BESS_EUNSUPPORTED, BOX_TOO_WIDE, d);
    return BESS_OK;
}

inline bool aligned_to(const void* p, uintptr_t bytes) { return reinterpret_cast<uintptr_t>(p) % bytes == 0; }

template <typename F>
void dispatch(const bess_model_desc* D, bool vec4, F&& f) {
    with_table_type(D->dtype, [&](auto t) {
        with_flag(vec4, [&](auto v4) {
            with_constant<1, 2>(D->norm_p, [&](auto p) {
                with_constant<0, 1, 2, 3>(D->reserved[0] & 3, [&](auto fl) {  // bit 0 = tanh, bit 1 = per dimension
                    f(t, std::integral_constant<int, decltype(v4)::value ? 4 : 1>{}, p,
                      std::bool_constant<(decltype(fl)::value & 1) != 0>{},
                      std::bool_constant<(decltype(fl)::value & 2) != 0>{});
                });
            });
        });
        return 0;
    });
}

}  // namespace
}  // namespace bess

using namespace bess;

extern "C" int bess_boxe_query_workspace(const bess_model_desc* desc, int64_t S, int64_t n_rel, int64_t* bytes) {
    BESS_REQUIRE(bytes && n_rel >= 1, "boxe_query_workspace: NULL pointer or n_rel < 1");
    if (int rc = check_box_desc("boxe_query_workspace", desc, S)) return rc;
    *bytes = workspace_bytes_of(desc->width / 2, S, n_rel);
    return BESS_OK;
}

// Chunks of four columns need: entity-type rows on 4-scalar boundaries, relation rows on pairs, fp32 rows on 16 bytes.
#define BOXQ_CHECK_ROWS(who)                                                                                          \
    if (int rc = check_box_desc(who, desc, S)) return rc;                                                             \
    BESS_REQUIRE(side == BESS_CORRUPT_HEAD || side == BESS_CORRUPT_TAIL, who ": bad side");                           \
    BESS_REQUIRE(eps > 0.f && eps - eps == 0.f, who ": eps is positive and finite");                                  \
    const int dd = desc->width / 2;                                                                                   \
    const int64_t W = desc->width, Wr = desc->rel_width;                                                              \
    BESS_REQUIRE(ld_ent >= W && ld_rel >= Wr && (!other_base || ld_other >= W), who ": bad leading dimension");      \
    const uintptr_t tab_align = desc->dtype == BESS_F32 ? 16 : 8;                                                     \
    bool vec4 = dd % 4 == 0 && ld_ent % 4 == 0 && ld_rel % 2 == 0 && aligned_to(ent_base, tab_align) &&               \
                aligned_to(rel_table, tab_align / 2) &&                                                               \
                (!other_base || (ld_other % 4 == 0 && aligned_to(other_base, tab_align)))

static void boxq_shape(const bess_model_desc* desc, int32_t side, float eps, bool vec4, BoxQArgs& A) {
    A.d = desc->width / 2;
    A.nch = A.d / (vec4 ? 4 : 1);
    A.gs_log2 = 0;
    while ((1 << A.gs_log2) < A.nch) ++A.gs_log2;
    A.gs = 1 << A.gs_log2;
    A.tail = side == BESS_CORRUPT_TAIL;
    A.eps = eps;
    A.p = static_cast<float>(desc->norm_p);
}

extern "C" int bess_boxe_query_fwd(const bess_model_desc* desc, int32_t side, float eps, const void* ent_base,
                                   int64_t ld_ent, const int32_t* ent_idx, const void* other_base, int64_t ld_other,
                                   const int32_t* other_idx, const void* rel_table, int64_t ld_rel,
                                   const int32_t* rel_idx, int64_t S, float* q, int64_t ldq, float* pos, void* stream) {
    BOXQ_CHECK_ROWS("boxe_query_fwd");
    BESS_REQUIRE(!q || ldq >= 3 * W, "boxe_query_fwd: bad leading dimension");
    BESS_REQUIRE(!pos == !other_base, "boxe_query_fwd: pos and the other rows come together");
    if (S == 0) return BESS_OK;
    BESS_REQUIRE(ent_base && rel_table && rel_idx && (q || pos), "boxe_query_fwd: NULL pointer");
    vec4 = vec4 && (!q || (ldq % 4 == 0 && aligned_to(q, 16)));
    if (!vec4 && dd > 128)
        return fail(BESS_EUNSUPPORTED, "boxe_query_fwd: rows of more than 128 columns need 16-byte aligned operands");
    BoxQArgs A{};
    boxq_shape(desc, side, eps, vec4, A);
    A.ent = ent_base, A.ent_idx = ent_idx, A.ld_ent = ld_ent, A.other = other_base, A.other_idx = other_idx;
    A.ld_other = ld_other, A.rel = rel_table, A.ld_rel = ld_rel, A.rel_idx = rel_idx, A.S = S;
    A.q = q, A.ldq = ldq, A.pos = pos;
    const unsigned grid = static_cast<unsigned>(ceil_div(S, 256 >> A.gs_log2));
    dispatch(desc, vec4, [&](auto t, auto vec, auto p, auto th, auto pd) {
        k_boxq_fwd<decltype(t), decltype(vec)::value, decltype(p)::value, decltype(th)::value, decltype(pd)::value>
            <<<grid, 256, 0, as_stream(stream)>>>(A);
    });
    return check_launch("boxe_query_fwd");
}

extern "C" int bess_boxe_query_bwd(const bess_model_desc* desc, int32_t side, float eps, const void* ent_base,
                                   int64_t ld_ent, const int32_t* ent_idx, const void* other_base, int64_t ld_other,
                                   const int32_t* other_idx, const void* rel_table, int64_t ld_rel, int64_t n_rel,
                                   const int32_t* rel_idx, const int32_t* refs_sorted, const int32_t* seg_rows,
                                   const int32_t* seg_offsets, const int32_t* n_seg, int64_t S, const float* dq,
                                   int64_t lddq, const float* d_pos, float* d_ent, int64_t ld_dent, float* d_other,
                                   int64_t ld_dother, float* d_rel, int64_t ld_drel, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
    BOXQ_CHECK_ROWS("boxe_query_bwd");
    BESS_REQUIRE(n_rel >= 1 && (!dq || lddq >= 3 * W) && ld_dent >= W && (!d_other || ld_dother >= W) &&
                     (!d_rel || ld_drel >= Wr),
                 "boxe_query_bwd: bad leading dimension or n_rel < 1");
    BESS_REQUIRE(!d_pos == !other_base && !d_other == !d_pos,
                 "boxe_query_bwd: d_pos, the other rows and d_other come together");
    if (S == 0) return BESS_OK;
    BESS_REQUIRE(ent_base && rel_table && rel_idx && d_ent && (dq || d_pos), "boxe_query_bwd: NULL pointer");
    vec4 = vec4 && (!dq || (lddq % 4 == 0 && aligned_to(dq, 16))) && ld_dent % 4 == 0 && aligned_to(d_ent, 16) &&
           (!d_other || (ld_dother % 4 == 0 && aligned_to(d_other, 16)));
    if (!vec4 && dd > 128)
        return fail(BESS_EUNSUPPORTED, "boxe_query_bwd: rows of more than 128 columns need 16-byte aligned operands");
    if (d_rel) {
        BESS_REQUIRE(refs_sorted && seg_rows && seg_offsets && n_seg, "boxe_query_bwd: NULL segment index");
        BESS_REQUIRE(workspace && workspace_bytes >= workspace_bytes_of(dd, S, n_rel),
                     "boxe_query_bwd: workspace too small (bess_boxe_query_workspace)");
    }
    BoxQArgs A{};
    boxq_shape(desc, side, eps, vec4, A);
    A.ent = ent_base, A.ent_idx = ent_idx, A.ld_ent = ld_ent, A.other = other_base, A.other_idx = other_idx;
    A.ld_other = ld_other, A.rel = rel_table, A.ld_rel = ld_rel, A.rel_idx = rel_idx, A.S = S;
    A.dq = dq, A.lddq = lddq, A.d_pos = d_pos, A.d_ent = d_ent, A.ld_dent = ld_dent, A.d_other = d_other;
    A.ld_dother = ld_dother, A.d_rel = d_rel, A.ld_drel = ld_drel;
    A.refs = refs_sorted, A.seg_rows = seg_rows, A.seg_offsets = seg_offsets, A.n_seg = n_seg;
    A.ws = static_cast<float*>(workspace), A.ws_by_seg = ws_by_seg(S, n_rel);
    hipStream_t st = as_stream(stream);
    const unsigned grid = static_cast<unsigned>(ceil_div(S, 256 >> A.gs_log2));
    dispatch(desc, vec4, [&](auto t, auto vec, auto p, auto th, auto pd) {
        k_boxq_bwd_rows<decltype(t), decltype(vec)::value, decltype(p)::value, decltype(th)::value, decltype(pd)::value>
            <<<grid, 256, 0, st>>>(A);
    });
    if (int rc = check_launch("boxe_query_bwd: rows")) return rc;
    if (!d_rel) return BESS_OK;
    const unsigned max_seg = static_cast<unsigned>(S < n_rel ? S : n_rel);
    const dim3 rel_grid(max_seg, N_SHARE);
    dispatch(desc, vec4, [&](auto t, auto vec, auto p, auto th, auto pd) {
        k_boxq_bwd_rel<decltype(t), decltype(vec)::value, decltype(p)::value, decltype(th)::value, decltype(pd)::value>
            <<<rel_grid, 256, 0, st>>>(A);
    });
    if (int rc = check_launch("boxe_query_bwd: relations")) return rc;
    k_boxq_merge<<<max_seg, 256, 0, st>>>(A);
    return check_launch("boxe_query_bwd: merge");
}
