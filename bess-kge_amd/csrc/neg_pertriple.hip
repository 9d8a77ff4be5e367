// K5 on gfx950: per-triple negatives, the HBM-bound hot kernel of the BESS step.
//
//   out[q, k] = sign * reduce_w f(query[q, w], E[neg_idx[q, k], w])       k < n_neg
//
// (reference `reduce_embedding(q.unsqueeze(1) o N)`, scoring.py:199 / 254, fed by
//  the gather `self.entity_embedding[gather_idx]`, bess.py:332-337 - here the
//  gather is fused: negative rows are read straight from the shard, exactly
//  once, and nothing of shape [S, N, W] is ever materialised.)
//
// Roofline: one gathered row (W*sz bytes: 2 KiB for ComplEx d=256 fp32) per
// scored triple against 2-3 flops per scalar -> HBM bound; algorithmic bytes =
// n_query*n_neg*(W*sz + 4 idx + 4 out) + n_query*W*4.
//
// Mapping (CDNA4, wave64): a wave owns one (query, block of NB negatives) work
// item.  Its four 16-lane DPP rows each stream a different negative row, lane g
// of a row reading the 16-byte chunks g, g+16, g+32, ... of that table row
// (256 contiguous bytes per DPP row per load instruction -> two full 128 B
// lines).  The query lives in registers in the same chunk layout, so the inner
// loop is loads + FMAs only; the cross-lane reduction is 4 DPP row-rotate adds
// shared by the four rows in flight.  UNROLL row-groups are issued back to back
// to keep >= 8 x 16 B loads per lane in flight (the guide's recipe for ~5.7 TB/s
// random-row gathers: "4 rows in flight per wave, 16 waves per CU").
#include "common.h"
#include "loss_rows.h"

namespace bess {

struct NegPtArgs {
    const float* query;
    const void* base;
    const int32_t* idx;
    int64_t n_query;
    int n_neg;
    int W;
    int nch;  // chunks (of VEC scalars) per row
    int nb;   // negatives per work item
    int items_per_query;
    float sign;
    int accum = 0;  // forward: add to the scores already there (a later column window of a wide row)
    float p = 2.f;  // the norm of the RED_L2 kernels (any p != 1)
    int dn_by_row = 0;  // backward: d_neg row of reference k is neg_idx[k] (BESS_FLAG_DNEG_BY_ROW), not q * n_neg + k
    int sweep_shift = -1;  // plain forward: >= 0 takes k_neg_pertriple_fwd_sweep, row buckets of 1 << sweep_shift rows
};

// Fused training forward (FUSE): besides the scores, accumulate the loss gradient wrt the query,
//     d_query[q] = sum_k dL/ds(q, k) * ds(q, k)/dq,
// in the same pass over the rows, so the backward never re-reads them.  dL/ds of all three
// losses has the form  C_q * g(s_k) * exp(beta * s_k) / sum_k' exp(beta * s_k')  (self-adversarial
// softmax weights, or the softmax of the sampled-softmax cross entropy; beta = 0 gives the
// uniform 1/N): an online-softmax accumulation (running max m, normaliser l, weighted sum
// acc - as in flash attention) needs no second pass.  Every work item writes its partial
// (m, l, acc[W]); k_combine_dq merges the items of a query and applies C_q / l.
struct FuseArgs {
    const float* pos;   // [n_query] positive scores (margin ranking); may be NULL otherwise
    int kind;           // BESS_LOSS_*
    float beta;         // adversarial_scale | 1 (ssce) | 0 (uniform weights)
    float margin;
    float shift;        // ssce: log(n_entity - 1) - log(N), added to the negative scores
    float* st_ml;       // [n_query, items, 2]
    float* st_acc;      // [n_query, items, W]
    const uint8_t* mask = nullptr;  // [mask_rows (1 | n_query), mask_cols] over the last mask_cols columns, or NULL
    int64_t mask_rows = 0;
    int mask_cols = 0, mask_from = 0;
};

// (host side) the loss descriptor's part of it
static FuseArgs fuse_args(const bess_loss_desc* l, const float* pos, float* st_ml, float* st_acc) {
    FuseArgs f;
    f.pos = pos;
    f.kind = l->kind;
    f.beta = l->kind == BESS_LOSS_SSCE ? 1.f : (l->adversarial ? l->adversarial_scale : 0.f);
    f.margin = l->margin;
    f.shift = l->kind == BESS_LOSS_SSCE ? l->ssce_shift : 0.f;
    f.st_ml = st_ml;
    f.st_acc = st_acc;
    return f;
}

__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

template <typename T, int VEC, int IT, int RED, int UNROLL, bool FUSE>
__global__ __launch_bounds__(256) void k_neg_pertriple_fwd(NegPtArgs a, float* __restrict__ out,
                                                           int64_t ld_out, FuseArgs f) {
    const int lane = threadIdx.x & 63;
    const int g = lane & 15;
    const int sub = lane >> 4;
    const int64_t item = blockIdx.x * 4ll + (threadIdx.x >> 6);
    if (item >= a.n_query * a.items_per_query) return;
    const int64_t q = item / a.items_per_query;
    const int k0 = static_cast<int>(item - q * a.items_per_query) * a.nb;
    const int k1 = min(k0 + a.nb, a.n_neg);

    // query chunks -> registers (f32, chunk c covers scalars [c*VEC, c*VEC+VEC))
    float qv[IT][VEC];
    const float* qp = a.query + q * a.W;
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        load_chunk<float, VEC>(qp, g + 16 * it, a.nch, qv[it]);
    }

    const T* base = static_cast<const T*>(a.base);
    const int32_t* idx = a.idx + q * a.n_neg;
    float* orow = out + q * ld_out;
    // online-softmax state of this 16-lane row group (FUSE)
    float fm = -INFINITY, fl = 0.f, facc[IT][VEC];
    float fpos = 0.f;
    if (FUSE) {
#pragma unroll
        for (int it = 0; it < IT; ++it)
#pragma unroll
            for (int v = 0; v < VEC; ++v) facc[it][v] = 0.f;
        if (f.kind == BESS_LOSS_MARGIN) fpos = f.pos[q];
    }

    // the row index of the *next* group of rows is fetched while the current rows are in
    // flight: no row load waits behind its own index load (matters most for short rows)
    int32_t nrow[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) nrow[u] = idx[min(k0 + sub + 4 * u, k1 - 1)];
    for (int kb = k0; kb < k1; kb += 4 * UNROLL) {  // kb is wave-uniform
        float ev[UNROLL][IT][VEC];
        bool valid[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int k = kb + sub + 4 * u;
            valid[u] = k < k1;
            const T* rp = base + static_cast<int64_t>(nrow[u]) * a.W;  // clamped: keeps the wave converged
            nrow[u] = idx[min(k + 4 * UNROLL, k1 - 1)];
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                load_chunk<T, VEC>(rp, g + 16 * it, a.nch, ev[u][it]);
            }
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            float acc = 0.f;
#pragma unroll
            for (int it = 0; it < IT; ++it) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    if (RED == RED_DOT) {
                        acc = fmaf(qv[it][v], ev[u][it][v], acc);
                    } else if (RED == RED_L1) {
                        acc += fabsf(qv[it][v] - ev[u][it][v]);
                    } else {
                        acc += lp_term(qv[it][v] - ev[u][it][v], a.p);
                    }
                }
            }
            acc = row16_allreduce_sum(acc);
            if (RED == RED_L2) acc = lp_root(acc, a.p);
            float sc = a.sign * acc;
            if (FUSE && f.mask && valid[u]) {
                // K7 inside the pass (the padding mask of triple-specific negatives): a masked-out candidate gets
                // BESS_BAD_NEGATIVE_SCORE added before it is stored and before it enters the softmax
                const int kcol = kb + sub + 4 * u - f.mask_from;
                const int64_t mrow = f.mask_rows == 1 ? 0 : q;
                if (kcol >= 0 && f.mask[mrow * f.mask_cols + kcol] == 0) sc += BESS_BAD_NEGATIVE_SCORE;
            }
            if (g == 0 && valid[u]) orow[kb + sub + 4 * u] = a.accum ? orow[kb + sub + 4 * u] + sc : sc;
            if (FUSE && valid[u]) {  // uniform within the 16-lane group
                const float z = f.beta * (sc + f.shift);
                const float m_new = fmaxf(fm, z);
                const float corr = expf(fm - m_new);
                const float e = expf(z - m_new);
                float gs = 1.f;
                if (f.kind == BESS_LOSS_LOGSIGMOID) gs = sigmoid_f(sc + f.margin);
                else if (f.kind == BESS_LOSS_MARGIN) gs = (sc - fpos + f.margin > 0.f) ? 1.f : 0.f;
                const float p = e * gs;
                fl = fmaf(fl, corr, e);
                fm = m_new;
                const float inv_norm = RED == RED_L2 ? lp_inv(acc, a.p) : 0.f;
#pragma unroll
                for (int it = 0; it < IT; ++it)
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        float dsdq;  // d score / d query_w
                        if (RED == RED_DOT) dsdq = ev[u][it][v];
                        else if (RED == RED_L1) dsdq = -sgnf(qv[it][v] - ev[u][it][v]);
                        else dsdq = -lp_dterm(qv[it][v] - ev[u][it][v], a.p) * inv_norm;
                        facc[it][v] = fmaf(facc[it][v], corr, p * dsdq);
                    }
            }
        }
    }
    if (FUSE) {
        // merge the four row groups of the wave, then one partial per work item
        float m_all = fmaxf(fm, __shfl_xor(fm, 16, 64));
        m_all = fmaxf(m_all, __shfl_xor(m_all, 32, 64));
        const float sc = (fm == -INFINITY) ? 0.f : expf(fm - m_all);
        float l = fl * sc;
        l += __shfl_xor(l, 16, 64);
        l += __shfl_xor(l, 32, 64);
        const int64_t slot = q * a.items_per_query + (item - q * a.items_per_query);
        if (lane == 0) {
            f.st_ml[slot * 2 + 0] = m_all;
            f.st_ml[slot * 2 + 1] = l;
        }
        float* ap = f.st_acc + slot * a.W;
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int c = g + 16 * it;
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                float x = facc[it][v] * sc;
                x += __shfl_xor(x, 16, 64);
                x += __shfl_xor(x, 32, 64);
                if (sub == 0 && c < a.nch) ap[c * VEC + v] = x;
            }
        }
    }
}

// ---- K5s: the plain forward in row order, for tables whose rows are each scored many times --------------------
//
// k_neg_pertriple_fwd reads n_query * n_neg random rows; with more pairs than table rows (C2: 1 M pairs over 93,773
// rows, each row ~11 times) nearly every read still comes from the Infinity Cache: a row's uses arrive from waves on
// all eight XCDs at random times, and one XCD's 4 MiB L2 holds 2 % of a 192 MB table.  This kernel scores the same
// pairs in an order that keeps a row's uses on one XCD and close together in time:
//
// - a query block (up to 32 queries x a chunk of their negatives, <= SW_PMAX pairs) is served by eight workgroups, labels
//   l = blockIdx.x % 8 (blocks b and b + 8 share an XCD under the observed round-robin placement: a speed hint only);
// - each of the eight reads the block's indices, builds the same histogram over coarse row buckets in LDS and takes
//   the l-th eighth of the block's pairs in (bucket, position) order - identical data, identical split, no
//   communication: every pair is scored exactly once wherever the blocks run, and with skewed indices (one hot row)
//   every label still gets 1/8 of the pairs.  Only the (at most two) buckets cut by the share's ends need the
//   position order (ballot ranks); the pairs of the other buckets take slots by LDS atomics;
// - the share (<= SW_PMAX / 8 pairs, bucket-sorted in LDS) is dealt to the 16-lane groups front to back in runs of
//   4 * UNROLL per wave: the workgroup walks its row range in order, and all workgroups of an XCD walk about the same
//   range in step (no inter-workgroup synchronisation);
// - the block's queries are staged in LDS in the chunk layout of the registers of k_neg_pertriple_fwd (16 lanes read
//   256 contiguous bytes per ds_read_b128: conflict-free without padding); a group's pairs belong to any query.
//
// Per pair the arithmetic is that of k_neg_pertriple_fwd in the same order (chunks g + 16 it, the same fmaf / fabsf /
// lp_term sequence, row16_allreduce_sum, lp_root, sign): the scores are bitwise equal.  Plain forward only (no fused
// loss, one column window, no accumulation); run() takes it when the caller gives the table's row count.
constexpr int SW_NB = 1024;                 // row buckets of the histogram
constexpr int SW_PMAX = 8192;               // pairs of one block chunk: qb queries x up to SW_PMAX / qb negatives
constexpr int SW_PPT = SW_PMAX / 256;       // pairs per thread while sorting
constexpr int SW_SHARE = SW_PMAX / 8;       // entries of one label's share
constexpr int SW_QFLOATS = 16384;           // LDS for the staged queries (64 KiB): qb = min(32, this / row stride)
constexpr int64_t SW_REUSE_MIN = 4;         // pairs per table row from which run() takes the sweep

struct SweepArgs {
    int qb;        // queries per block
    int kc;        // negatives per block chunk
    int n_kchunks;
    int shift;     // bucket of row r: min(r >> shift, SW_NB - 1)
    int qstride;   // floats per staged query (IT * 16 * VEC)
};

// acc + d * d in two roundings: lp_term's p == 2 term as k_neg_pertriple_fwd adds it, where the product comes out of
// the branch on p and is never fused into the sum (see the note at lp_term in common.h: the two must change together;
// tests/test_pertriple_l2_sweep.py and test_pertriple_sweep_pipeline.py compare them bit for bit)
__device__ __forceinline__ float add_square(float acc, float d) {
#pragma clang fp contract(off)
    const float m = d * d;
    return acc + m;
}

// The sweep of one wave over its entries e0, e0 + 16 UNROLL, ... < n of the share (e0 < n), software-pipelined: two
// register sets of UNROLL rows as loaded (table type: converted when scored); the rows of iteration i + 1 are issued
// before iteration i is scored, so a wave has row loads in flight all the time but in its last iteration, which
// issues nothing.  The loop holds no branch around a load (the compiler's wait counts stay exact) and every row
// address comes from an entry clamped into [0, n).  Lanes past the row's end read its last chunk and score zeros, as
// load_chunk gives them.
// !PIPE: one register set, each iteration waits for its own rows - for the p-norms that go through powf, which are
// bound by that arithmetic and whose scoring code leaves no room for a second set; PIPE with RED_L2 means p == 2.
template <typename T, int VEC, int IT, int RED, int UNROLL, bool PIPE>
__device__ __forceinline__ void sweep_share(const NegPtArgs& a, const float* qs, int qstride, const int2* ent, int n,
                                            int e0, float* __restrict__ oblk, int64_t ld_out) {
    typedef T raw_t __attribute__((ext_vector_type(VEC)));
    constexpr int STEP = 16 * UNROLL;
    const int g = threadIdx.x & 15;
    const int sub = (threadIdx.x & 63) >> 4;
    const T* base = static_cast<const T*>(a.base);
    auto entries = [&](int e, int2(&x)[UNROLL]) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) x[u] = ent[min(e + sub + 4 * u, n - 1)];  // clamped: keeps the wave converged
    };
    auto issue = [&](const int2(&x)[UNROLL], raw_t(&r)[UNROLL][IT]) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const T* rp = base + static_cast<int64_t>(x[u].x) * a.W;
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                r[u][it] = *reinterpret_cast<const raw_t*>(rp + min(g + 16 * it, a.nch - 1) * VEC);
            }
        }
    };
    auto score = [&](const int2(&x)[UNROLL], const raw_t(&r)[UNROLL][IT], int e) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int qi = x[u].y >> 16;
            const int kk = x[u].y & 0xffff;
            const float* qp = qs + qi * qstride;
            float acc = 0.f;
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                float qv[VEC];
                VecLoad<float, VEC>::load(qp + (g + 16 * it) * VEC, qv);
                const bool live = g + 16 * it < a.nch;
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    const float ev = live ? static_cast<float>(r[u][it][v]) : 0.f;
                    if (RED == RED_DOT) {
                        acc = fmaf(qv[v], ev, acc);
                    } else if (RED == RED_L1) {
                        acc += fabsf(qv[v] - ev);
                    } else if (PIPE) {
                        acc = add_square(acc, qv[v] - ev);
                    } else {
                        acc += lp_term(qv[v] - ev, a.p);
                    }
                }
            }
            acc = row16_allreduce_sum(acc);
            if (RED == RED_L2) acc = PIPE ? sqrtf(acc) : lp_root(acc, a.p);
            if (g == 0 && e + sub + 4 * u < n) oblk[qi * ld_out + kk] = a.sign * acc;
        }
    };

    raw_t r0[UNROLL][IT], r1[UNROLL][IT];
    int2 x0[UNROLL], x1[UNROLL], nx[UNROLL];  // nx: the entries of the iteration after the one in flight
    entries(e0, x0);
    if (!PIPE) {
        for (; e0 < n; e0 += STEP) {
            issue(x0, r0);
            entries(e0 + STEP, x1);
            score(x0, r0, e0);
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) x0[u] = x1[u];
        }
        return;
    }
    entries(e0 + STEP, nx);
    issue(x0, r0);
    // two iterations per trip, one per register set; the loop's only exit is at its top, so that no path on which a
    // set is still in flight leads back into it
    for (; e0 + 2 * STEP < n; e0 += 2 * STEP) {  // e0 is wave-uniform
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) x1[u] = nx[u];
        entries(e0 + 2 * STEP, nx);
        issue(x1, r1);
        score(x0, r0, e0);
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) x0[u] = nx[u];
        entries(e0 + 3 * STEP, nx);
        issue(x0, r0);
        score(x1, r1, e0 + STEP);
    }
    // one or two iterations are left, the first of them in flight
    const bool two = e0 + STEP < n;
    if (two) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) x1[u] = nx[u];
        issue(x1, r1);
    }
    score(x0, r0, e0);
    if (two) score(x1, r1, e0 + STEP);
}

template <typename T, int VEC, int IT, int RED, int UNROLL>
__global__ __launch_bounds__(256, 2) void k_neg_pertriple_fwd_sweep(NegPtArgs a, SweepArgs s, float* __restrict__ out,
                                                                    int64_t ld_out) {
    // (static arrays of whole 16-B units: the dynamic region after them stays 16-B aligned)
    extern __shared__ __attribute__((aligned(16))) float qs[];  // [qb][IT * 16 chunks][VEC]
    __shared__ int hist[SW_NB + 4];  // counts, then bucket starts (hist[SW_NB] = P), then slot cursors
    __shared__ int2 ent[SW_SHARE];  // (row, qi << 16 | k - kc0)
    __shared__ int rk[2][SW_PPT * 4];
    __shared__ int wsum[4];
    __shared__ int cut[4];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int label = blockIdx.x & 7;
    const int bc = blockIdx.x >> 3;
    const int qblk = bc / s.n_kchunks;
    const int kch = bc - qblk * s.n_kchunks;
    const int64_t q0 = static_cast<int64_t>(qblk) * s.qb;
    const int nqb = static_cast<int>(min(static_cast<int64_t>(s.qb), a.n_query - q0));
    const int kc0 = kch * s.kc;
    const int kcn = min(s.kc, a.n_neg - kc0);
    const int P = nqb * kcn;
    const int lo = static_cast<int>((static_cast<int64_t>(label) * P) >> 3);
    const int hi = static_cast<int>((static_cast<int64_t>(label + 1) * P) >> 3);

    // queries -> LDS (zeros past the row's end, as load_chunk gives the registers of k_neg_pertriple_fwd)
    for (int i = tid; i < nqb * IT * 16; i += 256) {
        const int qi = i / (IT * 16);
        const int c = i - qi * (IT * 16);
        float v[VEC];
        load_chunk<float, VEC>(a.query + (q0 + qi) * a.W, c, a.nch, v);
#pragma unroll
        for (int j = 0; j < VEC; ++j) qs[qi * s.qstride + c * VEC + j] = v[j];
    }
    for (int b = tid; b < SW_NB; b += 256) hist[b] = 0;
    if (tid < 2) cut[tid] = -1;
    // the block's row ids: pair p = qi * kcn + kk, thread tid holds p = tid + 256 j
    int rr[SW_PPT];
#pragma unroll
    for (int j = 0; j < SW_PPT; ++j) {
        const int p = tid + 256 * j;
        rr[j] = 0;
        if (p < P) {
            const int qi = p / kcn;
            rr[j] = a.idx[(q0 + qi) * a.n_neg + kc0 + (p - qi * kcn)];
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SW_PPT; ++j)
        if (tid + 256 * j < P) atomicAdd(&hist[min(static_cast<unsigned>(rr[j]) >> s.shift, SW_NB - 1u)], 1);
    __syncthreads();

    // exclusive scan of the counts (4 buckets per thread); note the buckets that the share's ends cut
    {
        int c[4], sum = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            c[i] = hist[4 * tid + i];
            sum += c[i];
        }
        int incl = sum;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int y = __shfl_up(incl, off, 64);
            if (lane >= off) incl += y;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int run = incl - sum;
        for (int w = 0; w < wave; ++w) run += wsum[w];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int b = 4 * tid + i;
            hist[b] = run;
            if (run < lo && lo < run + c[i]) cut[0] = b;
            if (run < hi && hi < run + c[i]) cut[1] = b;
            run += c[i];
        }
        if (tid == 255) hist[SW_NB] = run;
    }
    __syncthreads();

    // ranks in position order inside the cut buckets: per (j, wave) counts, scanned by wave 0
    const int cut0 = cut[0], cut1 = cut[1];
    const uint64_t lt = (1ull << lane) - 1ull;
#pragma unroll
    for (int j = 0; j < SW_PPT; ++j) {
        const bool live = tid + 256 * j < P;
        const unsigned b = min(static_cast<unsigned>(rr[j]) >> s.shift, SW_NB - 1u);
        const uint64_t m0 = __ballot(live && static_cast<int>(b) == cut0);
        const uint64_t m1 = __ballot(live && static_cast<int>(b) == cut1);
        if (lane == 0) {
            rk[0][j * 4 + wave] = __popcll(m0);
            rk[1][j * 4 + wave] = __popcll(m1);
        }
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int x0 = rk[h][2 * lane], x1 = rk[h][2 * lane + 1];
            int incl = x0 + x1;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int y = __shfl_up(incl, off, 64);
                if (lane >= off) incl += y;
            }
            rk[h][2 * lane] = incl - x0 - x1;
            rk[h][2 * lane + 1] = incl - x1;
        }
    }
    __syncthreads();

    // slot of each pair in the share: >= 0 fixed (cut buckets), -2 by atomic (whole bucket inside), -1 not ours
    int slot[SW_PPT];
#pragma unroll
    for (int j = 0; j < SW_PPT; ++j) {
        const bool live = tid + 256 * j < P;
        const unsigned b = min(static_cast<unsigned>(rr[j]) >> s.shift, SW_NB - 1u);
        const bool in0 = live && static_cast<int>(b) == cut0;
        const bool in1 = live && static_cast<int>(b) == cut1 && !in0;
        const uint64_t m0 = __ballot(in0);
        const uint64_t m1 = __ballot(in1);
        const int b0 = live ? hist[b] : 0, b1 = live ? hist[b + 1] : 0;
        slot[j] = -1;
        if (live) {
            if (in0 || in1) {
                const int r = in0 ? rk[0][j * 4 + wave] + __popcll(m0 & lt) : rk[1][j * 4 + wave] + __popcll(m1 & lt);
                const int pos = b0 + r;
                if (pos >= lo && pos < hi) slot[j] = pos - lo;
            } else if (b0 >= lo && b1 <= hi) {
                slot[j] = -2;
            }
        }
    }
    __syncthreads();  // hist[] is now the slot cursor of the buckets inside the share
#pragma unroll
    for (int j = 0; j < SW_PPT; ++j) {
        const int p = tid + 256 * j;
        if (slot[j] == -1) continue;
        const unsigned b = min(static_cast<unsigned>(rr[j]) >> s.shift, SW_NB - 1u);
        const int e = slot[j] >= 0 ? slot[j] : atomicAdd(&hist[b], 1) - lo;
        const int qi = p / kcn;
        ent[e] = make_int2(rr[j], (qi << 16) | (p - qi * kcn));
    }
    __syncthreads();

    // the sweep (sweep_share): in its i-th iteration, 16-lane group `sub` of wave `wave` scores the entries
    // i * 16 * UNROLL + wave * 4 * UNROLL + sub + 4 u, u < UNROLL
    const int n = hi - lo;
    // wave-uniform, and through readfirstlane the compiler knows it: the loop's counter and branches are scalar
    const int e0 = __builtin_amdgcn_readfirstlane(wave) * 4 * UNROLL;
    // A wave without an entry loads nothing: ent[] holds n entries and is uninitialised LDS past them - all of it when
    // the share is empty.  (No barrier follows, so the wave may leave.)
    if (e0 >= n) return;
    float* oblk = out + q0 * ld_out + kc0;
    if (RED == RED_L2 && a.p != 2.f)
        sweep_share<T, VEC, IT, RED, UNROLL, false>(a, qs, s.qstride, ent, n, e0, oblk, ld_out);
    else
        sweep_share<T, VEC, IT, RED, UNROLL, true>(a, qs, s.qstride, ent, n, e0, oblk, ld_out);
}

// d loss / d query from the items' partials, one wave per query (loss_rows.h: combine_dq_row)
__global__ __launch_bounds__(256) void k_combine_dq(const float* __restrict__ st_ml, const float* __restrict__ st_acc,
                                                    int64_t n_query, int items, int W, int kind, float loss_scale,
                                                    const float* __restrict__ pos, const float* __restrict__ weight,
                                                    int64_t weight_len, const float* __restrict__ norm,
                                                    float* __restrict__ d_query) {
    const int64_t q = blockIdx.x * 4ll + (threadIdx.x >> 6);
    if (q >= n_query) return;
    combine_dq_row(st_ml, st_acc, q, items, W, kind, loss_scale, pos, weight, weight_len, norm, d_query + q * W, nullptr);
}

// Backward: d_neg[(q, k), :] = g * df/de ; d_query[q, :] += sum_k g * df/dq  with
// g = d_out[q, k].  f = q.e (DOT) | -||q-e||_1 | -||q-e||_2 (sign folded in).
// Same mapping and the same load discipline as the forward: UNROLL row groups issued back to back,
// unconditional loads at clamped rows, the row ids and score gradients of the next groups fetched
// while the current rows are in flight (the first version of this kernel loaded one row group per
// iteration behind its own index load: 675 us for the launch the forward does in 293).  The per-item
// partial of d_query is added atomically (items_per_query partials per query).
template <typename T, int VEC, int IT, int RED, int UNROLL>
__global__ __launch_bounds__(256) void k_neg_pertriple_bwd(NegPtArgs a,
                                                           const float* __restrict__ d_out,
                                                           int64_t ld_dout,
                                                           float* __restrict__ d_query,
                                                           float* __restrict__ d_neg) {
    const int lane = threadIdx.x & 63;
    const int g = lane & 15;
    const int sub = lane >> 4;
    const int64_t item = blockIdx.x * 4ll + (threadIdx.x >> 6);
    if (item >= a.n_query * a.items_per_query) return;
    const int64_t q = item / a.items_per_query;
    const int k0 = static_cast<int>(item - q * a.items_per_query) * a.nb;
    const int k1 = min(k0 + a.nb, a.n_neg);

    float qv[IT][VEC], dq[IT][VEC];
    const float* qp = a.query + q * a.W;
#pragma unroll
    for (int it = 0; it < IT; ++it) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) dq[it][v] = 0.f;
        load_chunk<float, VEC>(qp, g + 16 * it, a.nch, qv[it]);
    }
    const T* base = static_cast<const T*>(a.base);
    const int32_t* idx = a.idx + q * a.n_neg;
    const float* grow = d_out + q * ld_dout;

    int32_t nrow[UNROLL];
    float ngo[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
        const int kk = min(k0 + sub + 4 * u, k1 - 1);
        nrow[u] = idx[kk];
        ngo[u] = grow[kk];
    }
    // d_query == NULL (it came out of the fused forward) and a bilinear scorer: d f / d e = g * q does not involve
    // the candidate rows - they are not read at all, the kernel only writes d_neg
    const bool need_rows = !(RED == RED_DOT && d_query == nullptr);
    for (int kb = k0; kb < k1; kb += 4 * UNROLL) {  // kb is wave-uniform
        float ev[UNROLL][IT][VEC], go[UNROLL];
        int ks[UNROLL];
        int32_t row_now[UNROLL];
        bool valid[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int k = kb + sub + 4 * u;
            valid[u] = k < k1;
            ks[u] = min(k, k1 - 1);
            const T* rp = base + static_cast<int64_t>(nrow[u]) * a.W;
            row_now[u] = nrow[u];
            go[u] = valid[u] ? a.sign * ngo[u] : 0.f;
            const int kn = min(k + 4 * UNROLL, k1 - 1);
            nrow[u] = idx[kn];
            ngo[u] = grow[kn];
            if (need_rows) {
#pragma unroll
                for (int it = 0; it < IT; ++it) load_chunk<T, VEC>(rp, g + 16 * it, a.nch, ev[u][it]);
            } else {
#pragma unroll
                for (int it = 0; it < IT; ++it)
#pragma unroll
                    for (int v = 0; v < VEC; ++v) ev[u][it][v] = 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            float gg = go[u];
            if (RED == RED_L2) {
                float ss = 0.f;
#pragma unroll
                for (int it = 0; it < IT; ++it)
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        ss += lp_term(qv[it][v] - ev[u][it][v], a.p);
                    }
                ss = row16_allreduce_sum(ss);
                gg *= lp_inv(lp_root(ss, a.p), a.p);
            }
            float* dn = d_neg + (a.dn_by_row ? static_cast<int64_t>(row_now[u]) : q * a.n_neg + ks[u]) * a.W;
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                const int c = g + 16 * it;
                float de[VEC];
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    float dqe;  // d f / d q_w  (d f / d e_w = -dqe for distances)
                    if (RED == RED_DOT) {
                        dqe = gg * ev[u][it][v];
                        de[v] = gg * qv[it][v];
                    } else if (RED == RED_L1) {
                        dqe = gg * sgnf(qv[it][v] - ev[u][it][v]);
                        de[v] = -dqe;
                    } else {
                        dqe = gg * lp_dterm(qv[it][v] - ev[u][it][v], a.p);
                        de[v] = -dqe;
                    }
                    dq[it][v] += dqe;
                }
                if (d_neg && valid[u] && c < a.nch) {  // d_neg == NULL: only d_query is wanted
                    // written once, read much later (by C8 / the update): streamed past the caches - for fp32 tables
                    // (one 16-byte piece per lane and chunk: 645 vs 665 us at C2, 533 vs 658 at C3, 119 vs 155 at C1;
                    // the two pieces per lane of fp16 rows came out 12-16 % slower non-temporal)
                    if constexpr (VEC == 4) {
                        typedef float f4 __attribute__((ext_vector_type(4)));
#pragma unroll
                        for (int v = 0; v < VEC; v += 4) {
                            f4 o = {de[v], de[v + 1], de[v + 2], de[v + 3]};
                            __builtin_nontemporal_store(o, reinterpret_cast<f4*>(dn + c * VEC + v));
                        }
                    } else {
#pragma unroll
                        for (int v = 0; v < VEC; ++v) dn[c * VEC + v] = de[v];
                    }
                }
            }
        }
    }
    if (!d_query) return;
    // combine the four DPP rows, then one atomic per scalar per work item
    float* dqp = d_query + q * a.W;
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int c = g + 16 * it;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            float x = dq[it][v];
            x += __shfl_xor(x, 16, 64);
            x += __shfl_xor(x, 32, 64);
            if (sub == 0 && c < a.nch) {
                if (a.items_per_query == 1) dqp[c * VEC + v] = x;
                else unsafeAtomicAdd(dqp + c * VEC + v, x);
            }
        }
    }
}

// ---- host dispatch ---------------------------------------------------------
template <typename T, int VEC, int IT, int RED>
static void launch_fwd(const NegPtArgs& a, float* out, int64_t ld, const FuseArgs* fuse, hipStream_t st) {
    const int64_t items = a.n_query * a.items_per_query;
    constexpr int EPL = IT * VEC;  // scalars per lane per row
    constexpr int UNROLL = EPL <= 16 ? 4 : (EPL <= 32 ? 2 : 1);
    if (!fuse && a.sweep_shift >= 0) {
        SweepArgs s;
        s.qstride = IT * 16 * VEC;
        s.qb = SW_QFLOATS / s.qstride < 32 ? SW_QFLOATS / s.qstride : 32;
        s.kc = a.n_neg < SW_PMAX / s.qb ? a.n_neg : SW_PMAX / s.qb;
        s.n_kchunks = static_cast<int>(ceil_div(a.n_neg, s.kc));
        s.shift = a.sweep_shift;
        const int64_t blocks = ceil_div(a.n_query, s.qb) * s.n_kchunks * 8;
        const int lds = s.qb * s.qstride * static_cast<int>(sizeof(float));  // <= 64 KiB (+ 13 KiB static)
        k_neg_pertriple_fwd_sweep<T, VEC, IT, RED, UNROLL>
            <<<static_cast<unsigned>(blocks), 256, lds, st>>>(a, s, out, ld);
    } else if (fuse) {
        constexpr int FU = EPL <= 16 ? 2 : 1;  // the running d_query sum takes EPL more registers
        k_neg_pertriple_fwd<T, VEC, IT, RED, FU, true><<<ceil_div(items, 4), 256, 0, st>>>(a, out, ld, *fuse);
    } else {
        k_neg_pertriple_fwd<T, VEC, IT, RED, UNROLL, false><<<ceil_div(items, 4), 256, 0, st>>>(a, out, ld, FuseArgs{});
    }
}
template <typename T, int VEC, int IT, int RED>
static void launch_bwd(const NegPtArgs& a, const float* d_out, int64_t ld, float* dq, float* dn,
                       hipStream_t st) {
    const int64_t items = a.n_query * a.items_per_query;
    constexpr int EPL = IT * VEC;          // scalars per lane per row; the running d_query sum takes EPL registers too
    constexpr int BU = EPL <= 16 ? 2 : 1;  // (as the fused forward)
    k_neg_pertriple_bwd<T, VEC, IT, RED, BU><<<ceil_div(items, 4), 256, 0, st>>>(a, d_out, ld, dq, dn);
}

// negatives per work item of this file's kernels (from 64: grown to ~128 KiB of rows, shrunk to fill the chip)
static int native_nb(const bess_model_desc* d, int64_t n_query, int64_t n_neg) {
    return negatives_per_item(n_query, n_neg, 64, row_bytes_of(d));
}

// Row-ordered plain forward (k_neg_pertriple_fwd_sweep)?  Only where the caller gave the table's row count
// (desc.reserved[1]; 0 = unknown) and each row is scored at least SW_REUSE_MIN times on average: a list that names
// each row about once (a receive buffer, a table far larger than the pairs) gains nothing from the order.  One column
// window only.  Returns the bucket shift (row buckets of 1 << shift rows, at most SW_NB of them), or -1.
static int sweep_shift_for(const bess_model_desc* d, int64_t n_query, int64_t n_neg) {
    if (d->scorer > BESS_COMPLEX || d->width > 16 * 16 * vec_of(d)) return -1;
    const int64_t rows = d->reserved[1];
    if (rows <= 0 || n_query <= 0 || n_neg <= 0 || n_query * n_neg < SW_REUSE_MIN * rows) return -1;
    if (ceil_div(n_query, 8) * ceil_div(n_neg, 256) * 8 >= (1ll << 31)) return -1;  // grid: >= 8 queries x 256 per block
    int shift = 0;
    while (((rows - 1) >> shift) >= SW_NB) ++shift;
    return shift;
}

static int run(const bess_model_desc* d, bool fwd, const float* query, int64_t n_query,
               const void* neg_base, const int32_t* neg_idx, int64_t n_neg, float* out,
               const float* d_out, int64_t ld, float* dq, float* dn, void* stream,
               const FuseArgs* fuse = nullptr) {
    if (int e = check_desc(d)) return e;
    BESS_REQUIRE(n_query >= 0 && n_neg >= 0 && n_neg < (1ll << 31), "neg_score_pertriple: bad sizes");
    if (n_query == 0 || n_neg == 0) return BESS_OK;
    BESS_REQUIRE(query && neg_base && neg_idx, "neg_score_pertriple: NULL pointer");
    BESS_REQUIRE(ld >= n_neg, "neg_score_pertriple: leading dimension %lld < n_neg %lld", (long long)ld,
                 (long long)n_neg);
    if (d->scorer == BESS_BOXE)
        return boxe_negatives(d, fwd, false, query, n_query, neg_base, neg_idx, n_neg, out, d_out, ld, dq, dn,
                              as_stream(stream));
    if (d->scorer == BESS_AFFINE)
        return affine_pertriple(d, fwd, query, n_query, neg_base, neg_idx, n_neg, out, d_out, ld, dq, dn,
                                as_stream(stream));
    const int W = d->width;
    const int vec = vec_of(d);
    NegPtArgs a;
    a.query = query;
    a.base = neg_base;
    a.idx = neg_idx;
    a.n_query = n_query;
    a.n_neg = static_cast<int>(n_neg);
    a.W = W;
    a.nch = W / vec;
    a.nb = native_nb(d, n_query, n_neg);
    a.items_per_query = static_cast<int>(ceil_div(n_neg, a.nb));
    a.sign = is_distance(d->scorer) ? -1.f : 1.f;
    a.p = static_cast<float>(d->norm_p);
    a.dn_by_row = (!fwd && (d->reserved[0] & BESS_FLAG_DNEG_BY_ROW)) ? 1 : 0;
    if (fwd && !fuse) a.sweep_shift = sweep_shift_for(d, n_query, n_neg);
    const int red = reduce_of(d);
    hipStream_t st = as_stream(stream);
    // A 16-lane group keeps 16 x 16 chunks of a row in registers (1024 f32 / 2048 f16 scalars at full vector
    // width).  Wider rows are processed in column windows of that size: the dot product and the p = 1 distance are
    // sums over columns (forward: later windows add to the scores; backward: every window writes its own columns).
    // Not for the p = 2 distance (its square root and its gradient need the whole row) nor for the fused training
    // forward (the softmax needs the finished score): BESS_EUNSUPPORTED, the callers use the shared / two-pass forms.
    const int max_cols = 16 * 16 * vec;
    if (W > max_cols) {
        if (red == RED_L2)
            return fail(BESS_EUNSUPPORTED, "neg_score_pertriple: p = 2 on rows of %d scalars (more than %d)", W, max_cols);
        if (fuse)
            return fail(BESS_EUNSUPPORTED, "neg_score_pertriple: fused training forward on rows of %d scalars (more than %d)",
                        W, max_cols);
    }
    // (cleared only now: a refused call leaves its outputs as they were)
    if (!fwd && a.items_per_query > 1 && dq) {
        hipError_t e = fill_words_async(dq, 0u, n_query * W, st);
        if (e != hipSuccess) return fail(static_cast<int>(e), "memset d_query: %s", hipGetErrorString(e));
    }
    const int64_t sz = scalar_bytes_of(d);
    const int rc = for_each_window(W, max_cols, vec, 1, [&](const ColWindow& win) {
        NegPtArgs w = a;
        w.query = query + win.col0;
        w.base = static_cast<const char*>(neg_base) + win.col0 * sz;
        w.nch = win.nch;
        w.accum = win.col0 > 0;
        const bool ok = dispatch_row_class<NativeRows>(d->dtype, vec, win.it, [&](auto c) {
            using C = decltype(c);
            with_constant<RED_DOT, RED_L1, RED_L2>(red, [&](auto r) {
                constexpr int RED = decltype(r)::value;
                if (fwd) launch_fwd<typename C::T, C::VEC, C::IT, RED>(w, out, ld, fuse, st);
                else launch_bwd<typename C::T, C::VEC, C::IT, RED>(w, d_out, ld, win.at(dq), win.at(dn), st);
            });
        });
        return ok ? BESS_OK : fail(BESS_EUNSUPPORTED, "neg_score_pertriple: row of %d scalars too wide", w.W);
    });
    if (rc) return rc;
    return check_launch(fwd ? "neg_score_pertriple_fwd" : "neg_score_pertriple_bwd");
}

}  // namespace bess

extern "C" int bess_neg_score_pertriple_fwd(const bess_model_desc* d, const float* query,
                                            int64_t n_query, const void* neg_base,
                                            const int32_t* neg_idx, int64_t n_neg, float* out,
                                            int64_t ld_out, void* stream) {
    if (n_query > 0 && n_neg > 0 && !out) return bess::fail(BESS_EINVAL, "neg_score_pertriple_fwd: NULL out");
    return bess::run(d, true, query, n_query, neg_base, neg_idx, n_neg, out, nullptr, ld_out, nullptr,
                     nullptr, stream);
}

extern "C" int bess_neg_score_pertriple_bwd(const bess_model_desc* d, const float* query,
                                            int64_t n_query, const void* neg_base,
                                            const int32_t* neg_idx, int64_t n_neg,
                                            const float* d_out, int64_t ld_dout, float* d_query,
                                            float* d_neg, void* stream) {
    if (n_query > 0 && n_neg > 0 && !(d_out && (d_query || d_neg)))
        return bess::fail(BESS_EINVAL, "neg_score_pertriple_bwd: NULL pointer");
    // (d_query == NULL: only d_neg is wanted - d_query came out of bess_neg_score_pertriple_fwd_dq; DistMult /
    // ComplEx then never read the candidate rows)
    return bess::run(d, false, query, n_query, neg_base, neg_idx, n_neg, nullptr, d_out, ld_dout,
                     d_query, d_neg, stream);
}

extern "C" int bess_neg_pertriple_sweep(const bess_model_desc* d, int64_t n_query, int64_t n_neg, int32_t* sweep) {
    if (int e = bess::check_desc(d)) return e;
    if (!sweep || n_query < 0 || n_neg < 0) return bess::fail(BESS_EINVAL, "neg_pertriple_sweep: bad argument");
    *sweep = bess::sweep_shift_for(d, n_query, n_neg) >= 0 ? 1 : 0;
    return BESS_OK;
}

extern "C" int bess_neg_pertriple_items(const bess_model_desc* d, int64_t n_query, int64_t n_neg, int32_t* items) {
    if (!d || !items || n_query < 0 || n_neg < 0) return bess::fail(BESS_EINVAL, "neg_pertriple_items: bad argument");
    *items = n_neg > 0 ? static_cast<int32_t>(bess::ceil_div(n_neg, bess::native_nb(d, n_query, n_neg)))
                       : 0;
    return BESS_OK;
}

extern "C" int bess_neg_score_pertriple_fwd_dq(const bess_model_desc* d, const bess_loss_desc* l, const float* query,
                                               int64_t n_query, const void* neg_base, const int32_t* neg_idx,
                                               int64_t n_neg, const float* pos, const float* weight,
                                               int64_t weight_len, float* out, int64_t ld_out, float* d_query,
                                               float* state_ml, float* state_acc, void* stream) {
    return bess_neg_score_pertriple_fwd_dq_masked(d, l, query, n_query, neg_base, neg_idx, n_neg, pos, weight, weight_len,
                                                  nullptr, 0, 0, out, ld_out, d_query, state_ml, state_acc, stream);
}

extern "C" int bess_neg_score_pertriple_fwd_dq_masked(const bess_model_desc* d, const bess_loss_desc* l,
                                                      const float* query, int64_t n_query, const void* neg_base,
                                                      const int32_t* neg_idx, int64_t n_neg, const float* pos,
                                                      const float* weight, int64_t weight_len, const uint8_t* mask,
                                                      int64_t mask_rows, int64_t mask_cols, float* out,
                                                      int64_t ld_out, float* d_query, float* state_ml,
                                                      float* state_acc, void* stream) {
    using namespace bess;
    if (int e = check_desc(d)) return e;
    BESS_REQUIRE(l, "neg_score_pertriple_fwd_dq: NULL loss descriptor");
    BESS_REQUIRE(d->scorer <= BESS_COMPLEX, "neg_score_pertriple_fwd_dq: scorer %d has no fused form", d->scorer);
    BESS_REQUIRE(l->kind == BESS_LOSS_LOGSIGMOID || l->kind == BESS_LOSS_MARGIN || l->kind == BESS_LOSS_SSCE,
                 "neg_score_pertriple_fwd_dq: unknown loss %d", l->kind);
    if (n_query <= 0 || n_neg <= 0) return BESS_OK;
    // (d_query may be NULL: the partials are then left for bess_pertriple_tail, which combines them where it uses them)
    BESS_REQUIRE(out && state_ml && state_acc && weight && (weight_len == 1 || weight_len == n_query),
                 "neg_score_pertriple_fwd_dq: NULL pointer or bad weight length");
    BESS_REQUIRE(pos || l->kind == BESS_LOSS_LOGSIGMOID, "neg_score_pertriple_fwd_dq: this loss needs the positive scores");
    FuseArgs f = fuse_args(l, pos, state_ml, state_acc);
    if (mask) {
        BESS_REQUIRE(mask_rows > 0 && mask_cols > 0, "neg_score_pertriple_fwd_dq_masked: mask [%lld, %lld]",
                     (long long)mask_rows, (long long)mask_cols);
        // (a mask this pass does not apply - K7's head / tail halves, mask_rows == 2, or more columns than scores - is
        // "not built", not a bad call: the caller masks with bess_mask_scores and takes the two-pass form)
        if (mask_cols > n_neg || (mask_rows != 1 && mask_rows != n_query))
            return fail(BESS_EUNSUPPORTED,
                        "neg_score_pertriple_fwd_dq_masked: mask [%lld, %lld] for %lld queries x %lld negatives",
                        (long long)mask_rows, (long long)mask_cols, (long long)n_query, (long long)n_neg);
        f.mask = mask;
        f.mask_rows = mask_rows;
        f.mask_cols = static_cast<int>(mask_cols);
        f.mask_from = static_cast<int>(n_neg - mask_cols);
    }
    const int rc = run(d, true, query, n_query, neg_base, neg_idx, n_neg, out, nullptr, ld_out, nullptr, nullptr, stream,
                       &f);
    if (rc) return rc;
    const int items = static_cast<int>(ceil_div(n_neg, native_nb(d, n_query, n_neg)));
    if (!d_query) return BESS_OK;  // the partials stay as they are: bess_pertriple_tail combines them where it uses them
    k_combine_dq<<<static_cast<unsigned>(ceil_div(n_query, 4)), 256, 0, as_stream(stream)>>>(
        state_ml, state_acc, n_query, items, d->width, l->kind, l->loss_scale, pos, weight, weight_len, nullptr, d_query);
    return check_launch("neg_score_pertriple_fwd_dq");
}

extern "C" int bess_neg_score_pertriple_fwd_partials(const bess_model_desc* d, const bess_loss_desc* l,
                                                     const float* query, int64_t n_query, const void* neg_base,
                                                     const int32_t* neg_idx, int64_t n_neg, float* out,
                                                     int64_t ld_out, float* state_ml, float* state_acc, void* stream) {
    using namespace bess;
    if (int e = check_desc(d)) return e;
    BESS_REQUIRE(l, "neg_score_pertriple_fwd_partials: NULL loss descriptor");
    BESS_REQUIRE(d->scorer <= BESS_COMPLEX, "neg_score_pertriple_fwd_partials: scorer %d has no fused form", d->scorer);
    if (l->kind != BESS_LOSS_LOGSIGMOID && l->kind != BESS_LOSS_SSCE)
        return fail(BESS_EUNSUPPORTED, "neg_score_pertriple_fwd_partials: loss %d weighs a negative by the positive score, "
                                       "which the scoring shard does not have", l->kind);
    if (n_query <= 0 || n_neg <= 0) return BESS_OK;
    BESS_REQUIRE(out && state_ml && state_acc, "neg_score_pertriple_fwd_partials: NULL pointer");
    FuseArgs f = fuse_args(l, nullptr, state_ml, state_acc);
    return run(d, true, query, n_query, neg_base, neg_idx, n_neg, out, nullptr, ld_out, nullptr, nullptr, stream, &f);
}

extern "C" int bess_combine_dq_partials(const float* state_ml, const float* state_acc, int64_t n_query, int32_t items,
                                        int32_t width, const float* norm, float* d_query, void* stream) {
    using namespace bess;
    BESS_REQUIRE(n_query >= 0 && items > 0 && width > 0, "combine_dq_partials: bad sizes");
    if (n_query == 0) return BESS_OK;
    BESS_REQUIRE(state_ml && state_acc && norm && d_query, "combine_dq_partials: NULL pointer");
    k_combine_dq<<<static_cast<unsigned>(ceil_div(n_query, 4)), 256, 0, as_stream(stream)>>>(
        state_ml, state_acc, n_query, items, width, 0, 1.f, nullptr, nullptr, 1, norm, d_query);
    return check_launch("combine_dq_partials");
}
