// The relation-grouped query product on the CDNA4 matrix cores: a grouped GEMM in which every row of the left operand
// is multiplied by the matrix of its own relation, and its two gradients (exact fp32, v_mfma_f32_32x32x2_f32):
//
//     q[m, n]      = sum_j x[m, j] B_{rel[m]}(j, n)          B_r(j, n) = M_r[j, n], with exchanged axes M_r[n, j]
//     d_x[m, j]    = sum_n dq[m, n] B_{rel[m]}(j, n)         the same product with the axes exchanged once more
//     d_M[r][a, b] = sum_{m : rel[m] = r} u[m, a] v[m, b]    (u, v) = (x, dq) or, with exchanged axes, (dq, x)
//
// M [n_rel, de * de] holds one row-major de x de matrix per relation.  RESCAL is this product on its relation table;
// TuckER's relation route is this product on M = rel_table @ core.  The batch arrives grouped by relation as a segment
// index (bess_build_segment_index over the relation ids): segment s is relation seg_rows[s] and holds the batch rows
// refs_sorted[seg_offsets[s] .. seg_offsets[s + 1]).  Its length *n_seg is only known on the device and stays there.
//
//   k_relq_plan      one workgroup: cuts every segment into row tiles of 64 - (segment, first sorted row, rows) - so
//                    that no tile spans two relations; writes their count.  The host launches the upper bound
//                    ceil(S / 64) + min(S, n_rel); workgroups past the count leave at once
//   k_relq_fwd       q and d_x: one 64 x 64 tile per workgroup.  The 64 rows of x are gathered through refs_sorted,
//                    the relation's matrix is read in place along either axis; both operands stream through LDS in
//                    slices of 32 (double-buffered), so de has no limit.  Every row of q is written once, at its
//                    original position
//   k_relq_bwd_mat   one 64 x 64 tile of one present relation's gradient matrix per workgroup, reduction over the
//                    segment's rows; both operands are "reduction index = row" images gathered through refs_sorted
//
// Tile, images and staging helpers are mfma_tile.h's.  No atomics anywhere: every output element is written once, by
// one lane, in a fixed order of summation.
#include "common.h"
#include "mfma_tile.h"

namespace bess {
namespace {

constexpr int PLAN_HEAD = 4;  // words in front of the tiles: [0] their count; the tiles start on a 16-byte boundary

// workspace: int32 [PLAN_HEAD] | tile_first [max_seg + 1] (first tile of every segment) | tiles [max_tiles] x int4
inline int64_t max_segments(int64_t S, int64_t n_rel) { return S < n_rel ? S : n_rel; }
inline int64_t max_tiles(int64_t S, int64_t n_rel) { return ceil_div(S, TT) + max_segments(S, n_rel); }
inline int64_t tile_first_words(int64_t S, int64_t n_rel) { return (max_segments(S, n_rel) + 1 + 3) / 4 * 4; }
inline int64_t plan_bytes(int64_t S, int64_t n_rel) {
    return (PLAN_HEAD + tile_first_words(S, n_rel) + 4 * max_tiles(S, n_rel)) * 4;
}

// Phase 1: tile_first[s] = tiles of the segments before s, 256 segments per round (Hillis-Steele scan in LDS).
// Phase 2: one thread per tile finds its segment by bisection of tile_first - a segment of any length costs no thread
// more than the others.
__global__ __launch_bounds__(256) void k_relq_plan(const int32_t* __restrict__ seg_offsets, const int32_t* __restrict__ n_seg,
                                                   int max_seg, int32_t* __restrict__ head,
                                                   int32_t* __restrict__ tile_first, int4* __restrict__ tiles) {
    __shared__ int scan[256];
    __shared__ int carry;
    const int t = threadIdx.x, ns = min(*n_seg, max_seg);  // (more: ids outside [0, n_rel), refused by the header)
    if (t == 0) carry = 0;
    __syncthreads();
    for (int s0 = 0; s0 < ns; s0 += 256) {
        const int s = s0 + t;
        const int mine = s < ns ? (seg_offsets[s + 1] - seg_offsets[s] + TT - 1) / TT : 0;
        scan[t] = mine;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const int add = t >= d ? scan[t - d] : 0;
            __syncthreads();
            scan[t] += add;
            __syncthreads();
        }
        if (s < ns) tile_first[s] = carry + scan[t] - mine;
        __syncthreads();
        if (t == 255) carry += scan[255];
        __syncthreads();
    }
    const int total = carry;
    if (t == 0) {
        tile_first[ns] = total;
        head[0] = total;
    }
    __syncthreads();  // tile_first, written by this workgroup, is visible to it
    for (int i = t; i < total; i += 256) {
        int lo = 0, hi = ns - 1;  // the last segment with tile_first[s] <= i (every segment has a tile)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (tile_first[mid] <= i) lo = mid;
            else hi = mid - 1;
        }
        const int first = seg_offsets[lo] + (i - tile_first[lo]) * TT;
        tiles[i] = make_int4(lo, first, min(TT, seg_offsets[lo + 1] - first), 0);
    }
}

struct FwdArgs {
    const float* x;  // [S, de], rows in batch order
    const float* M;  // [n_rel, de * de]
    float* q;        // [S, de]
    const int32_t* refs_sorted;
    const int32_t* seg_rows;
    const int32_t* head;
    const int4* tiles;
    int64_t ldx, ldm, ldq;
    int de;
};

// grid (tile bound, ceil(de / 64)): the tiles of one column block are neighbours, so the tiles of one long segment
// read the same slices of its matrix at about the same time.  LDS: [2][32 x 65] of x, [2][32 x 68] of B_r.
template <bool SWAP, bool VEC4>
__global__ __launch_bounds__(256) void k_relq_fwd(FwdArgs A) {
    if (static_cast<int>(blockIdx.x) >= A.head[0]) return;
    __shared__ __attribute__((aligned(16))) float Xs[2][B_IMG];
    __shared__ __attribute__((aligned(16))) float Bs[2][B_IMG];
    __shared__ int row_of[TT];  // batch row of the tile's row (-1: past the segment)
    using Slice = MatrixSlice<SWAP, VEC4>;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int l31 = lane & 31, lk = lane >> 5;
    const int4 tile = A.tiles[blockIdx.x];  // (segment, first sorted row, rows, -)
    const int64_t de = A.de, n0 = static_cast<int64_t>(blockIdx.y) * TT;
    const float* const mat = A.M + A.seg_rows[tile.x] * A.ldm;
    if (t < TT) row_of[t] = t < tile.z ? A.refs_sorted[tile.y + t] : -1;

    // this thread's two rows of the gathered x tile (rows past the segment: the tile's first row, loaded as zeros)
    const float* xrow[2];
    bool live[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int m = p * 32 + (t >> 3);
        live[p] = m < tile.z;
        xrow[p] = A.x + A.refs_sorted[tile.y + (live[p] ? m : 0)] * A.ldx;
    }
    float xv[2][4];
    auto load_x = [&](int64_t j0) {
#pragma unroll
        for (int p = 0; p < 2; ++p) load4<VEC4>(xrow[p], j0 + (t & 7) * 4, de, live[p], xv[p]);
    };
    Slice bs;
    load_x(0);
    bs.load(mat, de, 0, n0);
    store_transposed(Xs[0], xv);
    bs.store(Bs[0]);
    f32x16 acc;
    zero_acc(acc);
    __syncthreads();
    const int n_slice = (A.de + TK - 1) / TK;
    for (int s = 0; s < n_slice; ++s) {
        const int cur = s & 1;
        const bool more = s + 1 < n_slice;
        if (more) {  // issued ahead of this slice's MFMAs
            load_x(static_cast<int64_t>(s + 1) * TK);
            bs.load(mat, de, static_cast<int64_t>(s + 1) * TK, n0);
        }
        // a wave whose 32 rows are all past the segment (short segments: the usual case with many relations) idles
        if (wm < tile.z) mfma_slice<LD_T, Slice::LD, false>(Xs[cur], Bs[cur], acc, wm, wn, l31, lk, 1.f);
        if (more) {
            store_transposed(Xs[cur ^ 1], xv);
            bs.store(Bs[cur ^ 1]);
        }
        __syncthreads();
    }
    const int64_t col = n0 + wn + l31;
    if (col < de) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = row_of[wm + acc_row(r, lk)];
            if (row >= 0) A.q[row * A.ldq + col] = acc[r];
        }
    }
}

// d_M[seg_rows[s]][a0 .., b0 ..] = sum over the rows m of segment s of u[m, a] v[m, b].
// grid (segment bound, ceil(de / 64), ceil(de / 64)): segment, a tile, b tile.
template <bool VEC4>
__global__ __launch_bounds__(256) void k_relq_bwd_mat(const float* __restrict__ u, int64_t ldu, const float* __restrict__ v,
                                                      int64_t ldv, const int32_t* __restrict__ refs_sorted,
                                                      const int32_t* __restrict__ seg_rows,
                                                      const int32_t* __restrict__ seg_offsets,
                                                      const int32_t* __restrict__ n_seg, float* __restrict__ d_M,
                                                      int64_t lddm, int de) {
    if (static_cast<int>(blockIdx.x) >= *n_seg) return;
    __shared__ __attribute__((aligned(16))) float Us[2][B_IMG];
    __shared__ __attribute__((aligned(16))) float Vs[2][B_IMG];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int l31 = lane & 31, lk = lane >> 5;
    const int64_t a0 = static_cast<int64_t>(blockIdx.y) * TT, b0 = static_cast<int64_t>(blockIdx.z) * TT;
    const int r0 = seg_offsets[blockIdx.x], r1 = seg_offsets[blockIdx.x + 1];  // r1 > r0: a segment is never empty
    float* const out = d_M + seg_rows[blockIdx.x] * lddm;
    float su[2][4], sv[2][4];
    auto load = [&](int ms) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int m = r0 + ms + p * 16 + (t >> 4);
            const int64_t row = refs_sorted[min(m, r1 - 1)];
            const int64_t c = (t & 15) * 4;
            load4<VEC4>(u + row * ldu, a0 + c, de, m < r1, su[p]);
            load4<VEC4>(v + row * ldv, b0 + c, de, m < r1, sv[p]);
        }
    };
    load(0);
    store_direct(Us[0], su);
    store_direct(Vs[0], sv);
    f32x16 acc;
    zero_acc(acc);
    __syncthreads();
    const int n_slice = (r1 - r0 + TK - 1) / TK;
    for (int s = 0; s < n_slice; ++s) {
        const int cur = s & 1;
        const bool more = s + 1 < n_slice;
        if (more) load((s + 1) * TK);
        mfma_slice<LD_D, LD_D, false>(Us[cur], Vs[cur], acc, wm, wn, l31, lk, 1.f);
        if (more) {
            store_direct(Us[cur ^ 1], su);
            store_direct(Vs[cur ^ 1], sv);
        }
        __syncthreads();
    }
    const int64_t col = b0 + wn + l31;
    if (col < de) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t row = a0 + wm + acc_row(r, lk);
            if (row < de) out[row * de + col] = acc[r];
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------
int check_shape(const char* who, int64_t S, int64_t de, int64_t n_rel) {
    BESS_REQUIRE(S >= 0 && de >= 1 && n_rel >= 1, "%s: S >= 0, de >= 1 and n_rel >= 1 (got %lld, %lld, %lld)", who,
                 static_cast<long long>(S), static_cast<long long>(de), static_cast<long long>(n_rel));
    BESS_REQUIRE(S < (1ll << 22) && de <= 32768 && n_rel < (1ll << 31), "%s: S < 2^22, de <= 32768 and n_rel < 2^31", who);
    return BESS_OK;
}

struct Grouping {
    const int32_t *refs_sorted, *seg_rows, *seg_offsets, *n_seg;
};

struct Plan {
    int32_t *head, *tile_first;
    int4* tiles;
    Plan(void* ws, int64_t S, int64_t n_rel)
        : head(static_cast<int32_t*>(ws)), tile_first(head + PLAN_HEAD),
          tiles(reinterpret_cast<int4*>(tile_first + tile_first_words(S, n_rel))) {}
};

int launch_plan(const Grouping& G, const Plan& P, int64_t S, int64_t n_rel, hipStream_t st) {
    k_relq_plan<<<1, 256, 0, st>>>(G.seg_offsets, G.n_seg, static_cast<int>(max_segments(S, n_rel)), P.head, P.tile_first,
                                   P.tiles);
    return check_launch("relq_plan");
}

// out[m, :] = in[m, :] B_{rel[m]}, for the tiles of `P`
int launch_rows(bool swap, const float* in, int64_t ld_in, const float* M, int64_t ldm, float* out, int64_t ld_out,
                const Grouping& G, const Plan& P, int64_t S, int64_t de, int64_t n_rel, hipStream_t st) {
    const bool vec4 = de % 4 == 0 && ld_in % 4 == 0 && ldm % 4 == 0 && aligned16(in) && aligned16(M);
    const dim3 grid(static_cast<unsigned>(max_tiles(S, n_rel)), static_cast<unsigned>(ceil_div(de, TT)));
    const FwdArgs A{in, M, out, G.refs_sorted, G.seg_rows, P.head, P.tiles, ld_in, ldm, ld_out, static_cast<int>(de)};
    with_flag(swap, [&](auto sw) {
        with_flag(vec4, [&](auto v4) { k_relq_fwd<decltype(sw)::value, decltype(v4)::value><<<grid, 256, 0, st>>>(A); });
    });
    return check_launch("relq_fwd");
}

#define RELQ_CHECK_COMMON(who)                                                                                       \
    if (int rc = check_shape(who, S, de, n_rel)) return rc;                                                          \
    BESS_REQUIRE(swap_axes == 0 || swap_axes == 1, who ": swap_axes is 0 or 1");                                     \
    BESS_REQUIRE(ldx >= de && ldm >= de * de, who ": bad leading dimension")

}  // namespace
}  // namespace bess

using namespace bess;

extern "C" int bess_relation_query_workspace(int64_t S, int64_t de, int64_t n_rel, int64_t* bytes) {
    BESS_REQUIRE(bytes, "relation_query_workspace: NULL pointer");
    if (int rc = check_shape("relation_query_workspace", S, de, n_rel)) return rc;
    *bytes = plan_bytes(S, n_rel);
    return BESS_OK;
}

extern "C" int bess_relation_query_fwd(const float* x, int64_t ldx, const float* M, int64_t ldm, int32_t swap_axes,
                                       const int32_t* refs_sorted, const int32_t* seg_rows, const int32_t* seg_offsets,
                                       const int32_t* n_seg, int64_t S, int64_t de, int64_t n_rel, float* q, int64_t ldq,
                                       void* workspace, int64_t workspace_bytes, void* stream) {
    RELQ_CHECK_COMMON("relation_query_fwd");
    BESS_REQUIRE(ldq >= de, "relation_query_fwd: bad leading dimension");
    if (S == 0) return BESS_OK;
    BESS_REQUIRE(x && M && q && refs_sorted && seg_rows && seg_offsets && n_seg, "relation_query_fwd: NULL pointer");
    BESS_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= plan_bytes(S, n_rel),
                 "relation_query_fwd: workspace too small (bess_relation_query_workspace) or misaligned");
    const Grouping G{refs_sorted, seg_rows, seg_offsets, n_seg};
    const Plan P(workspace, S, n_rel);
    hipStream_t st = as_stream(stream);
    if (int rc = launch_plan(G, P, S, n_rel, st)) return rc;
    return launch_rows(swap_axes != 0, x, ldx, M, ldm, q, ldq, G, P, S, de, n_rel, st);
}

extern "C" int bess_relation_query_bwd(const float* x, int64_t ldx, const float* M, int64_t ldm, int32_t swap_axes,
                                       const int32_t* refs_sorted, const int32_t* seg_rows, const int32_t* seg_offsets,
                                       const int32_t* n_seg, int64_t S, int64_t de, int64_t n_rel, const float* dq,
                                       int64_t lddq, float* d_x, int64_t ld_dx, float* d_M, int64_t lddm,
                                       void* workspace, int64_t workspace_bytes, void* stream) {
    RELQ_CHECK_COMMON("relation_query_bwd");
    BESS_REQUIRE(lddq >= de && (!d_x || ld_dx >= de) && (!d_M || lddm >= de * de), "relation_query_bwd: bad leading dimension");
    const bool swap = swap_axes != 0;
    hipStream_t st = as_stream(stream);
    if (d_M) {  // the matrices of relations that the batch does not name get no other store
        hipError_t e = hipSuccess;
        if (lddm == de * de) e = fill_words_async(d_M, 0u, n_rel * de * de, st);
        else
            for (int64_t r = 0; r < n_rel && e == hipSuccess; ++r) e = fill_words_async(d_M + r * lddm, 0u, de * de, st);
        if (e != hipSuccess) return check_launch("relation_query_bwd: fill");
    }
    if (S == 0) return BESS_OK;
    BESS_REQUIRE(x && M && dq && refs_sorted && seg_rows && seg_offsets && n_seg, "relation_query_bwd: NULL pointer");
    const Grouping G{refs_sorted, seg_rows, seg_offsets, n_seg};
    if (d_x) {  // the forward product of dq along the matrices' other axis
        BESS_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= plan_bytes(S, n_rel),
                     "relation_query_bwd: workspace too small (bess_relation_query_workspace) or misaligned");
        const Plan P(workspace, S, n_rel);
        if (int rc = launch_plan(G, P, S, n_rel, st)) return rc;
        if (int rc = launch_rows(!swap, dq, lddq, M, ldm, d_x, ld_dx, G, P, S, de, n_rel, st)) return rc;
    }
    if (d_M) {
        const float* u = swap ? dq : x;
        const float* v = swap ? x : dq;
        const int64_t ldu = swap ? lddq : ldx, ldv = swap ? ldx : lddq;
        const bool vec4 = de % 4 == 0 && ldu % 4 == 0 && ldv % 4 == 0 && aligned16(u) && aligned16(v);
        const unsigned tiles = static_cast<unsigned>(ceil_div(de, TT));
        const dim3 grid(static_cast<unsigned>(max_segments(S, n_rel)), tiles, tiles);
        with_flag(vec4, [&](auto v4) {
            k_relq_bwd_mat<decltype(v4)::value><<<grid, 256, 0, st>>>(u, ldu, v, ldv, refs_sorted, seg_rows, seg_offsets,
                                                                      n_seg, d_M, lddm, static_cast<int>(de));
        });
        if (int rc = check_launch("relq_bwd_mat")) return rc;
    }
    return BESS_OK;
}
