// K9 of the per-triple negatives (segments.hip, affine.hip, boxe.hip): operands, launches, the long tier's tickets
#pragma once

#include <algorithm>

#include "common.h"

namespace bess {

constexpr int SEG_CAP = BESS_SEGMENT_CAP;  // longer segments go to the long tier (segments.hip: k_long_segments)

struct SegRefs {  // the index side of the pass: what is summed into which row
    const float* query;
    void* table;                 // read per reference; written where the pass applies the step in place
    const float* d_out;
    int64_t ld_dout;
    const int32_t* refs;         // sorted reference ids (q * n_neg + k)
    const int32_t* seg_rows;     // destination row of each segment
    const int32_t* seg_offsets;  // [n_seg + 1]
    const int32_t* n_seg;        // device scalar
    int n_neg;
    const int32_t* long_segs;    // optional: [0] = number of segments longer than SEG_CAP, [1..] = their ids
    float p;                     // the norm of the RED_L2 / P == 2 kernels (any p != 1)
};
struct SegPass {  // where the sums go, and the scratch of the long tier (zero on entry, left zero)
    int64_t max_seg;
    float* grad_seg;  // != NULL: the per-row gradients; NULL: table[row] -= fused_sgd_lr * sum in place
    float fused_sgd_lr;
    int64_t long_cap;
    float* long_grad;
    int32_t* long_count;
};
int affine_grad_segments(const bess_model_desc* d, const SegRefs& refs, const SegPass& pass, hipStream_t st);
int boxe_grad_segments(const bess_model_desc* d, const SegRefs& refs, const SegPass& pass, hipStream_t st);

// launch(blocks, false): 16 segments per 256-thread workgroup, grid-stride over the (device-side) segment count, the
// workgroups in sets of n_conc; then, with a list of long segments, launch(1024, true) for the rows left out (usually
// none: one launch that finds nothing to do; 16 K groups share the slices).
template <typename F>
int launch_segment_pass(const SegRefs& refs, const SegPass& ps, int n_conc, const char* what, F&& launch) {
    const unsigned grid = static_cast<unsigned>(n_conc * std::min<int64_t>(ceil_div(ps.max_seg, 16), 4096 / n_conc));
    if (int rc = launch(grid, false)) return rc;
    if (refs.long_segs)
        if (int rc = launch(1024u, true)) return rc;
    return check_launch(what);
}

// Long tier: the groups' partial sums of a row's slices meet in long_grad[li, :] through float atomics.  The 16 lanes
// of a group call seg_count_slice once their adds are issued; it returns the row's ticket before this slice.  The
// group with (ticket + 1) % parts == 0 added the last slice: it calls seg_last_slice (the ticket goes back to zero:
// the scratch serves the next launch as it is) and reads the row back with seg_take.
__device__ __forceinline__ int seg_count_slice(int32_t* cnt, int lane, int g) {
    __threadfence();  // this group's adds are performed before its slice is counted
    int old = 0;
    if (g == 0) old = atomicAdd(cnt, 1);
    return __shfl(old, lane & 48, 64);  // from the first lane of the 16-lane group
}
__device__ __forceinline__ void seg_last_slice(int32_t* cnt, int g) {
    if (g == 0) __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
}
__device__ __forceinline__ float seg_take(float* sp) {  // (device-scope load: past the L1); leaves zero behind
    const float v = __hip_atomic_load(sp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(sp, 0.f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return v;
}

}  // namespace bess
