// The per-element arithmetic of BoxE, shared by the candidate kernels (boxe.hip) and the query / positive-score
// kernels (boxe_query.hip); the formulas are in the header of boxe.hip.
#pragma once

#include "common.h"

namespace bess {

static const char* const BOX_TOO_WIDE =
    "BoxE: embedding size %d too wide for the kernels (max 512; 128 when not a multiple of 4)";

// per element: bumped point (after tanh), distance to the centre, inside flag
template <bool TANH>
__device__ __forceinline__ void box_point(float e, float s, float c, float h, float& xp, float& dist, bool& inside) {
    xp = e + s;
    if (TANH) xp = tanhf(xp);
    dist = fabsf(xp - c);
    inside = dist <= h;
}

__device__ __forceinline__ float box_final(float dist, float h, bool inside) {
    const float B = 1.f + 2.f * h;
    const float A = 1.f / B;
    return inside ? dist * A : dist * B - h * (B - A);
}

// Gradients of one element's f for gp = d loss / d ||f||_p * ||f||_p^(1 - p) (P == 1: d loss / d ||f||_1): with
// respect to the point before its tanh (dx), the centre (dc) and the half width (dh).  `inside` is a constant of the
// backward; sgn(0) = 0 at the kink of the distance.
template <bool TANH, int P>
__device__ __forceinline__ void box_grad(float xp, float dist, float c, float h, bool inside, float gp, float p,
                                         float& dx, float& dc, float& dh) {
    const float B = 1.f + 2.f * h, A = 1.f / B;
    const float f = inside ? dist * A : dist * B - h * (B - A);
    const float df = (P == 1) ? gp * sgnf(f) : gp * lp_dterm(f, p);
    const float dd = df * (inside ? A : B) * sgnf(xp - c);
    dc = -dd;
    dh = df * (inside ? -2.f * dist * A * A : 2.f * dist - (B - A) - h * (2.f + 2.f * A * A));
    dx = TANH ? dd * (1.f - xp * xp) : dd;
}

}  // namespace bess
