// torchvision's NMS suppression test, shared by the proposal layer / nms op
// (proposal.hip), the FPN proposal layer (fpn_proposal.hip) and the per-class
// detection NMS (detect.hip); and what the column-form NMS of the two proposal
// units is made of: the 64x64 IoU tile and first_bits.  The ballot fixed point
// that resolves a block stays written out in the three sweeps: the plan cases
// (tests/propose_plan_cases.py) read its loops from proposal.hip's text.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstring>

#include "common.h"

namespace frcnn {

// Exact form of torchvision's `(double)(inter / union) > iou_threshold`.
struct NmsThr {
    double thr;    // the raw threshold
    double mid;    // midpoint below the smallest float T with (double)T > thr
    int tie_incl;  // a quotient equal to `mid` rounds up to T
    int never;     // thr is NaN: nothing is ever suppressed
};

static NmsThr make_thr(double thr) {
    NmsThr t{};
    t.thr = thr;
    if (std::isnan(thr)) {
        t.never = 1;
        return t;
    }
    float f = static_cast<float>(thr);
    if (!(static_cast<double>(f) > thr)) f = std::nextafter(f, INFINITY);
    if (std::isinf(f) && f > 0) {
        t.mid = std::ldexp(1.0, 128) - std::ldexp(1.0, 103);  // overflow boundary, ties to inf
        t.tie_incl = 1;
        return t;
    }
    float pred = std::nextafter(f, -INFINITY);
    t.mid = (static_cast<double>(pred) + static_cast<double>(f)) * 0.5;
    uint32_t bits;
    std::memcpy(&bits, &f, 4);
    t.tie_incl = (bits & 1u) == 0;
    return t;
}

// IoU(a, b) > thr with torchvision's fp32 op order.
// Fast path: RN(inter/uni) > thr  <=>  inter >= mid*uni  (exact in fp64, since
// mid has <= 25 and uni 24 significant bits), valid for finite uni > 0.
__device__ __forceinline__ bool iou_over(float4 a, float aarea, float4 b, float barea,
                                         const NmsThr& t) {
    float xx1 = a.x < b.x ? b.x : a.x;
    float yy1 = a.y < b.y ? b.y : a.y;
    float xx2 = b.z < a.z ? b.z : a.z;
    float yy2 = b.w < a.w ? b.w : a.w;
    float w = xx2 - xx1;
    float h = yy2 - yy1;
    w = 0.0f < w ? w : 0.0f;
    h = 0.0f < h ? h : 0.0f;
    float inter = w * h;
    float uni = aarea + barea;
    uni = uni - inter;
    if (uni > 0.0f && uni <= FLT_MAX && inter <= FLT_MAX) {
        double lhs = static_cast<double>(inter);
        double rhs = t.mid * static_cast<double>(uni);
        return lhs > rhs || (t.tie_incl && lhs == rhs);
    }
    float ovr = inter / uni;
    return static_cast<double>(ovr) > t.thr;
}

__device__ __forceinline__ float box_area(float4 b) {
    float dx = b.z - b.x;
    float dy = b.w - b.y;
    return dx * dy;
}

// ---- the column-form 64x64 IoU tile (proposal.hip's stage and first-chunk tiles,
// fpn_proposal.hip's): 256 threads, lane = column, the tile's 64 row boxes and areas
// staged in LDS.  Wave wid tests rows [16 wid, 16 wid + 16): bit ii of the result =
// row ii, below iend and set in `rows`, suppresses this lane's column (bj, aj).
__device__ __forceinline__ uint64_t tile_rows16(const float4* rbox, const float* rarea, int wid, int iend,
                                                uint64_t rows, float4 bj, float aj, const NmsThr& thr) {
    uint64_t bits = 0;
    if (!thr.never) {
        const int r0 = wid * 16;
#pragma unroll 4
        for (int ii = r0; ii < r0 + 16; ++ii)
            if (ii < iend && ((rows >> ii) & 1ull) && iou_over(rbox[ii], rarea[ii], bj, aj, thr))
                bits |= 1ull << ii;
    }
    return bits;
}

// The four waves' partial words OR-ed through LDS: the column's whole word.  One
// barrier; part[] must stay as it is until the caller's next one.  The callers use
// the word in wave 0 only, where the compiler then keeps the reads.
__device__ __forceinline__ uint64_t tile_word(uint64_t (&part)[4][64], int wid, int lane, uint64_t bits) {
    part[wid][lane] = bits;
    __syncthreads();
    return part[0][lane] | part[1][lane] | part[2][lane] | part[3][lane];
}

// The first `room` set bits of K.
__device__ __forceinline__ uint64_t first_bits(uint64_t K, int room) {
    while (__popcll(K) > room) K &= ~(1ull << (63 - __clzll(K)));
    return K;
}

}  // namespace frcnn
