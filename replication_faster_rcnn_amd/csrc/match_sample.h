// Device pieces shared by the two training-target units, rpn_targets.hip (anchors against gt
// boxes) and box_head.hip (proposals against gt boxes): torchvision's box_iou of one pair, the
// presence rule of a gt row, the Philox4x32-10 sampling key and the correctly rounded fp32 log.
// One definition, so the two ops cannot drift apart in a rounding or a tie.
#pragma once

#include "common.h"

namespace frcnn {

// Correctly rounded fp32 log and log1p, the counterparts of exp_cr.
__device__ __forceinline__ float rt_log_cr(float v) { return static_cast<float>(log(static_cast<double>(v))); }
__device__ __forceinline__ float rt_log1p_cr(float v) { return static_cast<float>(log1p(static_cast<double>(v))); }

// Word 0 of Philox4x32-10 with counter (c0, c1, c2, c3) and key (k0, k1).
__device__ __forceinline__ uint32_t philox_word0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                 uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = static_cast<uint64_t>(0xD2511F53u) * c0;
        const uint64_t p1 = static_cast<uint64_t>(0xCD9E8D57u) * c2;
        const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n2 = static_cast<uint32_t>(p0 >> 32) ^ c3 ^ k1;
        c1 = static_cast<uint32_t>(p1);
        c3 = static_cast<uint32_t>(p0);
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

// The sampling key of candidate a (an anchor, a proposal) of image n, its low bits masked away.
struct RtKeyer {
    uint32_t c2, c3, k0, k1, mask;
    __device__ RtKeyer(const int64_t* rng, int key_bits) {
        const uint64_t seed = static_cast<uint64_t>(rng[0]), calls = static_cast<uint64_t>(rng[1]);
        k0 = static_cast<uint32_t>(seed);
        k1 = static_cast<uint32_t>(seed >> 32);
        c2 = static_cast<uint32_t>(calls);
        c3 = static_cast<uint32_t>(calls >> 32);
        mask = key_bits <= 0 ? 0u : key_bits >= 32 ? ~0u : ~(~0u >> key_bits);
    }
    __device__ __forceinline__ uint32_t operator()(unsigned a, unsigned n) const {
        return philox_word0(a, n, c2, c3, k0, k1) & mask;
    }
};

__device__ __forceinline__ bool rt_finite(float v) { return fabsf(v) <= 3.402823466e38f; }

// The image's gt rows to LDS: sarea[g] is the area of a present row, -1 of an absent one
// (past the clamped count, not finite, or x2 <= x1 or y2 <= y1).  Returns the clamped count;
// the caller puts a barrier behind it.
__device__ __forceinline__ int rt_load_gts(const float4* __restrict__ gt, const int32_t* __restrict__ gt_count, int n,
                                           int G, float4* sbox, float* sarea) {
    int cnt = gt_count[n];
    cnt = cnt < 0 ? 0 : cnt > G ? G : cnt;
    for (int t = threadIdx.x; t < G; t += blockDim.x) {
        float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
        bool ok = false;
        if (t < cnt) {
            b = gt[static_cast<size_t>(n) * G + t];
            ok = rt_finite(b.x) && rt_finite(b.y) && rt_finite(b.z) && rt_finite(b.w) && b.z > b.x && b.w > b.y;
        }
        sbox[t] = b;
        sarea[t] = ok ? (b.z - b.x) * (b.w - b.y) : -1.0f;
    }
    return cnt;
}

// torchvision's box_iou of one (gt, candidate) pair, fp32, every operation rounded separately.
// No intersection gives 0 without the divide (the quotient would be +-0 or NaN), and a NaN
// quotient (areas beyond fp32, a NaN coordinate) is 0 too: no IoU is ever NaN or negative.
__device__ __forceinline__ float rt_iou(const float4& gb, float garea, const float4& ab, float aarea) {
    float iw = fminf(gb.z, ab.z) - fmaxf(gb.x, ab.x);
    float ih = fminf(gb.w, ab.w) - fmaxf(gb.y, ab.y);
    iw = iw > 0.0f ? iw : 0.0f;
    ih = ih > 0.0f ? ih : 0.0f;
    const float inter = iw * ih;
    if (!(inter > 0.0f)) return 0.0f;
    const float iou = inter / ((garea + aarea) - inter);
    return iou == iou ? iou : 0.0f;
}

}  // namespace frcnn
