// RPN head epilogue (nets/rpn.py:117-124), SURVEY.md §8(f) row 1.
//
// The reference turns the two 1x1-conv outputs (NCHW) into the proposal
// layer's inputs with four separate passes: cls.permute(0,2,3,1).contiguous(),
// F.softmax(dim=-1), [:, :, 1].contiguous() and reg.permute(0,2,3,1).contiguous().
// Here ONE launch reads each conv output once and writes all three tensors:
//   cls_nhwc [N, A, 2]  (= the reference's cls before its final view-permute)
//   fg       [N, A]     (softmax of channel pair (2k, 2k+1), element 1)
//   reg_nhwc [N, A, 4]  (the proposal layer's deltas, and the loss's reg)
// with A = H*W*K and row (y*W + x)*K + k.
//
// HBM-bound transpose: a workgroup owns a 64-pixel strip of one image.  Reads
// are channel-major (64 consecutive pixels of one channel = one 256 B run per
// wave), staged through LDS, and the NHWC outputs are written as contiguous
// runs (the strip's rows of every output tensor are adjacent in memory), so
// both sides are fully coalesced.  Algorithmic bytes per image:
// 6K*H*W*4 read + 7K*H*W*4 written.
//
// float16 / bfloat16 conv outputs (rpn_head_epilogue_kernel_h, DESIGN.md §3
// "Predictions in 16-bit types"): the strip is staged in LDS as raw 16-bit
// values, cls_nhwc / reg_nhwc are copies of those bits in the input's type, and
// the values are widened only for the softmax (fg, fp32) and for a fourth
// output, deltas fp32 [N, A, 4], which is what the proposal layer reads.
// Algorithmic bytes per image: 6K*H*W*2 read + (6*2 + 5*4)K*H*W written.
#include "common.h"
#include "elem16.h"

namespace frcnn {

constexpr int kEpiPix = 64;      // pixels per workgroup strip
constexpr int kEpiThreads = 256;

// torch CPU softmax over a last dim of 2 (ATen _vec_softmax_lastdim): m = max,
// e_i = exp(x_i - m), s = e_0 + e_1, out_i = e_i * (1 / s).  Every op is fp32
// and separately rounded (library built with -ffp-contract=off); exp is the
// correctly rounded one (torch's vectorised exp is host-dependent in its last
// bits, like the decode's).
__device__ __forceinline__ float fg_softmax(float a, float b) {
    float m = fmaxf(a, b);
    float ea = exp_cr(a - m);
    float eb = exp_cr(b - m);
    float inv = 1.0f / (ea + eb);
    return eb * inv;
}

__global__ __launch_bounds__(kEpiThreads) void rpn_head_epilogue_kernel(
    const float* __restrict__ cls, const float* __restrict__ reg, int K, int HW,
    float* __restrict__ cls_nhwc, float* __restrict__ fg, float* __restrict__ reg_nhwc) {
    extern __shared__ float epi_lds[];
    const int n = blockIdx.y;
    const int p0 = blockIdx.x * kEpiPix;
    const int cnt = min(kEpiPix, HW - p0);
    const int C2 = 2 * K, C4 = 4 * K;
    float* lc = epi_lds;                 // [kEpiPix][2K]
    float* lr = epi_lds + kEpiPix * C2;  // [kEpiPix][4K]
    const float* cn = cls + static_cast<int64_t>(n) * C2 * HW + p0;
    const float* rn = reg + static_cast<int64_t>(n) * C4 * HW + p0;

    for (int i = threadIdx.x; i < kEpiPix * C2; i += kEpiThreads) {
        int c = i / kEpiPix, p = i % kEpiPix;
        if (p < cnt) lc[p * C2 + c] = cn[static_cast<int64_t>(c) * HW + p];
    }
    for (int i = threadIdx.x; i < kEpiPix * C4; i += kEpiThreads) {
        int c = i / kEpiPix, p = i % kEpiPix;
        if (p < cnt) lr[p * C4 + c] = rn[static_cast<int64_t>(c) * HW + p];
    }
    __syncthreads();

    const int64_t row0 = static_cast<int64_t>(n) * HW + p0;  // first pixel of the strip
    float* oc = cls_nhwc + row0 * C2;
    for (int i = threadIdx.x; i < cnt * C2; i += kEpiThreads) oc[i] = lc[i];
    float* of = fg + row0 * K;
    for (int i = threadIdx.x; i < cnt * K; i += kEpiThreads) {
        int p = i / K, k = i - p * K;
        of[i] = fg_softmax(lc[p * C2 + 2 * k], lc[p * C2 + 2 * k + 1]);
    }
    float* orr = reg_nhwc + row0 * C4;
    for (int i = threadIdx.x; i < cnt * C4; i += kEpiThreads) orr[i] = lr[i];
}

// n 16-bit values from LDS (4-byte aligned) to global memory that is only known
// to be 2-byte aligned: single elements up to the first 16-byte boundary, 16-byte
// stores (eight elements) from there, single elements for the rest.
__device__ __forceinline__ void copy_out16(uint16_t* __restrict__ dst, const uint16_t* src, int n, int tid) {
    const int mis = static_cast<int>((reinterpret_cast<uintptr_t>(dst) & 15) >> 1);
    int head = mis ? 8 - mis : 0;
    head = head < n ? head : n;
    const int nq = (n - head) >> 3;
    if (tid < head) dst[tid] = src[tid];
    uint4* d4 = reinterpret_cast<uint4*>(dst + head);
    if ((head & 1) == 0) {  // the source stays 4-byte aligned: four 32-bit LDS reads
        const uint32_t* s32 = reinterpret_cast<const uint32_t*>(src + head);
        for (int q = tid; q < nq; q += kEpiThreads)
            d4[q] = make_uint4(s32[4 * q], s32[4 * q + 1], s32[4 * q + 2], s32[4 * q + 3]);
    } else {
        const uint16_t* s = src + head;
        for (int q = tid; q < nq; q += kEpiThreads) {
            const uint16_t* e = s + 8 * q;
            d4[q] = make_uint4(e[0] | (static_cast<uint32_t>(e[1]) << 16), e[2] | (static_cast<uint32_t>(e[3]) << 16),
                               e[4] | (static_cast<uint32_t>(e[5]) << 16), e[6] | (static_cast<uint32_t>(e[7]) << 16));
        }
    }
    for (int i = head + 8 * nq + tid; i < n; i += kEpiThreads) dst[i] = src[i];
}

// The 16-bit sibling: E is ElemF16 or ElemBF16, PIX the strip's pixels.  PAIR: H*W
// is even and cls / reg are 4-byte aligned, so every channel row of a strip starts
// on a 4-byte boundary and is read two pixels at a time; otherwise (odd H*W: a
// channel plane starts only 2-byte aligned) the reads are 2-byte loads.  DVEC:
// deltas is 16-byte aligned (a strip's rows then are too): one float4 per anchor.
template <class E, int PIX, bool PAIR, bool DVEC>
__global__ __launch_bounds__(kEpiThreads) void rpn_head_epilogue_kernel_h(
    const uint16_t* __restrict__ cls, const uint16_t* __restrict__ reg, int K, int HW,
    uint16_t* __restrict__ cls_nhwc, float* __restrict__ fg, uint16_t* __restrict__ reg_nhwc,
    float* __restrict__ deltas) {
    extern __shared__ __align__(16) uint16_t epi_lds16[];
    const int n = blockIdx.y;
    const int p0 = blockIdx.x * PIX;
    const int cnt = min(PIX, HW - p0);
    const int C2 = 2 * K, C4 = 4 * K;
    uint16_t* lc = epi_lds16;             // [PIX][2K]
    uint16_t* lr = epi_lds16 + PIX * C2;  // [PIX][4K]  (8-byte aligned: PIX * 2K * 2 B)
    const uint16_t* cn = cls + static_cast<int64_t>(n) * C2 * HW + p0;
    const uint16_t* rn = reg + static_cast<int64_t>(n) * C4 * HW + p0;

    if (PAIR) {  // cnt is even: H*W and p0 are
        constexpr int HP = PIX / 2;
        for (int i = threadIdx.x; i < HP * C2; i += kEpiThreads) {
            const int c = i / HP, p = 2 * (i % HP);
            if (p < cnt) {
                const uint32_t v = *reinterpret_cast<const uint32_t*>(cn + static_cast<int64_t>(c) * HW + p);
                lc[p * C2 + c] = static_cast<uint16_t>(v);
                lc[(p + 1) * C2 + c] = static_cast<uint16_t>(v >> 16);
            }
        }
        for (int i = threadIdx.x; i < HP * C4; i += kEpiThreads) {
            const int c = i / HP, p = 2 * (i % HP);
            if (p < cnt) {
                const uint32_t v = *reinterpret_cast<const uint32_t*>(rn + static_cast<int64_t>(c) * HW + p);
                lr[p * C4 + c] = static_cast<uint16_t>(v);
                lr[(p + 1) * C4 + c] = static_cast<uint16_t>(v >> 16);
            }
        }
    } else {
        for (int i = threadIdx.x; i < PIX * C2; i += kEpiThreads) {
            const int c = i / PIX, p = i % PIX;
            if (p < cnt) lc[p * C2 + c] = cn[static_cast<int64_t>(c) * HW + p];
        }
        for (int i = threadIdx.x; i < PIX * C4; i += kEpiThreads) {
            const int c = i / PIX, p = i % PIX;
            if (p < cnt) lr[p * C4 + c] = rn[static_cast<int64_t>(c) * HW + p];
        }
    }
    __syncthreads();

    const int64_t row0 = static_cast<int64_t>(n) * HW + p0;  // first pixel of the strip
    copy_out16(cls_nhwc + row0 * C2, lc, cnt * C2, threadIdx.x);
    copy_out16(reg_nhwc + row0 * C4, lr, cnt * C4, threadIdx.x);
    float* of = fg + row0 * K;
    const uint32_t* pairs = reinterpret_cast<const uint32_t*>(lc);  // anchor i of the strip: (bg, fg) logits
    for (int i = threadIdx.x; i < cnt * K; i += kEpiThreads) {
        const uint32_t v = pairs[i];
        of[i] = fg_softmax(E::widen(static_cast<uint16_t>(v)), E::widen(static_cast<uint16_t>(v >> 16)));
    }
    float* od = deltas + row0 * C4;
    if (DVEC) {
        const uint2* quads = reinterpret_cast<const uint2*>(lr);
        for (int i = threadIdx.x; i < cnt * K; i += kEpiThreads) {
            const uint2 v = quads[i];
            reinterpret_cast<float4*>(od)[i] =
                make_float4(E::widen(static_cast<uint16_t>(v.x)), E::widen(static_cast<uint16_t>(v.x >> 16)),
                            E::widen(static_cast<uint16_t>(v.y)), E::widen(static_cast<uint16_t>(v.y >> 16)));
        }
    } else {
        for (int i = threadIdx.x; i < cnt * C4; i += kEpiThreads) od[i] = E::widen(lr[i]);
    }
}

template <class E, int PIX>
void launch_epilogue_h(const void* cls, const void* reg, int N, int K, int HW, void* cls_nhwc, float* fg,
                       void* reg_nhwc, float* deltas, hipStream_t st) {
    const size_t lds = static_cast<size_t>(PIX) * 6 * K * sizeof(uint16_t);  // <= 48 KB
    const dim3 grid(static_cast<unsigned>((HW + PIX - 1) / PIX), static_cast<unsigned>(N));
    const bool pair = HW % 2 == 0 && aligned_to(cls, 4) && aligned_to(reg, 4);
    const bool dvec = aligned_to(deltas, 16);
#define FRCNN_EPI_H(PAIR, DVEC)                                                                          \
    hipLaunchKernelGGL((rpn_head_epilogue_kernel_h<E, PIX, PAIR, DVEC>), grid, dim3(kEpiThreads), lds, st, \
                       static_cast<const uint16_t*>(cls), static_cast<const uint16_t*>(reg), K, HW,      \
                       static_cast<uint16_t*>(cls_nhwc), fg, static_cast<uint16_t*>(reg_nhwc), deltas)
    if (pair) {
        if (dvec) FRCNN_EPI_H(true, true); else FRCNN_EPI_H(true, false);
    } else {
        if (dvec) FRCNN_EPI_H(false, true); else FRCNN_EPI_H(false, false);
    }
#undef FRCNN_EPI_H
}

}  // namespace frcnn

using namespace frcnn;

extern "C" int frcnn_rpn_head_epilogue(const float* cls, const float* reg, int N, int K,
                                       int feat_h, int feat_w, float* cls_nhwc, float* fg,
                                       float* reg_nhwc, void* stream) {
    FRCNN_REQUIRE(N >= 0 && K > 0 && K <= 32 && feat_h >= 0 && feat_w >= 0,
                  "frcnn_rpn_head_epilogue: bad shape (need N >= 0, 1 <= K <= 32)");
    const int64_t hw = static_cast<int64_t>(feat_h) * feat_w;
    if (N == 0 || hw == 0) return FRCNN_OK;
    FRCNN_REQUIRE(hw <= (int64_t(1) << 30) && N <= 65535, "frcnn_rpn_head_epilogue: too large");
    FRCNN_REQUIRE(cls && reg && cls_nhwc && fg && reg_nhwc, "frcnn_rpn_head_epilogue: null pointer");
    const int HW = static_cast<int>(hw);
    const size_t lds = static_cast<size_t>(kEpiPix) * 6 * K * sizeof(float);  // <= 48 KB
    dim3 grid(static_cast<unsigned>((HW + kEpiPix - 1) / kEpiPix), static_cast<unsigned>(N));
    hipLaunchKernelGGL(rpn_head_epilogue_kernel, grid, dim3(kEpiThreads), lds, as_stream(stream),
                       cls, reg, K, HW, cls_nhwc, fg, reg_nhwc);
    FRCNN_LAUNCH_CHECK("rpn_head_epilogue_kernel");
    return FRCNN_OK;
}

extern "C" int frcnn_rpn_head_epilogue_t(int dtype, const void* cls, const void* reg, int N, int K, int feat_h,
                                         int feat_w, void* cls_nhwc, float* fg, void* reg_nhwc, float* deltas,
                                         void* stream) {
    FRCNN_REQUIRE(dtype_code_ok(dtype),
                  "frcnn_rpn_head_epilogue_t: dtype code %d is not FRCNN_F32, FRCNN_F16 or FRCNN_BF16", dtype);
    if (dtype == FRCNN_F32)  // the untyped function as it is; deltas is reg_nhwc there and is not written
        return frcnn_rpn_head_epilogue(static_cast<const float*>(cls), static_cast<const float*>(reg), N, K, feat_h,
                                       feat_w, static_cast<float*>(cls_nhwc), fg, static_cast<float*>(reg_nhwc),
                                       stream);
    FRCNN_REQUIRE(N >= 0 && K > 0 && K <= 32 && feat_h >= 0 && feat_w >= 0,
                  "frcnn_rpn_head_epilogue_t: bad shape (need N >= 0, 1 <= K <= 32)");
    const int64_t hw = static_cast<int64_t>(feat_h) * feat_w;
    if (N == 0 || hw == 0) return FRCNN_OK;
    FRCNN_REQUIRE(hw <= (int64_t(1) << 30) && N <= 65535, "frcnn_rpn_head_epilogue_t: too large");
    FRCNN_REQUIRE(cls && reg && cls_nhwc && fg && reg_nhwc && deltas, "frcnn_rpn_head_epilogue_t: null pointer");
    FRCNN_REQUIRE(aligned_to(cls, 2) && aligned_to(reg, 2) && aligned_to(cls_nhwc, 2) && aligned_to(reg_nhwc, 2) &&
                      aligned_to(fg, 4) && aligned_to(deltas, 4),
                  "frcnn_rpn_head_epilogue_t: a pointer is not aligned to its element type");
    const int HW = static_cast<int>(hw);
    hipStream_t st = as_stream(stream);
    // 64-pixel strips unless overridden (frcnn_set_path "rpn_epilogue_strip"; profiles/autocast_ops_bench.json)
    const bool wide = path_cfg().epi_strip == 128;
    if (dtype == FRCNN_F16) {
        if (wide) launch_epilogue_h<ElemF16, 128>(cls, reg, N, K, HW, cls_nhwc, fg, reg_nhwc, deltas, st);
        else launch_epilogue_h<ElemF16, kEpiPix>(cls, reg, N, K, HW, cls_nhwc, fg, reg_nhwc, deltas, st);
    } else {
        if (wide) launch_epilogue_h<ElemBF16, 128>(cls, reg, N, K, HW, cls_nhwc, fg, reg_nhwc, deltas, st);
        else launch_epilogue_h<ElemBF16, kEpiPix>(cls, reg, N, K, HW, cls_nhwc, fg, reg_nhwc, deltas, st);
    }
    FRCNN_LAUNCH_CHECK("rpn_head_epilogue_kernel_h");
    return FRCNN_OK;
}
