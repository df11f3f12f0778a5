// The four training losses of train.py:29-57, :81-83, :114-121 -- cross-entropy
// with ignore_index -1 and smooth-L1 over the positive rows -- forward and
// backward, one generic pair of entry points for the RPN and the head stage
// (DESIGN.md "Losses" is the contract).
//
//   forward : losses_fwd_kernel     one thread per row; label reads coalesced, only
//                                   labelled rows touch cls / reg / reg_t; per-workgroup
//                                   fp64 partials to the workspace
//             losses_reduce_kernel  one workgroup sums the partials in workgroup-index
//                                   order and writes loss[2] / stats[4]
//   backward: losses_bwd_kernel     a workgroup owns a tile of rows: softmax terms of its
//                                   labelled rows to LDS (one thread per logit), then
//                                   every element of the tile's dcls and dreg is stored
//                                   once (16-B stores)
//
// No floating-point atomics and no hand-off between workgroups inside a launch:
// the same inputs give the same bits on every call.
//
// float16 / bfloat16 predictions (DESIGN.md §3 "Predictions in 16-bit types"):
// the kernels are templates on the element type E of cls / reg / dcls / dreg.
// A 16-bit element is widened at its load, the fp32 / fp64 arithmetic below is
// the same code, and a gradient is rounded once, at its store.
#include "common.h"
#include "elem16.h"

#include <climits>
#include <cmath>

namespace frcnn {
namespace {

constexpr int kLossMaxC = 128;        // as frcnn_detect
constexpr int kLossThreads = 256;
constexpr int kLossMaxBlocks = 2048;  // forward grid cap (grid-stride beyond it) = partials
constexpr int kBwdXs = 8192;          // floats of softmax terms a backward tile keeps in LDS

struct LossPartial {  // 32 B per forward workgroup
    double cls, reg;
    int32_t n_valid, n_pos, n_skipped, pad;
};

struct LossConsts {   // sigma's constants, computed on the host in double (train.py:39-44)
    float s2;         // sigma^2
    float inv_s2;     // 1 / sigma^2
    float half_s2;    // 0.5 * sigma^2
    float half_inv;   // 0.5 / sigma^2
};

// Correctly rounded fp32 log, the counterpart of exp_cr.
__device__ __forceinline__ float log_cr(float v) { return static_cast<float>(log(static_cast<double>(v))); }

// A row's label: -1 unlabelled, 0..C-1 valid, -2 anything else (skipped and
// counted, never an index).  fp64 labels truncate toward zero (.type(LongTensor)).
template <bool F64>
__device__ __forceinline__ int read_label(const void* labels, int64_t r, int C) {
    int l;
    if (F64) {
        const double v = static_cast<const double*>(labels)[r];
        if (!(v > -2.0 && v < static_cast<double>(C))) return -2;  // NaN, inf, out of range
        l = static_cast<int>(v);
    } else {
        l = static_cast<const int32_t*>(labels)[r];
    }
    return (l >= -1 && l < C) ? l : -2;
}

// Sum of (cls, reg, n_valid, n_pos, n_skipped) over the workgroup, in a fixed
// order; the result is valid in thread 0.
__device__ __forceinline__ void block_sum(double& a, double& b, int& i0, int& i1, int& i2) {
    __shared__ double sd[2][kLossThreads / kWave];
    __shared__ int si[3][kLossThreads / kWave];
    // only lane 0's sums are used: there the butterfly adds the pairs of a shfl_down tree, in its order
    a = wave_reduce(a, op_add{});
    b = wave_reduce(b, op_add{});
    i0 = wave_reduce(i0, op_add{});
    i1 = wave_reduce(i1, op_add{});
    i2 = wave_reduce(i2, op_add{});
    const int w = threadIdx.x / kWave;
    if (lane_id() == 0) {
        sd[0][w] = a, sd[1][w] = b;
        si[0][w] = i0, si[1][w] = i1, si[2][w] = i2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kLossThreads / kWave; ++k) {
            a += sd[0][k], b += sd[1][k];
            i0 += si[0][k], i1 += si[1][k], i2 += si[2][k];
        }
    }
}

// Smooth-L1 term and derivative of one element (train.py:39-44), fp32, every op
// separately rounded as torch's elementwise kernels.
__device__ __forceinline__ float sl1_term(float x, double t64, const LossConsts& k) {
    const float t = static_cast<float>(t64);
    const float d = fabsf(x - t);
    return d < k.inv_s2 ? k.half_s2 * (d * d) : d - k.half_inv;
}

__device__ __forceinline__ float sl1_grad(float x, double t64, const LossConsts& k) {
    const float t = static_cast<float>(t64);
    const float diff = x - t;
    if (fabsf(diff) < k.inv_s2) return k.s2 * diff;
    return diff > 0.0f ? 1.0f : (diff < 0.0f ? -1.0f : diff);  // NaN stays NaN
}

template <bool F64, class E>
__global__ __launch_bounds__(kLossThreads) void losses_fwd_kernel(
    int64_t rows, int C, int P, const typename E::raw* __restrict__ cls, const typename E::raw* __restrict__ reg,
    const double* __restrict__ reg_t, const void* __restrict__ labels, LossConsts k,
    LossPartial* __restrict__ part) {
    double csum = 0.0, rsum = 0.0;
    int nv = 0, np = 0, ns = 0;
    const int64_t step = static_cast<int64_t>(gridDim.x) * kLossThreads;
    for (int64_t r = static_cast<int64_t>(blockIdx.x) * kLossThreads + threadIdx.x; r < rows; r += step) {
        const int l = read_label<F64>(labels, r, C);
        if (l == -2) ++ns;
        if (l < 0) continue;
        ++nv;
        // -log_softmax(x)[l] = log(sum exp(x - m)) - (x_l - m), the sum in ascending class order
        const typename E::raw* x = cls + static_cast<size_t>(r) * C;
        float m = E::widen(x[0]);
        for (int c = 1; c < C; ++c) m = E::widen(x[c]) > m ? E::widen(x[c]) : m;
        float s = exp_cr(E::widen(x[0]) - m);
        for (int c = 1; c < C; ++c) s = s + exp_cr(E::widen(x[c]) - m);
        csum += static_cast<double>(log_cr(s) - (E::widen(x[l]) - m));
        if (l > 0) {
            ++np;
            const typename E::raw* p = reg + static_cast<size_t>(r) * 4 * P + (P == 1 ? 0 : 4 * l);
            const double* t = reg_t + static_cast<size_t>(r) * 4;
            for (int j = 0; j < 4; ++j) rsum += static_cast<double>(sl1_term(E::widen(p[j]), t[j], k));
        }
    }
    block_sum(csum, rsum, nv, np, ns);
    if (threadIdx.x == 0) part[blockIdx.x] = LossPartial{csum, rsum, nv, np, ns, 0};
}

// One workgroup: the partials in workgroup-index order (thread t takes t, t+256,
// ...; then the fixed tree of block_sum).  nparts == 0 (no rows) gives (NaN, 0).
__global__ __launch_bounds__(kLossThreads) void losses_reduce_kernel(const LossPartial* __restrict__ part, int nparts,
                                                                     float* __restrict__ loss,
                                                                     int32_t* __restrict__ stats) {
    double csum = 0.0, rsum = 0.0;
    int nv = 0, np = 0, ns = 0;
    for (int i = threadIdx.x; i < nparts; i += kLossThreads) {
        const LossPartial p = part[i];
        csum += p.cls, rsum += p.reg;
        nv += p.n_valid, np += p.n_pos, ns += p.n_skipped;
    }
    block_sum(csum, rsum, nv, np, ns);
    if (threadIdx.x == 0) {
        loss[0] = static_cast<float>(csum / static_cast<double>(nv));  // 0/0 = NaN, as torch's mean of nothing
        loss[1] = static_cast<float>(rsum / static_cast<double>(np > 1 ? np : 1));
        stats[0] = nv, stats[1] = np, stats[2] = ns, stats[3] = 0;
    }
}

// Rows of a backward tile: a multiple of 4 (so a tile of dcls starts on a 16-B
// boundary for every C), at most one per thread, and their softmax terms (odd
// row stride: no LDS bank conflict between the rows' threads) within kBwdXs.
// Few rows get smaller tiles, down to 4 rows, until about two workgroups per CU
// exist: the exps of a tile are spread over its threads, so the head's 2048
// rows are one exp per thread instead of C in sequence.
// 16-bit gradients: the same rule with a multiple of 8 rows (gran = 8), so a tile
// of dcls (rows * C * 2 B) and of dreg (rows * 4P * 2 B) again starts on a 16-B
// boundary for every C and P, and a 16-B store holds eight elements.
__host__ __device__ inline int bwd_stride(int C) { return C | 1; }
inline int bwd_tile_rows(int64_t rows, int C, int gran = 4) {
    int t = kBwdXs / bwd_stride(C);
    t = (t < kLossThreads ? t : kLossThreads) & ~(gran - 1);
    while (t > gran && (rows + t - 1) / t < 512) t = (t / 2) & ~(gran - 1);
    return t < gran ? gran : t;
}

template <bool F64, bool VEC, class E>
__global__ __launch_bounds__(kLossThreads) void losses_bwd_kernel(
    int64_t rows, int C, int P, const typename E::raw* __restrict__ cls, const typename E::raw* __restrict__ reg,
    const double* __restrict__ reg_t, const void* __restrict__ labels, LossConsts k,
    const int32_t* __restrict__ stats, const float* __restrict__ g_cls, const float* __restrict__ g_reg,
    typename E::raw* __restrict__ dcls, typename E::raw* __restrict__ dreg, int T) {
    __shared__ float xs[kBwdXs];            // exp(x - max) of the tile's labelled rows
    __shared__ float ssum[kLossThreads];    // their maxima, then their sums
    __shared__ int slab[kLossThreads];      // the tile's labels (-1: nothing to write but zeros)
    const int tid = threadIdx.x;
    const int stride = bwd_stride(C);
    const int64_t row0 = static_cast<int64_t>(blockIdx.x) * T;
    const int nrow = static_cast<int>(rows - row0 < T ? rows - row0 : T);
    // NULL upstream gradient = 0: that output is all +0 and its inputs are not read
    const bool do_cls = g_cls != nullptr, do_reg = g_reg != nullptr;
    const int n_pos = stats[1];
    const float scale_c = do_cls ? *g_cls / static_cast<float>(stats[0]) : 0.0f;
    const float scale_r = do_reg ? *g_reg / static_cast<float>(n_pos > 1 ? n_pos : 1) : 0.0f;

    if (tid < nrow) {
        const int l = read_label<F64>(labels, row0 + tid, C);
        slab[tid] = l < 0 ? -1 : l;
    }
    __syncthreads();
    if (do_cls) {
        // exp(x - max) and its ascending-order sum for the labelled rows: one thread per
        // logit for the loads and the fp64-backed exps, one per row for the max and the sum
        const int nc = nrow * C;
        const typename E::raw* x = cls + static_cast<size_t>(row0) * C;
        for (int i = tid; i < nc; i += kLossThreads) {
            const int row = i / C;
            if (slab[row] >= 0) xs[row * stride + i - row * C] = E::widen(x[i]);
        }
        __syncthreads();
        if (tid < nrow && slab[tid] >= 0) {
            const float* v = xs + tid * stride;
            float m = v[0];
            for (int c = 1; c < C; ++c) m = v[c] > m ? v[c] : m;
            ssum[tid] = m;
        }
        __syncthreads();
        for (int i = tid; i < nc; i += kLossThreads) {
            const int row = i / C;
            if (slab[row] >= 0) {
                float* v = xs + row * stride + i - row * C;
                *v = exp_cr(*v - ssum[row]);
            }
        }
        __syncthreads();
        if (tid < nrow && slab[tid] >= 0) {
            const float* v = xs + tid * stride;
            float s = v[0];
            for (int c = 1; c < C; ++c) s = s + v[c];
            ssum[tid] = s;
        }
    }
    __syncthreads();

    // dcls[row, c] = (softmax - onehot) * g_cls / n_valid on labelled rows
    auto dcls_at = [&](int i) -> float {  // i: element of the tile, row-major
        const int row = i / C, c = i - row * C;
        const int l = slab[row];
        if (l < 0 || !do_cls) return 0.0f;
        const float p = xs[row * stride + c] / ssum[row];
        return (p - (c == l ? 1.0f : 0.0f)) * scale_c;
    };
    // dreg[row, 4*col + j] on the label's four columns of positive rows
    const int W = 4 * P;
    auto dreg_at = [&](int row, int col) -> float {
        const int l = slab[row];
        if (l <= 0 || !do_reg || (P != 1 && (col >> 2) != l)) return 0.0f;
        const size_t r = static_cast<size_t>(row0 + row);
        return sl1_grad(E::widen(reg[r * W + col]), reg_t[r * 4 + (col & 3)], k) * scale_r;
    };

    typename E::raw* oc = dcls + static_cast<size_t>(row0) * C;
    typename E::raw* orr = dreg + static_cast<size_t>(row0) * W;
    const int nc = nrow * C, nr = nrow * W;
    if constexpr (sizeof(typename E::raw) == 2) {
        // the one rounding of each gradient; two elements per 32-bit word, low half first
        auto pack2 = [&](float a, float b) -> uint32_t {
            return static_cast<uint32_t>(E::narrow(a)) | (static_cast<uint32_t>(E::narrow(b)) << 16);
        };
        if (VEC) {  // both tiles start 16-B aligned (T % 8 == 0): eight elements per store, the tails single
            for (int q = tid; q < nc / 8; q += kLossThreads) {
                const int i = 8 * q;
                reinterpret_cast<uint4*>(oc)[q] =
                    make_uint4(pack2(dcls_at(i), dcls_at(i + 1)), pack2(dcls_at(i + 2), dcls_at(i + 3)),
                               pack2(dcls_at(i + 4), dcls_at(i + 5)), pack2(dcls_at(i + 6), dcls_at(i + 7)));
            }
            for (int i = (nc & ~7) + tid; i < nc; i += kLossThreads) oc[i] = E::narrow(dcls_at(i));
            for (int q = tid; q < nr / 8; q += kLossThreads) {  // two groups of four columns, each within a row
                const int ra = (2 * q) / P, ca = 4 * (2 * q - ra * P);
                const int rb = (2 * q + 1) / P, cb = 4 * (2 * q + 1 - rb * P);
                reinterpret_cast<uint4*>(orr)[q] =
                    make_uint4(pack2(dreg_at(ra, ca), dreg_at(ra, ca + 1)), pack2(dreg_at(ra, ca + 2), dreg_at(ra, ca + 3)),
                               pack2(dreg_at(rb, cb), dreg_at(rb, cb + 1)), pack2(dreg_at(rb, cb + 2), dreg_at(rb, cb + 3)));
            }
            for (int i = (nr & ~7) + tid; i < nr; i += kLossThreads) {
                const int row = i / W;
                orr[i] = E::narrow(dreg_at(row, i - row * W));
            }
        } else {
            for (int i = tid; i < nc; i += kLossThreads) oc[i] = E::narrow(dcls_at(i));
            for (int i = tid; i < nr; i += kLossThreads) {
                const int row = i / W;
                orr[i] = E::narrow(dreg_at(row, i - row * W));
            }
        }
    } else if (VEC) {  // both tiles start 16-B aligned (T % 4 == 0); nr % 4 == 0, nc's tail is scalar
        for (int q = tid; q < nc / 4; q += kLossThreads)
            reinterpret_cast<float4*>(oc)[q] =
                make_float4(dcls_at(4 * q), dcls_at(4 * q + 1), dcls_at(4 * q + 2), dcls_at(4 * q + 3));
        for (int i = (nc & ~3) + tid; i < nc; i += kLossThreads) oc[i] = dcls_at(i);
        for (int q = tid; q < nr / 4; q += kLossThreads) {
            const int row = q / P, col = 4 * (q - row * P);
            reinterpret_cast<float4*>(orr)[q] =
                make_float4(dreg_at(row, col), dreg_at(row, col + 1), dreg_at(row, col + 2), dreg_at(row, col + 3));
        }
    } else {
        for (int i = tid; i < nc; i += kLossThreads) oc[i] = dcls_at(i);
        for (int i = tid; i < nr; i += kLossThreads) {
            const int row = i / W;
            orr[i] = dreg_at(row, i - row * W);
        }
    }
}

int fwd_blocks(int64_t rows) {
    const int64_t b = (rows + kLossThreads - 1) / kLossThreads;
    return static_cast<int>(b < kLossMaxBlocks ? b : kLossMaxBlocks);
}

// The argument rules of both entry points, checked before any HIP call.
int check_stage(const char* fn, int64_t rows, int C, int P, double sigma, LossConsts* k) {
    FRCNN_REQUIRE(C >= 2 && C <= kLossMaxC, "%s: C=%d must be in [2, %d]", fn, C, kLossMaxC);
    FRCNN_REQUIRE(rows >= 0 && rows <= INT_MAX, "%s: rows=%lld must be in [0, 2^31)", fn, static_cast<long long>(rows));
    FRCNN_REQUIRE(P == 1 || P == C, "%s: P=%d must be 1 (one box per row) or C=%d (one per class)", fn, P, C);
    FRCNN_REQUIRE(std::isfinite(sigma) && sigma > 0.0, "%s: sigma=%g must be positive and finite", fn, sigma);
    const double s2 = sigma * sigma;
    *k = LossConsts{static_cast<float>(s2), static_cast<float>(1.0 / s2), static_cast<float>(0.5 * s2),
                    static_cast<float>(0.5 / s2)};
    return FRCNN_OK;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <class E>
int losses_fwd_impl(const char* fn, int64_t rows, int C, int P, const void* cls_v, const void* reg_v,
                    const double* reg_t, const void* labels, int labels_f64, double sigma, float* loss,
                    int32_t* stats, void* workspace, size_t ws_bytes, void* stream) {
    using R = typename E::raw;
    const R* cls = static_cast<const R*>(cls_v);
    const R* reg = static_cast<const R*>(reg_v);
    LossConsts k;
    if (int rc = check_stage(fn, rows, C, P, sigma, &k)) return rc;
    FRCNN_REQUIRE(loss && stats, "%s: null output (loss / stats)", fn);
    FRCNN_REQUIRE(rows == 0 || (cls && reg && reg_t && labels), "%s: null input (cls / reg / reg_t / labels)", fn);
    FRCNN_REQUIRE(aligned_to(cls, sizeof(R)) && aligned_to(reg, sizeof(R)),
                  "%s: cls / reg not aligned to their element type", fn);
    const size_t need = frcnn_losses_workspace_size(rows, C);
    if (need > 0 && (!workspace || ws_bytes < need)) {
        set_error("%s: workspace of %zu B < %zu B", fn, workspace ? ws_bytes : size_t{0}, need);
        return FRCNN_EWORKSPACE;
    }
    hipStream_t st = as_stream(stream);
    LossPartial* part = static_cast<LossPartial*>(workspace);
    const int nb = fwd_blocks(rows);
    if (nb > 0) {
        if (labels_f64)
            losses_fwd_kernel<true, E><<<nb, kLossThreads, 0, st>>>(rows, C, P, cls, reg, reg_t, labels, k, part);
        else
            losses_fwd_kernel<false, E><<<nb, kLossThreads, 0, st>>>(rows, C, P, cls, reg, reg_t, labels, k, part);
        FRCNN_LAUNCH_CHECK("losses_fwd_kernel");
    }
    losses_reduce_kernel<<<1, kLossThreads, 0, st>>>(part, nb, loss, stats);
    FRCNN_LAUNCH_CHECK("losses_reduce_kernel");
    return FRCNN_OK;
}

template <class E>
int losses_bwd_impl(const char* fn, int64_t rows, int C, int P, const void* cls_v, const void* reg_v,
                    const double* reg_t, const void* labels, int labels_f64, double sigma, const int32_t* stats,
                    const float* g_cls, const float* g_reg, void* dcls_v, void* dreg_v, void* stream) {
    using R = typename E::raw;
    const R* cls = static_cast<const R*>(cls_v);
    const R* reg = static_cast<const R*>(reg_v);
    R* dcls = static_cast<R*>(dcls_v);
    R* dreg = static_cast<R*>(dreg_v);
    LossConsts k;
    if (int rc = check_stage(fn, rows, C, P, sigma, &k)) return rc;
    if (rows == 0) return FRCNN_OK;  // no output elements
    FRCNN_REQUIRE(cls && reg && reg_t && labels && stats, "%s: null input (cls / reg / reg_t / labels / stats)", fn);
    FRCNN_REQUIRE(dcls && dreg, "%s: null output (dcls / dreg)", fn);
    FRCNN_REQUIRE(aligned_to(cls, sizeof(R)) && aligned_to(reg, sizeof(R)) && aligned_to(dcls, sizeof(R)) &&
                      aligned_to(dreg, sizeof(R)),
                  "%s: cls / reg / dcls / dreg not aligned to their element type", fn);
    hipStream_t st = as_stream(stream);
    const int T = bwd_tile_rows(rows, C, sizeof(R) == 2 ? 8 : 4);
    const int nb = static_cast<int>((rows + T - 1) / T);
    const bool vec = aligned16(dcls) && aligned16(dreg);
#define FRCNN_LOSSES_BWD(F64, VEC)                                                                               \
    losses_bwd_kernel<F64, VEC, E><<<nb, kLossThreads, 0, st>>>(rows, C, P, cls, reg, reg_t, labels, k, stats, \
                                                                g_cls, g_reg, dcls, dreg, T)
    if (labels_f64) {
        if (vec) FRCNN_LOSSES_BWD(true, true); else FRCNN_LOSSES_BWD(true, false);
    } else {
        if (vec) FRCNN_LOSSES_BWD(false, true); else FRCNN_LOSSES_BWD(false, false);
    }
#undef FRCNN_LOSSES_BWD
    FRCNN_LAUNCH_CHECK("losses_bwd_kernel");
    return FRCNN_OK;
}

}  // namespace
}  // namespace frcnn

using namespace frcnn;

extern "C" size_t frcnn_losses_workspace_size(int64_t rows, int C) {
    if (C < 2 || C > kLossMaxC || rows < 0 || rows > INT_MAX) return 0;
    return align_up(static_cast<size_t>(fwd_blocks(rows)) * sizeof(LossPartial), 256);
}

extern "C" int frcnn_losses_fwd(int64_t rows, int C, int P, const float* cls, const float* reg, const double* reg_t,
                                const void* labels, int labels_f64, double sigma, float* loss, int32_t* stats,
                                void* workspace, size_t ws_bytes, void* stream) {
    return losses_fwd_impl<ElemF32>("frcnn_losses_fwd", rows, C, P, cls, reg, reg_t, labels, labels_f64, sigma, loss,
                                    stats, workspace, ws_bytes, stream);
}

extern "C" int frcnn_losses_bwd(int64_t rows, int C, int P, const float* cls, const float* reg, const double* reg_t,
                                const void* labels, int labels_f64, double sigma, const int32_t* stats,
                                const float* g_cls, const float* g_reg, float* dcls, float* dreg, void* stream) {
    return losses_bwd_impl<ElemF32>("frcnn_losses_bwd", rows, C, P, cls, reg, reg_t, labels, labels_f64, sigma, stats,
                                    g_cls, g_reg, dcls, dreg, stream);
}

extern "C" int frcnn_losses_fwd_t(int dtype, int64_t rows, int C, int P, const void* cls, const void* reg,
                                  const double* reg_t, const void* labels, int labels_f64, double sigma, float* loss,
                                  int32_t* stats, void* workspace, size_t ws_bytes, void* stream) {
    FRCNN_REQUIRE(dtype_code_ok(dtype), "frcnn_losses_fwd_t: dtype code %d is not FRCNN_F32, FRCNN_F16 or FRCNN_BF16",
                  dtype);
    if (dtype == FRCNN_F32)
        return frcnn_losses_fwd(rows, C, P, static_cast<const float*>(cls), static_cast<const float*>(reg), reg_t,
                                labels, labels_f64, sigma, loss, stats, workspace, ws_bytes, stream);
    if (dtype == FRCNN_F16)
        return losses_fwd_impl<ElemF16>("frcnn_losses_fwd_t", rows, C, P, cls, reg, reg_t, labels, labels_f64, sigma,
                                        loss, stats, workspace, ws_bytes, stream);
    return losses_fwd_impl<ElemBF16>("frcnn_losses_fwd_t", rows, C, P, cls, reg, reg_t, labels, labels_f64, sigma,
                                     loss, stats, workspace, ws_bytes, stream);
}

extern "C" int frcnn_losses_bwd_t(int dtype, int64_t rows, int C, int P, const void* cls, const void* reg,
                                  const double* reg_t, const void* labels, int labels_f64, double sigma,
                                  const int32_t* stats, const float* g_cls, const float* g_reg, void* dcls, void* dreg,
                                  void* stream) {
    FRCNN_REQUIRE(dtype_code_ok(dtype), "frcnn_losses_bwd_t: dtype code %d is not FRCNN_F32, FRCNN_F16 or FRCNN_BF16",
                  dtype);
    if (dtype == FRCNN_F32)
        return frcnn_losses_bwd(rows, C, P, static_cast<const float*>(cls), static_cast<const float*>(reg), reg_t,
                                labels, labels_f64, sigma, stats, g_cls, g_reg, static_cast<float*>(dcls),
                                static_cast<float*>(dreg), stream);
    if (dtype == FRCNN_F16)
        return losses_bwd_impl<ElemF16>("frcnn_losses_bwd_t", rows, C, P, cls, reg, reg_t, labels, labels_f64, sigma,
                                        stats, g_cls, g_reg, dcls, dreg, stream);
    return losses_bwd_impl<ElemBF16>("frcnn_losses_bwd_t", rows, C, P, cls, reg, reg_t, labels, labels_f64, sigma,
                                     stats, g_cls, g_reg, dcls, dreg, stream);
}
