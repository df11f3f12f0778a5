// Batched image preprocessing (utils/data_loader.py:38,61-75): uint8 HWC images of
// differing sizes -> resized, normalised fp32 [N,3,out_h,out_w], and the boxes'
// rescale that goes with it (DESIGN.md §3 "Preprocessing" is the contract).
//
//   preprocess_kernel     one workgroup per (image, tile of TH x 64 outputs), one launch:
//                         1. the tile's tap tables: per output row / column the first source
//                            index and the T = 2 + 2r weights of bilinear x Gaussian, formed in
//                            fp64 from the exact integer position and rounded to fp32 once
//                         2. the tile's source footprint, mirror-folded, as bytes to LDS
//                         3. the horizontal pass to an fp32 LDS image [row][channel][64]
//                         4. the vertical pass, normalise, 256-B stores along out_w
//                         An upscaled axis has r = 0: two taps, no exp, no Gaussian work.
//   rescale_boxes_kernel  one thread per coordinate, fp64
//
// Every output element is stored once by the one thread that owns it, each sum
// runs over its taps in ascending order, and neither depends on the tile size
// or on the other images of the batch: the same image gives the same bits in
// any batch and on every call.
#include "common.h"

#include <algorithm>
#include <climits>
#include <cmath>

namespace frcnn {
namespace {

constexpr int kPrepThreads = 256;
constexpr int kPrepTW = 64;          // tile width = one wave's lanes
// Tile heights tried: 32, 16, ..., 1 (the first that fits).  At cfg2's batch a largest height of
// 32 / 16 / 8 ran 15.5 / 17.2 / 22.6 us.
constexpr int kPrepMaxTH = 32;
constexpr int kPrepMaxRatio = 5;     // in <= 5 * out per axis
constexpr int kPrepMaxRadius = 8;    // int(4 * 2.0 + 0.5) at ratio 5
constexpr int kPrepGauss = 16;       // fp64 Gaussian weights kept per axis (>= radius + 1)
static_assert(kPrepMaxRadius < kPrepGauss, "the Gaussian's weights 0..radius fit their LDS array");
constexpr int kPrepTapRows = kPrepMaxTH + kPrepTW;
constexpr size_t kPrepLdsBudget = 64 * 1024;

struct PrepConsts {
    float scale[3];  // 1 / (255 * std)
    float bias[3];   // -mean / std
};

// Anti-aliasing radius of an axis and its sigma^2 (0 when n_in <= n_out).
__host__ __device__ inline int axis_radius(int n_in, int n_out, double* s2) {
    double s = (static_cast<double>(n_in) / static_cast<double>(n_out) - 1.0) / 2.0;
    if (!(s > 0.0)) s = 0.0;
    *s2 = s * s;
    return static_cast<int>(4.0 * s + 0.5);
}

// Source rows (columns) that L consecutive outputs of an axis can reach when
// its input is at most max_in: floor(pos(d0 + L - 1)) - floor(pos(d0)) <=
// ceil((L - 1) * in / out), plus the two bilinear taps and the radius each side.
inline int span_bound(int L, int max_in, int n_out) {
    const int64_t m = max_in < kPrepMaxRatio * n_out ? max_in : kPrepMaxRatio * n_out;
    double s2;
    const int r = axis_radius(static_cast<int>(m), n_out, &s2);
    return static_cast<int>(((L - 1) * m + n_out - 1) / n_out) + 2 + 2 * r;
}

struct PrepLds {  // byte offsets into the dynamic LDS of a workgroup
    size_t tmp, tapw, taps, src, total;
    int ts;  // floats per tap row: the most taps the host bounds allow, plus one (odd: the
             // lanes' rows fall on distinct LDS banks)
};

// gauss fp64 [2][kPrepGauss] first (8-byte aligned at offset 0), then the fp32 pass image,
// the tap weights and starts, the source bytes last.
inline PrepLds prep_lds(int rows, int cols, int max_taps) {
    PrepLds l;
    l.ts = max_taps + 1;
    l.tmp = 2 * kPrepGauss * sizeof(double);
    l.tapw = l.tmp + static_cast<size_t>(rows) * 3 * kPrepTW * sizeof(float);
    l.taps = l.tapw + static_cast<size_t>(kPrepTapRows) * l.ts * sizeof(float);
    l.src = l.taps + static_cast<size_t>(kPrepTapRows) * sizeof(int32_t);
    l.total = align_up(l.src + static_cast<size_t>(rows) * cols * 3, 16);
    return l;
}

// Mirror without edge repeat: period 2(n-1), -1 -> 1, n -> n-2, n == 1 -> 0.
__device__ __forceinline__ int fold_mirror(int i, int n) {
    if (static_cast<unsigned>(i) < static_cast<unsigned>(n)) return i;
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - m;
}

// FAST: both axes have two taps (no axis is downscaled).
template <bool FAST>
__device__ __forceinline__ void prep_tile(const uint8_t* __restrict__ img, int h, int w, int n, int out_h, int out_w,
                                          int y0, int x0, int ny, int nx, int rh, int rw, int nrows, int ncols,
                                          int r_lo, int c_lo, const float* tapw, int ts, const int32_t* taps,
                                          float* tmp, uint8_t* src, const PrepConsts& k, float* __restrict__ out) {
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int th = 2 + 2 * rh, tw = 2 + 2 * rw;
    const int row_b = ncols * 3;  // bytes of a staged row

    // 2. the footprint, folded, byte for byte: a wave per row, its lanes along the row
    for (int r = wv; r < nrows; r += kPrepThreads / kWave) {
        const uint8_t* g = img + static_cast<size_t>(fold_mirror(r_lo + r, h)) * w * 3;
        for (int b = lane; b < row_b; b += kWave) {
            const int col = b / 3, c = b - 3 * col;
            src[r * row_b + b] = g[fold_mirror(c_lo + col, w) * 3 + c];
        }
    }
    __syncthreads();

    // 3. horizontal pass: lane = output column, a wave per source row
    if (lane < nx) {
        const int sx = (taps[kPrepMaxTH + lane] - c_lo) * 3;
        const float* wx = tapw + (kPrepMaxTH + lane) * ts;
        const float w0 = wx[0], w1 = wx[1];
        for (int r = wv; r < nrows; r += kPrepThreads / kWave) {
            const uint8_t* s = src + r * row_b + sx;
            float a0, a1, a2;
            if (FAST) {
                a0 = fmaf(w1, static_cast<float>(s[3]), w0 * static_cast<float>(s[0]));
                a1 = fmaf(w1, static_cast<float>(s[4]), w0 * static_cast<float>(s[1]));
                a2 = fmaf(w1, static_cast<float>(s[5]), w0 * static_cast<float>(s[2]));
            } else {
                a0 = w0 * static_cast<float>(s[0]);
                a1 = w0 * static_cast<float>(s[1]);
                a2 = w0 * static_cast<float>(s[2]);
                for (int j = 1; j < tw; ++j) {
                    const float wj = wx[j];
                    a0 = fmaf(wj, static_cast<float>(s[3 * j]), a0);
                    a1 = fmaf(wj, static_cast<float>(s[3 * j + 1]), a1);
                    a2 = fmaf(wj, static_cast<float>(s[3 * j + 2]), a2);
                }
            }
            float* t = tmp + r * 3 * kPrepTW + lane;
            t[0] = a0, t[kPrepTW] = a1, t[2 * kPrepTW] = a2;
        }
    }
    __syncthreads();

    // 4. vertical pass: lane = output column, a wave per output row; 256-B stores
    if (lane < nx) {
        const size_t plane = static_cast<size_t>(out_h) * out_w;
        float* o = out + static_cast<size_t>(n) * 3 * plane + static_cast<size_t>(y0) * out_w + x0 + lane;
        for (int y = wv; y < ny; y += kPrepThreads / kWave) {
            const float* t = tmp + (taps[y] - r_lo) * 3 * kPrepTW + lane;
            const float* wy = tapw + y * ts;
            float a0 = wy[0] * t[0], a1 = wy[0] * t[kPrepTW], a2 = wy[0] * t[2 * kPrepTW];
            if (FAST) {
                a0 = fmaf(wy[1], t[3 * kPrepTW], a0);
                a1 = fmaf(wy[1], t[4 * kPrepTW], a1);
                a2 = fmaf(wy[1], t[5 * kPrepTW], a2);
            } else {
                for (int j = 1; j < th; ++j) {
                    const float wj = wy[j];
                    const float* tj = t + j * 3 * kPrepTW;
                    a0 = fmaf(wj, tj[0], a0);
                    a1 = fmaf(wj, tj[kPrepTW], a1);
                    a2 = fmaf(wj, tj[2 * kPrepTW], a2);
                }
            }
            float* oy = o + static_cast<size_t>(y) * out_w;
            oy[0] = fmaf(a0, k.scale[0], k.bias[0]);
            oy[plane] = fmaf(a1, k.scale[1], k.bias[1]);
            oy[2 * plane] = fmaf(a2, k.scale[2], k.bias[2]);
        }
    }
}

__global__ __launch_bounds__(kPrepThreads) void preprocess_kernel(
    const uint8_t* __restrict__ pixels, int64_t pixels_bytes, const int64_t* __restrict__ offset,
    const int32_t* __restrict__ hw, int max_h, int max_w, int out_h, int out_w, int TH, int lds_rows, int lds_cols,
    PrepLds L, PrepConsts k, float* __restrict__ out, int32_t* __restrict__ status) {
    extern __shared__ __align__(16) unsigned char lds[];
    double* gauss = reinterpret_cast<double*>(lds);              // [2][kPrepGauss]: axis h, axis w
    float* tmp = reinterpret_cast<float*>(lds + L.tmp);
    float* tapw = reinterpret_cast<float*>(lds + L.tapw);        // [kPrepTapRows][L.ts]
    int32_t* taps = reinterpret_cast<int32_t*>(lds + L.taps);    // rows 0..TH-1: axis h; kPrepMaxTH..: axis w
    uint8_t* src = lds + L.src;

    const int tid = threadIdx.x;
    const int n = blockIdx.z;
    const int y0 = blockIdx.y * TH, x0 = blockIdx.x * kPrepTW;
    const int ny = out_h - y0 < TH ? out_h - y0 : TH;
    const int nx = out_w - x0 < kPrepTW ? out_w - x0 : kPrepTW;

    // The image's size and offset come from the device: nothing below forms an
    // address from them until they have passed these checks.
    const int h = hw[2 * n], w = hw[2 * n + 1];
    const int64_t off = offset[n];
    int st = 0;
    if (h < 1 || h > max_h || w < 1 || w > max_w || h > kPrepMaxRatio * out_h || w > kPrepMaxRatio * out_w)
        st = 1;
    else if (off < 0 || off > pixels_bytes - 3 * static_cast<int64_t>(h) * w)
        st = 2;
    if (tid == 0 && blockIdx.x == 0 && blockIdx.y == 0) status[n] = st;
    if (st != 0) {  // never read: the tile's share of the three planes is zeros
        const size_t plane = static_cast<size_t>(out_h) * out_w;
        const int lane = tid & (kWave - 1);
        if (lane < nx) {
            float* o = out + static_cast<size_t>(n) * 3 * plane + static_cast<size_t>(y0) * out_w + x0 + lane;
            for (int y = tid / kWave; y < ny; y += kPrepThreads / kWave)
                for (int c = 0; c < 3; ++c) o[c * plane + static_cast<size_t>(y) * out_w] = 0.0f;
        }
        return;
    }

    // 1. tap tables.  Gaussian weights only where an axis is downscaled.
    double s2h, s2w;
    const int rh = axis_radius(h, out_h, &s2h), rw = axis_radius(w, out_w, &s2w);
    if (rh | rw) {
        if (tid < 2 * kPrepGauss) {
            const int kk = tid & (kPrepGauss - 1);
            const int r = tid < kPrepGauss ? rh : rw;
            const double s2 = tid < kPrepGauss ? s2h : s2w;
            gauss[tid] = kk == 0 ? 1.0 : (kk <= r ? exp(-0.5 / s2 * static_cast<double>(kk * kk)) : 0.0);
        }
        __syncthreads();
    }
    {
        const bool is_h = tid < ny, is_w = tid >= kWave && tid < kWave + nx;
        if (is_h || is_w) {
            const int d = is_h ? y0 + tid : x0 + tid - kWave;
            const int n_in = is_h ? h : w, n_out = is_h ? out_h : out_w, r = is_h ? rh : rw;
            const int row = is_h ? tid : kPrepMaxTH + tid - kWave;
            // position ((2d+1) n_in - n_out) / (2 n_out): exact integers, |num| < 2^28
            const int num = (2 * d + 1) * n_in - n_out, den = 2 * n_out;
            const int i0 = num < 0 ? -1 : num / den;   // floor: num > -den
            const double f = static_cast<double>(num - i0 * den) / static_cast<double>(den);
            taps[row] = i0 - r;
            float* wt = tapw + row * L.ts;
            if (r == 0) {
                wt[0] = static_cast<float>(1.0 - f);
                wt[1] = static_cast<float>(f);
            } else {
                const double* g = gauss + (is_h ? 0 : kPrepGauss);
                double sum = g[0];
                for (int kk = 1; kk <= r; ++kk) sum += 2.0 * g[kk];
                // tap j sits at i0 - r + j: (1-f) G(j-r) + f G(j-r-1), G(k) = g[|k|] / sum inside +-r
                for (int j = 0; j < 2 + 2 * r; ++j) {
                    const int ka = j - r < 0 ? r - j : j - r, kb = j - r - 1 < 0 ? r + 1 - j : j - r - 1;
                    const double ga = ka <= r ? g[ka] : 0.0, gb = kb <= r ? g[kb] : 0.0;
                    wt[j] = static_cast<float>(((1.0 - f) * ga + f * gb) / sum);
                }
            }
        }
    }
    __syncthreads();

    const int r_lo = taps[0], c_lo = taps[kPrepMaxTH];
    int nrows = taps[ny - 1] + 2 + 2 * rh - r_lo;
    int ncols = taps[kPrepMaxTH + nx - 1] + 2 + 2 * rw - c_lo;
    // span_bound() makes these hold; the clamp keeps LDS indices inside the allocation regardless
    nrows = nrows < lds_rows ? nrows : lds_rows;
    ncols = ncols < lds_cols ? ncols : lds_cols;

    const uint8_t* img = pixels + off;
    if ((rh | rw) == 0)
        prep_tile<true>(img, h, w, n, out_h, out_w, y0, x0, ny, nx, rh, rw, nrows, ncols, r_lo, c_lo, tapw, L.ts,
                        taps, tmp, src, k, out);
    else
        prep_tile<false>(img, h, w, n, out_h, out_w, y0, x0, ny, nx, rh, rw, nrows, ncols, r_lo, c_lo, tapw, L.ts,
                         taps, tmp, src, k, out);
}

__global__ __launch_bounds__(kPrepThreads) void rescale_boxes_kernel(int total, int G4, const double* __restrict__ boxes,
                                                                     const int32_t* __restrict__ hw, double out_h,
                                                                     double out_w, double* __restrict__ out) {
    const int i = blockIdx.x * kPrepThreads + threadIdx.x;
    if (i >= total) return;
    const int n = i / G4;
    const int h = hw[2 * n], w = hw[2 * n + 1];
    double v = -1.0;
    if (h >= 1 && w >= 1) {
        const bool col = i & 1;  // columns 1, 3 go by the width
        v = boxes[i] / static_cast<double>(col ? w : h);
        v = v * (col ? out_w : out_h);
        if (v < 0.0) v = -1.0;   // NaN stays NaN, as numpy's b[b < 0] = -1
    }
    out[i] = v;
}

// The argument rules of frcnn_preprocess and its workspace query.
const char* prep_args_error(int N, int max_h, int max_w, int out_h, int out_w) {
    if (N < 1 || N > 1024) return "N must be in [1, 1024]";
    if (out_h < 1 || out_h > 4096) return "out_h must be in [1, 4096]";
    if (out_w < 1 || out_w > 4096) return "out_w must be in [1, 4096]";
    if (max_h < 1 || max_h > 16384) return "max_h must be in [1, 16384]";
    if (max_w < 1 || max_w > 16384) return "max_w must be in [1, 16384]";
    return nullptr;
}

// The launch plan of frcnn_preprocess, from the host bounds alone: the tallest tile whose worst
// footprint fits the LDS budget, that footprint, the tap rows' width and the grid.  The launch and
// frcnn_preprocess_plan both read it from here.
struct PrepPlan {
    int TH, rows, cols, max_taps;
    PrepLds L;
    dim3 grid;
};

PrepPlan prep_plan(int N, int max_h, int max_w, int out_h, int out_w) {
    PrepPlan p;
    p.TH = kPrepMaxTH;
    p.cols = span_bound(kPrepTW, max_w, out_w);
    p.max_taps = std::max(span_bound(1, max_h, out_h), span_bound(1, max_w, out_w));  // 2 + 2r
    for (;; p.TH /= 2) {
        p.rows = span_bound(p.TH, max_h, out_h);
        p.L = prep_lds(p.rows, p.cols, p.max_taps);
        if (p.L.total <= kPrepLdsBudget || p.TH == 1) break;
    }
    p.grid = dim3((out_w + kPrepTW - 1) / kPrepTW, (out_h + p.TH - 1) / p.TH, N);
    return p;
}

}  // namespace
}  // namespace frcnn

using namespace frcnn;

extern "C" size_t frcnn_preprocess_workspace_size(int N, int max_h, int max_w, int out_h, int out_w) {
    if (prep_args_error(N, max_h, max_w, out_h, out_w)) return 0;
    return 256;  // nothing is kept between launches: one nominal block, so that 0 still means "rejected"
}

extern "C" int frcnn_preprocess_plan(int N, int max_h, int max_w, int out_h, int out_w, int32_t plan[8]) {
    if (const char* e = prep_args_error(N, max_h, max_w, out_h, out_w)) {
        set_error("frcnn_preprocess_plan: %s (N=%d, max_h=%d, max_w=%d, out_h=%d, out_w=%d)", e, N, max_h, max_w,
                  out_h, out_w);
        return FRCNN_EINVAL;
    }
    FRCNN_REQUIRE(plan, "frcnn_preprocess_plan: null plan");
    const PrepPlan p = prep_plan(N, max_h, max_w, out_h, out_w);
    FRCNN_REQUIRE(p.L.total <= kPrepLdsBudget, "frcnn_preprocess_plan: internal: a %d x %d footprint needs %zu B of LDS",
                  p.rows, p.cols, p.L.total);
    const int32_t v[8] = {p.TH, p.rows, p.cols, p.max_taps, static_cast<int32_t>(p.L.total),
                          static_cast<int32_t>(p.grid.x), static_cast<int32_t>(p.grid.y),
                          static_cast<int32_t>(p.grid.z)};
    std::copy(v, v + 8, plan);
    return FRCNN_OK;
}

extern "C" int frcnn_preprocess(int N, const uint8_t* pixels, int64_t pixels_bytes, const int64_t* offset,
                                const int32_t* hw, int max_h, int max_w, int out_h, int out_w, const float* mean,
                                const float* std, float* out, int32_t* status, void* workspace, size_t ws_bytes,
                                void* stream) {
    if (const char* e = prep_args_error(N, max_h, max_w, out_h, out_w)) {
        set_error("frcnn_preprocess: %s (N=%d, max_h=%d, max_w=%d, out_h=%d, out_w=%d)", e, N, max_h, max_w, out_h,
                  out_w);
        return FRCNN_EINVAL;
    }
    FRCNN_REQUIRE(mean && std, "frcnn_preprocess: null mean / std");
    PrepConsts k;
    for (int c = 0; c < 3; ++c) {
        FRCNN_REQUIRE(std::isfinite(mean[c]) && std::isfinite(std[c]) && std[c] > 0.0f,
                      "frcnn_preprocess: mean[%d]=%g must be finite and std[%d]=%g positive and finite", c, mean[c],
                      c, std[c]);
        k.scale[c] = static_cast<float>(1.0 / (255.0 * static_cast<double>(std[c])));
        k.bias[c] = static_cast<float>(-static_cast<double>(mean[c]) / static_cast<double>(std[c]));
    }
    FRCNN_REQUIRE(pixels_bytes >= 0, "frcnn_preprocess: pixels_bytes=%lld must not be negative",
                  static_cast<long long>(pixels_bytes));
    FRCNN_REQUIRE((pixels || pixels_bytes == 0) && offset && hw, "frcnn_preprocess: null input (pixels / offset / hw)");
    FRCNN_REQUIRE(out && status, "frcnn_preprocess: null output (out / status)");
    const size_t need = frcnn_preprocess_workspace_size(N, max_h, max_w, out_h, out_w);
    if (!workspace || ws_bytes < need) {
        set_error("frcnn_preprocess: workspace of %zu B < %zu B", workspace ? ws_bytes : size_t{0}, need);
        return FRCNN_EWORKSPACE;
    }
    const PrepPlan p = prep_plan(N, max_h, max_w, out_h, out_w);
    FRCNN_REQUIRE(p.L.total <= kPrepLdsBudget, "frcnn_preprocess: internal: a %d x %d footprint needs %zu B of LDS",
                  p.rows, p.cols, p.L.total);
    preprocess_kernel<<<p.grid, kPrepThreads, p.L.total, as_stream(stream)>>>(pixels, pixels_bytes, offset, hw, max_h,
                                                                           max_w, out_h, out_w, p.TH, p.rows, p.cols,
                                                                           p.L, k, out, status);
    FRCNN_LAUNCH_CHECK("preprocess_kernel");
    return FRCNN_OK;
}

extern "C" int frcnn_rescale_boxes(int N, int G, const double* boxes, const int32_t* hw, int out_h, int out_w,
                                   double* out, void* stream) {
    FRCNN_REQUIRE(N >= 1 && N <= 1024, "frcnn_rescale_boxes: N=%d must be in [1, 1024]", N);
    FRCNN_REQUIRE(G >= 0 && G <= 65536, "frcnn_rescale_boxes: G=%d must be in [0, 65536]", G);
    FRCNN_REQUIRE(out_h >= 1 && out_w >= 1, "frcnn_rescale_boxes: out_h=%d, out_w=%d must be positive", out_h, out_w);
    if (G == 0) return FRCNN_OK;  // no output elements
    FRCNN_REQUIRE(boxes && hw && out, "frcnn_rescale_boxes: null argument (boxes / hw / out)");
    const int total = N * G * 4;
    rescale_boxes_kernel<<<(total + kPrepThreads - 1) / kPrepThreads, kPrepThreads, 0, as_stream(stream)>>>(
        total, G * 4, boxes, hw, static_cast<double>(out_h), static_cast<double>(out_w), out);
    FRCNN_LAUNCH_CHECK("rescale_boxes_kernel");
    return FRCNN_OK;
}
