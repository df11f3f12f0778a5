// Pyramid mask head on gfx950: torchvision's project_masks_on_boxes (the mask targets of
// RoIHeads), maskrcnn_loss, and maskrcnn_inference + paste_masks_in_image for a whole batch
// (DESIGN.md §3 "Pyramid mask head"; include/frcnn_capi.h states the contract).  No host
// synchronisation, no float atomics, every output element stored exactly once.
//   mh_compact_kernel       one workgroup per image, thread = slot: ballot / prefix rank of the
//       positives (labels >= 1) in slot order; rows 0..count-1 of the image get their box, label,
//       gt index and source slot, the rows behind them the padding.
//   mh_targets_kernel       one workgroup per output row, thread = bin (lanes along the bin
//       columns, so neighbouring lanes read neighbouring mask bytes): RoIAlign of the matched
//       uint8 mask (scale 1, adaptive grid, aligned = false) in roi_align.hip's order of
//       operations, restated here for a one-channel byte plane.  "one": M * M <= 256, a thread
//       owns at most one bin; "strided" above.
//   mh_loss_rows_kernel<E>  one workgroup per row: the stable BCE of the labelled channel in fp32
//       per element, summed in fp64 (thread-strided, butterfly, waves in order) to partial[row].
//   mh_loss_final_kernel    one workgroup: S = sum of the counts, the partials in a fixed order,
//       loss = total / (S * M * M) (+0 for S == 0), the skipped rows counted.
//   mh_loss_bwd_kernel<E>   one thread per 16 bytes of the gradient: zeros, or
//       (sigmoid(x) - t) * (g / (S * M * M)) on the labelled plane of a real row.
//   mh_paste_kernel<E, Out> one workgroup per (detection, band of 32 canvas rows): the sigmoid of
//       the zero-padded mask goes to LDS once, each thread produces 16 consecutive bytes of a
//       canvas row (4 floats in the fp32 form) by ATen's bilinear formula and stores them with
//       one vector store; a row's unaligned head and tail are stored element by element.
#include <cmath>

#include "common.h"
#include "elem16.h"

namespace frcnn {
namespace {

constexpr int kMhMaxN = 1024;
constexpr int kMhMaxB = 1024;      // slots per image (B) and output rows per image (P, D)
constexpr int kMhMaxG = 256;
constexpr int kMhMaxM = 56;
constexpr int kMhMaxDim = 4096;    // mask and canvas edge
constexpr int kMhMaxC = 128;
constexpr int kMhMaxPad = 4;
constexpr int kMhScan = 16;        // kAlignScan: grids up to this many points per axis are walked whole
constexpr float kMhMaxCoord = 1048576;  // 2^20: a coordinate beyond it (NaN, inf included) guards the row
constexpr int kMhBand = 32;        // paste: canvas rows per workgroup
constexpr int kMhSide = kMhMaxM + 2 * kMhMaxPad;  // 64: the padded mask's largest edge

__device__ __forceinline__ bool mh_coord_ok(float v) { return fabsf(v) <= kMhMaxCoord; }
__device__ __forceinline__ int mh_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ------------------------------------------------------------------ targets
__global__ __launch_bounds__(1024) void mh_compact_kernel(const float* __restrict__ bt_rois,
                                                          const int32_t* __restrict__ bt_labels,
                                                          const int32_t* __restrict__ bt_matched, int B, int P,
                                                          float* __restrict__ rois, int32_t* __restrict__ labels,
                                                          int32_t* __restrict__ matched, int32_t* __restrict__ slot,
                                                          int32_t* __restrict__ count) {
    __shared__ int wcnt[16];
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const size_t src = static_cast<size_t>(n) * B + tid;
    int lab = -1;
    if (tid < B) lab = bt_labels[src];
    const bool pos = lab >= 1;
    const uint64_t bal = __ballot(pos);
    if (lane == 0) wcnt[wid] = __popcll(bal);
    __syncthreads();
    int before = 0, total = 0;
    for (int v = 0; v < 16; ++v) {
        const int c = wcnt[v];
        before += v < wid ? c : 0;
        total += c;
    }
    const int rank = before + __popcll(bal & lanemask_lt());
    const int cnt = total < P ? total : P;
    if (pos && rank < P) {
        const size_t o = static_cast<size_t>(n) * P + rank;
        const float* b = bt_rois + src * 5;
        float* r = rois + o * 5;
        r[0] = static_cast<float>(n);
        r[1] = b[1];
        r[2] = b[2];
        r[3] = b[3];
        r[4] = b[4];
        labels[o] = lab;
        matched[o] = bt_matched[src];
        slot[o] = tid;
    }
    if (tid >= cnt && tid < P) {
        const size_t o = static_cast<size_t>(n) * P + tid;
        float* r = rois + o * 5;
        r[0] = -1.f;
        r[1] = r[2] = r[3] = r[4] = 0.f;
        labels[o] = -1;
        matched[o] = -1;
        slot[o] = -1;
    }
    if (tid == 0) count[n] = cnt;
}

// roi_align.hip's align_pos / align_range / align_axis, restated (that unit's names and plans
// stay as they are).
__device__ __forceinline__ float mh_pos(float base, float bin, float gf, int i) {
    return base + ((static_cast<float>(i) + 0.5f) * bin) / gf;
}

// [a, e): the samples of an adaptive grid (bin > 0, pos nondecreasing in i) with -1 <= pos <= hi.
__device__ __forceinline__ void mh_range(float base, float bin, int g, float hi, int& a, int& e) {
    const float gf = static_cast<float>(g);
    int l = 0, r = g;
    while (l < r) {
        const int m = l + (r - l) / 2;
        if (mh_pos(base, bin, gf, m) >= -1.f) r = m; else l = m + 1;
    }
    a = l;
    r = g;
    while (l < r) {
        const int m = l + (r - l) / 2;
        if (mh_pos(base, bin, gf, m) <= hi) l = m + 1; else r = m;
    }
    e = l;
}

__device__ __forceinline__ void mh_axis(float v, int size, int& lo, int& hi, float& l, float& h) {
    if (v <= 0.f) v = 0.f;
    lo = static_cast<int>(v);
    if (lo >= size - 1) {
        hi = lo = size - 1;
        v = static_cast<float>(lo);
    } else {
        hi = lo + 1;
    }
    l = v - static_cast<float>(lo);
    h = 1.f - l;
}

__global__ __launch_bounds__(256) void mh_targets_kernel(const uint8_t* __restrict__ masks, int G, int H, int W, int P,
                                                         int M, const float* __restrict__ rois,
                                                         const int32_t* __restrict__ matched,
                                                         const int32_t* __restrict__ count,
                                                         float* __restrict__ targets) {
    const int row = blockIdx.x, tid = threadIdx.x;
    const int n = row / P, r = row - n * P;
    const int MM = M * M;
    float* o = targets + static_cast<size_t>(row) * MM;
    const int cnt = mh_clampi(count[n], 0, P);
    const int g = matched[row];
    const float* b = rois + static_cast<size_t>(row) * 5;
    const float x1 = b[1], y1 = b[2], x2 = b[3], y2 = b[4];
    const bool ok = r < cnt && g >= 0 && g < G && mh_coord_ok(x1) && mh_coord_ok(y1) && mh_coord_ok(x2) && mh_coord_ok(y2);
    if (!ok) {
        for (int i = tid; i < MM; i += 256) o[i] = 0.f;
        return;
    }
    const uint8_t* plane = masks + (static_cast<size_t>(n) * G + g) * H * W;  // g in [0, G)
    float rw = x2 - x1, rh = y2 - y1;
    rw = rw < 1.f ? 1.f : rw;
    rh = rh < 1.f ? 1.f : rh;
    const float fM = static_cast<float>(M);
    const float bh = rh / fM, bw = rw / fM;
    const int gh = static_cast<int>(ceilf(rh / fM)), gw = static_cast<int>(ceilf(rw / fM));  // >= 1, <= 2^21
    const int64_t c64 = static_cast<int64_t>(gh) * gw;
    const float scount = static_cast<float>(c64 > 1 ? c64 : 1);
    const float gfh = static_cast<float>(gh), gfw = static_cast<float>(gw);
    const float fH = static_cast<float>(H), fW = static_cast<float>(W);
    for (int bin = tid; bin < MM; bin += 256) {
        const int ph = bin / M, pw = bin - ph * M;
        const float basey = y1 + static_cast<float>(ph) * bh, basex = x1 + static_cast<float>(pw) * bw;
        int ya = 0, ye = gh, xa = 0, xe = gw;
        if (gh > kMhScan) mh_range(basey, bh, gh, fH, ya, ye);
        if (gw > kMhScan) mh_range(basex, bw, gw, fW, xa, xe);
        float acc = 0.f;
        for (int iy = ya; iy < ye; ++iy) {
            const float y = mh_pos(basey, bh, gfh, iy);
            if (y < -1.f || y > fH) continue;
            int yl, yh;
            float ly, hy;
            mh_axis(y, H, yl, yh, ly, hy);  // yl, yh in [0, H)
            const uint8_t* rl = plane + static_cast<size_t>(yl) * W;
            const uint8_t* rh_ = plane + static_cast<size_t>(yh) * W;
            for (int ix = xa; ix < xe; ++ix) {
                const float xx = mh_pos(basex, bw, gfw, ix);
                if (xx < -1.f || xx > fW) continue;
                int xl, xh;
                float lx, hx;
                mh_axis(xx, W, xl, xh, lx, hx);  // xl, xh in [0, W)
                const float w1 = hy * hx, w2 = hy * lx, w3 = ly * hx, w4 = ly * lx;
                const float v1 = static_cast<float>(rl[xl]), v2 = static_cast<float>(rl[xh]);
                const float v3 = static_cast<float>(rh_[xl]), v4 = static_cast<float>(rh_[xh]);
                const float val = ((w1 * v1 + w2 * v2) + w3 * v3) + w4 * v4;
                acc = acc + val;
            }
        }
        o[bin] = acc / scount;
    }
}

// ------------------------------------------------------------------- losses
struct MhLossWs {
    double* partial;   // [N * P]
    int32_t* skipped;  // [N * P]
    size_t bytes;
};

MhLossWs mh_loss_carve(void* ws, int N, int P) {
    Carver c(ws);
    MhLossWs w{};
    const size_t rows = static_cast<size_t>(N) * P;
    w.partial = c.take<double>(rows);
    w.skipped = c.take<int32_t>(rows);
    w.bytes = c.used();
    return w;
}

// 1 / (1 + exp(-x)): exp correctly rounded, the sum and the quotient rounded once each.
__device__ __forceinline__ float mh_sigmoid(float x) { return 1.f / (1.f + exp_cr(-x)); }

template <class E>
__global__ __launch_bounds__(256) void mh_loss_rows_kernel(const typename E::raw* __restrict__ logits,
                                                           const float* __restrict__ targets,
                                                           const int32_t* __restrict__ labels,
                                                           const int32_t* __restrict__ count, int P, int C, int MM,
                                                           MhLossWs w) {
    __shared__ double red[4];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int n = row / P, r = row - n * P;
    const int cnt = mh_clampi(count[n], 0, P);
    const int lab = labels[row];
    const bool real = r < cnt;
    const bool use = real && lab >= 0 && lab < C;
    double acc = 0.0;
    if (use) {
        const typename E::raw* x = logits + (static_cast<size_t>(row) * C + lab) * MM;
        const float* t = targets + static_cast<size_t>(row) * MM;
        for (int i = tid; i < MM; i += 256) {
            const float xv = E::widen(x[i]), tv = t[i];
            // max(x, 0) - x * t + log1p(exp(-|x|)): no overflow for any finite x
            const float e = exp_cr(-fabsf(xv));
            const float lg = static_cast<float>(log1p(static_cast<double>(e)));
            const float l = ((xv > 0.f ? xv : (xv != xv ? xv : 0.f)) - xv * tv) + lg;
            acc += static_cast<double>(l);
        }
    }
    acc = wave_reduce(acc, op_add());
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        w.partial[row] = ((red[0] + red[1]) + red[2]) + red[3];
        w.skipped[row] = real && !use ? 1 : 0;
    }
}

__global__ __launch_bounds__(1024) void mh_loss_final_kernel(const int32_t* __restrict__ count, int N, int P, int MM,
                                                             MhLossWs w, float* __restrict__ loss,
                                                             int32_t* __restrict__ stats) {
    __shared__ double rsum[16];
    __shared__ int rs[16], rk[16];
    const int tid = threadIdx.x;
    const int64_t rows = static_cast<int64_t>(N) * P;
    double a = 0.0;
    int sk = 0, s = 0;
    for (int64_t i = tid; i < rows; i += 1024) {
        a += w.partial[i];
        sk += w.skipped[i];
    }
    for (int i = tid; i < N; i += 1024) s += mh_clampi(count[i], 0, P);
    a = wave_reduce(a, op_add());
    sk = wave_reduce(sk, op_add());
    s = wave_reduce(s, op_add());
    if ((tid & 63) == 0) {
        rsum[tid >> 6] = a;
        rs[tid >> 6] = s;
        rk[tid >> 6] = sk;
    }
    __syncthreads();
    if (tid == 0) {
        double tot = 0.0;
        int S = 0, K = 0;
        for (int v = 0; v < 16; ++v) {
            tot += rsum[v];
            S += rs[v];
            K += rk[v];
        }
        loss[0] = S > 0 ? static_cast<float>(tot / (static_cast<double>(S) * MM)) : 0.f;
        stats[0] = S;
        stats[1] = K;
        stats[2] = 0;
        stats[3] = 0;
    }
}

template <class E>
__global__ __launch_bounds__(256) void mh_loss_bwd_kernel(const typename E::raw* __restrict__ logits,
                                                          const float* __restrict__ targets,
                                                          const int32_t* __restrict__ labels,
                                                          const int32_t* __restrict__ count,
                                                          const int32_t* __restrict__ stats, const float* __restrict__ g,
                                                          int P, int C, int MM, int64_t total,
                                                          typename E::raw* __restrict__ d) {
    using raw = typename E::raw;
    constexpr int V = 16 / sizeof(raw);
    const int64_t e0 = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) * V;
    if (e0 >= total) return;
    const int nel = total - e0 < V ? static_cast<int>(total - e0) : V;
    const int64_t row_sz = static_cast<int64_t>(C) * MM;
    const int64_t r0 = e0 / row_sz, r1 = (e0 + nel - 1) / row_sz;
    bool hot = false;
    if (g) {
        for (int64_t row = r0; row <= r1; ++row) {  // at most a few rows
            const int n = static_cast<int>(row / P), r = static_cast<int>(row - static_cast<int64_t>(n) * P);
            const int lab = labels[row];
            if (r < mh_clampi(count[n], 0, P) && lab >= 0 && lab < C) {
                const int64_t lp = (row * C + lab) * MM;
                hot = hot || (lp < e0 + nel && lp + MM > e0);
            }
        }
    }
    union {
        raw e[V];
        uint4 q;
    } out;
    out.q = make_uint4(0u, 0u, 0u, 0u);  // +0 in every element type
    if (hot) {
        const int S = stats[0];
        const float scale = g[0] / static_cast<float>(static_cast<int64_t>(S) * MM);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            if (j < nel) {
                const int64_t e = e0 + j;
                const int64_t row = e / row_sz;
                const int rem = static_cast<int>(e - row * row_sz);
                const int ch = rem / MM, k = rem - ch * MM;
                const int n = static_cast<int>(row / P), r = static_cast<int>(row - static_cast<int64_t>(n) * P);
                if (r < mh_clampi(count[n], 0, P) && ch == labels[row]) {
                    const float x = E::widen(logits[e]);
                    const float t = targets[row * MM + k];
                    out.e[j] = E::narrow((mh_sigmoid(x) - t) * scale);
                }
            }
        }
    }
    if (nel == V) {
        *reinterpret_cast<uint4*>(d + e0) = out.q;  // d is 16-byte aligned and e0 a multiple of V
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (j < nel) d[e0 + j] = out.e[j];
    }
}

// -------------------------------------------------------------------- paste
struct MhPaste {
    int D, C, M, pad, Hc, Wc, binary;
    float thr;
};

template <class Out>
__device__ __forceinline__ Out mh_pixel(float v, const MhPaste& q);
template <>
__device__ __forceinline__ uint8_t mh_pixel<uint8_t>(float v, const MhPaste& q) { return v > q.thr ? 1 : 0; }
template <>
__device__ __forceinline__ float mh_pixel<float>(float v, const MhPaste&) { return v; }

// ATen's area_pixel_compute_source_index (align_corners = false) and the two taps of an axis.
__device__ __forceinline__ void mh_taps(float scale, int d, int S, int& i0, int& i1, float& l0, float& l1) {
    float src = scale * (static_cast<float>(d) + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
    i0 = static_cast<int>(src);
    i0 = i0 > S - 1 ? S - 1 : i0;
    i1 = i0 + (i0 < S - 1 ? 1 : 0);
    l1 = src - static_cast<float>(i0);
    l0 = 1.f - l1;
}

template <class E, class Out>
__global__ __launch_bounds__(256) void mh_paste_kernel(MhPaste q, const typename E::raw* __restrict__ logits,
                                                       const float4* __restrict__ boxes,
                                                       const int32_t* __restrict__ labels,
                                                       const int32_t* __restrict__ count,
                                                       const float* __restrict__ img_sizes,
                                                       const float* __restrict__ orig_sizes, Out* __restrict__ out) {
    constexpr int V = 16 / sizeof(Out);
    __shared__ float prob[kMhSide * kMhSide];
    const int det = blockIdx.x, tid = threadIdx.x;
    const int n = det / q.D, dd = det - n * q.D;
    const int Hc = q.Hc, Wc = q.Wc, M = q.M, p = q.pad, S = M + 2 * p;
    const int ya = blockIdx.y * kMhBand, ye = ya + kMhBand < Hc ? ya + kMhBand : Hc;
    const int cnt = mh_clampi(count[n], 0, q.D);
    const int lab = labels[det];
    float4 b = boxes[det];
    bool ok = dd < cnt && lab >= 1 && lab < q.C && mh_coord_ok(b.x) && mh_coord_ok(b.y) && mh_coord_ok(b.z) &&
              mh_coord_ok(b.w) && b.z >= b.x && b.w >= b.y;
    int im_h = Hc, im_w = Wc;
    if (orig_sizes) {
        const float oh = orig_sizes[2 * n], ow = orig_sizes[2 * n + 1];
        // the image's own size clips the paste; the canvas clips it again (NaN, negative: nothing)
        const int ih = oh >= 1.f ? static_cast<int>(oh < 4096.f ? oh : 4096.f) : 0;
        const int iw = ow >= 1.f ? static_cast<int>(ow < 4096.f ? ow : 4096.f) : 0;
        im_h = ih < Hc ? ih : Hc;
        im_w = iw < Wc ? iw : Wc;
        if (img_sizes) {  // resize_boxes, as bd_merge_kernel does it
            const float ratio_h = oh / img_sizes[2 * n], ratio_w = ow / img_sizes[2 * n + 1];
            b.x = b.x * ratio_w;
            b.z = b.z * ratio_w;
            b.y = b.y * ratio_h;
            b.w = b.w * ratio_h;
        }
    }
    // expand_boxes: fp32, every operation rounded
    const float scale = static_cast<float>(S) / static_cast<float>(M);
    float w_half = (b.z - b.x) * 0.5f, h_half = (b.w - b.y) * 0.5f;
    const float x_c = (b.z + b.x) * 0.5f, y_c = (b.w + b.y) * 0.5f;
    w_half = w_half * scale;
    h_half = h_half * scale;
    const float ex1 = x_c - w_half, ex2 = x_c + w_half, ey1 = y_c - h_half, ey2 = y_c + h_half;
    ok = ok && mh_coord_ok(ex1) && mh_coord_ok(ex2) && mh_coord_ok(ey1) && mh_coord_ok(ey2);
    int b0 = 0, b1 = 0, b2 = 0, b3 = 0;
    if (ok) {  // truncation toward zero
        b0 = static_cast<int>(ex1);
        b1 = static_cast<int>(ey1);
        b2 = static_cast<int>(ex2);
        b3 = static_cast<int>(ey2);
    }
    int w = b2 - b0 + 1, h = b3 - b1 + 1;
    w = w > 1 ? w : 1;
    h = h > 1 ? h : 1;
    const int x0 = b0 > 0 ? b0 : 0, x1 = b2 + 1 < im_w ? b2 + 1 : im_w;
    const int y0 = b1 > 0 ? b1 : 0, y1 = b3 + 1 < im_h ? b3 + 1 : im_h;
    // [x0, x1) lies in [b0, b0 + w) and [y0, y1) in [b1, b1 + h): every tap index is in [0, S)
    const bool live = ok && x0 < x1 && y0 < y1 && ya < y1 && ye > y0;  // uniform
    if (live) {
        const typename E::raw* src = logits + (static_cast<size_t>(det) * q.C + lab) * M * M;
        for (int i = tid; i < S * S; i += 256) {
            const int yy = i / S - p, xx = i - (i / S) * S - p;
            float v = 0.f;
            if (yy >= 0 && yy < M && xx >= 0 && xx < M) v = mh_sigmoid(E::widen(src[yy * M + xx]));
            prob[i] = v;
        }
    }
    __syncthreads();
    const float scale_x = static_cast<float>(S) / static_cast<float>(w);
    const float scale_y = static_cast<float>(S) / static_cast<float>(h);
    const int items = 1 + (Wc + V - 1) / V;  // item 0: a row's unaligned head; then runs of V elements
    const int nwork = (ye - ya) * items;
    for (int it = tid; it < nwork; it += 256) {
        const int yr = it / items, k = it - yr * items;
        const int y = ya + yr;
        Out* rowp = out + (static_cast<size_t>(det) * Hc + y) * Wc;
        int head = static_cast<int>(((16u - (reinterpret_cast<uintptr_t>(rowp) & 15u)) & 15u) / sizeof(Out));
        head = head < Wc ? head : Wc;
        const int xs = k == 0 ? 0 : head + (k - 1) * V;
        int xn = k == 0 ? head : V;
        if (xs + xn > Wc) xn = Wc - xs;
        if (xn <= 0) continue;
        union {
            Out e[V];
            uint4 qv;
        } o;
        o.qv = make_uint4(0u, 0u, 0u, 0u);
        if (live && y >= y0 && y < y1 && xs < x1 && xs + xn > x0) {
            int iy0, iy1;
            float l0y, l1y;
            mh_taps(scale_y, y - b1, S, iy0, iy1, l0y, l1y);
            const float* r0 = prob + iy0 * S;
            const float* r1 = prob + iy1 * S;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const int X = xs + j;
                if (j < xn && X >= x0 && X < x1) {
                    int ix0, ix1;
                    float l0x, l1x;
                    mh_taps(scale_x, X - b0, S, ix0, ix1, l0x, l1x);
                    const float top = l0x * r0[ix0] + l1x * r0[ix1];
                    const float bot = l0x * r1[ix0] + l1x * r1[ix1];
                    o.e[j] = mh_pixel<Out>(l0y * top + l1y * bot, q);
                }
            }
        }
        if (xn == V && k > 0) {
            *reinterpret_cast<uint4*>(rowp + xs) = o.qv;  // rowp + head is 16-byte aligned
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j)
                if (j < xn) rowp[xs + j] = o.e[j];
        }
    }
}

const char* mh_elem_name(int dtype) { return dtype == FRCNN_F32 ? "ElemF32" : dtype == FRCNN_F16 ? "ElemF16" : "ElemBF16"; }

int mh_check_rows(const char* who, int N, int P, const char* pname) {
    FRCNN_REQUIRE(N >= 1 && N <= kMhMaxN, "%s: N must be in [1, %d], got %d", who, kMhMaxN, N);
    FRCNN_REQUIRE(P >= 1 && P <= kMhMaxB, "%s: %s must be in [1, %d], got %d", who, pname, kMhMaxB, P);
    return FRCNN_OK;
}

int mh_check_cm(const char* who, int C, int M) {
    FRCNN_REQUIRE(C >= 2 && C <= kMhMaxC, "%s: C must be in [2, %d], got %d", who, kMhMaxC, C);
    FRCNN_REQUIRE(M >= 1 && M <= kMhMaxM, "%s: mask_size M must be in [1, %d], got %d", who, kMhMaxM, M);
    return FRCNN_OK;
}

template <class E>
int mh_paste_launch(const MhPaste& q, int N, const void* logits, const float* boxes, const int32_t* labels,
                    const int32_t* count, const float* img, const float* orig, void* out, hipStream_t st) {
    const dim3 grid(N * q.D, (q.Hc + kMhBand - 1) / kMhBand);
    const typename E::raw* lg = static_cast<const typename E::raw*>(logits);
    const float4* bx = reinterpret_cast<const float4*>(boxes);
    if (q.binary)
        hipLaunchKernelGGL((mh_paste_kernel<E, uint8_t>), grid, dim3(256), 0, st, q, lg, bx, labels, count, img, orig,
                           static_cast<uint8_t*>(out));
    else
        hipLaunchKernelGGL((mh_paste_kernel<E, float>), grid, dim3(256), 0, st, q, lg, bx, labels, count, img, orig,
                           static_cast<float*>(out));
    FRCNN_LAUNCH_CHECK("mh_paste_kernel");
    return FRCNN_OK;
}

}  // namespace
}  // namespace frcnn

using namespace frcnn;

extern "C" int frcnn_mask_targets_kernel(int B, int P, int M, char* name, size_t len) {
    const char* who = "frcnn_mask_targets_kernel";
    FRCNN_REQUIRE(name && len > 0, "%s: null name buffer", who);
    int rc = mh_check_rows(who, 1, B, "B");
    if (rc) return rc;
    rc = mh_check_rows(who, 1, P, "positives_per_image");
    if (rc) return rc;
    FRCNN_REQUIRE(M >= 1 && M <= kMhMaxM, "%s: mask_size M must be in [1, %d], got %d", who, kMhMaxM, M);
    std::snprintf(name, len, "mh_compact_kernel mh_targets_kernel[%s]", M * M <= 256 ? "one" : "strided");
    return FRCNN_OK;
}

extern "C" int frcnn_mask_targets(int N, int B, int P, int G, int Hm, int Wm, int M, const float* bt_rois,
                                  const int32_t* bt_labels, const int32_t* bt_matched, const uint8_t* gt_masks,
                                  float* rois, int32_t* labels, int32_t* matched, int32_t* slot, int32_t* count,
                                  float* targets, void* stream) {
    const char* who = "frcnn_mask_targets";
    int rc = mh_check_rows(who, N, B, "B");
    if (rc) return rc;
    rc = mh_check_rows(who, N, P, "positives_per_image");
    if (rc) return rc;
    FRCNN_REQUIRE(G >= 1 && G <= kMhMaxG, "%s: G must be in [1, %d], got %d", who, kMhMaxG, G);
    FRCNN_REQUIRE(Hm >= 1 && Hm <= kMhMaxDim && Wm >= 1 && Wm <= kMhMaxDim,
                  "%s: gt_masks: Hm and Wm must be in [1, %d], got %d x %d", who, kMhMaxDim, Hm, Wm);
    FRCNN_REQUIRE(M >= 1 && M <= kMhMaxM, "%s: mask_size M must be in [1, %d], got %d", who, kMhMaxM, M);
    FRCNN_REQUIRE(bt_rois && bt_labels && bt_matched && gt_masks,
                  "%s: null input (rois / labels / matched of the box targets / gt_masks)", who);
    FRCNN_REQUIRE(rois && labels && matched && slot && count && targets,
                  "%s: null output (rois / labels / matched / slot / count / targets)", who);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(mh_compact_kernel, dim3(N), dim3(1024), 0, st, bt_rois, bt_labels, bt_matched, B, P, rois, labels,
                       matched, slot, count);
    FRCNN_LAUNCH_CHECK("mh_compact_kernel");
    hipLaunchKernelGGL(mh_targets_kernel, dim3(N * P), dim3(256), 0, st, gt_masks, G, Hm, Wm, P, M, rois, matched, count,
                       targets);
    FRCNN_LAUNCH_CHECK("mh_targets_kernel");
    return FRCNN_OK;
}

extern "C" size_t frcnn_mask_losses_workspace_size(int N, int P) {
    if (mh_check_rows("frcnn_mask_losses_workspace_size", N, P, "P")) return 0;
    return mh_loss_carve(nullptr, N, P).bytes;
}

extern "C" int frcnn_mask_losses_kernel(int dtype, int C, int M, char* name, size_t len) {
    const char* who = "frcnn_mask_losses_kernel";
    FRCNN_REQUIRE(name && len > 0, "%s: null name buffer", who);
    FRCNN_REQUIRE(dtype_code_ok(dtype), "%s: dtype must be FRCNN_F32, FRCNN_F16 or FRCNN_BF16, got %d", who, dtype);
    int rc = mh_check_cm(who, C, M);
    if (rc) return rc;
    const char* e = mh_elem_name(dtype);
    std::snprintf(name, len, "mh_loss_rows_kernel<%s> mh_loss_final_kernel mh_loss_bwd_kernel<%s>[vec%d]", e, e,
                  dtype == FRCNN_F32 ? 4 : 8);
    return FRCNN_OK;
}

extern "C" int frcnn_mask_losses_fwd_t(int dtype, int N, int P, int C, int M, const void* mask_logits,
                                       const float* targets, const int32_t* labels, const int32_t* count, float* loss,
                                       int32_t* stats, void* workspace, size_t ws_bytes, void* stream) {
    const char* who = "frcnn_mask_losses_fwd_t";
    FRCNN_REQUIRE(dtype_code_ok(dtype), "%s: dtype must be FRCNN_F32, FRCNN_F16 or FRCNN_BF16, got %d", who, dtype);
    int rc = mh_check_rows(who, N, P, "P");
    if (rc) return rc;
    rc = mh_check_cm(who, C, M);
    if (rc) return rc;
    FRCNN_REQUIRE(mask_logits && targets && labels && count, "%s: null input (mask_logits / targets / labels / count)",
                  who);
    FRCNN_REQUIRE(aligned_to(mask_logits, dtype == FRCNN_F32 ? 4 : 2), "%s: mask_logits not aligned to its element type",
                  who);
    FRCNN_REQUIRE(loss && stats, "%s: null output (loss / stats)", who);
    const MhLossWs w = mh_loss_carve(workspace, N, P);
    if (!workspace || ws_bytes < w.bytes) {
        set_error("%s: workspace %zu < %zu", who, workspace ? ws_bytes : size_t{0}, w.bytes);
        return FRCNN_EWORKSPACE;
    }
    FRCNN_REQUIRE(aligned_to(workspace, 256), "%s: workspace must be 256-byte aligned", who);
    hipStream_t st = as_stream(stream);
    const int MM = M * M;
    if (dtype == FRCNN_F32)
        hipLaunchKernelGGL((mh_loss_rows_kernel<ElemF32>), dim3(N * P), dim3(256), 0, st,
                           static_cast<const float*>(mask_logits), targets, labels, count, P, C, MM, w);
    else if (dtype == FRCNN_F16)
        hipLaunchKernelGGL((mh_loss_rows_kernel<ElemF16>), dim3(N * P), dim3(256), 0, st,
                           static_cast<const uint16_t*>(mask_logits), targets, labels, count, P, C, MM, w);
    else
        hipLaunchKernelGGL((mh_loss_rows_kernel<ElemBF16>), dim3(N * P), dim3(256), 0, st,
                           static_cast<const uint16_t*>(mask_logits), targets, labels, count, P, C, MM, w);
    FRCNN_LAUNCH_CHECK("mh_loss_rows_kernel");
    hipLaunchKernelGGL(mh_loss_final_kernel, dim3(1), dim3(1024), 0, st, count, N, P, MM, w, loss, stats);
    FRCNN_LAUNCH_CHECK("mh_loss_final_kernel");
    return FRCNN_OK;
}

extern "C" int frcnn_mask_losses_bwd_t(int dtype, int N, int P, int C, int M, const void* mask_logits,
                                       const float* targets, const int32_t* labels, const int32_t* count,
                                       const int32_t* stats, const float* g_loss, void* dlogits, void* stream) {
    const char* who = "frcnn_mask_losses_bwd_t";
    FRCNN_REQUIRE(dtype_code_ok(dtype), "%s: dtype must be FRCNN_F32, FRCNN_F16 or FRCNN_BF16, got %d", who, dtype);
    int rc = mh_check_rows(who, N, P, "P");
    if (rc) return rc;
    rc = mh_check_cm(who, C, M);
    if (rc) return rc;
    FRCNN_REQUIRE(mask_logits && targets && labels && count && stats,
                  "%s: null input (mask_logits / targets / labels / count / stats)", who);
    FRCNN_REQUIRE(aligned_to(mask_logits, dtype == FRCNN_F32 ? 4 : 2), "%s: mask_logits not aligned to its element type",
                  who);
    FRCNN_REQUIRE(dlogits, "%s: null output (dlogits)", who);
    FRCNN_REQUIRE(aligned_to(dlogits, 16), "%s: dlogits must be 16-byte aligned", who);
    hipStream_t st = as_stream(stream);
    const int MM = M * M;
    const int64_t total = static_cast<int64_t>(N) * P * C * MM;
    const int V = dtype == FRCNN_F32 ? 4 : 8;
    const int64_t vecs = (total + V - 1) / V;
    const dim3 grid(static_cast<unsigned>((vecs + 255) / 256));  // <= 2^20 * 128 * 3136 / (4 * 256) < 2^31
    if (dtype == FRCNN_F32)
        hipLaunchKernelGGL((mh_loss_bwd_kernel<ElemF32>), grid, dim3(256), 0, st, static_cast<const float*>(mask_logits),
                           targets, labels, count, stats, g_loss, P, C, MM, total, static_cast<float*>(dlogits));
    else if (dtype == FRCNN_F16)
        hipLaunchKernelGGL((mh_loss_bwd_kernel<ElemF16>), grid, dim3(256), 0, st,
                           static_cast<const uint16_t*>(mask_logits), targets, labels, count, stats, g_loss, P, C, MM,
                           total, static_cast<uint16_t*>(dlogits));
    else
        hipLaunchKernelGGL((mh_loss_bwd_kernel<ElemBF16>), grid, dim3(256), 0, st,
                           static_cast<const uint16_t*>(mask_logits), targets, labels, count, stats, g_loss, P, C, MM,
                           total, static_cast<uint16_t*>(dlogits));
    FRCNN_LAUNCH_CHECK("mh_loss_bwd_kernel");
    return FRCNN_OK;
}

extern "C" int frcnn_mask_paste_kernel(int dtype, int M, int padding, int Wc, int binary, char* name, size_t len) {
    const char* who = "frcnn_mask_paste_kernel";
    FRCNN_REQUIRE(name && len > 0, "%s: null name buffer", who);
    FRCNN_REQUIRE(dtype_code_ok(dtype), "%s: dtype must be FRCNN_F32, FRCNN_F16 or FRCNN_BF16, got %d", who, dtype);
    FRCNN_REQUIRE(M >= 1 && M <= kMhMaxM, "%s: mask_size M must be in [1, %d], got %d", who, kMhMaxM, M);
    FRCNN_REQUIRE(padding >= 0 && padding <= kMhMaxPad, "%s: padding must be in [0, %d], got %d", who, kMhMaxPad, padding);
    FRCNN_REQUIRE(Wc >= 1 && Wc <= kMhMaxDim, "%s: canvas_size: Wc must be in [1, %d], got %d", who, kMhMaxDim, Wc);
    const int V = binary ? 16 : 4;
    std::snprintf(name, len, "mh_paste_kernel<%s,%s>[vec%d%s]", mh_elem_name(dtype), binary ? "u8" : "f32", V,
                  Wc % V == 0 ? "" : "+edges");
    return FRCNN_OK;
}

extern "C" int frcnn_mask_paste_t(int dtype, int N, int D, int C, int M, const void* mask_logits, const float* boxes,
                                  const int32_t* labels, const int32_t* count, const float* image_sizes,
                                  const float* original_sizes, int padding, float threshold, int binary, int Hc, int Wc,
                                  void* masks, void* stream) {
    const char* who = "frcnn_mask_paste_t";
    FRCNN_REQUIRE(dtype_code_ok(dtype), "%s: dtype must be FRCNN_F32, FRCNN_F16 or FRCNN_BF16, got %d", who, dtype);
    int rc = mh_check_rows(who, N, D, "D");
    if (rc) return rc;
    rc = mh_check_cm(who, C, M);
    if (rc) return rc;
    FRCNN_REQUIRE(padding >= 0 && padding <= kMhMaxPad, "%s: padding must be in [0, %d], got %d", who, kMhMaxPad, padding);
    FRCNN_REQUIRE(Hc >= 1 && Hc <= kMhMaxDim && Wc >= 1 && Wc <= kMhMaxDim,
                  "%s: canvas_size: Hc and Wc must be in [1, %d], got %d x %d", who, kMhMaxDim, Hc, Wc);
    FRCNN_REQUIRE(!binary || threshold == threshold, "%s: threshold must not be NaN", who);
    FRCNN_REQUIRE(!image_sizes || original_sizes, "%s: image_sizes needs original_sizes", who);
    FRCNN_REQUIRE(mask_logits && boxes && labels && count, "%s: null input (mask_logits / boxes / labels / count)", who);
    FRCNN_REQUIRE(aligned_to(mask_logits, dtype == FRCNN_F32 ? 4 : 2), "%s: mask_logits not aligned to its element type",
                  who);
    FRCNN_REQUIRE(aligned_to(boxes, 16), "%s: boxes must be 16-byte aligned", who);
    FRCNN_REQUIRE(masks, "%s: null output (masks)", who);
    FRCNN_REQUIRE(binary || aligned_to(masks, 4), "%s: masks not aligned to fp32", who);
    MhPaste q{};
    q.D = D;
    q.C = C;
    q.M = M;
    q.pad = padding;
    q.Hc = Hc;
    q.Wc = Wc;
    q.binary = binary ? 1 : 0;
    q.thr = threshold;
    hipStream_t st = as_stream(stream);
    if (dtype == FRCNN_F32)
        return mh_paste_launch<ElemF32>(q, N, mask_logits, boxes, labels, count, image_sizes, original_sizes, masks, st);
    if (dtype == FRCNN_F16)
        return mh_paste_launch<ElemF16>(q, N, mask_logits, boxes, labels, count, image_sizes, original_sizes, masks, st);
    return mh_paste_launch<ElemBF16>(q, N, mask_logits, boxes, labels, count, image_sizes, original_sizes, masks, st);
}
