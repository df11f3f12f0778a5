// RoIAlign forward and backward for gfx950 (torchvision.ops.roi_align, CPU-kernel
// semantics; DESIGN.md §3 "RoIAlign" is the contract, include/frcnn_capi.h repeats it).
//
// Every fp32 operation below is rounded separately (-ffp-contract=off, correctly
// rounded divide), and both kernels add in the contract's order, so the results are
// bit-exact against the restatement in tests/roi_align_ref.py and the same on every
// call.  No atomics.
//
// Forward: one thread per bin of one RoI and run of 8 channels, which share the
// bin's geometry; consecutive lanes take consecutive bins of the RoI, so for each
// channel a wave reads neighbouring pixels of one feature plane and stores
// consecutive outputs.  Each output still sums its own samples in iy, ix order.
//
// Backward: one wave owns an 8 x 8 pixel tile of one image for 64 channels (lane =
// channel) and keeps its fp32 sums in LDS as [pixel][channel], each pixel row padded
// to 65 words: the accumulation (lane = channel) and the write-out (lane = pixel) are
// both free of bank conflicts.  The wave scans the RoIs 64 at a time (lane = RoI),
// keeps those of its image by ballot, and walks them in ascending index, their bins
// and samples in contract order; along each axis it first narrows the bins, then
// each bin's samples, to those that can touch its tile.  With up to 64 samples per
// axis the lanes work the samples of a RoI out once, one sample per lane, and the walk
// reads them lane by lane; a touching RoI's gradients for the wave's 64 channels are
// one contiguous block of grad and are staged in LDS by coalesced loads.  Every
// grad_in element is stored exactly once, rounded once for the 16-bit types (no
// memset, no workspace).
//
// Bounded work: a sampling grid of up to kAlignScan points per bin and axis is walked
// whole.  Larger grids occur only with adaptive sampling, where the bin size is
// positive and a sample's coordinate is a nondecreasing function of its index (every
// rounding is monotone), so the indices inside an interval are found by bisection on
// the exact fp32 coordinate; the exact test is then applied to each sample again.
//
// Pyramid (DESIGN.md §3 "Multi-scale RoIAlign"): roi_align_multi_fwd_kernel and
// roi_align_multi_bwd_tile_kernel run the same per-thread and per-wave work (align_fwd_bin,
// align_bwd_tile) over up to 8 maps in one launch each.  A RoI's level is the number of
// thresholds its fp32 sqrt(area) reaches; the forward takes the map of its RoI's level, the
// backward runs over the tiles of all levels and keeps the RoIs of its tile's level.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "common.h"
#include "elem16.h"

namespace frcnn {
namespace {

constexpr int kAlignMaxRatio = 16;         // largest sampling_ratio accepted
constexpr int kAlignScan = 16;             // grids up to this many points per axis are walked whole
constexpr float kAlignMaxCoord = 1048576;  // 2^20: a scaled coordinate beyond it guards the RoI
constexpr int kAlignTile = 8;              // backward: tile edge in pixels (one wave: 8 x 8 pixels x 64 channels)
constexpr int kAlignTileStride = 65;       // backward: words per pixel row of the LDS tile (64 channels + 1)
constexpr int kAlignWaves = 5;             // backward: waves (tiles) per workgroup (5 x 29,184 B of LDS)
constexpr int kAlignStageBins = 49;        // backward: a RoI's gradients are staged in LDS up to this many bins
constexpr int kAlignMaxDim = 1 << 24;      // H, W must be exact in fp32
constexpr int kAlignRun = 8;               // forward: channels per thread
constexpr int kAlignMaxLevels = 8;         // pyramid: most levels in one call
constexpr int kAlignLaneSamples = 64;      // backward: up to this many samples per axis go one per lane

struct AlignGeom {
    float sh, sw, bh, bw, count;
    int gh, gw, b;
    bool ok;  // false: guarded RoI (all-zero output, no gradient)
};

__device__ __forceinline__ bool align_coord_ok(float v) { return fabsf(v) <= kAlignMaxCoord; }  // false for NaN, inf

__device__ __forceinline__ AlignGeom align_geom(const float* __restrict__ roi, int N, int PH, int PW, float scale,
                                                int sampling_ratio, bool aligned) {
    AlignGeom g;
    const float bf = roi[0];
    const float x1 = roi[1] * scale, y1 = roi[2] * scale, x2 = roi[3] * scale, y2 = roi[4] * scale;
    g.ok = bf > -1.f && bf < static_cast<float>(N) && align_coord_ok(x1) && align_coord_ok(y1) &&
           align_coord_ok(x2) && align_coord_ok(y2);
    g.b = g.ok ? static_cast<int>(bf) : 0;
    const float off = aligned ? 0.5f : 0.f;
    g.sw = x1 - off;
    g.sh = y1 - off;
    const float ew = x2 - off, eh = y2 - off;
    float rw = ew - g.sw, rh = eh - g.sh;
    if (!aligned) {
        rw = rw < 1.f ? 1.f : rw;
        rh = rh < 1.f ? 1.f : rh;
    }
    g.bh = rh / static_cast<float>(PH);
    g.bw = rw / static_cast<float>(PW);
    g.gh = sampling_ratio > 0 ? sampling_ratio : static_cast<int>(ceilf(rh / static_cast<float>(PH)));
    g.gw = sampling_ratio > 0 ? sampling_ratio : static_cast<int>(ceilf(rw / static_cast<float>(PW)));
    if (!g.ok) g.gh = g.gw = 0;
    const int64_t cnt = static_cast<int64_t>(g.gh) * g.gw;
    g.count = static_cast<float>(cnt > 1 ? cnt : 1);
    return g;
}

// Coordinate of sample i of a bin: base = start + p * bin, gf = (float)grid.
__device__ __forceinline__ float align_pos(float base, float bin, float gf, int i) {
    return base + ((static_cast<float>(i) + 0.5f) * bin) / gf;
}

__device__ __forceinline__ bool align_below(float v, float hi, bool hi_incl) { return v < hi || (hi_incl && v == hi); }

// [a, e): a range of sample indices of one bin that holds every i in [0, g) with
// lo <= pos(i) and (pos(i) < hi, or pos(i) <= hi with hi_incl).  Empty: a >= e.
__device__ __forceinline__ void align_range(float base, float bin, int g, float lo, float hi, bool hi_incl, int& a,
                                            int& e) {
    const float gf = static_cast<float>(g);
    if (g <= kAlignScan) {
        a = g > 0 ? g : 0;  // g <= 0 (a negative box under `aligned`): no samples
        e = 0;
        for (int i = 0; i < g; ++i) {
            const float v = align_pos(base, bin, gf, i);
            if (v >= lo && align_below(v, hi, hi_incl)) {
                a = i < a ? i : a;
                e = i + 1;
            }
        }
        return;
    }
    // an adaptive grid: bin > 0 and pos is nondecreasing in i
    int l = 0, r = g;  // first i with pos(i) >= lo
    while (l < r) {
        const int m = l + (r - l) / 2;
        if (align_pos(base, bin, gf, m) >= lo) r = m; else l = m + 1;
    }
    a = l;
    r = g;  // first i >= a that is no longer below hi
    while (l < r) {
        const int m = l + (r - l) / 2;
        if (align_below(align_pos(base, bin, gf, m), hi, hi_incl)) l = m + 1; else r = m;
    }
    e = l;
}

// The two pixels and weights of an inside coordinate along an axis of `size` pixels.
__device__ __forceinline__ void align_axis(float v, int size, int& lo, int& hi, float& l, float& h) {
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

// The forward's work of one thread: bin (ph, pw) of RoI n for the channels [c0, c0 + kAlignRun)
// of the map x [N,C,H,W] (the geometry is theirs in common).  Shared by the single-map and the
// pyramid kernel, which differ only in where x, H, W and scale come from.
template <class E>
__device__ __forceinline__ void align_fwd_bin(const typename E::raw* __restrict__ x, const float* __restrict__ rois,
                                              int64_t n, int c0, int ph, int pw, int N, int C, int H, int W, int PH,
                                              int PW, float scale, int sampling_ratio, int aligned,
                                              typename E::raw* __restrict__ out) {
    constexpr int CH = kAlignRun;
    const int nc = C - c0 < CH ? C - c0 : CH;
    const size_t PHW = static_cast<size_t>(PH) * PW, HW = static_cast<size_t>(H) * W;
    typename E::raw* o = out + (static_cast<size_t>(n) * C + c0) * PHW + static_cast<size_t>(ph) * PW + pw;
    const AlignGeom g = align_geom(rois + n * 5, N, PH, PW, scale, sampling_ratio, aligned != 0);
    if (!g.ok) {
        for (int j = 0; j < nc; ++j) o[j * PHW] = E::narrow(0.f);
        return;
    }
    const typename E::raw* plane = x + (static_cast<size_t>(g.b) * C + c0) * HW;
    const float fH = static_cast<float>(H), fW = static_cast<float>(W);
    const float basey = g.sh + static_cast<float>(ph) * g.bh, basex = g.sw + static_cast<float>(pw) * g.bw;
    const float gfh = static_cast<float>(g.gh), gfw = static_cast<float>(g.gw);
    int ya = 0, ye = g.gh, xa = 0, xe = g.gw;
    if (g.gh > kAlignScan) align_range(basey, g.bh, g.gh, -1.f, fH, true, ya, ye);
    if (g.gw > kAlignScan) align_range(basex, g.bw, g.gw, -1.f, fW, true, xa, xe);
    float acc[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) acc[j] = 0.f;
    for (int iy = ya; iy < ye; ++iy) {
        const float y = align_pos(basey, g.bh, gfh, iy);
        if (y < -1.f || y > fH) continue;
        int yl, yh;
        float ly, hy;
        align_axis(y, H, yl, yh, ly, hy);
        const typename E::raw* rl = plane + static_cast<size_t>(yl) * W;
        const typename E::raw* rh = plane + static_cast<size_t>(yh) * W;
        for (int ix = xa; ix < xe; ++ix) {
            const float xx = align_pos(basex, g.bw, gfw, ix);
            if (xx < -1.f || xx > fW) continue;
            int xl, xh;
            float lx, hx;
            align_axis(xx, W, xl, xh, lx, hx);
            const float w1 = hy * hx, w2 = hy * lx, w3 = ly * hx, w4 = ly * lx;
#pragma unroll
            for (int j = 0; j < CH; ++j) {
                if (j < nc) {
                    const size_t po = j * HW;
                    const float v1 = E::widen(rl[po + xl]), v2 = E::widen(rl[po + xh]);
                    const float v3 = E::widen(rh[po + xl]), v4 = E::widen(rh[po + xh]);
                    const float val = ((w1 * v1 + w2 * v2) + w3 * v3) + w4 * v4;
                    acc[j] = acc[j] + val;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < CH; ++j)
        if (j < nc) o[j * PHW] = E::narrow(acc[j] / g.count);
}

template <class E>
__global__ __launch_bounds__(256) void roi_align_fwd_kernel(const typename E::raw* __restrict__ x,
                                                            const float* __restrict__ rois, int64_t total, int N,
                                                            int C, int H, int W, int PH, int PW, float scale,
                                                            int sampling_ratio, int aligned,
                                                            typename E::raw* __restrict__ out) {
    // one thread: one bin of one RoI for a run of kAlignRun channels
    constexpr int CH = kAlignRun;
    const int64_t idx = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (idx >= total) return;
    const int runs = (C + CH - 1) / CH;
    const int pw = static_cast<int>(idx % PW);
    const int ph = static_cast<int>((idx / PW) % PH);
    const int c0 = static_cast<int>((idx / PW / PH) % runs) * CH;
    const int64_t n = idx / PW / PH / runs;
    align_fwd_bin<E>(x, rois, n, c0, ph, pw, N, C, H, W, PH, PW, scale, sampling_ratio, aligned, out);
}

// ------------------------------------------------- pyramid (DESIGN.md §3 "Multi-scale RoIAlign")
// The levels of a call, by value in the kernel arguments.  Every index into the arrays is a
// constant after unrolling, so the table stays in the argument segment (scalar loads, no scratch).
struct AlignLevels {
    const void* p[kAlignMaxLevels];  // forward: x_l; backward: grad_in_l
    int H[kAlignMaxLevels], W[kAlignMaxLevels];
    float scale[kAlignMaxLevels];
    float thr[kAlignMaxLevels];  // thr[k - 1] = t_k for k in [1, n); ascending, none NaN
    int n;
};

// The backward's tile space: level l owns the units [first[l], first[l + 1]).
struct AlignTilePlan {
    int64_t first[kAlignMaxLevels + 1];
    int tiles_x[kAlignMaxLevels], tiles[kAlignMaxLevels];
};

// #{k : sqrt(area) >= t_k}; a NaN root (a NaN coordinate, a negative area) compares false: level 0.
__device__ __forceinline__ int align_level(const float* __restrict__ roi, const AlignLevels& lv) {
    const float w = roi[3] - roi[1], h = roi[4] - roi[2];
    const float s = sqrtf(w * h);  // correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt)
    int l = 0;
#pragma unroll
    for (int k = 0; k < kAlignMaxLevels - 1; ++k) l += (k < lv.n - 1 && s >= lv.thr[k]) ? 1 : 0;
    return l;
}

// A level's entry as the kernels index it: in LDS.  (Indexed by a run-time level the by-value
// table would be copied to scratch, a chain of selects over it included: the compiler folds the
// chain back into an indexed load.)  One thread copies it with constant indices, i.e. scalar
// loads from the argument segment; the caller's barrier publishes it.
struct AlignLevelView {
    const void* p;
    int H, W;
    float scale;
};

__device__ __forceinline__ void align_publish(const AlignLevels& lv, AlignLevelView* tab) {
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kAlignMaxLevels; ++k) tab[k] = AlignLevelView{lv.p[k], lv.H[k], lv.W[k], lv.scale[k]};
    }
}

// Entry l of the published table for a wave-uniform l, in scalar registers.
__device__ __forceinline__ AlignLevelView align_view_uniform(const AlignLevelView* tab, int l) {
    const AlignLevelView t = tab[l];
    const uint64_t p = reinterpret_cast<uint64_t>(t.p);
    const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(p));
    const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(p >> 32));
    return AlignLevelView{reinterpret_cast<const void*>((static_cast<uint64_t>(hi) << 32) | lo),
                          __builtin_amdgcn_readfirstlane(t.H), __builtin_amdgcn_readfirstlane(t.W),
                          __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(t.scale)))};
}

template <class E>
__global__ __launch_bounds__(256) void roi_align_multi_fwd_kernel(AlignLevels lv, const float* __restrict__ rois,
                                                                  int64_t total, int N, int C, int runs, int PH,
                                                                  int PW, int sampling_ratio, int aligned,
                                                                  typename E::raw* __restrict__ out,
                                                                  int* __restrict__ levels) {
    // roi_align_fwd_kernel's thread mapping; each thread pools from the map of its RoI's level
    constexpr int CH = kAlignRun;
    __shared__ AlignLevelView tab[kAlignMaxLevels];
    align_publish(lv, tab);
    __syncthreads();
    const int64_t idx = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (idx >= total) return;
    const int pw = static_cast<int>(idx % PW);
    const int ph = static_cast<int>((idx / PW) % PH);
    const int c0 = static_cast<int>((idx / PW / PH) % runs) * CH;  // runs >= 1 also for C == 0 (levels only)
    const int64_t n = idx / PW / PH / runs;
    const int l = align_level(rois + n * 5, lv);
    if (levels && c0 == 0 && ph == 0 && pw == 0) levels[n] = l;
    const AlignLevelView v = tab[l];  // l < lv.n <= kAlignMaxLevels
    // a level without pixels guards all its RoIs: zeros, nothing read
    const int n_img = v.H > 0 && v.W > 0 ? N : 0;
    align_fwd_bin<E>(static_cast<const typename E::raw*>(v.p), rois, n, c0, ph, pw, n_img, C, v.H, v.W, PH, PW,
                     v.scale, sampling_ratio, aligned, out);
}

// The four additions of one sample into the tile (al / ah: the rows of yl / yh at this
// lane's channel; ol / oh: the offsets of xl / xh), in the contract's order.
__device__ __forceinline__ void align_add4(float* al, float* ah, int ol, int oh, bool in_yl, bool in_yh, bool in_xl,
                                           bool in_xh, bool four_pixels, float gv, float w1, float w2, float w3,
                                           float w4, bool pow2, float inv, float count) {
    float q1, q2, q3, q4;
    if (pow2) {  // x * 2^-k and x / 2^k round the same real number: the same bits
        q1 = (gv * w1) * inv, q2 = (gv * w2) * inv, q3 = (gv * w3) * inv, q4 = (gv * w4) * inv;
    } else {
        q1 = (gv * w1) / count, q2 = (gv * w2) / count, q3 = (gv * w3) / count, q4 = (gv * w4) / count;
    }
    if (in_yl && in_yh && in_xl && in_xh && four_pixels) {
        // four different words: read them together, no add waits for another
        const float s1 = al[ol], s2 = al[oh], s3 = ah[ol], s4 = ah[oh];
        al[ol] = s1 + q1;
        al[oh] = s2 + q2;
        ah[ol] = s3 + q3;
        ah[oh] = s4 + q4;
    } else {  // clamped at the map's edge, or partly off the tile: one after the other
        if (in_yl && in_xl) al[ol] = al[ol] + q1;
        if (in_yl && in_xh) al[oh] = al[oh] + q2;
        if (in_yh && in_xl) ah[ol] = ah[ol] + q3;
        if (in_yh && in_xh) ah[oh] = ah[oh] + q4;
    }
}

__device__ __forceinline__ float align_bcast(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ int align_bcast(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
// bits [first, first + n) of m, moved down to bit 0 (first < 64, first + n <= 64)
__device__ __forceinline__ uint64_t align_bits(uint64_t m, int first, int n) {
    const uint64_t s = m >> first;
    return n >= 64 ? s : s & ((1ull << n) - 1ull);
}

// Which RoIs a backward wave sums: all of its image (one map), or those of its level too (pyramid).
struct AlignKeepAll {
    __device__ __forceinline__ bool operator()(const float*) const { return true; }
};
struct AlignKeepLevel {
    const AlignLevels& lv;
    int level;
    __device__ __forceinline__ bool operator()(const float* roi) const { return align_level(roi, lv) == level; }
};

// The backward's work of one wave: tile `unit` of the map [N,C,H,W] behind grad_in (`live`: the unit
// exists; a wave without one only joins the barrier).  Shared by the single-map and the pyramid kernel.
template <class E, int T, class Keep>
__device__ __forceinline__ void align_bwd_tile(const typename E::raw* __restrict__ grad,
                                               const float* __restrict__ rois, int R, int N, int C, int H, int W,
                                               int PH, int PW, float scale, int sampling_ratio, int aligned,
                                               int tiles_x, int tiles, int cgroups, int64_t unit, bool live,
                                               typename E::raw* __restrict__ grad_in, Keep keep) {
    static_assert(T * T == 64, "the write-out maps one lane to one pixel of the tile");
    extern __shared__ __attribute__((aligned(16))) float align_lds[];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    constexpr int kWaveWords = T * T * kAlignTileStride + 64 * kAlignStageBins;
    float* acc = align_lds + wid * kWaveWords;
    float* stage = acc + T * T * kAlignTileStride;  // [channel][bin], an odd stride: conflict-free either way
    for (int p = 0; p < T * T; ++p) acc[p * kAlignTileStride + lane] = 0.f;
    int b = 0, cg = 0, r0 = 0, c0 = 0, r1 = 0, c1 = 0;
    if (live) {
        const int tile = static_cast<int>(unit % tiles);
        cg = static_cast<int>((unit / tiles) % cgroups);
        b = static_cast<int>(unit / tiles / cgroups);
        r0 = (tile / tiles_x) * T;
        c0 = (tile % tiles_x) * T;
        r1 = r0 + T < H ? r0 + T : H;
        c1 = c0 + T < W ? c0 + T : W;
        const int c = cg * 64 + lane;
        const bool active = c < C;
        const float fH = static_cast<float>(H), fW = static_cast<float>(W);
        // a sample at v touches the pixels floor(v) and floor(v) + 1 (both clamped to the map)
        const float ylo = static_cast<float>(r0 - 1), yhi = static_cast<float>(r1);
        const float xlo = static_cast<float>(c0 - 1), xhi = static_cast<float>(c1);
        const bool yincl = r1 == H, xincl = c1 == W;
        const size_t PHW = static_cast<size_t>(PH) * PW;
        const bool staged = PHW <= kAlignStageBins;
        const int sstride = static_cast<int>(PHW) | 1, nch = C - cg * 64 < 64 ? C - cg * 64 : 64;
        for (int rbase = 0; rbase < R; rbase += 64) {
            const int r = rbase + lane;
            bool mine = false;
            if (r < R) {
                const AlignGeom gl = align_geom(rois + static_cast<size_t>(r) * 5, N, PH, PW, scale, sampling_ratio,
                                                aligned != 0);
                mine = gl.ok && gl.b == b && keep(rois + static_cast<size_t>(r) * 5);
            }
            uint64_t mask = __ballot(mine);
            while (mask) {
                const int j = __builtin_ctzll(mask);
                mask &= mask - 1;
                const int n = rbase + j;  // wave-uniform
                const AlignGeom g = align_geom(rois + static_cast<size_t>(n) * 5, N, PH, PW, scale, sampling_ratio,
                                               aligned != 0);
                const float gfh = static_cast<float>(g.gh), gfw = static_cast<float>(g.gw);
                const bool pow2 = (__float_as_uint(g.count) & 0x7fffffu) == 0;  // count = 2^k (1, 4, 16, ...)
                const float inv = 1.f / g.count;                                // exact then
                const typename E::raw* gp = grad + (static_cast<size_t>(n) * C + (active ? c : 0)) * PHW;
                // A touching RoI's gradients for the wave's channels are one contiguous block of
                // grad: copied to LDS with coalesced loads, widened, then read lane = channel.
                // (Read per bin straight from grad, every lane pulls a cache line of its own.)
                auto stage_in = [&]() {
                    if (!staged) return;
                    const typename E::raw* src = grad + (static_cast<size_t>(n) * C + static_cast<size_t>(cg) * 64) * PHW;
                    const int words = nch * static_cast<int>(PHW);
                    for (int i = lane; i < words; i += 64) {
                        const int ch = i / static_cast<int>(PHW);
                        stage[ch * sstride + (i - ch * static_cast<int>(PHW))] = E::widen(src[i]);
                    }
                    __builtin_amdgcn_wave_barrier();
                };
                auto grad_at = [&](int ph, int pw) -> float {
                    if (!active) return 0.f;
                    return staged ? stage[lane * sstride + ph * PW + pw] : E::widen(gp[static_cast<size_t>(ph) * PW + pw]);
                };
                constexpr int kLane = kAlignLaneSamples;
                if (g.gh > 0 && g.gw > 0 && g.gh <= kLane && g.gw <= kLane && PH <= kLane && PW <= kLane &&
                    PH * g.gh <= kLane && PW * g.gw <= kLane) {
                    // Up to 64 samples per axis (every fixed sampling_ratio at 7 x 7 up to 9): lane l works out
                    // sample l of each axis once, the walk below reads the values lane by lane.
                    int tyl = 0, tyh = 0, txl = 0, txh = 0;
                    float tly = 0.f, thy = 0.f, tlx = 0.f, thx = 0.f;
                    bool ty = false, tx = false;
                    if (lane < PH * g.gh) {
                        const int p = lane / g.gh;
                        const float y = align_pos(g.sh + static_cast<float>(p) * g.bh, g.bh, gfh, lane - p * g.gh);
                        if (!(y < -1.f || y > fH)) {
                            align_axis(y, H, tyl, tyh, tly, thy);
                            ty = (tyl >= r0 && tyl < r1) || (tyh >= r0 && tyh < r1);
                        }
                    }
                    if (lane < PW * g.gw) {
                        const int p = lane / g.gw;
                        const float xx = align_pos(g.sw + static_cast<float>(p) * g.bw, g.bw, gfw, lane - p * g.gw);
                        if (!(xx < -1.f || xx > fW)) {
                            align_axis(xx, W, txl, txh, tlx, thx);
                            tx = (txl >= c0 && txl < c1) || (txh >= c0 && txh < c1);
                        }
                    }
                    const uint64_t ymask = __ballot(ty), xmask = __ballot(tx);  // the samples that reach the tile
                    if (!ymask || !xmask) continue;
                    const int pha = __builtin_ctzll(ymask) / g.gh, phe = (63 - __builtin_clzll(ymask)) / g.gh + 1;
                    const int pwa = __builtin_ctzll(xmask) / g.gw, pwe = (63 - __builtin_clzll(xmask)) / g.gw + 1;
                    stage_in();
                    for (int ph = pha; ph < phe; ++ph) {
                        const uint64_t by = align_bits(ymask, ph * g.gh, g.gh);
                        if (!by) continue;
                        for (int pw = pwa; pw < pwe; ++pw) {
                            const uint64_t bx = align_bits(xmask, pw * g.gw, g.gw);
                            if (!bx) continue;
                            const float gv = grad_at(ph, pw);
                            for (uint64_t my = by; my; my &= my - 1) {
                                const int sy = ph * g.gh + __builtin_ctzll(my);
                                const int yl = align_bcast(tyl, sy), yh = align_bcast(tyh, sy);
                                const float ly = align_bcast(tly, sy), hy = align_bcast(thy, sy);
                                const bool in_yl = yl >= r0 && yl < r1, in_yh = yh >= r0 && yh < r1;
                                float* al = acc + (yl - r0) * T * kAlignTileStride + lane;
                                float* ah = acc + (yh - r0) * T * kAlignTileStride + lane;
                                for (uint64_t mx = bx; mx; mx &= mx - 1) {
                                    const int sx = pw * g.gw + __builtin_ctzll(mx);
                                    const int xl = align_bcast(txl, sx), xh = align_bcast(txh, sx);
                                    const float lx = align_bcast(tlx, sx), hx = align_bcast(thx, sx);
                                    const bool in_xl = xl >= c0 && xl < c1, in_xh = xh >= c0 && xh < c1;
                                    const float w1 = hy * hx, w2 = hy * lx, w3 = ly * hx, w4 = ly * lx;
                                    const int ol = (xl - c0) * kAlignTileStride, oh = (xh - c0) * kAlignTileStride;
                                    align_add4(al, ah, ol, oh, in_yl, in_yh, in_xl, in_xh, yl != yh && xl != xh, gv,
                                               w1, w2, w3, w4, pow2, inv, g.count);
                                }
                            }
                        }
                    }
                    continue;
                }
                // the bins that can touch the tile: a box [pha, phe) x [pwa, pwe) around them
                int pha = PH, phe = 0, pwa = PW, pwe = 0, ya, ye, xa, xe;
                for (int ph = 0; ph < PH; ++ph) {
                    align_range(g.sh + static_cast<float>(ph) * g.bh, g.bh, g.gh, ylo, yhi, yincl, ya, ye);
                    if (ya < ye) {
                        pha = ph < pha ? ph : pha;
                        phe = ph + 1;
                    }
                }
                if (pha >= phe) continue;
                for (int pw = 0; pw < PW; ++pw) {
                    align_range(g.sw + static_cast<float>(pw) * g.bw, g.bw, g.gw, xlo, xhi, xincl, xa, xe);
                    if (xa < xe) {
                        pwa = pw < pwa ? pw : pwa;
                        pwe = pw + 1;
                    }
                }
                if (pwa >= pwe) continue;
                stage_in();
                for (int ph = pha; ph < phe; ++ph) {
                    const float basey = g.sh + static_cast<float>(ph) * g.bh;
                    align_range(basey, g.bh, g.gh, ylo, yhi, yincl, ya, ye);
                    if (ya >= ye) continue;
                    for (int pw = pwa; pw < pwe; ++pw) {
                        const float basex = g.sw + static_cast<float>(pw) * g.bw;
                        align_range(basex, g.bw, g.gw, xlo, xhi, xincl, xa, xe);
                        if (xa >= xe) continue;
                        const float gv = grad_at(ph, pw);
                        for (int iy = ya; iy < ye; ++iy) {
                            const float y = align_pos(basey, g.bh, gfh, iy);
                            if (y < -1.f || y > fH) continue;
                            int yl, yh;
                            float ly, hy;
                            align_axis(y, H, yl, yh, ly, hy);
                            const bool in_yl = yl >= r0 && yl < r1, in_yh = yh >= r0 && yh < r1;
                            if (!in_yl && !in_yh) continue;
                            float* al = acc + (yl - r0) * T * kAlignTileStride + lane;
                            float* ah = acc + (yh - r0) * T * kAlignTileStride + lane;
                            for (int ix = xa; ix < xe; ++ix) {
                                const float xx = align_pos(basex, g.bw, gfw, ix);
                                if (xx < -1.f || xx > fW) continue;
                                int xl, xh;
                                float lx, hx;
                                align_axis(xx, W, xl, xh, lx, hx);
                                const bool in_xl = xl >= c0 && xl < c1, in_xh = xh >= c0 && xh < c1;
                                if (!in_xl && !in_xh) continue;
                                const float w1 = hy * hx, w2 = hy * lx, w3 = ly * hx, w4 = ly * lx;
                                const int ol = (xl - c0) * kAlignTileStride, oh = (xh - c0) * kAlignTileStride;
                                align_add4(al, ah, ol, oh, in_yl, in_yh, in_xl, in_xh, yl != yh && xl != xh, gv, w1,
                                           w2, w3, w4, pow2, inv, g.count);
                            }
                        }
                    }
                }
            }
        }
    }
    __syncthreads();  // the wave's sums are complete in LDS; lanes now read other lanes' words
    if (!live) return;
    const int py = lane / T, px = lane % T;
    if (r0 + py < r1 && c0 + px < c1) {
        const int nc = C - cg * 64 < 64 ? C - cg * 64 : 64;
        const size_t HW = static_cast<size_t>(H) * W;
        typename E::raw* dst = grad_in + (static_cast<size_t>(b) * C + static_cast<size_t>(cg) * 64) * HW +
                               static_cast<size_t>(r0 + py) * W + (c0 + px);
        const float* src = acc + lane * kAlignTileStride;
        for (int ci = 0; ci < nc; ++ci) dst[static_cast<size_t>(ci) * HW] = E::narrow(src[ci]);
    }
}

template <class E, int T>
__global__ __launch_bounds__(64 * kAlignWaves) void roi_align_bwd_tile_kernel(
    const typename E::raw* __restrict__ grad, const float* __restrict__ rois, int R, int N, int C, int H, int W, int PH,
    int PW, float scale, int sampling_ratio, int aligned, int tiles_x, int tiles, int cgroups, int64_t units,
    typename E::raw* __restrict__ grad_in) {
    const int64_t unit = static_cast<int64_t>(blockIdx.x) * kAlignWaves + (threadIdx.x >> 6);
    align_bwd_tile<E, T>(grad, rois, R, N, C, H, W, PH, PW, scale, sampling_ratio, aligned, tiles_x, tiles, cgroups,
                         unit, unit < units, grad_in, AlignKeepAll{});
}

// One launch over the tiles of every level, level after level: a wave finds its level from the
// prefix table, then runs the single-map walk on that level's geometry and RoIs.  A workgroup's
// waves may belong to different levels; each has its own LDS and they meet only at the barrier.
template <class E, int T>
__global__ __launch_bounds__(64 * kAlignWaves) void roi_align_multi_bwd_tile_kernel(
    const typename E::raw* __restrict__ grad, const float* __restrict__ rois, int R, int N, int C, int PH, int PW,
    int sampling_ratio, int aligned, int cgroups, int64_t units, AlignLevels lv, AlignTilePlan plan) {
    __shared__ AlignLevelView tab[kAlignMaxLevels];
    __shared__ int64_t tab_first[kAlignMaxLevels];
    __shared__ int tab_tiles_x[kAlignMaxLevels], tab_tiles[kAlignMaxLevels];
    align_publish(lv, tab);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kAlignMaxLevels; ++k)
            tab_first[k] = plan.first[k], tab_tiles_x[k] = plan.tiles_x[k], tab_tiles[k] = plan.tiles[k];
    }
    __syncthreads();
    const int64_t unit = static_cast<int64_t>(blockIdx.x) * kAlignWaves + (threadIdx.x >> 6);
    int l = 0;
#pragma unroll
    for (int k = 1; k < kAlignMaxLevels; ++k) l += (k < lv.n && unit >= plan.first[k]) ? 1 : 0;
    l = __builtin_amdgcn_readfirstlane(l);  // the same in every lane of the wave; l < lv.n <= kAlignMaxLevels
    const AlignLevelView v = align_view_uniform(tab, l);
    const int64_t first = tab_first[l];
    const int tiles_x = __builtin_amdgcn_readfirstlane(tab_tiles_x[l]);
    const int tiles = __builtin_amdgcn_readfirstlane(tab_tiles[l]);
    // a unit past the last one lands on the last level with tiles to spare; it is not live
    align_bwd_tile<E, T>(grad, rois, R, N, C, v.H, v.W, PH, PW, v.scale, sampling_ratio, aligned, tiles_x, tiles,
                         cgroups, unit - first, unit < units,
                         static_cast<typename E::raw*>(const_cast<void*>(v.p)), AlignKeepLevel{lv, l});
}

const char* align_elem_name(int dtype) {
    return dtype == FRCNN_F16 ? "ElemF16" : dtype == FRCNN_BF16 ? "ElemBF16" : "ElemF32";
}

// Argument checks shared by the two entry points and the name queries: everything
// that can be refused is refused here, before any HIP call.
int align_check(const char* fn, int dtype, int64_t R, int N, int C, int H, int W, int PH, int PW,
                int sampling_ratio) {
    FRCNN_REQUIRE(dtype_code_ok(dtype), "%s: dtype code %d is not FRCNN_F32, FRCNN_F16 or FRCNN_BF16", fn, dtype);
    FRCNN_REQUIRE(PH >= 1 && PW >= 1, "%s: bad output_size (%d, %d)", fn, PH, PW);
    FRCNN_REQUIRE(sampling_ratio <= kAlignMaxRatio, "%s: sampling_ratio %d > %d", fn, sampling_ratio, kAlignMaxRatio);
    FRCNN_REQUIRE(R >= 0 && N >= 0 && C >= 0 && H >= 0 && W >= 0, "%s: bad shape", fn);
    FRCNN_REQUIRE(R <= 0x7fffffff, "%s: too many rois", fn);
    FRCNN_REQUIRE(H <= kAlignMaxDim && W <= kAlignMaxDim && N <= kAlignMaxDim, "%s: N, H, W must be <= 2^24", fn);
    return FRCNN_OK;
}

// The launch numbers of both directions, from the shape alone.  The launches below and
// frcnn_roi_align_plan / frcnn_roi_align_multi_plan all read them from here.
struct AlignFwdPlan {
    int runs;             // runs of kAlignRun channels per bin
    int64_t total, grid;  // threads, workgroups of 256
};

AlignFwdPlan align_fwd_plan(int64_t R, int C, int PH, int PW, bool levels_only_row) {
    AlignFwdPlan p;
    p.runs = (C + kAlignRun - 1) / kAlignRun;
    if (levels_only_row && C == 0) p.runs = 1;  // pyramid, C == 0: one thread row, for `levels`
    p.total = R * p.runs * PH * PW;
    p.grid = (p.total + 255) / 256;
    return p;
}

struct AlignBwdPlan {
    int tiles_x, tiles_y, cgroups, idle;  // idle: waves of the last workgroup without a unit
    int64_t tiles, units, blocks;
    size_t lds;
    bool staged;
};

constexpr size_t kAlignBwdLds =
    sizeof(float) * kAlignWaves * (kAlignTile * kAlignTile * kAlignTileStride + 64 * kAlignStageBins);

// One map's tile grid; `units` and what follows from it are the caller's (the pyramid sums levels).
void align_tile_grid(int H, int W, AlignBwdPlan& p) {
    p.tiles_x = (W + kAlignTile - 1) / kAlignTile;
    p.tiles_y = (H + kAlignTile - 1) / kAlignTile;
    p.tiles = static_cast<int64_t>(p.tiles_x) * p.tiles_y;
}

void align_units(int64_t units, int PH, int PW, AlignBwdPlan& p) {
    p.units = units;
    p.blocks = (units + kAlignWaves - 1) / kAlignWaves;
    p.idle = static_cast<int>(p.blocks * kAlignWaves - units);
    p.lds = kAlignBwdLds;
    p.staged = static_cast<int64_t>(PH) * PW <= kAlignStageBins;
}

int align_bwd_plan(const char* fn, int N, int C, int H, int W, int PH, int PW, AlignBwdPlan& p) {
    align_tile_grid(H, W, p);
    p.cgroups = (C + 63) / 64;
    align_units(p.tiles * p.cgroups * N, PH, PW, p);
    FRCNN_REQUIRE(p.tiles <= 0x7fffffff && p.blocks <= 0x7fffffff, "%s: map too large (%lld tiles)", fn,
                  static_cast<long long>(p.units));
    return FRCNN_OK;
}

template <class E>
int align_fwd_launch(const void* x, const float* rois, int64_t R, int N, int C, int H, int W, int PH, int PW,
                     float scale, int sampling_ratio, int aligned, void* out, hipStream_t st) {
    using raw = typename E::raw;
    const AlignFwdPlan p = align_fwd_plan(R, C, PH, PW, false);
    hipLaunchKernelGGL(roi_align_fwd_kernel<E>, dim3(static_cast<unsigned>(p.grid)), dim3(256), 0, st,
                       static_cast<const raw*>(x), rois, p.total, N, C, H, W, PH, PW, scale, sampling_ratio, aligned,
                       static_cast<raw*>(out));
    return check_launch("roi_align_fwd_kernel");
}

template <class E>
int align_bwd_launch(const void* grad, const float* rois, int R, int N, int C, int H, int W, int PH, int PW,
                     float scale, int sampling_ratio, int aligned, void* grad_in, hipStream_t st) {
    using raw = typename E::raw;
    constexpr int T = kAlignTile;
    AlignBwdPlan p;
    if (int rc = align_bwd_plan("frcnn_roi_align_bwd_t", N, C, H, W, PH, PW, p)) return rc;
    hipLaunchKernelGGL((roi_align_bwd_tile_kernel<E, T>), dim3(static_cast<unsigned>(p.blocks)),
                       dim3(64 * kAlignWaves), p.lds, st, static_cast<const raw*>(grad), rois, R, N, C, H, W, PH, PW,
                       scale, sampling_ratio, aligned, p.tiles_x, static_cast<int>(p.tiles), p.cgroups, p.units,
                       static_cast<raw*>(grad_in));
    return check_launch("roi_align_bwd_tile_kernel");
}

// The pyramid calls' argument checks and level table, before any HIP call.  `p` may be null
// (the name queries); a level's pointer is needed only where the level has elements.
int align_levels(const char* fn, int dtype, int n_levels, const void* const* p, const int* H, const int* W,
                 const float* scales, const float* thresholds, int64_t R, int N, int C, int PH, int PW,
                 int sampling_ratio, AlignLevels& lv) {
    FRCNN_REQUIRE(n_levels >= 1 && n_levels <= kAlignMaxLevels, "%s: n_levels %d is not in [1, %d]", fn, n_levels,
                  kAlignMaxLevels);
    FRCNN_REQUIRE(H && W && scales, "%s: null %s", fn, !H ? "H" : !W ? "W" : "spatial_scales");
    FRCNN_REQUIRE(n_levels == 1 || thresholds, "%s: null thresholds", fn);
    std::memset(&lv, 0, sizeof(lv));
    lv.n = n_levels;
    for (int l = 0; l < n_levels; ++l) {
        if (int rc = align_check(fn, dtype, R, N, C, H[l], W[l], PH, PW, sampling_ratio)) return rc;
        lv.p[l] = p ? p[l] : nullptr;
        lv.H[l] = H[l];
        lv.W[l] = W[l];
        lv.scale[l] = scales[l];
    }
    for (int k = 0; k + 1 < n_levels; ++k) {
        const float t = thresholds[k];
        FRCNN_REQUIRE(t == t, "%s: thresholds[%d] is NaN", fn, k);
        FRCNN_REQUIRE(k == 0 || t >= thresholds[k - 1], "%s: thresholds[%d] = %g is below thresholds[%d] = %g", fn, k,
                      static_cast<double>(t), k - 1, static_cast<double>(thresholds[k - 1]));
        lv.thr[k] = t;
    }
    return FRCNN_OK;
}

template <class E>
int align_multi_fwd_launch(const AlignLevels& lv, const float* rois, int64_t R, int N, int C, int PH, int PW,
                           int sampling_ratio, int aligned, void* out, int* levels, hipStream_t st) {
    using raw = typename E::raw;
    const AlignFwdPlan p = align_fwd_plan(R, C, PH, PW, true);
    hipLaunchKernelGGL(roi_align_multi_fwd_kernel<E>, dim3(static_cast<unsigned>(p.grid)), dim3(256), 0, st, lv, rois,
                       p.total, N, C, p.runs, PH, PW, sampling_ratio, aligned, static_cast<raw*>(out), levels);
    return check_launch("roi_align_multi_fwd_kernel");
}

// The pyramid backward's tile space and launch numbers (level l owns [first[l], first[l + 1])).
int align_multi_bwd_plan(const char* fn, int n_levels, const int* H, const int* W, int N, int C, int PH, int PW,
                         AlignTilePlan& plan, AlignBwdPlan& p) {
    std::memset(&plan, 0, sizeof(plan));
    p.tiles_x = p.tiles_y = 0;
    p.tiles = 0;
    p.cgroups = (C + 63) / 64;
    int64_t units = 0;
    for (int l = 0; l < kAlignMaxLevels; ++l) {
        plan.first[l] = units;
        if (l >= n_levels) continue;
        AlignBwdPlan g;
        align_tile_grid(H[l], W[l], g);
        FRCNN_REQUIRE(g.tiles <= 0x7fffffff, "%s: level %d too large (%lld tiles)", fn, l,
                      static_cast<long long>(g.tiles));
        plan.tiles_x[l] = g.tiles_x;
        plan.tiles[l] = static_cast<int>(g.tiles);
        units += g.tiles * p.cgroups * N;
    }
    plan.first[kAlignMaxLevels] = units;
    align_units(units, PH, PW, p);
    FRCNN_REQUIRE(p.blocks <= 0x7fffffff, "%s: maps too large (%lld tiles)", fn, static_cast<long long>(units));
    return FRCNN_OK;
}

template <class E>
int align_multi_bwd_launch(const AlignLevels& lv, const void* grad, const float* rois, int R, int N, int C, int PH,
                           int PW, int sampling_ratio, int aligned, hipStream_t st) {
    using raw = typename E::raw;
    constexpr int T = kAlignTile;
    AlignTilePlan plan;
    AlignBwdPlan p;
    if (int rc = align_multi_bwd_plan("frcnn_roi_align_multi_bwd_t", lv.n, lv.H, lv.W, N, C, PH, PW, plan, p)) return rc;
    if (p.units == 0) return FRCNN_OK;
    hipLaunchKernelGGL((roi_align_multi_bwd_tile_kernel<E, T>), dim3(static_cast<unsigned>(p.blocks)),
                       dim3(64 * kAlignWaves), p.lds, st, static_cast<const raw*>(grad), rois, R, N, C, PH, PW,
                       sampling_ratio, aligned, p.cgroups, p.units, lv, plan);
    return check_launch("roi_align_multi_bwd_tile_kernel");
}

}  // namespace
}  // namespace frcnn

using namespace frcnn;

extern "C" size_t frcnn_roi_align_fwd_workspace_size(int64_t R, int N, int C) {
    if (R < 0 || N < 0 || C < 0) return 0;
    return 256;  // nothing is kept between launches: nominal, the buffer is not touched
}

extern "C" size_t frcnn_roi_align_bwd_workspace_size(int64_t R, int N, int PH, int PW) {
    if (R < 0 || N < 0 || PH <= 0 || PW <= 0) return 0;
    return 256;  // as above
}

extern "C" int frcnn_roi_align_fwd_t(int dtype, const void* x, const float* rois, int64_t R, int N, int C, int H,
                                     int W, int PH, int PW, float spatial_scale, int sampling_ratio, int aligned,
                                     void* out, void* workspace, size_t ws_bytes, void* stream) {
    (void)workspace;
    (void)ws_bytes;
    const char* fn = "frcnn_roi_align_fwd_t";
    if (int rc = align_check(fn, dtype, R, N, C, H, W, PH, PW, sampling_ratio)) return rc;
    const int64_t per_roi = static_cast<int64_t>(C) * PH * PW;
    FRCNN_REQUIRE(per_roi == 0 || R <= (int64_t{1} << 38) / per_roi, "%s: output too large", fn);
    const int64_t total = R * per_roi;  // output elements
    if (total == 0) return FRCNN_OK;
    FRCNN_REQUIRE(rois, "%s: null rois", fn);
    FRCNN_REQUIRE(out, "%s: null out", fn);
    hipStream_t st = as_stream(stream);
    if (N == 0 || H == 0 || W == 0) {  // no pixel to sample: every output is +0 (all bits zero in each type)
        if (hipMemsetAsync(out, 0, static_cast<size_t>(total) * (dtype == FRCNN_F32 ? 4 : 2), st) != hipSuccess)
            return check_launch("frcnn_roi_align_fwd_t memset");
        return FRCNN_OK;
    }
    FRCNN_REQUIRE(x, "%s: null x", fn);
    if (dtype == FRCNN_F16)
        return align_fwd_launch<ElemF16>(x, rois, R, N, C, H, W, PH, PW, spatial_scale, sampling_ratio, aligned,
                                         out, st);
    if (dtype == FRCNN_BF16)
        return align_fwd_launch<ElemBF16>(x, rois, R, N, C, H, W, PH, PW, spatial_scale, sampling_ratio, aligned,
                                          out, st);
    return align_fwd_launch<ElemF32>(x, rois, R, N, C, H, W, PH, PW, spatial_scale, sampling_ratio, aligned, out,
                                     st);
}

extern "C" int frcnn_roi_align_bwd_t(int dtype, const void* grad, const float* rois, int64_t R, int N, int C, int H,
                                     int W, int PH, int PW, float spatial_scale, int sampling_ratio, int aligned,
                                     void* grad_in, void* workspace, size_t ws_bytes, void* stream) {
    (void)workspace;
    (void)ws_bytes;
    const char* fn = "frcnn_roi_align_bwd_t";
    if (int rc = align_check(fn, dtype, R, N, C, H, W, PH, PW, sampling_ratio)) return rc;
    if (N == 0 || C == 0 || H == 0 || W == 0) return FRCNN_OK;
    FRCNN_REQUIRE(grad_in, "%s: null grad_in", fn);
    FRCNN_REQUIRE(R == 0 || (grad && rois), "%s: null %s", fn, grad ? "rois" : "grad");
    hipStream_t st = as_stream(stream);
    const int r = static_cast<int>(R);
    if (dtype == FRCNN_F16)
        return align_bwd_launch<ElemF16>(grad, rois, r, N, C, H, W, PH, PW, spatial_scale, sampling_ratio, aligned,
                                         grad_in, st);
    if (dtype == FRCNN_BF16)
        return align_bwd_launch<ElemBF16>(grad, rois, r, N, C, H, W, PH, PW, spatial_scale, sampling_ratio, aligned,
                                          grad_in, st);
    return align_bwd_launch<ElemF32>(grad, rois, r, N, C, H, W, PH, PW, spatial_scale, sampling_ratio, aligned,
                                     grad_in, st);
}

extern "C" int frcnn_roi_align_fwd_kernel(int dtype, int64_t R, int N, int C, int H, int W, int PH, int PW,
                                          int sampling_ratio, char* name, size_t len) {
    const char* fn = "frcnn_roi_align_fwd_kernel";
    if (int rc = align_check(fn, dtype, R, N, C, H, W, PH, PW, sampling_ratio)) return rc;
    FRCNN_REQUIRE(name && len > 0, "%s: null name", fn);
    const int n = snprintf(name, len, "roi_align_fwd_kernel<%s>", align_elem_name(dtype));
    FRCNN_REQUIRE(n >= 0 && static_cast<size_t>(n) < len, "%s: name buffer of %zu bytes too small", fn, len);
    return FRCNN_OK;
}

extern "C" int frcnn_roi_align_bwd_kernel(int dtype, int64_t R, int N, int C, int H, int W, int PH, int PW,
                                          int sampling_ratio, char* name, size_t len) {
    const char* fn = "frcnn_roi_align_bwd_kernel";
    if (int rc = align_check(fn, dtype, R, N, C, H, W, PH, PW, sampling_ratio)) return rc;
    FRCNN_REQUIRE(name && len > 0, "%s: null name", fn);
    const int n = snprintf(name, len, "roi_align_bwd_tile_kernel<%s, %d>", align_elem_name(dtype), kAlignTile);
    FRCNN_REQUIRE(n >= 0 && static_cast<size_t>(n) < len, "%s: name buffer of %zu bytes too small", fn, len);
    return FRCNN_OK;
}

// ------------------------------------------------------------------ pyramid
extern "C" int frcnn_roi_align_multi_fwd_t(int dtype, int n_levels, const void* const* x, const int* H, const int* W,
                                           const float* spatial_scales, const float* thresholds, const float* rois,
                                           int64_t R, int N, int C, int PH, int PW, int sampling_ratio, int aligned,
                                           void* out, int* levels, void* workspace, size_t ws_bytes, void* stream) {
    (void)workspace;
    (void)ws_bytes;
    const char* fn = "frcnn_roi_align_multi_fwd_t";
    AlignLevels lv;
    FRCNN_REQUIRE(n_levels < 1 || n_levels > kAlignMaxLevels || x, "%s: null x", fn);
    if (int rc = align_levels(fn, dtype, n_levels, x, H, W, spatial_scales, thresholds, R, N, C, PH, PW,
                              sampling_ratio, lv))
        return rc;
    const int64_t per_roi = static_cast<int64_t>(C) * PH * PW;
    FRCNN_REQUIRE(R <= (int64_t{1} << 38) / (per_roi > 0 ? per_roi : int64_t{PH} * PW), "%s: output too large", fn);
    if (R == 0 || (per_roi == 0 && !levels)) return FRCNN_OK;
    FRCNN_REQUIRE(rois, "%s: null rois", fn);
    FRCNN_REQUIRE(out || per_roi == 0, "%s: null out", fn);
    for (int l = 0; l < n_levels; ++l)
        FRCNN_REQUIRE(lv.p[l] || N == 0 || C == 0 || lv.H[l] == 0 || lv.W[l] == 0, "%s: null x[%d]", fn, l);
    hipStream_t st = as_stream(stream);
    if (dtype == FRCNN_F16)
        return align_multi_fwd_launch<ElemF16>(lv, rois, R, N, C, PH, PW, sampling_ratio, aligned, out, levels, st);
    if (dtype == FRCNN_BF16)
        return align_multi_fwd_launch<ElemBF16>(lv, rois, R, N, C, PH, PW, sampling_ratio, aligned, out, levels, st);
    return align_multi_fwd_launch<ElemF32>(lv, rois, R, N, C, PH, PW, sampling_ratio, aligned, out, levels, st);
}

extern "C" int frcnn_roi_align_multi_bwd_t(int dtype, int n_levels, const void* grad, const int* H, const int* W,
                                           const float* spatial_scales, const float* thresholds, const float* rois,
                                           int64_t R, int N, int C, int PH, int PW, int sampling_ratio, int aligned,
                                           void* const* grad_in, void* workspace, size_t ws_bytes, void* stream) {
    (void)workspace;
    (void)ws_bytes;
    const char* fn = "frcnn_roi_align_multi_bwd_t";
    AlignLevels lv;
    FRCNN_REQUIRE(n_levels < 1 || n_levels > kAlignMaxLevels || grad_in, "%s: null grad_in", fn);
    if (int rc = align_levels(fn, dtype, n_levels, grad_in, H, W, spatial_scales, thresholds, R, N, C, PH, PW,
                              sampling_ratio, lv))
        return rc;
    if (N == 0 || C == 0) return FRCNN_OK;
    for (int l = 0; l < n_levels; ++l)
        FRCNN_REQUIRE(lv.p[l] || lv.H[l] == 0 || lv.W[l] == 0, "%s: null grad_in[%d]", fn, l);
    FRCNN_REQUIRE(R == 0 || (grad && rois), "%s: null %s", fn, grad ? "rois" : "grad");
    hipStream_t st = as_stream(stream);
    const int r = static_cast<int>(R);
    if (dtype == FRCNN_F16)
        return align_multi_bwd_launch<ElemF16>(lv, grad, rois, r, N, C, PH, PW, sampling_ratio, aligned, st);
    if (dtype == FRCNN_BF16)
        return align_multi_bwd_launch<ElemBF16>(lv, grad, rois, r, N, C, PH, PW, sampling_ratio, aligned, st);
    return align_multi_bwd_launch<ElemF32>(lv, grad, rois, r, N, C, PH, PW, sampling_ratio, aligned, st);
}

extern "C" int frcnn_roi_align_multi_fwd_kernel(int dtype, int n_levels, int64_t R, int N, int C, int PH, int PW,
                                                int sampling_ratio, char* name, size_t len) {
    const char* fn = "frcnn_roi_align_multi_fwd_kernel";
    FRCNN_REQUIRE(n_levels >= 1 && n_levels <= kAlignMaxLevels, "%s: n_levels %d is not in [1, %d]", fn, n_levels,
                  kAlignMaxLevels);
    if (int rc = align_check(fn, dtype, R, N, C, 0, 0, PH, PW, sampling_ratio)) return rc;
    FRCNN_REQUIRE(name && len > 0, "%s: null name", fn);
    const int n = snprintf(name, len, "roi_align_multi_fwd_kernel<%s>", align_elem_name(dtype));
    FRCNN_REQUIRE(n >= 0 && static_cast<size_t>(n) < len, "%s: name buffer of %zu bytes too small", fn, len);
    return FRCNN_OK;
}

extern "C" int frcnn_roi_align_multi_bwd_kernel(int dtype, int n_levels, int64_t R, int N, int C, int PH, int PW,
                                                int sampling_ratio, char* name, size_t len) {
    const char* fn = "frcnn_roi_align_multi_bwd_kernel";
    FRCNN_REQUIRE(n_levels >= 1 && n_levels <= kAlignMaxLevels, "%s: n_levels %d is not in [1, %d]", fn, n_levels,
                  kAlignMaxLevels);
    if (int rc = align_check(fn, dtype, R, N, C, 0, 0, PH, PW, sampling_ratio)) return rc;
    FRCNN_REQUIRE(name && len > 0, "%s: null name", fn);
    const int n = snprintf(name, len, "roi_align_multi_bwd_tile_kernel<%s, %d>", align_elem_name(dtype), kAlignTile);
    FRCNN_REQUIRE(n >= 0 && static_cast<size_t>(n) < len, "%s: name buffer of %zu bytes too small", fn, len);
    return FRCNN_OK;
}

// ------------------------------------------------------------------ launch plans (host only)
extern "C" int frcnn_roi_align_plan(int64_t R, int N, int C, int H, int W, int PH, int PW, int64_t plan[17]) {
    const char* fn = "frcnn_roi_align_plan";
    if (int rc = align_check(fn, FRCNN_F32, R, N, C, H, W, PH, PW, 0)) return rc;
    FRCNN_REQUIRE(plan, "%s: null plan", fn);
    const int64_t per_roi = static_cast<int64_t>(C) * PH * PW;
    FRCNN_REQUIRE(per_roi == 0 || R <= (int64_t{1} << 38) / per_roi, "%s: output too large", fn);
    AlignFwdPlan f = align_fwd_plan(R, C, PH, PW, false);
    if (N == 0 || H == 0 || W == 0) f.total = f.grid = 0;  // no pixel to sample: a memset, no launch
    AlignBwdPlan b;
    if (int rc = align_bwd_plan(fn, N, C, H, W, PH, PW, b)) return rc;
    const int64_t v[17] = {kAlignRun, kAlignTile, kAlignTileStride, kAlignWaves, kAlignStageBins, kAlignScan,
                           kAlignLaneSamples, f.total, f.grid, b.tiles_x, b.tiles_y, b.cgroups, b.units, b.blocks,
                           b.idle, static_cast<int64_t>(b.lds), b.staged ? 1 : 0};
    for (int i = 0; i < 17; ++i) plan[i] = v[i];
    return FRCNN_OK;
}

extern "C" int frcnn_roi_align_multi_plan(int n_levels, const int* H, const int* W, int N, int C, int PH, int PW,
                                          int64_t plan[14]) {
    const char* fn = "frcnn_roi_align_multi_plan";
    FRCNN_REQUIRE(n_levels >= 1 && n_levels <= kAlignMaxLevels, "%s: n_levels %d is not in [1, %d]", fn, n_levels,
                  kAlignMaxLevels);
    FRCNN_REQUIRE(H && W, "%s: null %s", fn, !H ? "H" : "W");
    FRCNN_REQUIRE(plan, "%s: null plan", fn);
    for (int l = 0; l < n_levels; ++l)
        if (int rc = align_check(fn, FRCNN_F32, 0, N, C, H[l], W[l], PH, PW, 0)) return rc;
    AlignTilePlan t;
    AlignBwdPlan b;
    if (int rc = align_multi_bwd_plan(fn, n_levels, H, W, N, C, PH, PW, t, b)) return rc;
    for (int l = 0; l <= kAlignMaxLevels; ++l) plan[l] = t.first[l];
    plan[9] = b.cgroups;
    plan[10] = b.units;
    plan[11] = b.blocks;
    plan[12] = b.idle;
    plan[13] = b.staged ? 1 : 0;
    return FRCNN_OK;
}
