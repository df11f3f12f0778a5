// Pyramid RPN training on gfx950: torchvision's RegionProposalNetwork.assign_targets_to_anchors
// (box_iou, Matcher with set_low_quality_matches_), BalancedPositiveNegativeSampler,
// BoxCoder.encode with weights (1, 1, 1, 1) and compute_loss for a whole batch and pyramid
// (DESIGN.md §3 "Pyramid RPN training"; include/frcnn_capi.h states the contract).
//
// Targets, five launches, no host sync, no floating-point atomics:
//   rpnt_init_kernel     zeroes the per-gt maxima and the first-digit histograms and takes a
//                        snapshot of (seed, calls), which every later launch reads.
//   rpnt_gtmax_kernel    chip-wide, kRtChunk anchors per workgroup: the anchors are formed in
//                        registers, the image's gt rows sit in LDS; the largest IoU of every gt
//                        over the anchors by integer max on the fp32 bit patterns (LDS, then
//                        one global atomic per gt and workgroup).  The [G, A] matrix never exists.
//   rpnt_label_kernel    chip-wide, same grid: the IoUs again, the Matcher's result per anchor,
//                        the Philox key of every positive and negative (kept in the workspace)
//                        and the histogram of its top 8 bits per class (LDS, then integer
//                        atomics), so the selection starts at the boundary bucket.
//   rpnt_select_kernel   one workgroup per (image, class): the boundary bucket from the histogram
//                        (hist_find, radix_select.h), then one sweep over the image's matches that
//                        takes the buckets below it and lists the boundary bucket in LDS, where it
//                        is sorted; a bucket beyond the list (many equal keys) is refined by an
//                        exact radix select with further sweeps.  The chosen anchors are sorted by
//                        index in LDS and written with their regression targets, counts and padding.
//   rpnt_finish_kernel   chip-wide: the dense `sampled` map from the two thresholds of the
//                        image; its first thread adds 1 to calls.
// Losses: rpnl_fwd_kernel (one thread per sample slot, fp64 partials per workgroup),
// rpnl_reduce_kernel (one workgroup, fixed order) and rpnl_bwd_kernel (every element of every
// level's gradient stored once, found through the dense map; no scatter, no memset).
#include <algorithm>
#include <cmath>

#include "common.h"
#include "elem16.h"
#include "match_sample.h"
#include "radix_select.h"

namespace frcnn {
namespace {

constexpr int kRtMaxLevels = 8;
constexpr int kRtMaxK = 32;
constexpr int kRtMaxN = 1024;
constexpr int kRtMaxG = 256;
constexpr int kRtMaxB = 1024;
constexpr int kRtMaxA = 1 << 24;     // exclusive, per level: anchor indices and shifts stay exact in fp32
constexpr int kRtThreads = 256;      // gtmax / label / finish
constexpr int kRtPer = 4;            // anchors per thread there
constexpr int kRtChunk = kRtThreads * kRtPer;
constexpr int kRtBins0 = 256;        // first digit: the top 8 bits of the key
constexpr int kRtSelThreads = 1024;  // select (hist_find's workgroup)
constexpr int kRtBins = 4096;
constexpr int kRtCap = 4096;         // keys of the boundary bucket the select kernel sorts in LDS; the name query
                                     // reports it as lds=, which is where the tests' cases take it from

struct RtLevels {
    const float4* base[kRtMaxLevels];
    int H[kRtMaxLevels], W[kRtMaxLevels], sh[kRtMaxLevels], sw[kRtMaxLevels];
    int off[kRtMaxLevels + 1];  // first global anchor index of every level; off[L] = A
    int L, K;
};

struct RtWs {
    unsigned* gtmax;   // [N][G] bit pattern of the largest IoU of the gt over the anchors
    unsigned* hist;    // [N][2][kRtBins0] first-digit counts of the positives / the negatives
    uint64_t* thr;     // [N][2] inclusive threshold on (key << 32 | anchor)
    int* num;          // [N][2] samples of the class
    int64_t* rng;      // [2] (seed, calls) as the call found them
    uint32_t* keys;    // [N][A] the masked Philox key of every anchor (0 where matches is -2)
    size_t bytes;
};

RtWs rt_carve(void* ws, int N, int G, int A) {
    Carver c(ws);
    RtWs w{};
    w.gtmax = c.take<unsigned>(static_cast<size_t>(N) * G);
    w.hist = c.take<unsigned>(static_cast<size_t>(N) * 2 * kRtBins0);
    w.thr = c.take<uint64_t>(static_cast<size_t>(N) * 2);
    w.num = c.take<int>(static_cast<size_t>(N) * 2);
    w.rng = c.take<int64_t>(2);
    w.keys = c.take<uint32_t>(static_cast<size_t>(N) * A);
    w.bytes = c.used();
    return w;
}

// The sampling key of anchor a of image n (RtKeyer, match_sample.h) orders the anchors by
// rt_comp(key, a) = key << 32 | a.
__device__ __forceinline__ uint64_t rt_comp(uint32_t key, unsigned a) { return (static_cast<uint64_t>(key) << 32) | a; }

// Anchor a (global index) in registers: its level, cell and base row, one fp32 addition per coordinate.
__device__ __forceinline__ float4 rt_anchor(const RtLevels& g, unsigned a) {
    int l = 0;
    while (l + 1 < g.L && a >= static_cast<unsigned>(g.off[l + 1])) ++l;
    const unsigned loc = a - g.off[l], K = g.K, W = g.W[l];
    const unsigned cell = loc / K, k = loc - cell * K;
    const unsigned y = cell / W, x = cell - y * W;
    const float4 bb = g.base[l][k];
    const float sx = static_cast<float>(static_cast<int>(x) * g.sw[l]);
    const float sy = static_cast<float>(static_cast<int>(y) * g.sh[l]);
    return make_float4(bb.x + sx, bb.y + sy, bb.z + sx, bb.w + sy);
}

__global__ __launch_bounds__(kRtThreads) void rpnt_init_kernel(RtWs ws, int N, int G, const int64_t* __restrict__ rng) {
    const size_t i = static_cast<size_t>(blockIdx.x) * kRtThreads + threadIdx.x;
    if (i < static_cast<size_t>(N) * G) ws.gtmax[i] = 0u;
    if (i < static_cast<size_t>(N) * 2 * kRtBins0) ws.hist[i] = 0u;
    if (i < 2) ws.rng[i] = rng[i];
}

__global__ __launch_bounds__(kRtThreads) void rpnt_gtmax_kernel(RtLevels g, int G, const float4* __restrict__ gt,
                                                                const int32_t* __restrict__ gt_count, RtWs ws) {
    __shared__ float4 sbox[kRtMaxG];
    __shared__ float sarea[kRtMaxG];
    __shared__ unsigned smax[kRtMaxG];
    const int n = blockIdx.y, tid = threadIdx.x;
    const unsigned A = g.off[g.L];
    const int cnt = rt_load_gts(gt, gt_count, n, G, sbox, sarea);
    for (int t = tid; t < G; t += kRtThreads) smax[t] = 0u;
    __syncthreads();
    const int lane = tid & 63;
    float4 ab[kRtPer];
    float aarea[kRtPer];
    bool live[kRtPer];
#pragma unroll
    for (int q = 0; q < kRtPer; ++q) {
        const unsigned a = blockIdx.x * kRtChunk + q * kRtThreads + tid;
        live[q] = a < A;
        ab[q] = rt_anchor(g, live[q] ? a : 0u);
        aarea[q] = (ab[q].z - ab[q].x) * (ab[q].w - ab[q].y);
    }
#pragma unroll 1
    for (int j = 0; j < cnt; ++j) {  // whole waves stay in the loop: the wave's maximum goes to LDS once
        const float ga = sarea[j];
        if (ga < 0.0f) continue;
        const float4 gb = sbox[j];
        unsigned bits = 0u;  // IoUs are non-negative: their bits order as unsigned
#pragma unroll
        for (int q = 0; q < kRtPer; ++q) {
            const float iou = live[q] ? rt_iou(gb, ga, ab[q], aarea[q]) : 0.0f;
            const unsigned b = iou > 0.0f ? __float_as_uint(iou) : 0u;
            bits = b > bits ? b : bits;
        }
        if (__ballot(bits != 0u) == 0ull) continue;
        bits = wave_reduce(bits, op_max{});
        if (lane == 0) atomicMax(&smax[j], bits);
    }
    __syncthreads();
    for (int t = tid; t < cnt; t += kRtThreads)
        if (smax[t] != 0u) atomicMax(&ws.gtmax[static_cast<size_t>(n) * G + t], smax[t]);
}

// -1 below bg, -2 between, else the gt index; the low-quality rule gives the argmax back.
__global__ __launch_bounds__(kRtThreads) void rpnt_label_kernel(RtLevels g, int G, const float4* __restrict__ gt,
                                                                const int32_t* __restrict__ gt_count, float fg,
                                                                float bg, int allow_lq, int key_bits, RtWs ws,
                                                                int32_t* __restrict__ matches) {
    __shared__ float4 sbox[kRtMaxG];
    __shared__ float sarea[kRtMaxG];
    __shared__ float sgmax[kRtMaxG];
    __shared__ unsigned shist[2 * kRtBins0];
    const int n = blockIdx.y, tid = threadIdx.x;
    const unsigned A = g.off[g.L];
    const int cnt = rt_load_gts(gt, gt_count, n, G, sbox, sarea);
    for (int t = tid; t < G; t += kRtThreads) sgmax[t] = __uint_as_float(ws.gtmax[static_cast<size_t>(n) * G + t]);
    for (int t = tid; t < 2 * kRtBins0; t += kRtThreads) shist[t] = 0u;
    __syncthreads();
    const RtKeyer keyer(ws.rng, key_bits);
#pragma unroll 1
    for (int q = 0; q < kRtPer; ++q) {
        const unsigned a = blockIdx.x * kRtChunk + q * kRtThreads + tid;
        if (a >= A) break;
        const float4 ab = rt_anchor(g, a);
        const float aarea = (ab.z - ab.x) * (ab.w - ab.y);
        float best = -1.0f;
        int arg = -1;
        bool restore = false;
        for (int j = 0; j < cnt; ++j) {
            const float ga = sarea[j];
            if (ga < 0.0f) continue;
            const float iou = rt_iou(sbox[j], ga, ab, aarea);
            if (iou > best) {  // strict: the lowest index wins a tie
                best = iou;
                arg = j;
            }
            if (iou == sgmax[j]) restore = true;
        }
        int m = -1;
        if (arg >= 0) {
            m = best < bg ? -1 : best < fg ? -2 : arg;
            if (allow_lq && restore) m = arg;
        }
        matches[static_cast<size_t>(n) * A + a] = m;
        const uint32_t key = m != -2 ? keyer(a, n) : 0u;
        ws.keys[static_cast<size_t>(n) * A + a] = key;
        if (m != -2) atomicAdd(&shist[(m >= 0 ? 0 : kRtBins0) + (key >> 24)], 1u);
    }
    __syncthreads();
    for (int t = tid; t < 2 * kRtBins0; t += kRtThreads)
        if (shist[t] != 0u) atomicAdd(&ws.hist[static_cast<size_t>(n) * 2 * kRtBins0 + t], shist[t]);
}

struct RtSelShared {
    RadixBin bin;
    unsigned wsum[16];
    unsigned tot[2];
    unsigned cdef, cbkt;  // anchors chosen so far, keys in the boundary bucket's list
};

// Ascending bitonic sort of v[0, ns) in LDS by the select kernel's workgroup; ns a power of two.
// The caller puts a barrier before it; it ends on one.
template <class T>
__device__ __forceinline__ void rt_lds_sort(T* v, int ns) {
    for (int kk = 2; kk <= ns; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < ns; i += kRtSelThreads) {
                const int o = i ^ j;
                if (o > i) {
                    const T a = v[i], b = v[o];
                    if ((a > b) == ((i & kk) == 0)) {
                        v[i] = b;
                        v[o] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// Digits of the key below the first one, then of the anchor index.
__device__ __forceinline__ int rt_pass_shift(int pass) { return pass == 0 ? 44 : pass == 1 ? 32 : pass == 2 ? 20 : pass == 3 ? 8 : 0; }
__device__ __forceinline__ int rt_pass_width(int pass) { return pass == 4 ? 8 : 12; }

__global__ __launch_bounds__(kRtSelThreads) void rpnt_select_kernel(RtLevels g, int G, const float4* __restrict__ gt,
                                                                    int B, int max_pos, int key_bits, RtWs ws,
                                                                    const int32_t* __restrict__ matches,
                                                                    int32_t* __restrict__ samples,
                                                                    int32_t* __restrict__ n_pos,
                                                                    int32_t* __restrict__ n_neg,
                                                                    float4* __restrict__ reg_targets) {
    __shared__ unsigned hist[kRtBins];
    __shared__ uint64_t sbucket[kRtCap];   // the boundary bucket's keys
    __shared__ uint32_t schosen[kRtMaxB];  // the chosen anchors, then sorted
    __shared__ RtSelShared sh;
    const int cls = blockIdx.x, n = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const unsigned A = g.off[g.L];
    const int32_t* __restrict__ mt = matches + static_cast<size_t>(n) * A;
    const uint32_t* __restrict__ kt = ws.keys + static_cast<size_t>(n) * A;

    // class totals from the first-digit histograms (waves 0-3: positives, 4-7: negatives)
    {
        const unsigned* gh = ws.hist + static_cast<size_t>(n) * 2 * kRtBins0;
        unsigned v = tid < 2 * kRtBins0 ? gh[tid] : 0u;
        if (tid < 2 * kRtBins0 && (tid >> 8) == cls) hist[tid & (kRtBins0 - 1)] = v;
        v = wave_reduce(v, op_add{});
        if (lane == 0 && wid < 8) sh.wsum[wid] = v;
        __syncthreads();
        if (tid < 2) sh.tot[tid] = sh.wsum[4 * tid] + sh.wsum[4 * tid + 1] + sh.wsum[4 * tid + 2] + sh.wsum[4 * tid + 3];
        __syncthreads();
    }
    const unsigned P = sh.tot[0], Ng = sh.tot[1];
    const unsigned num_pos = P < static_cast<unsigned>(max_pos) ? P : static_cast<unsigned>(max_pos);
    const unsigned room = static_cast<unsigned>(B) - num_pos;
    const unsigned num_neg = Ng < room ? Ng : room;
    const unsigned num = cls == 0 ? num_pos : num_neg;
    const unsigned total = cls == 0 ? P : Ng;

    const auto in_class = [&](int m) { return cls == 0 ? m >= 0 : m == -1; };
    // f(anchor, key << 32 | anchor) for every anchor of the class; the matches and the keys the
    // label kernel left, four loads of each in flight per thread
    const auto sweep = [&](auto&& f) {
#pragma unroll 1
        for (unsigned a0 = 0; a0 < A; a0 += 4 * kRtSelThreads) {
            int m[4];
            uint32_t k[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const unsigned a = a0 + q * kRtSelThreads + tid;
                m[q] = a < A ? mt[a] : -2;
                k[q] = a < A ? kt[a] : 0u;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const unsigned a = a0 + q * kRtSelThreads + tid;
                if (in_class(m[q])) f(a, rt_comp(k[q], a));
            }
        }
    };
    const auto choose = [&](unsigned a) {
        const unsigned at = atomicAdd(&sh.cdef, 1u);
        if (at < static_cast<unsigned>(kRtMaxB)) schosen[at] = a;  // always: at most num are chosen
    };

    uint64_t T = ~0ull;
    if (tid == 0) sh.cdef = 0u, sh.cbkt = 0u;
    __syncthreads();
    if (num != 0u && num == total) {  // the whole class
        sweep([&](unsigned a, uint64_t) { choose(a); });
    } else if (num != 0u) {
        unsigned need = num;
        hist_find(hist, kRtBins0, need, sh.bin, sh.wsum);
        const unsigned before = sh.bin.before, bucket = sh.bin.bucket, d0 = sh.bin.digit;
        need -= before;
        uint64_t prefix = static_cast<uint64_t>(d0) << 56;
        T = prefix | ((1ull << 56) - 1ull);
        __syncthreads();  // sh.bin consumed
        if (bucket <= static_cast<unsigned>(kRtCap)) {
            // one sweep: the buckets below the boundary are chosen, the boundary bucket goes to LDS
            sweep([&](unsigned a, uint64_t key) {
                const unsigned dg = static_cast<unsigned>(key >> 56);
                if (dg < d0) {
                    choose(a);
                } else if (dg == d0) {
                    const unsigned at = atomicAdd(&sh.cbkt, 1u);
                    if (at < static_cast<unsigned>(kRtCap)) sbucket[at] = key;  // always: bucket of them exist
                }
            });
            __syncthreads();
            if (need != bucket) {  // its need smallest: sorted, the keys are distinct
                int ns = 64;
                while (ns < static_cast<int>(bucket)) ns <<= 1;
                for (int i = bucket + tid; i < ns; i += kRtSelThreads) sbucket[i] = ~0ull;
                __syncthreads();
                rt_lds_sort(sbucket, ns);
                T = sbucket[need - 1];
            }
            for (unsigned i = tid; i < need; i += kRtSelThreads)  // before + need = num <= kRtMaxB
                schosen[before + i] = static_cast<uint32_t>(sbucket[i]);
        } else {
            // a boundary bucket beyond the LDS list (many equal keys): radix select by further sweeps
            uint64_t hm = ~0ull << 56;
            bool whole = false;  // need <= kRtMaxB < bucket
#pragma unroll 1
            for (int pass = 0; pass < 5 && !whole; ++pass) {
                const int shift = rt_pass_shift(pass), width = rt_pass_width(pass);
                const int nbins = 1 << width;
                if (pass < 2 && key_bits <= 8 + 12 * pass) {  // these key bits are masked away: one bucket, digit 0
                    hm = ~0ull << shift;
                    T = prefix | ((1ull << shift) - 1ull);
                    continue;
                }
                for (int i = tid; i < nbins; i += kRtSelThreads) hist[i] = 0u;
                __syncthreads();
                sweep([&](unsigned, uint64_t key) {
                    if ((key & hm) == prefix) atomicAdd(&hist[static_cast<unsigned>(key >> shift) & (nbins - 1)], 1u);
                });
                __syncthreads();
                hist_find(hist, nbins, need, sh.bin, sh.wsum);
                need -= sh.bin.before;
                prefix |= static_cast<uint64_t>(sh.bin.digit) << shift;
                hm = ~0ull << shift;
                T = prefix | ((1ull << shift) - 1ull);
                whole = sh.bin.bucket == need;
                __syncthreads();  // sh.bin consumed before the next pass rewrites it
            }
            sweep([&](unsigned a, uint64_t key) {
                if (key <= T) choose(a);
            });
        }
    }
    __syncthreads();

    // the class's samples in ascending anchor order: positives from slot 0, negatives behind them
    const size_t row0 = static_cast<size_t>(n) * B;
    const unsigned slot0 = cls == 0 ? 0u : num_pos;
    if (num != 0u) {
        int ns = 64;
        while (ns < static_cast<int>(num)) ns <<= 1;  // <= kRtMaxB
        for (int i = num + tid; i < ns; i += kRtSelThreads) schosen[i] = ~0u;
        __syncthreads();
        rt_lds_sort(schosen, ns);
        for (unsigned i = tid; i < num; i += kRtSelThreads) {
            const unsigned a = schosen[i], slot = slot0 + i;
            if (a >= A || slot >= static_cast<unsigned>(B)) continue;  // never
            float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
            if (cls == 0) {
                const int m = mt[a];
                const float4 ab = rt_anchor(g, a);
                const float4 gb = gt[static_cast<size_t>(n) * G + max(0, min(m, G - 1))];
                const float aw = ab.z - ab.x, ah = ab.w - ab.y;
                const float acx = ab.x + 0.5f * aw, acy = ab.y + 0.5f * ah;
                const float gw = gb.z - gb.x, gh = gb.w - gb.y;
                const float gcx = gb.x + 0.5f * gw, gcy = gb.y + 0.5f * gh;
                t = make_float4((gcx - acx) / aw, (gcy - acy) / ah, rt_log_cr(gw / aw), rt_log_cr(gh / ah));
            }
            samples[row0 + slot] = static_cast<int32_t>(a);
            reg_targets[row0 + slot] = t;
        }
    }
    if (cls == 1) {  // padding behind the negatives
        for (unsigned s = num_pos + num_neg + tid; s < static_cast<unsigned>(B); s += kRtSelThreads) {
            samples[row0 + s] = -1;
            reg_targets[row0 + s] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    if (tid == 0) {
        (cls == 0 ? n_pos : n_neg)[n] = static_cast<int32_t>(num);
        ws.thr[2 * n + cls] = T;
        ws.num[2 * n + cls] = static_cast<int>(num);
    }
}

__global__ __launch_bounds__(kRtThreads) void rpnt_finish_kernel(int A_, RtWs ws,
                                                                 const int32_t* __restrict__ matches,
                                                                 int32_t* __restrict__ sampled, int64_t* rng) {
    const int n = blockIdx.y, tid = threadIdx.x;
    const unsigned A = A_;
    const uint64_t T0 = ws.thr[2 * n], T1 = ws.thr[2 * n + 1];
    const bool any0 = ws.num[2 * n] > 0, any1 = ws.num[2 * n + 1] > 0;
#pragma unroll
    for (int q = 0; q < kRtPer; ++q) {
        const unsigned a = blockIdx.x * kRtChunk + q * kRtThreads + tid;
        if (a >= A) break;
        const int m = matches[static_cast<size_t>(n) * A + a];
        const uint64_t key = rt_comp(ws.keys[static_cast<size_t>(n) * A + a], a);
        int s = -1;
        if (m >= 0) {
            if (any0 && key <= T0) s = 1;
        } else if (m == -1) {
            if (any1 && key <= T1) s = 0;
        }
        sampled[static_cast<size_t>(n) * A + a] = s;
    }
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0)
        rng[1] = static_cast<int64_t>(static_cast<uint64_t>(ws.rng[1]) + 1ull);  // the snapshot: others still read it
}

// Shape checks shared by the entry points of the targets; fills the level offsets.
int rt_check_shape(const char* who, int L, int N, int K, const int* H, const int* W, int G, int B, int off[]) {
    FRCNN_REQUIRE(L >= 1 && L <= kRtMaxLevels, "%s: n_levels must be in [1, %d], got %d", who, kRtMaxLevels, L);
    FRCNN_REQUIRE(N >= 1 && N <= kRtMaxN, "%s: N must be in [1, %d], got %d", who, kRtMaxN, N);
    FRCNN_REQUIRE(K >= 1 && K <= kRtMaxK, "%s: K must be in [1, %d], got %d", who, kRtMaxK, K);
    FRCNN_REQUIRE(G >= 1 && G <= kRtMaxG, "%s: G must be in [1, %d], got %d", who, kRtMaxG, G);
    FRCNN_REQUIRE(B >= 1 && B <= kRtMaxB, "%s: batch_size_per_image must be in [1, %d], got %d", who, kRtMaxB, B);
    FRCNN_REQUIRE(H && W, "%s: null H / W", who);
    int64_t A = 0;
    for (int l = 0; l < L; ++l) {
        FRCNN_REQUIRE(H[l] >= 1 && W[l] >= 1, "%s: level %d is %d x %d; H and W must be >= 1", who, l, H[l], W[l]);
        const int64_t Al = static_cast<int64_t>(K) * H[l] * W[l];
        FRCNN_REQUIRE(Al < kRtMaxA, "%s: level %d has %lld anchors; K*H*W must be below 2^24", who, l,
                      static_cast<long long>(Al));
        off[l] = static_cast<int>(A);
        A += Al;
    }
    FRCNN_REQUIRE(A < (int64_t{1} << 31), "%s: %lld anchors in all; A must be below 2^31", who, static_cast<long long>(A));
    off[L] = static_cast<int>(A);
    return FRCNN_OK;
}

int rt_check_key_bits(const char* who, int key_bits) {
    FRCNN_REQUIRE(key_bits >= 0 && key_bits <= 32, "%s: key_bits must be in [0, 32], got %d", who, key_bits);
    return FRCNN_OK;
}

// ------------------------------------------------------------------- losses
constexpr int kRlThreads = 256;
constexpr int kRlMaxBlocks = 2048;
constexpr int kRlPer = 4;  // gradient elements per thread

struct RlLevels {
    const void* obj[kRtMaxLevels];
    const void* del[kRtMaxLevels];
    void* dobj[kRtMaxLevels];
    void* ddel[kRtMaxLevels];
    int H[kRtMaxLevels], W[kRtMaxLevels];
    int off[kRtMaxLevels + 1];
    unsigned blk[2 * kRtMaxLevels + 1];  // first workgroup of segment 2l (dobj of level l) / 2l + 1 (ddel)
    int L, K;
};

struct RlPartial {
    double obj, box;
    int32_t cnt, pad;
};

struct RlConsts {
    float beta, half_beta;
};

__device__ __forceinline__ void rl_block_sum(double& a, double& b, int& c) {
    __shared__ double sd[2][kRlThreads / kWave];
    __shared__ int si[kRlThreads / kWave];
    a = wave_reduce(a, op_add{});
    b = wave_reduce(b, op_add{});
    c = wave_reduce(c, op_add{});
    const int w = threadIdx.x / kWave;
    if (lane_id() == 0) sd[0][w] = a, sd[1][w] = b, si[w] = c;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 1; k < kRlThreads / kWave; ++k) a += sd[0][k], b += sd[1][k], c += si[k];
}

// binary cross-entropy with logits against t in {0, 1}: (max(x, 0) - x*t) + log1p(exp(-|x|))
__device__ __forceinline__ float rl_bce(float x, float t) {
    const float e = exp_cr(-fabsf(x));
    const float lin = (x > 0.0f ? x : 0.0f) - x * t;
    return lin + rt_log1p_cr(e);
}

// its derivative sigmoid(x) - t, the sigmoid from the same exp
__device__ __forceinline__ float rl_bce_grad(float x, float t) {
    const float e = exp_cr(-fabsf(x));
    const float s = x >= 0.0f ? 1.0f / (1.0f + e) : e / (1.0f + e);
    return s - t;
}

__device__ __forceinline__ int rl_level(const RlLevels& g, unsigned a) {
    int l = 0;
    while (l + 1 < g.L && a >= static_cast<unsigned>(g.off[l + 1])) ++l;
    return l;
}

template <class E>
__global__ __launch_bounds__(kRlThreads) void rpnl_fwd_kernel(RlLevels g, int N, int B,
                                                              const int32_t* __restrict__ samples,
                                                              const int32_t* __restrict__ n_pos,
                                                              const int32_t* __restrict__ n_neg,
                                                              const float* __restrict__ reg_t, RlConsts k,
                                                              RlPartial* __restrict__ part) {
    using raw = typename E::raw;
    double osum = 0.0, bsum = 0.0;
    int cnt = 0;
    const unsigned A = g.off[g.L];
    const int64_t rows = static_cast<int64_t>(N) * B;
    const int64_t step = static_cast<int64_t>(gridDim.x) * kRlThreads;
    for (int64_t r = static_cast<int64_t>(blockIdx.x) * kRlThreads + threadIdx.x; r < rows; r += step) {
        const int n = static_cast<int>(r / B), j = static_cast<int>(r - static_cast<int64_t>(n) * B);
        const int np = max(0, min(n_pos[n], B));
        const int ng = max(0, min(n_neg[n], B - np));
        if (j >= np + ng) continue;
        const unsigned a = static_cast<unsigned>(samples[r]);
        if (a >= A) continue;  // never, for the targets op's output
        ++cnt;
        const int l = rl_level(g, a);
        const unsigned K = g.K, HW = static_cast<unsigned>(g.H[l]) * g.W[l];
        const unsigned loc = a - g.off[l], cell = loc / K, kk = loc - cell * K;
        const raw* obj = static_cast<const raw*>(g.obj[l]) + (static_cast<size_t>(n) * K + kk) * HW + cell;
        osum += static_cast<double>(rl_bce(E::widen(*obj), j < np ? 1.0f : 0.0f));
        if (j < np) {
            const raw* d = static_cast<const raw*>(g.del[l]) + (static_cast<size_t>(n) * 4 * K + 4 * kk) * HW + cell;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float z = fabsf(E::widen(d[static_cast<size_t>(c) * HW]) - reg_t[r * 4 + c]);
                bsum += static_cast<double>(z < k.beta ? 0.5f * z * z / k.beta : z - k.half_beta);
            }
        }
    }
    rl_block_sum(osum, bsum, cnt);
    if (threadIdx.x == 0) part[blockIdx.x] = RlPartial{osum, bsum, cnt, 0};
}

__global__ __launch_bounds__(kRlThreads) void rpnl_reduce_kernel(const RlPartial* __restrict__ part, int nparts,
                                                                 float* __restrict__ loss, int32_t* __restrict__ stats) {
    double osum = 0.0, bsum = 0.0;
    int cnt = 0;
    for (int i = threadIdx.x; i < nparts; i += kRlThreads) {
        const RlPartial p = part[i];
        osum += p.obj, bsum += p.box, cnt += p.cnt;
    }
    rl_block_sum(osum, bsum, cnt);
    if (threadIdx.x == 0) {
        loss[0] = static_cast<float>(osum / static_cast<double>(cnt));  // 0/0 = NaN, as torch
        loss[1] = static_cast<float>(bsum / static_cast<double>(cnt));
        stats[0] = cnt;
        stats[1] = 0;
    }
}

// Every element of every level's dobjectness / ddeltas, kRlPer consecutive ones per thread.
template <class E>
__global__ __launch_bounds__(kRlThreads) void rpnl_bwd_kernel(RlLevels g, int N, int B,
                                                              const int32_t* __restrict__ sampled,
                                                              const int32_t* __restrict__ samples,
                                                              const int32_t* __restrict__ n_pos,
                                                              const float* __restrict__ reg_t, RlConsts k,
                                                              const int32_t* __restrict__ stats,
                                                              const float* __restrict__ g_obj,
                                                              const float* __restrict__ g_box) {
    using raw = typename E::raw;
    int seg = 0;
    while (seg + 1 < 2 * g.L && blockIdx.x >= g.blk[seg + 1]) ++seg;
    const int l = seg >> 1;
    const bool is_del = seg & 1;
    const unsigned K = g.K, HW = static_cast<unsigned>(g.H[l]) * g.W[l];
    const unsigned A = g.off[g.L];
    const unsigned CH = is_del ? 4 * K : K;
    const size_t count = static_cast<size_t>(N) * CH * HW;
    const size_t e0 = (static_cast<size_t>(blockIdx.x - g.blk[seg]) * kRlThreads + threadIdx.x) * kRlPer;
    if (e0 >= count) return;
    const float S = static_cast<float>(stats[0]);
    const bool live = is_del ? g_box != nullptr : g_obj != nullptr;
    const float scale = live ? (is_del ? *g_box : *g_obj) / S : 0.0f;
    const raw* in = static_cast<const raw*>(is_del ? g.del[l] : g.obj[l]);
    raw* out = static_cast<raw*>(is_del ? g.ddel[l] : g.dobj[l]);
    float v[kRlPer];
#pragma unroll
    for (int q = 0; q < kRlPer; ++q) {
        v[q] = 0.0f;
        const size_t e = e0 + q;
        if (e >= count || !live || stats[0] <= 0) continue;
        const unsigned n = static_cast<unsigned>(e / (static_cast<size_t>(CH) * HW));
        const unsigned rem = static_cast<unsigned>(e - static_cast<size_t>(n) * CH * HW);
        const unsigned ch = rem / HW, cell = rem - ch * HW;
        const unsigned kk = is_del ? ch >> 2 : ch;
        const unsigned a = g.off[l] + cell * K + kk;
        const int s = sampled[static_cast<size_t>(n) * A + a];
        if (s < 0) continue;
        if (!is_del) {
            v[q] = rl_bce_grad(E::widen(in[e]), s > 0 ? 1.0f : 0.0f) * scale;
        } else if (s > 0) {
            // the positive's slot: its anchor among the ascending first n_pos samples
            const int np = max(0, min(n_pos[n], B));
            const int32_t* sm = samples + static_cast<size_t>(n) * B;
            const int j = count_before(sm, np, static_cast<int32_t>(a));
            if (j < np && sm[j] == static_cast<int32_t>(a)) {
                const float t = reg_t[(static_cast<size_t>(n) * B + j) * 4 + (ch & 3)];
                const float d = E::widen(in[e]) - t;
                const float z = fabsf(d);
                const float gr = z < k.beta ? d / k.beta : (d > 0.0f ? 1.0f : d < 0.0f ? -1.0f : d);
                v[q] = gr * scale;
            }
        }
    }
    if (e0 + kRlPer <= count && (reinterpret_cast<uintptr_t>(out + e0) & (sizeof(raw) * kRlPer - 1)) == 0) {
        if constexpr (sizeof(raw) == 2) {
            const uint32_t lo = static_cast<uint32_t>(E::narrow(v[0])) | (static_cast<uint32_t>(E::narrow(v[1])) << 16);
            const uint32_t hi = static_cast<uint32_t>(E::narrow(v[2])) | (static_cast<uint32_t>(E::narrow(v[3])) << 16);
            *reinterpret_cast<uint2*>(out + e0) = make_uint2(lo, hi);
        } else {
            *reinterpret_cast<float4*>(out + e0) = make_float4(v[0], v[1], v[2], v[3]);
        }
    } else {
#pragma unroll
        for (int q = 0; q < kRlPer; ++q)
            if (e0 + q < count) out[e0 + q] = E::narrow(v[q]);
    }
}

int rl_fwd_blocks(int64_t rows) {
    const int64_t b = (rows + kRlThreads - 1) / kRlThreads;
    return static_cast<int>(b < kRlMaxBlocks ? b : kRlMaxBlocks);
}

int rl_check(const char* who, int dtype, int L, int N, int K, const int* H, const int* W, int B, double beta,
             RlLevels* g, RlConsts* k) {
    FRCNN_REQUIRE(dtype_code_ok(dtype), "%s: dtype must be FRCNN_F32, FRCNN_F16 or FRCNN_BF16, got %d", who, dtype);
    int rc = rt_check_shape(who, L, N, K, H, W, 1, B, g->off);
    if (rc) return rc;
    FRCNN_REQUIRE(std::isfinite(beta) && beta >= 0.0, "%s: beta=%g must be finite and not negative", who, beta);
    g->L = L;
    g->K = K;
    for (int l = 0; l < L; ++l) g->H[l] = H[l], g->W[l] = W[l];
    k->beta = static_cast<float>(beta);
    k->half_beta = 0.5f * k->beta;
    return FRCNN_OK;
}

template <class E>
void rl_launch_fwd(const RlLevels& g, int nb, int N, int B, const int32_t* samples, const int32_t* n_pos,
                   const int32_t* n_neg, const float* reg_t, RlConsts k, RlPartial* part, hipStream_t st) {
    hipLaunchKernelGGL((rpnl_fwd_kernel<E>), dim3(nb), dim3(kRlThreads), 0, st, g, N, B, samples, n_pos, n_neg, reg_t, k,
                       part);
}

template <class E>
void rl_launch_bwd(const RlLevels& g, unsigned nb, int N, int B, const int32_t* sampled, const int32_t* samples,
                   const int32_t* n_pos, const float* reg_t, RlConsts k, const int32_t* stats, const float* g_obj,
                   const float* g_box, hipStream_t st) {
    hipLaunchKernelGGL((rpnl_bwd_kernel<E>), dim3(nb), dim3(kRlThreads), 0, st, g, N, B, sampled, samples, n_pos, reg_t, k,
                       stats, g_obj, g_box);
}

}  // namespace
}  // namespace frcnn

using namespace frcnn;

extern "C" size_t frcnn_rpn_targets_multi_workspace_size(int n_levels, int N, int K, const int* H, const int* W, int G,
                                                         int batch_size_per_image) {
    int off[kRtMaxLevels + 1];
    if (rt_check_shape("frcnn_rpn_targets_multi_workspace_size", n_levels, N, K, H, W, G, batch_size_per_image, off))
        return 0;
    return rt_carve(nullptr, N, G, off[n_levels]).bytes;
}

extern "C" int frcnn_rpn_targets_multi_kernel(int n_levels, int N, int K, const int* H, const int* W, int G,
                                              int batch_size_per_image, int key_bits, char* name, size_t len) {
    const char* who = "frcnn_rpn_targets_multi_kernel";
    FRCNN_REQUIRE(name && len > 0, "%s: null name buffer", who);
    int off[kRtMaxLevels + 1];
    int rc = rt_check_shape(who, n_levels, N, K, H, W, G, batch_size_per_image, off);
    if (rc) return rc;
    rc = rt_check_key_bits(who, key_bits);
    if (rc) return rc;
    const int A = off[n_levels];
    const int chunks = (A + kRtChunk - 1) / kRtChunk;
    const int steps = (A + 4 * kRtSelThreads - 1) / (4 * kRtSelThreads);  // of one sweep of the select kernel
    // which branch the select kernel takes depends on the data: a boundary bucket of at most kRtCap keys is
    // sorted in LDS, a larger one goes through the radix passes over these digits of the key
    const char* digits = key_bits <= 8 ? "8" : key_bits <= 20 ? "8+12" : "8+12+12";
    std::snprintf(name, len,
                  "rpnt_init_kernel rpnt_gtmax_kernel[chunks=%d,tail=%d] rpnt_label_kernel rpnt_select_kernel[lds=%d,"
                  "radix=%s,steps=%d] rpnt_finish_kernel",
                  chunks, A - (chunks - 1) * kRtChunk, kRtCap, digits, steps);
    return FRCNN_OK;
}

extern "C" int frcnn_rpn_targets_multi(int n_levels, const float* const* anchor_bases, const int* H, const int* W,
                                       const int* stride_h, const int* stride_w, int N, int K, const float* gt_boxes,
                                       const int32_t* gt_count, int G, int64_t* rng, int batch_size_per_image,
                                       double positive_fraction, double fg_iou_thresh, double bg_iou_thresh,
                                       int allow_low_quality_matches, int key_bits, int32_t* matches, int32_t* sampled,
                                       int32_t* samples, int32_t* n_pos, int32_t* n_neg, float* reg_targets,
                                       void* workspace, size_t ws_bytes, void* stream) {
    const char* who = "frcnn_rpn_targets_multi";
    RtLevels g{};
    const int B = batch_size_per_image;
    int rc = rt_check_shape(who, n_levels, N, K, H, W, G, B, g.off);
    if (rc) return rc;
    rc = rt_check_key_bits(who, key_bits);
    if (rc) return rc;
    FRCNN_REQUIRE(positive_fraction >= 0.0 && positive_fraction <= 1.0, "%s: positive_fraction=%g must be in [0, 1]", who,
                  positive_fraction);
    FRCNN_REQUIRE(bg_iou_thresh <= fg_iou_thresh, "%s: bg_iou_thresh=%g must not exceed fg_iou_thresh=%g", who,
                  bg_iou_thresh, fg_iou_thresh);
    FRCNN_REQUIRE(anchor_bases && stride_h && stride_w, "%s: null per-level array (anchor_bases, stride_h, stride_w)", who);
    FRCNN_REQUIRE(gt_boxes && gt_count && rng, "%s: null input (gt_boxes, gt_count, rng)", who);
    FRCNN_REQUIRE(matches && sampled && samples && n_pos && n_neg && reg_targets, "%s: null output pointer", who);
    FRCNN_REQUIRE(aligned_to(gt_boxes, 16) && aligned_to(reg_targets, 16) && aligned_to(rng, 8),
                  "%s: gt_boxes and reg_targets must be 16-byte aligned, rng 8-byte aligned", who);
    g.L = n_levels;
    g.K = K;
    for (int l = 0; l < n_levels; ++l) {
        FRCNN_REQUIRE(anchor_bases[l], "%s: null anchor_bases[%d]", who, l);
        FRCNN_REQUIRE(aligned_to(anchor_bases[l], 16), "%s: anchor_bases[%d] must be 16-byte aligned", who, l);
        FRCNN_REQUIRE(stride_h[l] >= 1 && stride_w[l] >= 1, "%s: strides of level %d must be >= 1", who, l);
        FRCNN_REQUIRE(static_cast<int64_t>(H[l] - 1) * stride_h[l] < kRtMaxA &&
                          static_cast<int64_t>(W[l] - 1) * stride_w[l] < kRtMaxA,
                      "%s: level %d: (H-1)*stride_h and (W-1)*stride_w must be below 2^24", who, l);
        g.base[l] = reinterpret_cast<const float4*>(anchor_bases[l]);
        g.H[l] = H[l];
        g.W[l] = W[l];
        g.sh[l] = stride_h[l];
        g.sw[l] = stride_w[l];
    }
    RtWs w = rt_carve(workspace, N, G, g.off[n_levels]);
    FRCNN_REQUIRE(workspace && ws_bytes >= w.bytes, "%s: workspace %zu < %zu", who, workspace ? ws_bytes : size_t{0},
                  w.bytes);
    FRCNN_REQUIRE(aligned_to(workspace, 256), "%s: workspace must be 256-byte aligned", who);
    const int max_pos = static_cast<int>(static_cast<double>(B) * positive_fraction);  // Python's int(B * fraction)
    const float fg = static_cast<float>(fg_iou_thresh), bg = static_cast<float>(bg_iou_thresh);
    hipStream_t st = as_stream(stream);
    const int A = g.off[n_levels];
    const unsigned chunks = (static_cast<unsigned>(A) + kRtChunk - 1) / kRtChunk;
    const size_t ninit = std::max<size_t>(static_cast<size_t>(N) * std::max(G, 2 * kRtBins0), 2);
    const float4* gt = reinterpret_cast<const float4*>(gt_boxes);
    hipLaunchKernelGGL(rpnt_init_kernel, dim3(static_cast<unsigned>((ninit + kRtThreads - 1) / kRtThreads)),
                       dim3(kRtThreads), 0, st, w, N, G, rng);
    FRCNN_LAUNCH_CHECK("rpnt_init_kernel");
    hipLaunchKernelGGL(rpnt_gtmax_kernel, dim3(chunks, N), dim3(kRtThreads), 0, st, g, G, gt, gt_count, w);
    FRCNN_LAUNCH_CHECK("rpnt_gtmax_kernel");
    hipLaunchKernelGGL(rpnt_label_kernel, dim3(chunks, N), dim3(kRtThreads), 0, st, g, G, gt, gt_count, fg, bg,
                       allow_low_quality_matches ? 1 : 0, key_bits, w, matches);
    FRCNN_LAUNCH_CHECK("rpnt_label_kernel");
    hipLaunchKernelGGL(rpnt_select_kernel, dim3(2, N), dim3(kRtSelThreads), 0, st, g, G, gt, B, max_pos, key_bits, w,
                       matches, samples, n_pos, n_neg, reinterpret_cast<float4*>(reg_targets));
    FRCNN_LAUNCH_CHECK("rpnt_select_kernel");
    hipLaunchKernelGGL(rpnt_finish_kernel, dim3(chunks, N), dim3(kRtThreads), 0, st, A, w, matches, sampled, rng);
    FRCNN_LAUNCH_CHECK("rpnt_finish_kernel");
    return FRCNN_OK;
}

extern "C" size_t frcnn_rpn_losses_multi_workspace_size(int N, int batch_size_per_image) {
    if (N < 1 || N > kRtMaxN || batch_size_per_image < 1 || batch_size_per_image > kRtMaxB) return 0;
    return align_up(static_cast<size_t>(rl_fwd_blocks(static_cast<int64_t>(N) * batch_size_per_image)) * sizeof(RlPartial),
                    256);
}

extern "C" int frcnn_rpn_losses_multi_fwd_t(int dtype, int n_levels, const void* const* objectness,
                                            const void* const* deltas, const int* H, const int* W, int N, int K,
                                            int batch_size_per_image, const int32_t* samples, const int32_t* n_pos,
                                            const int32_t* n_neg, const float* reg_targets, double beta, float* loss,
                                            int32_t* stats, void* workspace, size_t ws_bytes, void* stream) {
    const char* who = "frcnn_rpn_losses_multi_fwd_t";
    RlLevels g{};
    RlConsts k{};
    const int B = batch_size_per_image;
    int rc = rl_check(who, dtype, n_levels, N, K, H, W, B, beta, &g, &k);
    if (rc) return rc;
    FRCNN_REQUIRE(objectness && deltas, "%s: null per-level array (objectness, deltas)", who);
    FRCNN_REQUIRE(samples && n_pos && n_neg && reg_targets, "%s: null input (samples, n_pos, n_neg, reg_targets)", who);
    FRCNN_REQUIRE(loss && stats, "%s: null output (loss, stats)", who);
    const size_t esz = dtype == FRCNN_F32 ? 4 : 2;
    for (int l = 0; l < n_levels; ++l) {
        FRCNN_REQUIRE(objectness[l] && deltas[l], "%s: null pointer at level %d", who, l);
        FRCNN_REQUIRE(aligned_to(objectness[l], esz) && aligned_to(deltas[l], esz),
                      "%s: objectness / deltas of level %d not aligned to their element size", who, l);
        g.obj[l] = objectness[l];
        g.del[l] = deltas[l];
    }
    const size_t need = frcnn_rpn_losses_multi_workspace_size(N, B);
    FRCNN_REQUIRE(workspace && ws_bytes >= need, "%s: workspace %zu < %zu", who, workspace ? ws_bytes : size_t{0}, need);
    FRCNN_REQUIRE(aligned_to(workspace, 256), "%s: workspace must be 256-byte aligned", who);
    hipStream_t st = as_stream(stream);
    RlPartial* part = static_cast<RlPartial*>(workspace);
    const int nb = rl_fwd_blocks(static_cast<int64_t>(N) * B);
    if (dtype == FRCNN_F32)
        rl_launch_fwd<ElemF32>(g, nb, N, B, samples, n_pos, n_neg, reg_targets, k, part, st);
    else if (dtype == FRCNN_F16)
        rl_launch_fwd<ElemF16>(g, nb, N, B, samples, n_pos, n_neg, reg_targets, k, part, st);
    else
        rl_launch_fwd<ElemBF16>(g, nb, N, B, samples, n_pos, n_neg, reg_targets, k, part, st);
    FRCNN_LAUNCH_CHECK("rpnl_fwd_kernel");
    hipLaunchKernelGGL(rpnl_reduce_kernel, dim3(1), dim3(kRlThreads), 0, st, part, nb, loss, stats);
    FRCNN_LAUNCH_CHECK("rpnl_reduce_kernel");
    return FRCNN_OK;
}

extern "C" int frcnn_rpn_losses_multi_bwd_t(int dtype, int n_levels, const void* const* objectness,
                                            const void* const* deltas, const int* H, const int* W, int N, int K,
                                            int batch_size_per_image, const int32_t* sampled, const int32_t* samples,
                                            const int32_t* n_pos, const float* reg_targets, double beta,
                                            const int32_t* stats, const float* g_obj, const float* g_box,
                                            void* const* dobjectness, void* const* ddeltas, void* stream) {
    const char* who = "frcnn_rpn_losses_multi_bwd_t";
    RlLevels g{};
    RlConsts k{};
    const int B = batch_size_per_image;
    int rc = rl_check(who, dtype, n_levels, N, K, H, W, B, beta, &g, &k);
    if (rc) return rc;
    FRCNN_REQUIRE(objectness && deltas && dobjectness && ddeltas,
                  "%s: null per-level array (objectness, deltas, dobjectness, ddeltas)", who);
    FRCNN_REQUIRE(sampled && samples && n_pos && reg_targets && stats,
                  "%s: null input (sampled, samples, n_pos, reg_targets, stats)", who);
    const size_t esz = dtype == FRCNN_F32 ? 4 : 2;
    uint64_t blocks = 0;
    for (int l = 0; l < n_levels; ++l) {
        FRCNN_REQUIRE(objectness[l] && deltas[l] && dobjectness[l] && ddeltas[l], "%s: null pointer at level %d", who, l);
        FRCNN_REQUIRE(aligned_to(objectness[l], esz) && aligned_to(deltas[l], esz) && aligned_to(dobjectness[l], esz) &&
                          aligned_to(ddeltas[l], esz),
                      "%s: tensors of level %d not aligned to their element size", who, l);
        g.obj[l] = objectness[l];
        g.del[l] = deltas[l];
        g.dobj[l] = dobjectness[l];
        g.ddel[l] = ddeltas[l];
        const uint64_t no = static_cast<uint64_t>(N) * K * H[l] * W[l];
        const uint64_t per = static_cast<uint64_t>(kRlThreads) * kRlPer;
        g.blk[2 * l] = static_cast<unsigned>(blocks);
        blocks += (no + per - 1) / per;
        g.blk[2 * l + 1] = static_cast<unsigned>(blocks);
        blocks += (4 * no + per - 1) / per;
        FRCNN_REQUIRE(blocks < (uint64_t{1} << 31), "%s: N*A is too large for one backward launch", who);
    }
    g.blk[2 * n_levels] = static_cast<unsigned>(blocks);
    hipStream_t st = as_stream(stream);
    const unsigned nb = static_cast<unsigned>(blocks);
    if (dtype == FRCNN_F32)
        rl_launch_bwd<ElemF32>(g, nb, N, B, sampled, samples, n_pos, reg_targets, k, stats, g_obj, g_box, st);
    else if (dtype == FRCNN_F16)
        rl_launch_bwd<ElemF16>(g, nb, N, B, sampled, samples, n_pos, reg_targets, k, stats, g_obj, g_box, st);
    else
        rl_launch_bwd<ElemBF16>(g, nb, N, B, sampled, samples, n_pos, reg_targets, k, stats, g_obj, g_box, st);
    FRCNN_LAUNCH_CHECK("rpnl_bwd_kernel");
    return FRCNN_OK;
}
