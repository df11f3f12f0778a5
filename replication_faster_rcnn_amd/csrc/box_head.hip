// Pyramid box-head training on gfx950: torchvision's RoIHeads.select_training_samples
// (add_gt_proposals, box_iou, Matcher without low-quality matches, assign_targets_to_proposals,
// BalancedPositiveNegativeSampler, BoxCoder.encode with weights) and fastrcnn_loss for a whole
// batch (DESIGN.md §3 "Pyramid box-head training"; include/frcnn_capi.h states the contract).
//
// Targets, two launches, no host sync, no atomics on global memory:
//   bht_match_kernel    grid (ceil(M / 256), N), one thread per candidate (M = R + G: the
//                       proposals, then the gt rows), the image's gt rows in LDS: the Matcher's
//                       result, the class the label gives (positive / negative / neither) and the
//                       Philox key of every candidate.  The [G, M] matrix never exists.
//   bht_sample_kernel   one workgroup per image, the image's classes and keys in LDS: the
//                       inclusive threshold of each class's k smallest (key, index) by an exact
//                       radix select over LDS histograms (hist_find, radix_select.h), one blocked
//                       scan that gives every chosen candidate its slot in ascending index order,
//                       then the gather, the encode and the padding.  Its first thread adds 1 to
//                       calls: nothing reads rng behind it.
// Losses: bhl_fwd_kernel (one wave per row, a lane per class, fp64 partials per workgroup),
// bhl_reduce_kernel (one workgroup, fixed order) and bhl_bwd_kernel (one wave per row: every
// element of both gradients stored once; no scatter, no memset, no atomics).
#include <algorithm>
#include <cmath>

#include "common.h"
#include "elem16.h"
#include "match_sample.h"
#include "radix_select.h"

namespace frcnn {
namespace {

constexpr int kBhMaxN = 1024;
constexpr int kBhMaxR = 4096;
constexpr int kBhMaxG = 256;
constexpr int kBhMaxB = 1024;
constexpr int kBhMaxM = kBhMaxR + kBhMaxG;
constexpr int kBhMaxC = 128;
constexpr int kBhThreads = 256;      // match
constexpr int kBhSelThreads = 1024;  // sample (hist_find's workgroup)
constexpr int kBhBins = 4096;
constexpr int kBhIdxBits = 13;       // candidate indices are below 2^13
constexpr int kBhPasses = 4;         // 12-bit digits of key << 13 | index (45 bits), from the top
constexpr int kBhMaxPer = (kBhMaxM + kBhSelThreads - 1) / kBhSelThreads;
static_assert(kBhMaxM <= (1 << kBhIdxBits), "candidate index bits");

enum : int8_t { kBhNeither = -1, kBhNeg = 0, kBhPos = 1 };

struct BhWs {
    uint32_t* keys;  // [N][M] the masked Philox key of every candidate
    int8_t* cls;     // [N][M] kBhPos / kBhNeg / kBhNeither
    size_t bytes;
};

BhWs bh_carve(void* ws, int N, int M) {
    Carver c(ws);
    BhWs w{};
    w.keys = c.take<uint32_t>(static_cast<size_t>(N) * M);
    w.cls = c.take<int8_t>(static_cast<size_t>(N) * M);
    w.bytes = c.used();
    return w;
}

struct BhWeights {
    float wx, wy, ww, wh;
};

__device__ __forceinline__ uint64_t bh_comp(uint32_t key, unsigned c) {
    return (static_cast<uint64_t>(key) << kBhIdxBits) | c;
}

__device__ __forceinline__ int bh_clamp(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

// -1 below bg, -2 between, else the gt index, -3 for an absent candidate
__global__ __launch_bounds__(kBhThreads) void bht_match_kernel(int R, int G, const float4* __restrict__ proposals,
                                                               const int32_t* __restrict__ prop_count,
                                                               const float4* __restrict__ gt,
                                                               const int32_t* __restrict__ gt_labels,
                                                               const int32_t* __restrict__ gt_count,
                                                               const int64_t* __restrict__ rng, float fg, float bg,
                                                               int add_gt, int key_bits, BhWs ws,
                                                               int32_t* __restrict__ matches) {
    __shared__ float4 sbox[kBhMaxG];
    __shared__ float sarea[kBhMaxG];
    const int n = blockIdx.y, tid = threadIdx.x;
    const int M = R + G;
    const int cnt = rt_load_gts(gt, gt_count, n, G, sbox, sarea);
    __syncthreads();
    const int c = blockIdx.x * kBhThreads + tid;
    if (c >= M) return;
    const int pc = bh_clamp(prop_count[n], R);
    float4 box;
    bool present;
    if (c < R) {
        present = c < pc;
        box = present ? proposals[static_cast<size_t>(n) * R + c] : make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        present = add_gt && sarea[c - R] >= 0.0f;
        box = sbox[c - R];
    }
    int m = -3;
    int8_t cls = kBhNeither;
    if (present) {
        const float area = (box.z - box.x) * (box.w - box.y);
        float best = -1.0f;
        int arg = -1;
        for (int j = 0; j < cnt; ++j) {
            const float ga = sarea[j];
            if (ga < 0.0f) continue;
            const float iou = rt_iou(sbox[j], ga, box, area);
            if (iou > best) {  // strict: the lowest index wins a tie
                best = iou;
                arg = j;
            }
        }
        m = -1;  // no present gt row: background
        if (arg >= 0) m = best < bg ? -1 : best < fg ? -2 : arg;
        const int label = m >= 0 ? gt_labels[static_cast<size_t>(n) * G + m] : m == -1 ? 0 : -1;
        cls = label >= 1 ? kBhPos : label == 0 ? kBhNeg : kBhNeither;
    }
    const size_t at = static_cast<size_t>(n) * M + c;
    matches[at] = m;
    ws.cls[at] = cls;
    ws.keys[at] = cls != kBhNeither ? RtKeyer(rng, key_bits)(static_cast<unsigned>(c), static_cast<unsigned>(n)) : 0u;
}

struct BhSelShared {
    RadixBin bin;
    unsigned wsum[16];
    unsigned tot[2];
};

__global__ __launch_bounds__(kBhSelThreads) void bht_sample_kernel(
    int R, int G, int B, int max_pos, const float4* __restrict__ proposals, const float4* __restrict__ gt,
    const int32_t* __restrict__ gt_labels, BhWeights wt, BhWs ws, const int32_t* __restrict__ matches,
    float* __restrict__ rois, int32_t* __restrict__ labels, int32_t* __restrict__ matched,
    float4* __restrict__ reg_targets, int32_t* __restrict__ samples, int32_t* __restrict__ n_pos,
    int32_t* __restrict__ n_neg, int64_t* rng) {
    __shared__ unsigned hist[kBhBins];
    __shared__ uint32_t skey[kBhMaxM];
    __shared__ int8_t scls[kBhMaxM];
    __shared__ BhSelShared sh;
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int M = R + G;
    const size_t base = static_cast<size_t>(n) * M;

    // the image's classes and keys to LDS; the class totals
    unsigned cp = 0, cn = 0;
    for (int c = tid; c < M; c += kBhSelThreads) {
        const int8_t k = ws.cls[base + c];
        scls[c] = k;
        skey[c] = ws.keys[base + c];
        cp += k == kBhPos;
        cn += k == kBhNeg;
    }
    cp = wave_reduce(cp, op_add{});
    cn = wave_reduce(cn, op_add{});
    if (lane == 0) hist[wid] = cp, hist[16 + wid] = cn;
    __syncthreads();
    if (tid < 2) {
        unsigned t = 0;
        for (int w = 0; w < kBhSelThreads / kWave; ++w) t += hist[16 * tid + w];
        sh.tot[tid] = t;
    }
    __syncthreads();
    const unsigned P = sh.tot[0], Ng = sh.tot[1];
    const unsigned num_pos = P < static_cast<unsigned>(max_pos) ? P : static_cast<unsigned>(max_pos);
    const unsigned room = static_cast<unsigned>(B) - num_pos;
    const unsigned num_neg = Ng < room ? Ng : room;

    // T[k]: the inclusive threshold on key << 13 | index of class k.  Every branch below depends on
    // LDS words only, so the workgroup stays together through hist_find's barriers and scans.
    uint64_t T[2];
#pragma unroll 1
    for (int k = 0; k < 2; ++k) {
        const unsigned num = k == 0 ? num_pos : num_neg, total = k == 0 ? P : Ng;
        const int8_t want = k == 0 ? kBhPos : kBhNeg;
        T[k] = ~0ull;  // the whole class
        if (num == 0u || num == total) continue;
        unsigned need = num;
        uint64_t prefix = 0ull, hm = 0ull;
        bool whole = false;
#pragma unroll 1
        for (int pass = 0; pass < kBhPasses && !whole; ++pass) {
            const int shift = 12 * (kBhPasses - 1 - pass);
            for (int i = tid; i < kBhBins; i += kBhSelThreads) hist[i] = 0u;
            __syncthreads();
            for (int c = tid; c < M; c += kBhSelThreads) {
                const uint64_t v = bh_comp(skey[c], static_cast<unsigned>(c));
                if (scls[c] == want && (v & hm) == prefix)
                    atomicAdd(&hist[static_cast<unsigned>(v >> shift) & (kBhBins - 1)], 1u);
            }
            __syncthreads();
            hist_find(hist, kBhBins, need, sh.bin, sh.wsum);
            need -= sh.bin.before;
            prefix |= static_cast<uint64_t>(sh.bin.digit) << shift;
            hm = ~0ull << shift;
            T[k] = prefix | ((1ull << shift) - 1ull);
            whole = sh.bin.bucket == need;
            __syncthreads();  // sh.bin consumed before the next pass rewrites it
        }
    }

    // slots in ascending candidate order: thread t owns candidates [t * per, (t + 1) * per)
    const int per = (M + kBhSelThreads - 1) / kBhSelThreads;
    const int c0 = tid * per;
    bool take[kBhMaxPer];
    unsigned mine = 0;
#pragma unroll
    for (int q = 0; q < kBhMaxPer; ++q) {
        const int c = c0 + q;
        take[q] = false;
        if (q < per && c < M) {
            const int8_t k = scls[c];
            const uint64_t v = bh_comp(skey[c], static_cast<unsigned>(c));
            take[q] = (k == kBhPos && num_pos != 0u && v <= T[0]) || (k == kBhNeg && num_neg != 0u && v <= T[1]);
        }
        mine += take[q];
    }
    const unsigned incl = wave_scan_incl(mine, op_add{});
    if (lane == 63) sh.wsum[wid] = incl;
    __syncthreads();
    unsigned slot = incl - mine;
    for (int w = 0; w < wid; ++w) slot += sh.wsum[w];
    const unsigned S = num_pos + num_neg;  // = the workgroup's sum of `mine`, at most B

    const size_t row0 = static_cast<size_t>(n) * B;
#pragma unroll
    for (int q = 0; q < kBhMaxPer; ++q) {
        if (!take[q] || slot >= static_cast<unsigned>(B)) continue;  // the second: never
        const int c = c0 + q;
        const size_t r = row0 + slot;
        ++slot;
        const float4 pb = c < R ? proposals[static_cast<size_t>(n) * R + c] : gt[static_cast<size_t>(n) * G + (c - R)];
        const bool pos = scls[c] == kBhPos;
        int m = 0, label = 0;
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (pos) {
            m = bh_clamp(matches[base + c], G - 1);
            label = gt_labels[static_cast<size_t>(n) * G + m];
            const float4 gb = gt[static_cast<size_t>(n) * G + m];
            const float w = pb.z - pb.x, h = pb.w - pb.y;
            const float cx = pb.x + 0.5f * w, cy = pb.y + 0.5f * h;
            const float gw = gb.z - gb.x, gh = gb.w - gb.y;
            const float gcx = gb.x + 0.5f * gw, gcy = gb.y + 0.5f * gh;
            t = make_float4((wt.wx * (gcx - cx)) / w, (wt.wy * (gcy - cy)) / h, wt.ww * rt_log_cr(gw / w),
                            wt.wh * rt_log_cr(gh / h));
        }
        float* ro = rois + r * 5;
        ro[0] = static_cast<float>(n);
        ro[1] = pb.x, ro[2] = pb.y, ro[3] = pb.z, ro[4] = pb.w;
        labels[r] = label;
        matched[r] = m;
        reg_targets[r] = t;
        samples[r] = c;
    }
    for (unsigned s = S + tid; s < static_cast<unsigned>(B); s += kBhSelThreads) {
        const size_t r = row0 + s;
        float* ro = rois + r * 5;
        ro[0] = -1.0f;
        ro[1] = 0.0f, ro[2] = 0.0f, ro[3] = 0.0f, ro[4] = 0.0f;
        labels[r] = -1;
        matched[r] = -1;
        reg_targets[r] = make_float4(0.f, 0.f, 0.f, 0.f);
        samples[r] = -1;
    }
    if (tid == 0) {
        n_pos[n] = static_cast<int32_t>(num_pos);
        n_neg[n] = static_cast<int32_t>(num_neg);
        if (n == 0) rng[1] = static_cast<int64_t>(static_cast<uint64_t>(rng[1]) + 1ull);
    }
}

int bh_check_shape(const char* who, int N, int R, int G, int B) {
    FRCNN_REQUIRE(N >= 1 && N <= kBhMaxN, "%s: N must be in [1, %d], got %d", who, kBhMaxN, N);
    FRCNN_REQUIRE(R >= 1 && R <= kBhMaxR, "%s: R must be in [1, %d], got %d", who, kBhMaxR, R);
    FRCNN_REQUIRE(G >= 1 && G <= kBhMaxG, "%s: G must be in [1, %d], got %d", who, kBhMaxG, G);
    FRCNN_REQUIRE(B >= 1 && B <= kBhMaxB, "%s: batch_size_per_image must be in [1, %d], got %d", who, kBhMaxB, B);
    return FRCNN_OK;
}

int bh_check_key_bits(const char* who, int key_bits) {
    FRCNN_REQUIRE(key_bits >= 0 && key_bits <= 32, "%s: key_bits must be in [0, 32], got %d", who, key_bits);
    return FRCNN_OK;
}

// ------------------------------------------------------------------- losses
constexpr int kBlThreads = 256;
constexpr int kBlWaves = kBlThreads / kWave;  // rows per workgroup and step
constexpr int kBlMaxBlocks = 2048;
constexpr int kBlPerLane = kBhMaxC / kWave;   // classes per lane

struct BlPartial {
    double cls, box;
    int32_t n_valid, n_pos, n_skipped, pad;
};

struct BlConsts {
    float beta, half_beta;
};

// A row's label: 0..C-1 for a valid slot, -1 for padding (or a negative label, which the
// targets op never writes into a valid slot), -2 for a valid slot whose label is >= C: skipped
// and counted, never used as an index.
__device__ __forceinline__ int bl_label(const int32_t* __restrict__ labels, const int32_t* __restrict__ n_pos,
                                        const int32_t* __restrict__ n_neg, int64_t r, int B, int C) {
    const int n = static_cast<int>(r / B), j = static_cast<int>(r - static_cast<int64_t>(n) * B);
    const int np = bh_clamp(n_pos[n], B);
    const int ng = bh_clamp(n_neg[n], B - np);
    if (j >= np + ng) return -1;
    const int l = labels[r];
    return l < 0 ? -1 : l >= C ? -2 : l;
}

// The wave's row: lane i holds classes i and i + 64.  max over the row (exact), e[q] =
// exp_cr(x - max), and their sum: each lane adds its own two in ascending class order, then the
// butterfly of wave_reduce (32 down to 1) leaves the same bits in every lane.
template <class E>
__device__ __forceinline__ void bl_softmax_terms(const typename E::raw* __restrict__ x, int C, int lane,
                                                 float (&v)[kBlPerLane], float (&e)[kBlPerLane], float& mx, float& sum) {
    float m = -INFINITY;
#pragma unroll
    for (int q = 0; q < kBlPerLane; ++q) {
        const int c = lane + q * kWave;
        v[q] = c < C ? E::widen(x[c]) : -INFINITY;
        m = v[q] > m ? v[q] : m;
    }
    m = wave_reduce(m, op_max{});
    float s = 0.0f;
#pragma unroll
    for (int q = 0; q < kBlPerLane; ++q) {
        const int c = lane + q * kWave;
        e[q] = c < C ? exp_cr(v[q] - m) : 0.0f;
        s = q == 0 ? e[q] : s + e[q];
    }
    mx = m;
    sum = wave_reduce(s, op_add{});
}

__device__ __forceinline__ void bl_block_sum(double& a, double& b, int& c, int& d, int& e) {
    __shared__ double sd[2][kBlWaves];
    __shared__ int si[3][kBlWaves];
    const int w = threadIdx.x / kWave;
    if (lane_id() == 0) sd[0][w] = a, sd[1][w] = b, si[0][w] = c, si[1][w] = d, si[2][w] = e;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 1; k < kBlWaves; ++k) a += sd[0][k], b += sd[1][k], c += si[0][k], d += si[1][k], e += si[2][k];
}

template <class E>
__global__ __launch_bounds__(kBlThreads) void bhl_fwd_kernel(int64_t rows, int B, int C,
                                                             const typename E::raw* __restrict__ cls,
                                                             const typename E::raw* __restrict__ reg,
                                                             const int32_t* __restrict__ labels,
                                                             const float* __restrict__ reg_t,
                                                             const int32_t* __restrict__ n_pos,
                                                             const int32_t* __restrict__ n_neg, BlConsts k,
                                                             BlPartial* __restrict__ part) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    double csum = 0.0, bsum = 0.0;  // lane 0's are the wave's
    int nv = 0, np = 0, ns = 0;
    const int64_t step = static_cast<int64_t>(gridDim.x) * kBlWaves;
    for (int64_t r = static_cast<int64_t>(blockIdx.x) * kBlWaves + wid; r < rows; r += step) {
        const int l = bl_label(labels, n_pos, n_neg, r, B, C);  // the same in every lane
        if (l == -2) ++ns;
        if (l < 0) continue;
        ++nv;
        float v[kBlPerLane], e[kBlPerLane], m, s;
        bl_softmax_terms<E>(cls + static_cast<size_t>(r) * C, C, lane, v, e, m, s);
        const float xl = E::widen(cls[static_cast<size_t>(r) * C + l]);
        csum += static_cast<double>(rt_log_cr(s) - (xl - m));
        if (l > 0) {
            ++np;
            float term = 0.0f;
            if (lane < 4) {
                const float z = fabsf(E::widen(reg[static_cast<size_t>(r) * 4 * C + 4 * l + lane]) - reg_t[r * 4 + lane]);
                term = z < k.beta ? 0.5f * z * z / k.beta : z - k.half_beta;
            }
            for (int j = 0; j < 4; ++j) bsum += static_cast<double>(__shfl(term, j, 64));
        }
    }
    bl_block_sum(csum, bsum, nv, np, ns);
    if (threadIdx.x == 0) part[blockIdx.x] = BlPartial{csum, bsum, nv, np, ns, 0};
}

__global__ __launch_bounds__(kBlThreads) void bhl_reduce_kernel(const BlPartial* __restrict__ part, int nparts,
                                                                float* __restrict__ loss, int32_t* __restrict__ stats) {
    double csum = 0.0, bsum = 0.0;
    int nv = 0, np = 0, ns = 0;
    for (int i = threadIdx.x; i < nparts; i += kBlThreads) {
        const BlPartial p = part[i];
        csum += p.cls, bsum += p.box, nv += p.n_valid, np += p.n_pos, ns += p.n_skipped;
    }
    csum = wave_reduce(csum, op_add{});
    bsum = wave_reduce(bsum, op_add{});
    nv = wave_reduce(nv, op_add{});
    np = wave_reduce(np, op_add{});
    ns = wave_reduce(ns, op_add{});
    bl_block_sum(csum, bsum, nv, np, ns);
    if (threadIdx.x == 0) {
        loss[0] = static_cast<float>(csum / static_cast<double>(nv));  // 0/0 = NaN, as torch's mean of nothing
        loss[1] = static_cast<float>(bsum / static_cast<double>(nv));
        stats[0] = nv, stats[1] = np, stats[2] = ns, stats[3] = 0;
    }
}

// One wave per row: the row's C elements of dclass_logits and 4C of dbox_regression.
template <class E>
__global__ __launch_bounds__(kBlThreads) void bhl_bwd_kernel(int64_t rows, int B, int C,
                                                             const typename E::raw* __restrict__ cls,
                                                             const typename E::raw* __restrict__ reg,
                                                             const int32_t* __restrict__ labels,
                                                             const float* __restrict__ reg_t,
                                                             const int32_t* __restrict__ n_pos,
                                                             const int32_t* __restrict__ n_neg, BlConsts k,
                                                             const int32_t* __restrict__ stats,
                                                             const float* __restrict__ g_cls,
                                                             const float* __restrict__ g_box,
                                                             typename E::raw* __restrict__ dcls,
                                                             typename E::raw* __restrict__ dreg) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t r = static_cast<int64_t>(blockIdx.x) * kBlWaves + wid;
    if (r >= rows) return;
    const int S = stats[0];
    // NULL upstream gradient = 0: that output is all +0 and its inputs are not read
    const bool do_cls = g_cls != nullptr && S > 0, do_box = g_box != nullptr && S > 0;
    const float scale_c = do_cls ? *g_cls / static_cast<float>(S) : 0.0f;
    const float scale_b = do_box ? *g_box / static_cast<float>(S) : 0.0f;
    const int l = bl_label(labels, n_pos, n_neg, r, B, C);
    typename E::raw* oc = dcls + static_cast<size_t>(r) * C;
    typename E::raw* ob = dreg + static_cast<size_t>(r) * 4 * C;
    if (l >= 0 && do_cls) {
        float v[kBlPerLane], e[kBlPerLane], m, s;
        bl_softmax_terms<E>(cls + static_cast<size_t>(r) * C, C, lane, v, e, m, s);
#pragma unroll
        for (int q = 0; q < kBlPerLane; ++q) {
            const int c = lane + q * kWave;
            if (c < C) oc[c] = E::narrow((e[q] / s - (c == l ? 1.0f : 0.0f)) * scale_c);
        }
    } else {
        for (int c = lane; c < C; c += kWave) oc[c] = E::narrow(0.0f);
    }
    const int lo = 4 * l;  // the label's four columns of a positive
    for (int c = lane; c < 4 * C; c += kWave) {
        float g = 0.0f;
        if (l > 0 && do_box && c >= lo && c < lo + 4) {
            const float d = E::widen(reg[static_cast<size_t>(r) * 4 * C + c]) - reg_t[r * 4 + (c - lo)];
            const float z = fabsf(d);
            g = (z < k.beta ? d / k.beta : (d > 0.0f ? 1.0f : d < 0.0f ? -1.0f : d)) * scale_b;
        }
        ob[c] = E::narrow(g);
    }
}

int bl_fwd_blocks(int64_t rows) {
    const int64_t b = (rows + kBlWaves - 1) / kBlWaves;
    return static_cast<int>(b < kBlMaxBlocks ? b : kBlMaxBlocks);
}

int bl_check(const char* who, int dtype, int N, int B, int C, double beta, BlConsts* k) {
    FRCNN_REQUIRE(dtype_code_ok(dtype), "%s: dtype must be FRCNN_F32, FRCNN_F16 or FRCNN_BF16, got %d", who, dtype);
    FRCNN_REQUIRE(N >= 1 && N <= kBhMaxN, "%s: N must be in [1, %d], got %d", who, kBhMaxN, N);
    FRCNN_REQUIRE(B >= 1 && B <= kBhMaxB, "%s: batch_size_per_image must be in [1, %d], got %d", who, kBhMaxB, B);
    FRCNN_REQUIRE(C >= 2 && C <= kBhMaxC, "%s: C must be in [2, %d], got %d", who, kBhMaxC, C);
    FRCNN_REQUIRE(std::isfinite(beta) && beta >= 0.0, "%s: beta=%g must be finite and not negative", who, beta);
    k->beta = static_cast<float>(beta);
    k->half_beta = 0.5f * k->beta;
    return FRCNN_OK;
}

template <class E>
void bl_launch_fwd(int nb, int64_t rows, int B, int C, const void* cls, const void* reg, const int32_t* labels,
                   const float* reg_t, const int32_t* n_pos, const int32_t* n_neg, BlConsts k, BlPartial* part,
                   hipStream_t st) {
    using raw = typename E::raw;
    hipLaunchKernelGGL((bhl_fwd_kernel<E>), dim3(nb), dim3(kBlThreads), 0, st, rows, B, C, static_cast<const raw*>(cls),
                       static_cast<const raw*>(reg), labels, reg_t, n_pos, n_neg, k, part);
}

template <class E>
void bl_launch_bwd(int64_t rows, int B, int C, const void* cls, const void* reg, const int32_t* labels,
                   const float* reg_t, const int32_t* n_pos, const int32_t* n_neg, BlConsts k, const int32_t* stats,
                   const float* g_cls, const float* g_box, void* dcls, void* dreg, hipStream_t st) {
    using raw = typename E::raw;
    const unsigned nb = static_cast<unsigned>((rows + kBlWaves - 1) / kBlWaves);
    hipLaunchKernelGGL((bhl_bwd_kernel<E>), dim3(nb), dim3(kBlThreads), 0, st, rows, B, C, static_cast<const raw*>(cls),
                       static_cast<const raw*>(reg), labels, reg_t, n_pos, n_neg, k, stats, g_cls, g_box,
                       static_cast<raw*>(dcls), static_cast<raw*>(dreg));
}

}  // namespace
}  // namespace frcnn

using namespace frcnn;

extern "C" size_t frcnn_box_head_targets_workspace_size(int N, int R, int G, int batch_size_per_image) {
    if (bh_check_shape("frcnn_box_head_targets_workspace_size", N, R, G, batch_size_per_image)) return 0;
    return bh_carve(nullptr, N, R + G).bytes;
}

extern "C" int frcnn_box_head_targets_kernel(int N, int R, int G, int batch_size_per_image, int key_bits, char* name,
                                             size_t len) {
    const char* who = "frcnn_box_head_targets_kernel";
    FRCNN_REQUIRE(name && len > 0, "%s: null name buffer", who);
    int rc = bh_check_shape(who, N, R, G, batch_size_per_image);
    if (rc) return rc;
    rc = bh_check_key_bits(who, key_bits);
    if (rc) return rc;
    const int M = R + G;
    const int blocks = (M + kBhThreads - 1) / kBhThreads;
    // the selection's passes depend on the data (a class taken whole needs none, a pass whose bucket is
    // taken whole is the last); the shape fixes the candidates per thread of the slot scan
    std::snprintf(name, len, "bht_match_kernel[M=%d,blocks=%d,tail=%d] bht_sample_kernel[per=%d,digits=%dx12]", M, blocks,
                  M - (blocks - 1) * kBhThreads, (M + kBhSelThreads - 1) / kBhSelThreads, kBhPasses);
    return FRCNN_OK;
}

extern "C" int frcnn_box_head_targets(const float* proposals, const int32_t* prop_count, int N, int R,
                                      const float* gt_boxes, const int32_t* gt_labels, const int32_t* gt_count, int G,
                                      int64_t* rng, int batch_size_per_image, double positive_fraction,
                                      double fg_iou_thresh, double bg_iou_thresh, double wx, double wy, double ww,
                                      double wh, int add_gt, int key_bits, float* rois, int32_t* labels,
                                      int32_t* matched, float* reg_targets, int32_t* samples, int32_t* n_pos,
                                      int32_t* n_neg, int32_t* matches, void* workspace, size_t ws_bytes, void* stream) {
    const char* who = "frcnn_box_head_targets";
    const int B = batch_size_per_image;
    int rc = bh_check_shape(who, N, R, G, B);
    if (rc) return rc;
    rc = bh_check_key_bits(who, key_bits);
    if (rc) return rc;
    FRCNN_REQUIRE(positive_fraction >= 0.0 && positive_fraction <= 1.0, "%s: positive_fraction=%g must be in [0, 1]", who,
                  positive_fraction);
    FRCNN_REQUIRE(bg_iou_thresh <= fg_iou_thresh, "%s: bg_iou_thresh=%g must not exceed fg_iou_thresh=%g", who,
                  bg_iou_thresh, fg_iou_thresh);
    const BhWeights wt{static_cast<float>(wx), static_cast<float>(wy), static_cast<float>(ww), static_cast<float>(wh)};
    FRCNN_REQUIRE(std::isfinite(wt.wx) && std::isfinite(wt.wy) && std::isfinite(wt.ww) && std::isfinite(wt.wh) &&
                      wt.wx > 0.0f && wt.wy > 0.0f && wt.ww > 0.0f && wt.wh > 0.0f,
                  "%s: reg_weights=(%g, %g, %g, %g) must be finite and positive", who, wx, wy, ww, wh);
    FRCNN_REQUIRE(proposals && prop_count && gt_boxes && gt_labels && gt_count && rng,
                  "%s: null input (proposals, prop_count, gt_boxes, gt_labels, gt_count, rng)", who);
    FRCNN_REQUIRE(rois && labels && matched && reg_targets && samples && n_pos && n_neg && matches,
                  "%s: null output pointer", who);
    FRCNN_REQUIRE(aligned_to(proposals, 16) && aligned_to(gt_boxes, 16) && aligned_to(reg_targets, 16) && aligned_to(rng, 8),
                  "%s: proposals, gt_boxes and reg_targets must be 16-byte aligned, rng 8-byte aligned", who);
    const int M = R + G;
    BhWs w = bh_carve(workspace, N, M);
    FRCNN_REQUIRE(workspace && ws_bytes >= w.bytes, "%s: workspace %zu < %zu", who, workspace ? ws_bytes : size_t{0},
                  w.bytes);
    FRCNN_REQUIRE(aligned_to(workspace, 256), "%s: workspace must be 256-byte aligned", who);
    const int max_pos = static_cast<int>(static_cast<double>(B) * positive_fraction);  // Python's int(B * fraction)
    const float fg = static_cast<float>(fg_iou_thresh), bg = static_cast<float>(bg_iou_thresh);
    hipStream_t st = as_stream(stream);
    const float4* pr = reinterpret_cast<const float4*>(proposals);
    const float4* gt = reinterpret_cast<const float4*>(gt_boxes);
    hipLaunchKernelGGL(bht_match_kernel, dim3((M + kBhThreads - 1) / kBhThreads, N), dim3(kBhThreads), 0, st, R, G, pr,
                       prop_count, gt, gt_labels, gt_count, rng, fg, bg, add_gt ? 1 : 0, key_bits, w, matches);
    FRCNN_LAUNCH_CHECK("bht_match_kernel");
    hipLaunchKernelGGL(bht_sample_kernel, dim3(N), dim3(kBhSelThreads), 0, st, R, G, B, max_pos, pr, gt, gt_labels, wt, w,
                       matches, rois, labels, matched, reinterpret_cast<float4*>(reg_targets), samples, n_pos, n_neg,
                       rng);
    FRCNN_LAUNCH_CHECK("bht_sample_kernel");
    return FRCNN_OK;
}

extern "C" size_t frcnn_box_head_losses_workspace_size(int N, int batch_size_per_image) {
    if (N < 1 || N > kBhMaxN || batch_size_per_image < 1 || batch_size_per_image > kBhMaxB) return 0;
    return align_up(static_cast<size_t>(bl_fwd_blocks(static_cast<int64_t>(N) * batch_size_per_image)) * sizeof(BlPartial),
                    256);
}

extern "C" int frcnn_box_head_losses_fwd_t(int dtype, const void* class_logits, const void* box_regression, int N,
                                           int batch_size_per_image, int C, const int32_t* labels,
                                           const float* reg_targets, const int32_t* n_pos, const int32_t* n_neg,
                                           double beta, float* loss, int32_t* stats, void* workspace, size_t ws_bytes,
                                           void* stream) {
    const char* who = "frcnn_box_head_losses_fwd_t";
    BlConsts k{};
    const int B = batch_size_per_image;
    int rc = bl_check(who, dtype, N, B, C, beta, &k);
    if (rc) return rc;
    FRCNN_REQUIRE(class_logits && box_regression, "%s: null input (class_logits, box_regression)", who);
    FRCNN_REQUIRE(labels && reg_targets && n_pos && n_neg, "%s: null input (labels, reg_targets, n_pos, n_neg)", who);
    FRCNN_REQUIRE(loss && stats, "%s: null output (loss, stats)", who);
    const size_t esz = dtype == FRCNN_F32 ? 4 : 2;
    FRCNN_REQUIRE(aligned_to(class_logits, esz) && aligned_to(box_regression, esz),
                  "%s: class_logits / box_regression not aligned to their element size", who);
    const size_t need = frcnn_box_head_losses_workspace_size(N, B);
    FRCNN_REQUIRE(workspace && ws_bytes >= need, "%s: workspace %zu < %zu", who, workspace ? ws_bytes : size_t{0}, need);
    FRCNN_REQUIRE(aligned_to(workspace, 256), "%s: workspace must be 256-byte aligned", who);
    hipStream_t st = as_stream(stream);
    BlPartial* part = static_cast<BlPartial*>(workspace);
    const int64_t rows = static_cast<int64_t>(N) * B;
    const int nb = bl_fwd_blocks(rows);
    if (dtype == FRCNN_F32)
        bl_launch_fwd<ElemF32>(nb, rows, B, C, class_logits, box_regression, labels, reg_targets, n_pos, n_neg, k, part, st);
    else if (dtype == FRCNN_F16)
        bl_launch_fwd<ElemF16>(nb, rows, B, C, class_logits, box_regression, labels, reg_targets, n_pos, n_neg, k, part, st);
    else
        bl_launch_fwd<ElemBF16>(nb, rows, B, C, class_logits, box_regression, labels, reg_targets, n_pos, n_neg, k, part, st);
    FRCNN_LAUNCH_CHECK("bhl_fwd_kernel");
    hipLaunchKernelGGL(bhl_reduce_kernel, dim3(1), dim3(kBlThreads), 0, st, part, nb, loss, stats);
    FRCNN_LAUNCH_CHECK("bhl_reduce_kernel");
    return FRCNN_OK;
}

extern "C" int frcnn_box_head_losses_bwd_t(int dtype, const void* class_logits, const void* box_regression, int N,
                                           int batch_size_per_image, int C, const int32_t* labels,
                                           const float* reg_targets, const int32_t* n_pos, const int32_t* n_neg,
                                           double beta, const int32_t* stats, const float* g_cls, const float* g_box,
                                           void* dclass_logits, void* dbox_regression, void* stream) {
    const char* who = "frcnn_box_head_losses_bwd_t";
    BlConsts k{};
    const int B = batch_size_per_image;
    int rc = bl_check(who, dtype, N, B, C, beta, &k);
    if (rc) return rc;
    FRCNN_REQUIRE(class_logits && box_regression && dclass_logits && dbox_regression,
                  "%s: null tensor (class_logits, box_regression, dclass_logits, dbox_regression)", who);
    FRCNN_REQUIRE(labels && reg_targets && n_pos && n_neg && stats,
                  "%s: null input (labels, reg_targets, n_pos, n_neg, stats)", who);
    const size_t esz = dtype == FRCNN_F32 ? 4 : 2;
    FRCNN_REQUIRE(aligned_to(class_logits, esz) && aligned_to(box_regression, esz) && aligned_to(dclass_logits, esz) &&
                      aligned_to(dbox_regression, esz),
                  "%s: tensors not aligned to their element size", who);
    hipStream_t st = as_stream(stream);
    const int64_t rows = static_cast<int64_t>(N) * B;
    if (dtype == FRCNN_F32)
        bl_launch_bwd<ElemF32>(rows, B, C, class_logits, box_regression, labels, reg_targets, n_pos, n_neg, k, stats, g_cls,
                               g_box, dclass_logits, dbox_regression, st);
    else if (dtype == FRCNN_F16)
        bl_launch_bwd<ElemF16>(rows, B, C, class_logits, box_regression, labels, reg_targets, n_pos, n_neg, k, stats, g_cls,
                               g_box, dclass_logits, dbox_regression, st);
    else
        bl_launch_bwd<ElemBF16>(rows, B, C, class_logits, box_regression, labels, reg_targets, n_pos, n_neg, k, stats, g_cls,
                                g_box, dclass_logits, dbox_regression, st);
    FRCNN_LAUNCH_CHECK("bhl_bwd_kernel");
    return FRCNN_OK;
}
