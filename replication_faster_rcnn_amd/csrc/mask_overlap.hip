// Mask overlap counts: for every considered (detection, gt) pair of an image the
// number of pixels set in both masks, and every mask's own pixel count (DESIGN.md
// "COCO segm evaluation" is the contract; tests/coco_segm_ref.py restates it).
// A pixel is set iff its byte is non-zero.  Two launches:
//   mo_pack_kernel<EDGES> : one workgroup per live mask (the detections below
//                           det_count, every gt).  A band of rows at a time:
//                           step one, lane = 16 bytes of a row (one aligned
//                           uint4 load; with EDGES item 0 of a row is its
//                           unaligned head and the last item its tail, read by
//                           bytes) -> a 16-bit pattern in LDS; step two, thread =
//                           one 64-bit word of the row, ORed from the at most
//                           six patterns that cover its 64 columns, stored once.
//                           The same threads keep the mask's pixel count and its
//                           window (first / last non-empty row and word column);
//                           one thread stores them and the mask's area output.
//   mo_pair_kernel        : one workgroup per (image, detection).  Thread = gt
//                           slot decides whether the pair is considered and
//                           stores the 0 of a pair that is not; the considered gt
//                           are listed in LDS and claimed by the waves from an
//                           LDS counter.  A pair whose windows do not intersect
//                           gets 0 without a read of the bits; otherwise the
//                           wave's lanes stride over the (row, word) cells of the
//                           intersection, popcount(a & b), a shuffle reduction,
//                           one store.
// Integers only; the one atomic is the LDS claim counter; every output element
// and every workspace word is stored at most once, so two calls give the same bits.
#include <cstdio>

#include "common.h"

namespace frcnn {

constexpr int kMoMaxN = 1024;
constexpr int kMoMaxD = 1024;
constexpr int kMoMaxG = 256;
constexpr int kMoMaxDim = 4096;
constexpr int kMoMaxC = 128;
constexpr int64_t kMoMaxPixels = int64_t{1} << 24;
constexpr int kMoThreads = 256;
constexpr int kMoWaves = kMoThreads / kWave;
constexpr int kMoStage = 4096;  // 16-bit patterns a band holds in LDS
constexpr int kMoMeta = 8;      // int32 per mask: pixel count, r0, r1, c0, c1 (half-open window; words for c)

static_assert(kMoMaxG <= kMoThreads, "thread = gt slot in mo_pair_kernel");

// Words per row of the packed mask.
__host__ __device__ inline int mo_words(int W) { return (W + 63) / 64; }
// Patterns per row: whole vectors, or a head, the vectors and a tail among them.
__host__ __device__ inline int mo_items(int W, bool edges) { return edges ? 1 + (W + 15) / 16 : W / 16; }
// Rows per band.
__host__ __device__ inline int mo_band(int items) { return items >= kMoStage ? 1 : kMoStage / items; }
inline bool mo_edges(int W) { return W % 16 != 0; }

struct op_min {
    template <class T> __device__ T operator()(T a, T b) const { return a < b ? a : b; }
};

// Bit j = byte j of the 16 bytes is non-zero (byte 0 at the lowest address).
__device__ __forceinline__ uint32_t mo_nonzero4(uint32_t x) {
    // the top bit of every byte that is not zero, then the four of them gathered (no two partial products meet)
    const uint32_t t = (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
    return (((t >> 7) * 0x00204081u) >> 21) & 0xFu;
}
__device__ __forceinline__ uint32_t mo_nonzero16(uint4 v) {
    return mo_nonzero4(v.x) | (mo_nonzero4(v.y) << 4) | (mo_nonzero4(v.z) << 8) | (mo_nonzero4(v.w) << 12);
}

__device__ __forceinline__ int mo_count(const int32_t* det_count, int n, int D) {
    if (!det_count) return D;
    const int k = det_count[n];
    return k < 0 ? 0 : (k > D ? D : k);
}

template <bool EDGES>
__global__ __launch_bounds__(kMoThreads) void mo_pack_kernel(int N, int D, int G, int H, int W,
                                                             const uint8_t* __restrict__ det_masks,
                                                             const uint8_t* __restrict__ gt_masks,
                                                             const int32_t* __restrict__ det_count,
                                                             int32_t* __restrict__ det_area,
                                                             int32_t* __restrict__ gt_area, int32_t* __restrict__ meta,
                                                             uint64_t* __restrict__ bits) {
    __shared__ unsigned short pat[kMoStage];
    __shared__ int red[kMoWaves][5];
    const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int nd = N * D;
    const uint8_t* src;
    int32_t* area_out;
    if (m < nd) {
        const int n = m / D, d = m - n * D;
        if (d >= mo_count(det_count, n, D)) {  // not a detection: an empty mask, never read
            if (tid == 0) det_area[m] = 0;
            if (tid < kMoMeta) meta[static_cast<size_t>(m) * kMoMeta + tid] = 0;
            return;
        }
        src = det_masks + static_cast<size_t>(m) * H * W;
        area_out = det_area + m;
    } else {
        src = gt_masks + static_cast<size_t>(m - nd) * H * W;
        area_out = gt_area + (m - nd);
    }
    const int wpr = mo_words(W), items = mo_items(W, EDGES), band = mo_band(items);
    constexpr int first = EDGES ? 1 : 0;  // a row's first vector item
    uint64_t* dst = bits + static_cast<size_t>(m) * H * wpr;
    int area = 0, r0 = H, r1 = 0, c0 = wpr, c1 = 0;
    for (int ya = 0; ya < H; ya += band) {
        const int rows = ya + band < H ? band : H - ya;
        // ---- step one: 16 bytes -> 16 bits
        for (int it = tid; it < rows * items; it += kMoThreads) {
            const int yr = it / items, k = it - yr * items;
            const uint8_t* rowp = src + static_cast<size_t>(ya + yr) * W;
            int xs = k * 16, xn = 16;
            if (EDGES) {
                int head = static_cast<int>((16u - (reinterpret_cast<uintptr_t>(rowp) & 15u)) & 15u);
                head = head < W ? head : W;
                xs = k == 0 ? 0 : head + (k - 1) * 16;
                xn = k == 0 ? head : 16;
                if (xs + xn > W) xn = W - xs;
            }
            uint32_t b = 0;
            if (xn == 16 && k >= first) {
                b = mo_nonzero16(*reinterpret_cast<const uint4*>(rowp + xs));  // 16-byte aligned
            } else {
                for (int j = 0; j < xn; ++j) b |= (rowp[xs + j] != 0 ? 1u : 0u) << j;
            }
            pat[it] = static_cast<unsigned short>(b);
        }
        __syncthreads();
        // ---- step two: the patterns of 64 columns -> one word
        for (int o = tid; o < rows * wpr; o += kMoThreads) {
            const int yr = o / wpr, w = o - yr * wpr;
            const unsigned short* pr = pat + yr * items;
            int head = 0;
            if (EDGES) {
                const uint8_t* rowp = src + static_cast<size_t>(ya + yr) * W;
                head = static_cast<int>((16u - (reinterpret_cast<uintptr_t>(rowp) & 15u)) & 15u);
                head = head < W ? head : W;
            }
            const int c = 64 * w;
            uint64_t word = (EDGES && w == 0) ? static_cast<uint64_t>(pr[0]) : 0ull;  // the head: columns 0..head-1
            // vector item j covers columns head + 16 j .. +15; a pattern has no bit at or past column W
            for (int j = c <= head ? 0 : (c - head) / 16; j < items - first && head + 16 * j < c + 64; ++j) {
                const int sh = head + 16 * j - c;  // -15 .. 63
                const uint64_t v = pr[first + j];
                word |= sh >= 0 ? v << sh : v >> -sh;
            }
            const int y = ya + yr;
            dst[static_cast<size_t>(y) * wpr + w] = word;
            if (word) {
                area += __popcll(word);
                r0 = y < r0 ? y : r0;
                r1 = y + 1 > r1 ? y + 1 : r1;
                c0 = w < c0 ? w : c0;
                c1 = w + 1 > c1 ? w + 1 : c1;
            }
        }
        __syncthreads();
    }
    area = wave_reduce(area, op_add{});
    r0 = wave_reduce(r0, op_min{});
    r1 = wave_reduce(r1, op_max{});
    c0 = wave_reduce(c0, op_min{});
    c1 = wave_reduce(c1, op_max{});
    if (lane == 0) {
        red[wid][0] = area;
        red[wid][1] = r0;
        red[wid][2] = r1;
        red[wid][3] = c0;
        red[wid][4] = c1;
    }
    __syncthreads();
    if (tid == 0) {
        for (int v = 1; v < kMoWaves; ++v) {
            area += red[v][0];
            r0 = red[v][1] < r0 ? red[v][1] : r0;
            r1 = red[v][2] > r1 ? red[v][2] : r1;
            c0 = red[v][3] < c0 ? red[v][3] : c0;
            c1 = red[v][4] > c1 ? red[v][4] : c1;
        }
        const bool empty = area == 0;
        int32_t* mt = meta + static_cast<size_t>(m) * kMoMeta;
        mt[0] = area;
        mt[1] = empty ? 0 : r0;
        mt[2] = empty ? 0 : r1;
        mt[3] = empty ? 0 : c0;
        mt[4] = empty ? 0 : c1;
        mt[5] = mt[6] = mt[7] = 0;
        *area_out = area;
    }
}

__global__ __launch_bounds__(kMoThreads) void mo_pair_kernel(int N, int D, int G, int H, int W, int C,
                                                             const int32_t* __restrict__ det_labels,
                                                             const int32_t* __restrict__ det_count,
                                                             const int32_t* __restrict__ gt_labels,
                                                             const int32_t* __restrict__ meta,
                                                             const uint64_t* __restrict__ bits,
                                                             int32_t* __restrict__ inter) {
    __shared__ int members[kMoMaxG];
    __shared__ int wcnt[kMoWaves];
    __shared__ int next_gt;
    const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int n = m / D, d = m - n * D;
    bool live = d < mo_count(det_count, n, D);
    int dl = 0;
    if (det_labels) {
        dl = det_labels[m];
        live = live && dl >= 1 && dl < C;
    }
    if (tid == 0) next_gt = 0;
    int32_t* out = inter + static_cast<size_t>(m) * G;
    bool is = false;
    if (tid < G) {
        is = live && (!det_labels || gt_labels[static_cast<size_t>(n) * G + tid] == dl);
        if (!is) out[tid] = 0;  // a pair that is not considered
    }
    const uint64_t bal = __ballot(is);
    if (lane == 0) wcnt[wid] = __popcll(bal);
    __syncthreads();
    int off = 0, total = 0;
    for (int v = 0; v < kMoWaves; ++v) {
        off += v < wid ? wcnt[v] : 0;
        total += wcnt[v];
    }
    if (is) members[off + __popcll(bal & lanemask_lt())] = tid;
    __syncthreads();
    total = __builtin_amdgcn_readfirstlane(total);  // the same in every lane; a scalar for the loop's exit
    if (total == 0) return;
    const int wpr = mo_words(W);
    const int32_t* ma = meta + static_cast<size_t>(m) * kMoMeta;
    const int a_r0 = ma[1], a_r1 = ma[2], a_c0 = ma[3], a_c1 = ma[4];
    const uint64_t* A = bits + static_cast<size_t>(m) * H * wpr;
    for (;;) {
        // The claim has no branch on the lane and comes back as a scalar.  With `if (lane == 0) j =
        // atomicAdd(..)` here and `if (lane == 0) out[g] = ..` at the loop's end the compiler threads the
        // other lanes from one test past the next, into an inner loop of their own in which lane 0 is
        // masked off and the broadcast of its claim reads 0 for ever.  Every lane adds, lane 0 adds 1, and
        // lane 0's return is the claim whatever order the lanes' adds take.
        __builtin_amdgcn_wave_barrier();
        const int j = __builtin_amdgcn_readfirstlane(atomicAdd(&next_gt, lane == 0 ? 1 : 0));
        if (j >= total) break;
        const int g = members[j];
        const size_t gm = static_cast<size_t>(N) * D + static_cast<size_t>(n) * G + g;
        const int32_t* mb = meta + gm * kMoMeta;
        const int ra = a_r0 > mb[1] ? a_r0 : mb[1], rb = a_r1 < mb[2] ? a_r1 : mb[2];
        const int ca = a_c0 > mb[3] ? a_c0 : mb[3], cb = a_c1 < mb[4] ? a_c1 : mb[4];
        int acc = 0;
        if (ra < rb && ca < cb) {  // wave-uniform; an empty window (0, 0) intersects nothing
            const uint64_t* B = bits + gm * H * wpr;
            const int nc = cb - ca, cells = (rb - ra) * nc;
            for (int idx = lane; idx < cells; idx += kWave) {
                const int r = idx / nc;
                const size_t at = static_cast<size_t>(ra + r) * wpr + ca + (idx - r * nc);
                acc += __popcll(A[at] & B[at]);
            }
            acc = wave_reduce(acc, op_add{});
        }
        if (lane == 0) out[g] = acc;
    }
}

struct MoWs {
    int32_t* meta;   // [N * (D + G)][kMoMeta]
    uint64_t* bits;  // [N * (D + G)][H][words]
    size_t bytes;
};

static MoWs carve_mo(void* ws, int N, int D, int G, int H, int W) {
    Carver c(ws);
    MoWs w{};
    const size_t masks = static_cast<size_t>(N) * (static_cast<size_t>(D) + G);
    w.meta = c.take<int32_t>(masks * kMoMeta);
    w.bits = c.take<uint64_t>(masks * H * mo_words(W));
    w.bytes = c.used();
    return w;
}

static bool mo_shape_ok(int N, int D, int G, int H, int W) {
    return N >= 1 && N <= kMoMaxN && D >= 1 && D <= kMoMaxD && G >= 0 && G <= kMoMaxG && H >= 1 && H <= kMoMaxDim &&
           W >= 1 && W <= kMoMaxDim && static_cast<int64_t>(H) * W <= kMoMaxPixels;
}

}  // namespace frcnn

using namespace frcnn;

extern "C" size_t frcnn_mask_overlap_workspace_size(int N, int D, int G, int H, int W) {
    if (!mo_shape_ok(N, D, G, H, W)) return 0;
    return carve_mo(nullptr, N, D, G, H, W).bytes;
}

extern "C" int frcnn_mask_overlap_plan(int N, int D, int G, int H, int W, int64_t plan[8]) {
    const char* who = "frcnn_mask_overlap_plan";
    FRCNN_REQUIRE(plan, "%s: null plan", who);
    FRCNN_REQUIRE(mo_shape_ok(N, D, G, H, W),
                  "%s: N=%d must be in [1, %d], D=%d in [1, %d], G=%d in [0, %d], H=%d and W=%d in [1, %d] with H*W <= "
                  "2^24", who, N, kMoMaxN, D, kMoMaxD, G, kMoMaxG, H, W, kMoMaxDim);
    const bool edges = mo_edges(W);
    const int items = mo_items(W, edges), band = mo_band(items);
    plan[0] = mo_words(W);
    plan[1] = edges ? 1 : 0;
    plan[2] = static_cast<int64_t>(N) * (D + G);
    plan[3] = static_cast<int64_t>(N) * D;
    plan[4] = static_cast<int64_t>(carve_mo(nullptr, N, D, G, H, W).bytes);
    plan[5] = items;
    plan[6] = band;
    plan[7] = (H + band - 1) / band;
    return FRCNN_OK;
}

extern "C" int frcnn_mask_overlap_kernel(int H, int W, char* name, size_t len) {
    const char* who = "frcnn_mask_overlap_kernel";
    FRCNN_REQUIRE(name && len > 0, "%s: null name buffer", who);
    FRCNN_REQUIRE(mo_shape_ok(1, 1, 0, H, W), "%s: H=%d and W=%d must be in [1, %d] with H*W <= 2^24", who, H, W,
                  kMoMaxDim);
    std::snprintf(name, len, "mo_pack_kernel[vec16%s]+mo_pair_kernel", mo_edges(W) ? "+edges" : "");
    return FRCNN_OK;
}

extern "C" int frcnn_mask_overlap(int N, int D, int G, int H, int W, int C, const uint8_t* det_masks,
                                  const uint8_t* gt_masks, const int32_t* det_labels, const int32_t* det_count,
                                  const int32_t* gt_labels, int32_t* inter, int32_t* det_area, int32_t* gt_area,
                                  void* ws, size_t ws_bytes, void* stream) {
    const char* who = "frcnn_mask_overlap";
    FRCNN_REQUIRE(mo_shape_ok(N, D, G, H, W),
                  "%s: N=%d must be in [1, %d], D=%d in [1, %d], G=%d in [0, %d], H=%d and W=%d in [1, %d] with H*W <= "
                  "2^24", who, N, kMoMaxN, D, kMoMaxD, G, kMoMaxG, H, W, kMoMaxDim);
    FRCNN_REQUIRE((det_labels == nullptr) == (gt_labels == nullptr) || G == 0,
                  "%s: det_labels and gt_labels are given together or not at all", who);
    FRCNN_REQUIRE(!det_labels || (C >= 2 && C <= kMoMaxC), "%s: n_class C=%d must be in [2, %d] with labels", who, C,
                  kMoMaxC);
    FRCNN_REQUIRE(det_masks && det_area, "%s: null pointer (det_masks / det_area)", who);
    FRCNN_REQUIRE(G == 0 || (gt_masks && gt_area && inter), "%s: null pointer (gt_masks / gt_area / inter)", who);
    FRCNN_REQUIRE((reinterpret_cast<uintptr_t>(det_masks) & 15u) == 0 && (reinterpret_cast<uintptr_t>(gt_masks) & 15u) == 0,
                  "%s: det_masks and gt_masks must be 16-byte aligned", who);
    const MoWs w = carve_mo(ws, N, D, G, H, W);
    if (!ws || ws_bytes < w.bytes) {
        set_error("%s: workspace %zu < %zu", who, ws ? ws_bytes : size_t{0}, w.bytes);
        return FRCNN_EWORKSPACE;
    }
    hipStream_t st = as_stream(stream);
    const int packs = N * (D + G);
    if (mo_edges(W))
        mo_pack_kernel<true><<<packs, kMoThreads, 0, st>>>(N, D, G, H, W, det_masks, gt_masks, det_count, det_area,
                                                           gt_area, w.meta, w.bits);
    else
        mo_pack_kernel<false><<<packs, kMoThreads, 0, st>>>(N, D, G, H, W, det_masks, gt_masks, det_count, det_area,
                                                            gt_area, w.meta, w.bits);
    FRCNN_LAUNCH_CHECK("mo_pack_kernel");
    if (G > 0) {
        mo_pair_kernel<<<N * D, kMoThreads, 0, st>>>(N, D, G, H, W, C, det_labels, det_count, gt_labels, w.meta,
                                                     w.bits, inter);
        FRCNN_LAUNCH_CHECK("mo_pair_kernel");
    }
    return FRCNN_OK;
}
