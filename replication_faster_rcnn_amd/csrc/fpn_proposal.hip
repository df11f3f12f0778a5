// FPN proposal layer on gfx950: torchvision's RegionProposalNetwork.filter_proposals
// with BoxCoder(weights=(1, 1, 1, 1)) over a feature pyramid (DESIGN.md §3 "FPN
// proposals"; include/frcnn_capi.h states the contract).  Four launches, no host sync:
//   fpn_select_decode_kernel<Elem>  one 1024-thread workgroup per (image, level): the
//       first P = min(pre, A_l) anchors in the stable descending order of the raw logit
//       (key = desc_score_key(logit) << 32 | anchor index; logits read in place from
//       NCHW in their own dtype), sorted in LDS, then decoded, clipped and filtered;
//       the survivors are compacted in rank order.  A level of at most kFpnSortCap
//       anchors is sorted whole ("sort"); a larger one goes through an exact radix
//       select that re-reads the logits once per digit ("select"; hist_find,
//       radix_select.h).  The LDS sort is this kernel's own: up to 2,048 keys at
//       every distance, not the 64-key wave stage of wave_sort64.
//   fpn_nms_mask_kernel   chip-wide 64x64 column-form IoU tiles of every (image, level)
//       (tile_rows16 / tile_word, nms_iou.h).
//   fpn_sweep_kernel      one workgroup per (image, level): greedy sweep in rank order
//       with the ballot fixed point, stopping at post kept boxes.
//   fpn_merge_kernel      one workgroup per image: rank of every kept box among the at
//       most L sorted kept lists by (logit desc, level asc, anchor asc), outputs and
//       padding.  No atomics on global memory, every output element stored once.
#include <cmath>

#include "common.h"
#include "elem16.h"
#include "nms_iou.h"
#include "radix_select.h"

namespace frcnn {
namespace {

constexpr int kFpnMaxLevels = 8;
constexpr int kFpnMaxK = 32;
constexpr int kFpnMaxPre = 2048;
constexpr int kFpnMaxPost = 4096;
constexpr int kFpnMaxN = 1024;
constexpr int kFpnMaxA = 1 << 24;   // exclusive: anchor indices and shifts stay exact in fp32
constexpr int kFpnSortCap = 2048;   // keys the LDS sort holds = the largest level sorted whole
constexpr int kFpnBins = 4096;
constexpr int kFpnThreads = 1024;

struct FpnLevels {
    const void* obj[kFpnMaxLevels];
    const void* del[kFpnMaxLevels];
    const float4* base[kFpnMaxLevels];
    int H[kFpnMaxLevels], W[kFpnMaxLevels], sh[kFpnMaxLevels], sw[kFpnMaxLevels];
};

// Per-(image, level) slot s = n * L + l of the workspace; cap = max_l min(pre, A_l).
struct FpnWs {
    float4* cbox;     // [S][cap] filtered candidates in rank order
    float* clogit;    // [S][cap]
    int32_t* cidx;    // [S][cap] anchor index within the level
    int* V;           // [S] candidates
    uint64_t* mask;   // [S][Wc][Wc][64] tile (cb, rb): bit i of lane j = row 64rb+i suppresses column 64cb+j
    uint32_t* kkey;   // [S][cap] desc_score_key of the kept boxes, sweep order
    int32_t* kslot;   // [S][cap] their candidate ranks
    int* kcount;      // [S]
    size_t bytes;
};

FpnWs fpn_carve(void* ws, int N, int L, int cap) {
    Carver c(ws);
    FpnWs w{};
    const size_t S = static_cast<size_t>(N) * L;
    const size_t Wc = (cap + 63) / 64;
    w.cbox = c.take<float4>(S * cap);
    w.clogit = c.take<float>(S * cap);
    w.cidx = c.take<int32_t>(S * cap);
    w.V = c.take<int>(S);
    w.mask = c.take<uint64_t>(S * Wc * Wc * 64);
    w.kkey = c.take<uint32_t>(S * cap);
    w.kslot = c.take<int32_t>(S * cap);
    w.kcount = c.take<int>(S);
    w.bytes = c.used();
    return w;
}

struct FpnSelShared {
    RadixBin bin;
    unsigned ccount;
    unsigned wsum[16];
    unsigned vsum[2][16];
};

// Key of the logit at memory offset m = k * HW + cell of one image's [K, H, W] map:
// anchor a = cell * K + k in the low word.
template <class E>
__device__ __forceinline__ uint64_t fpn_key(const typename E::raw* __restrict__ obj, unsigned m, unsigned HW,
                                            unsigned K) {
    const unsigned k = m / HW, cell = m - k * HW;
    return (static_cast<uint64_t>(desc_score_key(E::widen(obj[m]))) << 32) | (cell * K + k);
}

template <class E>
__global__ __launch_bounds__(kFpnThreads) void fpn_select_decode_kernel(FpnLevels g, int L, int K, int pre, int cap,
                                                                         const float* __restrict__ img_sizes,
                                                                         float logit_thr, float min_size, float dclip, FpnWs ws) {
    using raw = typename E::raw;
    __shared__ unsigned hist[kFpnBins];
    __shared__ uint64_t skey[kFpnSortCap];
    __shared__ FpnSelShared sh;
    const int l = blockIdx.x, n = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int H = g.H[l], W = g.W[l];
    const unsigned HW = static_cast<unsigned>(H) * W;
    const unsigned A = HW * K;
    const int P = A < static_cast<unsigned>(pre) ? static_cast<int>(A) : pre;
    const raw* __restrict__ obj = static_cast<const raw*>(g.obj[l]) + static_cast<size_t>(n) * A;
    const raw* __restrict__ del = static_cast<const raw*>(g.del[l]) + static_cast<size_t>(n) * A * 4;

    int count;  // keys in skey
    if (A <= static_cast<unsigned>(kFpnSortCap)) {  // "sort": the whole level
        for (unsigned i = tid; i < A; i += kFpnThreads) skey[i] = fpn_key<E>(obj, i, HW, K);
        count = static_cast<int>(A);
    } else {  // "select": the P-th smallest key by radix select, digits 12/12/8 of the score, 12/12 of the index
        uint64_t prefix = 0, hm = 0, T = 0;
        unsigned need = static_cast<unsigned>(P);
#pragma unroll 1
        for (int pass = 0; pass < 5; ++pass) {
            const int width = pass == 2 ? 8 : 12;
            const int shift = pass == 0 ? 52 : pass == 1 ? 40 : pass == 2 ? 32 : pass == 3 ? 12 : 0;
            const int nbins = 1 << width;
            for (int i = tid; i < nbins; i += kFpnThreads) hist[i] = 0;
            __syncthreads();
            for (unsigned m = tid; m < A; m += kFpnThreads) {
                const uint64_t key = fpn_key<E>(obj, m, HW, K);
                if ((key & hm) == prefix) atomicAdd(&hist[static_cast<unsigned>(key >> shift) & (nbins - 1)], 1u);
            }
            __syncthreads();
            hist_find(hist, nbins, need, sh.bin, sh.wsum);
            need -= sh.bin.before;
            prefix |= static_cast<uint64_t>(sh.bin.digit) << shift;
            hm = ~0ull << shift;
            T = prefix | ((1ull << shift) - 1ull);
            const bool whole = sh.bin.bucket == need;  // every key of the bucket is selected
            __syncthreads();                       // sh.* consumed before the next pass rewrites them
            if (whole) break;
        }
        if (tid == 0) sh.ccount = 0;
        __syncthreads();
        for (unsigned m = tid; m < A; m += kFpnThreads) {
            const uint64_t key = fpn_key<E>(obj, m, HW, K);
            if (key <= T) {
                const unsigned at = atomicAdd(&sh.ccount, 1u);
                if (at < static_cast<unsigned>(kFpnSortCap)) skey[at] = key;  // exactly P keys: they are distinct
            }
        }
        count = P;
    }
    int ns = 64;
    while (ns < count) ns <<= 1;  // <= kFpnSortCap
    for (int i = count + tid; i < ns; i += kFpnThreads) skey[i] = ~0ull;
    __syncthreads();
    for (int kk = 2; kk <= ns; kk <<= 1) {  // bitonic sort, ascending
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < ns; i += kFpnThreads) {
                const int o = i ^ j;
                if (o > i) {
                    const uint64_t a = skey[i], b = skey[o];
                    if ((a > b) == ((i & kk) == 0)) {
                        skey[i] = b;
                        skey[o] = a;
                    }
                }
            }
            __syncthreads();
        }
    }

    // decode, clip and filter the first P keys; survivors keep their rank order
    const float img_h = img_sizes[2 * n], img_w = img_sizes[2 * n + 1];
    float4 bx[2];
    float lg[2];
    int32_t ai[2];
    bool ok[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int r = tid + q * kFpnThreads;
        ok[q] = false;
        bx[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        lg[q] = 0.f;
        ai[q] = 0;
        const unsigned a = r < P ? static_cast<uint32_t>(skey[r]) : A;
        if (a < A) {  // always, for r < P: the first P keys are valid
            const unsigned cell = a / K, k = a - cell * K;
            const unsigned y = cell / W, x = cell - y * W;
            const float logit = E::widen(obj[k * HW + cell]);
            const raw* d = del + static_cast<size_t>(4 * k) * HW + cell;
            const float dx = E::widen(d[0]), dy = E::widen(d[HW]);
            float dw = E::widen(d[2 * static_cast<size_t>(HW)]), dh = E::widen(d[3 * static_cast<size_t>(HW)]);
            const float4 bb = g.base[l][k];
            const float sx = static_cast<float>(static_cast<int>(x) * g.sw[l]);
            const float sy = static_cast<float>(static_cast<int>(y) * g.sh[l]);
            const float ax1 = bb.x + sx, ay1 = bb.y + sy, ax2 = bb.z + sx, ay2 = bb.w + sy;
            const float aw = ax2 - ax1, ah = ay2 - ay1;
            const float acx = ax1 + 0.5f * aw, acy = ay1 + 0.5f * ah;
            dw = dw > dclip ? dclip : dw;  // torch.clamp(max=): NaN stays
            dh = dh > dclip ? dclip : dh;
            float pcx = dx * aw;
            pcx = pcx + acx;
            float pcy = dy * ah;
            pcy = pcy + acy;
            const float pw = exp_cr(dw) * aw, ph = exp_cr(dh) * ah;
            const float hw = 0.5f * pw, hh = 0.5f * ph;
            float4 b = make_float4(pcx - hw, pcy - hh, pcx + hw, pcy + hh);
            b.x = clamp_nan(b.x, 0.0f, img_w);
            b.z = clamp_nan(b.z, 0.0f, img_w);
            b.y = clamp_nan(b.y, 0.0f, img_h);
            b.w = clamp_nan(b.w, 0.0f, img_h);
            ok[q] = (b.z - b.x >= min_size) && (b.w - b.y >= min_size) && (logit >= logit_thr);
            bx[q] = b;
            lg[q] = logit;
            ai[q] = static_cast<int32_t>(a);
        }
        const uint64_t vb = __ballot(ok[q]);
        if (lane == 0) sh.vsum[q][wid] = static_cast<unsigned>(__popcll(vb));
    }
    __syncthreads();
    const size_t slot = static_cast<size_t>(n) * L + l;
    unsigned run = 0;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        unsigned off = run;
        for (int w = 0; w < 16; ++w) {
            if (w < wid) off += sh.vsum[q][w];
            run += sh.vsum[q][w];
        }
        const uint64_t vb = __ballot(ok[q]);
        if (ok[q]) {
            const size_t at = slot * cap + off + __popcll(vb & lanemask_lt());  // < P <= cap
            ws.cbox[at] = bx[q];
            ws.clogit[at] = lg[q];
            ws.cidx[at] = ai[q];
        }
    }
    if (tid == 0) ws.V[slot] = static_cast<int>(run);
}

// Tile (row block blockIdx.x, column block blockIdx.y) of slot blockIdx.z; 256 threads:
// lane = column, the rows split over the four waves (tile_rows16 / tile_word).
__global__ __launch_bounds__(256) void fpn_nms_mask_kernel(FpnWs ws, int cap, int Wc, NmsThr thr) {
    const int rb = blockIdx.x, cb = blockIdx.y;
    if (rb > cb) return;
    const size_t slot = blockIdx.z;
    const int V = min(ws.V[slot], cap);
    if (cb * 64 >= V) return;  // rb <= cb: the row block holds candidates too
    const float4* cbox = ws.cbox + slot * cap;
    __shared__ float4 rbox[64];
    __shared__ float rarea[64];
    __shared__ uint64_t part[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int i0 = rb * 64;
    if (tid < 64 && i0 + tid < V) {
        const float4 b = cbox[i0 + tid];
        rbox[tid] = b;
        rarea[tid] = box_area(b);
    }
    const int j = cb * 64 + lane;
    const bool jv = j < V;
    const float4 bj = jv ? cbox[j] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float aj = box_area(bj);
    __syncthreads();
    const int iend = jv ? min(min(64, V - i0), j - i0) : 0;  // rows before column j
    const uint64_t word = tile_word(part, wid, lane, tile_rows16(rbox, rarea, wid, iend, ~0ull, bj, aj, thr));
    if (wid == 0 && jv) ws.mask[((slot * Wc + cb) * Wc + rb) * 64 + lane] = word;
}

// Greedy sweep of one (image, level) in rank order.  Thread t owns columns t and t + 1024
// (blocks wid and wid + 16).  Block b is resolved by wave b & 15: avail = its columns not hit
// by a kept row of an earlier block, then the fixed point K <- avail & ballot(diag & K == 0)
// (unique, = the greedy result), cut to the room left below post; every wave then folds K
// into the hit flags of its later columns from the tile words of row block b, which were
// loaded one block ahead.
__global__ __launch_bounds__(kFpnThreads) void fpn_sweep_kernel(FpnWs ws, int cap, int Wc, int post) {
    __shared__ uint64_t s_K[2];
    const size_t slot = blockIdx.x;
    const int V = min(ws.V[slot], cap);
    const int nb = (V + 63) / 64;  // <= Wc <= 32
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const uint64_t* mask = ws.mask + slot * Wc * Wc * 64;
    const int cbq[2] = {wid, wid + 16};
    bool hit[2] = {false, false};
    uint64_t diag[2] = {0ull, 0ull}, nxt[2] = {0ull, 0ull};
    uint32_t key[2] = {0u, 0u};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int j = cbq[q] * 64 + lane;
        if (j < V) {
            diag[q] = mask[(static_cast<size_t>(cbq[q]) * Wc + cbq[q]) * 64 + lane];
            key[q] = desc_score_key(ws.clogit[slot * cap + j]);
            if (cbq[q] > 0) nxt[q] = mask[(static_cast<size_t>(cbq[q]) * Wc + 0) * 64 + lane];
        }
    }
    int kcount = 0;
#pragma unroll 1
    for (int b = 0; b < nb && kcount < post; ++b) {
        const uint64_t cur[2] = {nxt[0], nxt[1]};
#pragma unroll
        for (int q = 0; q < 2; ++q) {  // the words of row block b + 1, in flight over the barrier
            const int j = cbq[q] * 64 + lane;
            if (j < V && cbq[q] > b + 1) nxt[q] = mask[(static_cast<size_t>(cbq[q]) * Wc + b + 1) * 64 + lane];
        }
        if (wid == (b & 15)) {
            const int q = b >> 4;
            const int j = b * 64 + lane;
            const bool h = q ? hit[1] : hit[0];
            const uint64_t dg = q ? diag[1] : diag[0];
            const uint64_t avail = __ballot(j < V && !h);
            uint64_t Kb = avail;
            for (int it = 0; it < 65; ++it) {
                const uint64_t Kn = avail & __ballot((dg & Kb) == 0ull);
                if (Kn == Kb) break;
                Kb = Kn;
            }
            Kb = first_bits(Kb, post - kcount);
            if ((Kb >> lane) & 1ull) {
                const size_t at = slot * cap + kcount + __popcll(Kb & lanemask_lt());  // kept <= V <= cap
                ws.kkey[at] = q ? key[1] : key[0];
                ws.kslot[at] = j;
            }
            if (lane == 0) s_K[b & 1] = Kb;
        }
        __syncthreads();
        const uint64_t Kb = s_K[b & 1];
        kcount += __popcll(Kb);
#pragma unroll
        for (int q = 0; q < 2; ++q)
            if (cbq[q] > b && (cur[q] & Kb) != 0ull) hit[q] = true;
    }
    if (tid == 0) ws.kcount[slot] = kcount;
}

// One workgroup per image: the kept lists of its levels are sorted by (key, anchor); the rank
// of a kept box of level l is its position plus, per other level, the boxes there that precede
// it -- keys <= its key in a lower level, keys < its key in a higher one.
__global__ __launch_bounds__(kFpnThreads) void fpn_merge_kernel(FpnWs ws, int L, int cap, int post,
                                                                 float4* __restrict__ boxes, float* __restrict__ logits,
                                                                 int32_t* __restrict__ levels,
                                                                 int32_t* __restrict__ anchor_idx,
                                                                 int32_t* __restrict__ count, float* __restrict__ rois) {
    extern __shared__ __attribute__((aligned(16))) uint32_t skeys[];  // [L][cap]
    __shared__ int s_cnt[kFpnMaxLevels];
    const int n = blockIdx.x, tid = threadIdx.x;
    if (tid < L) s_cnt[tid] = max(0, min(ws.kcount[static_cast<size_t>(n) * L + tid], cap));
    __syncthreads();
    int total = 0;
    for (int l = 0; l < L; ++l) {
        const int c = s_cnt[l];
        const size_t slot = static_cast<size_t>(n) * L + l;
        for (int p = tid; p < c; p += kFpnThreads) skeys[l * cap + p] = ws.kkey[slot * cap + p];
        total += c;
    }
    __syncthreads();
    for (int l = 0; l < L; ++l) {
        const int c = s_cnt[l];
        const size_t slot = static_cast<size_t>(n) * L + l;
        for (int p = tid; p < c; p += kFpnThreads) {
            const uint32_t ke = skeys[l * cap + p];
            int rank = p;
            for (int o = 0; o < L; ++o) {
                if (o == l) continue;
                // # of keys before ke: <= in a lower level (ke + 1 does not wrap: keys stay below
                // 0xFFFFFFFF), < in a higher one
                rank += count_before(skeys + o * cap, s_cnt[o], o < l ? ke + 1 : ke);
            }
            if (rank < post) {
                const size_t src = slot * cap + min(static_cast<unsigned>(ws.kslot[slot * cap + p]), cap - 1u);
                const size_t at = static_cast<size_t>(n) * post + rank;
                const float4 b = ws.cbox[src];
                boxes[at] = b;
                logits[at] = ws.clogit[src];
                levels[at] = l;
                anchor_idx[at] = ws.cidx[src];
                float* r = rois + at * 5;
                r[0] = static_cast<float>(n);
                r[1] = b.x;
                r[2] = b.y;
                r[3] = b.z;
                r[4] = b.w;
            }
        }
    }
    const int kept = total < post ? total : post;
    for (int s = kept + tid; s < post; s += kFpnThreads) {
        const size_t at = static_cast<size_t>(n) * post + s;
        boxes[at] = make_float4(0.f, 0.f, 0.f, 0.f);
        logits[at] = -INFINITY;
        levels[at] = -1;
        anchor_idx[at] = -1;
        float* r = rois + at * 5;
        r[0] = -1.0f;
        r[1] = r[2] = r[3] = r[4] = 0.0f;
    }
    if (tid == 0) count[n] = kept;
}

// Shape checks shared by the three entry points; cap_out = max_l min(pre, A_l).
int fpn_check_shape(const char* who, int L, int N, int K, const int* H, const int* W, int pre, int post, int* cap_out) {
    FRCNN_REQUIRE(L >= 1 && L <= kFpnMaxLevels, "%s: n_levels must be in [1, %d], got %d", who, kFpnMaxLevels, L);
    FRCNN_REQUIRE(N >= 1 && N <= kFpnMaxN, "%s: N must be in [1, %d], got %d", who, kFpnMaxN, N);
    FRCNN_REQUIRE(K >= 1 && K <= kFpnMaxK, "%s: K must be in [1, %d], got %d", who, kFpnMaxK, K);
    FRCNN_REQUIRE(H && W, "%s: null H / W", who);
    FRCNN_REQUIRE(pre >= 1 && pre <= kFpnMaxPre, "%s: pre_nms_top_n must be in [1, %d], got %d", who, kFpnMaxPre, pre);
    FRCNN_REQUIRE(post >= 1 && post <= kFpnMaxPost, "%s: post_nms_top_n must be in [1, %d], got %d", who, kFpnMaxPost,
                  post);
    int cap = 0;
    for (int l = 0; l < L; ++l) {
        FRCNN_REQUIRE(H[l] >= 1 && W[l] >= 1, "%s: level %d is %d x %d; H and W must be >= 1", who, l, H[l], W[l]);
        const int64_t A = static_cast<int64_t>(K) * H[l] * W[l];
        FRCNN_REQUIRE(A < kFpnMaxA, "%s: level %d has %lld anchors; K*H*W must be below 2^24", who, l,
                      static_cast<long long>(A));
        const int P = A < pre ? static_cast<int>(A) : pre;
        cap = P > cap ? P : cap;
    }
    *cap_out = cap;
    return FRCNN_OK;
}

template <class E>
void fpn_launch_select(const FpnLevels& g, int L, int N, int K, int pre, int cap, const float* img, float thr,
                       float min_size, const FpnWs& w, hipStream_t st) {
    const float dclip = static_cast<float>(std::log(1000.0 / 16.0));  // torchvision's bbox_xform_clip
    hipLaunchKernelGGL((fpn_select_decode_kernel<E>), dim3(L, N), dim3(kFpnThreads), 0, st, g, L, K, pre, cap, img,
                       thr, min_size, dclip, w);
}

}  // namespace
}  // namespace frcnn

using namespace frcnn;

extern "C" size_t frcnn_propose_multi_workspace_size(int n_levels, int N, int K, const int* H, const int* W,
                                                     int pre_nms, int post_nms) {
    int cap = 0;
    if (fpn_check_shape("frcnn_propose_multi_workspace_size", n_levels, N, K, H, W, pre_nms, post_nms, &cap)) return 0;
    return fpn_carve(nullptr, N, n_levels, cap).bytes;
}

extern "C" int frcnn_propose_multi_kernel(int dtype, int n_levels, int N, int K, const int* H, const int* W,
                                          int pre_nms, int post_nms, char* name, size_t len) {
    FRCNN_REQUIRE(name && len > 0, "frcnn_propose_multi_kernel: null name buffer");
    FRCNN_REQUIRE(dtype_code_ok(dtype), "frcnn_propose_multi_kernel: dtype must be FRCNN_F32, FRCNN_F16 or FRCNN_BF16");
    int cap = 0;
    int rc = fpn_check_shape("frcnn_propose_multi_kernel", n_levels, N, K, H, W, pre_nms, post_nms, &cap);
    if (rc) return rc;
    std::string s = std::string("fpn_select_decode_kernel<") +
                    (dtype == FRCNN_F32 ? "ElemF32" : dtype == FRCNN_F16 ? "ElemF16" : "ElemBF16") + ">[";
    for (int l = 0; l < n_levels; ++l) {
        const int64_t A = static_cast<int64_t>(K) * H[l] * W[l];
        s += A <= kFpnSortCap ? "sort" : "select";
        s += l + 1 < n_levels ? "," : "]";
    }
    s += " fpn_nms_mask_kernel fpn_sweep_kernel fpn_merge_kernel";
    std::snprintf(name, len, "%s", s.c_str());
    return FRCNN_OK;
}

extern "C" int frcnn_propose_multi_t(int dtype, int n_levels, const void* const* objectness,
                                     const void* const* deltas, const float* const* anchor_bases, const int* H,
                                     const int* W, const int* stride_h, const int* stride_w, int N, int K,
                                     const float* image_sizes, int pre_nms, int post_nms, double nms_thresh,
                                     float logit_thresh, float min_size, float* boxes, float* logits,
                                     int32_t* levels, int32_t* anchor_idx, int32_t* count, float* rois,
                                     void* workspace, size_t ws_bytes, void* stream) {
    const char* who = "frcnn_propose_multi_t";
    FRCNN_REQUIRE(dtype_code_ok(dtype), "%s: dtype must be FRCNN_F32, FRCNN_F16 or FRCNN_BF16, got %d", who, dtype);
    int cap = 0;
    int rc = fpn_check_shape(who, n_levels, N, K, H, W, pre_nms, post_nms, &cap);
    if (rc) return rc;
    FRCNN_REQUIRE(objectness && deltas && anchor_bases && stride_h && stride_w,
                  "%s: null per-level array (objectness, deltas, anchor_bases, stride_h, stride_w)", who);
    FRCNN_REQUIRE(image_sizes, "%s: null image_sizes", who);
    FRCNN_REQUIRE(boxes && logits && levels && anchor_idx && count && rois, "%s: null output pointer", who);
    FpnLevels g{};
    const size_t esz = dtype == FRCNN_F32 ? 4 : 2;
    for (int l = 0; l < n_levels; ++l) {
        FRCNN_REQUIRE(objectness[l] && deltas[l] && anchor_bases[l], "%s: null pointer at level %d", who, l);
        FRCNN_REQUIRE(aligned_to(objectness[l], esz) && aligned_to(deltas[l], esz),
                      "%s: objectness / deltas of level %d not aligned to their element size", who, l);
        FRCNN_REQUIRE(aligned_to(anchor_bases[l], 16), "%s: anchor_bases[%d] must be 16-byte aligned", who, l);
        FRCNN_REQUIRE(stride_h[l] >= 1 && stride_w[l] >= 1, "%s: strides of level %d must be >= 1", who, l);
        FRCNN_REQUIRE(static_cast<int64_t>(H[l] - 1) * stride_h[l] < kFpnMaxA &&
                          static_cast<int64_t>(W[l] - 1) * stride_w[l] < kFpnMaxA,
                      "%s: level %d: (H-1)*stride_h and (W-1)*stride_w must be below 2^24", who, l);
        g.obj[l] = objectness[l];
        g.del[l] = deltas[l];
        g.base[l] = reinterpret_cast<const float4*>(anchor_bases[l]);
        g.H[l] = H[l];
        g.W[l] = W[l];
        g.sh[l] = stride_h[l];
        g.sw[l] = stride_w[l];
    }
    FRCNN_REQUIRE(aligned_to(boxes, 16), "%s: boxes must be 16-byte aligned", who);
    FpnWs w = fpn_carve(workspace, N, n_levels, cap);
    FRCNN_REQUIRE(workspace && ws_bytes >= w.bytes, "%s: workspace %zu < %zu", who, ws_bytes, w.bytes);
    FRCNN_REQUIRE(aligned_to(workspace, 256), "%s: workspace must be 256-byte aligned", who);
    hipStream_t st = as_stream(stream);
    const int L = n_levels, Wc = (cap + 63) / 64;
    if (dtype == FRCNN_F32)
        fpn_launch_select<ElemF32>(g, L, N, K, pre_nms, cap, image_sizes, logit_thresh, min_size, w, st);
    else if (dtype == FRCNN_F16)
        fpn_launch_select<ElemF16>(g, L, N, K, pre_nms, cap, image_sizes, logit_thresh, min_size, w, st);
    else
        fpn_launch_select<ElemBF16>(g, L, N, K, pre_nms, cap, image_sizes, logit_thresh, min_size, w, st);
    FRCNN_LAUNCH_CHECK("fpn_select_decode_kernel");
    hipLaunchKernelGGL(fpn_nms_mask_kernel, dim3(Wc, Wc, N * L), dim3(256), 0, st, w, cap, Wc, make_thr(nms_thresh));
    FRCNN_LAUNCH_CHECK("fpn_nms_mask_kernel");
    hipLaunchKernelGGL(fpn_sweep_kernel, dim3(N * L), dim3(kFpnThreads), 0, st, w, cap, Wc, post_nms);
    FRCNN_LAUNCH_CHECK("fpn_sweep_kernel");
    hipLaunchKernelGGL(fpn_merge_kernel, dim3(N), dim3(kFpnThreads), static_cast<size_t>(L) * cap * sizeof(uint32_t),
                       st, w, L, cap, post_nms, reinterpret_cast<float4*>(boxes), logits, levels, anchor_idx, count,
                       rois);
    FRCNN_LAUNCH_CHECK("fpn_merge_kernel");
    return FRCNN_OK;
}
