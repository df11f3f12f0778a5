// Proposal layer (nets/rpn.py:47-79) and torchvision-style NMS on gfx950.
//
// decode_filter: anchors (generated in-register) + deltas -> decoded, clamped
// boxes; min-size mask; 64-bit sort key (desc score : anchor index) --
// nets/rpn.py:58-68.  Then one of two paths, batched over images:
//   fused (many images / small post_nms): one 1024-thread workgroup per image
//     selects, sorts and suppresses 1024-candidate chunks on chip (below);
//   wide (few images, large pre/post_nms: cfg1, cfg4, the nms op):
//     run_sort + merge_rank + rank_scatter -- every key sorted chip-wide,
//       the first min(#valid, pre_nms) ranks scattered in score order
//       (nets/rpn.py:71-74);
//     staged NMS -- column-form 64x64 IoU tiles of one stage of column
//       blocks, then a resumable one-workgroup greedy sweep over those
//       blocks; stages stop being built once post_nms boxes are kept
//       (nets/rpn.py:75-77).
// Ties in score are ordered by ascending anchor index (documented deviation:
// the reference's CPU argsort is unstable under ties).
// Shared with fpn_proposal.hip, each in one place: the 64x64 column-form tile
// (tile_rows16, tile_word) and first_bits in nms_iou.h; hist_find and wave_sort64 in radix_select.h; the
// wave reduction / scan and count_before in common.h.
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "common.h"
#include "nms_iou.h"
#include "radix_select.h"

namespace frcnn {

constexpr uint64_t kInvalidKey = ~0ull;

// The proposal chain's kernels (decode, first-chunk select / sort, IoU tiles,
// sweep) raise their waves' issue priority: in the bench pipeline they share
// CUs with the previous steps' RoIPool waves, which are VALU bound, and each
// chain is a step stream's serial latency (chain, then its pool).  cfg2 driver
// command 92.9-97.0k -> 100.1-101.2k images/s; the wide path's sort / NMS
// kernels likewise: cfg1 10.9-11.0k -> 11.3k, cfg4 7.1k -> 7.2-7.3k
// (profiles/r5_experiments.md).
#define FRCNN_CHAIN_PRIO() __builtin_amdgcn_s_setprio(3)

// ---------------------------------------------------------------- 1. decode
__global__ __launch_bounds__(256) void decode_filter_kernel(
    const float* __restrict__ scores, const float4* __restrict__ deltas,
    const float4* __restrict__ anchors, const float4* __restrict__ base, int A, int K, int W,
    int stride, float img_h, float img_w, float min_size, float4* __restrict__ boxes,
    uint64_t* __restrict__ keys) {
    FRCNN_CHAIN_PRIO();
    int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= A) return;
    size_t o = static_cast<size_t>(blockIdx.y) * A + a;
    float4 an;
    if (anchors) {
        an = anchors[a];
    } else {  // utils/anchors.py:46-59 in-register
        int k = a % K;
        int cell = a / K;
        float sx = static_cast<float>(stride * (cell % W));
        float sy = static_cast<float>(stride * (cell / W));
        float4 bb = base[k];
        an = make_float4(bb.x + sx, bb.y + sy, bb.z + sx, bb.w + sy);
    }
    float4 b = decode_box(an, deltas[o]);
    b.x = clamp_nan(b.x, 0.0f, img_h);
    b.z = clamp_nan(b.z, 0.0f, img_h);
    b.y = clamp_nan(b.y, 0.0f, img_w);
    b.w = clamp_nan(b.w, 0.0f, img_w);
    bool ok = (b.z - b.x >= min_size) && (b.w - b.y >= min_size);
    boxes[o] = b;
    keys[o] = ok ? (static_cast<uint64_t>(desc_score_key(scores[o])) << 32) | static_cast<uint32_t>(a)
                 : kInvalidKey;
}

// keys for the plain nms op: every box valid, index order breaks ties.
__global__ __launch_bounds__(256) void nms_keys_kernel(const float* __restrict__ scores, int n,
                                                       uint64_t* __restrict__ keys) {
    int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    keys[i] = (static_cast<uint64_t>(desc_score_key(scores[i])) << 32) | static_cast<uint32_t>(i);
}

// ------------------------------------------------- 2-4. sort (wide path)
// Every key of the image is sorted (no select pass): runs of 1024 keys are
// sorted in LDS, each key's rank in every other run is one binary search in
// that run (a workgroup per (run, run) pair, the searched run staged in LDS),
// and the ranks are summed and scattered.  O(A log A) work spread over the
// chip; the first min(#valid, pre_nms) ranks are the proposal layer's top-k
// (nets/rpn.py:71-74).  Invalid (filtered) keys are made unique and sorted
// after every valid key.
constexpr int kRun = 1024;

__device__ __forceinline__ uint64_t unique_key(uint64_t k, int a) {
    return k == kInvalidKey ? ((~0ull << 32) | static_cast<uint32_t>(a)) : k;
}

__global__ __launch_bounds__(1024) void run_sort_kernel(const uint64_t* __restrict__ keys_all, int A, int nr,
                                                        uint64_t* __restrict__ runs_all, int* __restrict__ vcount) {
    FRCNN_CHAIN_PRIO();
    const int n = blockIdx.y, i = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int base = i * kRun;
    const int len = min(kRun, A - base);
    __shared__ uint64_t s[kRun];
    __shared__ int s_v[16];
    const uint64_t raw = tid < len ? keys_all[static_cast<size_t>(n) * A + base + tid] : kInvalidKey;
    uint64_t key = tid < len ? unique_key(raw, base + tid) : ~0ull;
    const uint64_t vb = __ballot(tid < len && raw != kInvalidKey);
    if (lane == 0) s_v[wid] = __popcll(vb);
    key = wave_sort64(key);
    s[tid] = key;
    __syncthreads();
    int rank = lane;
#pragma unroll 1
    for (int w = 0; w < 16; ++w)
        if (w != wid) rank += count_before(s + 64 * w, 64, key);
    if (tid == 0) {
        int v = 0;
        for (int w = 0; w < 16; ++w) v += s_v[w];
        vcount[n * nr + i] = v;
    }
    __syncthreads();
    if (key != ~0ull) s[rank] = key;  // the padding (~0) is never placed
    __syncthreads();
    if (tid < len) runs_all[static_cast<size_t>(n) * nr * kRun + base + tid] = s[tid];
}

// Workgroup (i, j): for every key of run i, the number of keys of run j below it.
__global__ __launch_bounds__(1024) void merge_rank_kernel(const uint64_t* __restrict__ runs_all, int A, int nr,
                                                          int* __restrict__ part) {
    FRCNN_CHAIN_PRIO();
    const int n = blockIdx.z, j = blockIdx.y, i = blockIdx.x;
    if (i == j) return;
    const int tid = threadIdx.x;
    const int leni = min(kRun, A - i * kRun), lenj = min(kRun, A - j * kRun);
    const uint64_t* runs = runs_all + static_cast<size_t>(n) * nr * kRun;
    __shared__ uint64_t s[kRun];
    if (tid < lenj) s[tid] = runs[j * kRun + tid];
    __syncthreads();
    if (tid < leni)
        part[(static_cast<size_t>(n) * nr + j) * nr * kRun + i * kRun + tid] =
            count_before(s, lenj, runs[i * kRun + tid]);
}

// Per-image state of the staged NMS (carried from one stage launch to the next).
struct SweepState {
    int* count;        // [N] boxes kept so far
    int* done;         // [N] post_nms reached or every candidate examined
    uint64_t* kept;    // [N][Wc] kept bits of each 64-candidate block
    uint64_t* prehit;  // [N][Wc] columns hit by a box kept in an earlier stage
    int wc;
};

__global__ __launch_bounds__(1024) void rank_scatter_kernel(const uint64_t* __restrict__ runs_all,
                                                            const int* __restrict__ part,
                                                            const int* __restrict__ vcount, int A, int nr,
                                                            int pre, const float4* __restrict__ box_src,
                                                            float4* __restrict__ sbox, int32_t* __restrict__ sidx,
                                                            int* __restrict__ sel_P, SweepState ss) {
    FRCNN_CHAIN_PRIO();
    const int n = blockIdx.y, i = blockIdx.x;
    const int tid = threadIdx.x;
    int nvalid = 0;
    for (int j = 0; j < nr; ++j) nvalid += vcount[n * nr + j];
    const int P = nvalid < pre ? nvalid : pre;
    if (i == 0 && tid == 0) {
        sel_P[n] = P;
        ss.count[n] = 0;
        ss.done[n] = 0;
    }
    if (i == 0)
        for (int b = tid; b < ss.wc; b += 1024) ss.prehit[static_cast<size_t>(n) * ss.wc + b] = 0ull;
    const int len = min(kRun, A - i * kRun);
    if (tid >= len) return;
    const uint64_t key = runs_all[static_cast<size_t>(n) * nr * kRun + i * kRun + tid];
    int rank = tid;
    const int* pp = part + static_cast<size_t>(n) * nr * nr * kRun + i * kRun + tid;
#pragma unroll 8
    for (int j = 0; j < nr; ++j)  // independent loads: unrolled so they are in flight together
        rank += j != i ? pp[static_cast<size_t>(j) * nr * kRun] : 0;
    if (rank < P) {
        const uint32_t a = static_cast<uint32_t>(key);
        sidx[static_cast<size_t>(n) * pre + rank] = static_cast<int32_t>(a);
        sbox[static_cast<size_t>(n) * pre + rank] = box_src[static_cast<size_t>(n) * A + a];
    }
}

// ------------------------------------------------- 5-6. staged NMS (wide)
// The candidates are resolved in stages of column blocks [cb0, cb1) (64
// candidates each; stage widths 32, 64, 128, ... blocks).  A stage computes
// the IoU bits of its columns against every earlier row (64x64 tiles, upper
// triangle, chip-wide), then one workgroup per image continues the greedy
// sweep over the stage's blocks.  An image that has kept post_nms boxes (or
// run out of candidates) is marked done and every later stage returns at
// once, so the O(pre^2) triangle is only built as far as the sweep needs it
// (cfg4: ~2,600 of 30,000 rows).
__device__ __forceinline__ void tri_tile(int t, int nb, int& rb, int& cb) {  // full triangle (fused path)
    int total = nb * (nb + 1) / 2;
    int tr = total - 1 - t;  // reversed: row lengths 1, 2, 3, ...
    int r = static_cast<int>((sqrt(8.0 * tr + 1.0) - 1.0) * 0.5);
    while ((r + 1) * (r + 2) / 2 <= tr) ++r;
    while (r * (r + 1) / 2 > tr) --r;
    int off = tr - r * (r + 1) / 2;
    rb = nb - 1 - r;
    cb = nb - 1 - off;
}

// Tile t of the stage starting at column block cb0: columns in order, rows 0..cb.
__device__ __forceinline__ void stage_tile(int t, int cb0, int& rb, int& cb) {
    const int64_t u = static_cast<int64_t>(t) + static_cast<int64_t>(cb0) * (cb0 + 1) / 2;
    int c = static_cast<int>((sqrt(8.0 * static_cast<double>(u) + 1.0) - 1.0) * 0.5);
    while (static_cast<int64_t>(c + 1) * (c + 2) / 2 <= u) ++c;
    while (static_cast<int64_t>(c) * (c + 1) / 2 > u) --c;
    cb = c;
    rb = static_cast<int>(u - static_cast<int64_t>(c) * (c + 1) / 2);
}

// Column form: maskC[n][cb][rb][lane] bit i = row 64*rb + i suppresses column
// 64*cb + lane (torchvision's IoU test, rows before the column only), so the
// sweep turns a kept-row set into removed columns with one ballot per tile.
// 256 threads per tile: lane = column, wave w tests rows [16w, 16w+16) of the
// row block (4 independent waves per tile keep the SIMDs busy), the four
// partial words are OR-ed in LDS (tile_rows16 / tile_word, nms_iou.h; this
// kernel's own: the kept-row filter K and prehit).  The grid is capped
// (workgroups stride over the stage's tiles), so a stage of a finished image
// costs one short launch.
constexpr int kMaskGrid = 2048;

__global__ __launch_bounds__(256) void nms_mask_stage_kernel(const float4* __restrict__ sbox_all, int pre,
                                                             int Wc, const int* __restrict__ sel_P,
                                                             const int* __restrict__ done, int cb0,
                                                             int ntiles, NmsThr thr,
                                                             uint64_t* __restrict__ maskC,
                                                             const uint64_t* __restrict__ kept_all,
                                                             uint64_t* __restrict__ prehit) {
    FRCNN_CHAIN_PRIO();
    const int n = blockIdx.y;
    if (done[n]) return;
    const int P = sel_P[n];
    const int nbP = (P + 63) / 64;
    const float4* sbox = sbox_all + static_cast<size_t>(n) * pre;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    __shared__ float4 rbox[64];
    __shared__ float rarea[64];
    __shared__ uint64_t part[4][64];
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        int rb, cb;
        stage_tile(t, cb0, rb, cb);
        if (cb >= nbP) break;  // tiles go by column: the rest are past the candidates too
        if (rb >= nbP) continue;
        // Rows of earlier stages are settled: only their kept rows matter, and only
        // as "is the column hit" -- one bit per column, OR-ed into prehit.
        const bool settled = rb < cb0;
        const uint64_t K = settled ? kept_all[static_cast<size_t>(n) * Wc + rb] : ~0ull;
        if (K == 0ull) continue;  // uniform
        const int i0 = rb * 64;
        __syncthreads();  // the previous tile is done with rbox / part
        if (tid < 64 && i0 + tid < P) {
            const float4 b = sbox[i0 + tid];
            rbox[tid] = b;
            rarea[tid] = box_area(b);
        }
        const int j = cb * 64 + lane;
        const bool jv = j < P;
        const float4 bj = jv ? sbox[j] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float aj = box_area(bj);
        __syncthreads();
        int iend = min(64, P - i0);
        if (rb == cb) iend = min(iend, lane);  // rows before the column
        if (!jv) iend = 0;
        const uint64_t word = tile_word(part, wid, lane, tile_rows16(rbox, rarea, wid, iend, K, bj, aj, thr));
        if (wid == 0) {
            if (settled) {
                const uint64_t h = __ballot(jv && word != 0ull);
                if (lane == 0 && h) atomicOr(reinterpret_cast<unsigned long long*>(prehit) +
                                                 static_cast<size_t>(n) * Wc + cb,
                                             static_cast<unsigned long long>(h));
            } else if (jv) {
                maskC[((static_cast<size_t>(n) * Wc + cb) * Wc + rb) * 64 + lane] = word;
            }
        }
    }
}

// One 1024-thread workgroup per image continues the greedy sweep over the
// stage's blocks [cb0, cb1), 16 blocks (1024 candidates) at a time: wave w owns
// column block sb0 + w, lane = column.  Each lane starts from its prehit bit
// (hit by a box kept in an earlier stage, from the mask kernel), ORs in the
// kept rows of the stage's earlier blocks (one round of independent loads), then holds the
// column-form words of the sub-stage's earlier blocks in registers, so the
// sub-stage resolves block after block with one barrier each and no memory
// latency: wave q computes avail = ~hit, runs the fixed point
// K <- avail & ballot(diag & K == 0) (unique, = the greedy result), and the
// later waves fold K into their hit flags.
// OUT_MODE 0: propose outputs (boxes + int32 anchor index, zero padding);
// OUT_MODE 1: nms op output (int64 index into the original box array).
constexpr int kSub = 16;  // blocks per sub-stage (= waves of the workgroup)

template <int OUT_MODE>
__global__ __launch_bounds__(1024) void nms_sweep_stage_kernel(
    const uint64_t* __restrict__ maskC_all, const float4* __restrict__ sbox_all,
    const int32_t* __restrict__ sidx_all, int pre, int Wc, const int* __restrict__ sel_P, int post,
    int cb0, int cb1, SweepState ss, float4* __restrict__ out_rois, int32_t* __restrict__ out_idx,
    int64_t* __restrict__ out_keep, int32_t* __restrict__ out_count) {
    FRCNN_CHAIN_PRIO();
    extern __shared__ __attribute__((aligned(16))) uint64_t kept[];  // [Wc]
    __shared__ uint64_t s_K[2];
    __shared__ int s_count[2];
    const int n = blockIdx.x;
    if (ss.done[n]) return;  // uniform
    const int P = sel_P[n];
    const int nb = (P + 63) / 64;
    const int end = min(cb1, nb);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const uint64_t* maskC = maskC_all + static_cast<size_t>(n) * Wc * Wc * 64;
    const float4* sbox = sbox_all + static_cast<size_t>(n) * pre;
    const int32_t* sidx = sidx_all + static_cast<size_t>(n) * pre;
    uint64_t* gkept = ss.kept + static_cast<size_t>(n) * Wc;
    int count = ss.count[n];
    // rows of earlier stages reach this stage only through ss.prehit
    for (int sb0 = cb0; sb0 < end && count < post; sb0 += kSub) {
        const int nsb = min(kSub, end - sb0);
        const int cb = sb0 + wid;  // this wave's column block
        const bool mine = wid < nsb;
        const int j = 64 * cb + lane;
        const uint64_t* colw = maskC + static_cast<size_t>(cb) * Wc * 64 + lane;  // tile (cb, rb) at colw[rb*64]
        bool hit = false;
        uint64_t col[kSub];
        float4 bxj = make_float4(0.f, 0.f, 0.f, 0.f);
        int32_t sj = -1;
        if (mine && j < P) {  // the outputs' data, loaded before the serial part
            bxj = sbox[j];
            sj = sidx[j];
        }
        if (mine) {
            hit = ((ss.prehit[static_cast<size_t>(n) * Wc + cb] >> lane) & 1ull) != 0ull;  // earlier stages
            for (int rb = cb0; rb < sb0; ++rb) hit |= (colw[static_cast<size_t>(rb) * 64] & kept[rb]) != 0ull;
#pragma unroll
            for (int q = 0; q < kSub; ++q) col[q] = q <= wid ? colw[static_cast<size_t>(sb0 + q) * 64] : 0ull;
        }
#pragma unroll
        for (int q = 0; q < kSub; ++q) {
            if (q >= nsb || count >= post) break;  // uniform
            if (wid == q) {
                const uint64_t avail = __ballot(j < P && !hit);
                const uint64_t diag = col[q];
                uint64_t K = avail;
                for (int it = 0; it < 65; ++it) {
                    const uint64_t Kn = avail & __ballot((diag & K) == 0ull);
                    if (Kn == K) break;
                    K = Kn;
                }
                K = first_bits(K, post - count);
                if ((K >> lane) & 1ull) {
                    const int slot_i = count + __popcll(K & lanemask_lt());
                    if (OUT_MODE == 0) {
                        out_rois[static_cast<size_t>(n) * post + slot_i] = bxj;
                        out_idx[static_cast<size_t>(n) * post + slot_i] = sj;
                    } else {
                        out_keep[slot_i] = sj;
                    }
                }
                if (lane == 0) {
                    kept[cb] = K;
                    s_K[q & 1] = K;
                    s_count[q & 1] = count + __popcll(K);
                }
            }
            __syncthreads();
            const uint64_t K = s_K[q & 1];
            count = s_count[q & 1];
            if (wid > q && (col[q] & K) != 0ull) hit = true;
        }
        __syncthreads();  // kept[] of this sub-stage complete before the next one's loads
    }
    const bool fin = count >= post || end >= nb;
    if (fin) {
        if (OUT_MODE == 0)
            for (int s = count + tid; s < post; s += 1024) {
                out_rois[static_cast<size_t>(n) * post + s] = make_float4(0.f, 0.f, 0.f, 0.f);
                out_idx[static_cast<size_t>(n) * post + s] = -1;
            }
        if (tid == 0) {
            out_count[n] = count;
            ss.done[n] = 1;
        }
    } else {
        for (int b = cb0 + tid; b < end; b += 1024) gkept[b] = kept[b];
        if (tid == 0) ss.count[n] = count;
    }
}

// ==================================================== fused per-image path
// One 1024-thread workgroup per image does select -> sort -> NMS with all
// working state on chip:
//   * the image's score keys live in registers (KPT per lane, anchor index
//     implied by the slot: a = tid + k*1024);
//   * the next CHUNK(=1024) candidates in rank order are found with an exact
//     radix select (12/12/8-bit digits, LDS histograms; hist_find), compacted
//     into LDS and sorted (wave_sort64 per wave, then ranks over the wave runs);
//   * NMS is lazy: each block of 64 sorted candidates is tested only against
//     the boxes kept so far (16 waves split the kept list) and against itself
//     (64x64 tile), then resolved by a wave with a fixed-point iteration
//     (K <- avail & ~OR_{i in K} D[i]); it stops as soon as post_nms are kept.
// Work is O(rows_examined x kept), not O(pre_nms^2).
constexpr int kChunk = 1024;
constexpr int kHistBins = 4096;
constexpr int kFusedMaxA = 24 * 1024;  // keys held in registers: <= 24 per lane

struct FusedShared {
    RadixBin bin;
    unsigned ccount;
    int kcount;
    unsigned wsum[16];
    uint64_t red[16];
    uint64_t diag[64];
    uint64_t keptw[16];
};

// r-th smallest (1-based) valid key64 = (score_key << 32 | anchor index).
template <int KPT>
__device__ uint64_t select_rank(const uint32_t (&sk)[KPT], int A, unsigned r, unsigned* hist,
                                FusedShared& sh) {
    const int tid = threadIdx.x;
    uint64_t prefix = 0;
    unsigned need = r;
    int done = 0;
#pragma unroll 1
    for (int pass = 0; pass < 6; ++pass) {
        const int width = (pass % 3 == 2) ? 8 : 12;
        const int shift = 64 - done - width;
        const int nbins = 1 << width;
        for (int i = tid; i < nbins; i += 1024) hist[i] = 0;
        __syncthreads();
        const uint64_t hm = done == 0 ? 0ull : (~0ull << (64 - done));
#pragma unroll
        for (int k = 0; k < KPT; ++k) {
            const int a = tid + k * 1024;
            if (a < A && sk[k] != 0xFFFFFFFFu) {
                const uint64_t key = (static_cast<uint64_t>(sk[k]) << 32) | static_cast<uint32_t>(a);
                if ((key & hm) == prefix)
                    atomicAdd(&hist[static_cast<unsigned>(key >> shift) & (nbins - 1)], 1u);
            }
        }
        __syncthreads();
        hist_find(hist, nbins, need, sh.bin, sh.wsum);
        const unsigned d = sh.bin.digit;
        need -= sh.bin.before;
        prefix |= static_cast<uint64_t>(d) << shift;
        done += width;
        const bool whole = sh.bin.bucket == need;
        __syncthreads();  // sh.* consumed before the next pass rewrites them
        if (whole) return prefix | ((1ull << shift) - 1ull);
    }
    return prefix;
}

// ---------------------------------------------- hybrid first-chunk NMS
// The lazy path below tests every 64-candidate block against the kept list on
// the image's one CU.  The hybrid path (default) moves the first chunk's IoU
// tests onto the whole chip:
//   MODE 1 (one workgroup per image): select + sort the first kChunk
//          candidates exactly as the lazy path does and hand them over (HybWs);
//   chunk_colmask_kernel: every (row block, column block) tile of the chunk's
//          upper triangle, lane = column: colT[j][w] bit i = row 64w+i (an
//          earlier box) suppresses column j (torchvision's IoU test);
//   MODE 2 (one workgroup per image): greedy sweep of the chunk from those
//          bits (chunk_sweep), then the lazy path from the second chunk on --
//          only if the first chunk kept fewer than post_nms boxes.

struct HybWs {
    float4* cbox;    // [N][kChunk] first-chunk boxes, score order
    uint64_t* ckey;  // [N][kChunk] their keys (anchor index in the low word)
    int* cc;         // [N] rows in the first chunk
    int* P;          // [N] min(#valid, pre_nms)
    uint64_t* colT;  // [N][kChunk][kChunkBlocks] column-form IoU bits
};
constexpr int kChunkBlocks = kChunk / 64;                           // 16

// The tile of nms_mask_stage_kernel (tile_rows16 / tile_word), every row tested.
__global__ __launch_bounds__(256) void chunk_colmask_kernel(const float4* __restrict__ cbox_all,
                                                            const int* __restrict__ cc_all, NmsThr thr,
                                                            uint64_t* __restrict__ colT, int nbt) {
    FRCNN_CHAIN_PRIO();
    const int n = blockIdx.y;
    const int cc = cc_all[n];
    const int nb = (cc + 63) / 64;
    int rb, cb;
    tri_tile(blockIdx.x, nbt, rb, cb);
    if (rb >= nb || cb >= nb) return;
    const float4* cbox = cbox_all + static_cast<size_t>(n) * kChunk;
    __shared__ float4 rbox[64];
    __shared__ float rarea[64];
    __shared__ uint64_t part[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int i0 = rb * 64;
    if (tid < 64 && i0 + tid < cc) {
        const float4 bx = cbox[i0 + tid];
        rbox[tid] = bx;
        rarea[tid] = box_area(bx);
    }
    const int j = cb * 64 + lane;
    const bool jv = j < cc;
    const float4 bj = jv ? cbox[j] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float aj = box_area(bj);
    __syncthreads();
    const int iend = jv ? min(min(64, cc - i0), j - i0) : 0;  // rows before column j
    const uint64_t word = tile_word(part, wid, lane, tile_rows16(rbox, rarea, wid, iend, ~0ull, bj, aj, thr));
    if (wid == 0 && jv) colT[(static_cast<size_t>(n) * kChunk + j) * kChunkBlocks + rb] = word;
}

// Greedy NMS over the first chunk's rows [0, cc) from this image's colT.
// Wave c holds the bits of columns [64c, 64c+64); blocks are resolved in
// order, block b by wave b: avail = its columns not hit by a kept row of an
// earlier block, then the fixed point K <- avail & ~{j : diag_j & K != 0}
// (unique, = the greedy result); the later waves fold block b's kept set into
// their hit flags.  Kept boxes go to kbox/karea and the
// outputs, at most post.
__device__ int chunk_sweep(const uint64_t* __restrict__ colT, int cc, int post, const float4* cbox,
                           const float* carea, const uint64_t* ckey, float4* kbox, float* karea,
                           float4* orois, int32_t* oidx, FusedShared& sh) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int nb = (cc + 63) / 64;
    const int j = wid * 64 + lane;
    const bool jv = j < cc;
    uint64_t col[kChunkBlocks];
#pragma unroll
    for (int w = 0; w < kChunkBlocks; ++w)
        col[w] = (jv && w <= wid) ? colT[static_cast<size_t>(j) * kChunkBlocks + w] : 0ull;
    bool hit = false;
    int kcount = 0;
#pragma unroll
    for (int b = 0; b < kChunkBlocks; ++b) {
        if (b >= nb || kcount >= post) break;
        if (wid == b) {
            const uint64_t avail = __ballot(jv && !hit);
            const uint64_t diag = col[b];
            uint64_t K = avail;
            for (int it = 0; it < 65; ++it) {
                const uint64_t Kn = avail & __ballot((diag & K) == 0ull);
                if (Kn == K) break;
                K = Kn;
            }
            K = first_bits(K, post - kcount);
            if ((K >> lane) & 1ull) {
                const int slot = kcount + __popcll(K & lanemask_lt());
                const float4 bx = cbox[j];
                kbox[slot] = bx;
                karea[slot] = carea[j];
                orois[slot] = bx;
                oidx[slot] = static_cast<int32_t>(static_cast<uint32_t>(ckey[j]));
            }
            if (lane == 0) sh.keptw[b] = K;
        }
        __syncthreads();
        const uint64_t Kb = sh.keptw[b];
        kcount += __popcll(Kb);
        if (wid > b && (col[b] & Kb) != 0ull) hit = true;
    }
    __syncthreads();
    return kcount;
}

// Phase probe of the fused kernel (instrumented builds only, -DFRCNN_PROP_PROF,
// tools/probe_propose.py): realtime clock (100 MHz) per (image, mode) at entry,
// keys loaded, first select done, chunk compacted, chunk sorted, exit.
#ifdef FRCNN_PROP_PROF
__device__ unsigned long long g_prop_prof[3][256][8];
#define PRPROF(k)                                                                            \
    do {                                                                                     \
        if (threadIdx.x == 0 && blockIdx.x < 256)                                            \
            g_prop_prof[MODE][blockIdx.x][k] = __builtin_amdgcn_s_memrealtime();             \
    } while (0)
extern "C" int frcnn_debug_prop_prof(unsigned long long* out, int reset) {
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_prop_prof), sizeof(g_prop_prof));
    if (reset) {
        static unsigned long long z[3][256][8];
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_prop_prof), z, sizeof(z));
    }
    return 0;
}
#else
#define PRPROF(k) do {} while (0)
#endif

// MODE 0: the lazy path, every chunk; MODE 1 / 2: the hybrid path's two
// per-image halves (see above).
template <int KPT, int MODE>
__global__ __launch_bounds__(1024) void propose_fused_kernel(
    const uint64_t* __restrict__ keys_all, const float4* __restrict__ boxes_all, int A, int pre,
    int post, NmsThr thr, float4* __restrict__ out_rois, int32_t* __restrict__ out_idx,
    int32_t* __restrict__ out_count, HybWs hw, int first) {
    FRCNN_CHAIN_PRIO();
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    __shared__ FusedShared sh;
    unsigned* hist = reinterpret_cast<unsigned*>(lds_raw);                          // 16 KB
    uint64_t* ckey = reinterpret_cast<uint64_t*>(lds_raw + kHistBins * 4);          //  8 KB
    float4* cbox = reinterpret_cast<float4*>(lds_raw + kHistBins * 4 + kChunk * 8); // 16 KB
    float* carea = reinterpret_cast<float*>(lds_raw + kHistBins * 4 + kChunk * 24); //  4 KB
    float4* kbox = reinterpret_cast<float4*>(lds_raw + kHistBins * 4 + kChunk * 28);
    float* karea = reinterpret_cast<float*>(lds_raw + kHistBins * 4 + kChunk * 28 + post * 16);

    const int n = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    PRPROF(0);
    const uint64_t* keys = keys_all + static_cast<size_t>(n) * A;
    const float4* boxes = boxes_all + static_cast<size_t>(n) * A;
    float4* orois = out_rois + static_cast<size_t>(n) * post;
    int32_t* oidx = out_idx + static_cast<size_t>(n) * post;

    uint32_t sk[KPT];
    int P = 0;
    int r_done = 0;
    uint64_t T_prev = 0;
    bool have_prev = false;
    int kcount = 0;
    if (MODE == 2) {  // first chunk: sorted by MODE 1, IoU bits from chunk_colmask_kernel
        const int cc = hw.cc[n];
        P = hw.P[n];
        for (int i = tid; i < cc; i += 1024) {
            const float4 b = hw.cbox[static_cast<size_t>(n) * kChunk + i];
            cbox[i] = b;
            carea[i] = box_area(b);
            ckey[i] = hw.ckey[static_cast<size_t>(n) * kChunk + i];
        }
        __syncthreads();
        kcount = chunk_sweep(hw.colT + static_cast<size_t>(n) * kChunk * kChunkBlocks, cc, post, cbox,
                             carea, ckey, kbox, karea, orois, oidx, sh);
        r_done = cc;
        if (cc > 0) {
            T_prev = ckey[cc - 1];
            have_prev = true;
        }
        if (tid == 0) sh.kcount = kcount;
    }
    if (MODE != 2 || (kcount < post && r_done < P)) {  // the keys are needed (uniform)
        unsigned nv = 0;
#pragma unroll
        for (int k = 0; k < KPT; ++k) {
            const int a = tid + k * 1024;
            const uint64_t key = a < A ? keys[a] : kInvalidKey;
            sk[k] = key == kInvalidKey ? 0xFFFFFFFFu : static_cast<uint32_t>(key >> 32);
            nv += sk[k] != 0xFFFFFFFFu;
        }
        if (MODE != 2) {
            nv = wave_reduce(nv, op_add{});
            if (lane == 0) sh.wsum[wid] = nv;
            if (tid == 0) sh.kcount = 0;
            __syncthreads();
            unsigned M = 0;
            for (int w = 0; w < 16; ++w) M += sh.wsum[w];
            P = static_cast<int>(M < static_cast<unsigned>(pre) ? M : static_cast<unsigned>(pre));
        }
        __syncthreads();
    }
    PRPROF(1);
    while (r_done < P && kcount < post) {
        const int r_end = min(r_done + (r_done == 0 ? first : kChunk), P);
        const uint64_t T = select_rank<KPT>(sk, A, static_cast<unsigned>(r_end), hist, sh);
        if (r_done == 0) PRPROF(2);
        if (tid == 0) sh.ccount = 0;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < KPT; ++k) {
            const int a = tid + k * 1024;
            if (a < A && sk[k] != 0xFFFFFFFFu) {
                const uint64_t key = (static_cast<uint64_t>(sk[k]) << 32) | static_cast<uint32_t>(a);
                if (key <= T && (!have_prev || key > T_prev)) ckey[atomicAdd(&sh.ccount, 1u)] = key;
            }
        }
        __syncthreads();
        const int cc = r_end - r_done;  // == sh.ccount (keys are unique)
        if (r_done == 0) PRPROF(3);
        // ---- sort of the chunk, ascending: every wave bitonic-sorts its 64 keys
        // with shuffles; a key's final position is its rank = the number of keys
        // below it over the chunk's sorted runs (binary searches; valid keys are
        // distinct, the invalid padding sorts last and is not placed).  Only the
        // nrun waves that hold keys search (the other runs are all padding).
        const int nrun = (cc + 63) >> 6;
        const bool inrun = wid < nrun;  // wave-uniform
        uint64_t key = wave_sort64(tid < cc ? ckey[tid] : kInvalidKey);
        __syncthreads();  // the reads of ckey above are done
        ckey[tid] = key;
        __syncthreads();
        int rank = lane;  // within its own run
        if (inrun) {
            for (int w = 0; w < nrun; ++w) {
                if (w == wid) continue;
                const uint64_t* run = ckey + w * 64;
                int lo = 0;
#pragma unroll
                for (int step = 32; step > 0; step >>= 1)
                    if (run[lo + step - 1] < key) lo += step;
                lo += run[lo] < key ? 1 : 0;
                rank += lo;
            }
        }
        __syncthreads();
        if (inrun && key != kInvalidKey) ckey[rank] = key;
        __syncthreads();
        key = ckey[tid];
        ckey[tid] = key;
        if (tid < cc) {
            const float4 b = boxes[static_cast<uint32_t>(key)];
            cbox[tid] = b;
            carea[tid] = box_area(b);
        }
        __syncthreads();
        if (r_done == 0) PRPROF(4);
        if (MODE == 1) {  // hand the sorted first chunk to chunk_colmask_kernel
            PRPROF(5);
            if (tid < cc) {
                hw.cbox[static_cast<size_t>(n) * kChunk + tid] = cbox[tid];
                hw.ckey[static_cast<size_t>(n) * kChunk + tid] = key;
            }
            if (tid == 0) {
                hw.cc[n] = cc;
                hw.P[n] = P;
            }
            return;
        }
        // ---- lazy NMS over 64-candidate blocks
        const int nb = (cc + 63) / 64;
#pragma unroll 1
        for (int blk = 0; blk < nb && kcount < post; ++blk) {
            const int j = blk * 64 + lane;
            const bool jv = j < cc;
            float4 bj = make_float4(0.f, 0.f, 0.f, 0.f);
            float aj = 0.f;
            if (jv) {
                bj = cbox[j];
                aj = carea[j];
            }
            bool sup = false;
            if (jv && !thr.never)
                for (int i = wid; i < kcount; i += 16)
                    if (iou_over(kbox[i], karea[i], bj, aj, thr)) {
                        sup = true;
                        break;
                    }
            const uint64_t supm = __ballot(sup);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = wid + 16 * q;
                const int ia = blk * 64 + r;
                bool bit = false;
                if (jv && lane > r && ia < cc && !thr.never) bit = iou_over(cbox[ia], carea[ia], bj, aj, thr);
                const uint64_t D = __ballot(bit);
                if (lane == 0) sh.diag[r] = D;
            }
            if (lane == 0) sh.red[wid] = supm;
            __syncthreads();
            if (wid == 0) {
                uint64_t removed = 0;
                for (int w = 0; w < 16; ++w) removed |= sh.red[w];
                const int rows = cc - blk * 64;
                if (rows < 64) removed |= ~0ull << rows;
                const uint64_t avail = ~removed;
                const uint64_t Dl = sh.diag[lane];
                uint64_t K = avail;
#pragma unroll 1
                for (int it = 0; it < 65; ++it) {  // fixed point (<= 64 iterations)
                    const uint64_t rb = wave_reduce(((K >> lane) & 1ull) ? Dl : 0ull, op_or{});
                    const uint64_t Kn = avail & ~rb;
                    if (Kn == K) break;
                    K = Kn;
                }
                K = first_bits(K, post - kcount);
                if ((K >> lane) & 1ull) {
                    const int slot = kcount + __popcll(K & lanemask_lt());
                    kbox[slot] = bj;
                    karea[slot] = aj;
                    orois[slot] = bj;
                    oidx[slot] = static_cast<int32_t>(static_cast<uint32_t>(ckey[j]));
                }
                if (lane == 0) sh.kcount = kcount + __popcll(K);
            }
            __syncthreads();
            kcount = sh.kcount;
        }
        r_done = r_end;
        T_prev = T;
        have_prev = true;
    }
    if (MODE == 1) {  // no valid candidate: an empty chunk
        if (tid == 0) {
            hw.cc[n] = 0;
            hw.P[n] = P;
        }
        return;
    }
    for (int s = kcount + tid; s < post; s += 1024) {
        orois[s] = make_float4(0.f, 0.f, 0.f, 0.f);
        oidx[s] = -1;
    }
    if (tid == 0) out_count[n] = kcount;
    PRPROF(5);
}

static size_t fused_lds_bytes(int post) {
    return static_cast<size_t>(kHistBins) * 4 + kChunk * 28 + static_cast<size_t>(post) * 20;
}

// The first chunk's size: the rows the greedy sweep usually needs to keep
// post_nms boxes fit in it (cfg2: the 300th kept box is candidate ~420 of 6000,
// cfg5: the 600th ~1,000-1,100, oracle on the bench inputs), so the first-chunk
// IoU tiles are not spent on rows past the last kept box; when they do not, the
// continuation takes the next kChunk rows.  The result does not depend on it.
static int first_chunk(int post) {
    int f = 64;
    while (f < kChunk && f < post + post / 2) f <<= 1;
    return f;
}

static int launch_fused(const uint64_t* keys, const float4* boxes, int N, int A, int pre, int post,
                        const NmsThr& thr, float4* out_rois, int32_t* out_idx, int32_t* out_count,
                        const HybWs& hw, bool lazy, hipStream_t st) {
    const size_t lds = fused_lds_bytes(post);
    const int kpt = (A + 1023) / 1024;
    const int first = first_chunk(post), nbt = first / 64;
#define FRCNN_FUSED(KP, MD)                                                                          \
    hipLaunchKernelGGL((propose_fused_kernel<KP, MD>), dim3(N), dim3(1024), lds, st, keys, boxes, A, \
                       pre, post, thr, out_rois, out_idx, out_count, hw, first)
#define FRCNN_FUSED_KPT(MD)            \
    if (kpt <= 8) FRCNN_FUSED(8, MD);  \
    else if (kpt <= 16) FRCNN_FUSED(16, MD); \
    else FRCNN_FUSED(24, MD)
    if (lazy) {
        FRCNN_FUSED_KPT(0);
        FRCNN_LAUNCH_CHECK("propose_fused_kernel");
        return FRCNN_OK;
    }
    FRCNN_FUSED_KPT(1);
    FRCNN_LAUNCH_CHECK("propose_fused_kernel (first chunk)");
    hipLaunchKernelGGL(chunk_colmask_kernel, dim3(nbt * (nbt + 1) / 2, N), dim3(256), 0, st, hw.cbox, hw.cc,
                       thr, hw.colT, nbt);
    FRCNN_LAUNCH_CHECK("chunk_colmask_kernel");
    FRCNN_FUSED_KPT(2);
    FRCNN_LAUNCH_CHECK("propose_fused_kernel (sweep)");
#undef FRCNN_FUSED_KPT
#undef FRCNN_FUSED
    return FRCNN_OK;
}

// Which proposal path: the fused per-image kernel fills one CU per image and
// does O(rows x kept) IoU work; the wide path spreads an O(pre^2/2) bitmask
// over the whole chip.  Few images with a large post_nms -> wide.
static bool use_fused(int N, int A, int post) {
    if (A > kFusedMaxA || post > 4096) return false;
    const int forced = path_cfg().propose;  // frcnn_set_path("propose", ...)
    if (forced == kPathHybrid || forced == kPathLazy) return true;
    if (forced == kPathWide) return false;
    return N >= 4 || post <= 1000;
}

// ------------------------------------------------------------ workspace map
struct ProposeWs {
    uint64_t* keys;
    float4* boxes;
    uint64_t* runs;   // [N][nr * kRun] sorted runs
    int* part;        // [N][nr][nr * kRun] cross-run ranks
    int* vcount;      // [N][nr] valid keys per run
    int* sel_P;       // [N] min(#valid, pre)
    float4* sbox;     // [N][pre] candidates in score order
    int32_t* sidx;
    uint64_t* maskC;  // [N][Wc][Wc][64] column-form IoU tiles (built stage by stage)
    SweepState ss;
    HybWs hyb;
    size_t bytes;
};

static ProposeWs carve(void* ws, int N, int A, int pre, bool need_boxes) {
    Carver c(ws);
    ProposeWs w{};
    const int Wc = (pre + 63) / 64;
    const int nr = (A + kRun - 1) / kRun;
    w.keys = c.take<uint64_t>(static_cast<size_t>(N) * A);
    w.boxes = need_boxes ? c.take<float4>(static_cast<size_t>(N) * A) : nullptr;
    w.runs = c.take<uint64_t>(static_cast<size_t>(N) * nr * kRun);
    w.part = c.take<int>(static_cast<size_t>(N) * nr * nr * kRun);
    w.vcount = c.take<int>(static_cast<size_t>(N) * nr);
    w.sel_P = c.take<int>(N);
    w.sbox = c.take<float4>(static_cast<size_t>(N) * pre);
    w.sidx = c.take<int32_t>(static_cast<size_t>(N) * pre);
    w.maskC = c.take<uint64_t>(static_cast<size_t>(N) * Wc * Wc * 64);
    w.ss.count = c.take<int>(N);
    w.ss.done = c.take<int>(N);
    w.ss.kept = c.take<uint64_t>(static_cast<size_t>(N) * Wc);
    w.ss.prehit = c.take<uint64_t>(static_cast<size_t>(N) * Wc);
    w.ss.wc = Wc;
    w.hyb.cbox = c.take<float4>(static_cast<size_t>(N) * kChunk);
    w.hyb.ckey = c.take<uint64_t>(static_cast<size_t>(N) * kChunk);
    w.hyb.cc = c.take<int>(N);
    w.hyb.P = c.take<int>(N);
    w.hyb.colT = c.take<uint64_t>(static_cast<size_t>(N) * kChunk * kChunkBlocks);
    w.bytes = c.used();
    return w;
}

// Sort + staged NMS, shared by frcnn_propose (wide path) and frcnn_nms.
static int sort_and_suppress(const ProposeWs& w, const float4* box_src, int N, int A, int pre,
                             int post, double iou_thr, int out_mode, float4* out_rois,
                             int32_t* out_idx, int64_t* out_keep, int32_t* out_count,
                             hipStream_t st) {
    const int Wc = (pre + 63) / 64;
    const int nr = (A + kRun - 1) / kRun;
    hipLaunchKernelGGL(run_sort_kernel, dim3(nr, N), dim3(1024), 0, st, w.keys, A, nr, w.runs, w.vcount);
    FRCNN_LAUNCH_CHECK("run_sort_kernel");
    if (nr > 1) {
        hipLaunchKernelGGL(merge_rank_kernel, dim3(nr, nr, N), dim3(1024), 0, st, w.runs, A, nr, w.part);
        FRCNN_LAUNCH_CHECK("merge_rank_kernel");
    }
    hipLaunchKernelGGL(rank_scatter_kernel, dim3(nr, N), dim3(1024), 0, st, w.runs, w.part, w.vcount, A, nr,
                       pre, box_src, w.sbox, w.sidx, w.sel_P, w.ss);
    FRCNN_LAUNCH_CHECK("rank_scatter_kernel");
    const NmsThr thr = make_thr(iou_thr);
    // stage widths 48, 64, 128, ... blocks of 64 candidates (cfg4 needs 41
    // blocks for post_nms = 2000, cfg1 92): every later stage of an image that
    // is done returns at once
    for (int cb0 = 0, width = 48; cb0 < Wc; cb0 += width, width = cb0 == 48 ? 64 : 2 * width) {
        const int cb1 = cb0 + width < Wc ? cb0 + width : Wc;
        const int64_t tiles = static_cast<int64_t>(cb1) * (cb1 + 1) / 2 - static_cast<int64_t>(cb0) * (cb0 + 1) / 2;
        const unsigned grid = static_cast<unsigned>(tiles < kMaskGrid ? tiles : kMaskGrid);
        hipLaunchKernelGGL(nms_mask_stage_kernel, dim3(grid, N), dim3(256), 0, st, w.sbox, pre, Wc, w.sel_P,
                           w.ss.done, cb0, static_cast<int>(tiles), thr, w.maskC, w.ss.kept, w.ss.prehit);
        FRCNN_LAUNCH_CHECK("nms_mask_stage_kernel");
        const size_t lds = static_cast<size_t>(Wc) * sizeof(uint64_t);
        if (out_mode == 0)
            hipLaunchKernelGGL(nms_sweep_stage_kernel<0>, dim3(N), dim3(1024), lds, st, w.maskC, w.sbox, w.sidx,
                               pre, Wc, w.sel_P, post, cb0, cb1, w.ss, out_rois, out_idx, out_keep, out_count);
        else
            hipLaunchKernelGGL(nms_sweep_stage_kernel<1>, dim3(N), dim3(1024), lds, st, w.maskC, w.sbox, w.sidx,
                               pre, Wc, w.sel_P, post, cb0, cb1, w.ss, out_rois, out_idx, out_keep, out_count);
        FRCNN_LAUNCH_CHECK("nms_sweep_stage_kernel");
    }
    return FRCNN_OK;
}

}  // namespace frcnn

using namespace frcnn;

static int check_params(const frcnn_propose_params* p) {
    FRCNN_REQUIRE(p, "frcnn_propose: null params");
    FRCNN_REQUIRE(p->N > 0 && p->N <= 65535, "frcnn_propose: N must be in [1, 65535]");
    FRCNN_REQUIRE(p->A > 0, "frcnn_propose: A must be > 0");
    FRCNN_REQUIRE(p->pre_nms > 0 && p->post_nms > 0, "frcnn_propose: pre/post_nms must be > 0");
    FRCNN_REQUIRE(static_cast<int64_t>(p->pre_nms) <= (1 << 20), "frcnn_propose: pre_nms > 2^20");
    FRCNN_REQUIRE(p->A <= (1 << 18), "frcnn_propose: A > 2^18");
    return FRCNN_OK;
}

extern "C" size_t frcnn_propose_workspace_size(const frcnn_propose_params* p) {
    if (check_params(p)) return 0;
    const int pre = p->pre_nms < p->A ? p->pre_nms : p->A;
    return carve(nullptr, p->N, p->A, pre, true).bytes;
}

extern "C" int frcnn_propose(const frcnn_propose_params* p, const float* scores, const float* deltas,
                             const float* anchors, const float* anchor_base, float* out_rois,
                             int32_t* out_idx, int32_t* out_count, void* workspace,
                             size_t ws_bytes, void* stream) {
    int rc = check_params(p);
    if (rc) return rc;
    FRCNN_REQUIRE(scores && deltas && out_rois && out_idx && out_count,
                  "frcnn_propose: null pointer");
    FRCNN_REQUIRE(anchors || anchor_base, "frcnn_propose: need anchors or anchor_base");
    if (!anchors)
        FRCNN_REQUIRE(p->K > 0 && p->feat_h > 0 && p->feat_w > 0 &&
                          static_cast<int64_t>(p->K) * p->feat_h * p->feat_w == p->A,
                      "frcnn_propose: A != feat_h*feat_w*K");
    const int pre = p->pre_nms < p->A ? p->pre_nms : p->A;
    ProposeWs w = carve(workspace, p->N, p->A, pre, true);
    FRCNN_REQUIRE(workspace && ws_bytes >= w.bytes, "frcnn_propose: workspace %zu < %zu",
                  ws_bytes, w.bytes);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(decode_filter_kernel, dim3((p->A + 255) / 256, p->N), dim3(256), 0, st,
                       scores, reinterpret_cast<const float4*>(deltas),
                       reinterpret_cast<const float4*>(anchors),
                       reinterpret_cast<const float4*>(anchor_base), p->A, p->K, p->feat_w,
                       p->feat_stride, p->img_h, p->img_w, p->min_size, w.boxes, w.keys);
    FRCNN_LAUNCH_CHECK("decode_filter_kernel");
    if (use_fused(p->N, p->A, p->post_nms)) {
        return launch_fused(w.keys, w.boxes, p->N, p->A, pre, p->post_nms, make_thr(p->iou_threshold),
                            reinterpret_cast<float4*>(out_rois), out_idx, out_count, w.hyb,
                            path_cfg().propose == kPathLazy, st);
    }
    return sort_and_suppress(w, w.boxes, p->N, p->A, pre, p->post_nms, p->iou_threshold, 0,
                             reinterpret_cast<float4*>(out_rois), out_idx, nullptr, out_count, st);
}

constexpr int64_t kNmsMax = 1 << 16;  // bitmask workspace n * n / 8 B (512 MB at the cap)

extern "C" size_t frcnn_nms_workspace_size(int64_t n) {
    if (n <= 0 || n > kNmsMax) return 0;
    return carve(nullptr, 1, static_cast<int>(n), static_cast<int>(n), false).bytes;
}

extern "C" int frcnn_nms(const float* boxes, const float* scores, int64_t n, double iou_threshold,
                         int64_t* keep, int32_t* count, void* workspace, size_t ws_bytes,
                         void* stream) {
    FRCNN_REQUIRE(n >= 0 && n <= kNmsMax, "frcnn_nms: n must be in [0, 65536]");
    FRCNN_REQUIRE(count, "frcnn_nms: null count");
    hipStream_t st = as_stream(stream);
    if (n == 0) {
        if (hipMemsetAsync(count, 0, sizeof(int32_t), st) != hipSuccess)
            return check_launch("frcnn_nms memset");
        return FRCNN_OK;
    }
    FRCNN_REQUIRE(boxes && scores && keep, "frcnn_nms: null pointer");
    const int N = static_cast<int>(n);
    ProposeWs w = carve(workspace, 1, N, N, false);
    FRCNN_REQUIRE(workspace && ws_bytes >= w.bytes, "frcnn_nms: workspace %zu < %zu", ws_bytes,
                  w.bytes);
    hipLaunchKernelGGL(nms_keys_kernel, dim3((N + 255) / 256), dim3(256), 0, st, scores, N, w.keys);
    FRCNN_LAUNCH_CHECK("nms_keys_kernel");
    return sort_and_suppress(w, reinterpret_cast<const float4*>(boxes), 1, N, N, N, iou_threshold,
                             1, nullptr, nullptr, keep, count, st);
}

