// Block-level pieces of the exact radix select and of the run sort, shared by
// the proposal layer (proposal.hip) and the FPN proposal layer (fpn_proposal.hip).
#pragma once

#include "common.h"

namespace frcnn {

// What hist_find leaves in LDS for the whole workgroup.
struct RadixBin {
    unsigned digit, before, bucket;
};

// Block-wide: the bin d with cum(bins < d) < need <= cum(bins <= d), its count
// (bucket) and the count of the bins below it (before).  1024 threads, at most
// 4096 bins, wsum = 16 words of LDS; ends on a barrier, and the caller puts one
// behind its last read of `out`.
__device__ __forceinline__ void hist_find(const unsigned* hist, int nbins, unsigned need, RadixBin& out,
                                          unsigned* wsum) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    unsigned h[4], loc = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int bi = 4 * tid + q;
        h[q] = bi < nbins ? hist[bi] : 0u;
        loc += h[q];
    }
    const unsigned incl = wave_scan_incl(loc, op_add{});
    if (lane == 63) wsum[wid] = incl;
    __syncthreads();
    unsigned before = incl - loc;
    for (int w = 0; w < wid; ++w) before += wsum[w];
    if (before < need && before + loc >= need) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (before < need && before + h[q] >= need) {
                out.digit = 4 * tid + q;
                out.before = before;
                out.bucket = h[q];
            }
            before += h[q];
        }
    }
    __syncthreads();
}

// Ascending bitonic sort of the wave's 64 keys (one per lane), by shuffles.
__device__ __forceinline__ uint64_t wave_sort64(uint64_t key) {
    const int lane = threadIdx.x & 63;
    for (int kk = 2; kk <= 64; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            const uint64_t other = __shfl_xor(key, j, 64);
            const bool asc = (lane & kk) == 0;
            const bool lower = (lane & j) == 0;
            const uint64_t mn = other < key ? other : key;
            const uint64_t mx = other < key ? key : other;
            key = (lower == asc) ? mn : mx;
        }
    }
    return key;
}

}  // namespace frcnn
