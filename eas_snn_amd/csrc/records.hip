// Record segments copied from one buffer into another (eas_records_gather): the build step of data.Gen1WindowStore, which keeps of a
// .dat recording only the records its samples read.  A pure copy, bound by HBM bandwidth.
//   dst[seg_dst[s] + i] = src[seg_src[s] + i]   for 0 <= i < seg_dst[s + 1] - seg_dst[s],   0 <= s < S
// The work is cut along the DESTINATION, which is contiguous: a block owns a tile of kTile destination records, each of its waves a
// quarter of it.  A wave finds the segment that holds its first record by one binary search in seg_dst (every lane walks the same probes:
// one search per wave, not per record) and walks the segments from there; inside a segment the lanes copy consecutive records, so loads
// and stores are coalesced.  Where the source and the destination address of a run agree modulo 16 bytes, a lane moves two records (16
// bytes) at a time, with a single record in front and behind where the run starts or ends on an odd record; otherwise a lane moves one
// record (8 bytes).  Every destination record is written exactly once, by the wave that owns it, and nothing else is written.
#include "eas_common.h"

namespace {

constexpr int kGatherTile = 4096;                                       // destination records per block (32 KiB)
constexpr int kGatherWaveTile = kGatherTile / (EAS_BLOCK / EAS_WAVE);   // per wave: 1024 records = 8 rounds of 16 bytes per lane

// the segment s in [0, S) with seg_dst[s] <= pos < seg_dst[s + 1]; the caller guarantees seg_dst[0] <= pos < seg_dst[S]
__device__ __forceinline__ int64_t gather_segment_of(const int64_t* __restrict__ seg_dst, int64_t S, int64_t pos) {
    int64_t lo = 0, hi = S;                        // seg_dst[lo] <= pos < seg_dst[hi] throughout
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (seg_dst[mid] <= pos) lo = mid; else hi = mid;
    }
    return lo;
}

// n >= 1 consecutive records by the 64 lanes of a wave
__device__ __forceinline__ void gather_run(const uint2* __restrict__ s, uint2* __restrict__ d, int64_t n, int lane) {
    if ((((uintptr_t)s ^ (uintptr_t)d) & 8) == 0) {
        const int64_t head = ((uintptr_t)d & 8) ? 1 : 0;           // an odd first record: alone, the rest is 16-byte aligned on both sides
        if (head && lane == 0) d[0] = s[0];
        const int64_t pairs = (n - head) >> 1;
        const uint4* __restrict__ s4 = reinterpret_cast<const uint4*>(s + head);
        uint4* __restrict__ d4 = reinterpret_cast<uint4*>(d + head);
#pragma unroll 4
        for (int64_t i = lane; i < pairs; i += EAS_WAVE) d4[i] = s4[i];
        if (((n - head) & 1) && lane == EAS_WAVE - 1) d[n - 1] = s[n - 1];
    } else {
#pragma unroll 4
        for (int64_t i = lane; i < n; i += EAS_WAVE) d[i] = s[i];
    }
}

__global__ __launch_bounds__(EAS_BLOCK) void records_gather_kernel(const uint2* __restrict__ src, const int64_t* __restrict__ seg_src,
                                                                   const int64_t* __restrict__ seg_dst, int64_t S, uint2* __restrict__ dst) {
    const int lane = threadIdx.x & (EAS_WAVE - 1), wave = threadIdx.x / EAS_WAVE;
    const int64_t begin = seg_dst[0], end = seg_dst[S];
    const int64_t ntiles = (end - begin + kGatherTile - 1) / kGatherTile;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t w0 = begin + tile * kGatherTile + (int64_t)wave * kGatherWaveTile;
        const int64_t w1 = w0 + kGatherWaveTile < end ? w0 + kGatherWaveTile : end;
        if (w0 >= w1) continue;
        int64_t s = gather_segment_of(seg_dst, S, w0);
        for (int64_t d = w0; d < w1 && s < S; ++s) {               // s < S: a table that is not ascending ends the walk, it is never overrun
            const int64_t s_begin = seg_dst[s], s_end = seg_dst[s + 1];
            const int64_t e = s_end < w1 ? s_end : w1;
            if (e > d) {                                           // (an empty segment, or one that lies in front of d in a bad table: skipped)
                gather_run(src + (seg_src[s] + (d - s_begin)), dst + d, e - d, lane);
                d = e;
            }
        }
    }
}

}  // namespace

extern "C" int eas_records_gather(const void* src, const int64_t* seg_src, const int64_t* seg_dst, int64_t S, int64_t total, void* dst,
                                  eas_stream_t stream) {
    if (!src || !seg_src || !seg_dst || !dst || S < 1 || total < 0) return EAS_ERR_INVALID_ARG;
    if (((uintptr_t)src | (uintptr_t)seg_src | (uintptr_t)seg_dst | (uintptr_t)dst) & 7) return EAS_ERR_INVALID_ARG;
    if (total == 0) return EAS_OK;
    EAS_CLEAR_ERR();
    EAS_LAUNCH(records_gather_kernel, dim3(eas_grid_1d(total, kGatherTile)), dim3(EAS_BLOCK), 0, eas_s(stream), (const uint2*)src, seg_src, seg_dst,
               S, (uint2*)dst);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}
