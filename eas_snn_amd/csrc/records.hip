// Record segments copied from one buffer into another (eas_records_gather): the build step of data.Gen1WindowStore, which keeps of a
// .dat recording only the records its samples read.  A pure copy, bound by HBM bandwidth.
//   dst[seg_dst[s] + i] = src[seg_src[s] + i]   for 0 <= i < seg_dst[s + 1] - seg_dst[s],   0 <= s < S
// The work is cut along the DESTINATION, which is contiguous: a block owns a tile of kTile destination records, each of its waves a
// quarter of it.  A wave finds the segment that holds its first record by one binary search in seg_dst (every lane walks the same probes:
// one search per wave, not per record) and walks the segments from there; inside a segment the lanes copy consecutive records, so loads
// and stores are coalesced.  Where the source and the destination address of a run agree modulo 16 bytes, a lane moves two records (16
// bytes) at a time, with a single record in front and behind where the run starts or ends on an odd record; otherwise a lane moves one
// record (8 bytes).  Every destination record is written exactly once, by the wave that owns it, and nothing else is written.
// Behind it: the packed form of such records (eas_records_pack_measure / _pack / _unpack), the build of data.Gen1PackedWindowStore.
#include "eas_common.h"
#include "record_source.h"

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

// ---- packed records (include/eas_hip.h states the format; record_source.h holds the decoder the range kernels of events.hip share).
// One wave per block of 64 records, one record per lane; a block of a grid walks blocks in strides.  The records behind the last one of
// a call, in its last block, are copies of that last record: a copy of a record of the block neither moves the block's minimum nor
// breaks a condition the block meets, so padding never turns a narrow block wide.
constexpr int kPackWaves = EAS_BLOCK / EAS_WAVE;

__device__ __forceinline__ uint32_t wave_min_all(uint32_t v) {             // the minimum over the 64 lanes, in every lane
#pragma unroll
    for (int off = EAS_WAVE / 2; off > 0; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, off, EAS_WAVE);
        v = o < v ? o : v;
    }
    return v;
}

__device__ __forceinline__ uint2 pack_lane_record(const uint2* __restrict__ rec, int64_t n, int64_t blk, int lane) {
    const int64_t i = blk * EAS_REC_BLOCK + lane;
    return rec[i < n ? i : n - 1];
}

__global__ __launch_bounds__(EAS_BLOCK) void records_pack_measure_kernel(const uint2* __restrict__ rec, int64_t n, int64_t nb, int xb, int yb,
                                                                         uint2* __restrict__ table) {
    const int lane = threadIdx.x & (EAS_WAVE - 1);
    const uint32_t span = 1u << (31 - xb - yb);
    for (int64_t blk = (int64_t)blockIdx.x * kPackWaves + threadIdx.x / EAS_WAVE; blk < nb; blk += (int64_t)gridDim.x * kPackWaves) {
        const uint2 v = pack_lane_record(rec, n, blk, lane);
        const uint32_t base = wave_min_all(v.x);
        const bool fits = (v.y & 16383u) < (1u << xb) && ((v.y >> 14) & 16383u) < (1u << yb) && (v.y >> 29) == 0 && v.x - base < span;
        const bool narrow = __ballot(fits) == ~0ull;
        if (lane == 0) table[blk] = make_uint2(base, narrow ? 1u : 2u);
    }
}

// table[blk] = (base, unit | wide << 31): the class and the place are the table's; a block whose units do not lie in [unit_lo, unit_hi)
// is not written
__global__ __launch_bounds__(EAS_BLOCK) void records_pack_kernel(const uint2* __restrict__ rec, int64_t n, int64_t nb, int xb, int yb,
                                                                 const uint2* __restrict__ table, uint8_t* __restrict__ payload, int64_t unit_lo,
                                                                 int64_t unit_hi) {
    const int lane = threadIdx.x & (EAS_WAVE - 1);
    for (int64_t blk = (int64_t)blockIdx.x * kPackWaves + threadIdx.x / EAS_WAVE; blk < nb; blk += (int64_t)gridDim.x * kPackWaves) {
        const uint2 entry = table[blk];
        const int64_t unit = entry.y & 0x7fffffffu;
        const bool wide = (entry.y >> 31) != 0;
        if (unit < unit_lo || unit + (wide ? 2 : 1) > unit_hi) continue;
        const uint2 v = pack_lane_record(rec, n, blk, lane);
        if (wide) {
            reinterpret_cast<uint2*>(payload + unit * EAS_REC_UNIT)[lane] = v;
        } else {
            const uint32_t word = (v.y & 16383u) | (((v.y >> 14) & 16383u) << xb) | (((v.y >> 28) & 1u) << (xb + yb)) | ((v.x - entry.x) << (xb + yb + 1));
            reinterpret_cast<uint32_t*>(payload + unit * EAS_REC_UNIT)[lane] = word;
        }
    }
}

__global__ __launch_bounds__(EAS_BLOCK) void records_unpack_kernel(const PackedRecords src, int64_t a, int64_t e, uint2* __restrict__ out) {
    for (int64_t i = a + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < e; i += (int64_t)gridDim.x * blockDim.x) {
        uint2 v;
        out[i - a] = src.record(i, v) ? v : make_uint2(0u, 0u);
    }
}

// the arguments the three entries share: 0, or the status to return
int pack_args(const void* records_or_out, int64_t n, int H, int W, const void* table, RecWidths& w) {
    if (n < 0 || H < 1 || W < 1 || !table || ((uintptr_t)table & 7)) return EAS_ERR_INVALID_ARG;
    if (n > 0 && (!records_or_out || ((uintptr_t)records_or_out & 7))) return EAS_ERR_INVALID_ARG;
    return rec_widths(H, W, w) ? EAS_OK : EAS_ERR_UNSUPPORTED;
}

}  // namespace

extern "C" int eas_records_pack_measure(const void* records, int64_t n, int H, int W, uint32_t* table, eas_stream_t stream) {
    RecWidths w;
    const int rc = pack_args(records, n, H, W, table, w);
    if (rc != EAS_OK || n == 0) return rc;
    const int64_t nb = (n + EAS_REC_BLOCK - 1) / EAS_REC_BLOCK;
    EAS_CLEAR_ERR();
    EAS_LAUNCH(records_pack_measure_kernel, dim3(eas_grid_1d(nb, kPackWaves)), dim3(EAS_BLOCK), 0, eas_s(stream), (const uint2*)records, n, nb, w.xb,
               w.yb, (uint2*)table);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

extern "C" int eas_records_pack(const void* records, int64_t n, int H, int W, const uint32_t* table, uint8_t* payload, int64_t unit_lo,
                                int64_t unit_hi, eas_stream_t stream) {
    RecWidths w;
    const int rc = pack_args(records, n, H, W, table, w);
    if (unit_lo < 0 || unit_hi < unit_lo || unit_hi > ((int64_t)1 << 31) || ((uintptr_t)payload & 15)) return EAS_ERR_INVALID_ARG;
    if (rc != EAS_OK || n == 0 || unit_hi == unit_lo) return rc;
    if (!payload) return EAS_ERR_INVALID_ARG;
    const int64_t nb = (n + EAS_REC_BLOCK - 1) / EAS_REC_BLOCK;
    EAS_CLEAR_ERR();
    EAS_LAUNCH(records_pack_kernel, dim3(eas_grid_1d(nb, kPackWaves)), dim3(EAS_BLOCK), 0, eas_s(stream), (const uint2*)records, n, nb, w.xb, w.yb,
               (const uint2*)table, payload, unit_lo, unit_hi);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

extern "C" int eas_records_unpack(const uint32_t* table, int64_t nb, const uint8_t* payload, int64_t units, int64_t a, int64_t e, int H, int W,
                                  void* out, uint32_t* flags, eas_stream_t stream) {
    RecWidths w;
    if (nb < 0 || a < 0 || e < a) return EAS_ERR_INVALID_ARG;
    const int rc = pack_args(out, e - a, H, W, table, w);
    if (units < 0 || units > ((int64_t)1 << 31) || (units > 0 && !payload) || ((uintptr_t)payload & 15) || ((uintptr_t)flags & 3)) return EAS_ERR_INVALID_ARG;
    if (rc != EAS_OK) return rc;
    if (e > nb * EAS_REC_BLOCK) return EAS_ERR_INVALID_ARG;
    EAS_CLEAR_ERR();
    if (flags && hipMemsetAsync(flags, 0, sizeof(uint32_t), eas_s(stream)) != hipSuccess) return EAS_ERR_LAUNCH;
    if (e == a) return EAS_OK;
    EAS_LAUNCH(records_unpack_kernel, dim3(eas_grid_1d(e - a)), dim3(EAS_BLOCK), 0, eas_s(stream),
               PackedRecords{(const uint2*)table, payload, nb, units, w.xb, w.yb, flags}, a, e, (uint2*)out);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

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
