// N-Caltech101 front end: raw ATIS recordings (5 bytes per record) -> per-polarity frames [B][Tl][Tm][2][H][W]: int32 counts
// (eas_event_histogram_atis, measure='count') or float64 time-surface-weighted sums (eas_event_timesurface_atis, measure='timesurface').
// Reference: NCaltech.read_ATIS, generate_slices and agrregate('micro_sum') with overlap=0
// (yolox/data/datasets/ncaltech.py:63-96, 179-183, 218-237, 264-269, 368-379; yolox/utils/event_reps.py:9-19).
//   record b0..b4: x = b0, y = b1, p = b2 >> 7, raw = (b2 & 127) << 16 | b3 << 8 | b4;  y == 240 is an overflow record: no event, it adds
//   8192 to the time of every later record of its recording, so t = raw + 8192 * (overflow records at or before the record).
// Five launches (six for the time surface; 1 and 2, the index of the buffer, run in front of 0), no allocation, no host read
// (graph-capturable):
//   0. atis_zero_kernel             the frames
//   1. atis_overflow_count_kernel  overflow records per chunk of kChunk records of the whole buffer (reads the y byte of every record)
//   2. atis_overflow_scan_kernel    exclusive scan of the chunk counts, in place (one block)
//   3. atis_plan_kernel             one wave per recording: last event, window, t0 / tL, and per macro slice the first / last member
//                                   event (binary searches over decoded records; a probe's time = raw + 8192 * (chunk base + in-chunk
//                                   count - the recording's own base)) -> one AtisHead per recording, one AtisSlice per macro slice
//   4. atis_hist_kernel             blocks stride over the chunks of a recording: decode in registers, block scan of the overflow
//                                   records of the chunk, window / macro slice / micro slice (the SampleWin rule of event_bin.h bin_event),
//                                   integer atomics -- bit-exact in any order.  The accumulate step is the kernel's template
//                                   parameter, the only difference between the two measures: CountAcc (event_bin.h) adds 1 to an int32 bin,
//                                   TimeSurfaceAcc adds llrint(w * 2^48), w = 1 - tanh((t_target - t) / tau) in fp64 with t_target =
//                                   the time of the macro slice's last member event (a plan row), to a 64-bit bin
//   5. atis_ts_finish_kernel        (time surface only) the 64-bit sums, in place, -> double * 2^-48
//   aggregation 'timesurface' (eas_event_latest_surface_atis; agrregate('timesurface'), ncaltech.py:255-257 + to_timesurface_numpy,
//   event_reps.py:141-160, tau = 10e3) is a third accumulate step and a finishing pass of its own: LatestAcc takes the integer atomic max
//   of the event's time into the OUTPUT's 64-bit bin of its micro slice; latest_finish_kernel<AtisSliceWin>, one thread per (recording, macro slice,
//   polarity, pixel), walks the Tm bins with a running maximum m and overwrites each with exp(-((q + 1) * w + f - m) / tau), f and w read
//   from the plan's row (latest_surface.h).  Plan flag bit 3: a macro slice that holds events has micro window 0 (the reference raises).
// Time-surface sums are integers, so the frames do not depend on the order of the adds: bit-identical run to run, for any grid and any
// neighbours in the buffer.  Each event is off by <= 2^-49 (the rounding of w * 2^48) + the error of tanh; a bin holds 65 535 events of
// weight 1 (kTsCapacity): a macro slice of more records than that sets flag bit 2 (conservative: the records of ONE pixel would have to).
// Algorithmic bytes per recording: 5 * nrec + 4 * Tl * Tm * 2 * H * W (time surface: 8 * ..., and the finishing pass reads and writes them
// once more); the records are read twice (launches 1 and 4), the plan's probes
// re-read O(Tl * log nrec) chunks.
// The chunks are chunks of the BUFFER (record index / kChunk), not of a recording: the overflow count of a record inside recording
// [a, e) is prefix(i) - prefix(a - 1), so recordings need no chunk tables of their own.
// A store (a dataset resident in HBM) runs launches 1 and 2 ONCE (eas_atis_store_index -> uint32 [chunks + 1], caller-owned); a step then is
// launches 0, 3, 4 (5) of the *_store entries on the B recordings that sample_file picks out of file_offsets: 5 * sum n_b record bytes, not
// 10 * nrec.  Where recording b lies is the only difference between the two families: a range source (PackedRanges / StoreRanges), a
// template parameter of the plan and the histogram kernel.
#include <limits.h>

#include "eas_common.h"
#include "event_bin.h"
#include "latest_surface.h"

namespace {

constexpr int kChunk = 256;             // records per chunk = threads of a histogram block (a power of two <= 4096)
constexpr int kChunkShift = 8;
constexpr uint32_t kOverflowY = 240;
constexpr uint32_t kTimeIncrement = 8192;   // the reference's 2 ** 13, kept as it is
constexpr int kScanThreads = 1024;
constexpr double kTsOne = 281474976710656.0;            // 2^48: a time-surface weight of 1 in a 64-bit bin
constexpr int64_t kTsCapacity = 65535;                  // weights of 1 an unsigned 64-bit bin holds: floor((2^64 - 1) / 2^48)

struct AtisHead {                       // per recording
    int64_t wl, wh;                     // events with wl < t <= wh remain (no window: INT64_MIN, INT64_MAX)
    int64_t t0, mw;                     // first remaining time, macro slice length (0: nothing is binned)
    uint32_t ovf_base, pad;             // overflow records of the buffer in front of the recording
};
struct AtisSlice { uint32_t f, w; };    // per (recording, macro slice): time of its first member event, micro window (0: nothing is binned)

__device__ __forceinline__ void clamp_range(int64_t lo, int64_t hi, int64_t nrec, int64_t& a, int64_t& e) {
    a = lo < 0 ? 0 : lo;
    e = hi > nrec ? nrec : hi;
    if (e < a) e = a;                   // offsets that do not describe a range: an empty recording (flag bit 1), nothing past nrec is read
}

// ---- range sources: recording b of a call -> its records [a, e) of the buffer; false: b names no recording (an empty range, flag bit 4)
struct PackedRanges {                   // the batch back to back: offsets [B + 1]
    const int64_t* offsets;
    __device__ __forceinline__ bool operator()(int b, int64_t nrec, int64_t& a, int64_t& e) const {
        clamp_range(offsets[b], offsets[b + 1], nrec, a, e);
        return true;
    }
};
struct StoreRanges {                    // a resident store: recording b is file sample_file[b] of file_offsets [F + 1]
    const int64_t* file_offsets;
    int64_t F;
    const int64_t* sample_file;
    __device__ __forceinline__ bool operator()(int b, int64_t nrec, int64_t& a, int64_t& e) const {
        const int64_t f = sample_file[b];
        a = e = 0;
        if (f < 0 || f >= F) return false;                     // nothing is read through the index
        clamp_range(file_offsets[f], file_offsets[f + 1], nrec, a, e);
        return true;
    }
};

__device__ __forceinline__ uint32_t rec_y(const uint8_t* __restrict__ rec, int64_t i) { return rec[5 * i + 1]; }
__device__ __forceinline__ uint32_t rec_raw(const uint8_t* __restrict__ rec, int64_t i) {
    const uint8_t* p = rec + 5 * i;
    return ((uint32_t)(p[2] & 127u) << 16) | ((uint32_t)p[3] << 8) | (uint32_t)p[4];
}

__global__ __launch_bounds__(kChunk) void atis_overflow_count_kernel(const uint8_t* __restrict__ rec, int64_t nrec, int64_t nchunks,
                                                                      uint32_t* __restrict__ chunk_base) {
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int64_t i = c * kChunk + threadIdx.x;
        const int n = __syncthreads_count(i < nrec && rec_y(rec, i) == kOverflowY);
        if (threadIdx.x == 0) chunk_base[c] = (uint32_t)n;
    }
}

// exclusive scan in place: thread t owns a contiguous segment, the segment totals are scanned through LDS
__global__ __launch_bounds__(kScanThreads) void atis_overflow_scan_kernel(uint32_t* __restrict__ chunk_base, int64_t nchunks) {
    __shared__ uint32_t tot[kScanThreads];
    const int tid = threadIdx.x;
    const int64_t seg = (nchunks + kScanThreads - 1) / kScanThreads;
    const int64_t lo = tid * seg, hi = lo + seg < nchunks ? lo + seg : nchunks;
    uint32_t s = 0;
    for (int64_t i = lo; i < hi; ++i) s += chunk_base[i];
    tot[tid] = s;
    __syncthreads();
    for (int off = 1; off < kScanThreads; off <<= 1) {         // inclusive Hillis-Steele
        const uint32_t v = tid >= off ? tot[tid - off] : 0u;
        __syncthreads();
        tot[tid] += v;
        __syncthreads();
    }
    uint32_t run = tot[tid] - s;
    for (int64_t i = lo; i < hi; ++i) {
        const uint32_t v = chunk_base[i];
        chunk_base[i] = run;
        run += v;
    }
}

// ---- the plan: everything below is called by all 64 lanes of one wave with the same arguments and returns the same value in every lane
// overflow records of the buffer at or before record i
__device__ __forceinline__ uint32_t overflow_prefix(const uint8_t* __restrict__ rec, const uint32_t* __restrict__ chunk_base, int64_t i) {
    const int lane = threadIdx.x & (EAS_WAVE - 1);
    const int64_t c0 = i & ~(int64_t)(kChunk - 1);
    uint32_t n = chunk_base[i >> kChunkShift];
#pragma unroll
    for (int j = 0; j < kChunk / EAS_WAVE; ++j) {
        const int64_t k = c0 + j * EAS_WAVE + lane;
        n += (uint32_t)__popcll(__ballot(k <= i && rec_y(rec, k) == kOverflowY));
    }
    return n;
}

// first event record in [i, hi), hi when there is none
__device__ __forceinline__ int64_t next_event(const uint8_t* __restrict__ rec, int64_t i, int64_t hi) {
    const int lane = threadIdx.x & (EAS_WAVE - 1);
    for (; i < hi; i += EAS_WAVE) {
        const unsigned long long m = __ballot(i + lane < hi && rec_y(rec, i + lane) != kOverflowY);
        if (m) return i + __builtin_ctzll(m);
    }
    return hi;
}

// last event record in [lo, i], lo - 1 when there is none
__device__ __forceinline__ int64_t prev_event(const uint8_t* __restrict__ rec, int64_t i, int64_t lo) {
    const int lane = threadIdx.x & (EAS_WAVE - 1);
    for (; i >= lo; i -= EAS_WAVE) {
        const unsigned long long m = __ballot(i - lane >= lo && rec_y(rec, i - lane) != kOverflowY);
        if (m) return i - __builtin_ctzll(m);
    }
    return lo - 1;
}

struct AtisRec {
    const uint8_t* rec;
    const uint32_t* chunk_base;
    uint32_t ovf_base;
    __device__ __forceinline__ int64_t time(int64_t i) const {
        return (int64_t)(rec_raw(rec, i) + kTimeIncrement * (overflow_prefix(rec, chunk_base, i) - ovf_base));
    }
};

// a record index r in [lo, hi]: every event in [lo, r) has t < key, every event in [r, hi) has t >= key (event times ascending)
__device__ __forceinline__ int64_t lower_bound_events(const AtisRec& R, int64_t lo, int64_t hi, int64_t key) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int64_t m = next_event(R.rec, mid, hi);       // the probe steps over overflow records
        if (m < hi && R.time(m) < key) lo = m + 1; else hi = mid;
    }
    return lo;
}

template <typename Src>
__global__ __launch_bounds__(EAS_WAVE) void atis_plan_kernel(const uint8_t* __restrict__ rec, int64_t nrec, const Src src,
                                                             const uint32_t* __restrict__ chunk_base, int64_t window_lo, int64_t window_hi,
                                                             int Tl, int Tm, AtisHead* __restrict__ heads, AtisSlice* __restrict__ slices,
                                                             uint32_t* __restrict__ t_target, uint32_t window0_flag,
                                                             uint32_t* __restrict__ oob, uint32_t* __restrict__ flags) {
    const int b = blockIdx.x;
    const bool writer = threadIdx.x == 0;
    int64_t a, e;
    uint32_t flag = src(b, nrec, a, e) ? 0u : 16u;
    AtisRec R = {rec, chunk_base, 0u};
    if (a > 0 && a < e) R.ovf_base = overflow_prefix(rec, chunk_base, a - 1);
    AtisHead h = {LLONG_MIN, LLONG_MAX, 0, 0, R.ovf_base, 0u};
    AtisSlice* rows = slices + (int64_t)b * Tl;
    int64_t ia = a, ib = e;
    const int64_t last = prev_event(rec, e - 1, a);
    bool any = last >= a;
    if (any && window_lo < 0) {
        const int64_t t_end = R.time(last);
        h.wl = t_end + window_lo;
        h.wh = t_end + window_hi;
        ia = lower_bound_events(R, a, e, h.wl + 1);
        ib = lower_bound_events(R, ia, e, h.wh + 1);
    }
    int64_t first = ib, lastr = ia - 1;
    if (any) {
        first = next_event(rec, ia, ib);
        lastr = prev_event(rec, ib - 1, ia);
        any = first < ib;
    }
    if (any) {
        h.t0 = R.time(first);
        const int64_t tl = R.time(lastr);
        h.mw = tl > h.t0 ? (tl - h.t0) / Tl : 0;
    }
    int64_t start = ia;
    for (int k = 0; k < Tl; ++k) {
        AtisSlice s = {0u, 0u};
        uint32_t target = 0u;                               // time of the slice's last member event (the time surface's t_target)
        bool members = false;
        if (h.mw > 0) {
            const int64_t end = lower_bound_events(R, start, ib, h.t0 + (int64_t)(k + 1) * h.mw);
            const int64_t fe = next_event(rec, start, end);
            if (fe < end) {
                members = true;
                const int64_t f = R.time(fe), l = R.time(prev_event(rec, end - 1, start));
                s.f = (uint32_t)f;
                s.w = l > f ? (uint32_t)((l - f) / Tm) : 0u;
                target = (uint32_t)l;
                if (t_target && end - start > kTsCapacity) flag |= 4u;     // more records than one 64-bit bin holds at weight 1
                if (s.w == 0u) flag |= window0_flag;                       // (the latest-time surface: 8, the reference raises; else 0)
            }
            start = end;
        }
        if (!members) flag |= 2u;
        if (writer) {
            rows[k] = s;
            if (t_target) t_target[(int64_t)b * Tl + k] = target;
        }
    }
    if (writer) {
        heads[b] = h;
        if (oob) oob[b] = 0u;
        if (flags) flags[b] = flag;
    }
}

// The 5 bytes of record i in the low 40 bits.  Two aligned 32-bit loads wherever both words lie inside the buffer -- a record spans
// exactly two aligned words at every alignment of the base address --, byte loads for the few records at the ends whose words do not.
__device__ __forceinline__ uint64_t load_record(const uint8_t* __restrict__ rec, int64_t nrec, int64_t i) {
    const uint8_t* p = rec + 5 * i;
    const uintptr_t o = (uintptr_t)p & 3;
    const uint8_t* w = p - o;
    if (w >= rec && w + 8 <= rec + 5 * nrec) {
        const uint32_t w0 = reinterpret_cast<const uint32_t*>(w)[0], w1 = reinterpret_cast<const uint32_t*>(w)[1];
        return (((uint64_t)w1 << 32) | w0) >> (8 * o);
    }
    return (uint64_t)p[0] | ((uint64_t)p[1] << 8) | ((uint64_t)p[2] << 16) | ((uint64_t)p[3] << 24) | ((uint64_t)p[4] << 32);
}

// ---- the accumulate step of the histogram: what an event of time t in macro slice `row` (= b * Tl + k) adds to its bin.  CountAcc (measure
// 'count') and LatestAcc (aggregation 'timesurface') are event_bin.h's, shared with the Gen1 sources; the time-surface measure is ATIS-only
struct TimeSurfaceAcc {                 // measure 'timesurface' (decay 'tanh'): 1 - tanh((t_target - t) / tau) in units of 2^-48
    typedef unsigned long long Bin;
    const uint32_t* t_target;           // [B * Tl], written by the plan
    double tau;
    __device__ __forceinline__ void operator()(Bin* bin, int64_t row, uint32_t t) const {
        // t <= t_target for every member of the slice (ascending times); the signed difference keeps w in [0, 2] whatever the records say
        const double w = 1.0 - tanh((double)((int64_t)t_target[row] - (int64_t)t) / tau);
        atomicAdd(bin, (Bin)llrint(w * kTsOne));
    }
};

template <typename Acc, typename Src>
__global__ __launch_bounds__(kChunk) void atis_hist_kernel(const uint8_t* __restrict__ rec, int64_t nrec, const Src src,
                                                           const uint32_t* __restrict__ chunk_base, const AtisHead* __restrict__ heads,
                                                           const AtisSlice* __restrict__ slices, int Tl, int Tm, int H, int W,
                                                           typename Acc::Bin* __restrict__ out, uint32_t* __restrict__ oob,
                                                           uint32_t* __restrict__ flags, const Acc acc) {
    __shared__ uint32_t wave_total[kChunk / EAS_WAVE];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & (EAS_WAVE - 1), wid = tid / EAS_WAVE;
    int64_t a, e;
    src(b, nrec, a, e);
    if (e <= a) return;
    const AtisHead h = heads[b];
    const AtisSlice* rows = slices + (int64_t)b * Tl;
    const int64_t c_last = (e - 1) >> kChunkShift;
    for (int64_t c = (a >> kChunkShift) + blockIdx.x; c <= c_last; c += gridDim.x) {
        const int64_t i = c * kChunk + tid;
        const uint64_t v = i < nrec ? load_record(rec, nrec, i) : 0ull;
        const uint32_t xx = (uint32_t)(v & 255u), yy = (uint32_t)((v >> 8) & 255u), b2 = (uint32_t)((v >> 16) & 255u);
        const uint32_t raw = ((b2 & 127u) << 16) | ((uint32_t)((v >> 24) & 255u) << 8) | (uint32_t)((v >> 32) & 255u);
        // overflow records of the chunk at or before this record (the chunk's records of a neighbouring recording count too: they are
        // part of the buffer-wide prefix that ovf_base is taken from)
        const unsigned long long m = __ballot(i < nrec && yy == kOverflowY);
        uint32_t before = (uint32_t)__popcll(m & (~0ull >> (EAS_WAVE - 1 - lane)));
        if (lane == 0) wave_total[wid] = (uint32_t)__popcll(m);
        __syncthreads();
        for (int w = 0; w < wid; ++w) before += wave_total[w];
        __syncthreads();
        if (i < a || i >= e || yy == kOverflowY) continue;
        const uint32_t nov = chunk_base[c] + before - h.ovf_base;
        const uint32_t t = raw + kTimeIncrement * nov;
        if (flags) {                                               // bit 0: the event in front of this one has a later time
            int64_t j = i - 1;
            while (j >= a && rec_y(rec, j) == kOverflowY) --j;   // (the records between the two events are overflow records)
            if (j >= a && rec_raw(rec, j) + kTimeIncrement * (nov - (uint32_t)(i - j - 1)) > t) atomicOr(flags + b, 1u);
        }
        if ((int64_t)t <= h.wl || (int64_t)t > h.wh || h.mw == 0 || (int64_t)t < h.t0) continue;
        const uint32_t k = (t - (uint32_t)h.t0) / (uint32_t)h.mw;
        if (k >= (uint32_t)Tl) continue;                           // the events on the last timestamp (Tl == 1) and the tail beyond Tl * mw
        const AtisSlice s = rows[k];
        if (s.w == 0 || t < s.f) continue;
        const uint32_t q = (t - s.f) / s.w;
        if (q >= (uint32_t)Tm) continue;
        if (xx >= (uint32_t)W || yy >= (uint32_t)H) {
            if (oob) atomicAdd(oob + b, 1u);
            continue;
        }
        const int ch = (b2 >> 7) != 0 ? 1 : 0;
        const int64_t row = (int64_t)b * Tl + k;
        acc(out + (((row * Tm + q) * 2 + ch) * H + yy) * W + xx, row, t);
    }
}

// the frames are zeroed by a kernel of the call's own (16-byte stores; torch hands out 16-byte aligned frames, a scalar loop otherwise)
__global__ __launch_bounds__(EAS_BLOCK) void atis_zero_kernel(int32_t* __restrict__ out, int64_t n) {
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    if (((uintptr_t)out & 15) == 0) {
        for (int64_t i = i0; i < n / 4; i += stride) reinterpret_cast<int4*>(out)[i] = make_int4(0, 0, 0, 0);
        for (int64_t i = (n & ~(int64_t)3) + i0; i < n; i += stride) out[i] = 0;
    } else {
        for (int64_t i = i0; i < n; i += stride) out[i] = 0;
    }
}

// the time surface's finishing pass, in place: a bin's integer sum (units of 2^-48) -> the double the frame holds
__global__ __launch_bounds__(EAS_BLOCK) void atis_ts_finish_kernel(unsigned long long* __restrict__ bins, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        bins[i] = __builtin_bit_cast(unsigned long long, (double)bins[i] * (1.0 / kTsOne));
}

// the latest-time surface's finishing pass (latest_surface.h) takes f and w of a row from the plan (w == 0: nothing was binned, zero frames)
struct AtisSliceWin {
    const AtisSlice* slices;
    __device__ __forceinline__ void operator()(int row, uint32_t& t0, uint32_t& win) const {
        const AtisSlice s = slices[row];
        t0 = s.f;
        win = s.w;
    }
};

inline int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }
inline int64_t chunks_of(int64_t nrec) { return (nrec + kChunk - 1) / kChunk; }
inline int64_t index_bytes(int64_t nrec) { return (chunks_of(nrec) + 1) * (int64_t)sizeof(uint32_t); }

// the workspace of a step: one head per recording, one row per (recording, macro slice), and -- behind what the count entry uses -- the
// time surface's t_target rows.  The packed entries keep their overflow index in front of it (align16(index_bytes(nrec)) bytes)
struct AtisWorkspace {
    int64_t slices, t_target, count_bytes, ts_bytes;                 // byte offsets behind the heads and the two totals
    AtisWorkspace(int B, int Tl) {
        slices = align16((int64_t)B * sizeof(AtisHead));
        t_target = count_bytes = slices + align16((int64_t)B * Tl * sizeof(AtisSlice));
        ts_bytes = t_target + align16((int64_t)B * Tl * sizeof(uint32_t));
    }
};

// launches 1 and 2: overflow records in front of every chunk of the buffer -> chunk_base [chunks + 1] (the last word: all of them)
int atis_index(const uint8_t* rec, int64_t nrec, uint32_t* chunk_base, hipStream_t st) {
    EAS_CLEAR_ERR();
    const int64_t n = chunks_of(nrec) + 1;                 // the chunk behind the last one holds no record: it counts 0
    EAS_LAUNCH(atis_overflow_count_kernel, dim3(eas_grid_1d(n, 1)), dim3(kChunk), 0, st, rec, nrec, n, chunk_base);
    EAS_CHECK_LAUNCH();
    EAS_LAUNCH(atis_overflow_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, chunk_base, n);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

// what the entry points of both families hand to the launches they share (arguments checked by the caller)
struct AtisCall {
    const uint8_t* rec;
    int64_t nrec;
    int B;
    int64_t window_lo, window_hi;
    int Tl, Tm, H, W;
    uint32_t *oob_count, *flags;
    const uint32_t* chunk_base;         // the overflow index of the buffer
    void* workspace;                    // AtisWorkspace(B, Tl)
    int64_t per;                        // histogram blocks per recording
    hipStream_t st;
    AtisSlice* slices() const { return (AtisSlice*)((char*)workspace + AtisWorkspace(B, Tl).slices); }
    uint32_t* t_target() const { return (uint32_t*)((char*)workspace + AtisWorkspace(B, Tl).t_target); }
    int64_t nout() const { return (int64_t)B * Tl * Tm * 2 * H * W; }
};

// Launches 0, 3 and 4.  t_target: NULL but for the time-surface measure; window0_flag: the flag bits of a macro slice that holds events
// and has micro window 0 (8 for the latest-time surface, else 0).
template <typename Acc, typename Src>
int atis_frames(const AtisCall& c, const Src& src, typename Acc::Bin* out, uint32_t* t_target, uint32_t window0_flag, const Acc& acc) {
    const int64_t far = (int64_t)1 << 40;                  // decoded times fit 32 bits: a bound beyond +-2^40 selects what 2^40 selects
    const int64_t window_lo = c.window_lo < -far ? -far : c.window_lo;
    const int64_t window_hi = c.window_hi > far ? far : (c.window_hi < -far ? -far : c.window_hi);
    EAS_CLEAR_ERR();
    AtisHead* heads = (AtisHead*)c.workspace;
    AtisSlice* slices = c.slices();
    const int64_t nwords = c.nout() * (int64_t)(sizeof(typename Acc::Bin) / sizeof(int32_t));
    EAS_LAUNCH(atis_zero_kernel, dim3(eas_grid_1d((nwords + 3) / 4)), dim3(EAS_BLOCK), 0, c.st, (int32_t*)out, nwords);
    EAS_CHECK_LAUNCH();
    EAS_LAUNCH(atis_plan_kernel<Src>, dim3(c.B), dim3(EAS_WAVE), 0, c.st, c.rec, c.nrec, src, c.chunk_base, window_lo, window_hi, c.Tl, c.Tm, heads,
               slices, t_target, window0_flag, c.oob_count, c.flags);
    EAS_CHECK_LAUNCH();
    if (c.nrec > 0) {
        // the recordings' lengths live on the device: a fixed number of blocks per recording strides over whatever it holds
        EAS_LAUNCH((atis_hist_kernel<Acc, Src>), dim3((unsigned)c.per, c.B), dim3(kChunk), 0, c.st, c.rec, c.nrec, src, c.chunk_base, heads, slices,
                   c.Tl, c.Tm, c.H, c.W, out, c.oob_count, c.flags, acc);
        EAS_CHECK_LAUNCH();
    }
    return EAS_OK;
}

// ---- the three representations, for either range source
template <typename Src>
int atis_counts(const AtisCall& c, const Src& src, int32_t* out) {
    return atis_frames(c, src, out, nullptr, 0u, CountAcc{});
}

template <typename Src>
int atis_timesurface(const AtisCall& c, const Src& src, double tau, double* out) {
    unsigned long long* bins = reinterpret_cast<unsigned long long*>(out);
    uint32_t* t_target = c.t_target();
    const int launched = atis_frames(c, src, bins, t_target, 0u, TimeSurfaceAcc{t_target, tau});
    if (launched != EAS_OK) return launched;
    EAS_LAUNCH(atis_ts_finish_kernel, dim3(eas_grid_1d(c.nout())), dim3(EAS_BLOCK), 0, c.st, bins, c.nout());
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

template <typename Src>
int atis_latest_surface(const AtisCall& c, const Src& src, double tau, double* out) {
    unsigned long long* bins = reinterpret_cast<unsigned long long*>(out);
    const int launched = atis_frames(c, src, bins, nullptr, 8u, LatestAcc{});
    if (launched != EAS_OK) return launched;
    const int64_t nrows = (int64_t)c.B * c.Tl;
    EAS_LAUNCH(latest_finish_kernel<AtisSliceWin>, dim3(eas_grid_1d(nrows * 2 * c.H * c.W)), dim3(EAS_BLOCK), 0, c.st, nrows, c.Tm, c.H, c.W, tau, bins,
               AtisSliceWin{c.slices()});
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

inline int64_t hist_blocks(int64_t chunks) { return chunks + 1 > 64 ? 64 : chunks + 1; }

// the argument rules the entry points share
int atis_check_args(const void* records, int64_t nrec, const void* ranges, int B, int Tl, int Tm, int H, int W, const void* out,
                    const void* workspace) {
    if (!out || !ranges || !workspace || B < 1 || Tl < 1 || Tm < 1 || H < 1 || W < 1 || nrec < 0) return EAS_ERR_INVALID_ARG;
    if ((nrec > 0 && !records) || ((uintptr_t)workspace & 15) || nrec > (INT64_MAX >> 3)) return EAS_ERR_INVALID_ARG;
    if ((int64_t)B * Tl >= (1 << 24) || B > 65535) return EAS_ERR_UNSUPPORTED;
    return EAS_OK;
}

// a packed entry: checks, then index and frames on its own workspace (the index in front, the step's workspace behind it)
template <typename Frames>
int atis_packed(const void* records, int64_t nrec, const int64_t* sample_offsets, int B, int64_t window_lo, int64_t window_hi, int Tl, int Tm, int H,
                int W, const void* out, uint32_t* oob_count, uint32_t* flags, void* workspace, eas_stream_t stream, const Frames& frames) {
    const int rc = atis_check_args(records, nrec, sample_offsets, B, Tl, Tm, H, W, out, workspace);
    if (rc != EAS_OK) return rc;
    uint32_t* chunk_base = (uint32_t*)workspace;
    const AtisCall c = {(const uint8_t*)records, nrec, B, window_lo, window_hi, Tl, Tm, H, W, oob_count, flags, chunk_base,
                        (char*)workspace + align16(index_bytes(nrec)), hist_blocks(chunks_of(nrec) / B), eas_s(stream)};
    if (nrec > 0) {
        const int indexed = atis_index(c.rec, nrec, chunk_base, c.st);
        if (indexed != EAS_OK) return indexed;
    }
    return frames(c, PackedRanges{sample_offsets});
}

// a store entry: checks, then the frames of the B recordings sample_file picks, on the store's index
template <typename Frames>
int atis_store(const void* records, int64_t nrec, const int64_t* file_offsets, int64_t F, const int64_t* sample_file, int B,
               const uint32_t* chunk_base, int64_t max_file_records, int64_t window_lo, int64_t window_hi, int Tl, int Tm, int H, int W,
               const void* out, uint32_t* oob_count, uint32_t* flags, void* workspace, eas_stream_t stream, const Frames& frames) {
    const int rc = atis_check_args(records, nrec, sample_file, B, Tl, Tm, H, W, out, workspace);
    if (rc != EAS_OK) return rc;
    if (!file_offsets || !chunk_base || F < 0 || max_file_records < 0) return EAS_ERR_INVALID_ARG;
    const AtisCall c = {(const uint8_t*)records, nrec, B, window_lo, window_hi, Tl, Tm, H, W, oob_count, flags, chunk_base, workspace,
                        hist_blocks(chunks_of(max_file_records)), eas_s(stream)};
    return frames(c, StoreRanges{file_offsets, F, sample_file});
}

}  // namespace

extern "C" {

int64_t eas_event_histogram_atis_workspace_bytes(int64_t nrec, int B, int Tl) {
    if (nrec < 0 || B < 1 || Tl < 1) return 0;
    return align16(index_bytes(nrec)) + AtisWorkspace(B, Tl).count_bytes;
}

int eas_event_histogram_atis(const void* records, int64_t nrec, const int64_t* sample_offsets, int B, int64_t window_lo, int64_t window_hi,
                             int Tl, int Tm, int H, int W, int32_t* out, uint32_t* oob_count, uint32_t* flags, void* workspace,
                             eas_stream_t stream) {
    return atis_packed(records, nrec, sample_offsets, B, window_lo, window_hi, Tl, Tm, H, W, out, oob_count, flags, workspace, stream,
                       [=](const AtisCall& c, const PackedRanges& src) { return atis_counts(c, src, out); });
}

int64_t eas_event_timesurface_atis_workspace_bytes(int64_t nrec, int B, int Tl) {
    if (nrec < 0 || B < 1 || Tl < 1) return 0;
    return align16(index_bytes(nrec)) + AtisWorkspace(B, Tl).ts_bytes;
}

int64_t eas_event_timesurface_atis_capacity(void) { return kTsCapacity; }

int eas_event_timesurface_atis(const void* records, int64_t nrec, const int64_t* sample_offsets, int B, int64_t window_lo, int64_t window_hi,
                               int Tl, int Tm, int H, int W, double tau, double* out, uint32_t* oob_count, uint32_t* flags, void* workspace,
                               eas_stream_t stream) {
    if (!(tau > 0.0)) return EAS_ERR_INVALID_ARG;          // also NaN
    return atis_packed(records, nrec, sample_offsets, B, window_lo, window_hi, Tl, Tm, H, W, out, oob_count, flags, workspace, stream,
                       [=](const AtisCall& c, const PackedRanges& src) { return atis_timesurface(c, src, tau, out); });
}

int eas_event_latest_surface_atis(const void* records, int64_t nrec, const int64_t* sample_offsets, int B, int64_t window_lo, int64_t window_hi,
                                  int Tl, int Tm, int H, int W, double tau, double* out, uint32_t* oob_count, uint32_t* flags, void* workspace,
                                  eas_stream_t stream) {
    if (!(tau > 0.0)) return EAS_ERR_INVALID_ARG;          // also NaN
    return atis_packed(records, nrec, sample_offsets, B, window_lo, window_hi, Tl, Tm, H, W, out, oob_count, flags, workspace, stream,
                       [=](const AtisCall& c, const PackedRanges& src) { return atis_latest_surface(c, src, tau, out); });
}

// ---- a store: the index once, then steps whose work is the batch's
int64_t eas_atis_store_index_bytes(int64_t nrec) { return nrec < 0 ? 0 : index_bytes(nrec); }

int eas_atis_store_index(const void* records, int64_t nrec, uint32_t* chunk_base, eas_stream_t stream) {
    if (!chunk_base || nrec < 0 || (nrec > 0 && !records) || nrec > (INT64_MAX >> 3)) return EAS_ERR_INVALID_ARG;
    return atis_index((const uint8_t*)records, nrec, chunk_base, eas_s(stream));
}

int64_t eas_atis_store_workspace_bytes(int B, int Tl) { return B < 1 || Tl < 1 ? 0 : AtisWorkspace(B, Tl).count_bytes; }
int64_t eas_atis_store_timesurface_workspace_bytes(int B, int Tl) { return B < 1 || Tl < 1 ? 0 : AtisWorkspace(B, Tl).ts_bytes; }

int eas_event_histogram_atis_store(const void* records, int64_t nrec, const int64_t* file_offsets, int64_t F, const int64_t* sample_file, int B,
                                   const uint32_t* chunk_base, int64_t max_file_records, int64_t window_lo, int64_t window_hi, int Tl, int Tm,
                                   int H, int W, int32_t* out, uint32_t* oob_count, uint32_t* flags, void* workspace, eas_stream_t stream) {
    return atis_store(records, nrec, file_offsets, F, sample_file, B, chunk_base, max_file_records, window_lo, window_hi, Tl, Tm, H, W, out,
                      oob_count, flags, workspace, stream, [=](const AtisCall& c, const StoreRanges& src) { return atis_counts(c, src, out); });
}

int eas_event_timesurface_atis_store(const void* records, int64_t nrec, const int64_t* file_offsets, int64_t F, const int64_t* sample_file, int B,
                                     const uint32_t* chunk_base, int64_t max_file_records, int64_t window_lo, int64_t window_hi, int Tl, int Tm,
                                     int H, int W, double tau, double* out, uint32_t* oob_count, uint32_t* flags, void* workspace,
                                     eas_stream_t stream) {
    if (!(tau > 0.0)) return EAS_ERR_INVALID_ARG;          // also NaN
    return atis_store(records, nrec, file_offsets, F, sample_file, B, chunk_base, max_file_records, window_lo, window_hi, Tl, Tm, H, W, out,
                      oob_count, flags, workspace, stream,
                      [=](const AtisCall& c, const StoreRanges& src) { return atis_timesurface(c, src, tau, out); });
}

int eas_event_latest_surface_atis_store(const void* records, int64_t nrec, const int64_t* file_offsets, int64_t F, const int64_t* sample_file, int B,
                                        const uint32_t* chunk_base, int64_t max_file_records, int64_t window_lo, int64_t window_hi, int Tl,
                                        int Tm, int H, int W, double tau, double* out, uint32_t* oob_count, uint32_t* flags, void* workspace,
                                        eas_stream_t stream) {
    if (!(tau > 0.0)) return EAS_ERR_INVALID_ARG;          // also NaN
    return atis_store(records, nrec, file_offsets, F, sample_file, B, chunk_base, max_file_records, window_lo, window_hi, Tl, Tm, H, W, out,
                      oob_count, flags, workspace, stream,
                      [=](const AtisCall& c, const StoreRanges& src) { return atis_latest_surface(c, src, tau, out); });
}

}  // extern "C"
