// K1: raw (t, x, y, p) event streams -> per-polarity count frames / voxel grids.
// Integer scatter: HBM/atomic bound.  Algorithmic bytes per sample: 9 B per event read
// (u32 t + u16 x + u16 y + u8 p) + 4*Tm*2*H*W B for the frames (zero-fill + result).
// One thread handles 4 consecutive events (16-B / 8-B / 8-B / 4-B vector loads); the atomics are
// int32 `global_atomic_add` without return, so results are bit-exact and order independent.
// Every source (decoded arrays, .dat records with offsets, .dat record ranges) sends an event to its bin, a count or a latest time, by one route:
// bin_event<Acc> (event_bin.h).  Record ranges: one walk, dat_ranges_kernel<Acc, Src>, behind one host template, ranges_frames<Acc, Src>
// (Src, record_source.h: the 8-byte records or the packed records of records.hip).
#include <stdlib.h>

#include <string.h>

#include "eas_common.h"
#include "count_resize.h"
#include "event_bin.h"
#include "record_source.h"
#include "latest_surface.h"

namespace {

// sample index of event i: largest b with offsets[b] <= i  (offsets ascending, offsets[B] = nev)
__device__ __forceinline__ int find_sample(const int64_t* __restrict__ offsets, int B, int64_t i) {
    int lo = 0, hi = B;  // invariant: offsets[lo] <= i < offsets[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ SampleWin sample_window(const uint32_t* __restrict__ t, const int64_t* __restrict__ offsets,
                                                   int b, int Tm) {
    return make_window(t[offsets[b]], t[offsets[b + 1] - 1], Tm);
}

// the count's reading of the polarity byte: p != 0 is channel 1
__device__ __forceinline__ void bin_one(uint32_t tt, uint32_t xx, uint32_t yy, uint32_t pp, const SampleWin& w, int b,
                                        int Tm, int H, int W, int32_t* __restrict__ out, uint32_t* __restrict__ oob) {
    bin_event(tt, xx, yy, pp != 0 ? 1u : 0u, w, b, Tm, H, W, out, oob, CountAcc{});
}

template <bool VEC4>
__global__ __launch_bounds__(EAS_BLOCK) void event_hist_kernel(const uint32_t* __restrict__ t, const uint16_t* __restrict__ x,
                                                               const uint16_t* __restrict__ y, const uint8_t* __restrict__ p,
                                                               int64_t nev, const int64_t* __restrict__ offsets, int B,
                                                               int Tm, int H, int W, int32_t* __restrict__ out,
                                                               uint32_t* __restrict__ oob) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    if (VEC4) {
        const int64_t ngroups = nev / 4;
        for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += stride) {
            const uint4 tv = reinterpret_cast<const uint4*>(t)[g];
            const ushort4 xv = reinterpret_cast<const ushort4*>(x)[g];
            const ushort4 yv = reinterpret_cast<const ushort4*>(y)[g];
            const uchar4 pv = reinterpret_cast<const uchar4*>(p)[g];
            const int64_t i0 = g * 4;
            int b = find_sample(offsets, B, i0);
            SampleWin w = sample_window(t, offsets, b, Tm);
            int64_t end = offsets[b + 1];
            const uint32_t ts[4] = {tv.x, tv.y, tv.z, tv.w};
            const uint32_t xs[4] = {xv.x, xv.y, xv.z, xv.w};
            const uint32_t ys[4] = {yv.x, yv.y, yv.z, yv.w};
            const uint32_t ps[4] = {pv.x, pv.y, pv.z, pv.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                while (i0 + e >= end) {  // group straddles a sample boundary (also skips empty samples)
                    ++b;
                    end = offsets[b + 1];
                    if (i0 + e < end) w = sample_window(t, offsets, b, Tm);
                }
                bin_one(ts[e], xs[e], ys[e], ps[e], w, b, Tm, H, W, out, oob);
            }
        }
        // the last nev % 4 events
        if (blockIdx.x == 0 && threadIdx.x < (nev & 3)) {
            const int64_t i = (nev & ~(int64_t)3) + threadIdx.x;
            const int b = find_sample(offsets, B, i);
            const SampleWin w = sample_window(t, offsets, b, Tm);
            bin_one(t[i], x[i], y[i], p[i], w, b, Tm, H, W, out, oob);
        }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nev; i += stride) {
            const int b = find_sample(offsets, B, i);
            const SampleWin w = sample_window(t, offsets, b, Tm);
            bin_one(t[i], x[i], y[i], p[i], w, b, Tm, H, W, out, oob);
        }
    }
}

// Same binning straight from Prophesee .dat records (8 bytes: u32 t, u32 packed with x = bits 0..13, y = bits 14..27,
// p = bit 28; yolox/utils/psee_loader/io/dat_events_tools.py:24-54): decode + window + histogram in one pass, so the raw
// file bytes are the only thing that crosses PCIe.  Two records per thread (one 16-byte load) when the buffer is aligned.
__device__ __forceinline__ SampleWin sample_window_dat(const uint2* __restrict__ rec, const int64_t* __restrict__ offsets, int b, int Tm) {
    return make_window(rec[offsets[b]].x, rec[offsets[b + 1] - 1].x, Tm);
}

__device__ __forceinline__ void bin_dat(uint32_t tt, uint32_t packed, const SampleWin& w, int b, int Tm, int H, int W,
                                        int32_t* __restrict__ out, uint32_t* __restrict__ oob) {
    bin_one(tt, packed & 16383u, (packed >> 14) & 16383u, (packed >> 28) & 1u, w, b, Tm, H, W, out, oob);
}

template <bool VEC2>
__global__ __launch_bounds__(EAS_BLOCK) void event_hist_dat_kernel(const uint2* __restrict__ rec, int64_t nev,
                                                                   const int64_t* __restrict__ offsets, int B, int Tm, int H, int W,
                                                                   int32_t* __restrict__ out, uint32_t* __restrict__ oob) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    if (VEC2) {
        const int64_t npairs = nev / 2;
        for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < npairs; g += stride) {
            const uint4 v = reinterpret_cast<const uint4*>(rec)[g];
            const int64_t i0 = g * 2;
            int b = find_sample(offsets, B, i0);
            SampleWin w = sample_window_dat(rec, offsets, b, Tm);
            bin_dat(v.x, v.y, w, b, Tm, H, W, out, oob);
            if (i0 + 1 >= offsets[b + 1]) {           // the pair straddles a sample boundary (also skips empty samples)
                b = find_sample(offsets, B, i0 + 1);
                w = sample_window_dat(rec, offsets, b, Tm);
            }
            bin_dat(v.z, v.w, w, b, Tm, H, W, out, oob);
        }
        if ((nev & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
            const int64_t i = nev - 1;
            const int b = find_sample(offsets, B, i);
            bin_dat(rec[i].x, rec[i].y, sample_window_dat(rec, offsets, b, Tm), b, Tm, H, W, out, oob);
        }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nev; i += stride) {
            const int b = find_sample(offsets, B, i);
            bin_dat(rec[i].x, rec[i].y, sample_window_dat(rec, offsets, b, Tm), b, Tm, H, W, out, oob);
        }
    }
}

// ---- timestamp-window search on the device (second half) ------------------------------------------
// GEN1Dataset.search_events (yolox/data/datasets/gen1.py:217-232) over PSEELoader.seek_time / load_delta_t
// (yolox/utils/psee_loader/io/psee_loader.py:128-238), per label: the events of [ts + w0, ts + w0 + (w1 - w0)); while that is
// empty the window steps back by its own length, num_slice + 2 attempts at most.  The reader's quirks are kept, because they
// decide which events a sample is made of:
//   seek_time(T): T past the last timestamp -> end of file; T <= 0 -> first event AND current time 0 (not T); otherwise a
//   bisection that probes t[middle] while more than 100 000 events remain -- a probe that equals T exactly leaves the reader
//   one event AFTER the probed one -- then the first event with t >= T;  load_delta_t(d): events up to the first with
//   t >= current time + d.
// One thread per label; a recording is records [file_offsets[f], file_offsets[f + 1]) of the .dat image in HBM.
constexpr int64_t kSeekTermCriterion = 100000;

__device__ __forceinline__ int64_t lower_bound_rec(const uint2* __restrict__ rec, int64_t lo, int64_t hi, int64_t key) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)rec[mid].x < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(EAS_WAVE) void event_window_search_kernel(const uint2* __restrict__ rec, const int64_t* __restrict__ file_offsets,
                                                                       const int32_t* __restrict__ file_id,
                                                                       const int64_t* __restrict__ label_t, int B, int64_t w0, int64_t w1,
                                                                       int num_slice, int64_t* __restrict__ ranges) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int f = file_id ? file_id[b] : 0;
    const int64_t base = file_offsets[f], n = file_offsets[f + 1] - base;
    const uint2* r = rec + base;
    const int64_t delta = w1 - w0;
    const int64_t total = n > 0 ? (int64_t)r[n - 1].x : 0;
    int64_t cur = label_t[b] + w0;
    int64_t a = 0, e = 0;
    for (int attempt = 0; attempt <= num_slice + 1; ++attempt, cur -= delta) {
        int64_t pos, now;
        if (cur > total) { pos = n; now = total + 1; }
        else if (cur <= 0) { pos = 0; now = 0; }
        else {
            int64_t low = 0, high = n;
            pos = -1;
            while (high - low > kSeekTermCriterion) {
                const int64_t middle = (low + high) / 2;
                const int64_t mid = (int64_t)r[middle].x;
                if (mid > cur) high = middle;
                else if (mid < cur) low = middle + 1;
                else { pos = middle + 1; break; }
            }
            if (pos < 0) pos = lower_bound_rec(r, low, high, cur);
            now = cur;
        }
        a = pos;
        e = pos >= n ? pos : lower_bound_rec(r, pos, n, now + delta);
        if (e > a) break;
    }
    ranges[2 * b] = base + a;
    ranges[2 * b + 1] = base + e;
}

// Samples given as arbitrary (possibly overlapping) record ranges of a .dat image: blockIdx.y = sample, blocks stride over its range; nothing
// is read back.  ``Acc`` (event_bin.h) is the difference between the frames: CountAcc -> micro-slice count frames, LatestAcc -> the latest
// times in the output's own 64-bit bins (eas_event_latest_surface_*_ranges, finished by latest_finish_kernel).  ``Src`` (record_source.h)
// is where record i comes from: RawRecords -> the 8-byte records (the _dat_ranges entries), PackedRecords -> the packed records (the
// _packed_ranges entries).  The window of a range is the one rule for the walk and for the finishing pass (RangesWin).
template <typename Src>
__device__ __forceinline__ SampleWin ranges_window(const Src& src, int64_t a, int64_t e, int ns) {
    RecEvent first, last;
    if (!src.admit(a, e) || !src.load(a, first) || !src.load(e - 1, last)) return SampleWin{0u, 0u};
    return make_window(first.t, last.t, ns);
}

template <typename Acc, typename Src>
__global__ __launch_bounds__(EAS_BLOCK) void dat_ranges_kernel(const Src src, const int64_t* __restrict__ ranges, int ns, int H, int W,
                                                               typename Acc::Bin* __restrict__ out, uint32_t* __restrict__ oob, const Acc acc) {
    const int b = blockIdx.y;
    const int64_t a = ranges[2 * b], e = ranges[2 * b + 1];
    const SampleWin w = ranges_window(src, a, e, ns);
    if (w.win == 0) return;                        // (empty, refused, or a window of zero length: bin_event would drop every event)
    for (int64_t i = a + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < e; i += (int64_t)gridDim.x * blockDim.x) {
        RecEvent v;
        if (src.load(i, v)) bin_event(v.t, v.x, v.y, v.p, w, b, ns, H, W, out, oob, acc);
    }
}

// the window of sample b of such ranges, for the finishing pass (latest_surface.h latest_finish_kernel)
template <typename Src>
struct RangesWin {
    Src src; const int64_t* ranges; int ns;
    __device__ __forceinline__ void operator()(int b, uint32_t& t0, uint32_t& win) const {
        const SampleWin w = ranges_window(src, ranges[2 * b], ranges[2 * b + 1], ns);
        t0 = w.t0;
        win = w.win;
    }
};

// LDS-privatised form of the histogram for streams with many events per frame: one block owns one (sample, micro-slice,
// band of rows) and keeps that band's two polarity planes in LDS (<= 150 KB).  The events of a micro-slice are a
// contiguous run of the time-sorted stream (two binary searches = the reference's np.searchsorted, gen1.py:324-325), so the
// block streams through that run with coalesced loads, counts the events that fall into its rows with LDS atomics, and
// writes its band once with coalesced stores: no global atomics, no zero-fill pass, every output element written
// exactly once.  Each event is read by every band of its slice (L2-resident re-reads); bit-exact like the scatter form.
constexpr int kBandThreads = 1024;
constexpr int kBandLdsBytes = 150 * 1024;
constexpr int kMaxBands = 8;

// A lower bound found by the 64 lanes of one wave: a round probes the last elements of 64 equal sub-ranges with ONE load per lane and
// keeps the sub-range that holds the answer -- 3 dependent rounds for a 200 k-event sample instead of the 18 dependent loads of the binary
// search (each a full HBM round trip issued by a single thread: the two searches of a block were ~25 us of its ~45 us).  All lanes of
// the wave call it with the same arguments and get the same result.
__device__ __forceinline__ int64_t lower_bound_wave(const uint32_t* __restrict__ t, int64_t lo, int64_t hi, uint32_t key) {
    const int lane = threadIdx.x & (EAS_WAVE - 1);
    while (hi - lo > EAS_WAVE) {
        const int64_t n = hi - lo, step = (n + EAS_WAVE - 1) / EAS_WAVE;
        const int64_t end = (lane + 1) * step < n ? (lane + 1) * step : n;          // sub-range `lane` = [lane * step, end) (empty ones probe the last element)
        const bool below = t[lo + end - 1] < key;                                    // sorted: the whole sub-range is below the key
        const int c = __popcll(__ballot(below));                                     // the lanes form 1..10..0: c sub-ranges lie below
        if (c == EAS_WAVE) return hi;
        const int64_t nlo = lo + c * step, nhi = lo + ((c + 1) * step < n ? (c + 1) * step : n);
        lo = nlo;
        hi = nhi;
    }
    const int64_t i = lo + lane;
    const bool below = i < hi && t[i] < key;
    return lo + __popcll(__ballot(below));
}

// ---- the band form: two kernels over shared pieces (block mapping, range search, zero-fill, per-event count, write-out of a pass) -----
__device__ __forceinline__ void band_zero(int* cnt, int words, bool vec4) {
    if (vec4) {
        for (int i = threadIdx.x; i < words / 4; i += kBandThreads) reinterpret_cast<int4*>(cnt)[i] = make_int4(0, 0, 0, 0);
    } else {
        for (int i = threadIdx.x; i < words; i += kBandThreads) cnt[i] = 0;
    }
}

// counter idx of a pass: wide = one 32-bit word each, packed = two 16-bit counters per word;  packed4: four consecutive ones, one 8-byte read
__device__ __forceinline__ int band_counter(const int* cnt, int idx, bool packed) {
    return packed ? (int)(((unsigned)cnt[idx >> 1] >> (16 * (idx & 1))) & 0xffffu) : cnt[idx];
}
__device__ __forceinline__ int4 band_packed4(const int* cnt, int idx) {
    const uint2 w = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(cnt) + idx);
    return make_int4((int)(w.x & 0xffffu), (int)(w.x >> 16), (int)(w.y & 0xffffu), (int)(w.y >> 16));
}

// one event into the counters [2][plane] of rows [ya, yb); events outside the sensor are tallied in the first pass only
__device__ __forceinline__ void band_count_one(unsigned xv, unsigned yv, unsigned pv, int H, int W, int ya, int yb, int plane, bool packed,
                                               bool first, int* cnt, unsigned& bad) {
    if (xv >= (unsigned)W || yv >= (unsigned)H) {
        if (first) ++bad;
        return;
    }
    if (yv < (unsigned)ya || yv >= (unsigned)yb) return;
    const int idx = (pv != 0 ? plane : 0) + (int)(yv - ya) * W + (int)xv;
    if (packed) atomicAdd(&cnt[idx >> 1], (idx & 1) ? 65536 : 1);
    else atomicAdd(&cnt[idx], 1);
}

// The counters of a pass (rows [ya, yb) of polarity frames ``frame``, ``frame + 1``) to the int32 counts, or as fp32 into the zero-padded
// model canvas [B][Tm][2][Hc][Wc] (gen1.py:447-455 + trainer.py:99 cast): the rows with their right padding down to row yend (Hc in the
// last pass of the last band: the bottom padding).  16-byte stores where the layout allows (the wide counters: WIDE_VEC, counts only).
template <bool WIDE_VEC>
__device__ __forceinline__ void band_write_pass(const int* cnt, bool packed, int plane, int W, int ya, int yb, int yend, int64_t frame, int H,
                                                int32_t* __restrict__ out, float* __restrict__ canvas, int Hc, int Wc) {
    const int tid = threadIdx.x;
    if (canvas) {
        const bool quads = packed && (W & 3) == 0 && (Wc & 3) == 0 && (plane & 3) == 0 && ((uintptr_t)canvas & 15) == 0;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            float* dst = canvas + ((frame + c) * Hc + ya) * Wc;
            if (quads) {                                      // four columns per thread
                const int q4 = Wc / 4, total4 = (yend - ya) * q4;
                for (int i = tid; i < total4; i += kBandThreads) {
                    const int r = i / q4, col = (i - r * q4) * 4;
                    int4 v = make_int4(0, 0, 0, 0);
                    if (r < yb - ya && col < W) v = band_packed4(cnt, c * plane + r * W + col);
                    *reinterpret_cast<float4*>(dst + (int64_t)r * Wc + col) = make_float4((float)v.x, (float)v.y, (float)v.z, (float)v.w);
                }
                continue;
            }
            const int total = (yend - ya) * Wc;
            for (int i = tid; i < total; i += kBandThreads) {
                const int r = i / Wc, col = i - r * Wc;
                dst[i] = (r < yb - ya && col < W) ? (float)band_counter(cnt, c * plane + r * W + col, packed) : 0.0f;
            }
        }
        return;
    }
    const int n = (yb - ya) * W;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        int32_t* dst = out + ((frame + c) * H + ya) * W;         // the band's rows are contiguous in the output as in LDS
        if ((packed || WIDE_VEC) && (n & 3) == 0 && (plane & 3) == 0 && ((uintptr_t)dst & 15) == 0) {
            if (packed) for (int i = tid; i < n / 4; i += kBandThreads) reinterpret_cast<int4*>(dst)[i] = band_packed4(cnt, c * plane + 4 * i);
            else for (int i = tid; i < n / 4; i += kBandThreads) reinterpret_cast<int4*>(dst)[i] = reinterpret_cast<const int4*>(cnt + c * plane)[i];
        } else {
            for (int i = tid; i < n; i += kBandThreads) dst[i] = band_counter(cnt, c * plane + i, packed);
        }
    }
}

// One block = one (sample, micro-slice, band of rows).  XCD-aware order: consecutive workgroup ids go round-robin over the 8 XCDs, so the
// bands of one (sample, slice) get ids 8 apart -- same XCD, one L2: the slice's events come from HBM once and from that L2 for the other
// bands.  false: a block past the last slice
struct BandBlock { int b, k, band, y0, y1; };

__device__ __forceinline__ bool band_of_block(int nbands, int B, int Tm, int rows, int H, BandBlock& bb) {
    const int L = blockIdx.x;
    const int sl = (L & 7) + 8 * (L / (8 * nbands));
    if (sl >= B * Tm) return false;
    bb.band = (L >> 3) % nbands;
    bb.b = sl / Tm;
    bb.k = sl - bb.b * Tm;
    bb.y0 = bb.band * rows;
    bb.y1 = bb.y0 + rows < H ? bb.y0 + rows : H;
    return true;
}

// the event range [range[0], range[1]) of micro-slice k of sample b into LDS: searched by the first wave (lower_bound_wave)
__device__ __forceinline__ void band_slice_range(const uint32_t* __restrict__ t, const int64_t* __restrict__ offsets, int b, int k, int Tm,
                                                 int64_t* range) {
    if (threadIdx.x < EAS_WAVE) {
        const int64_t a = offsets[b], e = offsets[b + 1];
        int64_t lo = 0, hi = 0;
        if (e > a) {
            const SampleWin w = make_window(t[a], t[e - 1], Tm);
            if (w.win != 0) {
                lo = lower_bound_wave(t, a, e, w.t0 + (uint32_t)k * w.win);
                hi = lower_bound_wave(t, lo, e, w.t0 + (uint32_t)(k + 1) * w.win);
            }
        }
        if (threadIdx.x == 0) {
            range[0] = lo;
            range[1] = hi;
        }
    }
}

// 32-bit counters [2][rows][W]: one pass, one event per load with UN loads per array issued before the first LDS atomic, int4 zero-fill
// (issued before the range search) and copy-out
__global__ __launch_bounds__(kBandThreads) void event_hist_banded_kernel(const uint32_t* __restrict__ t, const uint16_t* __restrict__ x,
                                                                         const uint16_t* __restrict__ y, const uint8_t* __restrict__ p,
                                                                         const int64_t* __restrict__ offsets, int B, int Tm, int H, int W,
                                                                         int rows, int nbands, int32_t* __restrict__ out,
                                                                         uint32_t* __restrict__ oob, float* __restrict__ canvas, int Hc,
                                                                         int Wc) {
    extern __shared__ int cnt[];
    __shared__ int64_t range[2];
    BandBlock bb;
    if (!band_of_block(nbands, B, Tm, rows, H, bb)) return;
    const int tid = threadIdx.x, plane = rows * W;
    band_zero(cnt, 2 * plane, (plane & 3) == 0);
    band_slice_range(t, offsets, bb.b, bb.k, Tm, range);
    __syncthreads();
    const int64_t lo = range[0], hi = range[1];
    unsigned bad = 0;
    constexpr int UN = 4;
    for (int64_t i0 = lo + tid; i0 < hi; i0 += (int64_t)UN * kBandThreads) {
        unsigned xs[UN], ys[UN], ps[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int64_t i = i0 + (int64_t)u * kBandThreads;
            const bool in = i < hi;
            xs[u] = in ? x[i] : 0u;
            ys[u] = in ? y[i] : 0xffffffffu;          // sentinel: neither counted nor out-of-range
            ps[u] = in ? p[i] : 0u;
        }
#pragma unroll
        for (int u = 0; u < UN; ++u)
            if (ys[u] != 0xffffffffu) band_count_one(xs[u], ys[u], ps[u], H, W, bb.y0, bb.y1, plane, false, true, cnt, bad);
    }
    __syncthreads();
    band_write_pass<true>(cnt, false, plane, W, bb.y0, bb.y1, bb.band == nbands - 1 ? Hc : bb.y1, ((int64_t)bb.b * Tm + bb.k) * 2, H, out, canvas,
                          Hc, Wc);
    if (bb.band == 0 && oob && bad) atomicAdd(oob, bad);
}

// 16-bit counters, two per LDS word: a band is twice as many rows (2 bands instead of 4 for the 240-row sensor: every event is read by half
// as many blocks and the grid is two rounds of blocks instead of four), and the events come in aligned groups of four (one 8-byte load each
// for x and y, one 4-byte load for p, instead of twelve 1- and 2-byte loads).  A counter cannot overflow while the slice holds < 65536
// events; a block whose slice holds more (known only on the device) counts its band in two halves with 32-bit counters
// [2][ceil(rows / 2)][W], one after the other -- the same LDS, the events read twice by that block only.  Bit-exact like the other forms.
// The counting loop stands here and not in a callee shared with the 32-bit kernel: inside any inlined callee the compiler allocates it 93
// registers instead of 85 and the kernel takes 2 % longer (profiles/events_one_body_ab.txt).
__global__ __launch_bounds__(kBandThreads) void event_hist_banded16_kernel(const uint32_t* __restrict__ t, const uint16_t* __restrict__ x,
                                                                           const uint16_t* __restrict__ y, const uint8_t* __restrict__ p,
                                                                           const int64_t* __restrict__ offsets, int64_t nev, int B, int Tm, int H,
                                                                           int W, int rows, int nbands, int32_t* __restrict__ out,
                                                                           uint32_t* __restrict__ oob, float* __restrict__ canvas, int Hc, int Wc) {
    extern __shared__ int cnt[];
    __shared__ int64_t range[2];
    BandBlock bb;
    if (!band_of_block(nbands, B, Tm, rows, H, bb)) return;
    const int tid = threadIdx.x;
    band_slice_range(t, offsets, bb.b, bb.k, Tm, range);
    __syncthreads();
    const int64_t lo = range[0], hi = range[1];
    const bool packed = hi - lo < 65536;
    const int npass = packed ? 1 : 2;
    const int prow = packed ? rows : (rows + 1) / 2;          // rows per polarity plane in a pass
    const int plane = prow * W;
    unsigned bad = 0;
    for (int pass = 0; pass < npass; ++pass) {
        // (a last band shorter than prow leaves the second pass no rows: it starts at y1, where the canvas's bottom padding begins)
        const int ya = pass == 0 ? bb.y0 : (bb.y0 + prow < bb.y1 ? bb.y0 + prow : bb.y1);
        const int yb = ya + prow < bb.y1 ? ya + prow : bb.y1;
        __syncthreads();                                      // pass 1: pass 0's counters have been written out
        band_zero(cnt, packed ? (2 * plane + 1) / 2 : 2 * plane, false);
        __syncthreads();
        constexpr int UN = 4;                                 // aligned groups of four events in flight per thread
        for (int64_t i0 = (lo & ~(int64_t)3) + 4 * (int64_t)tid; i0 < hi; i0 += (int64_t)UN * 4 * kBandThreads) {
            uint2 xs[UN], ys[UN];
            unsigned ps[UN];
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                const int64_t i = i0 + (int64_t)u * 4 * kBandThreads;
                if (i < hi && i + 3 < nev) {
                    xs[u] = *reinterpret_cast<const uint2*>(x + i);
                    ys[u] = *reinterpret_cast<const uint2*>(y + i);
                    ps[u] = *reinterpret_cast<const unsigned*>(p + i);
                } else {                                      // past the slice, or the last (ragged) group of the whole stream
                    unsigned xv[4] = {0, 0, 0, 0}, yv[4] = {0, 0, 0, 0}, pv = 0;
                    for (int j = 0; j < 4; ++j)
                        if (i + j < hi) { xv[j] = x[i + j]; yv[j] = y[i + j]; pv |= (unsigned)p[i + j] << (8 * j); }
                    xs[u] = make_uint2(xv[0] | (xv[1] << 16), xv[2] | (xv[3] << 16));
                    ys[u] = make_uint2(yv[0] | (yv[1] << 16), yv[2] | (yv[3] << 16));
                    ps[u] = pv;
                }
            }
#pragma unroll
            for (int u = 0; u < UN; ++u) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int64_t e = i0 + (int64_t)u * 4 * kBandThreads + j;
                    if (e < lo || e >= hi) continue;          // the group's events outside the slice
                    band_count_one(((j < 2 ? xs[u].x : xs[u].y) >> (16 * (j & 1))) & 0xffffu, ((j < 2 ? ys[u].x : ys[u].y) >> (16 * (j & 1))) & 0xffffu,
                                   (ps[u] >> (8 * j)) & 0xffu, H, W, ya, yb, plane, packed, pass == 0, cnt, bad);
                }
            }
        }
        __syncthreads();
        const int yend = bb.band == nbands - 1 && pass == npass - 1 ? Hc : yb;
        band_write_pass<false>(cnt, packed, plane, W, ya, yb, yend, ((int64_t)bb.b * Tm + bb.k) * 2, H, out, canvas, Hc, Wc);
    }
    if (bb.band == 0 && oob && bad) atomicAdd(oob, bad);
}

__global__ __launch_bounds__(EAS_BLOCK) void counts_to_canvas_kernel(const int32_t* __restrict__ counts, int64_t F, int H,
                                                                     int W, int Hc, int Wc, float* __restrict__ out) {
    const int64_t total = F * Hc * Wc;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int xx = (int)(i % Wc);
        const int64_t r = i / Wc;
        const int yy = (int)(r % Hc);
        const int64_t f = r / Hc;
        out[i] = (xx < W && yy < H) ? (float)counts[(f * H + yy) * W + xx] : 0.0f;
    }
}

__global__ __launch_bounds__(EAS_BLOCK) void voxel_grid_kernel(const uint32_t* __restrict__ t, const uint16_t* __restrict__ x,
                                                               const uint16_t* __restrict__ y, const uint8_t* __restrict__ p,
                                                               int64_t nev, const int64_t* __restrict__ offsets, int B,
                                                               int nb, int H, int W, double* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nev; i += (int64_t)gridDim.x * blockDim.x) {
        const int b = find_sample(offsets, B, i);
        const int64_t a = offsets[b], e = offsets[b + 1];
        const double t0 = (double)t[a];
        const double span = (double)t[e - 1] - t0;
        if (span == 0.0) continue;  // single-timestamp stream: declared invalid, left zero
        const uint32_t xx = x[i], yy = y[i];
        if (xx >= (uint32_t)W || yy >= (uint32_t)H) continue;
        // same operation order as event_reps.py:53-57 in float64
        const double ts = (double)nb * ((double)t[i] - t0) / span;
        const int64_t ti = (int64_t)ts;
        const double dt = ts - (double)ti;
        const double pol = p[i] != 0 ? 1.0 : -1.0;
        double* base = out + (int64_t)b * nb * H * W + (int64_t)yy * W + xx;
        if (ti < nb) atomicAdd(base + ti * H * W, pol * (1.0 - dt));
        if (ti + 1 < nb) atomicAdd(base + (ti + 1) * H * W, pol * dt);
    }
}

// Voxel cube (to_voxel_cube_numpy, yolox/utils/event_reps.py:92-138): counts per (slice, channel, y, x) with
// slice = floor(float32(t_rel) / float32(window)) and channel = (p + 1) * (tbin + 1) - 1, tbin = floor((t_rel % window) /
// (window / tbins)) in float64 -- the reference's own arithmetic, quirks included (channel collisions for tbins >= 2).
__global__ __launch_bounds__(EAS_BLOCK) void voxel_cube_kernel(const uint32_t* __restrict__ t, const uint16_t* __restrict__ x,
                                                               const uint16_t* __restrict__ y, const uint8_t* __restrict__ p,
                                                               int64_t nev, const int64_t* __restrict__ offsets, int B, int ns,
                                                               int tbins, int H, int W, int32_t* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nev; i += (int64_t)gridDim.x * blockDim.x) {
        const int b = find_sample(offsets, B, i);
        const SampleWin w = sample_window(t, offsets, b, ns);
        const uint32_t win = w.win;
        if (win == 0) continue;
        const uint32_t tr = t[i] - w.t0;
        if ((uint64_t)tr >= (uint64_t)win * (uint64_t)ns) continue;        // tail beyond ns whole windows is dropped
        const uint32_t xx = x[i], yy = y[i];
        if (xx >= (uint32_t)W || yy >= (uint32_t)H) continue;
        const int sl = (int)floorf((float)(int32_t)tr / (float)win);
        const int tb = (int)floor((double)(tr % win) / ((double)win / (double)tbins));
        const int ch = ((int)p[i] + 1) * (tb + 1) - 1;
        if (sl >= ns || ch >= 2 * tbins) continue;                         // the reference raises on these; never for p in {0,1}
        atomicAdd(out + ((((int64_t)b * ns + sl) * (2 * tbins) + ch) * H + yy) * W + xx, 1);
    }
}

// Time surface (GEN1Dataset.agrregate 'timesurface', gen1.py:362-369 + to_timesurface_numpy, event_reps.py:141-160).
// Pass 1: latest timestamp per (sample, slice, polarity, pixel) by integer atomic max (timestamps ascend, so the
// maximum is the reference's "last write wins").  Pass 2: running maximum over the slices, then
// exp(-((i + 1) * window + t0 - latest) / tau) in float64; untouched pixels keep latest = 0 exactly like the reference.
// Both steps live in latest_surface.h; the event goes to its bin by the route of the counts (event_bin.h bin_event).
__global__ __launch_bounds__(EAS_BLOCK) void time_surface_scatter_kernel(const uint32_t* __restrict__ t, const uint16_t* __restrict__ x,
                                                                         const uint16_t* __restrict__ y, const uint8_t* __restrict__ p,
                                                                         int64_t nev, const int64_t* __restrict__ offsets, int B,
                                                                         int ns, int H, int W, uint32_t* __restrict__ latest) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nev; i += (int64_t)gridDim.x * blockDim.x) {
        const int b = find_sample(offsets, B, i);
        const uint32_t pp = p[i];
        if (pp > 1u) continue;  // to_timesurface_numpy indexes its two planes by p: a polarity byte above 1 has no plane (the count: p != 0 is channel 1)
        bin_event(t[i], x[i], y[i], pp, sample_window(t, offsets, b, ns), b, ns, H, W, latest, nullptr, LatestAccT<uint32_t>{});
    }
}

__global__ __launch_bounds__(EAS_BLOCK) void time_surface_exp_kernel(const uint32_t* __restrict__ t, const int64_t* __restrict__ offsets,
                                                                     int B, int ns, int H, int W, double tau,
                                                                     const uint32_t* __restrict__ latest, double* __restrict__ out) {
    const int64_t plane = (int64_t)2 * H * W, total = (int64_t)B * plane;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)(i / plane);
        const int64_t first = (int64_t)b * ns * plane + (i - (int64_t)b * plane);
        const SampleWin w = sample_window_of(offsets[b], offsets[b + 1], [t](int64_t j) { return t[j]; }, ns);   // (0, 0) or win == 0: zeros
        surface_walk(w.t0, w.win, ns, tau, [latest, first, plane](int k) { return latest[first + k * plane]; },
                     [out, first, plane](int k, double v) { out[first + k * plane] = v; });
    }
}

// Letterbox / jitter augmentation of count frames on the device (GEN1Dataset.get_random_data, gen1.py:433-521; NCaltech.batch_resize,
// ncaltech.py:98-105): every frame of sample b is resized to (nw, nh) with the cv2.resize semantics of ``Rule`` (LinearRule: INTER_LINEAR,
// CubicRule: INTER_CUBIC), pasted at (dx, dy) into a zero canvas, optionally mirrored left-right, and cast to fp32 (trainer.py:99).  The
// paste rule, the tap rules and the tap-weighted sum live in count_resize.h: eas_stacked_hist_frames resizes with the same ones.
// ``Src``: int32 counts, or the float64 frames of a weighted measure (eas_frames_letterbox_f64: cv2.resize sees float64 images either way).
template <typename Rule, typename Src>
__global__ __launch_bounds__(EAS_BLOCK) void counts_letterbox_kernel(const Src* __restrict__ counts, const int32_t* __restrict__ params,
                                                                     int B, int F, int H, int W, int Hc, int Wc, float* __restrict__ out) {
    const int64_t total = (int64_t)B * F * Hc * Wc;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int xx = (int)(i % Wc);
        const int64_t r = i / Wc;
        const int yy = (int)(r % Hc);
        const int64_t f = r / Hc;
        const Paste paste(params + 5 * (int)(f / F));
        const int xs = paste.src_col(xx, Wc), ys = paste.src_row(yy);
        float v = 0.f;
        if (paste.inside(xs, ys)) {
            const Src* src = counts + f * H * W;
            if (paste.identity(W, H))
                v = (float)src[ys * W + xs];
            else
                v = resample<Rule::N>([src, W](int y) { return src + y * W; }, Rule::tap(xs, W, paste.nw), Rule::tap(ys, H, paste.nh));
        }
        out[i] = v;
    }
}

// ---- host side of the band form: one plan, one launch ------------------------------------------------------------------------------
struct BandPlan {
    int rows, nbands;       // even bands of ``rows`` rows; the last one may be shorter
    size_t lds_bytes;
};

// The row bands of an H x W frame with counters of ``counter_bytes`` (4, or 2 = packed with the wide two-pass fallback); false when
// the frame does not split into at most kMaxBands bands of kBandLdsBytes.  The 16-bit capacity is rounded down to an even row count:
// the fallback counts ceil(rows / 2) rows per pass in 32-bit words, which is the packed need of rows + 1 rows when rows is odd.
bool hist_band_plan(int H, int W, int counter_bytes, BandPlan* plan) {
    int64_t cap = kBandLdsBytes / ((int64_t)2 * counter_bytes * W);
    if (counter_bytes == 2) cap &= ~(int64_t)1;
    if (cap > H) cap = H;
    if (cap < 1 || (H + cap - 1) / cap > kMaxBands) return false;
    const int nb = (int)((H + cap - 1) / cap), rows = (H + nb - 1) / nb;          // even bands
    const size_t wide = (size_t)2 * (counter_bytes == 2 ? (rows + 1) / 2 : rows) * W, packed = ((size_t)2 * rows * W + 1) / 2;
    plan->rows = rows;
    plan->nbands = (H + rows - 1) / rows;
    plan->lds_bytes = 4 * (counter_bytes == 2 && packed > wide ? packed : wide);
    return true;
}

// The form a call takes: 0 scatter, 1 band / 32-bit counters, 2 band / 16-bit counters (+ its plan).  Dense streams (>= 2048 events per
// frame on average) whose frame has a band plan take the LDS form; 16-bit counters need 8- / 4-byte loads of x, y / p (aligned16).
// EAS_HIST_FORM (development switch) forces "scatter" / "banded" / "banded32" (the 32-bit band form).
int hist_form(int64_t nev, int B, int Tm, int H, int W, bool aligned16, BandPlan* plan) {
    const char* force = getenv("EAS_HIST_FORM");
    const bool band = force ? force[0] == 'b' : nev >= (int64_t)B * Tm * 2048;
    if (!band || (int64_t)B * Tm >= (1 << 24)) return 0;
    // (a 16-bit band is at least as tall as a 32-bit one: where both apply the 16-bit form has no more bands)
    if (aligned16 && !(force && strcmp(force, "banded32") == 0) && hist_band_plan(H, W, 2, plan)) return 2;
    return hist_band_plan(H, W, 4, plan) ? 1 : 0;
}

template <auto Kernel, typename... Args>
int launch_band(const BandPlan& plan, int nslices, hipStream_t st, Args... args) {
    static bool attr_set = false;           // per kernel: one instantiation each
    if (!attr_set) {
        if (hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kBandLdsBytes) != hipSuccess) return EAS_ERR_LAUNCH;
        attr_set = true;
    }
    const int64_t groups = ((int64_t)nslices + 7) / 8;
    EAS_LAUNCH(Kernel, dim3((unsigned)(groups * 8 * plan.nbands)), dim3(kBandThreads), plan.lds_bytes, st, args...);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

// zero the counts (``out`` may be NULL: a form that writes every element itself) and the out-of-range word (may be NULL)
bool zero_counts(int32_t* out, size_t count_bytes, uint32_t* oob_count, hipStream_t st) {
    if (out && hipMemsetAsync(out, 0, count_bytes, st) != hipSuccess) return false;
    return !oob_count || hipMemsetAsync(oob_count, 0, sizeof(uint32_t), st) == hipSuccess;
}

// counts into ``out``; or, when ``canvas`` is given and a band form applies, fp32 frames straight into the canvas
// (*wrote_canvas = 1) without touching ``out``
int histogram_impl(const uint32_t* t, const uint16_t* x, const uint16_t* y, const uint8_t* p, int64_t nev,
                   const int64_t* sample_offsets, int B, int Tm, int H, int W, int32_t* out,
                   uint32_t* oob_count, float* canvas, int Hc, int Wc, int* wrote_canvas, eas_stream_t stream) {
    if (wrote_canvas) *wrote_canvas = 0;
    if (!out || !sample_offsets || B < 1 || Tm < 1 || H < 1 || W < 1 || nev < 0) return EAS_ERR_INVALID_ARG;
    if (nev > 0 && (!t || !x || !y || !p)) return EAS_ERR_INVALID_ARG;
    hipStream_t st = eas_s(stream);
    EAS_CLEAR_ERR();
    BandPlan plan;
    const bool aligned16 = ((((uintptr_t)x | (uintptr_t)y) & 7) | ((uintptr_t)p & 3)) == 0;
    const int form = hist_form(nev, B, Tm, H, W, aligned16, &plan);
    if (!zero_counts(form ? nullptr : out, (size_t)B * Tm * 2 * H * W * sizeof(int32_t), oob_count, st)) return EAS_ERR_LAUNCH;
    if (form) {
        const int rc = form == 2 ? launch_band<event_hist_banded16_kernel>(plan, B * Tm, st, t, x, y, p, sample_offsets, nev, B, Tm, H, W, plan.rows,
                                                                           plan.nbands, out, oob_count, canvas, Hc, Wc)
                                 : launch_band<event_hist_banded_kernel>(plan, B * Tm, st, t, x, y, p, sample_offsets, B, Tm, H, W, plan.rows,
                                                                         plan.nbands, out, oob_count, canvas, Hc, Wc);
        if (rc == EAS_OK && canvas && wrote_canvas) *wrote_canvas = 1;
        return rc;
    }
    if (nev == 0) return EAS_OK;
    const bool vec = (((uintptr_t)t & 15) | ((uintptr_t)x & 7) | ((uintptr_t)y & 7) | ((uintptr_t)p & 3)) == 0;
    if (vec) {
        EAS_LAUNCH(event_hist_kernel<true>, dim3(eas_grid_1d((nev + 3) / 4)), dim3(EAS_BLOCK), 0, st, t, x, y, p,
                           nev, sample_offsets, B, Tm, H, W, out, oob_count);
    } else {
        EAS_LAUNCH(event_hist_kernel<false>, dim3(eas_grid_1d(nev)), dim3(EAS_BLOCK), 0, st, t, x, y, p, nev,
                           sample_offsets, B, Tm, H, W, out, oob_count);
    }
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

// The entries for record ranges: one argument rule, the bins (and the words the walk counts and flags in) zeroed, one launch.  The ranges
// live on the device (no host read): a fixed number of blocks per sample strides over whatever it holds; the sample is a block's y index,
// hence the bound on B.  ``src_ok``: what the source's own arguments came to (raw_source / packed_source below).
static inline uint32_t* source_flags(const RawRecords&) { return nullptr; }
static inline uint32_t* source_flags(const PackedRecords& src) { return src.flags; }
static inline RawRecords without_flags(const RawRecords& src) { return src; }
static inline PackedRecords without_flags(PackedRecords src) {
    src.flags = nullptr;
    return src;
}

template <typename Acc, typename Src>
int ranges_frames(const Src& src, int src_ok, const int64_t* ranges, int B, int ns, int H, int W, typename Acc::Bin* out, uint32_t* oob_count,
                  const Acc& acc, hipStream_t st) {
    if (src_ok == EAS_ERR_INVALID_ARG || !ranges || !out || B < 1 || ns < 1 || H < 1 || W < 1) return EAS_ERR_INVALID_ARG;
    if (src_ok != EAS_OK) return src_ok;
    if (B > 65535) return EAS_ERR_UNSUPPORTED;
    EAS_CLEAR_ERR();
    if (!zero_counts((int32_t*)out, (size_t)B * ns * 2 * H * W * sizeof(typename Acc::Bin), oob_count, st)) return EAS_ERR_LAUNCH;
    if (!zero_counts(nullptr, 0, source_flags(src), st)) return EAS_ERR_LAUNCH;          // the flags are written by a call, not accumulated
    EAS_LAUNCH((dat_ranges_kernel<Acc, Src>), dim3(64, B), dim3(EAS_BLOCK), 0, st, src, ranges, ns, H, W, out, oob_count, acc);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

// the time surfaces: the walk into the output's own bins, then the finishing pass in place (it finds the windows again, without flagging
// what the walk has flagged)
template <typename Src>
int ranges_surfaces(const Src& src, int src_ok, const int64_t* ranges, int B, int num_slices, int H, int W, double tau, double* out,
                    uint32_t* oob_count, hipStream_t st) {
    if (!(tau > 0.0)) return EAS_ERR_INVALID_ARG;  // also NaN
    unsigned long long* bins = reinterpret_cast<unsigned long long*>(out);
    const int launched = ranges_frames(src, src_ok, ranges, B, num_slices, H, W, bins, oob_count, LatestAcc{}, st);
    if (launched != EAS_OK) return launched;
    EAS_LAUNCH(latest_finish_kernel<RangesWin<Src>>, dim3(eas_grid_1d((int64_t)B * 2 * H * W)), dim3(EAS_BLOCK), 0, st, (int64_t)B, num_slices, H,
               W, tau, bins, RangesWin<Src>{without_flags(src), ranges, num_slices});
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

int raw_source(const void* records, RawRecords& src) {
    src = RawRecords{(const uint2*)records};
    return !records || ((uintptr_t)records & 7) ? EAS_ERR_INVALID_ARG : EAS_OK;
}

// table [nb][2] and payload [units] of packed records (record_source.h) as a source
int packed_source(const uint32_t* table, int64_t nb, const uint8_t* payload, int64_t units, int H, int W, uint32_t* flags, PackedRecords& src) {
    RecWidths w = {1, 1, 29};
    const bool geometry = rec_widths(H, W, w);
    src = PackedRecords{(const uint2*)table, payload, nb, units, w.xb, w.yb, flags};
    if (nb < 0 || units < 0 || (nb > 0 && !table) || (units > 0 && !payload) || units > ((int64_t)1 << 31) || H < 1 || W < 1)
        return EAS_ERR_INVALID_ARG;                // (a store that holds nothing: no table, no payload, every range empty or refused)
    if (((uintptr_t)table & 7) || ((uintptr_t)payload & 15) || ((uintptr_t)flags & 3)) return EAS_ERR_INVALID_ARG;
    return geometry ? EAS_OK : EAS_ERR_UNSUPPORTED;
}

}  // namespace

extern "C" {

int eas_event_histogram(const uint32_t* t, const uint16_t* x, const uint16_t* y, const uint8_t* p, int64_t nev,
                        const int64_t* sample_offsets, int B, int Tm, int H, int W, int32_t* out,
                        uint32_t* oob_count, eas_stream_t stream) {
    return histogram_impl(t, x, y, p, nev, sample_offsets, B, Tm, H, W, out, oob_count, nullptr, 0, 0, nullptr, stream);
}

int eas_event_histogram_plan(int64_t nev, int B, int Tm, int H, int W, int aligned16, int* rows, int* nbands, int64_t* lds_bytes) {
    if (B < 1 || Tm < 1 || H < 1 || W < 1 || nev < 0) return EAS_ERR_INVALID_ARG;
    BandPlan plan = {0, 0, 0};
    const int form = hist_form(nev, B, Tm, H, W, aligned16 != 0, &plan);
    if (rows) *rows = form ? plan.rows : 0;
    if (nbands) *nbands = form ? plan.nbands : 0;
    if (lds_bytes) *lds_bytes = form ? (int64_t)plan.lds_bytes : 0;
    return form;
}

int eas_event_window_search(const void* records, const int64_t* file_offsets, int F, const int32_t* file_id, const int64_t* label_t, int B,
                            int64_t window_lo, int64_t window_hi, int num_slice, int64_t* ranges, eas_stream_t stream) {
    if (!records || !file_offsets || !label_t || !ranges || F < 1 || B < 1 || window_hi - window_lo < 1 || num_slice < 0) return EAS_ERR_INVALID_ARG;
    if ((uintptr_t)records & 7) return EAS_ERR_INVALID_ARG;
    EAS_CLEAR_ERR();
    EAS_LAUNCH(event_window_search_kernel, dim3((B + EAS_WAVE - 1) / EAS_WAVE), dim3(EAS_WAVE), 0, eas_s(stream), (const uint2*)records,
                       file_offsets, file_id, label_t, B, window_lo, window_hi, num_slice, ranges);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

int eas_event_histogram_dat_ranges(const void* records, const int64_t* ranges, int B, int Tm, int H, int W, int32_t* out, uint32_t* oob_count,
                                   eas_stream_t stream) {
    RawRecords src;
    const int ok = raw_source(records, src);
    return ranges_frames(src, ok, ranges, B, Tm, H, W, out, oob_count, CountAcc{}, eas_s(stream));
}

int eas_event_latest_surface_dat_ranges(const void* records, const int64_t* ranges, int B, int num_slices, int H, int W, double tau, double* out,
                                        uint32_t* oob_count, eas_stream_t stream) {
    RawRecords src;
    const int ok = raw_source(records, src);
    return ranges_surfaces(src, ok, ranges, B, num_slices, H, W, tau, out, oob_count, eas_s(stream));
}

int eas_event_histogram_packed_ranges(const uint32_t* table, int64_t nb, const uint8_t* payload, int64_t units, const int64_t* ranges, int B,
                                      int Tm, int H, int W, int32_t* out, uint32_t* oob_count, uint32_t* flags, eas_stream_t stream) {
    PackedRecords src;
    const int ok = packed_source(table, nb, payload, units, H, W, flags, src);
    return ranges_frames(src, ok, ranges, B, Tm, H, W, out, oob_count, CountAcc{}, eas_s(stream));
}

int eas_event_latest_surface_packed_ranges(const uint32_t* table, int64_t nb, const uint8_t* payload, int64_t units, const int64_t* ranges, int B,
                                           int num_slices, int H, int W, double tau, double* out, uint32_t* oob_count, uint32_t* flags,
                                           eas_stream_t stream) {
    PackedRecords src;
    const int ok = packed_source(table, nb, payload, units, H, W, flags, src);
    return ranges_surfaces(src, ok, ranges, B, num_slices, H, W, tau, out, oob_count, eas_s(stream));
}

int eas_counts_to_canvas(const int32_t* counts, int64_t F, int H, int W, int Hc, int Wc, float* out,
                         eas_stream_t stream) {
    if (!counts || !out || F < 0 || H < 1 || W < 1 || Hc < H || Wc < W) return EAS_ERR_INVALID_ARG;
    if (F == 0) return EAS_OK;
    EAS_CLEAR_ERR();
    EAS_LAUNCH(counts_to_canvas_kernel, dim3(eas_grid_1d(F * Hc * Wc)), dim3(EAS_BLOCK), 0, eas_s(stream), counts,
                       F, H, W, Hc, Wc, out);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

int eas_event_frames(const uint32_t* t, const uint16_t* x, const uint16_t* y, const uint8_t* p, int64_t nev,
                     const int64_t* sample_offsets, int B, int Tm, int H, int W, int Hc, int Wc, float* frames,
                     int32_t* scratch_counts, uint32_t* oob_count, eas_stream_t stream) {
    if (!frames || !scratch_counts || Hc < H || Wc < W) return EAS_ERR_INVALID_ARG;
    int wrote = 0;
    const int rc = histogram_impl(t, x, y, p, nev, sample_offsets, B, Tm, H, W, scratch_counts, oob_count, frames, Hc, Wc, &wrote, stream);
    if (rc != EAS_OK || wrote) return rc;
    return eas_counts_to_canvas(scratch_counts, (int64_t)B * Tm * 2, H, W, Hc, Wc, frames, stream);
}

int eas_event_histogram_dat(const void* records, int64_t nev, const int64_t* sample_offsets, int B, int Tm, int H, int W,
                            int32_t* out, uint32_t* oob_count, eas_stream_t stream) {
    if (!out || !sample_offsets || B < 1 || Tm < 1 || H < 1 || W < 1 || nev < 0) return EAS_ERR_INVALID_ARG;
    if (nev > 0 && (!records || ((uintptr_t)records & 7))) return EAS_ERR_INVALID_ARG;
    hipStream_t st = eas_s(stream);
    EAS_CLEAR_ERR();
    if (!zero_counts(out, (size_t)B * Tm * 2 * H * W * sizeof(int32_t), oob_count, st)) return EAS_ERR_LAUNCH;
    if (nev == 0) return EAS_OK;
    const uint2* rec = (const uint2*)records;
    if (((uintptr_t)records & 15) == 0)
        EAS_LAUNCH(event_hist_dat_kernel<true>, dim3(eas_grid_1d((nev + 1) / 2)), dim3(EAS_BLOCK), 0, st, rec, nev, sample_offsets, B,
                           Tm, H, W, out, oob_count);
    else
        EAS_LAUNCH(event_hist_dat_kernel<false>, dim3(eas_grid_1d(nev)), dim3(EAS_BLOCK), 0, st, rec, nev, sample_offsets, B, Tm, H,
                           W, out, oob_count);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

int eas_event_voxel_grid(const uint32_t* t, const uint16_t* x, const uint16_t* y, const uint8_t* p, int64_t nev,
                         const int64_t* sample_offsets, int B, int n_bins, int H, int W, double* out,
                         eas_stream_t stream) {
    if (!out || !sample_offsets || B < 1 || n_bins < 1 || H < 1 || W < 1 || nev < 0) return EAS_ERR_INVALID_ARG;
    if (nev > 0 && (!t || !x || !y || !p)) return EAS_ERR_INVALID_ARG;
    hipStream_t st = eas_s(stream);
    EAS_CLEAR_ERR();
    if (hipMemsetAsync(out, 0, (size_t)B * n_bins * H * W * sizeof(double), st) != hipSuccess) return EAS_ERR_LAUNCH;
    if (nev == 0) return EAS_OK;
    EAS_LAUNCH(voxel_grid_kernel, dim3(eas_grid_1d(nev)), dim3(EAS_BLOCK), 0, st, t, x, y, p, nev, sample_offsets,
                       B, n_bins, H, W, out);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

int eas_event_voxel_cube(const uint32_t* t, const uint16_t* x, const uint16_t* y, const uint8_t* p, int64_t nev,
                         const int64_t* sample_offsets, int B, int num_slices, int tbins, int H, int W, int32_t* out,
                         eas_stream_t stream) {
    if (!out || !sample_offsets || B < 1 || num_slices < 1 || tbins < 1 || H < 1 || W < 1 || nev < 0) return EAS_ERR_INVALID_ARG;
    if (nev > 0 && (!t || !x || !y || !p)) return EAS_ERR_INVALID_ARG;
    hipStream_t st = eas_s(stream);
    EAS_CLEAR_ERR();
    if (hipMemsetAsync(out, 0, (size_t)B * num_slices * 2 * tbins * H * W * sizeof(int32_t), st) != hipSuccess) return EAS_ERR_LAUNCH;
    if (nev == 0) return EAS_OK;
    EAS_LAUNCH(voxel_cube_kernel, dim3(eas_grid_1d(nev)), dim3(EAS_BLOCK), 0, st, t, x, y, p, nev, sample_offsets, B, num_slices,
                       tbins, H, W, out);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

int eas_event_time_surface(const uint32_t* t, const uint16_t* x, const uint16_t* y, const uint8_t* p, int64_t nev,
                           const int64_t* sample_offsets, int B, int num_slices, int H, int W, double tau, uint32_t* workspace,
                           double* out, eas_stream_t stream) {
    if (!out || !workspace || !sample_offsets || B < 1 || num_slices < 1 || H < 1 || W < 1 || nev < 0 || !(tau > 0.0)) return EAS_ERR_INVALID_ARG;
    if (nev > 0 && (!t || !x || !y || !p)) return EAS_ERR_INVALID_ARG;
    hipStream_t st = eas_s(stream);
    EAS_CLEAR_ERR();
    const int64_t total = (int64_t)B * num_slices * 2 * H * W;
    if (hipMemsetAsync(workspace, 0, (size_t)total * sizeof(uint32_t), st) != hipSuccess) return EAS_ERR_LAUNCH;
    if (nev > 0) {
        EAS_LAUNCH(time_surface_scatter_kernel, dim3(eas_grid_1d(nev)), dim3(EAS_BLOCK), 0, st, t, x, y, p, nev, sample_offsets, B,
                           num_slices, H, W, workspace);
        EAS_CHECK_LAUNCH();
    }
    EAS_LAUNCH(time_surface_exp_kernel, dim3(eas_grid_1d((int64_t)B * 2 * H * W)), dim3(EAS_BLOCK), 0, st, t, sample_offsets, B,
                       num_slices, H, W, tau, workspace, out);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

}  // extern "C"

// the letterbox of int32 counts and of float64 frames: one argument rule, one launch
template <typename Src>
static int letterbox_launch(const Src* frames, const int32_t* params, int interp, int B, int F, int H, int W, int Hc, int Wc, float* out,
                            eas_stream_t stream) {
    if (interp != 0 && interp != 1) return EAS_ERR_INVALID_ARG;
    if (!frames || !params || !out || B < 1 || F < 1 || H < 1 || W < 1 || Hc < 1 || Wc < 1) return EAS_ERR_INVALID_ARG;
    const dim3 grid(eas_grid_1d((int64_t)B * F * Hc * Wc));
    EAS_CLEAR_ERR();
    if (interp == 0)
        EAS_LAUNCH((counts_letterbox_kernel<LinearRule, Src>), grid, dim3(EAS_BLOCK), 0, eas_s(stream), frames, params, B, F, H, W, Hc, Wc, out);
    else
        EAS_LAUNCH((counts_letterbox_kernel<CubicRule, Src>), grid, dim3(EAS_BLOCK), 0, eas_s(stream), frames, params, B, F, H, W, Hc, Wc, out);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

extern "C" {

int eas_counts_letterbox_ex(const int32_t* counts, const int32_t* params, int interp, int B, int F, int H, int W, int Hc, int Wc, float* out,
                            eas_stream_t stream) {
    return letterbox_launch(counts, params, interp, B, F, H, W, Hc, Wc, out, stream);
}

int eas_frames_letterbox_f64(const double* frames, const int32_t* params, int interp, int B, int F, int H, int W, int Hc, int Wc, float* out,
                             eas_stream_t stream) {
    return letterbox_launch(frames, params, interp, B, F, H, W, Hc, Wc, out, stream);
}

int eas_counts_letterbox(const int32_t* counts, const int32_t* params, int B, int F, int H, int W, int Hc, int Wc, float* out,
                         eas_stream_t stream) {
    return eas_counts_letterbox_ex(counts, params, 0, B, F, H, W, Hc, Wc, out, stream);
}

}  // extern "C"
