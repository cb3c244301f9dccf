// The exponential time surface of the reference's aggregation 'timesurface' (to_timesurface_numpy, yolox/utils/event_reps.py:141-160), shared
// by the three entries that make it: eas_event_time_surface (decoded arrays), eas_event_latest_surface_dat_ranges (.dat record ranges) and
// eas_event_latest_surface_atis (raw ATIS records).  Two steps.
//   latest_time_max   an event of time t in micro slice k: integer atomic max of t into the bin of its (slice, polarity, pixel).  Times
//                     ascend inside a slice, so the maximum is the reference's "last write wins"; any order of the atomics gives the same bits.
//   surface_walk      one thread per (sample or macro slice, polarity, pixel): the running maximum m of the bins of micro slices 0 .. ns - 1
//                     (the reference does not clear its memory between micro slices), and per slice
//                     exp(-((k + 1) * win + t0 - m) / tau) in float64; an untouched pixel keeps m = 0 exactly like the reference.
// The two record entries keep the latest times in the OUTPUT's own 64-bit bins (zeroed by the call) and the walk overwrites every bin, after it
// has read it, with the double it becomes: no workspace the size of the frames, and a bin is read and written by the same thread only.  Their
// finishing pass is latest_finish_kernel<RowWin> (below).
#pragma once
#include "eas_common.h"

template <typename Bin>
__device__ __forceinline__ void latest_time_max(Bin* bin, uint32_t t) {
    atomicMax(bin, (Bin)t);
}

// the ns surfaces of one pixel.  t0 / win: time of the first event of micro slice 0 and the micro window (0: no events, or a window of zero
// length -- zeros); latest(k) -> the bin of micro slice k, put(k, v) stores its surface (put(k) may overwrite what latest(k) read).
// (k + 1) * win + t0 in uint32 arithmetic as numpy's on Gen1's uint32 times; the ATIS times fit 32 bits with their ends, so there the
// reference's int64 arithmetic gives the same number.
template <typename Latest, typename Put>
__device__ __forceinline__ void surface_walk(uint32_t t0, uint32_t win, int ns, double tau, Latest latest, Put put) {
    uint32_t m = 0;
    for (int k = 0; k < ns; ++k) {
        if (win == 0) {
            put(k, 0.0);
            continue;
        }
        const uint32_t l = latest(k);
        m = l > m ? l : m;
        const uint32_t end = (uint32_t)(k + 1) * win + t0;
        const int64_t diff = -((int64_t)end - (int64_t)m);
        put(k, exp((double)diff / tau));
    }
}

// the walk in place over 64-bit bins `stride` apart (the plane stride 2 * H * W of frames [..][ns][2][H][W])
__device__ __forceinline__ void surface_walk_in_place(unsigned long long* bins, int64_t stride, uint32_t t0, uint32_t win, int ns, double tau) {
    surface_walk(t0, win, ns, tau, [bins, stride](int k) { return (uint32_t)bins[k * stride]; },
                 [bins, stride](int k, double v) { bins[k * stride] = __builtin_bit_cast(unsigned long long, v); });
}

// The finishing pass of the record entries, in place over bins [rows][ns][2][H][W]: one thread per (row, polarity, pixel), adjacent lanes on
// adjacent pixels, the ns micro slices 2 * H * W bins apart.  ``win(row, t0, w)`` gives a row's first time and micro window: RangesWin<Src>
// (events.hip; row = sample: its range's two record times, from the 8-byte or the packed records, window 0 when empty) or AtisSliceWin (events_atis.hip; row = the plan's AtisSlice).
template <typename RowWin>
__global__ __launch_bounds__(EAS_BLOCK) void latest_finish_kernel(int64_t nrows, int ns, int H, int W, double tau, unsigned long long* __restrict__ bins,
                                                                  const RowWin win) {
    const int64_t plane = (int64_t)2 * H * W, total = nrows * plane;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int row = (int)(i / plane);          // (the entries bound their rows far below 2^31)
        uint32_t t0, w;
        win(row, t0, w);
        surface_walk_in_place(bins + (int64_t)row * ns * plane + (i - (int64_t)row * plane), plane, t0, w, ns, tau);
    }
}
