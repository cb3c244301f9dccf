// An event's way to its bin, shared by the Gen1 sources (events.hip) and, for the accumulate steps, by the ATIS source (events_atis.hip): the
// window rule (SampleWin, make_window, sample_window_of), the route (bin_event<Acc>) and the accumulate steps CountAcc / LatestAcc.
#pragma once
#include "eas_common.h"
#include "latest_surface.h"

struct SampleWin {
    uint32_t t0;
    uint32_t win;  // 0 -> nothing is binned
};

// the one micro-slice window rule (gen1.py:313-328): t0 = first timestamp of the range, win = (last - first) / Tm, integer floor
__device__ __forceinline__ SampleWin make_window(uint32_t t_first, uint32_t t_last, int Tm) {
    SampleWin w;
    w.t0 = t_first;
    w.win = (t_last - t_first) / (uint32_t)Tm;
    return w;
}

// the window of the sample that is events [a, e), time(i) = timestamp of event i.  No events: window (0, 0), nothing is binned, zero frames
template <typename Time>
__device__ __forceinline__ SampleWin sample_window_of(int64_t a, int64_t e, Time time, int ns) {
    if (e <= a) return SampleWin{0u, 0u};
    return make_window(time(a), time(e - 1), ns);
}

// ---- the accumulate step: what an event of time t adds to its bin (`row`: the sample, or the ATIS macro slice b * Tl + k)
struct CountAcc {                       // measure 'count': 1
    typedef int32_t Bin;
    __device__ __forceinline__ void operator()(Bin* bin, int64_t, uint32_t) const { atomicAdd(bin, 1); }
};
template <typename BinT>
struct LatestAccT {                     // aggregation 'timesurface': the latest time of the bin (latest_surface.h), finished by a surface walk
    typedef BinT Bin;
    __device__ __forceinline__ void operator()(Bin* bin, int64_t, uint32_t t) const { latest_time_max(bin, t); }
};
typedef LatestAccT<unsigned long long> LatestAcc;       // into the output's own 64-bit bins (the record entries)

// the one route to a bin: event (tt, xx, yy) of sample b, polarity channel c in {0, 1}
template <typename Acc>
__device__ __forceinline__ void bin_event(uint32_t tt, uint32_t xx, uint32_t yy, uint32_t c, const SampleWin& w, int b, int ns, int H, int W,
                                          typename Acc::Bin* __restrict__ out, uint32_t* __restrict__ oob, const Acc& acc) {
    if (w.win == 0) return;
    const uint32_t k = (tt - w.t0) / w.win;
    if (k >= (uint32_t)ns) return;  // tail beyond t0 + ns * win is dropped (gen1.py:321-326)
    if (xx >= (uint32_t)W || yy >= (uint32_t)H) {
        if (oob) atomicAdd(oob, 1u);
        return;
    }
    acc(out + ((((int64_t)b * ns + k) * 2 + c) * H + yy) * W + xx, b, tt);
}
