// RVT "stacked histogram" representations -> per-polarity event counts on the model canvas: three kernels over shared pieces (SliceRule:
// which representation feeds a slice; bin_sums16: the bin sum of 16 pixels; the paste and resize rule of count_resize.h; the row sources
// BinPlanes / SumPlanes / PackedPlanes: what the band kernel stages, from the representations as they are, from their bin sums or from the
// bin sums in packed rows), and the three kernels that measure, pack and unpack such rows.
//
// eas_stacked_hist_event_sum, the config-4 input: replaces RVTGEN4Dataset.generate_slices(..., method='event_sum') + the zero padding of the
// validation letterbox (yolox/data/datasets/rvt_gen4.py:109-125 and :516-533 with scale 1).
//   hist  u8  [B][Tm][2*nbins][H][W]   channel = polarity * nbins + bin  (the reference's reshape(n, 2, -1, H, W))
//   out   f32 [B][Tm][2][Hc][Wc]       out[b][j][p] = sum over bins of hist[b][i][p*nbins + bin], zero outside H x W
// A sample whose sequence is younger than Tm representations supplies only its first n_valid[b] slices; they are the
// LAST n_valid[b] output slices (j = Tm - n_valid[b] + i), the leading ones are zero (rvt_gen4.py:122-123).
//
// HBM-bound integer work: per output element nbins bytes read + 4 bytes written (14 B at nbins = 10).  Sums <= 255 * nbins are exact in fp32.
#include "eas_common.h"
#include "count_resize.h"

namespace {

// ---- shared pieces -------------------------------------------------------------------------------------------------------------------
// Which representation of the store [R] feeds output slice j of sample b: f0 + j, where it lies in [low, R); a zero slice otherwise.
//   store addressing: f0 = first[b], low = lo[b] (NULL: 0) -- any int64 may come in: f0 is clamped to [-Tm, R] before j is added, low to >= 0
//   batch addressing (first == NULL): the store is a batch [B][Tm] whose sample b supplies its first n_valid[b] (NULL: Tm; clamped to
//   [0, Tm]) slices as the last output slices: f0 = b * Tm - (Tm - n_valid[b]), low = b * Tm, R = B * Tm
struct SliceRule {
    int64_t f0, low, R;

    __device__ __forceinline__ SliceRule(int64_t R_, const int64_t* __restrict__ first, const int64_t* __restrict__ lo,
                                         const int32_t* __restrict__ n_valid, int b, int Tm) : R(R_) {
        if (first) {
            f0 = first[b];
            f0 = f0 > R ? R : (f0 < -(int64_t)Tm ? -(int64_t)Tm : f0);
            low = lo ? lo[b] : 0;
            low = low < 0 ? 0 : low;
        } else {
            int nv = n_valid ? n_valid[b] : Tm;
            nv = nv < 0 ? 0 : (nv > Tm ? Tm : nv);
            low = (int64_t)b * Tm;
            f0 = low - (Tm - nv);
        }
    }
    __device__ __forceinline__ int64_t index(int j) const { return f0 + j; }
    __device__ __forceinline__ bool have(int j) const { return f0 + j >= low && f0 + j < R; }
    // the sample's flag word: bit 0 = one of its Tm slices lies at or behind the end of the store
    __device__ __forceinline__ uint32_t flag(int Tm) const {
        uint32_t fl = 0;
        for (int k = 0; k < Tm; ++k) fl |= (f0 + k >= low && f0 + k >= R) ? 1u : 0u;
        return fl;
    }
};

// the 16 bytes of one bin's pixels onto the sums: even and odd bytes of a word go to accumulators of two 16-bit lanes each, two bytes per
// operation (ev[q]: pixels 4q, 4q + 2; od[q]: pixels 4q + 1, 4q + 3)
__device__ __forceinline__ void add_bytes16(const uint4& v, uint32_t (&ev)[4], uint32_t (&od)[4]) {
    const uint32_t wds[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        ev[q] += wds[q] & 0x00ff00ffu;
        od[q] += (wds[q] >> 8) & 0x00ff00ffu;
    }
}

// 16 bin sums (pixels x0 .. x0 + 15 of one source row) as eight words of two 16-bit sums, pixel order.  NB > 0: the bin count at compile
// time, all its loads issued before the first add (NB = 10 is the measured form)
template <int NB>
__device__ __forceinline__ void bin_sums16(const uint8_t* __restrict__ src, int64_t plane, int nbins, bool vec, int n_left, uint32_t (&sum)[8]) {
    uint32_t ev[4] = {0, 0, 0, 0}, od[4] = {0, 0, 0, 0};
    if (vec && NB > 0) {
        uint4 v[NB > 0 ? NB : 1];
#pragma unroll
        for (int k = 0; k < NB; ++k) v[k] = *reinterpret_cast<const uint4*>(src + (int64_t)k * plane);
#pragma unroll
        for (int k = 0; k < NB; ++k) add_bytes16(v[k], ev, od);
    } else if (vec) {
        for (int k = 0; k < nbins; ++k) add_bytes16(*reinterpret_cast<const uint4*>(src + (int64_t)k * plane), ev, od);
    } else {                                  // rows that are not 16-byte aligned, ragged row end: n_left < 16 pixels exist
        for (int k = 0; k < nbins; ++k) {
            const uint8_t* row = src + (int64_t)k * plane;
            uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (e < n_left) w[e >> 2] |= (uint32_t)row[e] << (8 * (e & 3));
            add_bytes16(make_uint4(w[0], w[1], w[2], w[3]), ev, od);
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        sum[2 * q] = (ev[q] & 0xffffu) | (od[q] << 16);
        sum[2 * q + 1] = (ev[q] >> 16) | (od[q] & 0xffff0000u);
    }
}

// eas_stacked_hist_event_sum: one thread owns 16 consecutive pixels of one (b, j, p, canvas row) -- their bin sums, four float4 stores; the
// batch is a store of B * Tm representations in SliceRule's batch addressing
template <int NB>
__global__ __launch_bounds__(EAS_BLOCK) void stacked_hist_sum_kernel(const uint8_t* __restrict__ hist, const int32_t* __restrict__ n_valid, int B,
                                                                     int Tm, int nbins_rt, int H, int W, int Hc, int Wc,
                                                                     float* __restrict__ out, int64_t total_groups) {
    const int nbins = NB > 0 ? NB : nbins_rt;
    const int wg = Wc / 16;                              // 16-pixel groups per output row
    const int64_t plane = (int64_t)H * W;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total_groups; g += (int64_t)gridDim.x * blockDim.x) {
        const int xg = (int)(g % wg);
        int64_t r = g / wg;
        const int y = (int)(r % Hc);
        r /= Hc;
        const int p = (int)(r & 1);
        r >>= 1;
        const int j = (int)(r % Tm);
        const int b = (int)(r / Tm);
        const int x0 = xg * 16;
        float4* dst = reinterpret_cast<float4*>(out + ((((int64_t)b * Tm + j) * 2 + p) * Hc + y) * (int64_t)Wc + x0);
        const SliceRule slice((int64_t)B * Tm, nullptr, nullptr, n_valid, b, Tm);
        if (!slice.have(j) || y >= H || x0 >= W) {
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            dst[0] = z; dst[1] = z; dst[2] = z; dst[3] = z;
            continue;
        }
        uint32_t sum[8];
        bin_sums16<NB>(hist + ((slice.index(j) * 2 + p) * nbins) * plane + (int64_t)y * W + x0, plane, nbins, x0 + 16 <= W && (W & 15) == 0, W - x0, sum);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            dst[q] = make_float4((float)(sum[2 * q] & 0xffffu), (float)(sum[2 * q] >> 16), (float)(sum[2 * q + 1] & 0xffffu), (float)(sum[2 * q + 1] >> 16));
    }
}

// eas_stacked_hist_bin_sums, the builder of the summed store: one thread owns 16 consecutive pixels of one (representation, polarity, row)
// -- nbins 16-byte loads, two 16-byte stores; bytes and 16-bit elements one by one where rows are not 16-byte aligned (W % 16 != 0)
template <int NB>
__global__ __launch_bounds__(EAS_BLOCK) void stacked_hist_bin_sums_kernel(const uint8_t* __restrict__ hist, int nbins_rt, int H, int W,
                                                                          uint16_t* __restrict__ sums, int64_t total_groups) {
    const int nbins = NB > 0 ? NB : nbins_rt;
    const int wg = (W + 15) / 16;                        // 16-pixel groups per row, the last one ragged
    const int64_t plane = (int64_t)H * W;
    const bool vec = (W & 15) == 0;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total_groups; g += (int64_t)gridDim.x * blockDim.x) {
        const int x0 = (int)(g % wg) * 16;
        int64_t r = g / wg;
        const int y = (int)(r % H);
        r /= H;                                          // representation * 2 + polarity
        uint32_t sum[8];
        bin_sums16<NB>(hist + r * nbins * plane + (int64_t)y * W + x0, plane, nbins, vec, W - x0, sum);
        uint16_t* d = sums + r * plane + (int64_t)y * W + x0;
        if (vec) {
            reinterpret_cast<uint4*>(d)[0] = make_uint4(sum[0], sum[1], sum[2], sum[3]);
            reinterpret_cast<uint4*>(d)[1] = make_uint4(sum[4], sum[5], sum[6], sum[7]);
        } else {
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (e < W - x0) d[e] = (uint16_t)(sum[e >> 1] >> (16 * (e & 1)));
        }
    }
}

// ---- row sources of the band kernel ----------------------------------------------------------------------------------------------------
// A source is one polarity of one representation; sums16 hands out the bin sums of pixels x0 .. x0 + 15 of one of its rows as eight words
// of two 16-bit sums, pixel order (pixels at and behind W: zero).
// the representations as they are, u8 [R][2 * nbins][H][W]: nbins byte-plane loads and adds
template <int NB>
struct BinPlanes {
    using handle = const uint8_t* __restrict__;
    static constexpr int kMaxW = 65536;                                       // a tap is 16 bits
    static bool valid(const uint8_t* store) { return store && !((uintptr_t)store & 15); }
    const uint8_t* src0;
    int64_t plane;
    int nbins, W;
    bool aligned;
    __device__ __forceinline__ BinPlanes(const uint8_t* __restrict__ store, int64_t rep, int p, int nbins_rt, int H, int W_)
        : plane((int64_t)H * W_), nbins(NB > 0 ? NB : nbins_rt), W(W_), aligned((W_ & 15) == 0) {
        src0 = store + ((rep * 2 + p) * nbins) * plane;
    }
    __device__ __forceinline__ void sums16(int row, int x0, uint32_t (&sum)[8]) const {
        bin_sums16<NB>(src0 + (int64_t)row * W + x0, plane, nbins, aligned, W - x0, sum);
    }
};
// their bin sums, u16 [R][2][H][W] (eas_stacked_hist_bin_sums): a copy of 16-bit rows, 16-byte loads where rows are 16-byte aligned
// (W % 8 == 0: a row then ends on a 16-byte boundary, so a group holds 8 or 16 pixels), element by element otherwise
struct SumPlanes {
    using handle = const uint16_t* __restrict__;
    static constexpr int kMaxW = 65536;
    static bool valid(const uint16_t* store) { return store && !((uintptr_t)store & 15); }
    const uint16_t* src0;
    int W;
    bool aligned;
    __device__ __forceinline__ SumPlanes(const uint16_t* __restrict__ store, int64_t rep, int p, int, int H, int W_) : W(W_), aligned((W_ & 7) == 0) {
        src0 = store + (rep * 2 + p) * ((int64_t)H * W_);
    }
    __device__ __forceinline__ void sums16(int row, int x0, uint32_t (&sum)[8]) const {
        const uint16_t* src = src0 + (int64_t)row * W + x0;
        const int n_left = W - x0;
        if (aligned) {
            const uint4 a = reinterpret_cast<const uint4*>(src)[0];
            const uint4 b = n_left >= 16 ? reinterpret_cast<const uint4*>(src)[1] : make_uint4(0u, 0u, 0u, 0u);
            sum[0] = a.x; sum[1] = a.y; sum[2] = a.z; sum[3] = a.w;
            sum[4] = b.x; sum[5] = b.y; sum[6] = b.z; sum[7] = b.w;
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) sum[q] = 0;
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (e < n_left) sum[e >> 1] |= (uint32_t)src[e] << (16 * (e & 1));
        }
    }
};

// ---- packed rows ---------------------------------------------------------------------------------------------------------------------------
// The bin sums of one source row (one polarity of one representation), cut into G = ceil(W / 16) <= 64 groups of 16 pixels (pixels at and
// behind W: zero).  A group is zero (nothing stored), narrow (every sum <= 255: 16 bytes, pixel order) or wide (sixteen u16: the eight
// words of sums16).  Row table int64 [rows][3] = (nz, wide, offset): bit g of nz / wide = group g is not zero / is wide, offset = the row's
// first 16-byte unit in the payload; group g starts at unit offset + popcount(nz & below(g)) + popcount(wide & below(g)).
__device__ __forceinline__ uint4 narrow_bytes(const uint32_t (&sum)[8]) {
    uint32_t w[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
        w[q] = (sum[2 * q] & 0xffu) | ((sum[2 * q] >> 8) & 0xff00u) | ((sum[2 * q + 1] & 0xffu) << 16) | ((sum[2 * q + 1] & 0xff0000u) << 8);
    return make_uint4(w[0], w[1], w[2], w[3]);
}
__device__ __forceinline__ void widen_bytes(const uint4& v, uint32_t (&sum)[8]) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        sum[2 * q] = (w[q] & 0xffu) | ((w[q] & 0xff00u) << 8);
        sum[2 * q + 1] = ((w[q] >> 16) & 0xffu) | ((w[q] >> 8) & 0xff0000u);
    }
}
// units of the payload in front of group g of a row, counted from the row's offset
__device__ __forceinline__ uint64_t units_below(uint64_t nz, uint64_t wide, int g) {
    const uint64_t below = ((uint64_t)1 << g) - 1;
    return (uint64_t)(__popcll(nz & below) + __popcll(wide & below));
}

// a store of packed rows as the kernels take it, by value: the row table, the payload and its length in units.  The table is device data
// nobody has validated: a group whose units do not lie inside [0, units) is never read and comes out as zeros.
struct PackedRows {
    const int64_t* rows;
    const uint4* payload;
    int64_t units;
};
// group g (0 <= g < 64) of the row whose three words stand at ``words``, as the eight words of sums16
__device__ __forceinline__ void packed_group16(const int64_t* __restrict__ words, const uint4* __restrict__ payload, uint64_t units, int g,
                                               uint32_t (&sum)[8]) {
#pragma unroll
    for (int q = 0; q < 8; ++q) sum[q] = 0;
    const uint64_t nz = (uint64_t)words[0];
    if (!((nz >> g) & 1)) return;                                               // a zero group: the payload is not touched
    const uint64_t wide = (uint64_t)words[1], unit = (uint64_t)words[2] + units_below(nz, wide, g);
    const bool is_wide = (wide >> g) & 1;
    if (unit >= units || units - unit < (is_wide ? 2u : 1u)) return;
    const uint4 a = payload[unit];
    if (is_wide) {
        const uint4 b = payload[unit + 1];
        sum[0] = a.x; sum[1] = a.y; sum[2] = a.z; sum[3] = a.w;
        sum[4] = b.x; sum[5] = b.y; sum[6] = b.z; sum[7] = b.w;
    } else {
        widen_bytes(a, sum);
    }
}
// the packed rows of the summed store, table int64 [R][2][H][3] (eas_count_rows_pack): per group the row's three words, then nothing, 16 or
// 32 bytes of payload
struct PackedPlanes {
    using handle = PackedRows;
    static constexpr int kMaxW = 1024;                                        // 64 groups: one bit each in nz and wide
    static bool valid(const PackedRows& s) {
        return s.rows && !((uintptr_t)s.rows & 7) && s.units >= 0 && (s.payload || s.units == 0) && !((uintptr_t)s.payload & 15);
    }
    const int64_t* rows0;
    const uint4* payload;
    uint64_t units;
    __device__ __forceinline__ PackedPlanes(const PackedRows& store, int64_t rep, int p, int, int H, int)
        : rows0(store.rows + (rep * 2 + p) * ((int64_t)H * 3)), payload(store.payload), units((uint64_t)store.units) {}
    __device__ __forceinline__ void sums16(int row, int x0, uint32_t (&sum)[8]) const {
        packed_group16(rows0 + (int64_t)row * 3, payload, units, x0 >> 4, sum);
    }
};

// The three row kernels: one wave per row, lane g takes group g (G <= 64).  ``row`` runs over [n][2][H] of a chunk of u16 sums.
constexpr int kRowsPerBlock = EAS_BLOCK / 64;

// lane g's group of row ``row`` of the u16 sums [n][2][H][W], through SumPlanes
__device__ __forceinline__ void sums_group16(const uint16_t* __restrict__ sums, int64_t row, int H, int W, int g, uint32_t (&sum)[8]) {
    const int64_t plane = row / H;
    const SumPlanes src(sums, plane >> 1, (int)(plane & 1), 0, H, W);
    src.sums16((int)(row - plane * H), g * 16, sum);
}

// eas_count_rows_measure: two ballots give the row's masks; lane 0 writes (nz, wide, units of the row)
__global__ __launch_bounds__(EAS_BLOCK) void count_rows_measure_kernel(const uint16_t* __restrict__ sums, int64_t n_rows, int H, int W,
                                                                       int64_t* __restrict__ table) {
    const int lane = threadIdx.x & 63, G = (W + 15) >> 4;
    const int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (row >= n_rows) return;                                                  // (the whole wave)
    uint32_t any = 0, high = 0;
    if (lane < G) {
        uint32_t sum[8];
        sums_group16(sums, row, H, W, lane, sum);
#pragma unroll
        for (int q = 0; q < 8; ++q) { any |= sum[q]; high |= sum[q] & 0xff00ff00u; }
    }
    const uint64_t nz = __ballot(any != 0), wide = __ballot(high != 0);
    if (lane == 0) {
        table[row * 3] = (int64_t)nz;
        table[row * 3 + 1] = (int64_t)wide;
        table[row * 3 + 2] = __popcll(nz) + __popcll(wide);
    }
}

// eas_count_rows_pack: the table is trusted for the class and the place of every group; nothing outside units [unit_lo, unit_hi) is written
__global__ __launch_bounds__(EAS_BLOCK) void count_rows_pack_kernel(const uint16_t* __restrict__ sums, int64_t n_rows, int H, int W,
                                                                    const int64_t* __restrict__ table, uint4* __restrict__ payload, uint64_t unit_lo,
                                                                    uint64_t unit_hi) {
    const int lane = threadIdx.x & 63, G = (W + 15) >> 4;
    const int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (row >= n_rows || lane >= G) return;
    const uint64_t nz = (uint64_t)table[row * 3], wide = (uint64_t)table[row * 3 + 1];
    if (!((nz >> lane) & 1)) return;
    const uint64_t unit = (uint64_t)table[row * 3 + 2] + units_below(nz, wide, lane);
    const bool is_wide = (wide >> lane) & 1;
    if (unit < unit_lo || unit >= unit_hi || unit_hi - unit < (is_wide ? 2u : 1u)) return;
    uint32_t sum[8];
    sums_group16(sums, row, H, W, lane, sum);
    if (is_wide) {
        payload[unit] = make_uint4(sum[0], sum[1], sum[2], sum[3]);
        payload[unit + 1] = make_uint4(sum[4], sum[5], sum[6], sum[7]);
    } else {
        payload[unit] = narrow_bytes(sum);
    }
}

// eas_count_rows_unpack: the inverse -- 16-byte stores where rows are 16-byte aligned (W % 8 == 0), elements otherwise
__global__ __launch_bounds__(EAS_BLOCK) void count_rows_unpack_kernel(PackedRows store, int64_t n_rows, int W, uint16_t* __restrict__ sums) {
    const int lane = threadIdx.x & 63, G = (W + 15) >> 4;
    const int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (row >= n_rows || lane >= G) return;
    uint32_t sum[8];
    packed_group16(store.rows + row * 3, store.payload, (uint64_t)store.units, lane, sum);
    const int x0 = lane * 16, n_left = W - x0;
    uint16_t* d = sums + row * W + x0;
    if ((W & 7) == 0) {
        reinterpret_cast<uint4*>(d)[0] = make_uint4(sum[0], sum[1], sum[2], sum[3]);
        if (n_left >= 16) reinterpret_cast<uint4*>(d)[1] = make_uint4(sum[4], sum[5], sum[6], sum[7]);
    } else {
#pragma unroll
        for (int e = 0; e < 16; ++e)
            if (e < n_left) d[e] = (uint16_t)(sum[e >> 1] >> (16 * (e & 1)));
    }
}

// ---- training input: indices into a resident store -> augmented frames (eas_stacked_hist_frames) --------------------------------------
// RVTGEN4Dataset.__getitem__ for a training sample (rvt_gen4.py:190-235): the last Tm representations up to the label's
// (generate_slices, :109-125, zero slices in front of a young sequence), the bin sum, then get_random_data's resize / paste / flip with cv2.INTER_LINEAR (:510-598) -- the arithmetic of
// counts_letterbox_kernel<LinearRule> (events.hip) on the integer bin sums, without the int32 frames in between.
//
// One block takes a band of output rows of one (sample, slice, polarity).  The vertical taps of the band name at most 2 * rows source
// rows; only those are read: their bin sums (<= 255 * nbins <= 65025: 16 bits) are staged in LDS, 16 pixels per lane and step with nbins
// 16-byte loads issued up front (64 lanes x 16 B = 1 KiB contiguous per plane row; bytes one by one when rows are not 16-byte aligned), then
// every output pixel is a gather from LDS with the horizontal taps of the band (one table per block) and the stores are float4.  Zero
// slices and bands outside the paste rectangle are stores only.  Everything read from device memory is clamped: a slice index by
// SliceRule, the paste row by Paste (count_resize.h), and a source row or column index comes out of linear_tap, which clamps to the sensor.
// The staging step reads through a row source (above): BinPlanes for eas_stacked_hist_frames, SumPlanes -- the same rows already summed,
// 2 bytes per pixel in place of nbins -- for eas_count_store_frames, PackedPlanes -- those rows packed -- for eas_packed_store_frames;
// everything else is one body.  The source's handle (a pointer, or PackedRows) comes in by value.
constexpr int kFrameBandRows = 8;             // output rows per block at most (fewer on wide sensors: frames_band_rows)
constexpr int kFrameLdsBytes = 48 * 1024;     // staged rows + tap tables

struct XTap { uint32_t s01; float w1; };      // s0 | s1 << 16; w1 < 0: outside the paste rectangle

template <typename Src>
__global__ __launch_bounds__(EAS_BLOCK) void stacked_hist_frames_kernel(typename Src::handle store, int64_t R,
                                                                        const int64_t* __restrict__ first, const int64_t* __restrict__ lo,
                                                                        const int32_t* __restrict__ params, int Tm, int nbins_rt, int H, int W,
                                                                        int Hc, int Wc, int band_rows, int nbands, float* __restrict__ out,
                                                                        uint32_t* __restrict__ flags) {
    extern __shared__ __attribute__((aligned(16))) unsigned char frames_lds[];
    __shared__ int y_s0[kFrameBandRows], y_s1[kFrameBandRows], y_slot0[kFrameBandRows], y_slot1[kFrameBandRows];
    __shared__ float y_w1[kFrameBandRows];
    __shared__ int slot_row[2 * kFrameBandRows];
    __shared__ int n_slots;
    const int wp = (W + 15) & ~15;                        // staged row pitch in pixels
    uint16_t* stage = reinterpret_cast<uint16_t*>(frames_lds);                                             // [2 * band_rows][wp]
    XTap* xtab = reinterpret_cast<XTap*>(frames_lds + (size_t)2 * band_rows * wp * sizeof(uint16_t));      // [Wc]
    const int tid = threadIdx.x;
    int r = blockIdx.x;
    const int band = r % nbands;
    r /= nbands;
    const int p = r & 1;
    r >>= 1;
    const int j = r % Tm;
    const int b = r / Tm;
    const int y0 = band * band_rows, rows = min(band_rows, Hc - y0);

    const SliceRule slice(R, first, lo, nullptr, b, Tm);
    if (flags && band == 0 && p == 0 && j == 0 && tid == 0) flags[b] = slice.flag(Tm);
    const Paste paste = params ? Paste(params + 5 * (int64_t)b) : Paste(W, H);
    const bool identity = paste.identity(W, H);
    float4* dst = reinterpret_cast<float4*>(out + ((((int64_t)b * Tm + j) * 2 + p) * Hc + y0) * (int64_t)Wc);
    const int wc4 = Wc / 4;

    // a zero slice, or a band that does not meet the paste rectangle at all (block-uniform)
    if (!slice.have(j) || !paste.touches(y0, rows, Wc)) {
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int i = tid; i < rows * wc4; i += EAS_BLOCK) dst[i] = z;
        return;
    }
    // taps of the band's rows and of every canvas column; a copy is the tap (s, s) with weights (1, 0)
    if (tid < rows) {
        const int ys = paste.src_row(y0 + tid);
        Taps<2> t = {{0, 0}, {0.f, -1.f}};
        if (paste.has_row(ys)) t = identity ? Taps<2>{{ys, ys}, {1.f, 0.f}} : linear_tap(ys, H, paste.nh);
        y_s0[tid] = t.s[0]; y_s1[tid] = t.s[1]; y_w1[tid] = t.c[1];
    }
    for (int xx = tid; xx < Wc; xx += EAS_BLOCK) {
        const int xs = paste.src_col(xx, Wc);
        Taps<2> t = {{0, 0}, {0.f, -1.f}};
        if (paste.has_col(xs)) t = identity ? Taps<2>{{xs, xs}, {1.f, 0.f}} : linear_tap(xs, W, paste.nw);
        xtab[xx] = XTap{(uint32_t)t.s[0] | ((uint32_t)t.s[1] << 16), t.c[1]};
    }
    __syncthreads();
    if (tid == 0) {                                       // the distinct source rows the band names -> staging slots (at most 2 * rows)
        int n = 0;
        for (int q = 0; q < rows; ++q) {
            if (y_w1[q] < 0.f) continue;
            for (int h = 0; h < 2; ++h) {
                const int s = h ? y_s1[q] : y_s0[q];
                int slot = -1;
                for (int k = 0; k < n; ++k) slot = slot_row[k] == s ? k : slot;
                if (slot < 0) { slot_row[n] = s; slot = n++; }
                if (h) y_slot1[q] = slot; else y_slot0[q] = slot;
            }
        }
        n_slots = n;
    }
    __syncthreads();

    // stage the bin sums of the named rows
    const int wg = wp / 16, n_groups = n_slots * wg;
    const Src src(store, slice.index(j), p, nbins_rt, H, W);
    for (int g = tid; g < n_groups; g += EAS_BLOCK) {
        const int slot = g / wg, x0 = (g - slot * wg) * 16;
        uint32_t sum[8];
        src.sums16(slot_row[slot], x0, sum);
        uint4* d = reinterpret_cast<uint4*>(stage + (size_t)slot * wp + x0);
        d[0] = make_uint4(sum[0], sum[1], sum[2], sum[3]);
        d[1] = make_uint4(sum[4], sum[5], sum[6], sum[7]);
    }
    __syncthreads();

    // gather: four canvas pixels per lane and step
    for (int i = tid; i < rows * wc4; i += EAS_BLOCK) {
        const int q = i / wc4, x4 = (i - q * wc4) * 4;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        const float wy1 = y_w1[q];
        if (wy1 >= 0.f) {
            const Taps<2> ty = {{y_slot0[q], y_slot1[q]}, {1.f - wy1, wy1}};          // rows as staging slots
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const XTap t = xtab[x4 + e];
                if (t.w1 < 0.f) continue;
                const Taps<2> tx = {{(int)(t.s01 & 0xffffu), (int)(t.s01 >> 16)}, {1.f - t.w1, t.w1}};
                if (identity)
                    v[e] = (float)(int)stage[(size_t)ty.s[0] * wp + tx.s[0]];
                else
                    v[e] = resample<2>([stage, wp](int y) { return stage + (size_t)y * wp; }, tx, ty);
            }
        }
        dst[i] = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// output rows per block: kFrameBandRows, fewer where 2 * rows staged rows of the sensor's width and the column table would not fit; 0: none does
int frames_band_rows(int W, int Wc) {
    const int64_t wp = ((int64_t)W + 15) & ~(int64_t)15, table = (int64_t)Wc * sizeof(XTap);
    int rows = kFrameBandRows;
    while (rows > 0 && 2 * rows * wp * (int64_t)sizeof(uint16_t) + table > kFrameLdsBytes) rows >>= 1;
    return rows;
}

// the three frame entries: the argument checks, the band plan and the launch of the band kernel on the entry's row source
template <typename Src>
int frames_call(typename Src::handle store, int64_t R, const int64_t* first, const int64_t* lo, const int32_t* params, int B, int Tm, int nbins,
                int H, int W, int Hc, int Wc, float* out, uint32_t* flags, eas_stream_t stream) {
    if (!Src::valid(store) || !first || !out || R < 1 || B < 1 || Tm < 1 || nbins < 1 || H < 1 || W < 1 || Hc < 1 || Wc < 1) return EAS_ERR_INVALID_ARG;
    if (((uintptr_t)out & 15) || (((uintptr_t)first | (uintptr_t)lo) & 7) || (((uintptr_t)params | (uintptr_t)flags) & 3))
        return EAS_ERR_INVALID_ARG;
    if (Wc % 16 != 0 || nbins > 255 || W > Src::kMaxW) return EAS_ERR_UNSUPPORTED;      // model canvases are multiples of 32; taps are 16 bits
    const int band_rows = frames_band_rows(W, Wc);
    if (band_rows < 1) return EAS_ERR_UNSUPPORTED;
    const int nbands = (Hc + band_rows - 1) / band_rows;
    const int64_t blocks = (int64_t)B * Tm * 2 * nbands;
    if (blocks > INT32_MAX) return EAS_ERR_UNSUPPORTED;
    const size_t lds = (size_t)2 * band_rows * ((W + 15) & ~15) * sizeof(uint16_t) + (size_t)Wc * sizeof(XTap);
    hipStream_t st = eas_s(stream);
    EAS_CLEAR_ERR();
    EAS_LAUNCH((stacked_hist_frames_kernel<Src>), dim3((unsigned)blocks), dim3(EAS_BLOCK), lds, st, store, R, first, lo, params, Tm, nbins, H, W, Hc,
               Wc, band_rows, nbands, out, flags);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

}  // namespace

extern "C" int eas_stacked_hist_event_sum(const uint8_t* hist, const int32_t* n_valid, int B, int Tm, int nbins, int H, int W, int Hc,
                                          int Wc, float* out, eas_stream_t stream) {
    if (!hist || !out || B < 0 || Tm < 1 || nbins < 1 || H < 1 || W < 1 || Hc < H || Wc < W) return EAS_ERR_INVALID_ARG;
    if (Wc % 16 != 0 || nbins > 255) return EAS_ERR_UNSUPPORTED;      // model canvases are multiples of 32; a bin sum is 16 bits
    if ((((uintptr_t)hist | (uintptr_t)out) & 15) || ((uintptr_t)n_valid & 3)) return EAS_ERR_INVALID_ARG;
    if (B == 0) return EAS_OK;
    const int64_t groups = (int64_t)B * Tm * 2 * Hc * (Wc / 16);
    const int grid = eas_grid_1d(groups, EAS_BLOCK, 1 << 20);
    hipStream_t st = eas_s(stream);
    EAS_CLEAR_ERR();
    if (nbins == 10)
        EAS_LAUNCH((stacked_hist_sum_kernel<10>), dim3(grid), dim3(EAS_BLOCK), 0, st, hist, n_valid, B, Tm, nbins, H, W, Hc, Wc, out, groups);
    else
        EAS_LAUNCH((stacked_hist_sum_kernel<0>), dim3(grid), dim3(EAS_BLOCK), 0, st, hist, n_valid, B, Tm, nbins, H, W, Hc, Wc, out, groups);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

extern "C" int eas_stacked_hist_frames(const uint8_t* store, int64_t R, const int64_t* first, const int64_t* lo, const int32_t* params, int B,
                                       int Tm, int nbins, int H, int W, int Hc, int Wc, float* out, uint32_t* flags, eas_stream_t stream) {
    if (nbins == 10) return frames_call<BinPlanes<10>>(store, R, first, lo, params, B, Tm, nbins, H, W, Hc, Wc, out, flags, stream);
    return frames_call<BinPlanes<0>>(store, R, first, lo, params, B, Tm, nbins, H, W, Hc, Wc, out, flags, stream);
}

extern "C" int eas_count_store_frames(const uint16_t* sums, int64_t R, const int64_t* first, const int64_t* lo, const int32_t* params, int B, int Tm,
                                      int H, int W, int Hc, int Wc, float* out, uint32_t* flags, eas_stream_t stream) {
    return frames_call<SumPlanes>(sums, R, first, lo, params, B, Tm, 1, H, W, Hc, Wc, out, flags, stream);
}

extern "C" int eas_packed_store_frames(const int64_t* table, const uint8_t* payload, int64_t units, int64_t R, const int64_t* first, const int64_t* lo,
                                       const int32_t* params, int B, int Tm, int H, int W, int Hc, int Wc, float* out, uint32_t* flags,
                                       eas_stream_t stream) {
    return frames_call<PackedPlanes>(PackedRows{table, reinterpret_cast<const uint4*>(payload), units}, R, first, lo, params, B, Tm, 1, H, W, Hc, Wc, out,
                                     flags, stream);
}

namespace {
// what the three row entries ask of their common arguments; the u16 side is read or written in 16-byte pieces where W % 8 == 0
int rows_args(const uint16_t* sums, int64_t n, int H, int W, const int64_t* table, int64_t* blocks) {
    if (!sums || !table || n < 0 || H < 1 || W < 1) return EAS_ERR_INVALID_ARG;
    if (((uintptr_t)table & 7) || ((uintptr_t)sums & ((W & 7) == 0 ? 15 : 1))) return EAS_ERR_INVALID_ARG;
    if (W > PackedPlanes::kMaxW) return EAS_ERR_UNSUPPORTED;
    *blocks = (n * 2 * H + kRowsPerBlock - 1) / kRowsPerBlock;
    return *blocks > INT32_MAX ? EAS_ERR_UNSUPPORTED : EAS_OK;
}
}  // namespace

extern "C" int eas_count_rows_measure(const uint16_t* sums, int64_t n, int H, int W, int64_t* table, eas_stream_t stream) {
    int64_t blocks;
    if (const int err = rows_args(sums, n, H, W, table, &blocks)) return err;
    if (n == 0) return EAS_OK;
    hipStream_t st = eas_s(stream);
    EAS_CLEAR_ERR();
    EAS_LAUNCH(count_rows_measure_kernel, dim3((unsigned)blocks), dim3(EAS_BLOCK), 0, st, sums, n * 2 * H, H, W, table);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

extern "C" int eas_count_rows_pack(const uint16_t* sums, int64_t n, int H, int W, const int64_t* table, uint8_t* payload, int64_t unit_lo,
                                   int64_t unit_hi, eas_stream_t stream) {
    int64_t blocks;
    if (const int err = rows_args(sums, n, H, W, table, &blocks)) return err;
    if (unit_lo < 0 || unit_hi < unit_lo || (!payload && unit_hi > unit_lo) || ((uintptr_t)payload & 15)) return EAS_ERR_INVALID_ARG;
    if (n == 0 || unit_hi == unit_lo) return EAS_OK;
    hipStream_t st = eas_s(stream);
    EAS_CLEAR_ERR();
    EAS_LAUNCH(count_rows_pack_kernel, dim3((unsigned)blocks), dim3(EAS_BLOCK), 0, st, sums, n * 2 * H, H, W, table, reinterpret_cast<uint4*>(payload),
               (uint64_t)unit_lo, (uint64_t)unit_hi);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

extern "C" int eas_count_rows_unpack(const int64_t* table, const uint8_t* payload, int64_t units, int64_t n, int H, int W, uint16_t* sums,
                                     eas_stream_t stream) {
    int64_t blocks;
    if (const int err = rows_args(sums, n, H, W, table, &blocks)) return err;
    const PackedRows store{table, reinterpret_cast<const uint4*>(payload), units};
    if (!PackedPlanes::valid(store)) return EAS_ERR_INVALID_ARG;
    if (n == 0) return EAS_OK;
    hipStream_t st = eas_s(stream);
    EAS_CLEAR_ERR();
    EAS_LAUNCH(count_rows_unpack_kernel, dim3((unsigned)blocks), dim3(EAS_BLOCK), 0, st, store, n * 2 * H, W, sums);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

extern "C" int eas_stacked_hist_bin_sums(const uint8_t* hist, int64_t n, int nbins, int H, int W, uint16_t* sums, eas_stream_t stream) {
    if (!hist || !sums || n < 0 || nbins < 1 || H < 1 || W < 1) return EAS_ERR_INVALID_ARG;
    if (nbins > 255) return EAS_ERR_UNSUPPORTED;                                    // a bin sum is held in 16 bits
    // rows of 16-byte loads and stores (W % 16 == 0: every chunk offset of such a store keeps the alignment); else bytes and 16-bit elements
    if (((uintptr_t)sums & 1) || ((W & 15) == 0 && (((uintptr_t)hist | (uintptr_t)sums) & 15))) return EAS_ERR_INVALID_ARG;
    if (n == 0) return EAS_OK;
    const int64_t groups = n * 2 * H * ((W + 15) / 16);
    const int grid = eas_grid_1d(groups, EAS_BLOCK, 1 << 20);
    hipStream_t st = eas_s(stream);
    EAS_CLEAR_ERR();
    if (nbins == 10)
        EAS_LAUNCH((stacked_hist_bin_sums_kernel<10>), dim3(grid), dim3(EAS_BLOCK), 0, st, hist, nbins, H, W, sums, groups);
    else
        EAS_LAUNCH((stacked_hist_bin_sums_kernel<0>), dim3(grid), dim3(EAS_BLOCK), 0, st, hist, nbins, H, W, sums, groups);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}
