// Config-4 input: RVT "stacked histogram" representation -> per-polarity event counts on the model canvas.
// Replaces RVTGEN4Dataset.generate_slices(..., method='event_sum') + the zero padding of the validation letterbox
// (yolox/data/datasets/rvt_gen4.py:109-125 and :516-533 with scale 1).
//
//   hist  u8  [B][Tm][2*nbins][H][W]   channel = polarity * nbins + bin  (the reference's reshape(n, 2, -1, H, W))
//   out   f32 [B][Tm][2][Hc][Wc]       out[b][j][p] = sum over bins of hist[b][i][p*nbins + bin], zero outside H x W
// A sample whose sequence is younger than Tm representations supplies only its first n_valid[b] slices; they are the
// LAST n_valid[b] output slices (j = Tm - n_valid[b] + i), the leading ones are zero (rvt_gen4.py:122-123).
//
// HBM-bound integer work: per output element nbins bytes read + 4 bytes written (14 B at nbins = 10).  One thread owns 16
// consecutive pixels of one (b, j, p, row): nbins 16-byte loads issued up front (64 lanes x 16 B = 1 KiB contiguous per plane
// row), byte-wise unpack-accumulate in 16 integer registers, four float4 stores.  Sums <= 255 * nbins are exact in fp32.
#include "eas_common.h"
#include "linear_tap.h"

namespace {


template <int NB>
__global__ __launch_bounds__(EAS_BLOCK) void stacked_hist_sum_kernel(const uint8_t* __restrict__ hist, const int32_t* __restrict__ n_valid,
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
        const int nv = n_valid ? n_valid[b] : Tm;
        const int i = j - (Tm - nv);                     // input slice feeding output slice j
        if (i < 0 || y >= H || x0 >= W) {
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            dst[0] = z; dst[1] = z; dst[2] = z; dst[3] = z;
            continue;
        }
        const uint8_t* src = hist + ((((int64_t)b * Tm + i) * 2 + p) * nbins) * plane + (int64_t)y * W + x0;
        uint32_t acc[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0;
        if (x0 + 16 <= W && (W & 15) == 0) {
            uint4 v[NB > 0 ? NB : 1];
            if (NB > 0) {
#pragma unroll
                for (int k = 0; k < NB; ++k) v[k] = *reinterpret_cast<const uint4*>(src + (int64_t)k * plane);
#pragma unroll
                for (int k = 0; k < NB; ++k) {
                    const uint32_t wds[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        acc[4 * q + 0] += wds[q] & 0xffu;
                        acc[4 * q + 1] += (wds[q] >> 8) & 0xffu;
                        acc[4 * q + 2] += (wds[q] >> 16) & 0xffu;
                        acc[4 * q + 3] += wds[q] >> 24;
                    }
                }
            } else {
                for (int k = 0; k < nbins; ++k) {
                    const uint4 u = *reinterpret_cast<const uint4*>(src + (int64_t)k * plane);
                    const uint32_t wds[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        acc[4 * q + 0] += wds[q] & 0xffu;
                        acc[4 * q + 1] += (wds[q] >> 8) & 0xffu;
                        acc[4 * q + 2] += (wds[q] >> 16) & 0xffu;
                        acc[4 * q + 3] += wds[q] >> 24;
                    }
                }
            }
        } else {                                         // ragged row end or rows that are not 16-byte aligned: bytes one by one
            for (int k = 0; k < nbins; ++k) {
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    if (x0 + e < W) acc[e] += src[(int64_t)k * plane + e];
            }
        }
        dst[0] = make_float4((float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]);
        dst[1] = make_float4((float)acc[4], (float)acc[5], (float)acc[6], (float)acc[7]);
        dst[2] = make_float4((float)acc[8], (float)acc[9], (float)acc[10], (float)acc[11]);
        dst[3] = make_float4((float)acc[12], (float)acc[13], (float)acc[14], (float)acc[15]);
    }
}

// ---- training input: indices into a resident store -> augmented frames (eas_stacked_hist_frames) --------------------------------------
// RVTGEN4Dataset.__getitem__ for a training sample (rvt_gen4.py:190-235): the last Tm representations up to the label's
// (generate_slices, :109-125, zero slices in front of a young sequence), the bin sum, then get_random_data's resize / paste / flip with
// cv2.INTER_LINEAR (:510-598) -- the arithmetic of counts_letterbox_kernel (events.hip) on the integer bin sums, without the int32 frames in
// between.
//
// One block takes a band of output rows of one (sample, slice, polarity).  The vertical taps of the band name at most 2 * rows source
// rows; only those are read: their bin sums (<= 255 * nbins <= 65025: 16 bits) are staged in LDS, 16 pixels per lane and step with nbins
// 16-byte loads issued up front (bytes one by one when rows are not 16-byte aligned), then every output pixel is a gather from LDS with
// the horizontal taps of the band (one table per block) and the stores are float4.  Zero slices and bands outside the paste rectangle are
// stores only.  params are device data nobody has validated: the paste rectangle is whatever part of [dx, dx + nw) x [dy, dy + nh) lies on
// the canvas, nw <= 0 or nh <= 0 is an empty one, and a source row or column index comes out of linear_tap, which clamps to the sensor.
constexpr int kFrameBandRows = 8;             // output rows per block at most (fewer on wide sensors: frames_band_rows)
constexpr int kFrameLdsBytes = 48 * 1024;     // staged rows + tap tables

struct XTap { uint32_t s01; float w1; };      // s0 | s1 << 16; w1 < 0: outside the paste rectangle

// 16 bin sums (pixels x0 .. x0 + 15 of one source row) as eight words of two 16-bit sums, pixel order.  Two bytes of a word are added per
// operation: even and odd bytes go to accumulators of two 16-bit lanes each.
template <int NB>
__device__ __forceinline__ void bin_sums16(const uint8_t* __restrict__ src, int64_t plane, int nbins, bool vec, int n_left, uint32_t (&sum)[8]) {
    uint32_t ev[4] = {0, 0, 0, 0}, od[4] = {0, 0, 0, 0};     // ev[q]: pixels 4q, 4q + 2; od[q]: pixels 4q + 1, 4q + 3
    if (vec) {
        if (NB > 0) {
            uint4 v[NB > 0 ? NB : 1];
#pragma unroll
            for (int k = 0; k < NB; ++k) v[k] = *reinterpret_cast<const uint4*>(src + (int64_t)k * plane);
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                const uint32_t wds[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    ev[q] += wds[q] & 0x00ff00ffu;
                    od[q] += (wds[q] >> 8) & 0x00ff00ffu;
                }
            }
        } else {
            for (int k = 0; k < nbins; ++k) {
                const uint4 u = *reinterpret_cast<const uint4*>(src + (int64_t)k * plane);
                const uint32_t wds[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    ev[q] += wds[q] & 0x00ff00ffu;
                    od[q] += (wds[q] >> 8) & 0x00ff00ffu;
                }
            }
        }
    } else {                                  // rows that are not 16-byte aligned, ragged row end: n_left < 16 pixels exist
        for (int k = 0; k < nbins; ++k) {
            const uint8_t* row = src + (int64_t)k * plane;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const uint32_t v = e < n_left ? (uint32_t)row[e] : 0u;
                if (e & 1) od[e >> 2] += v << (8 * (e & 2)); else ev[e >> 2] += v << (8 * (e & 2));
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        sum[2 * q] = (ev[q] & 0xffffu) | (od[q] << 16);
        sum[2 * q + 1] = (ev[q] >> 16) | (od[q] & 0xffff0000u);
    }
}

template <int NB>
__global__ __launch_bounds__(EAS_BLOCK) void stacked_hist_frames_kernel(const uint8_t* __restrict__ store, int64_t R, const int64_t* __restrict__ first,
                                                                        const int64_t* __restrict__ lo, const int32_t* __restrict__ params,
                                                                        int Tm, int nbins_rt, int H, int W, int Hc, int Wc, int band_rows,
                                                                        int nbands, float* __restrict__ out, uint32_t* __restrict__ flags) {
    extern __shared__ __attribute__((aligned(16))) unsigned char frames_lds[];
    __shared__ int y_s0[kFrameBandRows], y_s1[kFrameBandRows], y_slot0[kFrameBandRows], y_slot1[kFrameBandRows];
    __shared__ float y_w1[kFrameBandRows];
    __shared__ int slot_row[2 * kFrameBandRows];
    __shared__ int n_slots;
    const int nbins = NB > 0 ? NB : nbins_rt;
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

    // slice index: clamped to [-Tm, R] before j is added (any int64 may come in); below the recording's first representation: zero,
    // at or behind the end of the store: zero and flagged
    int64_t f0 = first[b];
    f0 = f0 > R ? R : (f0 < -(int64_t)Tm ? -(int64_t)Tm : f0);
    int64_t low = lo ? lo[b] : 0;
    low = low < 0 ? 0 : low;
    if (flags && band == 0 && p == 0 && j == 0 && tid == 0) {
        uint32_t fl = 0;
        for (int k = 0; k < Tm; ++k) fl |= (f0 + k >= low && f0 + k >= R) ? 1u : 0u;
        flags[b] = fl;
    }
    const int64_t idx = f0 + j;
    const bool have = idx >= low && idx < R;

    int nw = W, nh = H, dx = 0, dy = 0, flip = 0;
    if (params) {
        const int32_t* pr = params + 5 * (int64_t)b;
        nw = pr[0]; nh = pr[1]; dx = pr[2]; dy = pr[3]; flip = pr[4];
    }
    const bool identity = nw == W && nh == H;             // cv2.resize with dsize == size is a copy
    float4* dst = reinterpret_cast<float4*>(out + ((((int64_t)b * Tm + j) * 2 + p) * Hc + y0) * (int64_t)Wc);
    const int wc4 = Wc / 4;

    // vertical taps of the band's rows, and whether the band meets the paste rectangle at all (block-uniform)
    const int64_t ys_first = (int64_t)y0 - dy, ys_last = ys_first + rows - 1;
    const bool touches = have && nw > 0 && nh > 0 && ys_last >= 0 && ys_first < nh && (int64_t)dx < Wc && (int64_t)dx + nw > 0;
    if (!touches) {
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int i = tid; i < rows * wc4; i += EAS_BLOCK) dst[i] = z;
        return;
    }
    if (tid < rows) {
        const int64_t ys = ys_first + tid;
        float w1 = -1.f;
        int s0 = 0, s1 = 0;
        if (ys >= 0 && ys < nh) {
            if (identity) {
                s0 = s1 = (int)ys;
                w1 = 0.f;
            } else {
                const AxisTap t = linear_tap((int)ys, H, nh);
                s0 = t.s0; s1 = t.s1; w1 = t.w1;
            }
        }
        y_s0[tid] = s0; y_s1[tid] = s1; y_w1[tid] = w1;
    }
    // horizontal taps of every canvas column
    for (int xx = tid; xx < Wc; xx += EAS_BLOCK) {
        const int64_t xs = (int64_t)(flip ? Wc - 1 - xx : xx) - dx;
        XTap t{0u, -1.f};
        if (xs >= 0 && xs < nw) {
            if (identity) {
                t.s01 = (uint32_t)xs | ((uint32_t)xs << 16);
                t.w1 = 0.f;
            } else {
                const AxisTap a = linear_tap((int)xs, W, nw);
                t.s01 = (uint32_t)a.s0 | ((uint32_t)a.s1 << 16);
                t.w1 = a.w1;
            }
        }
        xtab[xx] = t;
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
    const int64_t plane = (int64_t)H * W;
    const uint8_t* src0 = store + ((idx * 2 + p) * nbins) * plane;
    const bool aligned = (W & 15) == 0;
    for (int g = tid; g < n_groups; g += EAS_BLOCK) {
        const int slot = g / wg, x0 = (g - slot * wg) * 16;
        uint32_t sum[8];
        bin_sums16<NB>(src0 + (int64_t)slot_row[slot] * W + x0, plane, nbins, aligned, W - x0, sum);
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
            const uint16_t* r0 = stage + (size_t)y_slot0[q] * wp;
            const uint16_t* r1 = stage + (size_t)y_slot1[q] * wp;
            const float wy0 = 1.f - wy1;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const XTap t = xtab[x4 + e];
                if (t.w1 < 0.f) continue;
                const int s0 = t.s01 & 0xffffu, s1 = t.s01 >> 16;
                if (identity) {
                    v[e] = (float)(int)r0[s0];
                } else {
                    const float wx0 = 1.f - t.w1;
                    const double a0 = (double)(int)r0[s0] * (double)wx0 + (double)(int)r0[s1] * (double)t.w1;
                    const double a1 = (double)(int)r1[s0] * (double)wx0 + (double)(int)r1[s1] * (double)t.w1;
                    v[e] = (float)(a0 * (double)wy0 + a1 * (double)wy1);
                }
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

}  // namespace

extern "C" int eas_stacked_hist_event_sum(const uint8_t* hist, const int32_t* n_valid, int B, int Tm, int nbins, int H, int W, int Hc,
                                          int Wc, float* out, eas_stream_t stream) {
    if (!hist || !out || B < 0 || Tm < 1 || nbins < 1 || H < 1 || W < 1 || Hc < H || Wc < W) return EAS_ERR_INVALID_ARG;
    if (Wc % 16 != 0 || nbins > 255) return EAS_ERR_UNSUPPORTED;      // model canvases are multiples of 32
    if (((uintptr_t)hist | (uintptr_t)out) & 15) return EAS_ERR_INVALID_ARG;
    if (B == 0) return EAS_OK;
    const int64_t groups = (int64_t)B * Tm * 2 * Hc * (Wc / 16);
    const int grid = eas_grid_1d(groups, EAS_BLOCK, 1 << 20);
    hipStream_t st = eas_s(stream);
    EAS_CLEAR_ERR();
    if (nbins == 10)
        EAS_LAUNCH((stacked_hist_sum_kernel<10>), dim3(grid), dim3(EAS_BLOCK), 0, st, hist, n_valid, Tm, nbins, H, W, Hc, Wc, out, groups);
    else
        EAS_LAUNCH((stacked_hist_sum_kernel<0>), dim3(grid), dim3(EAS_BLOCK), 0, st, hist, n_valid, Tm, nbins, H, W, Hc, Wc, out, groups);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

extern "C" int eas_stacked_hist_frames(const uint8_t* store, int64_t R, const int64_t* first, const int64_t* lo, const int32_t* params, int B,
                                       int Tm, int nbins, int H, int W, int Hc, int Wc, float* out, uint32_t* flags, eas_stream_t stream) {
    if (!store || !first || !out || R < 1 || B < 1 || Tm < 1 || nbins < 1 || H < 1 || W < 1 || Hc < 1 || Wc < 1) return EAS_ERR_INVALID_ARG;
    if ((((uintptr_t)store | (uintptr_t)out) & 15) || (((uintptr_t)first | (uintptr_t)lo) & 7) || (((uintptr_t)params | (uintptr_t)flags) & 3))
        return EAS_ERR_INVALID_ARG;
    if (Wc % 16 != 0 || nbins > 255 || W > 65536) return EAS_ERR_UNSUPPORTED;      // model canvases are multiples of 32; taps are 16 bits
    const int band_rows = frames_band_rows(W, Wc);
    if (band_rows < 1) return EAS_ERR_UNSUPPORTED;
    const int nbands = (Hc + band_rows - 1) / band_rows;
    const int64_t blocks = (int64_t)B * Tm * 2 * nbands;
    if (blocks > INT32_MAX) return EAS_ERR_UNSUPPORTED;
    const size_t lds = (size_t)2 * band_rows * ((W + 15) & ~15) * sizeof(uint16_t) + (size_t)Wc * sizeof(XTap);
    hipStream_t st = eas_s(stream);
    EAS_CLEAR_ERR();
    if (nbins == 10)
        EAS_LAUNCH((stacked_hist_frames_kernel<10>), dim3((unsigned)blocks), dim3(EAS_BLOCK), lds, st, store, R, first, lo, params, Tm, nbins, H, W,
                   Hc, Wc, band_rows, nbands, out, flags);
    else
        EAS_LAUNCH((stacked_hist_frames_kernel<0>), dim3((unsigned)blocks), dim3(EAS_BLOCK), lds, st, store, R, first, lo, params, Tm, nbins, H, W,
                   Hc, Wc, band_rows, nbands, out, flags);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}
