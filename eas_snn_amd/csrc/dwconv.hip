// Depthwise 3x3 convolution (groups == Cin == Cout == C, padding 1, stride 1 / 2): forward, input gradient, weight gradient.
//
// The geometry network_blocks.DWConv instantiates (yolox/models/network_blocks.py:59-76, always ksize 3): the depthwise half of every block
// of the depthwise=True models (YOLOX-nano family).  9 multiply-adds per output element: no matrix cores, vector FMA at the memory
// roofline.  Everything here is built on ONE tile:
//
//   tile   = 8 consecutive channels (one channel group: the 16-byte unit of the spike planes) x a band of `bh` output rows of `IB`
//            consecutive images (IB > 1 only when a whole map is one band: the small maps at the end of the backbone)
//   LDS    = the input rows of the band with a zero halo, fp32, [IB][8][rows_in][Wi + 2], rows_in = (bh - 1) * stride + 3: nothing is
//            masked in the compute loop.  At most DW_TILE_FLOATS floats (48 KiB: three blocks per CU).
//   lanes  = consecutive output pixels of the band; every lane computes its pixel for the 8 channels (the 72 weights are block-uniform:
//            scalar registers), so each channel is stored as a contiguous run of pixels across the wave.
//
// Both input forms (fp32 NCHW, spike planes [NI][C/8][HW][8] bf16) fill the same LDS image and run the same compute body (dw_pixel): the
// nine products are added kh-major, kw-minor, bias last, as written fma -- on an input that is exact in bf16 the two forms give
// bit-identical y, the convention eas_conv_fwd_planes keeps.
//
// forward          grid (nb, C/8): nb = image tiles x row bands = the statistics blocks of the epilogue (stats[C][nb][2] doubles)
// dgrad stride 1   the forward on grad_y with the taps flipped
// dgrad stride 2   gather per 2x2 input quad: the four pixels of a quad read the same four grad_y values, each through the taps whose
//                  parity matches (1, 2, 2 and 4 of the 9); no scatter, no atomics
// wgrad            stage 1: a block walks `tiles per part` forward tiles, keeps 8 x 9 fp32 accumulators per lane, reduces them over the
//                  wave (shuffles, fixed order) and the block's waves (in wave order) into workspace[C][nparts][9]; stage 2 adds the
//                  nparts partials in double in a fixed order.  Deterministic; no float atomics.
#include "eas_common.h"

namespace {

constexpr int DW_TILE_FLOATS = 12288;      // LDS image of one tile (48 KiB)
constexpr int DW_CG = 8;                   // channels per tile
constexpr int DW_NW = EAS_BLOCK / EAS_WAVE;
constexpr int DW_STAGE_U = 4;               // loads in flight per lane while a tile is staged
constexpr int DW_RED_FLOATS = 16 * EAS_BLOCK + 2 * 16 * 16;      // statistics epilogue: 16 fp32 values per thread + 16 x 16 doubles

struct DwPlan {
    int NI, C, Hi, Wi, Ho, Wo, stride;
    int G;            // channel groups
    int Wp;           // LDS row pitch (Wi + 2)
    int bh;           // output rows per band
    int rows_in;      // staged input rows per band
    int nbands;
    int IB;           // images per tile
    int nimg_tiles;   // ceil(NI / IB)
    int nb;           // tiles per channel group = nimg_tiles * nbands
};

// 0 = no tile for this geometry
bool dw_plan(int NI, int C, int Hi, int Wi, int stride, DwPlan& p) {
    if (NI < 1 || C < 1 || Hi < 1 || Wi < 1 || (stride != 1 && stride != 2)) return false;
    p.NI = NI; p.C = C; p.Hi = Hi; p.Wi = Wi; p.stride = stride;
    p.Ho = (Hi - 1) / stride + 1;
    p.Wo = (Wi - 1) / stride + 1;
    p.G = (C + DW_CG - 1) / DW_CG;
    p.Wp = Wi + 2;
    if (p.G > 65535) return false;
    const int max_rows = DW_TILE_FLOATS / (DW_CG * p.Wp);          // staged rows that fit
    if (max_rows < 3) return false;
    int bh = (max_rows - 3) / stride + 1;
    if (bh > p.Ho) bh = p.Ho;
    p.nbands = (p.Ho + bh - 1) / bh;
    p.bh = (p.Ho + p.nbands - 1) / p.nbands;                       // even bands
    p.rows_in = (p.bh - 1) * stride + 3;
    p.IB = 1;
    if (p.nbands == 1) {
        p.IB = DW_TILE_FLOATS / (DW_CG * p.rows_in * p.Wp);
        if (p.IB > NI) p.IB = NI;
        if (p.IB < 1) p.IB = 1;
    }
    p.nimg_tiles = (NI + p.IB - 1) / p.IB;
    const int64_t nb = (int64_t)p.nimg_tiles * p.nbands;
    if (nb > 0x7fffffff) return false;
    p.nb = (int)nb;
    return true;
}

struct DwGeom {
    int NI, C, Hi, Wi, Ho, Wo, Wp, bh, rows_in, nbands, IB, G;
};

DwGeom dw_geom(const DwPlan& p) {
    return DwGeom{p.NI, p.C, p.Hi, p.Wi, p.Ho, p.Wo, p.Wp, p.bh, p.rows_in, p.nbands, p.IB, p.G};
}

__device__ __forceinline__ float dw_bf16(unsigned short b) { return __uint_as_float((unsigned)b << 16); }

// Fill the LDS image of tile (images n0 .. n0 + IB, channel group g, output rows from h0) from x.  FORM 1: fp32 [NI][C][Hi][Wi] (VEC: rows
// are 16-byte aligned, float4 loads); FORM 2: spike planes [NI][C/8][Hi*Wi][8] bf16, one 16-byte load per pixel.  Rows outside the image,
// images past NI and channels past C are written as zeros; so are the two halo columns.
template <int FORM, int S, bool VEC>
__device__ __forceinline__ void dw_stage(const void* __restrict__ xv, float* __restrict__ tile, const DwGeom& d, int g, int n0, int h0) {
    const int tid = threadIdx.x;
    const int in_row0 = h0 * S - 1;
    const int nrows = d.IB * DW_CG * d.rows_in;          // LDS rows
    for (int r = tid; r < nrows; r += EAS_BLOCK) {
        tile[r * d.Wp] = 0.0f;
        tile[r * d.Wp + d.Wp - 1] = 0.0f;
    }
    // DW_STAGE_U loads of a lane are issued before the first of them is written to LDS: the staging is pure memory latency, and with one
    // load in flight per lane a CU's 12 waves do not cover it
    if (FORM == 2) {
        const uint4* __restrict__ xp = reinterpret_cast<const uint4*>(xv);
        const int total = d.IB * d.rows_in * d.Wi;
        const int plane = DW_CG * d.rows_in * d.Wp;      // LDS floats per image
        const int cs = d.rows_in * d.Wp;
        for (int e0 = tid; e0 < total; e0 += DW_STAGE_U * EAS_BLOCK) {
            uint4 v[DW_STAGE_U];
            int off[DW_STAGE_U];
#pragma unroll
            for (int u = 0; u < DW_STAGE_U; ++u) {
                const int e = e0 + u * EAS_BLOCK;
                const int ir = e / d.Wi, col = e - ir * d.Wi;
                const int i = ir / d.rows_in, rr = ir - i * d.rows_in;
                const int in_row = in_row0 + rr;
                off[u] = e < total ? i * plane + rr * d.Wp + col + 1 : -1;
                v[u] = make_uint4(0u, 0u, 0u, 0u);
                if (e < total && n0 + i < d.NI && in_row >= 0 && in_row < d.Hi)
                    v[u] = xp[((int64_t)(n0 + i) * d.G + g) * ((int64_t)d.Hi * d.Wi) + (int64_t)in_row * d.Wi + col];
            }
#pragma unroll
            for (int u = 0; u < DW_STAGE_U; ++u) {
                if (off[u] < 0) continue;
                float* t = tile + off[u];
                t[0 * cs] = dw_bf16((unsigned short)(v[u].x & 0xffffu));
                t[1 * cs] = dw_bf16((unsigned short)(v[u].x >> 16));
                t[2 * cs] = dw_bf16((unsigned short)(v[u].y & 0xffffu));
                t[3 * cs] = dw_bf16((unsigned short)(v[u].y >> 16));
                t[4 * cs] = dw_bf16((unsigned short)(v[u].z & 0xffffu));
                t[5 * cs] = dw_bf16((unsigned short)(v[u].z >> 16));
                t[6 * cs] = dw_bf16((unsigned short)(v[u].w & 0xffffu));
                t[7 * cs] = dw_bf16((unsigned short)(v[u].w >> 16));
            }
        }
    } else {
        const float* __restrict__ x = reinterpret_cast<const float*>(xv);
        const int wq = VEC ? d.Wi / 4 : d.Wi;             // loads per row
        const int total = nrows * wq;
        for (int e0 = tid; e0 < total; e0 += DW_STAGE_U * EAS_BLOCK) {
            float4 v[DW_STAGE_U];
            int off[DW_STAGE_U];
#pragma unroll
            for (int u = 0; u < DW_STAGE_U; ++u) {
                const int e = e0 + u * EAS_BLOCK;
                const int r = e / wq, q = e - r * wq;     // LDS row ((i * 8 + ch) * rows_in + rr), load q of the row
                const int ic = r / d.rows_in, rr = r - ic * d.rows_in;
                const int i = ic / DW_CG, ch = ic - i * DW_CG;
                const int in_row = in_row0 + rr;
                const int c = g * DW_CG + ch;
                const bool ok = e < total && n0 + i < d.NI && c < d.C && in_row >= 0 && in_row < d.Hi;
                const int64_t src = (((int64_t)(n0 + i) * d.C + c) * d.Hi + in_row) * (int64_t)d.Wi;
                off[u] = e < total ? r * d.Wp + 1 + (VEC ? 4 * q : q) : -1;
                v[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (ok) {
                    if (VEC) v[u] = *reinterpret_cast<const float4*>(x + src + 4 * q);
                    else v[u].x = x[src + q];
                }
            }
#pragma unroll
            for (int u = 0; u < DW_STAGE_U; ++u) {
                if (off[u] < 0) continue;
                float* t = tile + off[u];
                t[0] = v[u].x;
                if (VEC) {
                    t[1] = v[u].y;
                    t[2] = v[u].z;
                    t[3] = v[u].w;
                }
            }
        }
    }
}

// THE compute body: one output pixel of one channel from the LDS image, the nine products added kh-major, kw-minor
template <int S, bool FLIP>
__device__ __forceinline__ float dw_pixel(const float* __restrict__ t, int Wp, const float (&w)[9]) {
    float acc = t[0] * w[FLIP ? 8 : 0];
#pragma unroll
    for (int k = 1; k < 9; ++k) acc = __builtin_fmaf(t[(k / 3) * Wp + (k % 3)], w[FLIP ? 8 - k : k], acc);
    return acc;
}

// output pixel p of a tile -> (image i, row r, column c) and whether it exists
struct DwPix {
    int i, r, c;
    bool valid;
};
__device__ __forceinline__ DwPix dw_pix(int p, const DwGeom& d, int n0, int h0) {
    DwPix o;
    const int q = p / d.Wo;
    o.c = p - q * d.Wo;
    o.i = q / d.bh;
    o.r = q - o.i * d.bh;
    o.valid = n0 + o.i < d.NI && h0 + o.r < d.Ho;
    return o;
}

// ---------------------------------------------------------------------------------------------------------------- forward
template <int FORM, int S, bool FLIP, bool VEC>
__global__ __launch_bounds__(EAS_BLOCK) void dwconv_fwd_kernel(const void* __restrict__ x, const float* __restrict__ wgt, const float* __restrict__ bias,
                                                               float* __restrict__ y, DwGeom d, double* __restrict__ stats, int nb) {
    extern __shared__ __align__(16) float tile[];
    const int g = blockIdx.y;
    const int it = blockIdx.x / d.nbands, band = blockIdx.x - it * d.nbands;
    const int n0 = it * d.IB, h0 = band * d.bh;
    const int tid = threadIdx.x;

    float w[DW_CG][9], b[DW_CG];
#pragma unroll
    for (int ch = 0; ch < DW_CG; ++ch) {
        const int c = min(g * DW_CG + ch, d.C - 1);
#pragma unroll
        for (int k = 0; k < 9; ++k) w[ch][k] = wgt[c * 9 + k];
        b[ch] = bias ? bias[c] : 0.0f;
    }

    dw_stage<FORM, S, VEC>(x, tile, d, g, n0, h0);
    __syncthreads();

    float s[DW_CG], q[DW_CG];
#pragma unroll
    for (int ch = 0; ch < DW_CG; ++ch) { s[ch] = 0.0f; q[ch] = 0.0f; }

    const int npix = d.IB * d.bh * d.Wo;
    const int cs = d.rows_in * d.Wp;
    const int64_t HWo = (int64_t)d.Ho * d.Wo;
    for (int p = tid; p < npix; p += EAS_BLOCK) {
        const DwPix o = dw_pix(p, d, n0, h0);
        if (!o.valid) continue;
        const float* t = tile + (o.i * DW_CG * d.rows_in + o.r * S) * d.Wp + o.c * S;
        float* yo = y + ((int64_t)(n0 + o.i) * d.C + g * DW_CG) * HWo + (int64_t)(h0 + o.r) * d.Wo + o.c;
#pragma unroll
        for (int ch = 0; ch < DW_CG; ++ch) {
            if (g * DW_CG + ch < d.C) {           // block-uniform
                float v = dw_pixel<S, FLIP>(t + ch * cs, d.Wp, w[ch]);
                if (bias) v += b[ch];
                yo[ch * HWo] = v;
                s[ch] += v;
                q[ch] = __builtin_fmaf(v, v, q[ch]);
            }
        }
    }
    if (!stats) return;             // kernel argument: uniform

    // Statistics epilogue.  A lane's own values (at most npix / 256 <= 6 per channel) were added in fp32; everything above in double, in a
    // fixed order: thread (k, part) adds the values of lanes part, part + 16, ... of quantity k (channel, sum | sum of squares), then thread k
    // adds the 16 parts in order.
    __syncthreads();                // the LDS image is free
    float* red = tile;
    double* red2 = reinterpret_cast<double*>(tile + 16 * EAS_BLOCK);
#pragma unroll
    for (int ch = 0; ch < DW_CG; ++ch) {
        red[(2 * ch + 0) * EAS_BLOCK + tid] = s[ch];
        red[(2 * ch + 1) * EAS_BLOCK + tid] = q[ch];
    }
    __syncthreads();
    {
        const int k = tid >> 4, part = tid & 15;
        double a = 0.0;
#pragma unroll
        for (int j = 0; j < 16; ++j) a += (double)red[k * EAS_BLOCK + j * 16 + part];
        red2[k * 16 + part] = a;
    }
    __syncthreads();
    if (tid < 16) {
        const int ch = tid >> 1, c = g * DW_CG + ch;
        if (c < d.C) {
            double a = 0.0;
#pragma unroll
            for (int j = 0; j < 16; ++j) a += red2[tid * 16 + j];
            stats[((int64_t)c * nb + blockIdx.x) * 2 + (tid & 1)] = a;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- input gradient, stride 2
// Block = one channel (blockIdx.y) and a grid-stride share of its (image, 2x2 input quad) items.  Quad (a, b) = input pixels
// (2a + {0,1}, 2b + {0,1}); with g = grad_y of the channel (zero outside), from y[ho][wo] = sum x[2ho - 1 + kh][2wo - 1 + kw] w[kh][kw]:
//   gx[2a  ][2b  ] = g[a][b] w11
//   gx[2a  ][2b+1] = g[a][b+1] w10 + g[a][b] w12
//   gx[2a+1][2b  ] = g[a+1][b] w01 + g[a][b] w21
//   gx[2a+1][2b+1] = g[a+1][b+1] w00 + g[a+1][b] w02 + g[a][b+1] w20 + g[a][b] w22
__global__ __launch_bounds__(EAS_BLOCK) void dwconv_dgrad_s2_kernel(const float* __restrict__ gy, const float* __restrict__ wgt, float* __restrict__ gx,
                                                                    int NI, int C, int Hi, int Wi, int Ho, int Wo) {
    const int c = blockIdx.y;
    float w[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) w[k] = wgt[c * 9 + k];
    const int Ha = (Hi + 1) / 2, Wb = (Wi + 1) / 2, Q = Ha * Wb;
    const int64_t total = (int64_t)NI * Q;
    const bool pair = (Wi & 1) == 0;          // (h * Wi + 2b) is even: 8-byte stores
    for (int64_t idx = (int64_t)blockIdx.x * EAS_BLOCK + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * EAS_BLOCK) {
        const int n = (int)(idx / Q), qd = (int)(idx - (int64_t)n * Q);
        const int a = qd / Wb, b = qd - a * Wb;
        const float* gp = gy + ((int64_t)n * C + c) * ((int64_t)Ho * Wo);
        const bool a1 = a + 1 < Ho, b1 = b + 1 < Wo;          // (a < Ho and b < Wo always: Ho = Ha, Wo = Wb)
        const float g00 = gp[a * Wo + b];
        const float g01 = b1 ? gp[a * Wo + b + 1] : 0.0f;
        const float g10 = a1 ? gp[(a + 1) * Wo + b] : 0.0f;
        const float g11 = (a1 && b1) ? gp[(a + 1) * Wo + b + 1] : 0.0f;
        const float o00 = g00 * w[4];
        const float o01 = __builtin_fmaf(g00, w[5], g01 * w[3]);
        const float o10 = __builtin_fmaf(g00, w[7], g10 * w[1]);
        const float o11 = __builtin_fmaf(g00, w[8], __builtin_fmaf(g01, w[6], __builtin_fmaf(g10, w[2], g11 * w[0])));
        float* xp = gx + ((int64_t)n * C + c) * ((int64_t)Hi * Wi);
        const int h = 2 * a, wc = 2 * b;
        const bool h1 = h + 1 < Hi, w1 = wc + 1 < Wi;
        if (pair) {
            *reinterpret_cast<float2*>(xp + h * Wi + wc) = make_float2(o00, o01);
            if (h1) *reinterpret_cast<float2*>(xp + (h + 1) * Wi + wc) = make_float2(o10, o11);
        } else {
            xp[h * Wi + wc] = o00;
            if (w1) xp[h * Wi + wc + 1] = o01;
            if (h1) {
                xp[(h + 1) * Wi + wc] = o10;
                if (w1) xp[(h + 1) * Wi + wc + 1] = o11;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- weight gradient
// stage 1: block (part, g) walks the forward tiles [part * tpb, (part + 1) * tpb) of channel group g
template <int FORM, int S, bool VEC>
__global__ __launch_bounds__(EAS_BLOCK) void dwconv_wgrad_kernel(const void* __restrict__ x, const float* __restrict__ gy, float* __restrict__ ws, DwGeom d,
                                                                 int nb, int tpb, int nparts) {
    extern __shared__ __align__(16) float tile[];
    __shared__ float wred[DW_NW][DW_CG * 9];
    const int g = blockIdx.y, part = blockIdx.x;
    const int tid = threadIdx.x;
    float acc[DW_CG][9];
#pragma unroll
    for (int ch = 0; ch < DW_CG; ++ch)
#pragma unroll
        for (int k = 0; k < 9; ++k) acc[ch][k] = 0.0f;

    const int npix = d.IB * d.bh * d.Wo;
    const int cs = d.rows_in * d.Wp;
    const int64_t HWo = (int64_t)d.Ho * d.Wo;
    const int t_end = min(nb, (part + 1) * tpb);
    for (int tl = part * tpb; tl < t_end; ++tl) {
        const int it = tl / d.nbands, band = tl - it * d.nbands;
        const int n0 = it * d.IB, h0 = band * d.bh;
        dw_stage<FORM, S, VEC>(x, tile, d, g, n0, h0);
        __syncthreads();
        for (int p = tid; p < npix; p += EAS_BLOCK) {
            const DwPix o = dw_pix(p, d, n0, h0);
            if (!o.valid) continue;
            const float* t = tile + (o.i * DW_CG * d.rows_in + o.r * S) * d.Wp + o.c * S;
            const float* go = gy + ((int64_t)(n0 + o.i) * d.C + g * DW_CG) * HWo + (int64_t)(h0 + o.r) * d.Wo + o.c;
#pragma unroll
            for (int ch = 0; ch < DW_CG; ++ch) {
                if (g * DW_CG + ch < d.C) {       // block-uniform
                    const float gv = go[ch * HWo];
                    const float* tc = t + ch * cs;
#pragma unroll
                    for (int k = 0; k < 9; ++k) acc[ch][k] = __builtin_fmaf(gv, tc[(k / 3) * d.Wp + (k % 3)], acc[ch][k]);
                }
            }
        }
        __syncthreads();            // everyone is done with the image before the next one is staged
    }
    const int lane = tid & (EAS_WAVE - 1), wid = tid / EAS_WAVE;
#pragma unroll
    for (int ch = 0; ch < DW_CG; ++ch)
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const float v = eas_wave_sum(acc[ch][k]);
            if (lane == 0) wred[wid][ch * 9 + k] = v;
        }
    __syncthreads();
    if (tid < DW_CG * 9) {
        const int c = g * DW_CG + tid / 9;
        if (c < d.C) {
            float v = wred[0][tid];
#pragma unroll
            for (int w_ = 1; w_ < DW_NW; ++w_) v += wred[w_][tid];
            ws[((int64_t)c * nparts + part) * 9 + tid % 9] = v;
        }
    }
}

// stage 2: one wave per (channel, tap): lane l adds partials l, l + 64, ... in double, then the lanes are added in a fixed order
__global__ __launch_bounds__(EAS_BLOCK) void dwconv_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ gw, int C, int nparts) {
    const int lane = threadIdx.x & (EAS_WAVE - 1);
    const int item = blockIdx.x * DW_NW + threadIdx.x / EAS_WAVE;          // c * 9 + k
    if (item >= C * 9) return;
    const int c = item / 9, k = item - c * 9;
    double a = 0.0;
    for (int i = lane; i < nparts; i += EAS_WAVE) a += (double)ws[((int64_t)c * nparts + i) * 9 + k];
    a = eas_wave_sum(a);
    if (lane == 0) gw[item] = (float)a;
}

// weight-gradient decomposition: tiles per block and partials per channel
void dw_wgrad_split(const DwPlan& p, int& tpb, int& nparts) {
    int want = 2048 / p.G;                  // blocks per channel group for ~2048 blocks in all (8 per CU)
    if (want < 1) want = 1;
    if (want > p.nb) want = p.nb;
    tpb = (p.nb + want - 1) / want;
    nparts = (p.nb + tpb - 1) / tpb;
}

size_t dw_lds_bytes(const DwPlan& p, bool stats) {
    int fl = p.IB * DW_CG * p.rows_in * p.Wp;
    if (stats && fl < DW_RED_FLOATS) fl = DW_RED_FLOATS;
    return (size_t)fl * sizeof(float);
}

template <int FORM, bool FLIP>
int dw_launch_fwd(const void* x, const float* w, const float* bias, float* y, const DwPlan& p, double* stats, hipStream_t st) {
    const DwGeom d = dw_geom(p);
    const dim3 grid(p.nb, p.G), block(EAS_BLOCK);
    const size_t lds = dw_lds_bytes(p, stats != nullptr);
    const bool vec = FORM == 1 && p.Wi % 4 == 0 && ((uintptr_t)x & 15) == 0;
    EAS_CLEAR_ERR();
    if (p.stride == 1) {
        if (vec) EAS_LAUNCH((dwconv_fwd_kernel<FORM, 1, FLIP, true>), grid, block, lds, st, x, w, bias, y, d, stats, p.nb);
        else EAS_LAUNCH((dwconv_fwd_kernel<FORM, 1, FLIP, false>), grid, block, lds, st, x, w, bias, y, d, stats, p.nb);
    } else {
        if (vec) EAS_LAUNCH((dwconv_fwd_kernel<FORM, 2, FLIP, true>), grid, block, lds, st, x, w, bias, y, d, stats, p.nb);
        else EAS_LAUNCH((dwconv_fwd_kernel<FORM, 2, FLIP, false>), grid, block, lds, st, x, w, bias, y, d, stats, p.nb);
    }
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

template <int FORM>
int dw_fwd_entry(const void* x, const float* w, const float* bias, float* y, int NI, int C, int Hi, int Wi, int stride, double* stats, int nb,
                 eas_stream_t stream) {
    if (!x || !w || !y) return EAS_ERR_INVALID_ARG;
    DwPlan p;
    if (!dw_plan(NI, C, Hi, Wi, stride, p) || (FORM == 2 && C % 8 != 0)) return EAS_ERR_UNSUPPORTED;
    if (FORM == 2 && ((uintptr_t)x & 15)) return EAS_ERR_INVALID_ARG;
    if (((uintptr_t)y | (uintptr_t)w | (uintptr_t)bias) & 3) return EAS_ERR_INVALID_ARG;
    if (stats) {
        if (bias || nb != p.nb || ((uintptr_t)stats & 7)) return EAS_ERR_INVALID_ARG;
    } else if (nb != 0) {
        return EAS_ERR_INVALID_ARG;
    }
    return dw_launch_fwd<FORM, false>(x, w, bias, y, p, stats, eas_s(stream));
}

template <int FORM>
int dw_wgrad_entry(const void* x, const float* gy, float* ws, float* gw, int NI, int C, int Hi, int Wi, int stride, eas_stream_t stream) {
    if (!x || !gy || !ws || !gw) return EAS_ERR_INVALID_ARG;
    DwPlan p;
    if (!dw_plan(NI, C, Hi, Wi, stride, p) || (FORM == 2 && C % 8 != 0)) return EAS_ERR_UNSUPPORTED;
    if (FORM == 2 && ((uintptr_t)x & 15)) return EAS_ERR_INVALID_ARG;
    if (((uintptr_t)x | (uintptr_t)gy | (uintptr_t)ws | (uintptr_t)gw) & 3) return EAS_ERR_INVALID_ARG;
    int tpb, nparts;
    dw_wgrad_split(p, tpb, nparts);
    const DwGeom d = dw_geom(p);
    const dim3 grid(nparts, p.G), block(EAS_BLOCK);
    const size_t lds = dw_lds_bytes(p, false);
    const bool vec = FORM == 1 && Wi % 4 == 0 && ((uintptr_t)x & 15) == 0;
    hipStream_t st = eas_s(stream);
    EAS_CLEAR_ERR();
    if (stride == 1) {
        if (vec) EAS_LAUNCH((dwconv_wgrad_kernel<FORM, 1, true>), grid, block, lds, st, x, gy, ws, d, p.nb, tpb, nparts);
        else EAS_LAUNCH((dwconv_wgrad_kernel<FORM, 1, false>), grid, block, lds, st, x, gy, ws, d, p.nb, tpb, nparts);
    } else {
        if (vec) EAS_LAUNCH((dwconv_wgrad_kernel<FORM, 2, true>), grid, block, lds, st, x, gy, ws, d, p.nb, tpb, nparts);
        else EAS_LAUNCH((dwconv_wgrad_kernel<FORM, 2, false>), grid, block, lds, st, x, gy, ws, d, p.nb, tpb, nparts);
    }
    EAS_CHECK_LAUNCH();
    EAS_LAUNCH(dwconv_wgrad_reduce_kernel, dim3((C * 9 + DW_NW - 1) / DW_NW), block, 0, st, (const float*)ws, gw, C, nparts);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

}  // namespace

extern "C" {

int eas_dwconv_supported(int NI, int C, int Hi, int Wi, int stride, int x_form) {
    DwPlan p;
    if (x_form != 1 && x_form != 2) return 0;
    if (x_form == 2 && C % 8 != 0) return 0;
    return dw_plan(NI, C, Hi, Wi, stride, p) ? 1 : 0;
}

int eas_dwconv_fwd_stats_blocks(int NI, int C, int Hi, int Wi, int stride, int x_form) {
    DwPlan p;
    if (!eas_dwconv_supported(NI, C, Hi, Wi, stride, x_form) || !dw_plan(NI, C, Hi, Wi, stride, p)) return 0;
    return p.nb;
}

int eas_dwconv_fwd(const float* x, const float* w, const float* bias, float* y, int NI, int C, int Hi, int Wi, int stride, double* stats, int nb,
                   eas_stream_t stream) {
    if ((uintptr_t)x & 3) return EAS_ERR_INVALID_ARG;
    return dw_fwd_entry<1>(x, w, bias, y, NI, C, Hi, Wi, stride, stats, nb, stream);
}

int eas_dwconv_fwd_planes(const void* x_planes, const float* w, const float* bias, float* y, int NI, int C, int Hi, int Wi, int stride,
                          double* stats, int nb, eas_stream_t stream) {
    return dw_fwd_entry<2>(x_planes, w, bias, y, NI, C, Hi, Wi, stride, stats, nb, stream);
}

int eas_dwconv_dgrad(const float* grad_y, const float* w, float* grad_x, int NI, int C, int Hi, int Wi, int stride, eas_stream_t stream) {
    if (!grad_y || !w || !grad_x) return EAS_ERR_INVALID_ARG;
    if (((uintptr_t)grad_y | (uintptr_t)w | (uintptr_t)grad_x) & 3) return EAS_ERR_INVALID_ARG;
    DwPlan p;
    if (!dw_plan(NI, C, Hi, Wi, stride, p)) return EAS_ERR_UNSUPPORTED;
    if (stride == 1) return dw_launch_fwd<1, true>(grad_y, w, nullptr, grad_x, p, nullptr, eas_s(stream));
    if (C > 65535) return EAS_ERR_UNSUPPORTED;
    const int Q = ((Hi + 1) / 2) * ((Wi + 1) / 2);
    const bool pair = (Wi & 1) == 0;
    if (pair && ((uintptr_t)grad_x & 7)) return EAS_ERR_INVALID_ARG;
    int64_t chunks = ((int64_t)NI * Q + 4 * EAS_BLOCK - 1) / (4 * EAS_BLOCK);          // ~4 quads per thread
    const int64_t cap = 8192 / C > 1 ? 8192 / C : 1;
    if (chunks > cap) chunks = cap;
    EAS_CLEAR_ERR();
    EAS_LAUNCH(dwconv_dgrad_s2_kernel, dim3((unsigned)chunks, C), dim3(EAS_BLOCK), 0, eas_s(stream), grad_y, w, grad_x, NI, C, Hi, Wi, p.Ho, p.Wo);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

int64_t eas_dwconv_wgrad_workspace_floats(int NI, int C, int Hi, int Wi, int stride) {
    DwPlan p;
    if (!dw_plan(NI, C, Hi, Wi, stride, p)) return 0;
    int tpb, nparts;
    dw_wgrad_split(p, tpb, nparts);
    return (int64_t)C * nparts * 9;
}

int eas_dwconv_wgrad(const float* x, const float* grad_y, float* workspace, float* grad_w, int NI, int C, int Hi, int Wi, int stride,
                     eas_stream_t stream) {
    return dw_wgrad_entry<1>(x, grad_y, workspace, grad_w, NI, C, Hi, Wi, stride, stream);
}

int eas_dwconv_wgrad_planes(const void* x_planes, const float* grad_y, float* workspace, float* grad_w, int NI, int C, int Hi, int Wi, int stride,
                            eas_stream_t stream) {
    return dw_wgrad_entry<2>(x_planes, grad_y, workspace, grad_w, NI, C, Hi, Wi, stride, stream);
}

}  // extern "C"
