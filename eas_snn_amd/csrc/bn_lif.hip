// K4 (second half): BatchNorm(step_mode='m') + multi-step LIF fused, forward and backward.
//
// Data: y = conv output, [T][N][C][HW] fp32.  BN statistics couple all of T*N*HW per channel, so
// training needs a statistics pass before the fused apply pass (SURVEY "Hard parts").
// Work decomposition for every kernel here: blockIdx.y = channel c, blockIdx.x = chunk of that
// channel's N*HW/4 float4 groups.  Per-channel constants (scale, shift, means) are block-uniform,
// reductions are per block -> per (channel, chunk) partial -> fixed-order finalize (deterministic).
// Reads are contiguous runs of HW floats (one (n,c) plane), 16 B per lane.
//
// HBM traffic per neuron-step: stats 4 B (read y); fwd 8 B (read y, write s);
// bwd 20 B (pass 1 reads y, grad_s; pass 2 reads them again and writes grad_y).  Only y is kept
// for backward: h_t is recomputed in registers from y (T <= 8).
//
// Shared with bn_act.hip through eas_common.h: the chunk plan (bn_pick_chunks, EAS_BN_MAX_CHUNKS), the pending-statistics rule (bn_fin_from),
// mean / invstd from totals (bn_from_totals), and the BatchNorm backward skeleton -- chunk partials -> means (bn_bwd_means), one-pass block
// totals (eas_block_totals), the apply expression (bn_bwd_apply).  The scalar parameter gradients' final stage (eas_lif_scalar_grads) and
// the flag dispatch of the forward (eas_lif_dispatch) are the ones lif.hip uses.
#include <stdlib.h>
#include <string.h>

#include "bn_lif_policy.h"
#include "eas_common.h"

namespace {

constexpr int NW = EAS_BLOCK / EAS_WAVE;

// ------------------------------------------------------------------------------------------------ stats
__global__ __launch_bounds__(EAS_BLOCK) void bn_stats_partial(const float* __restrict__ y, int TN, int C, int HW,
                                                              double* __restrict__ part, int Cy) {
    __shared__ double red[NW];
    const int c = blockIdx.y;
    const int hw4 = HW / EAS_VEC;
    const int64_t groups = (int64_t)TN * hw4;
    double s = 0.0, ss = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    GroupWalk gw((int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride, hw4);
    int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    // two groups in flight per thread (both loads issued before the double-precision accumulation of either); the order in
    // which a thread adds its groups is unchanged
    for (; g + stride < groups; g += 2 * stride) {
        const float4 v0 = reinterpret_cast<const float4*>(y + (((int64_t)gw.n * Cy + c) * (int64_t)HW))[gw.q];
        gw.next();
        const float4 v1 = reinterpret_cast<const float4*>(y + (((int64_t)gw.n * Cy + c) * (int64_t)HW))[gw.q];
        gw.next();
        s += (double)v0.x + (double)v0.y + (double)v0.z + (double)v0.w;
        ss += (double)v0.x * v0.x + (double)v0.y * v0.y + (double)v0.z * v0.z + (double)v0.w * v0.w;
        s += (double)v1.x + (double)v1.y + (double)v1.z + (double)v1.w;
        ss += (double)v1.x * v1.x + (double)v1.y * v1.y + (double)v1.z * v1.z + (double)v1.w * v1.w;
    }
    if (g < groups) {
        const float4 v = reinterpret_cast<const float4*>(y + (((int64_t)gw.n * Cy + c) * (int64_t)HW))[gw.q];
        s += (double)v.x + (double)v.y + (double)v.z + (double)v.w;
        ss += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
    }
    const double ts = eas_block_sum<double, NW>(s, red);
    const double tss = eas_block_sum<double, NW>(ss, red);
    if (threadIdx.x == 0) {
        part[((int64_t)c * EAS_BN_MAX_CHUNKS + blockIdx.x) * 2 + 0] = ts;
        part[((int64_t)c * EAS_BN_MAX_CHUNKS + blockIdx.x) * 2 + 1] = tss;
    }
}

// scalar path for HW % 4 != 0
__global__ __launch_bounds__(EAS_BLOCK) void bn_stats_partial_scalar(const float* __restrict__ y, int TN, int C, int HW,
                                                                     double* __restrict__ part) {
    __shared__ double red[NW];
    const int c = blockIdx.y;
    const int64_t groups = (int64_t)TN * HW;
    double s = 0.0, ss = 0.0;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t n = g / HW;
        const int q = (int)(g - n * HW);
        const float v = y[(n * C + c) * (int64_t)HW + q];
        s += v;
        ss += (double)v * v;
    }
    const double ts = eas_block_sum<double, NW>(s, red);
    const double tss = eas_block_sum<double, NW>(ss, red);
    if (threadIdx.x == 0) {
        part[((int64_t)c * EAS_BN_MAX_CHUNKS + blockIdx.x) * 2 + 0] = ts;
        part[((int64_t)c * EAS_BN_MAX_CHUNKS + blockIdx.x) * 2 + 1] = tss;
    }
}

// one wave per channel: the chunk partials of bn_stats_partial -> mean / invstd and the running statistics (identical replicas leave
// mean / var unchanged, only the sample count grows)
__global__ __launch_bounds__(EAS_WAVE) void bn_stats_finalize(BnFin fin) {
    const int c = blockIdx.x;
    double s, ss;
    bn_wave_partials<2>(fin.part, (int64_t)c * fin.pitch, fin.nchunks, s, ss);
    float mu, istd;
    if (threadIdx.x == 0) bn_from_totals(fin, c, s, ss, true, mu, istd);
}

struct BnLifOut {
    const float* residual;   // nullable [T][N][C][HW]: spikes_out = spikes + residual (SEW shortcut, network_blocks.py:99-104)
    int out_ctot;            // 0: dense; else spikes are channels of a [T][N][out_ctot][HW] tensor (pointer already at channel 0 of the slice)
    int y_ctot;              // 0: dense; else y is such a channel slice of a [T][N][y_ctot][HW] tensor (one convolution feeding two BN+LIF layers)
};

// Spike planes (eas_hip.h "spike planes"): the output values (0/1 spikes, SEW sums: exact in bf16) as bf16 in blocks of 8 channels,
// [T*N][C/8][HW][8] -- the layout in which every consumer's matrix-core fragment (8 consecutive input channels of one pixel) is ONE
// 16-byte load, at half the bytes of fp32.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// ------------------------------------------------------------------------------------------------ forward
template <int T_, bool HARD, bool DI, bool STRICT>
__global__ __launch_bounds__(EAS_BLOCK) void bn_lif_fwd_kernel(const float* __restrict__ y, const float* __restrict__ mean,
                                                               const float* __restrict__ invstd,
                                                               const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, const float* v_in, float* v_out,
                                                               EasLifParams p, float* __restrict__ spikes,
                                                               float* __restrict__ mean_out, int N, int C, int HW, int bcast,
                                                               BnFin fin, BnLifOut ox) {
    __shared__ float st[2];
    const int c = blockIdx.z * 8 + blockIdx.x;      // EAS_CHAN_GRID: the chunks of a channel share an XCD
    if (c >= C) return;
    const int chunk = blockIdx.y, nchunks_g = gridDim.y;
    float mu, istd;
    if (fin.part) {
        bn_finalize_in_block(fin, c, st, mu, istd, chunk == 0);
    } else {
        mu = mean[c];
        istd = invstd[c];
    }
    const float scale = gamma[c] * istd;
    const float shift = beta[c] - mu * scale;
    const int64_t Mo = ox.out_ctot ? (int64_t)N * ox.out_ctot * HW : (int64_t)N * C * HW;
    const float k = eas_lif_k(p);
    const float omk = 1.0f - k;
    const int hw4 = HW / EAS_VEC;
    const int64_t groups = (int64_t)N * hw4;
    const int64_t M = (int64_t)N * C * HW;
    const int Cy = ox.y_ctot ? ox.y_ctot : C;
    const int64_t yts = bcast ? 0 : (int64_t)N * Cy * HW;       // T identical input frames: one plane stands for all steps
    GroupWalk gw((int64_t)chunk * blockDim.x + threadIdx.x, (int64_t)nchunks_g * blockDim.x, hw4);
    for (int64_t g = (int64_t)chunk * blockDim.x + threadIdx.x; g < groups; g += (int64_t)nchunks_g * blockDim.x, gw.next()) {
        const int64_t n = gw.n;
        const int q = gw.q;
        const int64_t base = (n * C + c) * (int64_t)HW + (int64_t)q * EAS_VEC;
        float4 ys[T_];
        const int64_t ybase = (n * Cy + c) * (int64_t)HW + (int64_t)q * EAS_VEC;
#pragma unroll
        for (int t = 0; t < T_; ++t) ys[t] = *reinterpret_cast<const float4*>(y + (int64_t)t * yts + ybase);
        const float vr0 = HARD ? p.v_reset : 0.0f;
        float4 v = v_in ? *reinterpret_cast<const float4*>(v_in + base) : make_float4(vr0, vr0, vr0, vr0);
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int t = 0; t < T_; ++t) {
            float4 h, s;
            eas_lif_step<HARD, DI, STRICT>(v.x, fmaf(ys[t].x, scale, shift), k, omk, p.v_th, p.v_reset, h.x, s.x);
            eas_lif_step<HARD, DI, STRICT>(v.y, fmaf(ys[t].y, scale, shift), k, omk, p.v_th, p.v_reset, h.y, s.y);
            eas_lif_step<HARD, DI, STRICT>(v.z, fmaf(ys[t].z, scale, shift), k, omk, p.v_th, p.v_reset, h.z, s.z);
            eas_lif_step<HARD, DI, STRICT>(v.w, fmaf(ys[t].w, scale, shift), k, omk, p.v_th, p.v_reset, h.w, s.w);
            acc.x += s.x; acc.y += s.y; acc.z += s.z; acc.w += s.w;
            if (ox.residual) {
                const float4 r = *reinterpret_cast<const float4*>(ox.residual + (int64_t)t * M + base);
                s.x += r.x; s.y += r.y; s.z += r.z; s.w += r.w;
            }
            const int64_t obase = ox.out_ctot ? (n * ox.out_ctot + c) * (int64_t)HW + (int64_t)q * EAS_VEC : base;
            *reinterpret_cast<float4*>(spikes + (int64_t)t * Mo + obase) = s;
        }
        if (v_out) *reinterpret_cast<float4*>(v_out + base) = v;
        if (mean_out) {
            const float Tf = (float)T_;   // sum / T, like ATen's mean
            *reinterpret_cast<float4*>(mean_out + base) = make_float4(acc.x / Tf, acc.y / Tf, acc.z / Tf, acc.w / Tf);
        }
    }
}

// mean / invstd (and the running statistics) of every channel from the chunk partials, one block per channel, in the summation order of
// bn_finalize_in_block: the statistics the plane-writing kernel below reads are bit-identical to the ones the fp32 kernel forms itself.
__global__ __launch_bounds__(EAS_BLOCK) void bn_finalize_kernel(BnFin fin) {
    __shared__ float st[2];
    float mu, istd;
    bn_finalize_in_block(fin, (int)blockIdx.x, st, mu, istd, true);
}

// The same layer writing its output as spike planes.  A thread owns the 8 channels of one group for PV consecutive pixels of an image
// (PV = 1 is what runs): 8 x T loads of PV floats (each channel row is contiguous over the lanes), the neuron over T in registers, and
// per step ONE 16-byte store per pixel.  blockIdx -> (channel group, chunk of the group's N * HW / PV pixel groups).  residual: planes as well.
template <int T_, bool HARD, bool DI, bool STRICT, int PV>
__global__ __launch_bounds__(EAS_BLOCK) void bn_lif_fwd_sp_kernel(const float* __restrict__ y, const float* __restrict__ mean,
                                                                  const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, const float* v_in, float* v_out,
                                                                  EasLifParams p, bf16x8* __restrict__ planes, const bf16x8* __restrict__ res_planes,
                                                                  float* __restrict__ mean_out, int N, int C, int HW, int bcast, int y_ctot,
                                                                  int out_groups_tot, int res_groups_tot) {
    typedef float vecp __attribute__((ext_vector_type(PV)));
    const int grp = blockIdx.z * 8 + blockIdx.x;
    const int G = C / 8;
    if (grp >= G) return;
    const int chunk = blockIdx.y, nchunks_g = gridDim.y;
    float scale[8], shift[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = 8 * grp + j;
        scale[j] = gamma[c] * invstd[c];
        shift[j] = beta[c] - mean[c] * scale[j];
    }
    const float k = eas_lif_k(p);
    const float omk = 1.0f - k;
    const int hwp = HW / PV;
    const int64_t groups = (int64_t)N * hwp;
    const int Cy = y_ctot ? y_ctot : C;
    const int64_t yts = bcast ? 0 : (int64_t)N * Cy * HW;
    const float vr0 = HARD ? p.v_reset : 0.0f;
    const float Tf = (float)T_;
    GroupWalk gw((int64_t)chunk * blockDim.x + threadIdx.x, (int64_t)nchunks_g * blockDim.x, hwp);
    for (int64_t g = (int64_t)chunk * blockDim.x + threadIdx.x; g < groups; g += (int64_t)nchunks_g * blockDim.x, gw.next()) {
        const int64_t n = gw.n;
        const int q = gw.q;
        vecp ys[8][T_];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int64_t yb = (n * Cy + 8 * grp + j) * (int64_t)HW + (int64_t)q * PV;
#pragma unroll
            for (int t = 0; t < T_; ++t) ys[j][t] = *reinterpret_cast<const vecp*>(y + (int64_t)t * yts + yb);
        }
        float v[8][PV], acc[8][PV];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            vecp v0;
            if (v_in) v0 = *reinterpret_cast<const vecp*>(v_in + (n * C + 8 * grp + j) * (int64_t)HW + (int64_t)q * PV);
#pragma unroll
            for (int e = 0; e < PV; ++e) { v[j][e] = v_in ? v0[e] : vr0; acc[j][e] = 0.f; }
        }
#pragma unroll
        for (int t = 0; t < T_; ++t) {
            bf16x8 rp[PV];
            if (res_planes) {
#pragma unroll
                for (int e = 0; e < PV; ++e) rp[e] = res_planes[(((int64_t)t * N + n) * res_groups_tot + grp) * (int64_t)HW + (int64_t)q * PV + e];
            }
#pragma unroll
            for (int e = 0; e < PV; ++e) {
                bf16x8 o;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float h, s;
                    eas_lif_step<HARD, DI, STRICT>(v[j][e], fmaf(ys[j][t][e], scale[j], shift[j]), k, omk, p.v_th, p.v_reset, h, s);
                    acc[j][e] += s;
                    if (res_planes) s += (float)rp[e][j];
                    o[j] = (__bf16)s;
                }
                planes[(((int64_t)t * N + n) * out_groups_tot + grp) * (int64_t)HW + (int64_t)q * PV + e] = o;
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int64_t base = (n * C + 8 * grp + j) * (int64_t)HW + (int64_t)q * PV;
            if (v_out) {
                vecp o;
#pragma unroll
                for (int e = 0; e < PV; ++e) o[e] = v[j][e];
                *reinterpret_cast<vecp*>(v_out + base) = o;
            }
            if (mean_out) {
                vecp o;
#pragma unroll
                for (int e = 0; e < PV; ++e) o[e] = acc[j][e] / Tf;
                *reinterpret_cast<vecp*>(mean_out + base) = o;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ backward
// Recompute h_t from y, then walk the LIF backward: dz[t] = dL/dz_t (z = BN output), dk += dL/dk.
// POL (bn_lif_policy.h): a fast policy fixes the surrogate and the reset form at compile time (detach / sg_id are then not read); the
// generic policy takes them from the arguments at every step.
template <int T_, bool HARD, bool DI, bool STRICT, class POL>
__device__ __forceinline__ void recompute_dz(const float (&yv)[T_], const float (&gs)[T_], float v0, float scale,
                                             float shift, float k, float omk, const EasLifParams& p, bool detach,
                                             int sg_id, float alpha, float (&dz)[T_], float& dk, float& da) {
    float h[T_], vprev[T_], z[T_];
    float v = v0;
#pragma unroll
    for (int t = 0; t < T_; ++t) {
        float s;
        vprev[t] = v;
        z[t] = fmaf(yv[t], scale, shift);
        eas_lif_step<HARD, DI, STRICT>(v, z[t], k, omk, p.v_th, p.v_reset, h[t], s);
    }
    float gv = 0.f;
#pragma unroll
    for (int t = T_ - 1; t >= 0; --t) {
        float dkt, gx;
        if constexpr (POL::fast)
            eas_lif_step_bwd_ct<HARD, DI, STRICT, POL::sg, POL::detach>(gs[t], gv, h[t], vprev[t], z[t], k, omk, p.v_th, p.v_reset, alpha, dkt,
                                                                        gx, da);
        else
            eas_lif_step_bwd<HARD, DI, STRICT>(gs[t], gv, h[t], vprev[t], z[t], k, omk, p.v_th, p.v_reset, detach, sg_id, alpha, dkt, gx, da);
        dz[t] = gx;
        dk += dkt;
    }
}

// A fast instance (POL::fast) is launched for plain operands only (bwd_select): grad_s present, no grad_mean, no v_init, no broadcast input
// frame.  Its loop has no launch-uniform branch: the optional operands are compiled out and a channel slice (gs_ctot / y_ctot) is addressed
// through the channel count like a dense tensor.  Per element the expressions of the generic body (0 + grad_s included: it turns -0 into
// +0), so both forms give the same bits.
template <int T_, bool HARD, bool DI, bool STRICT, bool APPLY, class POL>
__global__ __launch_bounds__(EAS_BLOCK) void bn_lif_bwd_kernel(
    const float* __restrict__ grad_s, const float* __restrict__ grad_mean, const float* __restrict__ y,
    const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ v_init, EasLifParams p, int sg_id, float alpha,
    int batch_stats, double* __restrict__ part, int nchunks, float* __restrict__ grad_y, float* __restrict__ grad_gamma,
    float* __restrict__ grad_beta, float* __restrict__ grad_w, int N, int C, int HW, int bcast, int gs_ctot, int y_ctot,
    const float* __restrict__ alpha_dev, float* __restrict__ grad_alpha, int c_begin, int c_end, int finalize) {
    __shared__ double red[NW];
    __shared__ float bc[2];
    constexpr bool FAST = POL::fast;
    if (FAST) { bcast = 0; sg_id = POL::sg; }
    if (alpha_dev) alpha = fabsf(*alpha_dev);    // learnable slope (EAS_SG_PATAN)
    // channels [c_begin, c_end) of the layer: a launch pair (sums, apply) may cover a channel group only, so that the apply pass finds the
    // group's y / grad_s still in the Infinity Cache (launch_bwd_t)
    const int c = c_begin + blockIdx.z * 8 + blockIdx.x;      // EAS_CHAN_GRID: the chunks of a channel share an XCD
    if (c >= c_end) return;
    const int chunk = blockIdx.y, nchunks_g = gridDim.y;
    const float mu = mean[c], istd = invstd[c];
    const float scale = gamma[c] * istd;
    const float shift = beta[c] - mu * scale;
    const float k = eas_lif_k(p);
    const float omk = 1.0f - k;
    const bool detach = (p.flags & EAS_LIF_DETACH_RESET) != 0;
    const int hw4 = HW / EAS_VEC;
    const int64_t groups = (int64_t)N * hw4;
    const int64_t M = (int64_t)N * C * HW;
    const float invT = 1.0f / (float)T_;
    const int Cy = y_ctot ? y_ctot : C;                               // y / grad_y may be channel slices of a wider tensor
    const int64_t My = (int64_t)N * Cy * HW;
    const int64_t yts = bcast ? 0 : My;
    const int64_t Mg = gs_ctot ? (int64_t)N * gs_ctot * HW : M;      // grad_s may be a channel slice of a wider tensor
    const int Cg = gs_ctot ? gs_ctot : C;
    float m1 = 0.f, m2 = 0.f;
    if (APPLY) bn_bwd_means<4>(part, c, nchunks, (double)T_ * N * HW, chunk, batch_stats, grad_beta, grad_gamma, bc, m1, m2);
    float s1 = 0.f, s2 = 0.f, dk = 0.f, da = 0.f;
    GroupWalk gw((int64_t)chunk * blockDim.x + threadIdx.x, (int64_t)nchunks_g * blockDim.x, hw4);
    for (int64_t g = (int64_t)chunk * blockDim.x + threadIdx.x; g < groups; g += (int64_t)nchunks_g * blockDim.x, gw.next()) {
        const int64_t n = gw.n;
        const int q = gw.q;
        const int64_t base = (n * C + c) * (int64_t)HW + (int64_t)q * EAS_VEC;
        float4 ys[T_], gsv[T_];
        const int64_t ybase = (n * Cy + c) * (int64_t)HW + (int64_t)q * EAS_VEC;
#pragma unroll
        for (int t = 0; t < T_; ++t) ys[t] = *reinterpret_cast<const float4*>(y + (int64_t)t * yts + ybase);
        float4 gm = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!FAST && grad_mean) {
            gm = *reinterpret_cast<const float4*>(grad_mean + base);
            gm.x *= invT; gm.y *= invT; gm.z *= invT; gm.w *= invT;
        }
#pragma unroll
        for (int t = 0; t < T_; ++t) {
            gsv[t] = gm;
            if (FAST || grad_s) {
                const int64_t gbase = FAST ? (n * Cg + c) * (int64_t)HW + (int64_t)q * EAS_VEC
                                           : (gs_ctot ? (n * gs_ctot + c) * (int64_t)HW + (int64_t)q * EAS_VEC : base);
                const float4 g4 = *reinterpret_cast<const float4*>(grad_s + (int64_t)t * Mg + gbase);
                gsv[t].x += g4.x; gsv[t].y += g4.y; gsv[t].z += g4.z; gsv[t].w += g4.w;
            }
        }
        const float vr0 = HARD ? p.v_reset : 0.0f;
        float4 v0 = make_float4(vr0, vr0, vr0, vr0);
        if (!FAST && v_init) v0 = *reinterpret_cast<const float4*>(v_init + base);
        float4 outv[T_];
#pragma unroll
        for (int e = 0; e < EAS_VEC; ++e) {
            float yv[T_], gs[T_], dz[T_];
#pragma unroll
            for (int t = 0; t < T_; ++t) {
                yv[t] = reinterpret_cast<const float*>(&ys[t])[e];
                gs[t] = reinterpret_cast<const float*>(&gsv[t])[e];
            }
            const float v0e = reinterpret_cast<const float*>(&v0)[e];
            float dke = 0.f;
            recompute_dz<T_, HARD, DI, STRICT, POL>(yv, gs, v0e, scale, shift, k, omk, p, detach, sg_id, alpha, dz, dke, da);
#pragma unroll
            for (int t = 0; t < T_; ++t) {
                const float xhat = bn_xhat(yv[t], mu, istd);
                if (APPLY) {
                    reinterpret_cast<float*>(&outv[t])[e] = bn_bwd_apply(scale, dz[t], xhat, m1, m2);
                } else {
                    s1 += dz[t];
                    s2 += dz[t] * xhat;
                }
            }
            dk += dke;
        }
        if (APPLY) {
            if (bcast) {                            // the T steps share one input plane: its gradient is their sum
                float4 a = outv[0];
#pragma unroll
                for (int t = 1; t < T_; ++t) { a.x += outv[t].x; a.y += outv[t].y; a.z += outv[t].z; a.w += outv[t].w; }
                *reinterpret_cast<float4*>(grad_y + ybase) = a;
            } else {
#pragma unroll
                for (int t = 0; t < T_; ++t) *reinterpret_cast<float4*>(grad_y + (int64_t)t * My + ybase) = outv[t];
            }
        }
    }
    if (APPLY && finalize && chunk == 0 && c == c_begin) {
        // dL/dw of the (scalar) PLIF decay and dL/dalpha of the learnable surrogate slope: fixed-order sums of every (channel, chunk) partial
        // of pass 1 (slots 2 / 3), by one block
        auto slot = [&](int i, int k_) {
            const int cc = i / nchunks, j = i - cc * nchunks;
            return part[((int64_t)cc * EAS_BN_MAX_CHUNKS + j) * 4 + k_];
        };
        eas_lif_scalar_grads(C * nchunks, [&](int i) { return slot(i, 2); }, [&](int i) { return slot(i, 3); }, p.w_logit, alpha_dev, grad_w,
                             grad_alpha, red);
    }
    if (!APPLY) {
        const double t1 = eas_block_sum<double, NW>((double)s1, red);
        const double t2 = eas_block_sum<double, NW>((double)s2, red);
        const double t3 = eas_block_sum<double, NW>((double)dk, red);
        double t4 = 0.0;
        if (sg_id == EAS_SG_PATAN) t4 = eas_block_sum<double, NW>((double)da, red);
        if (threadIdx.x == 0) {
            double* o = part + ((int64_t)c * EAS_BN_MAX_CHUNKS + chunk) * 4;
            o[0] = t1; o[1] = t2; o[2] = t3; o[3] = t4;
        }
    }
}

// One pass for the layers whose channel fits the registers of one block (8x10 maps at batch 64: 1280 float4 groups per channel and time
// step): one block per channel keeps y and grad_s of the channel in registers, sums dz and dz * xhat over the block (fixed order), and
// applies the BatchNorm backward from the registers -- 12 B per neuron-step instead of 20 and one real launch instead of two of ~17 us
// each (these layers are bound by the launches, not by their 30 MB).  Per element the arithmetic of the two-pass kernels; the per-channel
// dL/dk / dL/dalpha partials go to the same workspace slots (chunk 0) and a one-block kernel adds them over the channels in fixed order.
// (first half.)
template <int T_, bool HARD, bool DI, bool STRICT, int NT_, int GPT, class POL>
__global__ __launch_bounds__(NT_) void bn_lif_bwd_small_kernel(
    const float* __restrict__ grad_s, const float* __restrict__ grad_mean, const float* __restrict__ y,
    const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ v_init, EasLifParams p, int sg_id, float alpha,
    int batch_stats, double* __restrict__ part, float* __restrict__ grad_y, float* __restrict__ grad_gamma,
    float* __restrict__ grad_beta, int N, int C, int HW, int gs_ctot, int y_ctot, const float* __restrict__ alpha_dev) {
    constexpr int NWV = NT_ / EAS_WAVE;
    __shared__ double red[4][NWV];
    __shared__ float bc[2];
    // (a fast instance of this kernel takes every operand form: the optional operands are read once per thread in front of the two
    // passes, not inside them)
    if (POL::fast) sg_id = POL::sg;
    if (alpha_dev) alpha = fabsf(*alpha_dev);
    const int c = blockIdx.x;
    const float mu = mean[c], istd = invstd[c];
    const float scale = gamma[c] * istd;
    const float shift = beta[c] - mu * scale;
    const float k = eas_lif_k(p);
    const float omk = 1.0f - k;
    const bool detach = (p.flags & EAS_LIF_DETACH_RESET) != 0;
    const int hw4 = HW / EAS_VEC;
    const int groups = N * hw4;
    const int64_t M = (int64_t)N * C * HW;
    const int Cy = y_ctot ? y_ctot : C;
    const int64_t My = (int64_t)N * Cy * HW;
    const int64_t Mg = gs_ctot ? (int64_t)N * gs_ctot * HW : M;
    const float invT = 1.0f / (float)T_;
    float4 ys[GPT][T_], gsv[GPT][T_], v0[GPT];
    int64_t ybase[GPT];
#pragma unroll
    for (int i = 0; i < GPT; ++i) {
        const int g = threadIdx.x + i * NT_;
        const int gg = g < groups ? g : groups - 1;          // surplus threads re-read the last group (their results are not used)
        const int n = gg / hw4, q = gg - n * hw4;
        const int64_t base = ((int64_t)n * C + c) * (int64_t)HW + (int64_t)q * EAS_VEC;
        ybase[i] = ((int64_t)n * Cy + c) * (int64_t)HW + (int64_t)q * EAS_VEC;
#pragma unroll
        for (int t = 0; t < T_; ++t) ys[i][t] = *reinterpret_cast<const float4*>(y + (int64_t)t * My + ybase[i]);
        float4 gm = make_float4(0.f, 0.f, 0.f, 0.f);
        if (grad_mean) {
            gm = *reinterpret_cast<const float4*>(grad_mean + base);
            gm.x *= invT; gm.y *= invT; gm.z *= invT; gm.w *= invT;
        }
#pragma unroll
        for (int t = 0; t < T_; ++t) {
            gsv[i][t] = gm;
            if (grad_s) {
                const int64_t gbase = gs_ctot ? ((int64_t)n * gs_ctot + c) * (int64_t)HW + (int64_t)q * EAS_VEC : base;
                const float4 g4 = *reinterpret_cast<const float4*>(grad_s + (int64_t)t * Mg + gbase);
                gsv[i][t].x += g4.x; gsv[i][t].y += g4.y; gsv[i][t].z += g4.z; gsv[i][t].w += g4.w;
            }
        }
        const float vr0 = HARD ? p.v_reset : 0.0f;
        v0[i] = make_float4(vr0, vr0, vr0, vr0);
        if (v_init) v0[i] = *reinterpret_cast<const float4*>(v_init + base);
    }
    // pass 1 (registers): the channel's sums
    float sum[4] = {0.f, 0.f, 0.f, 0.f};      // dz, dz * xhat, dL/dk, dL/d|alpha|
#pragma unroll
    for (int i = 0; i < GPT; ++i) {
        const bool live = threadIdx.x + i * NT_ < groups;
#pragma unroll
        for (int e = 0; e < EAS_VEC; ++e) {
            float yv[T_], gs[T_], dz[T_];
#pragma unroll
            for (int t = 0; t < T_; ++t) {
                yv[t] = reinterpret_cast<const float*>(&ys[i][t])[e];
                gs[t] = reinterpret_cast<const float*>(&gsv[i][t])[e];
            }
            float dke = 0.f, dae = 0.f;
            recompute_dz<T_, HARD, DI, STRICT, POL>(yv, gs, reinterpret_cast<const float*>(&v0[i])[e], scale, shift, k, omk, p, detach, sg_id, alpha, dz, dke, dae);
            if (live) {
#pragma unroll
                for (int t = 0; t < T_; ++t) {
                    sum[0] += dz[t];
                    sum[1] += dz[t] * bn_xhat(yv[t], mu, istd);
                }
                sum[2] += dke;
                sum[3] += dae;
            }
        }
    }
    double t[4];
    eas_block_totals<NWV, 4>(sum, red, t);
    if (threadIdx.x == 0) {
        bn_bwd_publish(t[0], t[1], (double)T_ * N * HW, true, c, grad_beta, grad_gamma, bc);
        double* o = part + ((int64_t)c * EAS_BN_MAX_CHUNKS) * 4;      // chunk 0 of the two-pass layout: read by bn_lif_bwd_scalars_kernel
        o[0] = t[0]; o[1] = t[1]; o[2] = t[2]; o[3] = sg_id == EAS_SG_PATAN ? t[3] : 0.0;
    }
    __syncthreads();
    const float m1 = batch_stats ? bc[0] : 0.f, m2 = batch_stats ? bc[1] : 0.f;
    // pass 2 (registers): the neuron again, grad_y
#pragma unroll
    for (int i = 0; i < GPT; ++i) {
        if (threadIdx.x + i * NT_ >= groups) continue;
        float4 outv[T_];
#pragma unroll
        for (int e = 0; e < EAS_VEC; ++e) {
            float yv[T_], gs[T_], dz[T_];
#pragma unroll
            for (int t = 0; t < T_; ++t) {
                yv[t] = reinterpret_cast<const float*>(&ys[i][t])[e];
                gs[t] = reinterpret_cast<const float*>(&gsv[i][t])[e];
            }
            float dke = 0.f, dae = 0.f;
            recompute_dz<T_, HARD, DI, STRICT, POL>(yv, gs, reinterpret_cast<const float*>(&v0[i])[e], scale, shift, k, omk, p, detach, sg_id, alpha, dz, dke, dae);
#pragma unroll
            for (int t = 0; t < T_; ++t) reinterpret_cast<float*>(&outv[t])[e] = bn_bwd_apply(scale, dz[t], bn_xhat(yv[t], mu, istd), m1, m2);
        }
#pragma unroll
        for (int t = 0; t < T_; ++t) *reinterpret_cast<float4*>(grad_y + (int64_t)t * My + ybase[i]) = outv[t];
    }
}

// dL/dw of the scalar PLIF decay and dL/dalpha of a learnable surrogate slope from the per-channel partials of bn_lif_bwd_small_kernel
// (slot 2 / 3 of chunk 0), added over the channels in fixed order by one block -- what the apply pass of the two-pass form does at its end
__global__ __launch_bounds__(EAS_BLOCK) void bn_lif_bwd_scalars_kernel(const double* __restrict__ part, int C, EasLifParams p, float* __restrict__ grad_w,
                                                                       const float* __restrict__ alpha_dev, float* __restrict__ grad_alpha) {
    __shared__ double red[NW];
    auto slot = [&](int i, int k_) { return part[((int64_t)i * EAS_BN_MAX_CHUNKS) * 4 + k_]; };
    eas_lif_scalar_grads(C, [&](int i) { return slot(i, 2); }, [&](int i) { return slot(i, 3); }, p.w_logit, alpha_dev, grad_w, grad_alpha, red);
}

template <int T_, bool HARD, bool DI, bool STRICT>
int launch_fwd_t(const float* y, const float* mean, const float* invstd, const float* gamma, const float* beta,
                 const float* v_in, float* v_out, EasLifParams p, float* spikes, float* mean_out, int N, int C, int HW,
                 int bcast, const BnFin& fin, const BnLifOut& ox, bf16x8* planes, const bf16x8* res_planes, int out_groups, int res_groups,
                 hipStream_t st) {
    if (planes) {
        // spike planes out: the statistics are finalized by their own small launch (a block of this kernel owns 8 channels: finalizing
        // them inside every block would cost 8x the partial-sum traffic), then one thread = 8 channels x PV pixels
        if (fin.part) {              // publishes mean / invstd (the arrays this launch was given) and updates the running statistics
            EAS_LAUNCH(bn_finalize_kernel, dim3(C), dim3(EAS_BLOCK), 0, st, fin);
            EAS_CHECK_LAUNCH();
        }
        // one pixel per thread: 8 x T dword loads (each channel row contiguous over the lanes) and T 16-byte stores, few registers, many
        // waves in flight (measured on config 2: 1.02 ms per step for all layers against 1.10 / 1.24 ms with 2 / 4 pixels per thread and
        // 1.10 ms for the fp32-writing kernel)
        constexpr int PV = 1;
        const int chunks = bn_pick_chunks((int64_t)N * (HW / PV), C / 8);
        EAS_LAUNCH((bn_lif_fwd_sp_kernel<T_, HARD, DI, STRICT, PV>), EAS_CHAN_GRID(chunks, C / 8), dim3(EAS_BLOCK), 0, st, y,
                           mean, invstd, gamma, beta, v_in,
                           v_out, p, planes, res_planes, mean_out, N, C, HW, bcast, ox.y_ctot, out_groups, res_groups);
        EAS_CHECK_LAUNCH();
        return EAS_OK;
    }
    const int chunks = bn_pick_chunks((int64_t)N * (HW / EAS_VEC), C);
    EAS_LAUNCH((bn_lif_fwd_kernel<T_, HARD, DI, STRICT>), EAS_CHAN_GRID(chunks, C), dim3(EAS_BLOCK), 0, st, y, mean,
                       invstd, gamma, beta, v_in, v_out, p, spikes, mean_out, N, C, HW, bcast, fin, ox);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

template <bool HARD, bool DI, bool STRICT>
int launch_fwd(int T, const float* y, const float* mean, const float* invstd, const float* gamma, const float* beta,
               const float* v_in, float* v_out, EasLifParams p, float* spikes, float* mean_out, int N, int C, int HW,
               int bcast, const BnFin& fin, const BnLifOut& ox, bf16x8* planes, const bf16x8* res_planes, int out_groups, int res_groups,
               hipStream_t st) {
#define EAS_CASE(TT) \
    case TT: return launch_fwd_t<TT, HARD, DI, STRICT>(y, mean, invstd, gamma, beta, v_in, v_out, p, spikes, mean_out, N, C, HW, bcast, fin, ox, planes, res_planes, out_groups, res_groups, st);
    switch (T) {
        EAS_CASE(1) EAS_CASE(2) EAS_CASE(3) EAS_CASE(4) EAS_CASE(5) EAS_CASE(6) EAS_CASE(7) EAS_CASE(8)
        default: return EAS_ERR_UNSUPPORTED;
    }
#undef EAS_CASE
}

// One backward call: the operands of eas_bn_lif_bwd_ex / _patan after validation.
struct BwdCall {
    const float *grad_s, *grad_mean, *y, *mean, *invstd, *gamma, *beta, *v_init;
    EasLifParams p;
    int sg;
    float alpha;
    int batch_stats;
    float *grad_y, *grad_gamma, *grad_beta, *grad_w;
    double* ws;
    int T, N, C, HW, bcast, gs_ctot, y_ctot;
    const float* alpha_dev;
    float* grad_alpha;
    hipStream_t st;
};

// development switch, read per call (a test compares the forms in one process): EAS_BNLIF_BWD holds "two" (keep the two-pass launches where
// one block per channel would do) and / or "generic" (the generic instance where the table has a fast one), e.g. "two,generic"
static inline bool bwd_form(const char* word) {
    const char* form = getenv("EAS_BNLIF_BWD");
    return form && strstr(form, word);
}

// one block per channel where a channel fits the registers of a block (bn_lif_bwd_small_kernel): groups per thread, 0 = two passes
static inline int bwd_one_pass_gpt(const BwdCall& c) {
    const int gpt = c.T <= 3 ? 3 : (c.T <= 5 ? 2 : 1);                // 8 * T floats per group in registers
    const int64_t groups = (int64_t)c.N * (c.HW / EAS_VEC);
    return (!bwd_form("two") && !c.bcast && c.C >= 64 && groups <= 512 * gpt) ? gpt : 0;       // (1024-thread blocks are capped at 128 registers: they spill)
}

template <int T_, bool HARD, bool DI, bool STRICT, class POL>
int launch_bwd_t(const BwdCall& c) {
    const int N = c.N, C = c.C, HW = c.HW;
    const int chunks = bn_pick_chunks((int64_t)N * (HW / EAS_VEC), C);
    if (bwd_one_pass_gpt(c)) {
        constexpr int GPT = T_ <= 3 ? 3 : (T_ <= 5 ? 2 : 1);
        const int64_t groups = (int64_t)N * (HW / EAS_VEC);
#define EAS_SMALL(NT_) EAS_LAUNCH((bn_lif_bwd_small_kernel<T_, HARD, DI, STRICT, NT_, GPT, POL>), dim3(C), dim3(NT_), 0, c.st, c.grad_s, c.grad_mean, c.y, \
                                   c.mean, c.invstd, c.gamma, c.beta, c.v_init, c.p, c.sg, c.alpha, c.batch_stats, c.ws, c.grad_y, c.grad_gamma,       \
                                   c.grad_beta, N, C, HW, c.gs_ctot, c.y_ctot, c.alpha_dev)
        if (groups <= 256 * GPT) EAS_SMALL(256);
        else EAS_SMALL(512);
#undef EAS_SMALL
        EAS_CHECK_LAUNCH();
        if (c.grad_w || c.grad_alpha) {
            EAS_LAUNCH(bn_lif_bwd_scalars_kernel, dim3(1), dim3(EAS_BLOCK), 0, c.st, c.ws, C, c.p, c.grad_w, c.alpha_dev, c.grad_alpha);
            EAS_CHECK_LAUNCH();
        }
        return EAS_OK;
    }
    // two passes: the BatchNorm backward needs the channel's sums of dz and dz * xhat before any grad_y; pass 2 recomputes the neuron
    // (cheaper than parking dz: measured).
    // Channel groups (EAS_BNLIF_BWD_GROUP_MB, development; 0 = one pair of launches for the whole layer): the pair runs group by group with
    // at most that many MB of y + grad_s per group, so that the apply pass of a group re-reads what its sum pass has just read while it is
    // still in the 256 MB Infinity Cache.
    static const int group_mb = eas_dev_env("EAS_BNLIF_BWD_GROUP_MB") ? atoi(eas_dev_env("EAS_BNLIF_BWD_GROUP_MB")) : 0;
    int gc = C;
    if (group_mb > 0) {
        const double per_channel = (double)N * HW * 4.0 * ((c.bcast ? 1 : T_) + T_);
        gc = (int)(group_mb * 1048576.0 / per_channel) / 8 * 8;
        if (gc < 8) gc = 8;
        if (gc > C) gc = C;
    }
    for (int c0 = 0; c0 < C; c0 += gc) {
        const int c1 = c0 + gc < C ? c0 + gc : C;
        const int last = c1 == C;
        EAS_LAUNCH((bn_lif_bwd_kernel<T_, HARD, DI, STRICT, false, POL>), EAS_CHAN_GRID(chunks, c1 - c0), dim3(EAS_BLOCK), 0, c.st, c.grad_s,
                   c.grad_mean, c.y, c.mean, c.invstd, c.gamma, c.beta, c.v_init, c.p, c.sg, c.alpha, c.batch_stats, c.ws, chunks, c.grad_y,
                   c.grad_gamma, c.grad_beta, (float*)nullptr, N, C, HW, c.bcast, c.gs_ctot, c.y_ctot, c.alpha_dev, (float*)nullptr, c0, c1, 0);
        EAS_CHECK_LAUNCH();
        EAS_LAUNCH((bn_lif_bwd_kernel<T_, HARD, DI, STRICT, true, POL>), EAS_CHAN_GRID(chunks, c1 - c0), dim3(EAS_BLOCK), 0, c.st, c.grad_s,
                   c.grad_mean, c.y, c.mean, c.invstd, c.gamma, c.beta, c.v_init, c.p, c.sg, c.alpha, c.batch_stats, c.ws, chunks, c.grad_y,
                   c.grad_gamma, c.grad_beta, c.grad_w, N, C, HW, c.bcast, c.gs_ctot, c.y_ctot, c.alpha_dev, c.grad_alpha, c0, c1, last);
        EAS_CHECK_LAUNCH();
    }
    return EAS_OK;
}

// The instances of the backward: every row is one set of kernels (sums, apply, one-pass at 256 and 512 threads).  A fast row serves the
// launches with exactly its surrogate and reset form and -- in the two-pass form -- plain operands; a generic row (sg = EAS_SG_RUNTIME) serves every launch of its
// (T, reset, decay) form.  Fast rows exist for what the bench workloads and the published recipes train with (eas_snn_amd/workloads.py:
// soft reset, decay_input = False, attached reset, spike_fn atan, T = 3 / 5 / 7); everything else runs the generic row of its form.
struct BwdRow {
    int T;
    bool hard, di;
    int sg;
    bool detach;
    int (*fn)(const BwdCall&);
};
template <int T_, bool HARD, bool DI, int SG = EAS_SG_RUNTIME, bool DETACH = false>
constexpr BwdRow bwd_row() {
    return {T_, HARD, DI, SG, DETACH, launch_bwd_t<T_, HARD, DI, false, BnLifBwdPolicy<SG, DETACH>>};
}
#define EAS_BWD_GENERIC_ROWS(H, D) \
    bwd_row<1, H, D>(), bwd_row<2, H, D>(), bwd_row<3, H, D>(), bwd_row<4, H, D>(), bwd_row<5, H, D>(), bwd_row<6, H, D>(), bwd_row<7, H, D>(), bwd_row<8, H, D>()
const BwdRow kBwdInstances[] = {
    // fast (first: the first matching row is taken)
    bwd_row<3, false, false, EAS_SG_ATAN>(), bwd_row<5, false, false, EAS_SG_ATAN>(), bwd_row<7, false, false, EAS_SG_ATAN>(),
    // generic
    EAS_BWD_GENERIC_ROWS(false, false), EAS_BWD_GENERIC_ROWS(true, false), EAS_BWD_GENERIC_ROWS(false, true), EAS_BWD_GENERIC_ROWS(true, true),
};
#undef EAS_BWD_GENERIC_ROWS

// the table decides: the first row that serves the call
int bwd_select(const BwdCall& c) {
    const bool hard = c.p.flags & EAS_LIF_HARD_RESET, di = c.p.flags & EAS_LIF_DECAY_INPUT, detach = c.p.flags & EAS_LIF_DETACH_RESET;
    if (c.p.flags & EAS_LIF_FIRE_STRICT) return EAS_ERR_UNSUPPORTED;      // strict '>' firing only exists in the sampler / in-repo LIFCell
    const bool plain = bwd_one_pass_gpt(c) || (c.grad_s && !c.grad_mean && !c.v_init && !c.bcast);      // the one-pass kernel takes every operand form
    const bool fast_ok = plain && !bwd_form("generic");
    for (const BwdRow& r : kBwdInstances) {
        if (r.T != c.T || r.hard != hard || r.di != di) continue;
        if (r.sg == EAS_SG_RUNTIME || (fast_ok && r.sg == c.sg && r.detach == detach)) return r.fn(c);
    }
    return EAS_ERR_UNSUPPORTED;
}

}  // namespace

extern "C" {

int64_t eas_bn_workspace_doubles(int C) { return (int64_t)C * EAS_BN_MAX_CHUNKS * 4; }

// launches the partial-sum kernel; returns the number of chunks per channel (> 0) or a negative status
static int stats_partial(const float* y, int TN, int C, int HW, double* workspace, int y_ctot, hipStream_t st) {
    const int Cy = y_ctot ? y_ctot : C;
    int chunks;
    if (HW % EAS_VEC == 0 && (((uintptr_t)y) & 15) == 0) {
        chunks = bn_pick_chunks((int64_t)TN * (HW / EAS_VEC), C);
        EAS_LAUNCH(bn_stats_partial, dim3(chunks, C), dim3(EAS_BLOCK), 0, st, y, TN, C, HW, workspace, Cy);
    } else {
        if (Cy != C) return EAS_ERR_UNSUPPORTED;
        chunks = bn_pick_chunks((int64_t)TN * HW, C);
        EAS_LAUNCH(bn_stats_partial_scalar, dim3(chunks, C), dim3(EAS_BLOCK), 0, st, y, TN, C, HW, workspace);
    }
    if (hipGetLastError() != hipSuccess) return EAS_ERR_LAUNCH;
    return chunks;
}

int eas_bn_stats(const float* y, int TN, int C, int HW, int replicas, float eps, float momentum, float* mean,
                 float* invstd, float* running_mean, float* running_var, double* workspace, eas_stream_t stream) {
    if (!y || !mean || !invstd || !workspace || TN < 1 || C < 1 || HW < 1 || replicas < 1) return EAS_ERR_INVALID_ARG;
    if ((running_mean == nullptr) != (running_var == nullptr)) return EAS_ERR_INVALID_ARG;
    if (C > 65535) return EAS_ERR_UNSUPPORTED;
    hipStream_t st = eas_s(stream);
    EAS_CLEAR_ERR();
    const int chunks = stats_partial(y, TN, C, HW, workspace, 0, st);
    if (chunks < 0) return chunks;
    const BnFin fin{workspace, chunks, EAS_BN_MAX_CHUNKS, replicas, (double)TN * HW, eps, momentum, mean, invstd, running_mean, running_var};
    EAS_LAUNCH(bn_stats_finalize, dim3(C), dim3(EAS_WAVE), 0, st, fin);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

int eas_bn_stats_partial(const float* y, int y_ctot, int TN, int C, int HW, double* workspace, eas_stream_t stream) {
    if (!y || !workspace || TN < 1 || C < 1 || HW < 1 || !bn_slice(y_ctot, C)) return EAS_ERR_INVALID_ARG;
    if (C > 65535) return EAS_ERR_UNSUPPORTED;
    EAS_CLEAR_ERR();
    return stats_partial(y, TN, C, HW, workspace, y_ctot, eas_s(stream));
}

int eas_bn_lif_fwd_ex(const float* y, int y_ctot, float* mean, float* invstd, const float* gamma, const float* beta,
                      const float* v_in, float* v_out, const float* w_logit, float k_const, float v_th, float v_reset,
                      int flags, float* spikes, float* mean_out, int T, int N, int C, int HW, int y_bcast,
                      const EasBnPending* pending, const float* residual, int out_ctot, void* spikes_planes, const void* residual_planes,
                      int residual_ctot, eas_stream_t stream) {
    if (!y || !mean || !invstd || !gamma || !beta || (!spikes && !spikes_planes) || (spikes && spikes_planes) || T < 1 || N < 1 || C < 1 || HW < 1)
        return EAS_ERR_INVALID_ARG;
    if (HW % EAS_VEC != 0 || C > 65535 || T > 8) return EAS_ERR_UNSUPPORTED;
    if (((uintptr_t)y | (uintptr_t)v_in | (uintptr_t)v_out | (uintptr_t)spikes | (uintptr_t)mean_out | (uintptr_t)residual |
         (uintptr_t)spikes_planes | (uintptr_t)residual_planes) & 15)
        return EAS_ERR_INVALID_ARG;
    // (the broadcast test reads y_ctot as given, before bn_slice turns y_ctot == C into 0)
    if ((y_ctot != 0 && y_bcast) || !bn_slice(out_ctot, C) || !bn_slice(y_ctot, C)) return EAS_ERR_INVALID_ARG;
    if (spikes_planes) {
        // planes are blocks of 8 channels: the layer's channels, its slice of a concatenation and a residual must be whole blocks
        if (C % 8 != 0 || (out_ctot % 8) != 0 || residual || (residual_planes && (residual_ctot % 8 != 0 || !bn_slice(residual_ctot, C))))
            return EAS_ERR_UNSUPPORTED;
    } else if (residual_planes) {
        return EAS_ERR_UNSUPPORTED;
    }
    BnFin fin;
    if (int rc = bn_fin_from(pending, mean, invstd, fin)) return rc;
    const BnLifOut ox{residual, out_ctot, y_ctot};
    EasLifParams p{w_logit, k_const, v_th, v_reset, flags};
    hipStream_t st = eas_s(stream);
    EAS_CLEAR_ERR();
    const int out_groups = (out_ctot ? out_ctot : C) / 8, res_groups = (residual_ctot ? residual_ctot : C) / 8;
    return eas_lif_dispatch(flags, [&](auto h, auto d, auto strict) {
        if constexpr (decltype(strict)::value) {
            return (int)EAS_ERR_UNSUPPORTED;      // strict '>' firing only exists in the sampler / in-repo LIFCell
        } else {
            return launch_fwd<decltype(h)::value, decltype(d)::value, false>(T, y, mean, invstd, gamma, beta, v_in, v_out, p, spikes, mean_out, N, C, HW,
                                                                             y_bcast, fin, ox, (bf16x8*)spikes_planes,
                                                                             (const bf16x8*)residual_planes, out_groups, res_groups, st);
        }
    });
}

int eas_bn_lif_fwd(const float* y, const float* mean, const float* invstd, const float* gamma, const float* beta,
                   const float* v_in, float* v_out, const float* w_logit, float k_const, float v_th, float v_reset,
                   int flags, float* spikes, float* mean_out, int T, int N, int C, int HW, int y_bcast,
                   eas_stream_t stream) {
    return eas_bn_lif_fwd_ex(y, 0, const_cast<float*>(mean), const_cast<float*>(invstd), gamma, beta, v_in, v_out, w_logit, k_const, v_th,
                             v_reset, flags, spikes, mean_out, T, N, C, HW, y_bcast, nullptr, nullptr, 0, nullptr, nullptr, 0, stream);
}

static int bn_lif_bwd_impl(const float* grad_s, int grad_s_ctot, const float* grad_mean, const float* y, int y_ctot, const float* mean,
                           const float* invstd, const float* gamma, const float* beta, const float* v_init,
                           const float* w_logit, float k_const, float v_th, float v_reset, int flags, int surrogate,
                           float alpha, const float* alpha_dev, float* grad_alpha, int batch_stats, float* grad_y, float* grad_gamma,
                           float* grad_beta, float* grad_w, double* workspace, int T, int N, int C, int HW, int y_bcast,
                           eas_stream_t stream) {
    if (!y || !mean || !invstd || !gamma || !beta || !grad_y || !grad_gamma || !grad_beta || !workspace ||
        (!grad_s && !grad_mean) || T < 1 || N < 1 || C < 1 || HW < 1)
        return EAS_ERR_INVALID_ARG;
    if (surrogate < EAS_SG_ATAN || surrogate > EAS_SG_PATAN) return EAS_ERR_INVALID_ARG;
    if (surrogate == EAS_SG_PATAN ? !alpha_dev : !(alpha > 0.f)) return EAS_ERR_INVALID_ARG;
    if (grad_w && !w_logit) return EAS_ERR_INVALID_ARG;
    if (HW % EAS_VEC != 0 || C > 65535 || T > 8) return EAS_ERR_UNSUPPORTED;
    if (((uintptr_t)y | (uintptr_t)grad_s | (uintptr_t)grad_mean | (uintptr_t)v_init | (uintptr_t)grad_y) & 15)
        return EAS_ERR_INVALID_ARG;
    // (the broadcast test reads y_ctot as given, before bn_slice turns y_ctot == C into 0)
    if ((y_ctot != 0 && y_bcast) || !bn_slice(grad_s_ctot, C) || !bn_slice(y_ctot, C)) return EAS_ERR_INVALID_ARG;
    const BwdCall call{grad_s, grad_mean, y, mean, invstd, gamma, beta, v_init, EasLifParams{w_logit, k_const, v_th, v_reset, flags}, surrogate, alpha,
                       batch_stats, grad_y, grad_gamma, grad_beta, grad_w, workspace, T, N, C, HW, y_bcast, grad_s_ctot, y_ctot, alpha_dev, grad_alpha,
                       eas_s(stream)};
    EAS_CLEAR_ERR();
    return bwd_select(call);
}

int eas_bn_lif_bwd_ex(const float* grad_s, int grad_s_ctot, const float* grad_mean, const float* y, int y_ctot, const float* mean,
                      const float* invstd, const float* gamma, const float* beta, const float* v_init,
                      const float* w_logit, float k_const, float v_th, float v_reset, int flags, int surrogate,
                      float alpha, int batch_stats, float* grad_y, float* grad_gamma, float* grad_beta,
                      float* grad_w, double* workspace, int T, int N, int C, int HW, int y_bcast, eas_stream_t stream) {
    if (surrogate == EAS_SG_PATAN) return EAS_ERR_INVALID_ARG;      // learnable slope: eas_bn_lif_bwd_patan
    return bn_lif_bwd_impl(grad_s, grad_s_ctot, grad_mean, y, y_ctot, mean, invstd, gamma, beta, v_init, w_logit, k_const, v_th, v_reset,
                           flags, surrogate, alpha, nullptr, nullptr, batch_stats, grad_y, grad_gamma, grad_beta, grad_w, workspace, T, N, C,
                           HW, y_bcast, stream);
}

int eas_bn_lif_bwd_patan(const float* grad_s, int grad_s_ctot, const float* grad_mean, const float* y, int y_ctot, const float* mean,
                         const float* invstd, const float* gamma, const float* beta, const float* v_init,
                         const float* w_logit, float k_const, float v_th, float v_reset, int flags, const float* alpha,
                         float* grad_alpha, int batch_stats, float* grad_y, float* grad_gamma, float* grad_beta,
                         float* grad_w, double* workspace, int T, int N, int C, int HW, int y_bcast, eas_stream_t stream) {
    return bn_lif_bwd_impl(grad_s, grad_s_ctot, grad_mean, y, y_ctot, mean, invstd, gamma, beta, v_init, w_logit, k_const, v_th, v_reset,
                           flags, EAS_SG_PATAN, 0.f, alpha, grad_alpha, batch_stats, grad_y, grad_gamma, grad_beta, grad_w, workspace, T, N, C,
                           HW, y_bcast, stream);
}

int eas_bn_lif_bwd(const float* grad_s, const float* grad_mean, const float* y, const float* mean,
                   const float* invstd, const float* gamma, const float* beta, const float* v_init,
                   const float* w_logit, float k_const, float v_th, float v_reset, int flags, int surrogate,
                   float alpha, int batch_stats, float* grad_y, float* grad_gamma, float* grad_beta,
                   float* grad_w, double* workspace, int T, int N, int C, int HW, int y_bcast, eas_stream_t stream) {
    return eas_bn_lif_bwd_ex(grad_s, 0, grad_mean, y, 0, mean, invstd, gamma, beta, v_init, w_logit, k_const, v_th, v_reset, flags,
                             surrogate, alpha, batch_stats, grad_y, grad_gamma, grad_beta, grad_w, workspace, T, N, C, HW, y_bcast, stream);
}

}  // extern "C"
