// K2: multi-step (P)LIF integrate-fire-reset, forward and backward, and the time-mean readout.
// HBM-bound elementwise kernels.  One thread owns 4 consecutive neurons (16-B loads/stores) and
// walks the T time steps with the membrane potential in registers, so each [T][M] tensor is
// touched exactly once: fwd reads x (4 B) and writes s (4 B) [+ h (4 B) when training];
// bwd reads grad_s, h (8 B) and writes grad_x (4 B) per neuron-step.
//
// The forward states its per-neuron work ONCE, for W neurons of a thread (Cols<W>): lif_walk runs it with W = 4 over the float4 columns
// and with W = 1 over what is left; the backward does so for its float4 columns.  Its scalar columns and the time mean keep loops of
// their own, where the shared form measured slower (notes at both).  The (reset, decay, firing) form reaches the kernels through eas_lif_dispatch (eas_common.h), the
// fire-and-reset rule and the scalar parameter gradients' final stage are the ones of eas_common.h as well.
#include "eas_common.h"

namespace {

// W consecutive floats of a row, W = 4: one 16-byte access
template <int W>
struct alignas(4 * W) Cols {
    float e[W];
};
template <int W>
__device__ __forceinline__ Cols<W> ld(const float* p) { return *reinterpret_cast<const Cols<W>*>(p); }
template <int W>
__device__ __forceinline__ void st(float* p, const Cols<W>& v) { *reinterpret_cast<Cols<W>*>(p) = v; }

// The columns of a [T][M] tensor, grid-strided: body(width, j) for the W = width() columns from j on.  float4 columns where every row is
// 16-byte aligned (M % 4 == 0, or a single row), scalar columns for the remainder (M % 4 columns, or all of them).
// lif_walk_vec: the float4 columns only; returns the first column that is left for a scalar walk.
template <class F>
__device__ __forceinline__ int64_t lif_walk_vec(int T, int64_t M, F&& body) {
    const int64_t nvec = (M % EAS_VEC == 0 || T == 1) ? M / EAS_VEC : 0;
    const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = first; i < nvec; i += stride) body(std::integral_constant<int, EAS_VEC>{}, i * EAS_VEC);
    return nvec * EAS_VEC;
}
template <class F>
__device__ __forceinline__ void lif_walk(int T, int64_t M, F&& body) {
    const int64_t rest = lif_walk_vec(T, M, body);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = rest + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < M; j += stride) body(std::integral_constant<int, 1>{}, j);
}
static inline int lif_grid(int64_t M) { return eas_grid_1d(M % EAS_VEC == 0 ? M / EAS_VEC : M); }

// T_ = 1..8: the time steps as a template constant (all loads of x issued before the first step); 0: any T
template <int T_, bool HARD, bool DI, bool STRICT>
__global__ __launch_bounds__(EAS_BLOCK) void lif_fwd_kernel(const float* __restrict__ x, const float* v_in, float* v_out,
                                                            EasLifParams p, float* __restrict__ spikes,
                                                            float* __restrict__ h_save, float* __restrict__ mean_out,
                                                            int T_rt, int64_t M) {
    const float k = eas_lif_k(p);
    const float omk = 1.0f - k;
    const int T = T_ > 0 ? T_ : T_rt;
    lif_walk(T, M, [&](auto width, int64_t j) {
        constexpr int W = decltype(width)::value;
        Cols<W> v, acc;
        if (v_in) v = ld<W>(v_in + j);
#pragma unroll
        for (int e = 0; e < W; ++e) {
            if (!v_in) v.e[e] = HARD ? p.v_reset : 0.0f;
            acc.e[e] = 0.f;
        }
        auto step = [&](int t, const Cols<W>& xt) {
            Cols<W> h, s;
#pragma unroll
            for (int e = 0; e < W; ++e) {
                eas_lif_step<HARD, DI, STRICT>(v.e[e], xt.e[e], k, omk, p.v_th, p.v_reset, h.e[e], s.e[e]);
                acc.e[e] += s.e[e];
            }
            st<W>(spikes + (int64_t)t * M + j, s);
            if (h_save) st<W>(h_save + (int64_t)t * M + j, h);
        };
        if constexpr (T_ > 0 && W > 1) {
            Cols<W> xs[T_ > 0 ? T_ : 1];
#pragma unroll
            for (int t = 0; t < T_; ++t) xs[t] = ld<W>(x + (int64_t)t * M + j);
#pragma unroll
            for (int t = 0; t < T_; ++t) step(t, xs[t]);
        } else {
            for (int t = 0; t < T; ++t) step(t, ld<W>(x + (int64_t)t * M + j));
        }
        if (v_out) st<W>(v_out + j, v);
        if (mean_out) {
#pragma unroll
            for (int e = 0; e < W; ++e) acc.e[e] /= (float)T;   // sum / T, like ATen's mean
            st<W>(mean_out + j, acc);
        }
    });
}

template <int T_, bool HARD, bool DI, bool STRICT>
__global__ __launch_bounds__(EAS_BLOCK) void lif_bwd_kernel(const float* __restrict__ grad_s,
                                                            const float* __restrict__ grad_mean,
                                                            const float* __restrict__ h_save,
                                                            const float* __restrict__ v_init,
                                                            const float* __restrict__ x, EasLifParams p, int sg_id,
                                                            float alpha, const float* __restrict__ alpha_dev,
                                                            float* __restrict__ grad_x, float* __restrict__ partial,
                                                            float* __restrict__ partial_a, int T_rt, int64_t M) {
    __shared__ float red[EAS_BLOCK / EAS_WAVE];
    if (alpha_dev) alpha = fabsf(*alpha_dev);    // learnable slope (EAS_SG_PATAN)
    const float k = eas_lif_k(p);
    const float omk = 1.0f - k;
    const bool detach = (p.flags & EAS_LIF_DETACH_RESET) != 0;
    const int T = T_ > 0 ? T_ : T_rt;
    const float invT = 1.0f / (float)T;
    float dk = 0.f, da = 0.f;
    const int64_t rest = lif_walk_vec(T, M, [&](auto width, int64_t j) {
        constexpr int W = decltype(width)::value;
        Cols<W> gv, gm;
#pragma unroll
        for (int e = 0; e < W; ++e) gv.e[e] = gm.e[e] = 0.f;
        if (grad_mean) {
            gm = ld<W>(grad_mean + j);
#pragma unroll
            for (int e = 0; e < W; ++e) gm.e[e] *= invT;
        }
        Cols<W> hn = ld<W>(h_save + (int64_t)(T - 1) * M + j);
        for (int t = T - 1; t >= 0; --t) {
            const Cols<W> hc = hn;
            // v_{t-1} recomputed from h_{t-1}, so only h is stored
            Cols<W> vp, gs = gm, xv, gx;
            if (t > 0) {
                hn = ld<W>(h_save + (int64_t)(t - 1) * M + j);
#pragma unroll
                for (int e = 0; e < W; ++e) {
                    float s;
                    vp.e[e] = eas_lif_fire_reset<HARD, STRICT>(hn.e[e], p.v_th, p.v_reset, s);
                }
            } else if (v_init) {
                vp = ld<W>(v_init + j);
            } else {
#pragma unroll
                for (int e = 0; e < W; ++e) vp.e[e] = HARD ? p.v_reset : 0.f;
            }
            if (grad_s) {
                const Cols<W> g = ld<W>(grad_s + (int64_t)t * M + j);
#pragma unroll
                for (int e = 0; e < W; ++e) gs.e[e] += g.e[e];
            }
            if (DI && x) {
                xv = ld<W>(x + (int64_t)t * M + j);
            } else {
#pragma unroll
                for (int e = 0; e < W; ++e) xv.e[e] = 0.f;
            }
#pragma unroll
            for (int e = 0; e < W; ++e) {
                float dkt;
                eas_lif_step_bwd<HARD, DI, STRICT>(gs.e[e], gv.e[e], hc.e[e], vp.e[e], xv.e[e], k, omk, p.v_th, p.v_reset, detach, sg_id,
                                                   alpha, dkt, gx.e[e], da);
                dk += dkt;
            }
            st<W>(grad_x + (int64_t)t * M + j, gx);
        }
    });
    // The scalar columns keep a loop of their own: the body above instantiated for one column (h_{t-1} carried or read again) measured
    // 3.5 % slower on rows that are not 16-byte aligned than this form, which reads h_t and h_{t-1} in every step
    // (profiles/bn_family_one_rule_ab.txt).  Same arithmetic per neuron-step.
    for (int64_t j = rest + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < M; j += (int64_t)gridDim.x * blockDim.x) {
        float gv = 0.f, s_;
        const float gm = grad_mean ? grad_mean[j] * invT : 0.f;
        for (int t = T - 1; t >= 0; --t) {
            const float h = h_save[(int64_t)t * M + j];
            const float vp = t > 0 ? eas_lif_fire_reset<HARD, STRICT>(h_save[(int64_t)(t - 1) * M + j], p.v_th, p.v_reset, s_)
                                   : (v_init ? v_init[j] : (HARD ? p.v_reset : 0.f));
            const float gs = gm + (grad_s ? grad_s[(int64_t)t * M + j] : 0.f);
            const float xv = (DI && x) ? x[(int64_t)t * M + j] : 0.f;
            float dkt, gx;
            eas_lif_step_bwd<HARD, DI, STRICT>(gs, gv, h, vp, xv, k, omk, p.v_th, p.v_reset, detach, sg_id, alpha, dkt, gx, da);
            dk += dkt;
            grad_x[(int64_t)t * M + j] = gx;
        }
    }
    if (partial) {
        const float tot = eas_block_sum<float, EAS_BLOCK / EAS_WAVE>(dk, red);
        if (threadIdx.x == 0) partial[blockIdx.x] = tot;
    }
    if (partial_a) {
        const float tot = eas_block_sum<float, EAS_BLOCK / EAS_WAVE>(da, red);
        if (threadIdx.x == 0) partial_a[blockIdx.x] = tot;
    }
}

// final stage of the grad_w / grad_alpha reduction: the per-block partials in a fixed order (deterministic), eas_lif_scalar_grads
__global__ __launch_bounds__(EAS_BLOCK) void lif_gradw_finalize(const float* __restrict__ partial, int n,
                                                                const float* __restrict__ w_logit,
                                                                float* __restrict__ grad_w,
                                                                const float* __restrict__ partial_a,
                                                                const float* __restrict__ alpha_dev,
                                                                float* __restrict__ grad_alpha) {
    __shared__ double red[EAS_BLOCK / EAS_WAVE];
    eas_lif_scalar_grads(n, [&](int i) { return partial[i]; }, [&](int i) { return partial_a[i]; }, w_logit, alpha_dev, grad_w, grad_alpha, red);
}

// (two loops written out: the shared walk with its 64-bit column index costs this kernel, which has nothing but its loads, 4 registers
// and measured 0.2 to 0.5 us slower per call -- profiles/bn_family_one_rule_ab.txt)
__global__ __launch_bounds__(EAS_BLOCK) void time_mean_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                              int T, int64_t M) {
    const int64_t nvec = (M % EAS_VEC == 0 || T == 1) ? M / EAS_VEC : 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const float Tf = (float)T;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int t = 0; t < T; ++t) {
            const float4 v = reinterpret_cast<const float4*>(x + (int64_t)t * M)[i];
            a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
        }
        reinterpret_cast<float4*>(out)[i] = make_float4(a.x / Tf, a.y / Tf, a.z / Tf, a.w / Tf);
    }
    {
        for (int64_t j = nvec * EAS_VEC + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < M; j += stride) {
            float a = 0.f;
            for (int t = 0; t < T; ++t) a += x[(int64_t)t * M + j];
            out[j] = a / Tf;
        }
    }
}

constexpr int kReduceBlocks = 2048;

template <bool HARD, bool DI, bool STRICT>
int launch_fwd(const float* x, const float* v_in, float* v_out, EasLifParams p, float* spikes, float* h_save, float* mean_out, int T,
               int64_t M, hipStream_t st) {
    // instance T for T = 1..8, instance 0 (runtime T) above
    static constexpr decltype(&lif_fwd_kernel<0, HARD, DI, STRICT>) kern[9] = {
        lif_fwd_kernel<0, HARD, DI, STRICT>, lif_fwd_kernel<1, HARD, DI, STRICT>, lif_fwd_kernel<2, HARD, DI, STRICT>,
        lif_fwd_kernel<3, HARD, DI, STRICT>, lif_fwd_kernel<4, HARD, DI, STRICT>, lif_fwd_kernel<5, HARD, DI, STRICT>,
        lif_fwd_kernel<6, HARD, DI, STRICT>, lif_fwd_kernel<7, HARD, DI, STRICT>, lif_fwd_kernel<8, HARD, DI, STRICT>};
    EAS_LAUNCH(kern[T <= 8 ? T : 0], dim3(lif_grid(M)), dim3(EAS_BLOCK), 0, st, x, v_in, v_out, p, spikes, h_save, mean_out, T, M);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

template <bool HARD, bool DI, bool STRICT>
int launch_bwd(const float* grad_s, const float* grad_mean, const float* h_save, const float* v_init, const float* x,
               EasLifParams p, int sg, float alpha, const float* alpha_dev, float* grad_alpha, float* grad_x, float* grad_w,
               float* workspace, int T, int64_t M, hipStream_t st) {
    int grid = lif_grid(M);
    if (grid > kReduceBlocks) grid = kReduceBlocks;
    float* partial = grad_w ? workspace : nullptr;
    float* partial_a = grad_alpha ? workspace + kReduceBlocks : nullptr;
    EAS_LAUNCH((lif_bwd_kernel<0, HARD, DI, STRICT>), dim3(grid), dim3(EAS_BLOCK), 0, st, grad_s, grad_mean,
                       h_save, v_init, x, p, sg, alpha, alpha_dev, grad_x, partial, partial_a, T, M);
    EAS_CHECK_LAUNCH();
    if (grad_w || grad_alpha) {
        EAS_LAUNCH(lif_gradw_finalize, dim3(1), dim3(EAS_BLOCK), 0, st, partial, grid, p.w_logit, grad_w, partial_a, alpha_dev,
                           grad_alpha);
        EAS_CHECK_LAUNCH();
    }
    return EAS_OK;
}

}  // namespace

extern "C" {

int64_t eas_reduce_workspace_floats(int64_t) { return 2 * kReduceBlocks; }   // grad_w partials | grad_alpha partials

int eas_lif_fwd(const float* x, const float* v_in, float* v_out, const float* w_logit, float k_const, float v_th,
                float v_reset, int flags, float* spikes, float* h_save, float* mean_out, int T, int64_t M, eas_stream_t stream) {
    if (!x || !spikes || T < 1 || M < 0) return EAS_ERR_INVALID_ARG;
    if (M == 0) return EAS_OK;
    if (((uintptr_t)x | (uintptr_t)v_in | (uintptr_t)v_out | (uintptr_t)spikes | (uintptr_t)h_save | (uintptr_t)mean_out) & 15)
        return EAS_ERR_INVALID_ARG;
    EasLifParams p{w_logit, k_const, v_th, v_reset, flags};
    hipStream_t st = eas_s(stream);
    EAS_CLEAR_ERR();
    return eas_lif_dispatch(flags, [&](auto h, auto d, auto s) {
        return launch_fwd<decltype(h)::value, decltype(d)::value, decltype(s)::value>(x, v_in, v_out, p, spikes, h_save, mean_out, T, M, st);
    });
}

static int lif_bwd_impl(const float* grad_s, const float* grad_mean, const float* h_save, const float* v_init,
                        const float* x, const float* w_logit, float k_const, float v_th, float v_reset, int flags,
                        int surrogate, float alpha, const float* alpha_dev, float* grad_alpha, float* grad_x, float* grad_w,
                        float* workspace, int T, int64_t M, eas_stream_t stream) {
    if (!h_save || !grad_x || T < 1 || M < 0 || (!grad_s && !grad_mean)) return EAS_ERR_INVALID_ARG;
    if (surrogate < EAS_SG_ATAN || surrogate > EAS_SG_PATAN) return EAS_ERR_INVALID_ARG;
    if (surrogate == EAS_SG_PATAN ? !alpha_dev : !(alpha > 0.f)) return EAS_ERR_INVALID_ARG;
    if ((grad_w && (!workspace || !w_logit)) || (grad_alpha && (!workspace || !alpha_dev))) return EAS_ERR_INVALID_ARG;
    if (M == 0) return EAS_OK;
    if (((uintptr_t)grad_s | (uintptr_t)grad_mean | (uintptr_t)h_save | (uintptr_t)v_init | (uintptr_t)x |
         (uintptr_t)grad_x) & 15)
        return EAS_ERR_INVALID_ARG;
    if ((flags & EAS_LIF_DECAY_INPUT) && w_logit && grad_w && !x) return EAS_ERR_INVALID_ARG;
    EasLifParams p{w_logit, k_const, v_th, v_reset, flags};
    hipStream_t st = eas_s(stream);
    EAS_CLEAR_ERR();
    return eas_lif_dispatch(flags, [&](auto h, auto d, auto s) {
        return launch_bwd<decltype(h)::value, decltype(d)::value, decltype(s)::value>(grad_s, grad_mean, h_save, v_init, x, p, surrogate, alpha, alpha_dev, grad_alpha, grad_x, grad_w,
                                         workspace, T, M, st);
    });
}

int eas_lif_bwd(const float* grad_s, const float* grad_mean, const float* h_save, const float* v_init,
                const float* x, const float* w_logit, float k_const, float v_th, float v_reset, int flags,
                int surrogate, float alpha, float* grad_x, float* grad_w, float* workspace, int T, int64_t M,
                eas_stream_t stream) {
    if (surrogate == EAS_SG_PATAN) return EAS_ERR_INVALID_ARG;      // learnable slope: eas_lif_bwd_patan
    return lif_bwd_impl(grad_s, grad_mean, h_save, v_init, x, w_logit, k_const, v_th, v_reset, flags, surrogate, alpha, nullptr, nullptr,
                        grad_x, grad_w, workspace, T, M, stream);
}

int eas_lif_bwd_patan(const float* grad_s, const float* grad_mean, const float* h_save, const float* v_init,
                      const float* x, const float* w_logit, float k_const, float v_th, float v_reset, int flags,
                      const float* alpha, float* grad_alpha, float* grad_x, float* grad_w, float* workspace, int T, int64_t M,
                      eas_stream_t stream) {
    return lif_bwd_impl(grad_s, grad_mean, h_save, v_init, x, w_logit, k_const, v_th, v_reset, flags, EAS_SG_PATAN, 0.f, alpha, grad_alpha,
                        grad_x, grad_w, workspace, T, M, stream);
}

int eas_time_mean(const float* x, float* out, int T, int64_t M, eas_stream_t stream) {
    if (!x || !out || T < 1 || M < 0) return EAS_ERR_INVALID_ARG;
    if (M == 0) return EAS_OK;
    if (((uintptr_t)x | (uintptr_t)out) & 15) return EAS_ERR_INVALID_ARG;
    EAS_CLEAR_ERR();
    EAS_LAUNCH(time_mean_kernel, dim3(lif_grid(M)), dim3(EAS_BLOCK), 0, eas_s(stream), x, out, T, M);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

}  // extern "C"
