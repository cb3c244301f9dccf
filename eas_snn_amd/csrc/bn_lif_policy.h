// Launch-time policy of the BN+LIF backward kernels (bn_lif.hip).
//
// The surrogate, the reset form (attached / detached) and the presence of the optional operands (grad_mean, v_init, the broadcast input
// frame) are the same for every thread of a launch.  The generic kernel body decides them at every neuron-step through scalar compares
// and branches around the code of all four surrogates; a policy makes them template constants, so that an instance carries the code of
// ONE surrogate and no launch-uniform branch in its loop.
//
// The compile-time forms below are the runtime forms of eas_common.h (eas_surrogate_grad(int, ...), eas_lif_step_bwd(..., int sg_id, ...)),
// expression by expression and in the same order of evaluation: with -ffp-contract=off every instance rounds like the generic body, and a
// fast instance equals the generic one bit for bit (tests/test_gpu_bn_lif_bwd_instances.py).  The runtime forms stay for the generic
// instance and for lif.hip / arsnn.hip.
#pragma once
#include "eas_common.h"

#define EAS_SG_RUNTIME (-1)      // surrogate id of the generic policy: decided per step from the launch argument

// SG: EAS_SG_ATAN .. EAS_SG_PATAN, or EAS_SG_RUNTIME (then DETACH is not read: the generic body takes everything from its arguments)
// DETACH: detached reset (EAS_LIF_DETACH_RESET)
// In the two-pass kernels a fast policy (SG >= 0) also means plain operands: grad_s present, no grad_mean, no v_init, no broadcast input
// frame.  Channel slices (gs_ctot / y_ctot) are plain: a fast instance addresses every operand through its channel count, sliced or not.
// The one-pass kernel reads its optional operands once per thread in front of its passes; its fast instances take every operand form.
template <int SG, bool DETACH>
struct BnLifBwdPolicy {
    static constexpr int sg = SG;
    static constexpr bool detach = DETACH;
    static constexpr bool fast = SG != EAS_SG_RUNTIME;
};
typedef BnLifBwdPolicy<EAS_SG_RUNTIME, false> BnLifBwdGeneric;

// surrogate gradient g'(u), u = h - v_th: eas_surrogate_grad with the id as a template constant
template <int SG>
__device__ __forceinline__ float eas_surrogate_grad_ct(float alpha, float u) {
    if constexpr (SG == EAS_SG_ATAN || SG == EAS_SG_PATAN) {
        const float q = 1.57079632679489661923f * alpha * u;
        return alpha * 0.5f * __builtin_amdgcn_rcpf(1.0f + q * q);
    } else if constexpr (SG == EAS_SG_SIGMOID) {
        const float sg = eas_sigmoidf(alpha * u);
        return (1.0f - sg) * sg * alpha;
    } else {
        static_assert(SG == EAS_SG_RECT, "unknown surrogate");
        return (fabsf(u) < 0.5f / alpha) ? alpha : 0.0f;
    }
}

// eas_lif_step_bwd with the surrogate and the reset form as template constants (same contract, same expressions)
template <bool HARD, bool DI, bool STRICT, int SG, bool DETACH>
__device__ __forceinline__ float eas_lif_step_bwd_ct(float gs, float& gv, float h, float v_prev, float x, float k, float omk, float v_th,
                                                     float v_reset, float alpha, float& dk_term, float& gx, float& da) {
    const float u = h - v_th;
    const float s = STRICT ? (u > 0.0f ? 1.0f : 0.0f) : (u >= 0.0f ? 1.0f : 0.0f);
    const float sg = eas_surrogate_grad_ct<SG>(alpha, u);
    if constexpr (SG == EAS_SG_PATAN) {
        const float q = 1.57079632679489661923f * alpha * u;
        const float gs_all = DETACH ? gs : (HARD ? gs + gv * (v_reset - h) : gs - gv * v_th);
        da += gs_all * (0.5f * u * __builtin_amdgcn_rcpf(1.0f + q * q));
    }
    float dvdh;
    if (HARD) {
        dvdh = DETACH ? (1.0f - s) : (1.0f - s) + (v_reset - h) * sg;
    } else {
        dvdh = DETACH ? 1.0f : 1.0f - v_th * sg;
    }
    const float dh = gs * sg + gv * dvdh;
    if (DI) {
        gx = dh * k;
        dk_term = dh * (HARD ? (x - (v_prev - v_reset)) : (x - v_prev));
    } else {
        gx = dh;
        dk_term = dh * ((HARD && v_reset != 0.0f) ? -(v_prev - v_reset) : -v_prev);
    }
    gv = dh * omk;
    return dh;
}
