// Activation values and derivatives of the FFN passes (actdrop.hip, biasgrad.hip): one copy, so that every kernel that applies
// act'(x) rounds it the same way.
#pragma once
#include "common.h"
#include "kernels.h"

// The pass is as much instruction-bound as memory-bound (an element has ~30 VALU slots at the HBM rate), so the
// transcendental forms are the cheap ones: one v_exp_f32 and one v_rcp_f32 per element.
//   erf form:  Phi(x) = 1 - h (x >= 0), h (x < 0),  h = 0.5 * poly(t) * exp(-x^2 / 2),  t = 1 / (1 + p |x| / sqrt(2))
//              (Abramowitz & Stegun 7.1.26: |error of erf| <= 1.5e-7), and the same exponential is the density of the derivative;
//   tanh form: 0.5 (1 + tanh(u)) = 1 / (1 + exp(-2 u)).
struct GeluParts { float cdf, e; };           // Phi(x) and exp(-x^2 / 2)
__device__ __forceinline__ GeluParts gelu_erf_parts(float x) {
    const float ax = __builtin_fabsf(x);
    const float t = __builtin_amdgcn_rcpf(__builtin_fmaf(0.3275911f * 0.7071067811865476f, ax, 1.0f));
    const float e = __builtin_amdgcn_exp2f(-0.5f * 1.4426950408889634f * x * x);
    float q = __builtin_fmaf(1.061405429f, t, -1.453152027f);
    q = __builtin_fmaf(q, t, 1.421413741f);
    q = __builtin_fmaf(q, t, -0.284496736f);
    q = __builtin_fmaf(q, t, 0.254829592f);
    const float h = 0.5f * q * t * e;
    return {x >= 0.f ? 1.0f - h : h, e};
}
__device__ __forceinline__ float sigmoid_fast(float v) {      // 1 / (1 + exp(-v)); exp overflow -> 1 / inf = 0
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * v));
}

template <int ACT> __device__ __forceinline__ float act_f(float x) {
    if constexpr (ACT == VLPET_ACT_RELU) return x > 0.f ? x : 0.f;
    else if constexpr (ACT == VLPET_ACT_GELU_NEW) {
        const float u = 0.7978845608028654f * (x + 0.044715f * x * x * x);
        return x * sigmoid_fast(2.0f * u);
    } else return x * gelu_erf_parts(x).cdf;
}
// The derivative with every rounding point written out (no contraction left to the compiler: whether it fuses a product into the
// following sum depends on how the surrounding kernel was vectorised, and two kernels that must store the same bits -- actdrop.hip's
// backward and biasgrad.hip's column-summing one -- would otherwise differ in the last place).
template <int ACT> __device__ __forceinline__ float act_df(float x) {
#pragma clang fp contract(off)
    if constexpr (ACT == VLPET_ACT_RELU) return x > 0.f ? 1.f : 0.f;
    else if constexpr (ACT == VLPET_ACT_GELU_NEW) {
        const float x2 = x * x;
        const float u = 0.7978845608028654f * __builtin_fmaf(0.044715f * x, x2, x);
        // sg = 0.5 (1 + tanh u) = 1 / (1 + e), e = exp(-2 u);  1 - tanh^2 u = 4 sg (1 - sg), with 1 - sg formed as e sg: the
        // difference 1.0f - sg cancels for x > 0 down to the last bits of sg (x = 4: 1 - sg = 1.8e-5 known to 6e-8, 0.4 % of the
        // term, 7e-7 of the derivative -- tests/test_gpu_act.py value sweep).  e sg <= 1; e = inf gives inf * 0, which the min drops.
        const float e = __builtin_amdgcn_exp2f(-1.4426950408889634f * (2.0f * u));
        const float sg = __builtin_amdgcn_rcpf(1.0f + e);     // = sigmoid_fast(2 u)
        const float om = __builtin_fminf(e * sg, 1.0f);
        return __builtin_fmaf(x * 2.0f * sg * om * 0.7978845608028654f, __builtin_fmaf(0.134145f, x2, 1.0f), sg);
    } else {
        const float ax = __builtin_fabsf(x);
        const float t = __builtin_amdgcn_rcpf(__builtin_fmaf(0.3275911f * 0.7071067811865476f, ax, 1.0f));
        const float e = __builtin_amdgcn_exp2f(-0.5f * 1.4426950408889634f * x * x);
        float q = __builtin_fmaf(1.061405429f, t, -1.453152027f);
        q = __builtin_fmaf(q, t, 1.421413741f);
        q = __builtin_fmaf(q, t, -0.284496736f);
        q = __builtin_fmaf(q, t, 0.254829592f);
        const float ht = 0.5f * q * t;
        const float cdf = x >= 0.f ? __builtin_fmaf(-ht, e, 1.0f) : ht * e;      // 1 - h in one rounding
        return __builtin_fmaf(x * 0.3989422804014327f, e, cdf);
    }
}
