// pika_amd/csrc/ctc_numerics.h -- the "log zero" arithmetic shared by ctc_loss.hip, ctc_decode.hip and ctc_lm.hip (not
// part of the C ABI).
#ifndef PIKA_CTC_NUMERICS_H
#define PIKA_CTC_NUMERICS_H

#include <hip/hip_runtime.h>

namespace {

constexpr float NEG = -1.0e30f;  // "log zero": finite, so NEG+NEG / NEG-NEG never make NaN
constexpr float NEG_HALF = -0.5e30f;
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

typedef float v4f __attribute__((ext_vector_type(4)));

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ inline float addn(float a, float b) { return fmaxf(a + b, NEG); }

// log(exp(x)+exp(y)) on the transcendental pipe; NEG when both are "log zero"
__device__ inline float lse2(float x, float y) {
    const float m = fmaxf(x, y);
    if (!(m > NEG_HALF)) return NEG;
    const float e = __builtin_amdgcn_exp2f((x - m) * LOG2E) + __builtin_amdgcn_exp2f((y - m) * LOG2E);
    return m + LN2 * __builtin_amdgcn_logf(e);
}

}  // namespace

#endif
