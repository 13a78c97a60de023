// The activations of ConvLayer (reference networks/cnn.py:128-147: ReLU, LeakyReLU(0.2), SELU, GELU, SiLU) and their derivatives as
// device functions: ONE definition for every kernel that applies them unfused (activation.hip, film_act.hip, groupnorm.hip), so that the same
// input gives the same bits whichever kernel it passes through.  `kind` is an ACT_KINDS value of functional.py.
#pragma once
#include <hip/hip_runtime.h>

#define ACT_NONE 0
#define ACT_RELU 1
#define ACT_LEAKY 2   // LeakyReLU(0.2)
#define ACT_SELU 3
#define ACT_GELU 4    // exact (erf) form: nn.GELU() default
#define ACT_SILU 5

#define SELU_ALPHA 1.6732632423543772848170429916717f
#define SELU_SCALE 1.0507009873554804934193349852946f

__device__ __forceinline__ float act_fwd(float u, int kind) {
    switch (kind) {
        case ACT_RELU: return fmaxf(u, 0.f);
        case ACT_LEAKY: return u > 0.f ? u : 0.2f * u;
        case ACT_SELU: return SELU_SCALE * (u > 0.f ? u : SELU_ALPHA * expm1f(u));
        case ACT_GELU: return 0.5f * u * (1.f + erff(u * 0.70710678118654752440f));
        case ACT_SILU: return u / (1.f + expf(-u));
        default: return u;
    }
}

// d act / d u (torch's conventions at u == 0: ReLU 0, LeakyReLU the slope, SELU the exponential branch)
__device__ __forceinline__ float act_grad(float u, int kind) {
    switch (kind) {
        case ACT_RELU: return u > 0.f ? 1.f : 0.f;
        case ACT_LEAKY: return u > 0.f ? 1.f : 0.2f;
        case ACT_SELU: return u > 0.f ? SELU_SCALE : SELU_SCALE * SELU_ALPHA * expf(u);
        case ACT_GELU: {
            const float cdf = 0.5f * (1.f + erff(u * 0.70710678118654752440f));
            const float pdf = 0.39894228040143267794f * expf(-0.5f * u * u);
            return cdf + u * pdf;
        }
        case ACT_SILU: {
            const float s = 1.f / (1.f + expf(-u));
            return s * (1.f + u * (1.f - s));
        }
        default: return 1.f;
    }
}
