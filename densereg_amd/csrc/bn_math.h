// bn_math.h -- the element formulas of train-mode BatchReNorm, ONE definition each for the forward passes, every backward pass
// (train_kernels.h) and the sums fused into a reader's input-gradient launch (conv_epilogue.inc).
// Plain expressions under the translation unit's default contraction: the backward mask [bn_affine > 0] equals the sign of what the
// forward pass stored because both are THIS expression, compiled the same way -- give it no pragma and no explicit fmaf.
#pragma once
#include "dr_platform.h"

namespace dr {

// out (before the ReLU) = x*scale + shift, the folded form of gamma*(r*yhat + d) + beta
__device__ __forceinline__ float bn_affine(float x, float sc, float sh) { return x * sc + sh; }
// yhat = (x - mean) * inv_std
__device__ __forceinline__ float bn_yhat(float x, float mean, float istd) { return (x - mean) * istd; }
// dx = c1*(g - c2 - yhat*c3) with c1 = gamma*r*inv_std, c2 = mean(g), c3 = mean(g*yhat) (bn_bwd_coefs)
__device__ __forceinline__ float bn_dx(float c1, float c2, float c3, float g, float yh) { return c1 * (g - c2 - yh * c3); }

}  // namespace dr
