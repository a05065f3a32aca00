// fp64 normal-distribution functions of the probit link, shared by
// ame_binary.hip (the working network) and ame_predict.hip (MODE 3 scoring).
// One formula each, so both kernels and the reference (tests/probit_ref.py)
// agree on the branch a value takes.
#pragma once
#include "ame_common.h"

#define AME_SQRT1_2 0.70710678118654752440     // 1 / sqrt(2)
#define AME_SQRT_2_PI 0.79788456080286535588   // sqrt(2 / pi)

// kappa(x) = phi(x) / Phi(x) = sqrt(2 / pi) / erfcx(-x / sqrt 2) and log Phi(x):
// log(erfcx(-x / sqrt 2) / 2) - x^2 / 2 for x < 0, log1p(-erfc(x / sqrt 2) / 2)
// otherwise.  Finite for every finite x (kappa underflows to 0 for large x).
__device__ __forceinline__ void ame_probit_kl(double x, double& kappa, double& logphi) {
    const double t = x * AME_SQRT1_2;
    const double ex = erfcx(-t);
    kappa = AME_SQRT_2_PI / ex;
    logphi = x < 0.0 ? log(0.5 * ex) - 0.5 * x * x : log1p(-0.5 * erfc(t));
}
__device__ __forceinline__ double ame_probit_logphi(double x) {
    const double t = x * AME_SQRT1_2;
    return x < 0.0 ? log(0.5 * erfcx(-t)) - 0.5 * x * x : log1p(-0.5 * erfc(t));
}
// Phi(x)
__device__ __forceinline__ double ame_probit_phi(double x) { return 0.5 * erfc(-x * AME_SQRT1_2); }
