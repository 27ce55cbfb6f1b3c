// Pieces of the fused discriminator forward (K12, csrc/k12_disc_forward.hip) that the discriminator's fit (K15,
// csrc/k15_disc_fit.hip) shares: the packed operand stream's layout and the float32 exp of the reparameterisation; and the pieces GAIL's
// discriminator (K18, csrc/k18_gail_disc.hip) shares with them: the reward formula and the float32 tanh.
#pragma once
#include "oly_common.h"

namespace oly_disc {
constexpr int H1 = 256;          // encoder hidden width
constexpr int H2 = 128;          // encoder output width
constexpr int ZD = 128;          // latent width
constexpr int MAX_IN = 64;

struct DiscLayout {
  int in_dim, g1;                // g1: groups of four k-steps (8 k values) in layer 1: 4 (in <= 32) or 8
  size_t w0, b0, w1, b1, wmu, bmu, wlv, blv, wd, bd;
  // the same matrices as 16-column-tile streams (mlp_tiles.h: P16[tile][group of 16 k][lane][4]) for the 16-row
  // kernel that small batches take
  size_t w0n, w1n, wmun, wlvn;
  size_t total;
};
constexpr int G1N16 = MAX_IN / 16;   // 16-wide layout, layer 1: 4 groups of 16 k (zero beyond in_dim)

__host__ __device__ inline DiscLayout disc_layout(int in_dim) {
  DiscLayout L;
  L.in_dim = in_dim;
  L.g1 = in_dim <= 32 ? 4 : 8;
  L.w0 = 0;
  L.b0 = L.w0 + (size_t)(H1 / 32) * L.g1 * 256;
  L.w1 = L.b0 + H1;
  L.b1 = L.w1 + (size_t)(H2 / 32) * (H1 / 8) * 256;
  L.wmu = L.b1 + H2;
  L.bmu = L.wmu + (size_t)(ZD / 32) * (H2 / 8) * 256;
  L.wlv = L.bmu + ZD;
  L.blv = L.wlv + (size_t)(ZD / 32) * (H2 / 8) * 256;
  L.wd = L.blv + ZD;
  L.bd = L.wd + ZD;
  L.w0n = L.bd + 4;
  L.w1n = L.w0n + (size_t)(H1 / 16) * G1N16 * 256;
  L.wmun = L.w1n + (size_t)(H2 / 16) * (H1 / 16) * 256;
  L.wlvn = L.wmun + (size_t)(ZD / 16) * (H2 / 16) * 256;
  L.total = L.wlvn + (size_t)(ZD / 16) * (H2 / 16) * 256;
  return L;
}

// What every paired entry point (oly_disc_pair: the discriminator's second part) refuses before a launch, or NULL.
// Ds: the first part's width.
inline const char* pair_error(const oly_disc_pair* pr, int Ds) {
  if (!pr->x2 || pr->d2 <= 0 || pr->stride2 <= 0) return "NULL x2, or d2 / stride2 not positive";
  if (Ds + pr->d2 > MAX_IN) return "the two parts are wider than 64 columns together";
  if (!pr->mask2 && pr->d2 > pr->stride2) return "d2 exceeds stride2 and there is no mask2";
  if (pr->standardise && pr->d2 != Ds) return "a standardised second part (next states) has the first part's width";
  return nullptr;
}

// exp in float32 from fma / rint / exponent arithmetic only, so that the oracle's copy returns the same bits:
// n = rint(x log2 e), r = x - n ln2 (two-constant Cody-Waite), e^r = 1 + (r + r^2 P(r)) with a degree-5 minimax
// P, result scaled by 2^n in two exact steps.  Within 1 ulp of exp over the whole float range (checked
// against fp64 exp by tests/test_oracle_golden.py), the error class of torch's own float32 exp.
__device__ __forceinline__ float pow2i(int e) { return __int_as_float((e + 127) << 23); }
// the reduction and the polynomial: n = rint(x log2 e) and e^(x - n ln2), which exp32 and tanh32 scale by 2^n
__device__ __forceinline__ float exp_reduced(float x, float& n) {
  n = rintf(x * 1.4426950408889634f);
  float r = fmaf(n, -0.693145751953125f, x);
  r = fmaf(n, -1.428606765330187045e-06f, r);
  float u = 0.000198527617612853646278381f;
  u = fmaf(u, r, 0.00139304355252534151077271f);
  u = fmaf(u, r, 0.00833336077630519866943359f);
  u = fmaf(u, r, 0.0416664853692054748535156f);
  u = fmaf(u, r, 0.166666671633720397949219f);
  u = fmaf(u, r, 0.5f);
  return 1.0f + fmaf(r * r, u, r);
}
__device__ __forceinline__ float exp32(float x) {
  if (x != x) return x;
  if (x > 88.72283935546875f) return __int_as_float(0x7f800000);
  if (x < -103.97208404541016f) return 0.f;
  float n;
  const float u = exp_reduced(x, n);
  const int q = (int)n, q1 = q >> 1;
  return (u * pow2i(q1)) * pow2i(q - q1);
}

// make_discrim_reward's formula (gail_TRPO.py:320-327), -log(1 - sigmoid(d) + 1e-8), for the elementwise reward kernel
// (K8) and the fused GAIL forward (K18).
__device__ __forceinline__ float reward_of(float d) {
  // numpy evaluates every step in float32 (gail_TRPO.py:320-327 on the network's float32 output), and so
  // does this: expf / logf are the <= 1 ulp device functions, the same class of error as numpy's own
  // float32 exp / log; the 1 - p cancellation amplifies either to the tolerance the tests state.
  // (Round 1 took exp / log in fp64: 27 % of the HBM peak, fp64-transcendental-bound.)
  const float e = expf(-d);
  const float p = 1.0f / (1.0f + e);
  const float q = 1.0f - p + 1e-8f;
  return -logf(q);
}

// tanh in float32, the hidden activation of GAIL's discriminator (K18: the reward forward and the fit's forward both
// call it, so they produce the same hidden values).  Branch-free, since a wave of hidden units always holds both kinds
// of argument.  |x| < 0.25 (and NaN): the odd Taylor polynomial through x^9 (the first dropped term is below 1e-8 of
// the result).  Otherwise 1 - 2 / (exp(2 |x|) + 1) with exp32's reduction and polynomial (no range checks are needed:
// 2 |x| is clamped to 18.04, where the result has rounded to 1), one exact scaling by 2^n and the hardware reciprocal
// (1 ulp); the subtraction loses at most two bits (the quotient is below 0.76).  Measured against fp64 tanh over 5e7
// arguments in [-12, 12]: at most 5.6 ulp, at |x| just above 0.25; 0.5 ulp below 0.01.
__device__ __forceinline__ float tanh32(float x) {
  const float ax = fabsf(x), s = x * x;
  float u = 62.0f / 2835.0f;
  u = fmaf(u, s, -17.0f / 315.0f);
  u = fmaf(u, s, 2.0f / 15.0f);
  u = fmaf(u, s, -1.0f / 3.0f);
  const float small = fmaf(x * s, u, x);
  float n;
  const float e = exp_reduced(2.0f * fminf(ax, 9.02f), n) * pow2i((int)n);          // n in [0, 27]
  const float big = fmaf(-2.0f, __builtin_amdgcn_rcpf(e + 1.0f), 1.0f);
  return ax >= 0.25f ? copysignf(big, x) : small;
}

}  // namespace oly_disc
