// K21: one acting step of the imitation-learning collection loop (core.learn / core.evaluate of
// examples/imitation_learning/experiment.py:51-57): GaussianTorchPolicy.draw_action on the policy of
// examples/imitation_learning/utils.py:126-134 and _preprocess_action's control vector, in one call:
//
//   oly_il_act   [oly_col_stats in accumulate mode: Standardizer.update_mean_std, networks.py:76-81]
//                act_kernel: standardise (fp64), mean network in -> 512 -> 256 -> act on the f32 matrix cores, the
//                Gaussian sample mu + exp(log_sigma) eps, and the clamped controls in actuator order.
//
// The act launch is K16's forward (ilmlp_common.h: 256 threads, 16-row sub-tiles, tiles<>, the packed stream, the same
// row-tile choice) with another epilogue, so every pre-activation is the same fma chain and mu has oly_ilmlp_forward's
// bits.  The output-layer waves write mu / action and stage the action tile in LDS over the input image (dead after
// layer 1); after a barrier all 256 threads form the control rows from it: actuator j gathers action column
// ctrl_src[j], which with act_dim > 16 another wave computed.  The control expression is il_ctrl_kernel's
// (k1_il_step.hip): fp64 un-normalise, clamp, narrow.
#include "ilmlp_common.h"
#include "oly_common.h"

namespace {
using namespace oly_ilmlp;

struct ActArgs {
  long N;
  int in_dim, act_dim;
  const float* x;
  const double* colstats;
  const float* packed;
  const float* log_sigma;
  const float* eps;
  float* action;
  float* mu;
  void* ctrl;          // NULL: no controls
  const IlDev* md;     // the configured model (read only when ctrl is given)
};

template <int RS, int G1, bool CTRL64>
__global__ __launch_bounds__(FWD_THREADS) void act_kernel(ActArgs p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xT = lds;                                   // [RS][64 x 16]   input images; later the action tile [16 RS][32]
  float* hA = xT + (size_t)RS * IN_MAX * 16;         // [RS][512 x 16]  layer-1 images
  float* hB = hA + (size_t)RS * H1 * 16;             // [RS][256 x 16]  layer-2 images
  double* s_mean = reinterpret_cast<double*>(hB + (size_t)RS * H2 * 16);
  double* s_sd = s_mean + IN_MAX;
  static_assert(16 * OUT_MAX <= IN_MAX * 16, "the action tile fits the input image");
  const float* __restrict__ P = p.packed;
  const float4* P4 = reinterpret_cast<const float4*>(P);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long row0 = (long)blockIdx.x * (16 * RS);
  const int in_dim = p.in_dim;

  if (tid < in_dim) {   // Standardizer.update_mean_std's derivation (networks.py:54-56,76-81), as K16
    const double* cs = p.colstats;
    const double cnt = cs[tid] + 1e-2;
    const double mean = cs[in_dim + tid] / cnt;
    s_mean[tid] = mean;
    s_sd[tid] = sqrt(fmax((cs[2 * in_dim + tid] + 1e-2) / cnt - mean * mean, 1e-2));
  }
  __syncthreads();
  for (int e = tid; e < RS * 16 * IN_MAX; e += FWD_THREADS) {
    const int s = e / (16 * IN_MAX), m = (e / IN_MAX) & 15, k = e & (IN_MAX - 1);
    const long row = row0 + 16 * s + m;
    float v = 0.f;
    // f32((f64(x) - mean) / std): the reference subtracts fp64 statistics and narrows afterwards (networks.py:68-74)
    if (row < p.N && k < in_dim) v = (float)(((double)p.x[row * in_dim + k] - s_mean[k]) / s_sd[k]);
    xT[(size_t)s * IN_MAX * 16 + act16_index(k, m)] = v;
  }
  __syncthreads();
  {  // ---- layer 1: [16 RS, in] x [in, 512]
    f32x4 acc[RS][8];
#pragma unroll
    for (int s = 0; s < RS; ++s)
#pragma unroll
      for (int t = 0; t < 8; ++t) acc[s][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float4* a4[RS];
#pragma unroll
    for (int s = 0; s < RS; ++s) a4[s] = reinterpret_cast<const float4*>(xT + (size_t)s * IN_MAX * 16);
    tiles<G1, 8, RS>(a4, P4 + P_W1 / 4 + (size_t)(8 * wave) * (IN_MAX / 16) * 64, (IN_MAX / 16) * 64, lane, acc);
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const float bv = P[P_B1 + 16 * (8 * wave + t) + (lane & 15)];
#pragma unroll
      for (int s = 0; s < RS; ++s) store_act16v<false>(acc[s][t], bv, 8 * wave + t, lane, hA + (size_t)s * H1 * 16);
    }
  }
  __syncthreads();
  {  // ---- layer 2: [16 RS, 512] x [512, 256]
    f32x4 acc[RS][4];
#pragma unroll
    for (int s = 0; s < RS; ++s)
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[s][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float4* a4[RS];
#pragma unroll
    for (int s = 0; s < RS; ++s) a4[s] = reinterpret_cast<const float4*>(hA + (size_t)s * H1 * 16);
    tiles<H1 / 16, 4, RS>(a4, P4 + P_W2 / 4 + (size_t)(4 * wave) * (H1 / 16) * 64, (H1 / 16) * 64, lane, acc);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float bv = P[P_B2 + 16 * (4 * wave + t) + (lane & 15)];
#pragma unroll
      for (int s = 0; s < RS; ++s) store_act16v<false>(acc[s][t], bv, 4 * wave + t, lane, hB + (size_t)s * H2 * 16);
    }
  }
  __syncthreads();
  // ---- output layer: [16, 256] x [256, 16] per (sub-tile, column tile) pair; mu, the sample, the action tile in LDS
  float* sA = xT;                                    // [16 RS][OUT_MAX]: row-major action rows of this workgroup
  const int nt3 = p.act_dim > 16 ? 2 : 1;
  if (wave < RS * nt3) {
    const int s = wave / nt3, t = wave - s * nt3;
    f32x4 acc[1][1] = {{f32x4{0.f, 0.f, 0.f, 0.f}}};
    const float4* a4[1] = {reinterpret_cast<const float4*>(hB + (size_t)s * H2 * 16)};
    tiles<H2 / 16, 1, 1>(a4, P4 + P_W3 / 4 + (size_t)t * (H2 / 16) * 64, 0, lane, acc);
    const int col = 16 * t + (lane & 15);
    if (col < p.act_dim) {
      const float bv = P[P_B3 + col];
      const float sigma = p.eps ? expf(p.log_sigma[col]) : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int rl = 16 * s + 4 * (lane >> 4) + i;
        const long row = row0 + rl;
        if (row < p.N) {
          const float m = acc[0][0][i] + bv;
          float a = m;
          if (p.eps) {
            const float se = sigma * p.eps[row * p.act_dim + col];
            a = m + se;
          }
          if (p.mu) p.mu[row * p.act_dim + col] = m;
          p.action[row * p.act_dim + col] = a;
          sA[rl * OUT_MAX + col] = a;
        }
      }
    }
  }
  if (!p.ctrl) return;                               // uniform over the launch
  __syncthreads();
  // ---- controls: un-normalise in fp64, clamp to ctrlrange, actuator order (il_ctrl_kernel's expression)
  const IlDev* __restrict__ md = p.md;
  const int nu = md->nu;
  const long left = p.N - row0;
  const int rows = left < 16 * RS ? (int)left : 16 * RS;
  for (int e = tid; e < rows * nu; e += FWD_THREADS) {
    const int r = e / nu, j = e - r * nu;
    const int k = md->ctrl_src[j];
    double u = 0.0;
    if (k >= 0) {
      u = (double)sA[r * OUT_MAX + k] * md->act_delta[k] + md->act_mean[k];
      if (u < md->ctrl_lo[k]) u = md->ctrl_lo[k];
      if (u > md->ctrl_hi[k]) u = md->ctrl_hi[k];
    }
    const long o = (row0 + r) * nu + j;
    if (CTRL64)
      static_cast<double*>(p.ctrl)[o] = u;
    else
      static_cast<float*>(p.ctrl)[o] = (float)u;
  }
}

template <int RS, bool CTRL64>
int launch_act(oly_ctx* ctx, const ActArgs& a, oly_stream stream) {
  const int G = (a.in_dim + 15) / 16;
  const unsigned bit = 1u << (8 * (RS - 1) + 4 * (CTRL64 ? 1 : 0) + (G - 1));
  const dim3 grid((unsigned)((a.N + 16 * RS - 1) / (16 * RS)));
  const size_t lds = fwd_lds<RS>();
  switch (G) {
#define OLY_ILACT_CASE(G)                                                                                             \
  case G:                                                                                                             \
    if (!(ctx->ilact_attr_done & bit)) {                                                                              \
      OLY_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(act_kernel<RS, G, CTRL64>),                      \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                        \
      ctx->ilact_attr_done |= bit;                                                                                    \
    }                                                                                                                 \
    hipLaunchKernelGGL((act_kernel<RS, G, CTRL64>), grid, dim3(FWD_THREADS), lds, oly_s(stream), a);                  \
    break;
    OLY_ILACT_CASE(1)
    OLY_ILACT_CASE(2)
    OLY_ILACT_CASE(3)
    OLY_ILACT_CASE(4)
#undef OLY_ILACT_CASE
  }
  OLY_LAUNCH_CHECK(ctx, "act_kernel");
  return OLY_OK;
}
}  // namespace

extern "C" int oly_il_act(oly_ctx* ctx, const oly_il_act_args* f, oly_stream stream) {
  if (!ctx) return OLY_EINVAL;
  if (!f) OLY_FAIL(ctx, OLY_EINVAL, "oly_il_act: NULL argument block");
  if (f->n < 1 || f->in_dim < 1 || f->in_dim > IN_MAX || f->act_dim < 1 || f->act_dim > OUT_MAX)
    OLY_FAIL(ctx, OLY_EINVAL, "oly_il_act: supported: n >= 1, 0 < in_dim <= %d, 0 < act_dim <= %d (got n %d, in %d, act %d)",
             IN_MAX, OUT_MAX, f->n, f->in_dim, f->act_dim);
  if (!f->x || !f->colstats || !f->packed || !f->log_sigma || !f->action)
    OLY_FAIL(ctx, OLY_EINVAL, "oly_il_act: NULL x / colstats / packed / log_sigma / action");
  if ((reinterpret_cast<uintptr_t>(f->packed) & 15) != 0) OLY_FAIL(ctx, OLY_EINVAL, "oly_il_act: packed must be 16-byte aligned");
  if (f->ctrl && !ctx->il_ok) OLY_FAIL(ctx, OLY_EINVAL, "oly_il_act: ctrl requested before oly_il_configure");
  if (f->ctrl && ctx->il_host.n_act != f->act_dim)
    OLY_FAIL(ctx, OLY_EINVAL, "oly_il_act: ctrl requested for act_dim %d, the configured model has n_act %d", f->act_dim,
             ctx->il_host.n_act);
  if (f->update_stats) {   // Standardizer.update_mean_std before the forward (networks.py:70)
    const int rc = oly_col_stats(ctx, f->n, f->in_dim, f->x, f->colstats, 1, stream);
    if (rc != OLY_OK) return rc;
  }
  const ActArgs a{(long)f->n, f->in_dim, f->act_dim, f->x, f->colstats, f->packed, f->log_sigma, f->eps, f->action,
                  f->mu,      f->ctrl,   ctx->il_dev};
  // the row-tile choice of oly_ilmlp_forward: 16-row tiles while 32-row tiles would leave CUs without a second workgroup
  const long slots = 2L * (ctx->num_cu > 0 ? ctx->num_cu : 256);
  const bool c64 = f->ctrl && (f->out_flags & OLY_OUT_CTRL_F64);
  if ((a.N + 31) / 32 < slots) return c64 ? launch_act<1, true>(ctx, a, stream) : launch_act<1, false>(ctx, a, stream);
  return c64 ? launch_act<2, true>(ctx, a, stream) : launch_act<2, false>(ctx, a, stream);
}
