// K25: the squashed-Gaussian policy's act and log-probability (IQ_Learn_Policy.compute_action_and_log_prob_t,
// imitation_lib/imitation/iq_sac.py:102-151) in one call:
//
//   oly_sg_act   [oly_col_stats in accumulate mode: Standardizer.update_mean_std, networks.py:76-81]
//                sg_act_kernel: standardise (fp64), the network in -> 512 -> 256 -> 2A on the f32 matrix cores, the split
//                into mu | log_sigma and the clamp, the sample, tanh, the action, the log-probability per row and the
//                clamped controls in actuator order.
//
// The launch is K16's forward (ilmlp_common.h: 256 threads, 16-row sub-tiles, tiles<>, the packed stream, the same
// row-tile choice) with another epilogue, as K21's (k21_il_act.hip): every pre-activation is the same fma chain, so mu
// and the clamped log_sigma have oly_ilmlp_forward's bits.  The mu / log_sigma boundary lies inside the first output
// tile for A < 16 and the two halves of a row may sit in different waves, so the output-layer waves stage the raw
// outputs in LDS over the input image (dead after layer 1); after a barrier one thread per (row, action) forms the
// sample, the action and the two fp64 terms of the log-probability (in layer 1's image, dead after layer 2); after a
// second barrier one thread per row adds the terms with j in order and all threads form the control rows from the
// action tile (il_ctrl_kernel's expression, k1_il_step.hip).
//
// With oly_sg_act_args' trailing fields (the inverse action model's draw, K28) the kernel is instantiated over
// oly_sg::PairArgs: the staging loop reads row i of two tables, i = idx[r] or r, and the action is clipped in fp64
// before it is stored.  Everything else is the same text, so the outputs have the bits of the call on materialised rows.
#include <type_traits>

#include "ilmlp_common.h"
#include "oly_common.h"
#include "sg_act.h"

namespace {
using namespace oly_ilmlp;
using oly_sg::Args;
using oly_sg::PairArgs;

constexpr int MAX_ACT = OLY_BC_MAX_ACT;
constexpr double HALF_LOG_2PI = 0.5 * 1.8378770664093454835606594728112;
static_assert(2 * MAX_ACT <= OUT_MAX, "2A output columns");

template <int RS, int G1, class KA>
__global__ __launch_bounds__(FWD_THREADS) void sg_act_kernel(KA p) {
  constexpr bool PAIR = std::is_same<KA, PairArgs>::value;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xT = lds;                                   // [RS][64 x 16]   input images; later raw outputs and the action tile
  float* hA = xT + (size_t)RS * IN_MAX * 16;         // [RS][512 x 16]  layer-1 images; later the log-probability's terms
  float* hB = hA + (size_t)RS * H1 * 16;             // [RS][256 x 16]  layer-2 images
  double* s_mean = reinterpret_cast<double*>(hB + (size_t)RS * H2 * 16);
  double* s_sd = s_mean + IN_MAX;
  static_assert(16 * OUT_MAX + 16 * MAX_ACT <= IN_MAX * 16, "the raw outputs and the action tile fit the input image");
  static_assert(2 * 16 * MAX_ACT * sizeof(double) <= H1 * 16 * sizeof(float), "the terms fit layer 1's image");
  const float* __restrict__ P = p.packed;
  const float4* P4 = reinterpret_cast<const float4*>(P);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long row0 = (long)blockIdx.x * (16 * RS);
  const int in_dim = p.in_dim, A = p.act_dim;
  const bool standardise = p.colstats != nullptr;

  if (tid < in_dim && standardise) {   // Standardizer.update_mean_std's derivation (networks.py:54-56,76-81), as K16
    const double* cs = p.colstats;
    double cnt, sum, sq;
    if (p.extra) {                     // the statistics with a minibatch's rows taken in once more (the logged fit)
      cnt = cs[tid] + p.extra_cnt + 1e-2;
      sum = cs[in_dim + tid] + p.extra[tid];
      sq = cs[2 * in_dim + tid] + p.extra[IN_MAX + tid];
    } else {
      cnt = cs[tid] + 1e-2;
      sum = cs[in_dim + tid];
      sq = cs[2 * in_dim + tid];
    }
    const double mean = sum / cnt;
    s_mean[tid] = mean;
    s_sd[tid] = sqrt(fmax((sq + 1e-2) / cnt - mean * mean, 1e-2));
  }
  __syncthreads();
  for (int e = tid; e < RS * 16 * IN_MAX; e += FWD_THREADS) {
    const int s = e / (16 * IN_MAX), m = (e / IN_MAX) & 15, k = e & (IN_MAX - 1);
    const long row = row0 + 16 * s + m;
    float v = 0.f;
    if (row < p.N && k < in_dim) {
      long src = row;
      if (p.rows) {
        const int i = p.rows[row];
        src = i < 0 ? 0 : i >= p.n_rows ? p.n_rows - 1 : i;
      }
      float xv;
      if constexpr (PAIR)
        xv = k < p.d1 ? p.x[src * p.stride1 + k] : p.x2[src * p.stride2 + (k - p.d1)];
      else
        xv = p.x[src * in_dim + k];
      // f32((f64(x) - mean) / std): the reference subtracts fp64 statistics and narrows afterwards (networks.py:68-74)
      v = standardise ? (float)(((double)xv - s_mean[k]) / s_sd[k]) : xv;
    }
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
  // ---- output layer: [16, 256] x [256, 16] per (sub-tile, column tile) pair; the raw outputs by row into LDS
  float* sZ = xT;                                    // [16 RS][OUT_MAX] raw outputs
  float* sA = xT + (size_t)RS * 16 * OUT_MAX;        // [16 RS][MAX_ACT] actions
  double* sT = reinterpret_cast<double*>(hA);        // [2][16 RS][MAX_ACT] the Gaussian term, the tanh correction
  const int nt3 = 2 * A > 16 ? 2 : 1;
  if (wave < RS * nt3) {
    const int s = wave / nt3, t = wave - s * nt3;
    f32x4 acc[1][1] = {{f32x4{0.f, 0.f, 0.f, 0.f}}};
    const float4* a4[1] = {reinterpret_cast<const float4*>(hB + (size_t)s * H2 * 16)};
    tiles<H2 / 16, 1, 1>(a4, P4 + P_W3 / 4 + (size_t)t * (H2 / 16) * 64, 0, lane, acc);
    const int col = 16 * t + (lane & 15);
    const float bv = P[P_B3 + col];
#pragma unroll
    for (int i = 0; i < 4; ++i) sZ[(16 * s + 4 * (lane >> 4) + i) * OUT_MAX + col] = acc[0][0][i] + bv;
  }
  __syncthreads();
  const long left = p.N - row0;
  const int rows = left < 16 * RS ? (int)left : 16 * RS;
  for (int e = tid; e < rows * A; e += FWD_THREADS) {   // ---- thread (row r, action j)
    const int r = e / A, j = e - r * A;
    const long o = (row0 + r) * A + j;
    const float m = sZ[r * OUT_MAX + j];
    const float ls = fminf(fmaxf(sZ[r * OUT_MAX + A + j], p.ls_min), p.ls_max);       // iq_sac.py:146
    float a_raw = m;
    if (p.eps) {
      const float se = expf(ls) * p.eps[o];
      a_raw = m + se;
    }
    const double th = tanh((double)a_raw);
    float act = p.delta ? (float)th * p.delta[j] + p.central[j] : 0.f;   // no bounds: the logged fit (no action)
    if constexpr (PAIR) {
      if (p.clip_lo) {     // np.clip(action, low, high) against float64 bounds (lsiqfo.py:90); a NaN passes through
        double v = (double)act;
        v = v < p.clip_lo[j] ? p.clip_lo[j] : v;
        v = v > p.clip_hi[j] ? p.clip_hi[j] : v;
        act = (float)v;
      }
    }
    if (p.mu) p.mu[o] = m;
    if (p.log_sigma) p.log_sigma[o] = ls;
    if (p.action) p.action[o] = act;
    sA[r * MAX_ACT + j] = act;
    if (p.log_prob) {
      const double sg = exp((double)ls), d = (double)a_raw - (double)m;
      sT[r * MAX_ACT + j] = -(d * d) / (2.0 * sg * sg) - (double)ls - HALF_LOG_2PI;   // Normal(mu, sigma).log_prob(a_raw)
      sT[(16 * RS + r) * MAX_ACT + j] = log(1.0 - th * th + 1e-6);                      // iq_sac.py:124
    }
  }
  if (!p.log_prob && !p.ctrl) return;                // uniform over the launch
  __syncthreads();
  if (p.log_prob && tid < rows) {                    // the row's two sums, actions in order
    double g = 0.0, c = 0.0;
    for (int j = 0; j < A; ++j) {
      g += sT[tid * MAX_ACT + j];
      c += sT[(16 * RS + tid) * MAX_ACT + j];
    }
    p.log_prob[row0 + tid] = (float)(g - c);
  }
  if (!p.ctrl) return;
  // ---- controls: un-normalise in fp64, clamp to ctrlrange, actuator order (il_ctrl_kernel's expression)
  const IlDev* __restrict__ md = p.md;
  const int nu = md->nu;
  for (int e = tid; e < rows * nu; e += FWD_THREADS) {
    const int r = e / nu, j = e - r * nu;
    const int k = md->ctrl_src[j];
    double u = 0.0;
    if (k >= 0) {
      u = (double)sA[r * MAX_ACT + k] * md->act_delta[k] + md->act_mean[k];
      if (u < md->ctrl_lo[k]) u = md->ctrl_lo[k];
      if (u > md->ctrl_hi[k]) u = md->ctrl_hi[k];
    }
    const long o = (row0 + r) * nu + j;
    if (p.ctrl64)
      static_cast<double*>(p.ctrl)[o] = u;
    else
      static_cast<float*>(p.ctrl)[o] = (float)u;
  }
}

template <int RS, class KA>
int launch_rs(oly_ctx* ctx, const KA& a, oly_stream stream) {
  const int G = (a.in_dim + 15) / 16;
  const unsigned bit = 1u << ((std::is_same<KA, PairArgs>::value ? 8 : 0) + 4 * (RS - 1) + (G - 1));
  const dim3 grid((unsigned)((a.N + 16 * RS - 1) / (16 * RS)));
  const size_t lds = fwd_lds<RS>();
  switch (G) {
#define OLY_SGACT_CASE(G)                                                                                             \
  case G:                                                                                                             \
    if (!(ctx->sgact_attr_done & bit)) {                                                                              \
      OLY_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(sg_act_kernel<RS, G, KA>),                       \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                        \
      ctx->sgact_attr_done |= bit;                                                                                    \
    }                                                                                                                 \
    hipLaunchKernelGGL((sg_act_kernel<RS, G, KA>), grid, dim3(FWD_THREADS), lds, oly_s(stream), a);                   \
    break;
    OLY_SGACT_CASE(1)
    OLY_SGACT_CASE(2)
    OLY_SGACT_CASE(3)
    OLY_SGACT_CASE(4)
#undef OLY_SGACT_CASE
  }
  OLY_LAUNCH_CHECK(ctx, "sg_act_kernel");
  return OLY_OK;
}

template <class KA>
int launch_any(oly_ctx* ctx, const KA& a, oly_stream stream) {
  // the row-tile choice of oly_ilmlp_forward: 16-row tiles while 32-row tiles would leave CUs without a second workgroup
  const long slots = 2L * (ctx->num_cu > 0 ? ctx->num_cu : 256);
  if ((a.N + 31) / 32 < slots) return launch_rs<1>(ctx, a, stream);
  return launch_rs<2>(ctx, a, stream);
}
}  // namespace

int oly_sg::launch(oly_ctx* ctx, const Args& a, oly_stream stream) { return launch_any(ctx, a, stream); }
int oly_sg::launch(oly_ctx* ctx, const PairArgs& a, oly_stream stream) { return launch_any(ctx, a, stream); }

extern "C" int oly_sg_act(oly_ctx* ctx, const oly_sg_act_args* f, oly_stream stream) {
  if (!ctx) return OLY_EINVAL;
  if (!f) OLY_FAIL(ctx, OLY_EINVAL, "oly_sg_act: NULL argument block");
  if (f->n < 1 || f->in_dim < 1 || f->in_dim > IN_MAX || f->act_dim < 1 || f->act_dim > MAX_ACT)
    OLY_FAIL(ctx, OLY_EINVAL, "oly_sg_act: supported: n >= 1, 0 < in_dim <= %d, 0 < act_dim <= %d (got n %d, in %d, act %d)",
             IN_MAX, MAX_ACT, f->n, f->in_dim, f->act_dim);
  if (!f->x || !f->packed || !f->central || !f->delta || !f->action)
    OLY_FAIL(ctx, OLY_EINVAL, "oly_sg_act: NULL x / packed / central / delta / action");
  if (f->update_stats && !f->colstats) OLY_FAIL(ctx, OLY_EINVAL, "oly_sg_act: update_stats without colstats");
  if ((reinterpret_cast<uintptr_t>(f->packed) & 15) != 0) OLY_FAIL(ctx, OLY_EINVAL, "oly_sg_act: packed must be 16-byte aligned");
  if (!(f->log_std_min <= f->log_std_max)) OLY_FAIL(ctx, OLY_EINVAL, "oly_sg_act: log_std_min <= log_std_max is required");
  if (f->ctrl && !ctx->il_ok) OLY_FAIL(ctx, OLY_EINVAL, "oly_sg_act: ctrl requested before oly_il_configure");
  if (f->ctrl && ctx->il_host.n_act != f->act_dim)
    OLY_FAIL(ctx, OLY_EINVAL, "oly_sg_act: ctrl requested for act_dim %d, the configured model has n_act %d", f->act_dim,
             ctx->il_host.n_act);
  const bool paired = f->x2 || f->d2 || f->stride1 || f->stride2 || f->idx || f->clip_lo || f->clip_hi;
  if (paired) {
    const int d2 = f->d2, d1 = f->in_dim - d2;
    if (d2 < 0 || d2 >= f->in_dim) OLY_FAIL(ctx, OLY_EINVAL, "oly_sg_act: d2 %d outside [0, in_dim %d)", d2, f->in_dim);
    if ((d2 > 0) != (f->x2 != nullptr)) OLY_FAIL(ctx, OLY_EINVAL, "oly_sg_act: x2 and d2 > 0 go together (d2 %d)", d2);
    if ((f->stride1 != 0 && f->stride1 < d1) || f->stride2 < d2)
      OLY_FAIL(ctx, OLY_EINVAL, "oly_sg_act: a stride below its width (stride1 %d, d1 %d; stride2 %d, d2 %d)", f->stride1, d1,
               f->stride2, d2);
    if (f->idx && f->n_rows < 1) OLY_FAIL(ctx, OLY_EINVAL, "oly_sg_act: idx with n_rows %d (>= 1)", f->n_rows);
    if ((f->clip_lo != nullptr) != (f->clip_hi != nullptr))
      OLY_FAIL(ctx, OLY_EINVAL, "oly_sg_act: one clip bound without the other");
  }
  if (f->update_stats && !paired) {   // Standardizer.update_mean_std before the forward (networks.py:70)
    const int rc = oly_col_stats(ctx, f->n, f->in_dim, f->x, f->colstats, 1, stream);
    if (rc != OLY_OK) return rc;
  }
  PairArgs pa{};
  Args& a = pa;
  a.N = f->n;
  a.in_dim = f->in_dim;
  a.act_dim = f->act_dim;
  a.x = f->x;
  a.colstats = f->colstats;
  a.packed = f->packed;
  a.ls_min = f->log_std_min;
  a.ls_max = f->log_std_max;
  a.central = f->central;
  a.delta = f->delta;
  a.eps = f->eps;
  a.action = f->action;
  a.log_prob = f->log_prob;
  a.mu = f->mu;
  a.log_sigma = f->log_sigma;
  a.ctrl = f->ctrl;
  a.ctrl64 = f->ctrl && (f->out_flags & OLY_OUT_CTRL_F64);
  a.md = ctx->il_dev;
  if (!paired) return oly_sg::launch(ctx, a, stream);
  pa.rows = f->idx;
  pa.n_rows = f->n_rows;
  pa.d1 = f->in_dim - f->d2;
  pa.stride1 = f->stride1 ? f->stride1 : pa.d1;
  pa.stride2 = f->stride2;
  pa.x2 = f->x2;
  pa.clip_lo = f->clip_lo;
  pa.clip_hi = f->clip_hi;
  if (f->update_stats) {
    const int rc = oly_sg::col_stats_pair(ctx, f->n, pa, f->colstats, stream);
    if (rc != OLY_OK) return rc;
  }
  return oly_sg::launch(ctx, pa, stream);
}
