// K27: the policy and temperature update of the SAC-family imitation agents, IQ_SAC.update_policy with _actor_loss and
// _update_alpha (imitation_lib/imitation/iq_sac.py:431-465, 587-595; SQIL's iq_update has the same lines inline,
// imitation_lib/imitation/sqil_sac.py:16-62).  The policy is IQ_Learn_Policy's FullyConnectedNetwork(in -> [512, 256] ->
// 2A, relu / relu / identity), the critic FullyConnectedNetwork((obs | act) -> [512, 256] -> 1); each has its own
// Standardizer (imitation_lib/utils/networks.py:68-81).
//
//   oly_iq_pi_update   one update.  With a policy Standardizer oly_col_stats adds the rows to it first (its launches and
//                      its summation order: the statistics, and so the action and the log-probability, have oly_sg_act's
//                      bits).  Then five launches:
//   P   iqpi_prologue_kernel  the transposed streams of the policy's W2 and W3 and of the critic's W2 (the B operands of
//                             the data gradients, fit_common.h's pt_index), the A action columns of the critic's W1.
//   A1  iqpi_act_kernel       one 16-row tile per workgroup (8 waves): standardise, the policy's forward on the f32 matrix
//                             cores in the forward kernel's chain order (ilmlp_common.h), K25's epilogue (the sample, the
//                             correctly rounded tanh, the action, the fp64 log-probability).  xs, h1, h2 go to the
//                             workspace in row quads, the raw outputs and the sample u by row; the tile's fp64 column sums of
//                             (x | a_new) to fixed slots.
//   A2  iqpi_grad_kernel      same tiling.  The critic's statistics WITH all the rows of (x | a_new) from the tiles' slots
//                             in slot order (this is why A1 and A2 are two launches: a_new of every row comes first), the
//                             critic's forward (Q has oly_ilmlp_forward's bits), its data gradients only (the critic's
//                             parameters do not step: dZ2 = f32(-1 / Bp) W3 [h2 > 0], dZ1 on the matrix cores over the
//                             transposed stream, dX on the action columns divided by the column's std), the chain through
//                             the squash and the sample in fp64 per element narrowed once, then K24's policy backward.
//   B   iqpi_weights_kernel   ilmlp_fit.h's launch B (weight_tile, dw_accumulate, meet_waves, tile_step,
//                             gradnorm_partial) over the policy's weights: dW, weight decay, Adam, the
//                             stepped value into param, the moments and the packed stream; the tile's sum of squared
//                             gradients to a fixed slot.
//   F   iqpi_fold_kernel      one workgroup: the four scalars, the critic's Standardizer += the rows.
//   oly_iq_alpha_update  one launch of one workgroup: the fp64 mean of log_prob + target_entropy (thread t adds rows t,
//                        t + 256, ..., a halving tree joins them), Adam on the scalar log_alpha.
// Every reduction has a fixed order and there are no atomics: two runs give identical bits.
//
// The loss: mean(alpha log_prob - q).  The reference's critic has squeeze_out=False, so q is [Bp, 1] against log_prob
// [Bp] and the difference broadcasts to [Bp, Bp]; its mean and its gradient are the row-wise ones up to float32 rounding,
// and the row-wise ones are what is computed here.  With u = mu + sigma eps, a = tanh(u), a_new = a delta + central:
//   dL/du_j          = [alpha 2 a (1 - a^2) / (1 - a^2 + 1e-6) - dq/da_new_j delta_j (1 - a^2)] / Bp
//   dL/dmu_j         = dL/du_j
//   dL/dlog_sigma_j  = dL/du_j sigma eps - alpha / Bp, 0 where the clamp cuts (inclusive mask)
// (the Normal's quadratic term is eps^2 / 2: it carries no gradient).
//
// LSIQ_H / LSIQ_HC's _actor_loss (imitation_lib/imitation/lsiq_h.py:104-108) is mean(alpha log_prob - (q + H)) over TWO live
// critics on the same rows (x | a_new), each standardised with its own Standardizer, which the call updates by the Bp rows.
// With h_packed set P also builds H's transposed W2 stream and its action columns of W1 in the second workspace h_ws (the
// layout of the first, of which cw2t, cw1a and qv are used), A2 runs in instantiations of its own (iqpi_grad_kernel<GC,
// true>): the critic's forward and data gradients, then H's, each net's dX on an action column divided by THAT net's std
// of the column in fp64 and added, the critic's first, before the chain; F adds the rows to both Standardizers and
// reports mean(q + H) with q + H formed in float32 as the reference's soft_q.  Neither critic's parameters are written.
#include <cstdlib>

#include "ilmlp_fit.h"
#include "oly_common.h"

namespace {
using namespace oly_ilfit;
using oly_fit::adam1;

constexpr int MAX_BATCH = OLY_BC_MAX_BATCH;
constexpr int MAX_ACT = OLY_BC_MAX_ACT;
constexpr int OUTP = OUT_MAX;
constexpr double HALF_LOG_2PI = 0.5 * 1.8378770664093454835606594728112;
static_assert(MAX_BATCH <= 16 * THREADS && 2 * MAX_ACT <= OUTP && MAX_ACT == 16, "tiles per fold thread; 2A output columns");

// workspace (floats), BP = batch rounded up to 16 rows; [BP][W] arrays in row quads, element (row, col) at
// ((row / 4) W + col) 4 + row % 4:
//   xs [BP][64] | h1 [BP][512] | h2 [BP][256] | dZ1 [BP][512] | dZ2 [BP][256] | dZ3 [BP][32] (the policy's, row quads) |
//   the policy's raw outputs zr [BP][32] and the samples u th [BP][16] by row | Q qv [BP] | loss partials [BP / 16][4] f64 |
//   the tiles' column sums of (x | a_new) [BP / 16][2][64] f64 | their total [2][64] f64 | gradient-norm partials
//   [weight tiles] f64 | the transposed streams W2T, W3T (policy), W2T (critic) | the critic's W1 action columns [16][512]
struct WsL {
  size_t xs, h1, h2, dz1, dz2, dz3, zr, th, qv, lossp, cpart, cdelta, gnp, w2t, w3t, cw2t, cw1a, total;
};
constexpr int MAX_WTILES = 32 * (IN_MAX / 16) + 512 + 32;
__host__ __device__ inline WsL ws_layout(int batch) {
  const size_t BP = (size_t)(batch + 15) / 16 * 16;
  WsL W;
  W.xs = 0;
  W.h1 = W.xs + BP * IN_MAX;
  W.h2 = W.h1 + BP * H1;
  W.dz1 = W.h2 + BP * H2;
  W.dz2 = W.dz1 + BP * H1;
  W.dz3 = W.dz2 + BP * H2;
  W.zr = W.dz3 + BP * OUTP;
  W.th = W.zr + BP * OUTP;
  W.qv = W.th + BP * MAX_ACT;
  W.lossp = W.qv + BP;
  W.cpart = W.lossp + BP / 16 * 4 * 2;
  W.cdelta = W.cpart + BP / 16 * 2 * IN_MAX * 2;
  W.gnp = W.cdelta + 2 * IN_MAX * 2;
  W.w2t = W.gnp + (size_t)MAX_WTILES * 2;
  W.w3t = W.w2t + (size_t)H2 * H1;
  W.cw2t = W.w3t + (size_t)OUTP * H2;
  W.cw1a = W.cw2t + (size_t)H2 * H1;
  W.total = W.cw1a + (size_t)MAX_ACT * H1;
  return W;
}

struct PiArgs {
  int in_dim, act_dim, out_dim, D, B;
  const float *x, *eps, *central, *delta;
  const double* colstats;      // the policy's, the rows already in (oly_col_stats), or NULL
  double* ccolstats;           // the critic's, or NULL
  float *param, *m, *v, *packed, *ws;
  const float *cpacked, *cparam;
  float *action, *log_prob;
  const float *hpacked, *hparam;   // LSIQ_H's second critic H (NULL: one critic), its statistics and its workspace
  double* hcolstats;
  float* hws;
  float alpha, ls_min, ls_max, coef;   // coef: f32(-1 / Bp), dL/dq of every row
  oly_fit::AdamK ad;
  float wd;
  double* out;
  ParamLayout P, CP;           // the policy's (in, 2A) and the critic's (D, 1)
  WsL W;
};

// grid PRO_BLOCKS, grid-stride
__global__ __launch_bounds__(THREADS) void iqpi_prologue_kernel(PiArgs a) {
  build_w2t(a);
  const int g0 = blockIdx.x * THREADS + threadIdx.x, gs = PRO_BLOCKS * THREADS;
  for (int e = g0; e < OUTP * H2; e += gs)
    a.ws[a.W.w3t + pt_index(OUTP, e / H2, e % H2)] = e / H2 < a.out_dim ? a.param[a.P.w3 + e] : 0.f;
  for (int e = g0; e < H2 * H1; e += gs) a.ws[a.W.cw2t + pt_index(H2, e / H1, e % H1)] = a.cparam[a.CP.w2 + e];
  for (int e = g0; e < MAX_ACT * H1; e += gs) {
    const int j = e / H1, n = e % H1;
    a.ws[a.W.cw1a + e] = j < a.act_dim ? a.cparam[a.CP.w1 + (size_t)n * a.D + a.in_dim + j] : 0.f;
  }
  if (!a.hparam) return;               // H's streams, into its own workspace
  for (int e = g0; e < H2 * H1; e += gs) a.hws[a.W.cw2t + pt_index(H2, e / H1, e % H1)] = a.hparam[a.CP.w2 + e];
  for (int e = g0; e < MAX_ACT * H1; e += gs) {
    const int j = e / H1, n = e % H1;
    a.hws[a.W.cw1a + e] = j < a.act_dim ? a.hparam[a.CP.w1 + (size_t)n * a.D + a.in_dim + j] : 0.f;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Launch A1.  RTHREADS = 512 threads = 8 waves, the chains of ilmlp_fit.h.
constexpr size_t A1_LDS_FLOATS = (size_t)(IN_MAX + H1 + H2) * 16 + 16 * OUTP + 16 * MAX_ACT;
constexpr size_t A1_LDS = sizeof(float) * A1_LDS_FLOATS + sizeof(double) * (2 * IN_MAX + 2 * 16 * MAX_ACT);
static_assert(A1_LDS_FLOATS % 4 == 0, "the fp64 arrays must be 8-byte aligned");

template <int G1>
__global__ __launch_bounds__(RTHREADS) void iqpi_act_kernel(PiArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xT = lds;                       // [64 x 16]   standardised input (act16 images, mlp_tiles.h)
  float* hA = xT + IN_MAX * 16;          // [512 x 16]  h1
  float* hB = hA + H1 * 16;              // [256 x 16]  h2
  float* z3 = hB + H2 * 16;              // [16][32]    the raw outputs by row
  float* sA = z3 + 16 * OUTP;            // [16][16]    the actions by row
  double* st = reinterpret_cast<double*>(lds + A1_LDS_FLOATS);   // [2][IN_MAX] mean, std
  double* sT = st + 2 * IN_MAX;          // [2][16][16] the Gaussian term, the tanh correction
  const float* P = a.packed;
  const float4* P4 = reinterpret_cast<const float4*>(P);
  const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, h4 = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row0 = blockIdx.x * 16, B = a.B, in_dim = a.in_dim, A = a.act_dim;
  const int rows = min(16, B - row0);
  const bool standardise = a.colstats != nullptr;
  float* ws = a.ws;
  float4* ws4 = reinterpret_cast<float4*>(ws);
  const size_t quad = (size_t)(row0 >> 2) + h4;

  if (standardise && tid < in_dim) {   // the statistics hold the rows already; K25's derivation
    double mean, sd;
    col_moments(a.colstats[tid], a.colstats[in_dim + tid], a.colstats[2 * in_dim + tid], mean, sd);
    st[tid] = mean;
    st[IN_MAX + tid] = sd;
  }
  __syncthreads();
  stage_rows(xT, in_dim, standardise, st, [&](int m) { return m < rows; },
             [&](int m, int k) { return a.x[(size_t)(row0 + m) * in_dim + k]; }, true, ws + a.W.xs, row0);
  __syncthreads();
  hidden_layer<Relu, G1, IN_MAX / 16, 4, P_W1, P_B1>(xT, P, hA, true, ws4, a.W.h1, quad);
  __syncthreads();
  hidden_layer<Relu, H1 / 16, H1 / 16, 2, P_W2, P_B2>(hA, P, hB, true, ws4, a.W.h2, quad);
  __syncthreads();
  if (wave < (a.out_dim > 16 ? 2 : 1)) {  // ---- the output layer's column tile `wave`: one chain over k < 256
    f32x4 acc[1][1] = {{f32x4{0.f, 0.f, 0.f, 0.f}}};
    const float4* a4[1] = {reinterpret_cast<const float4*>(hB)};
    tiles<H2 / 16, 1, 1>(a4, P4 + P_W3 / 4 + (size_t)wave * (H2 / 16) * 64, 0, lane, acc);
    const int col = 16 * wave + c;
    const float bv = P[P_B3 + col];
#pragma unroll
    for (int i = 0; i < 4; ++i) z3[(4 * h4 + i) * OUTP + col] = acc[0][0][i] + bv;
  }
  __syncthreads();
  if (tid < rows * A) {   // ---- thread (row r, action j): K25's epilogue (k25_sg_act.hip), expression for expression
    const int r = tid / A, j = tid - r * A;
    const size_t row = (size_t)row0 + r, o = row * A + j;
    const float m = z3[r * OUTP + j], raw = z3[r * OUTP + A + j];
    const float ls = fminf(fmaxf(raw, a.ls_min), a.ls_max);                         // iq_sac.py:146
    const float se = expf(ls) * a.eps[o];
    const float a_raw = m + se;
    const double th = tanh((double)a_raw);
    const float act = (float)th * a.delta[j] + a.central[j];
    a.action[o] = act;
    sA[r * MAX_ACT + j] = act;
    const double sg = exp((double)ls), d = (double)a_raw - (double)m;
    sT[r * MAX_ACT + j] = -(d * d) / (2.0 * sg * sg) - (double)ls - HALF_LOG_2PI;      // Normal(mu, sigma).log_prob(a_raw)
    sT[(16 + r) * MAX_ACT + j] = log(1.0 - th * th + 1e-6);                            // iq_sac.py:124
    ws[a.W.zr + row * OUTP + j] = m;
    ws[a.W.zr + row * OUTP + A + j] = raw;
    ws[a.W.th + row * MAX_ACT + j] = a_raw;
  }
  __syncthreads();
  if (tid < rows) {                    // the row's two sums, actions in order
    double g = 0.0, cc = 0.0;
    for (int j = 0; j < A; ++j) {
      g += sT[tid * MAX_ACT + j];
      cc += sT[(16 + tid) * MAX_ACT + j];
    }
    a.log_prob[row0 + tid] = (float)(g - cc);
  }
  if (tid >= 64 && tid < 64 + a.D) {   // the tile's column sums of (x | a_new), rows in order
    const int k = tid - 64;
    double s = 0.0, ss = 0.0;
    for (int r = 0; r < rows; ++r) {
      const double v = k < in_dim ? a.x[(size_t)(row0 + r) * in_dim + k] : sA[r * MAX_ACT + (k - in_dim)];
      s += v;
      ss += v * v;
    }
    double* cp = reinterpret_cast<double*>(ws + a.W.cpart) + (size_t)blockIdx.x * 2 * IN_MAX;
    cp[k] = s;
    cp[IN_MAX + k] = ss;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Launch A2.  The critic's forward and data gradients, the chain through the squash, the policy's backward.
constexpr size_t A2_LDS_FLOATS = (size_t)(IN_MAX + H1 + 2 * H2) * 16 + OUTP * 16 + 2 * 16 * MAX_ACT;
constexpr size_t A2_LDS = sizeof(float) * A2_LDS_FLOATS + sizeof(double) * (2 * IN_MAX);
constexpr size_t A2H_LDS = A2_LDS + sizeof(double) * 16 * MAX_ACT;     // two critics: the critic's dX / std by (row, action)
static_assert(A2_LDS_FLOATS % 4 == 0, "the fp64 arrays must be 8-byte aligned");

template <int GC, bool HB = false>
__global__ __launch_bounds__(RTHREADS) void iqpi_grad_kernel(PiArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xT = lds;                       // [64 x 16]   the critic's standardised input
  float* hA = xT + IN_MAX * 16;          // [512 x 16]  the critic's h1, then its dZ1 in place
  float* hB = hA + H1 * 16;              // [256 x 16]  the critic's h2
  float* gz = hB + H2 * 16;              // [256 x 16]  the critic's dZ2, then the policy's
  float* gz3 = gz + H2 * 16;             // [32 x 16]   the policy's dZ3
  float* dxp = gz3 + OUTP * 16;          // [2][16][16] the halves of dX by (row, action)
  double* st = reinterpret_cast<double*>(lds + A2_LDS_FLOATS);   // [2][IN_MAX] mean, std of the critic's columns
  double* dq = st + 2 * IN_MAX;          // HB: [16][16] the critic's dX / std, while H's pass runs
  __shared__ float zq[16];
  __shared__ float zh[16];               // HB: H's raw outputs by row
  const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, h4 = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row0 = blockIdx.x * 16, B = a.B, in_dim = a.in_dim, A = a.act_dim, D = a.D;
  const int rows = min(16, B - row0);
  float* ws = a.ws;
  float4* ws4 = reinterpret_cast<float4*>(ws);
  const size_t quad = (size_t)(row0 >> 2) + h4;
  gz3[tid] = 0.f;                        // RTHREADS = 32 x 16
  static_assert(RTHREADS == OUTP * 16, "one thread per element of the dZ3 image");

#pragma unroll
  for (int net = 0; net < (HB ? 2 : 1); ++net) {   // the critic, then (HB) H: the same rows, each net's own statistics
  const float* CPk = net ? a.hpacked : a.cpacked;
  const float* cparam = net ? a.hparam : a.cparam;
  const double* ccol = net ? a.hcolstats : a.ccolstats;
  const float* nws = net ? a.hws : ws;             // where P left this net's cw2t and cw1a
  const bool standardise = ccol != nullptr;
  if (tid < D) {   // Standardizer.update_mean_std with all Bp rows of (x | a_new) (networks.py:76-81): the tiles' slots in order
    const double* cp = reinterpret_cast<const double*>(ws + a.W.cpart);
    double s = 0.0, ss = 0.0;
    for (int t = 0; t < (int)gridDim.x; ++t) {
      s += cp[(size_t)t * 2 * IN_MAX + tid];
      ss += cp[(size_t)t * 2 * IN_MAX + IN_MAX + tid];
    }
    if (blockIdx.x == 0 && net == 0) {
      double* d = reinterpret_cast<double*>(ws + a.W.cdelta);
      d[tid] = s;
      d[IN_MAX + tid] = ss;
    }
    double mean = 0.0, sd = 1.0;
    if (standardise) col_moments(ccol[tid] + (double)B, ccol[D + tid] + s, ccol[2 * D + tid] + ss, mean, sd);
    st[tid] = mean;
    st[IN_MAX + tid] = sd;
  }
  __syncthreads();
  stage_rows(xT, D, standardise, st, [&](int m) { return m < rows; },
             [&](int m, int k) {
               const size_t row = (size_t)row0 + m;
               return k < in_dim ? a.x[row * in_dim + k] : a.action[row * A + (k - in_dim)];
             }, false, nullptr, 0);
  __syncthreads();
  // ---- the critic's forward: no activations kept (its parameters do not step)
  hidden_layer<Relu, GC, IN_MAX / 16, 4, P_W1, P_B1>(xT, CPk, hA, false, ws4, 0, quad);
  __syncthreads();
  hidden_layer<Relu, H1 / 16, H1 / 16, 2, P_W2, P_B2>(hA, CPk, hB, false, ws4, 0, quad);
  __syncthreads();
  output_unit(hB, CPk, net ? zh : zq, (net ? a.hws : ws) + a.W.qv + row0);
  {  // ---- the critic's dZ2 = (f32(-1 / Bp) W3) [h2 > 0], zero beyond the batch
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int col = 16 * (2 * wave + t) + c;
      const float w3 = cparam[a.CP.w3 + col];
      const float4 h = get_quad(hB, col, h4);
      const float g0 = a.coef * w3;
      float4 g;
      g.x = h.x > 0.f && 4 * h4 < rows ? g0 : 0.f;
      g.y = h.y > 0.f && 4 * h4 + 1 < rows ? g0 : 0.f;
      g.z = h.z > 0.f && 4 * h4 + 2 < rows ? g0 : 0.f;
      g.w = h.w > 0.f && 4 * h4 + 3 < rows ? g0 : 0.f;
      put_quad(gz, col, h4, g);
    }
  }
  __syncthreads();
  {  // ---- the critic's dZ1 = (dZ2 W2) [h1 > 0] over the transposed stream, written over h1 by the thread that read it
    f32x4 acc[1][4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[0][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float4* a4[1] = {reinterpret_cast<const float4*>(gz)};
    tiles<H2 / 16, 4, 1>(a4, reinterpret_cast<const float4*>(nws) + (a.W.cw2t >> 2) + (size_t)(4 * wave) * (H2 / 16) * 64,
                         (H2 / 16) * 64, lane, acc);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int col = 16 * (4 * wave + t) + c;
      const float4 h = get_quad(hA, col, h4);
      float4 g;
      g.x = Relu::back(acc[0][t][0], h.x);
      g.y = Relu::back(acc[0][t][1], h.y);
      g.z = Relu::back(acc[0][t][2], h.z);
      g.w = Relu::back(acc[0][t][3], h.w);
      put_quad(hA, col, h4, g);
    }
  }
  __syncthreads();
  {  // ---- dX on the action columns: thread (row m, action j, half hf) one fma chain over its 256 units in order
    const int m = tid >> 5, j = (tid >> 1) & 15, hf = tid & 1;
    const float* w = nws + a.W.cw1a + (size_t)j * H1;
    float s = 0.f;
    for (int n = hf * (H1 / 2); n < (hf + 1) * (H1 / 2); ++n) s = fmaf(hA[act16_index(n, m)], w[n], s);
    dxp[(hf * 16 + m) * MAX_ACT + j] = s;
  }
  __syncthreads();
  if (HB && net == 0) {   // the critic's dX / std_Q in fp64, kept while H's pass reuses dxp and st
    if (tid < 256) dq[tid] = (tid & 15) < A ? (double)(dxp[tid] + dxp[256 + tid]) / st[IN_MAX + in_dim + (tid & 15)] : 0.0;
    __syncthreads();
  }
  }   // net
  if (tid < 256) {  // ---- the chain through the action's bounds, the squash and the sample: thread (row m, action j), fp64
    const int m = tid >> 4, j = tid & 15;
    if (m < rows && j < A) {
      const size_t row = (size_t)row0 + m;
      const double Bd = (double)B, al = (double)a.alpha;
      // d(q [+ H])/da_new: each net's dX over that net's std of the column, the critic's term first
      double dxa = (double)(dxp[m * MAX_ACT + j] + dxp[(16 + m) * MAX_ACT + j]) / st[IN_MAX + in_dim + j];
      if (HB) dxa = dq[m * MAX_ACT + j] + dxa;
      const double th = tanh((double)ws[a.W.th + row * MAX_ACT + j]);   // from the stored sample u, as A1 formed it
      const float raw = ws[a.W.zr + row * OUTP + A + j];
      const float ls = fminf(fmaxf(raw, a.ls_min), a.ls_max);
      const double one = 1.0 - th * th;
      const double du = al * (2.0 * th * one / (one + 1e-6)) / Bd + dxa * (double)a.delta[j] * one;
      gz3[act16_index(j, m)] = (float)du;
      gz3[act16_index(A + j, m)] = (raw >= a.ls_min && raw <= a.ls_max)
                                       ? (float)(du * exp((double)ls) * (double)a.eps[row * A + j] - al / Bd)
                                       : 0.f;
    }
  }
  __syncthreads();
  {  // the policy's dZ3 for launch B: all 32 columns of all 16 rows (zeros beyond the batch and the 2A columns)
    const int m = tid >> 5, col = tid & (OUTP - 1);
    ws[a.W.dz3 + ((size_t)((row0 + m) >> 2) * OUTP + col) * 4 + (m & 3)] = gz3[act16_index(col, m)];
  }
  if (tid < 3) {    // this tile's loss partials, rows in order: alpha log_prob - q, log_prob, q
    double s = 0.0;
    for (int r = 0; r < rows; ++r) {
      const double lp = (double)a.log_prob[row0 + r], q = (double)(HB ? zq[r] + zh[r] : zq[r]);   // soft_q = q + H in float32
      s += tid == 0 ? (double)a.alpha * lp - q : tid == 1 ? lp : q;
    }
    reinterpret_cast<double*>(ws + a.W.lossp)[(size_t)blockIdx.x * 4 + tid] = s;
  }
  {  // ---- the policy's dZ2 = (dZ3 W3) [h2 > 0] from the stored h2
    f32x4 acc[1][2];
#pragma unroll
    for (int t = 0; t < 2; ++t) acc[0][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float4* a4[1] = {reinterpret_cast<const float4*>(gz3)};
    tiles<OUTP / 16, 2, 1>(a4, reinterpret_cast<const float4*>(ws) + (a.W.w3t >> 2) + (size_t)(2 * wave) * (OUTP / 16) * 64,
                           (OUTP / 16) * 64, lane, acc);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int col = 16 * (2 * wave + t) + c;
      const float4 h = ws4[(a.W.h2 >> 2) + quad * H2 + col];
      float4 g;
      g.x = Relu::back(acc[0][t][0], h.x);
      g.y = Relu::back(acc[0][t][1], h.y);
      g.z = Relu::back(acc[0][t][2], h.z);
      g.w = Relu::back(acc[0][t][3], h.w);
      put_quad(gz, col, h4, g);
      ws4[(a.W.dz2 >> 2) + quad * H2 + col] = g;
    }
  }
  __syncthreads();
  // ---- the policy's dZ1 = (dZ2 W2) [h1 > 0] from the stored h1
  dz1_tiles<Relu>(gz, reinterpret_cast<const float4*>(ws) + (a.W.w2t >> 2),
                  [&](int col) { return ws4[(a.W.h1 >> 2) + quad * H1 + col]; }, ws4, a.W.dz1, quad);
}

// ---------------------------------------------------------------------------------------------------------------
// Launch B (the tiles: weight_tiles, ilmlp_fit.h; W3 is (1 or 2) x 16): ilmlp_fit.h's phases, the step Adam and the re-pack.
__global__ __launch_bounds__(THREADS) void iqpi_weights_kernel(PiArgs a) {
  __shared__ float red[4 * 256];
  __shared__ float bred[4 * 64];
  __shared__ double dred[THREADS];
  __shared__ double bsq[16];
  const WeightTile T = weight_tile(a, a.in_dim, a.out_dim, OUTP);
  f32x4 acc;
  float bsum;
  dw_accumulate(T.dl, T.al, T.dw, T.aw, T.n0, T.N, T.k0, T.K, (a.B + 15) / 16, acc, bsum);
  meet_waves(red, bred, acc, bsum);
  double g2, b2;
  tile_step(T, a, a.in_dim, red, bred, [&](int, int, int, size_t i, size_t pk, float g) { a.packed[pk] = adam1(a, i, g); },
            g2, b2);
  gradnorm_partial(dred, bsq, g2, b2, reinterpret_cast<double*>(a.ws + a.W.gnp));
}

// Launch F: one workgroup.  Thread j < 3 adds loss partial j of the tiles in order; thread t adds the gradient-norm
// partials t, t + 256, ... and a halving tree joins them; thread 0 writes the four scalars; threads < D add the rows'
// column sums to the critic's Standardizer.
__global__ __launch_bounds__(THREADS) void iqpi_fold_kernel(PiArgs a, int tiles_a, int tiles_b) {
  __shared__ double S[3];
  __shared__ double dred[THREADS];
  const int tid = threadIdx.x, D = a.D;
  if (tid < 3) {
    const double* lp = reinterpret_cast<const double*>(a.ws + a.W.lossp);
    double s = 0.0;
    for (int t = 0; t < tiles_a; ++t) s += lp[(size_t)t * 4 + tid];
    S[tid] = s;
  }
  const double gn2 = gradnorm_total(dred, reinterpret_cast<const double*>(a.ws + a.W.gnp), tiles_b);
  if (tid == 0) {
    const double n = (double)a.B;
    a.out[0] = S[0] / n;           // Actor/Loss
    a.out[1] = sqrt(gn2);          // the gradient's 2-norm
    a.out[2] = S[1] / n;           // mean(log_prob)
    a.out[3] = S[2] / n;           // mean(Q), with H mean(Q + H)
  }
  if (tid < D && a.ccolstats) {
    const double* d = reinterpret_cast<const double*>(a.ws + a.W.cdelta);
    a.ccolstats[tid] += (double)a.B;
    a.ccolstats[D + tid] += d[tid];
    a.ccolstats[2 * D + tid] += d[IN_MAX + tid];
  }
  if (tid < D && a.hpacked && a.hcolstats) {   // H's Standardizer takes the same rows: the same sums
    const double* d = reinterpret_cast<const double*>(a.ws + a.W.cdelta);
    a.hcolstats[tid] += (double)a.B;
    a.hcolstats[D + tid] += d[tid];
    a.hcolstats[2 * D + tid] += d[IN_MAX + tid];
  }
}

// _update_alpha (iq_sac.py:592-595): alpha_loss = -mean(exp(log_alpha) (log_prob + target_entropy)), Adam on log_alpha
struct AlphaArgs {
  int n;
  const float* log_prob;
  float target_entropy;
  oly_fit::AdamK ad;
  float* state;    // log_alpha, exp_avg, exp_avg_sq
};
__global__ __launch_bounds__(THREADS) void iq_alpha_kernel(AlphaArgs a) {
  __shared__ double dred[THREADS];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < a.n; i += THREADS) s += (double)a.log_prob[i] + (double)a.target_entropy;
  const double sum = tree_sum(dred, s);
  if (tid == 0) {
    float p = a.state[0], m = a.state[1], v = a.state[2];
    const float g = (float)(-exp((double)p) * (sum / (double)a.n));
    const oly_fit::AdamK& k = a.ad;     // adam1's order (fit_common.h), no weight decay
    m = m + (g - m) * k.w1;
    v = v * k.beta2 + (k.w2 * g) * g;
    const float denom = sqrtf(v) / k.bc2_sqrt + k.eps;
    p = p + k.neg_step * (m / denom);
    a.state[0] = p;
    a.state[1] = m;
    a.state[2] = v;
  }
}

}  // namespace

extern "C" int64_t oly_iq_pi_ws(int batch, int in_dim, int act_dim) {
  if (batch < 1 || batch > MAX_BATCH || in_dim <= 0 || act_dim <= 0 || act_dim > MAX_ACT || in_dim + act_dim > IN_MAX)
    return -1;
  return (int64_t)ws_layout(batch).total;
}

extern "C" int64_t oly_iq_pi_ws_values(int batch, int in_dim, int act_dim) {
  if (oly_iq_pi_ws(batch, in_dim, act_dim) < 0) return -1;
  return (int64_t)ws_layout(batch).qv;
}

extern "C" int oly_iq_pi_update(oly_ctx* ctx, const oly_iq_pi* f, oly_stream stream) {
  const char* name = "oly_iq_pi_update";
  if (!ctx) return OLY_EINVAL;
  if (!f) OLY_FAIL(ctx, OLY_EINVAL, "%s: NULL argument", name);
  const int in_dim = f->in_dim, A = f->act_dim, B = f->batch, D = in_dim + A;
  if (oly_iq_pi_ws(B, in_dim, A) < 0)
    OLY_FAIL(ctx, OLY_EINVAL,
             "%s: supported: 1 <= batch <= %d, in_dim >= 1, 1 <= act_dim <= %d, in_dim + act_dim <= %d (got batch %d, in %d, "
             "act %d)",
             name, MAX_BATCH, MAX_ACT, IN_MAX, B, in_dim, A);
  if (!f->x || !f->eps || !f->central || !f->delta || !f->param || !f->m || !f->v || !f->packed || !f->critic_packed ||
      !f->critic_param || !f->ws || !f->action || !f->log_prob || !f->out)
    OLY_FAIL(ctx, OLY_EINVAL, "%s: NULL pointer in the argument block", name);
  if (!(f->log_std_min <= f->log_std_max)) OLY_FAIL(ctx, OLY_EINVAL, "%s: log_std_min <= log_std_max is required", name);
  const WsL W = ws_layout(B);
  int rc = oly_fit::refuse_buffers(ctx, name, f->ws_floats, W.total, f->ws, f->packed, f->step, 1);
  if (rc != OLY_OK) return rc;
  if ((reinterpret_cast<uintptr_t>(f->critic_packed) & 15) != 0)
    OLY_FAIL(ctx, OLY_EINVAL, "%s: critic_packed must be 16-byte aligned", name);
  if (f->packed_floats < (int64_t)P_TOTAL || f->critic_packed_floats < (int64_t)P_TOTAL)
    OLY_FAIL(ctx, OLY_EINVAL, "%s: a packed stream holds %ld floats", name, (long)P_TOTAL);
  if ((reinterpret_cast<uintptr_t>(f->out) & 7) != 0 || (reinterpret_cast<uintptr_t>(f->colstats) & 7) != 0 ||
      (reinterpret_cast<uintptr_t>(f->critic_colstats) & 7) != 0)
    OLY_FAIL(ctx, OLY_EINVAL, "%s: out and the colstats must be 8-byte aligned", name);
  const bool hb = f->h_packed != nullptr;
  if (hb) {
    if (!f->h_param || !f->h_ws) OLY_FAIL(ctx, OLY_EINVAL, "%s: h_packed needs h_param and h_ws", name);
    if ((reinterpret_cast<uintptr_t>(f->h_packed) & 15) != 0 || (reinterpret_cast<uintptr_t>(f->h_ws) & 15) != 0)
      OLY_FAIL(ctx, OLY_EINVAL, "%s: h_packed and h_ws must be 16-byte aligned", name);
    if (f->h_packed_floats < (int64_t)P_TOTAL) OLY_FAIL(ctx, OLY_EINVAL, "%s: a packed stream holds %ld floats", name, (long)P_TOTAL);
    if (f->h_ws_floats < (int64_t)W.total)
      OLY_FAIL(ctx, OLY_EINVAL, "%s: h_ws holds %ld floats, %ld are needed", name, (long)f->h_ws_floats, (long)W.total);
    if ((reinterpret_cast<uintptr_t>(f->h_colstats) & 7) != 0) OLY_FAIL(ctx, OLY_EINVAL, "%s: h_colstats must be 8-byte aligned", name);
    if (f->h_ws == f->ws || f->h_packed == f->critic_packed)
      OLY_FAIL(ctx, OLY_EINVAL, "%s: H needs a stream and a workspace of its own", name);
  }

  PiArgs a{};
  a.in_dim = in_dim;
  a.act_dim = A;
  a.out_dim = 2 * A;
  a.D = D;
  a.B = B;
  a.x = f->x;
  a.eps = f->eps;
  a.central = f->central;
  a.delta = f->delta;
  a.colstats = f->colstats;
  a.ccolstats = f->critic_colstats;
  a.param = f->param;
  a.m = f->m;
  a.v = f->v;
  a.packed = f->packed;
  a.ws = f->ws;
  a.cpacked = f->critic_packed;
  a.cparam = f->critic_param;
  a.hpacked = f->h_packed;
  a.hparam = hb ? f->h_param : nullptr;
  a.hcolstats = hb ? f->h_colstats : nullptr;
  a.hws = hb ? f->h_ws : nullptr;
  a.action = f->action;
  a.log_prob = f->log_prob;
  a.alpha = f->alpha;
  a.ls_min = f->log_std_min;
  a.ls_max = f->log_std_max;
  a.coef = (float)(-1.0 / (double)B);
  a.ad = oly_fit::adam_scalars(f->beta1, f->beta2, f->adam_eps, f->lr, (long)f->step + 1);
  a.wd = f->weight_decay;
  a.out = f->out;
  a.P = param_layout(in_dim, 2 * A);
  a.CP = param_layout(D, 1);
  a.W = W;

  if (f->colstats) {   // Standardizer.update_mean_std before the forward (networks.py:70), as oly_sg_act
    rc = oly_col_stats(ctx, B, in_dim, f->x, f->colstats, 1, stream);
    if (rc != OLY_OK) return rc;
  }
  const int tiles_a = (B + 15) / 16, tiles_b = weight_tiles(in_dim, 2 * A);
  hipLaunchKernelGGL(iqpi_prologue_kernel, dim3(PRO_BLOCKS), dim3(THREADS), 0, oly_s(stream), a);
  rc = launch_rows(ctx, ctx->iqpi_attr_done, 1u, iqpi_act_kernel<2>, iqpi_act_kernel<4>, in_dim, dim3(tiles_a), A1_LDS, stream, a);
  if (rc != OLY_OK) return rc;
  rc = hb ? launch_rows(ctx, ctx->iqpi_attr_done, 16u, iqpi_grad_kernel<2, true>, iqpi_grad_kernel<4, true>, D, dim3(tiles_a),
                        A2H_LDS, stream, a)
          : launch_rows(ctx, ctx->iqpi_attr_done, 4u, iqpi_grad_kernel<2>, iqpi_grad_kernel<4>, D, dim3(tiles_a), A2_LDS, stream, a);
  if (rc != OLY_OK) return rc;
  hipLaunchKernelGGL(iqpi_weights_kernel, dim3(tiles_b), dim3(THREADS), 0, oly_s(stream), a);
  hipLaunchKernelGGL(iqpi_fold_kernel, dim3(1), dim3(THREADS), 0, oly_s(stream), a, tiles_a, tiles_b);
  OLY_LAUNCH_CHECK(ctx, "SAC-family policy update kernels");
  return OLY_OK;
}

extern "C" int oly_iq_alpha_update(oly_ctx* ctx, const oly_iq_alpha* f, oly_stream stream) {
  const char* name = "oly_iq_alpha_update";
  if (!ctx) return OLY_EINVAL;
  if (!f) OLY_FAIL(ctx, OLY_EINVAL, "%s: NULL argument", name);
  if (f->n < 1 || !f->log_prob || !f->state) OLY_FAIL(ctx, OLY_EINVAL, "%s: n >= 1, log_prob and state are required", name);
  if (f->step < 0 || (long)f->step + 1 > 0x7fffffffL) OLY_FAIL(ctx, OLY_EINVAL, "%s: bad step", name);
  AlphaArgs a{};
  a.n = f->n;
  a.log_prob = f->log_prob;
  a.target_entropy = f->target_entropy;
  a.ad = oly_fit::adam_scalars(f->beta1, f->beta2, f->eps, f->lr, (long)f->step + 1);
  a.state = f->state;
  hipLaunchKernelGGL(iq_alpha_kernel, dim3(1), dim3(THREADS), 0, oly_s(stream), a);
  OLY_LAUNCH_CHECK(ctx, "temperature update kernel");
  return OLY_OK;
}
