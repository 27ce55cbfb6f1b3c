// K26: the soft-Q critic update of the SAC-family imitation agents, IQ_SAC.update_Q_function with _lossQ, getV,
// get_targetV, regularizer_loss, update_Q_parameters and _update_all_targets (imitation_lib/imitation/iq_sac.py:421-429,
// 467-595, 674-676), SQIL's loss (imitation_lib/imitation/sqil_sac.py:64-136) and LSIQ's two losses with their clipped
// target (imitation_lib/imitation/lsiq.py:9-195).  The critic is a
// FullyConnectedNetwork((obs | act) -> [512, 256] -> 1, relu / relu / identity) whose Standardizer takes the whole
// concatenated row.  The policy passes (compute_action_and_log_prob_t on next_obs and on obs) are K25's and come in as
// the blocks a_next / logp_next and a_pi / logp_pi.
//
//   oly_iq_q_update   one update in four launches:
//   P  iq_prologue_kernel  the transposed W2 stream of the backward from param; the column sums of the three critic
//                          inputs X0 = (obs | act), X1 = (next_obs | a_next), X2 = (obs | a_pi) in NSP fixed slices.
//   A  iq_rows_kernel      one 16-row tile per workgroup (8 waves) runs every pass of its rows: each pass standardised
//                          with the statistics its network's Standardizer holds AT that pass (live: S + X0, then
//                          + X1 without a target, then + X2; target: T + X1), the forward on the f32 matrix cores in
//                          the forward kernel's chain order (ilmlp_common.h), so Q has oly_ilmlp_forward's bits.  Then
//                          per row V, y (LSIQ: from the clipped next_v), the loss terms and the coefficients dL/dQ,
//                          dL/dQ', dL/dV (fp64 from the f32 values, narrowed once; the per-row section has the split), and
//                          the backward of every pass that carries a gradient through the
//                          relus from the stored outputs.  Activations and deltas go to the workspace in row quads, one
//                          slot of BP rows per gradient pass; the tile's loss sums to fixed slots.
//   B  iq_weights_kernel   ilmlp_fit.h's launch B (weight_tile, dw_accumulate, meet_waves, tile_step, gradnorm_partial):
//                          one 16 x 16 weight tile per workgroup, dW summed over the slots' rows in a
//                          fixed order, weight decay, Adam, the stepped value into param, the moments and the packed
//                          stream; with update_target the soft target update f32(tau) w + f32(1 - tau) t (two float32
//                          products, one add) into target_param and its packed stream; the tile's sum of squared
//                          gradients to a fixed slot.
//   F  iq_fold_kernel      one workgroup: the 16 scalars from the per-tile partials, the two Standardizers' sums.
// LSIQ's sqil_like / value_plcy runs the third pass on the policy's rows alone (QArgs::n_v): the column sums of X2, the
// count its Standardizer takes and the rows' coefficients cover rows [0, n_policy), and nothing of a_pi / logp_pi past
// them is read.
// OLY_IQ_ALGO_LSIQ_H is the TD update of the second critic H of LSIQ_H / LSIQ_HC (update_H_function,
// imitation_lib/imitation/lsiq_h.py:57-102, imitation_lib/imitation/lsiq_hc.py:23-88): the block's network fields carry H,
// passes 0 (live, a gradient) and 1 (target) run, the last workgroup of P also forms the batch's count of absorbing rows
// and the running maximum of -log pi, launch A runs in instantiations of its own (iq_rows_kernel<G1, true>: the other
// algorithms' code is compiled without the branch), and F commits the running maximum.
// plcy_loss_mode v0 (iq_sac.py:508-510, lsiq.py:90-92; what LSIQ_Offline runs, imitation_lib/imitation/offline/
// lsiq_offline.py:50-159) comes with the block oly_iq_v0: a fourth pass Q_v0 = critic(obs[expert] | a_v0) on the expert
// rows, standardised with S + X0 (+ X1) + X2 + X3 and carrying the gradient of mean(f32(1 - gamma) (Q_v0 - alpha logp_v0)).
// The pass on (obs | a_pi) then has no gradient and the v0 pass takes its workspace slot; P sums X3's columns in the
// workgroups 3 NSP .. 4 NSP - 1, launch A runs in instantiations of its own (iq_rows_kernel<G1, false, true>, four passes),
// F adds X3 to the Standardizer.  With the block's all_expert a batch may have no policy rows: the policy subset's means
// come out as 0 / 0.
// Every reduction has a fixed order and there are no atomics: two runs give identical bits.  The Standardizer's head, the
// rows' staging, the hidden layers, dZ1, launch B's phases and the gradient norm's sums are ilmlp_fit.h's, shared with
// K18, K24 and K27.
#include <cstdlib>

#include "ilmlp_fit.h"
#include "oly_common.h"

namespace {
using namespace oly_ilfit;
using oly_fit::adam1;
static_assert(IN_MAX == oly_fit::MAX_IN, "fit_common.h's statistics arrays have this file's pitch");

constexpr int MAX_BATCH = OLY_BC_MAX_BATCH;
constexpr int MAX_ACT = OLY_BC_MAX_ACT;
constexpr int NSLOT = 3;     // gradient passes at most: Q(obs|act), Q(next_obs|a') without a target, Q(obs|a_pi)
constexpr int NTERM = 12;    // per-row loss terms, by subset (policy rows, expert rows)
static_assert(MAX_BATCH <= 16 * THREADS, "the fold kernel's loops run over at most 256 tiles");

// terms of a row: Q, Q^2, reward = Q - y, y, V, V - y, w reward^2, Q [absorbing], [absorbing],
//                 SQIL (Q - (R + y))^2, SQIL (V - (R_min + y))^2, unused; LSIQ keeps the row's expert loss (term 1) in
//                 T_SQ and its policy loss (sqil_like's term 2) in T_SV; plcy_loss_mode v0 keeps f32(1 - gamma) V0 of an
//                 expert row in T_V0
enum { T_Q, T_Q2, T_R, T_Y, T_V, T_VY, T_CHI, T_QABS, T_ABS, T_SQ, T_SV, T_V0 };

// workspace (floats), BP = batch rounded up to 16 rows, RP = NSLOT BP; [RP][W] arrays in row quads, element (row, col) at
// ((row / 4) W + col) 4 + row % 4, slot s in rows [s BP, (s + 1) BP):
//   xs [RP][64] | h1 [RP][512] | h2 [RP][256] | dZ1 [RP][512] | dZ2 [RP][256] | dZ3 [RP] | the raw outputs qv [4][BP] of
//   the passes (row 3: the v0 pass) | loss partials [BP / 16][2][NTERM] f64 | statistics partials [4][NSP][2][64] f64 | the
//   inputs' column sums [4][2][64] f64 | gradient-norm partials [weight tiles] f64 | the transposed stream W2T | LSIQ_H's batch
//   scalars [4]: the updated running maximum, the count of absorbing rows
struct WsL {
  size_t xs, h1, h2, dz1, dz2, dz3, qv, lossp, statp, delta, gnp, w2t, hsc, total;
};
constexpr int MAX_WTILES = 32 * (IN_MAX / 16) + 512 + 16;
__host__ __device__ inline WsL ws_layout(int batch) {
  const size_t BP = (size_t)(batch + 15) / 16 * 16, RP = NSLOT * BP;
  WsL W;
  W.xs = 0;
  W.h1 = W.xs + RP * IN_MAX;
  W.h2 = W.h1 + RP * H1;
  W.dz1 = W.h2 + RP * H2;
  W.dz2 = W.dz1 + RP * H1;
  W.dz3 = W.dz2 + RP * H2;
  W.qv = W.dz3 + RP;
  W.lossp = W.qv + 4 * BP;
  W.statp = W.lossp + BP / 16 * 2 * NTERM * 2;
  W.delta = W.statp + (size_t)4 * NSP * 2 * IN_MAX * 2;
  W.gnp = W.delta + (size_t)4 * 2 * IN_MAX * 2;
  W.w2t = W.gnp + (size_t)MAX_WTILES * 2;
  W.hsc = W.w2t + (size_t)H2 * H1;
  W.total = W.hsc + 4;
  return W;
}

struct QArgs {
  int in_dim, act_dim, D, B, n_policy;
  int algo, loss_mode, reg_mode, treat_abs, use_target, update_target, has_v;
  int iq_like;                 // the loss family: IQ's three terms (IQ, LSIQ iq_like) or squared / Huber residuals
  int exp_mode, exp_loss, clip;   // LSIQ: loss_mode_exp, Q_exp_loss, target_clipping
  int n_v;                     // rows of the third pass: B, or n_policy for LSIQ's sqil_like / value_plcy
  float q_min, q_max;          // LSIQ's bounds
  float inv_rm, g1;            // LSIQ sqil_like: f32(1 / reg_mult) and 1 / (1 - gamma) in float32
  int h_loss, h_cost, h_clip;  // LSIQ_H: the block's h_loss, h_cost, h_clip_expert
  float h_tu, h_omu, h_td, h_omd;   // LSIQ_H: f32(tau_up), f32(1 - tau_up), f32(tau_down), f32(1 - tau_down)
  float h_lo, h_hi, h_omg;     // LSIQ_H: the target's clip bounds; 1 - gamma in float32
  float* h_max;                // LSIQ_H: the block's h_max_state
  const float *h_q_t, *h_v_t;
  int slot[4];                 // the workspace slot of each pass's gradient rows, -1: the pass has no gradient
  int n_slots;
  const float *obs, *act, *next_obs, *absorbing, *a_next, *logp_next, *a_pi, *logp_pi;
  double *colstats, *tcolstats;
  float *param, *m, *v, *packed, *tparam, *tpacked, *ws;
  float gamma, alpha, reg_mult, r_min, r_max, tau, omt;
  oly_fit::AdamK ad;
  float wd;
  double* out;
  ParamLayout P;
  WsL W;
  // plcy_loss_mode v0: the fourth pass Q_v0 = critic(obs[expert] | a_v0) on the n_v0 = B - n_policy expert rows
  int v0, n_v0;
  float omg;                   // 1 - gamma in float32
  const float *a_v0, *logp_v0;
};

// column k < D of row `row` of critic input `src`
__device__ __forceinline__ float input_at(const QArgs& a, int src, size_t row, int k) {
  const float* s = src == 1 ? a.next_obs : a.obs;
  const float* u = src == 0 ? a.act : src == 1 ? a.a_next : a.a_pi;
  return k < a.in_dim ? s[row * a.in_dim + k] : u[row * a.act_dim + (k - a.in_dim)];
}

// column k < D of row `row` >= n_policy of the v0 pass's input (obs | a_v0); a_v0's rows count from the first expert row
__device__ __forceinline__ float v0_input_at(const QArgs& a, size_t row, int k) {
  return k < a.in_dim ? a.obs[row * a.in_dim + k] : a.a_v0[(row - (size_t)a.n_policy) * a.act_dim + (k - a.in_dim)];
}

// LSIQ_H, one workgroup: n1 = the count of absorbing rows and cur = max(-logp_next[0, n_policy)), thread t over rows t,
// t + THREADS, ... and a halving tree (a count of at most 4096 ones and a maximum: exact in any order); thread 0 then
// forms the running maximum as lsiq_h.py:64-74 does, in float32: the first call takes cur, a later one
// f32(1 - tau) M + f32(tau) cur (two float32 products, one add) with tau_up where cur > M, else tau_down.  Both go to the
// workspace; h_max_state itself is written by launch F.
__device__ __forceinline__ void h_batch_scalars(const QArgs& a, double* part) {
  const int tid = threadIdx.x;
  float* cnt = reinterpret_cast<float*>(part);
  float* mx = cnt + THREADS;
  float n1 = 0.f, cur = -INFINITY;
  for (int r = tid; r < a.B; r += THREADS) {
    n1 += a.absorbing[r] != 0.f ? 1.f : 0.f;
    if (r < a.n_policy) cur = fmaxf(cur, -a.logp_next[r]);
  }
  cnt[tid] = n1;
  mx[tid] = cur;
  __syncthreads();
  for (int h = THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) {
      cnt[tid] += cnt[tid + h];
      mx[tid] = fmaxf(mx[tid], mx[tid + h]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    float M = 0.f;
    if (a.h_clip) {
      const float M0 = a.h_max[0];
      cur = mx[0];
      M = a.h_max[1] == 0.f ? cur : cur > M0 ? a.h_omu * M0 + a.h_tu * cur : a.h_omd * M0 + a.h_td * cur;
    }
    a.ws[a.W.hsc] = M;
    a.ws[a.W.hsc + 1] = cnt[0];
  }
  __syncthreads();
}

// grid PRO_BLOCKS: the transposed stream from param (grid-stride) and, workgroups 0 .. 4 NSP - 1, slice b % NSP of input
// b / NSP (input 3: the v0 pass's X3 = (obs[expert] | a_v0)): four row-strided chains per column, met in a fixed order
// (fit_common.h's fold_chains)
static_assert(4 * NSP <= PRO_BLOCKS, "one workgroup per statistics slice");
__global__ __launch_bounds__(THREADS) void iq_prologue_kernel(QArgs a) {
  __shared__ double part[8 * IN_MAX];
  build_w2t(a);
  if (a.algo == OLY_IQ_ALGO_LSIQ_H && blockIdx.x == PRO_BLOCKS - 1) h_batch_scalars(a, part);
  const int src = blockIdx.x / NSP, s = blockIdx.x % NSP;
  if (src >= 4 || (src == 2 && !a.has_v) || (src == 3 && !a.v0) || (!a.colstats && !a.tcolstats)) return;
  const int tid = threadIdx.x, k = tid & (IN_MAX - 1), grp = tid >> 6;
  const int nb = src == 3 ? a.n_v0 : src == 2 ? a.n_v : a.B;     // the rows of this pass
  const int per = (nb + NSP - 1) / NSP, r0 = s * per, r1 = min(nb, r0 + per);
  double sum = 0.0, ss = 0.0;
  if (k < a.D)
    for (int r = r0 + grp; r < r1; r += 4) {
      const double v = src == 3 ? v0_input_at(a, (size_t)(a.n_policy + r), k) : input_at(a, src, (size_t)r, k);
      sum += v;
      ss += v * v;
    }
  oly_fit::fold_chains(sum, ss, a.D, part,
                       reinterpret_cast<double*>(a.ws + a.W.statp) + (size_t)(src * NSP + s) * 2 * IN_MAX);
}

// ---------------------------------------------------------------------------------------------------------------
// Launch A.  RTHREADS = 512 threads = 8 waves, the chains of ilmlp_fit.h: layer 1 wave w -> column tiles 4w .. 4w+3, layer 2 -> 2w, 2w+1, the
// output column by wave 0 as one chain over k < 256.  Backward: dZ2 = dQ W3 [h2 > 0] (one float32 product per element:
// the output layer has one unit), dH1 = dZ2 W2 on the matrix cores (wave w -> tiles 4w .. 4w+3, the transposed stream).
constexpr size_t ROWS_LDS_FLOATS = (size_t)(IN_MAX + H1 + 2 * H2) * 16;
constexpr size_t rows_lds(int passes) {
  return sizeof(float) * ROWS_LDS_FLOATS + sizeof(double) * ((size_t)passes * 2 * IN_MAX + 16 * NTERM);
}
constexpr size_t ROWS_LDS = rows_lds(3), ROWS_LDS_V0 = rows_lds(4);
static_assert(ROWS_LDS_FLOATS % 4 == 0, "the fp64 arrays must be 8-byte aligned");

static_assert(OLY_LSIQ_VALUE == OLY_IQ_VALUE && OLY_LSIQ_VALUE_EXPERT == OLY_IQ_VALUE_EXPERT &&
                  OLY_LSIQ_VALUE_POLICY == OLY_IQ_VALUE_POLICY && OLY_LSIQ_Q_OLD_POLICY == OLY_IQ_Q_OLD_POLICY &&
                  OLY_LSIQ_V0 == OLY_IQ_V0,
              "LSIQ's iq_like modes extend IQ's: the rows and fold kernels read both through OLY_IQ_*");

// One residual d under LSIQ's Q_exp_loss: F.mse_loss / torch.square (d^2) or F.huber_loss with delta 1 (0.5 d^2 below 1,
// |d| - 0.5 from there; torch's backward passes d inside [-1, 1] and its sign outside).  The value and d(value)/dd.
__device__ __forceinline__ void point_loss(int kind, float d, double& value, double& grad) {
  const double x = (double)d;
  if (kind == OLY_LSIQ_LOSS_HUBER) {
    const double ax = fabs(x);
    value = ax < 1.0 ? 0.5 * x * x : ax - 0.5;
    grad = x < -1.0 ? -1.0 : x > 1.0 ? 1.0 : x;
  } else {
    value = x * x;
    grad = 2.0 * x;
  }
}

// LSIQ_H's row (lsiq_h.py:57-83, lsiq_hc.py:23-69): the two targets of the [B, B] broadcast, t0 against the n0
// non-absorbing columns and t1 against the n1 absorbing ones, in float32 in the reference's order; the row's share of the
// loss sum n0 l(H - t0) + n1 l(H - t1) and dL/dH = (n0 l'(H - t0) + n1 l'(H - t1)) / B^2 in fp64.
__device__ __forceinline__ float h_row(const QArgs& a, size_t i, int expert, float H, float Ht, double* t) {
  const float M = a.ws[a.W.hsc], n1 = a.ws[a.W.hsc + 1];
  const float neg = -a.logp_next[i];
  float nc = neg;
  if (a.h_clip && expert) {                                   // torch.clip(neg[expert], M, 100000): min(max(., M), 1e5)
    nc = nc < M ? M : nc;
    nc = nc > 100000.f ? 100000.f : nc;
  }
  const float nH = Ht + a.alpha * nc;
  const float cy0 = (1.f - 0.f) * a.gamma, cy1 = (1.f - 1.f) * a.gamma;    // (1 - absorbing[j]) * gamma
  float t0 = cy0 * nH, t1 = cy1 * nH;
  if (a.h_cost) {
    const float Q = a.h_q_t[i], V = a.h_v_t[i];
    const float Vc = V < a.q_min ? a.q_min : V > a.q_max ? a.q_max : V;
    const float d0 = Q - cy0 * Vc, d1 = Q - cy1 * Vc;
    const float rn = d0 < -a.inv_rm ? -a.inv_rm : d0 > a.inv_rm ? a.inv_rm : d0;
    const float ra = d1 < a.q_min ? a.q_min : d1 > a.q_max ? a.q_max : d1;
    // (1 - ab) reg_mult reward_non_abs + (ab (1 - gamma)) reg_mult reward_abs: the other product is an exact zero
    t0 = a.reg_mult * (rn * rn) + t0;
    t1 = (a.h_omg * a.reg_mult) * (ra * ra) + t1;
  }
  t0 = t0 < a.h_lo ? a.h_lo : t0 > a.h_hi ? a.h_hi : t0;
  t1 = t1 < a.h_lo ? a.h_lo : t1 > a.h_hi ? a.h_hi : t1;
  double l0, g0, l1, g1;
  point_loss(a.h_loss, H - t0, l0, g0);
  point_loss(a.h_loss, H - t1, l1, g1);
  const double c1 = (double)n1, c0 = (double)a.B - c1, n = (double)a.B;
  t[T_Q] = H;
  t[T_R] = neg;
  // a count of zero takes its term out (0 x inf would be NaN; torch's mean has no such column)
  t[T_SQ] = (c0 != 0.0 ? c0 * l0 : 0.0) + (c1 != 0.0 ? c1 * l1 : 0.0);
  return (float)(((c0 != 0.0 ? c0 * g0 : 0.0) + (c1 != 0.0 ? c1 * g1 : 0.0)) / (n * n));
}

// The three loss families of the Q critic's row (e: 1 expert, 0 policy) from its Q, y = cy clip(next_v), V and absorbing
// flag ab: the family's terms into t[] and, added to the caller's zeros, dL/d(reward) dr (on Q and, negated, on y),
// dL/dQ beside it dq (LSIQ's fix losses see Q alone), dL/dV and dL/dy beside -dL/d(reward), all fp64.
//
// IQ's three terms (iq_sac.py:467-563) and LSIQ's iq_like (lsiq.py:51-128)
__device__ __forceinline__ void iq_like_row(const QArgs& a, int e, float Q, float y, float ab, double* t, double& dr,
                                            double& dq, double& dV, double& dy) {
  const double n_all = (double)a.B, n_p = (double)a.n_policy, n_e = (double)(a.B - a.n_policy);
  const double n_own = e ? n_e : n_p;
  const float r = Q - y;
  if (e) {
    if (a.algo != OLY_IQ_ALGO_LSIQ || a.exp_mode == OLY_LSIQ_EXP_BOOTSTRAP) {
      dr -= 1.0 / n_e;                                          // loss_term1 = -mean(reward[expert])
    } else {                                                    // lsiq.py:56-60: Q[expert] against the constant Q_max
      double g;
      point_loss(a.exp_loss, Q - a.q_max, t[T_SQ], g);
      dq = g / n_e;
    }
  }
  const int md = a.loss_mode;          // LSIQ adds value_q_old_policy (both terms) and off (neither), lsiq.py:87-94
  if (md == OLY_IQ_VALUE || md == OLY_LSIQ_VALUE_Q_OLD_POLICY) dV = 1.0 / n_all;
  else if (md == OLY_IQ_VALUE_EXPERT) dV = e ? 1.0 / n_e : 0.0;
  else if (md == OLY_IQ_VALUE_POLICY) dV = e ? 0.0 : 1.0 / n_p;
  if ((md == OLY_IQ_Q_OLD_POLICY || md == OLY_LSIQ_VALUE_Q_OLD_POLICY) && !e)
    dr += 1.0 / n_p;                                            // q_old_policy: mean(reward[~expert])
  dy = -dV;
  const double ra = a.treat_abs ? (double)ab : 0.0;
  const double w = (1.0 - ra) * (double)a.reg_mult + ra * (1.0 - (double)a.gamma) * (double)a.reg_mult;
  const bool in = a.reg_mode == OLY_IQ_REG_EXP_AND_PLCY || (a.reg_mode == OLY_IQ_REG_EXP && e) ||
                  (a.reg_mode == OLY_IQ_REG_PLCY && !e);
  if (in) {
    const double nr = a.reg_mode == OLY_IQ_REG_EXP_AND_PLCY ? n_all : n_own;
    dr += 2.0 * w * (double)r / nr;
    t[T_CHI] = w * (double)r * (double)r;
  }
}

// LSIQ's sqil_like (lsiq.py:130-178): no factor 0.5, no reg_mult multiplier, no chi2 term
__device__ __forceinline__ void lsiq_sq_row(const QArgs& a, int e, float Q, float y, float V, float ab, double* t, double& dr,
                                            double& dq, double& dV, double& dy) {
  const double n_all = (double)a.B, n_p = (double)a.n_policy, n_e = (double)(a.B - a.n_policy);
  // r_max = -r_min in float32, the reference's order: (1 - ab) (1 / reg_mult) + (ab (1 / (1 - gamma))) (1 / reg_mult)
  const float rw = a.treat_abs ? (1.f - ab) * a.inv_rm + (ab * a.g1) * a.inv_rm : a.inv_rm;
  double g;
  if (e) {
    const float d = a.exp_mode == OLY_LSIQ_EXP_BOOTSTRAP ? Q - (rw + y) : Q - a.q_max;   // :146-148, :153-155
    point_loss(a.exp_loss, d, t[T_SQ], g);
    if (a.exp_mode == OLY_LSIQ_EXP_BOOTSTRAP) dr += g / n_e;
    else dq = g / n_e;
  }
  // mode value (:165): r_min[~expert] and then as many plain -1 / reg_mult, which land on the expert rows
  const float rmin = e ? -a.inv_rm : -rw;
  if (a.loss_mode == OLY_LSIQ_SQ_VALUE || (a.loss_mode == OLY_LSIQ_SQ_VALUE_PLCY && !e)) {
    point_loss(a.exp_loss, V - (rmin + y), t[T_SV], g);         // :162-168, 173-176
    dV = g / (a.loss_mode == OLY_LSIQ_SQ_VALUE ? n_all : n_p);
    dy = -dV;
  } else if (a.loss_mode == OLY_LSIQ_SQ_Q_OLD_POLICY && !e) {
    point_loss(a.exp_loss, Q - (rmin + y), t[T_SV], g);         // :169-171
    dr += g / n_p;
  }
}

// SQIL's squared residuals against R_max (expert rows) and R_min (sqil_sac.py:64-92)
__device__ __forceinline__ void sqil_row(const QArgs& a, int e, float Q, float y, float V, double* t, double& dr, double& dV,
                                         double& dy) {
  const double n_all = (double)a.B, n_p = (double)a.n_policy, n_e = (double)(a.B - a.n_policy);
  const double rm = (double)a.reg_mult;
  if (e) {
    const float d = Q - (a.r_max + y);                          // sqil_sac.py:80
    dr += rm * (double)d / n_e;
    t[T_SQ] = (double)d * (double)d;
  } else if (a.loss_mode == OLY_SQIL_PLCY) {
    const float d = Q - (a.r_min + y);                          // :90
    dr += rm * (double)d / n_p;
    t[T_SQ] = (double)d * (double)d;
  }
  if (a.loss_mode == OLY_SQIL_VALUE || (a.loss_mode == OLY_SQIL_VALUE_PLCY && !e)) {
    const float d = V - (a.r_min + y);                          // :85, :88
    dV = rm * (double)d / (a.loss_mode == OLY_SQIL_VALUE ? n_all : n_p);
    dy = -dV;
    t[T_SV] = (double)d * (double)d;
  }
}

// V0: the instantiations of plcy_loss_mode v0, with the fourth pass; the others are compiled without it (NP = 3).
template <int G1, bool HB = false, bool V0 = false>
__global__ __launch_bounds__(RTHREADS) void iq_rows_kernel(QArgs a) {
  constexpr int NP = V0 ? 4 : 3;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xT = lds;                       // [64 x 16]   standardised input (act16 images, mlp_tiles.h)
  float* hA = xT + IN_MAX * 16;          // [512 x 16]  h1
  float* hB = hA + H1 * 16;              // [256 x 16]  h2
  float* gz = hB + H2 * 16;              // [256 x 16]  dZ2
  double* st = reinterpret_cast<double*>(lds + ROWS_LDS_FLOATS);   // [NP passes][2][IN_MAX] mean, std
  double* terms = st + NP * 2 * IN_MAX;  // [16 rows][NTERM]
  __shared__ float z[NP][16];            // the raw outputs of the passes by row
  __shared__ float coef[NP][16];         // dL/d(output) of the passes by row
  __shared__ int sub[16];                // 0 policy row, 1 expert row, -1 beyond the batch
  const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, h4 = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row0 = blockIdx.x * 16, B = a.B, D = a.D;
  const size_t BP = (size_t)gridDim.x * 16;
  float* ws = a.ws;
  float4* ws4 = reinterpret_cast<float4*>(ws);

  if (tid < D) {   // Standardizer.update_mean_std with each pass's rows (networks.py:76-81): the sums pass by pass
    const double* sp = reinterpret_cast<const double*>(ws + a.W.statp);
    double s[NP], ss[NP];
    for (int p = 0; p < NP; ++p) {
      s[p] = ss[p] = 0.0;
      if ((a.colstats || a.tcolstats) && (p < 2 || a.has_v)) slice_sums(sp + (size_t)p * NSP * 2 * IN_MAX, tid, s[p], ss[p]);
    }
    if (blockIdx.x == 0) {
      double* d = reinterpret_cast<double*>(ws + a.W.delta);
      for (int p = 0; p < NP; ++p) {
        d[p * 2 * IN_MAX + tid] = s[p];
        d[p * 2 * IN_MAX + IN_MAX + tid] = ss[p];
      }
    }
    double cnt = 0.0, sum = 0.0, sq = 0.0;
    if (a.colstats) cnt = a.colstats[tid], sum = a.colstats[D + tid], sq = a.colstats[2 * D + tid];
    for (int p = 0; p < NP; ++p) {
      double pc, ps, pq;
      bool have;
      if (p == 1 && a.use_target) {
        have = a.tcolstats != nullptr;
        pc = have ? a.tcolstats[tid] + (double)B : 0.0;
        ps = have ? a.tcolstats[D + tid] + s[1] : 0.0;
        pq = have ? a.tcolstats[2 * D + tid] + ss[1] : 0.0;
      } else {
        have = a.colstats != nullptr;
        if (V0 && p == 3) cnt += (double)a.n_v0, sum += s[p], sq += ss[p];
        else if (p < 2 || a.has_v) cnt += (double)(p == 2 ? a.n_v : B), sum += s[p], sq += ss[p];
        pc = cnt, ps = sum, pq = sq;
      }
      double mean = 0.0, sd = 1.0;
      if (have) col_moments(pc, ps, pq, mean, sd);
      st[(p * 2) * IN_MAX + tid] = mean;
      st[(p * 2 + 1) * IN_MAX + tid] = sd;
    }
  }
  if (tid < 16) sub[tid] = row0 + tid < B ? (row0 + tid >= a.n_policy ? 1 : 0) : -1;
  __syncthreads();

  // ---- the forwards
  for (int p = 0; p < NP; ++p) {
    if (p == 2 && !a.has_v) break;
    const bool tgt = p == 1 && a.use_target;
    const bool standardise = tgt ? a.tcolstats != nullptr : a.colstats != nullptr;
    const float* P = tgt ? a.tpacked : a.packed;
    const int slot = a.slot[p];
    const size_t srow0 = (size_t)(slot < 0 ? 0 : slot) * BP + row0;
    const size_t quad = (srow0 >> 2) + h4;           // this lane's accumulator rows: 4 h4 + i = one row quad
    stage_rows(xT, D, standardise, st + (p * 2) * IN_MAX,      // a row the pass does not take goes through as zeros
               [&](int m) {     // the v0 pass takes the expert rows
                 if constexpr (V0)
                   if (p == 3) return sub[m] == 1;
                 return sub[m] >= 0 && (p < 2 || row0 + m < a.n_v);
               },
               [&](int m, int k) {
                 if constexpr (V0)
                   if (p == 3) return v0_input_at(a, (size_t)(row0 + m), k);
                 return input_at(a, p, (size_t)(row0 + m), k);
               },
               slot >= 0, ws + a.W.xs, srow0);
    __syncthreads();
    // ---- layer 1: [16, D] x [D, 512], layer 2: [16, 512] x [512, 256]; a pass without a gradient keeps no activations
    hidden_layer<Relu, G1, IN_MAX / 16, 4, P_W1, P_B1>(xT, P, hA, slot >= 0, ws4, a.W.h1, quad);
    __syncthreads();
    hidden_layer<Relu, H1 / 16, H1 / 16, 2, P_W2, P_B2>(hA, P, hB, slot >= 0, ws4, a.W.h2, quad);
    __syncthreads();
    // ---- the output unit: ilmlp_fit.h's output_unit in its own text.  Through the function this kernel is allocated two
    // to four registers fewer and scheduled for one more wave per SIMD (which a 512-thread workgroup with this much LDS
    // never has), and the call ran 0.4 to 1.1 us longer at 512 rows without a target in each of three alternating runs.
    if (wave == 0) {
      f32x4 acc[1][1] = {{f32x4{0.f, 0.f, 0.f, 0.f}}};
      const float4* a4[1] = {reinterpret_cast<const float4*>(hB)};
      tiles<H2 / 16, 1, 1>(a4, reinterpret_cast<const float4*>(P) + P_W3 / 4, 0, lane, acc);
      if (c == 0) {
        const float bv = P[P_B3];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float q = acc[0][0][i] + bv;
          z[p][4 * h4 + i] = q;
          ws[a.W.qv + (size_t)p * BP + row0 + 4 * h4 + i] = q;
        }
      }
    }
    __syncthreads();
  }

  // ---- the loss terms and the coefficients of row tid (iq_sac.py:467-563, sqil_sac.py:64-92)
  if (tid < 16) {
    const int e = sub[tid];
    double t[NTERM];
    for (int j = 0; j < NTERM; ++j) t[j] = 0.0;
    float cQ = 0.f, cN = 0.f, cV = 0.f;
    [[maybe_unused]] float c0 = 0.f;
    if constexpr (HB) {
      if (e >= 0) cQ = h_row(a, (size_t)row0 + tid, e, z[0][tid], z[1][tid], t);
    } else if (e >= 0) {
      const size_t i = (size_t)row0 + tid;
      const float ab = a.absorbing[i];
      const float Q = z[0][tid];
      const float nv = z[1][tid] - a.alpha * a.logp_next[i];          // getV / get_targetV (:571-585)
      const float cy = (1.f - ab) * a.gamma;
      // LSIQ's target_clipping (lsiq.py:46-49, 125-128): torch.clip keeps a NaN and lets the gradient through where
      // q_min <= next_v <= q_max, bounds included
      const bool lsiq = a.algo == OLY_IQ_ALGO_LSIQ, clip = lsiq && a.clip;
      const float nvc = clip ? (nv < a.q_min ? a.q_min : nv > a.q_max ? a.q_max : nv) : nv;
      const bool through = !clip || (nv >= a.q_min && nv <= a.q_max);
      const float y = cy * nvc;                                       // :482
      const float V = a.has_v && i < (size_t)a.n_v ? z[2][tid] - a.alpha * a.logp_pi[i] : 0.f;
      const float r = Q - y, vy = V - y;
      // dL/d(reward) (on Q and, negated, on y), dL/dQ beside it (LSIQ's fix losses see Q alone), dL/dV, dL/dy beside
      // -dL/d(reward)
      double dr = 0.0, dq = 0.0, dV = 0.0, dy = 0.0;
      t[T_Q] = Q;
      t[T_Q2] = (double)Q * (double)Q;
      t[T_R] = r;
      t[T_Y] = y;
      t[T_V] = V;
      t[T_VY] = vy;
      t[T_QABS] = ab != 0.f ? (double)Q : 0.0;
      t[T_ABS] = ab != 0.f ? 1.0 : 0.0;
      if (a.iq_like) iq_like_row(a, e, Q, y, ab, t, dr, dq, dV, dy);
      else if (lsiq) lsiq_sq_row(a, e, Q, y, V, ab, t, dr, dq, dV, dy);
      else sqil_row(a, e, Q, y, V, t, dr, dV, dy);
      cQ = (float)(dr + dq);
      cV = (float)dV;
      // y = cy clip(next_v) carries a gradient without a target, where the clip lets it through
      cN = a.use_target || !through ? 0.f : (float)((double)cy * (dy - dr));
      if constexpr (V0) {
        if (e == 1) {   // loss_term2 = mean(f32(1 - gamma) getV(obs[expert])) (iq_sac.py:508-510, lsiq.py:90-92)
          const float v0 = z[3][tid] - a.alpha * a.logp_v0[i - (size_t)a.n_policy];
          t[T_V0] = (double)(a.omg * v0);
          c0 = (float)((double)a.omg / (double)(a.B - a.n_policy));
        }
      }
    }
    coef[0][tid] = cQ;
    coef[1][tid] = cN;
    coef[2][tid] = cV;
    if constexpr (V0) coef[3][tid] = c0;
    for (int j = 0; j < NTERM; ++j) terms[tid * NTERM + j] = t[j];
  }
  __syncthreads();
  if (tid < 2 * NTERM) {      // this tile's partials: subset tid / NTERM, term tid % NTERM, rows in order
    const int e = tid / NTERM, j = tid % NTERM;
    double s = 0.0;
    for (int r = 0; r < 16; ++r)
      if (sub[r] == e) s += terms[r * NTERM + j];
    reinterpret_cast<double*>(ws + a.W.lossp)[(size_t)blockIdx.x * 2 * NTERM + tid] = s;
  }

  // ---- the backwards
  for (int p = 0; p < NP; ++p) {
    const int slot = a.slot[p];
    if (slot < 0) continue;
    const size_t srow0 = (size_t)slot * BP + row0;
    const size_t quad = (srow0 >> 2) + h4;
    if (tid < 16) ws[a.W.dz3 + srow0 + tid] = coef[p][tid];
    {  // ---- dZ2 = (dQ W3) [h2 > 0]; this thread wrote the h2 and h1 values it reads back
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int col = 16 * (2 * wave + t) + c;
        const float w3 = a.param[a.P.w3 + col];
        const float4 h = ws4[(a.W.h2 >> 2) + quad * H2 + col];
        float4 g;
        g.x = h.x > 0.f && sub[4 * h4] >= 0 ? coef[p][4 * h4] * w3 : 0.f;
        g.y = h.y > 0.f && sub[4 * h4 + 1] >= 0 ? coef[p][4 * h4 + 1] * w3 : 0.f;
        g.z = h.z > 0.f && sub[4 * h4 + 2] >= 0 ? coef[p][4 * h4 + 2] * w3 : 0.f;
        g.w = h.w > 0.f && sub[4 * h4 + 3] >= 0 ? coef[p][4 * h4 + 3] * w3 : 0.f;
        put_quad(gz, col, h4, g);
        ws4[(a.W.dz2 >> 2) + quad * H2 + col] = g;
      }
    }
    __syncthreads();
    // ---- dZ1 = (dZ2 W2) [h1 > 0]; hA holds a later pass by now: the stored h1 comes from the workspace
    dz1_tiles<Relu>(gz, reinterpret_cast<const float4*>(ws) + (a.W.w2t >> 2),
                    [&](int col) { return ws4[(a.W.h1 >> 2) + quad * H1 + col]; }, ws4, a.W.dz1, quad);
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Launch B (the tiles: weight_tiles, ilmlp_fit.h; W3 is 1 x 16).
// the soft target update of the parameter at i (packed at pk): f32(tau) w + f32(1 - tau) t
__device__ __forceinline__ void step_target(const QArgs& a, size_t i, size_t pk, float p) {
  if (!a.update_target) return;
  const float t = a.tau * p + a.omt * a.tparam[i];
  a.tparam[i] = t;
  a.tpacked[pk] = t;
}

__global__ __launch_bounds__(THREADS) void iq_weights_kernel(QArgs a) {
  __shared__ float red[4 * 256];
  __shared__ float bred[4 * 64];
  __shared__ double dred[THREADS];
  __shared__ double bsq[16];
  const WeightTile T = weight_tile(a, a.D, 1, 1);
  // the steps run over the rows of every slot
  f32x4 acc;
  float bsum;
  dw_accumulate(T.dl, T.al, T.dw, T.aw, T.n0, T.N, T.k0, T.K, a.n_slots * ((a.B + 15) / 16), acc, bsum);
  meet_waves(red, bred, acc, bsum);
  double g2, b2;
  tile_step(T, a, a.D, red, bred, [&](int, int, int, size_t i, size_t pk, float g) {
    const float p = adam1(a, i, g);
    a.packed[pk] = p;
    step_target(a, i, pk, p);
  }, g2, b2);
  gradnorm_partial(dred, bsq, g2, b2, reinterpret_cast<double*>(a.ws + a.W.gnp));
}

// ---------------------------------------------------------------------------------------------------------------
// Launch F: one workgroup.  Thread j < 2 NTERM adds term j of the tiles in order; thread t adds the gradient-norm
// partials t, t + 256, ... and a halving tree joins them; thread 0 writes the 16 scalars; threads < D add the passes'
// column sums to the Standardizers in the order of the passes.
__global__ __launch_bounds__(THREADS) void iq_fold_kernel(QArgs a, int tiles_a, int tiles_b) {
  __shared__ double S[2 * NTERM];
  __shared__ double dred[THREADS];
  const int tid = threadIdx.x, D = a.D;
  if (tid < 2 * NTERM) {
    const double* lp = reinterpret_cast<const double*>(a.ws + a.W.lossp);
    double s = 0.0;
    for (int t = 0; t < tiles_a; ++t) s += lp[(size_t)t * 2 * NTERM + tid];
    S[tid] = s;
  }
  const double gn2 = gradnorm_total(dred, reinterpret_cast<const double*>(a.ws + a.W.gnp), tiles_b);
  if (tid == 0) {
    const double* Sp = S;            // policy rows
    const double* Se = S + NTERM;    // expert rows
    const double n_all = (double)a.B, n_p = (double)a.n_policy, n_e = n_all - n_p;
    double o[16];
    for (int j = 0; j < 16; ++j) o[j] = 0.0;
    const bool lsiq = a.algo == OLY_IQ_ALGO_LSIQ;
    if (a.algo == OLY_IQ_ALGO_LSIQ_H) {      // the seven scalars of lsiq_h.py:94-100, the gradient's norm, the maximum
      const float M = a.ws[a.W.hsc];
      o[0] = (Sp[T_SQ] + Se[T_SQ]) / (n_all * n_all);
      o[1] = (Sp[T_Q] + Se[T_Q]) / n_all;
      o[2] = Sp[T_Q] / n_p;
      o[3] = Se[T_Q] / n_e;
      o[4] = (Sp[T_R] + Se[T_R]) / n_all;
      o[5] = Sp[T_R] / n_p;
      o[6] = Se[T_R] / n_e;
      o[7] = sqrt(gn2);
      o[8] = a.h_clip ? (double)M : 0.0;
      if (a.h_clip) {
        a.h_max[0] = M;
        a.h_max[1] = 1.f;
      }
    } else if (a.iq_like) {
      o[0] = lsiq && a.exp_mode == OLY_LSIQ_EXP_FIX ? Se[T_SQ] / n_e : -Se[T_R] / n_e;
      o[1] = a.v0 ? Se[T_V0] / n_e
             : a.loss_mode == OLY_IQ_VALUE ? (Sp[T_VY] + Se[T_VY]) / n_all
             : a.loss_mode == OLY_IQ_VALUE_EXPERT ? Se[T_VY] / n_e
             : a.loss_mode == OLY_IQ_VALUE_POLICY ? Sp[T_VY] / n_p
             : a.loss_mode == OLY_IQ_Q_OLD_POLICY ? Sp[T_R] / n_p
             : a.loss_mode == OLY_LSIQ_VALUE_Q_OLD_POLICY ? Sp[T_R] / n_p + (Sp[T_VY] + Se[T_VY]) / n_all
                                                         : 0.0;
      o[2] = a.reg_mode == OLY_IQ_REG_EXP_AND_PLCY ? (Sp[T_CHI] + Se[T_CHI]) / n_all
             : a.reg_mode == OLY_IQ_REG_EXP ? Se[T_CHI] / n_e
             : a.reg_mode == OLY_IQ_REG_PLCY ? Sp[T_CHI] / n_p
                                             : 0.0;
    } else if (lsiq) {   // sqil_like returns (loss_term1, loss_term2, 0.0), lsiq.py:195
      o[0] = Se[T_SQ] / n_e;
      o[1] = a.loss_mode == OLY_LSIQ_SQ_VALUE ? (Sp[T_SV] + Se[T_SV]) / n_all : Sp[T_SV] / n_p;
    } else {
      const double second = a.loss_mode == OLY_SQIL_VALUE ? 0.5 * (Sp[T_SV] + Se[T_SV]) / n_all
                            : a.loss_mode == OLY_SQIL_VALUE_PLCY ? 0.5 * Sp[T_SV] / n_p
                                                                 : 0.5 * Sp[T_SQ] / n_p;
      o[0] = (double)a.reg_mult * (0.5 * Se[T_SQ] / n_e + second);
    }
    if (a.algo != OLY_IQ_ALGO_LSIQ_H) {
      o[3] = a.has_v && (a.iq_like || !lsiq) ? (Sp[T_V] + Se[T_V]) / n_all : 0.0;
      o[4] = Se[T_Q] / n_e;
      o[5] = Se[T_Q2] / n_e;
      o[6] = Sp[T_Q] / n_p;
      o[7] = Sp[T_Q2] / n_p;
      o[8] = (Sp[T_R] + Se[T_R]) / n_all;
      o[9] = Se[T_R] / n_e;
      o[10] = Sp[T_R] / n_p;
      o[11] = Se[T_Y] / n_e;
      o[12] = Sp[T_Y] / n_p;
      o[13] = Se[T_QABS] / Se[T_ABS];      // 0 / 0 = NaN for an empty subset, as torch.mean of nothing
      o[14] = Sp[T_QABS] / Sp[T_ABS];
      o[15] = sqrt(gn2);
    }
    for (int j = 0; j < 16; ++j) a.out[j] = o[j];
  }
  if (tid < D) {
    const double* d = reinterpret_cast<const double*>(a.ws + a.W.delta);
    const double Bd = (double)a.B;
    if (a.colstats) {
      double cnt = a.colstats[tid], sum = a.colstats[D + tid], sq = a.colstats[2 * D + tid];
      for (int p = 0; p < 4; ++p) {
        if ((p == 1 && a.use_target) || (p == 2 && !a.has_v) || (p == 3 && !a.v0)) continue;
        cnt += p == 3 ? (double)a.n_v0 : p == 2 ? (double)a.n_v : Bd;
        sum += d[p * 2 * IN_MAX + tid];
        sq += d[p * 2 * IN_MAX + IN_MAX + tid];
      }
      a.colstats[tid] = cnt;
      a.colstats[D + tid] = sum;
      a.colstats[2 * D + tid] = sq;
    }
    if (a.tcolstats && a.use_target) {
      a.tcolstats[tid] += Bd;
      a.tcolstats[D + tid] += d[2 * IN_MAX + tid];
      a.tcolstats[2 * D + tid] += d[2 * IN_MAX + IN_MAX + tid];
    }
  }
}

}  // namespace

extern "C" int64_t oly_iq_q_ws(int batch, int in_dim, int act_dim) {
  if (batch < 2 || batch > MAX_BATCH || in_dim <= 0 || act_dim <= 0 || act_dim > MAX_ACT || in_dim + act_dim > IN_MAX)
    return -1;
  return (int64_t)ws_layout(batch).total;
}

extern "C" int64_t oly_iq_q_ws_values(int batch, int in_dim, int act_dim) {
  if (oly_iq_q_ws(batch, in_dim, act_dim) < 0) return -1;
  return (int64_t)ws_layout(batch).qv;
}

extern "C" int oly_iq_q_update(oly_ctx* ctx, const oly_iq_q* f, oly_stream stream) {
  const char* name = "oly_iq_q_update";
  if (!ctx) return OLY_EINVAL;
  if (!f) OLY_FAIL(ctx, OLY_EINVAL, "%s: NULL argument", name);
  const int in_dim = f->in_dim, A = f->act_dim, B = f->batch, D = in_dim + A;
  // the block of plcy_loss_mode v0 and of all-expert batches: behind an argument block that says it is an oly_iq_q_ext
  const oly_iq_v0* vb = f->pad == OLY_IQ_Q_EXT ? reinterpret_cast<const oly_iq_q_ext*>(f)->v0 : nullptr;
  const bool all_expert = vb && vb->all_expert != 0;
  if (oly_iq_q_ws(B, in_dim, A) < 0 || f->n_policy < (all_expert ? 0 : 1) || f->n_policy >= B)
    OLY_FAIL(ctx, OLY_EINVAL,
             "%s: supported: 2 <= batch <= %d, in_dim >= 1, 1 <= act_dim <= %d, in_dim + act_dim <= %d, 1 <= n_policy < "
             "batch, n_policy 0 with the v0 block's all_expert alone (got batch %d, in %d, act %d, n_policy %d)",
             name, MAX_BATCH, MAX_ACT, IN_MAX, B, in_dim, A, f->n_policy);
  const bool iq = f->algo == OLY_IQ_ALGO_IQ, sqil = f->algo == OLY_IQ_ALGO_SQIL, lsiq = f->algo == OLY_IQ_ALGO_LSIQ;
  const bool hb = f->algo == OLY_IQ_ALGO_LSIQ_H;
  if (!iq && !sqil && !lsiq && !hb) OLY_FAIL(ctx, OLY_EINVAL, "%s: unknown algorithm %d", name, f->algo);
  const oly_lsiq* ls = lsiq || hb ? f->lsiq : nullptr;      // read for LSIQ and LSIQ_H alone
  if ((lsiq || hb) && !ls) OLY_FAIL(ctx, OLY_EINVAL, "%s: NULL lsiq block with algo OLY_IQ_ALGO_LSIQ / _LSIQ_H", name);
  const int md = f->plcy_loss_mode;
  bool iq_like = iq;
  if (hb) {      // the H update reads the block's bounds and its tail; the Q loss's enumerants are not its own
    if (!(ls->Q_min < ls->Q_max)) OLY_FAIL(ctx, OLY_EINVAL, "%s: Q_min %g must lie below Q_max %g", name, ls->Q_min, ls->Q_max);
    if (ls->h_loss != OLY_LSIQ_LOSS_MSE && ls->h_loss != OLY_LSIQ_LOSS_HUBER)
      OLY_FAIL(ctx, OLY_EINVAL, "%s: h_loss %d is neither OLY_LSIQ_LOSS_MSE nor OLY_LSIQ_LOSS_HUBER", name, ls->h_loss);
    if (ls->h_cost != 0 && ls->h_cost != 1) OLY_FAIL(ctx, OLY_EINVAL, "%s: h_cost %d is neither 0 nor 1", name, ls->h_cost);
    if (!(ls->h_tau_up >= 0.0 && ls->h_tau_up <= 1.0) || !(ls->h_tau_down >= 0.0 && ls->h_tau_down <= 1.0))
      OLY_FAIL(ctx, OLY_EINVAL, "%s: h_tau_up %g / h_tau_down %g outside [0, 1]", name, ls->h_tau_up, ls->h_tau_down);
    if (!f->use_target) OLY_FAIL(ctx, OLY_EINVAL, "%s: the H update needs use_target (H' is the target H)", name);
    if (md != 0 || f->regularizer_mode != 0)
      OLY_FAIL(ctx, OLY_EINVAL, "%s: the H update takes plcy_loss_mode 0 and regularizer_mode 0 (got %d, %d)", name, md,
               f->regularizer_mode);
    if (!(f->reg_mult > 0.f) && ls->h_cost) OLY_FAIL(ctx, OLY_EINVAL, "%s: h_cost needs reg_mult > 0", name);
    if ((ls->h_clip_expert && !ls->h_max_state) || (ls->h_cost && (!ls->h_q_t || !ls->h_v_t)))
      OLY_FAIL(ctx, OLY_EINVAL, "%s: NULL h_max_state (with h_clip_expert) or h_q_t / h_v_t (with h_cost)", name);
    if ((reinterpret_cast<uintptr_t>(ls->h_max_state) & 3) != 0)
      OLY_FAIL(ctx, OLY_EINVAL, "%s: h_max_state must be 4-byte aligned", name);
  }
  if (lsiq) {
    if (ls->lossQ_type != OLY_LSIQ_IQ_LIKE && ls->lossQ_type != OLY_LSIQ_SQIL_LIKE)
      OLY_FAIL(ctx, OLY_EINVAL, "%s: unknown lossQ_type %d", name, ls->lossQ_type);
    if (ls->loss_mode_exp != OLY_LSIQ_EXP_FIX && ls->loss_mode_exp != OLY_LSIQ_EXP_BOOTSTRAP)
      OLY_FAIL(ctx, OLY_EINVAL, "%s: unknown loss_mode_exp %d", name, ls->loss_mode_exp);
    if (ls->Q_exp_loss < OLY_LSIQ_LOSS_NONE || ls->Q_exp_loss > OLY_LSIQ_LOSS_HUBER)
      OLY_FAIL(ctx, OLY_EINVAL, "%s: unknown Q_exp_loss %d", name, ls->Q_exp_loss);
    if (!(ls->Q_min < ls->Q_max)) OLY_FAIL(ctx, OLY_EINVAL, "%s: Q_min %g must lie below Q_max %g", name, ls->Q_min, ls->Q_max);
    iq_like = ls->lossQ_type == OLY_LSIQ_IQ_LIKE;
    if (ls->Q_exp_loss == OLY_LSIQ_LOSS_NONE && (!iq_like || ls->loss_mode_exp == OLY_LSIQ_EXP_FIX))
      OLY_FAIL(ctx, OLY_EINVAL, "%s: loss_mode_exp fix and lossQ_type sqil_like need a Q_exp_loss (MSE or Huber)", name);
    if (!iq_like && md == OLY_LSIQ_SQ_VALUE && 2 * f->n_policy != B)
      OLY_FAIL(ctx, OLY_EINVAL, "%s: sqil_like with plcy_loss_mode value needs as many policy rows as expert rows (n_policy %d of %d)",
               name, f->n_policy, B);
  }
  const bool v0_family = iq || (lsiq && iq_like);
  if (vb && !v0_family)
    OLY_FAIL(ctx, OLY_EINVAL, "%s: the v0 block goes with OLY_IQ_ALGO_IQ and LSIQ's iq_like alone", name);
  const bool v0 = v0_family && md == OLY_IQ_V0;
  if (v0 && !vb) OLY_FAIL(ctx, OLY_EINVAL, "%s: plcy_loss_mode v0 needs the v0 block (oly_iq_q_ext)", name);
  if (v0 && (!vb->a_v0 || !vb->logp_v0)) OLY_FAIL(ctx, OLY_EINVAL, "%s: NULL a_v0 / logp_v0 in the v0 block", name);
  if (all_expert && (f->regularizer_mode == OLY_IQ_REG_PLCY || md == OLY_IQ_VALUE_POLICY || md == OLY_IQ_Q_OLD_POLICY ||
                     md == OLY_LSIQ_VALUE_Q_OLD_POLICY))
    OLY_FAIL(ctx, OLY_EINVAL, "%s: all_expert leaves no policy rows for plcy_loss_mode %d / regularizer_mode %d", name, md,
             f->regularizer_mode);
  if (hb     ? false
      : iq   ? (md < OLY_IQ_VALUE || md > OLY_IQ_V0)
      : sqil ? (md < OLY_SQIL_PLCY || md > OLY_SQIL_VALUE_PLCY)
      : iq_like ? (md < OLY_LSIQ_VALUE || md > OLY_LSIQ_OFF)
                : (md < OLY_LSIQ_SQ_VALUE || md > OLY_LSIQ_SQ_Q_OLD_POLICY))
    OLY_FAIL(ctx, OLY_EINVAL, "%s: unknown plcy_loss_mode %d", name, md);
  if (f->regularizer_mode < OLY_IQ_REG_EXP_AND_PLCY || f->regularizer_mode > OLY_IQ_REG_OFF)
    OLY_FAIL(ctx, OLY_EINVAL, "%s: unknown regularizer_mode %d", name, f->regularizer_mode);
  if (f->gradient_penalty_lambda > 0.f || f->gradient_penalty_lambda != f->gradient_penalty_lambda)
    OLY_FAIL(ctx, OLY_EINVAL, "%s: the gradient penalty is not built (gradient_penalty_lambda must be 0)", name);
  if (!(f->tau >= 0.0 && f->tau <= 1.0)) OLY_FAIL(ctx, OLY_EINVAL, "%s: tau %g outside [0, 1]", name, f->tau);
  // the pass on (obs | a_pi): always in IQ's family (getV(obs) runs in every mode, lsiq.py:72), in SQIL's but for plcy, in
  // LSIQ's sqil_like but for q_old_policy
  const bool has_v = !hb && (iq_like || (sqil ? md != OLY_SQIL_PLCY : md != OLY_LSIQ_SQ_Q_OLD_POLICY));
  const bool need_target = f->use_target || f->update_target;
  if (!f->obs || !f->act || !f->next_obs || !f->absorbing || !f->a_next || !f->logp_next || !f->param || !f->m || !f->v ||
      !f->packed || !f->ws || !f->out || (has_v && (!f->a_pi || !f->logp_pi)) ||
      (need_target && (!f->target_param || !f->target_packed)))
    OLY_FAIL(ctx, OLY_EINVAL, "%s: NULL pointer in the argument block", name);
  const WsL W = ws_layout(B);
  int rc = oly_fit::refuse_buffers(ctx, name, f->ws_floats, W.total, f->ws, f->packed, f->step, 1);
  if (rc != OLY_OK) return rc;
  if (need_target && (reinterpret_cast<uintptr_t>(f->target_packed) & 15) != 0)
    OLY_FAIL(ctx, OLY_EINVAL, "%s: target_packed must be 16-byte aligned", name);
  if (f->packed_floats < (int64_t)P_TOTAL || (need_target && f->target_packed_floats < (int64_t)P_TOTAL))
    OLY_FAIL(ctx, OLY_EINVAL, "%s: a packed stream holds %ld floats", name, (long)P_TOTAL);
  if ((reinterpret_cast<uintptr_t>(f->out) & 7) != 0 || (reinterpret_cast<uintptr_t>(f->colstats) & 7) != 0 ||
      (reinterpret_cast<uintptr_t>(f->target_colstats) & 7) != 0)
    OLY_FAIL(ctx, OLY_EINVAL, "%s: out and the colstats must be 8-byte aligned", name);

  QArgs a{};
  a.in_dim = in_dim;
  a.act_dim = A;
  a.D = D;
  a.B = B;
  a.n_policy = f->n_policy;
  a.algo = f->algo;
  a.loss_mode = f->plcy_loss_mode;
  a.reg_mode = f->regularizer_mode;
  a.treat_abs = f->treat_absorbing != 0;
  a.use_target = f->use_target != 0;
  a.update_target = f->update_target != 0;
  a.has_v = has_v;
  a.iq_like = iq_like;
  a.n_v = B;
  if (lsiq) {
    a.exp_mode = ls->loss_mode_exp;
    a.exp_loss = ls->Q_exp_loss;
    a.clip = ls->target_clipping != 0;
    a.q_min = ls->Q_min;
    a.q_max = ls->Q_max;
    a.inv_rm = (float)(1.0 / (double)f->reg_mult);
    a.g1 = 1.f / (1.f - f->gamma);
    if (!iq_like && md == OLY_LSIQ_SQ_VALUE_PLCY) a.n_v = f->n_policy;
  }
  if (hb) {
    a.q_min = ls->Q_min;
    a.q_max = ls->Q_max;
    a.inv_rm = (float)(1.0 / (double)f->reg_mult);
    a.h_loss = ls->h_loss;
    a.h_cost = ls->h_cost;
    a.h_clip = ls->h_clip_expert != 0;
    a.h_tu = (float)ls->h_tau_up;
    a.h_omu = (float)(1.0 - ls->h_tau_up);
    a.h_td = (float)ls->h_tau_down;
    a.h_omd = (float)(1.0 - ls->h_tau_down);
    a.h_omg = 1.f - f->gamma;
    a.h_lo = ls->h_cost ? -1000.f : -10000.f;
    a.h_hi = 1000.f;
    if (ls->h_cost) {   // Q2_max + 100, Q2_max = (1 / reg_mult)^2 / (1 - gamma): a double over a float32 tensor, which torch
                        // evaluates as the tensor's float32 reciprocal times the float32 of the double (lsiq_hc.py:61-62)
      const double r = 1.0 / (double)f->reg_mult;
      const float rec = 1.f / a.h_omg;
      const float q2 = rec * (float)(r * r);
      a.h_hi = q2 + 100.f;
    }
    a.h_max = ls->h_max_state;
    a.h_q_t = ls->h_q_t;
    a.h_v_t = ls->h_v_t;
  }
  int ns = 0;
  a.slot[0] = ns++;
  a.slot[1] = a.use_target ? -1 : ns++;
  a.slot[2] = has_v && !v0 ? ns++ : -1;    // v0: the pass on (obs | a_pi) feeds the Standardizer and the logged V alone
  a.slot[3] = v0 ? ns++ : -1;
  a.n_slots = ns;
  a.v0 = v0;
  a.n_v0 = B - f->n_policy;
  a.omg = 1.f - f->gamma;
  a.a_v0 = v0 ? vb->a_v0 : nullptr;
  a.logp_v0 = v0 ? vb->logp_v0 : nullptr;
  a.obs = f->obs;
  a.act = f->act;
  a.next_obs = f->next_obs;
  a.absorbing = f->absorbing;
  a.a_next = f->a_next;
  a.logp_next = f->logp_next;
  a.a_pi = f->a_pi;
  a.logp_pi = f->logp_pi;
  a.colstats = f->colstats;
  a.tcolstats = a.use_target ? f->target_colstats : nullptr;
  a.param = f->param;
  a.m = f->m;
  a.v = f->v;
  a.packed = f->packed;
  a.tparam = f->target_param;
  a.tpacked = f->target_packed;
  a.ws = f->ws;
  a.gamma = f->gamma;
  a.alpha = f->alpha;
  a.reg_mult = f->reg_mult;
  a.r_min = f->R_min;
  a.r_max = f->R_max;
  a.tau = (float)f->tau;
  a.omt = (float)(1.0 - f->tau);
  a.ad = oly_fit::adam_scalars(f->beta1, f->beta2, f->eps, f->lr, (long)f->step + 1);
  a.wd = f->weight_decay;
  a.out = f->out;
  a.P = param_layout(D, 1);
  a.W = W;

  const int tiles_a = (B + 15) / 16, tiles_b = weight_tiles(D, 1);
  hipLaunchKernelGGL(iq_prologue_kernel, dim3(PRO_BLOCKS), dim3(THREADS), 0, oly_s(stream), a);
  rc = hb ? launch_rows(ctx, ctx->iqq_attr_done, 4u, iq_rows_kernel<2, true>, iq_rows_kernel<4, true>, D, dim3(tiles_a),
                        ROWS_LDS, stream, a)
     : v0 ? launch_rows(ctx, ctx->iqq_attr_done, 16u, iq_rows_kernel<2, false, true>, iq_rows_kernel<4, false, true>, D,
                        dim3(tiles_a), ROWS_LDS_V0, stream, a)
          : launch_rows(ctx, ctx->iqq_attr_done, 1u, iq_rows_kernel<2>, iq_rows_kernel<4>, D, dim3(tiles_a), ROWS_LDS, stream, a);
  if (rc != OLY_OK) return rc;
  hipLaunchKernelGGL(iq_weights_kernel, dim3(tiles_b), dim3(THREADS), 0, oly_s(stream), a);
  hipLaunchKernelGGL(iq_fold_kernel, dim3(1), dim3(THREADS), 0, oly_s(stream), a, tiles_a, tiles_b);
  OLY_LAUNCH_CHECK(ctx, "soft-Q critic update kernels");
  return OLY_OK;
}
