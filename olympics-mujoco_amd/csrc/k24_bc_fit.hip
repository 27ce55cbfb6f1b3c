// K24: behavioural cloning (BehavioralCloning.fit_offline, imitation_lib/imitation/offline/behavioral_cloning.py:46-80)
// of the squashed-Gaussian policy IQ_Learn_Policy (imitation_lib/imitation/iq_sac.py:18-167): a
// FullyConnectedNetwork(in -> [512, 256] -> 2A, relu / relu / identity) whose output columns [0, A) are mu and [A, 2A)
// log_sigma, trained by Adam over torch.nn.GaussianNLLLoss() on the un-squashed demonstration actions.
//
//   oly_bc_targets    atanh(clip((a - central) / delta, -+(1 - 1e-7))) over the whole action table (:63-66), one launch.
//   oly_bc_fit_steps  n_steps iterations of fit_offline in one call.  Per call: oly_ilmlp_pack (the stream from param),
//                     bc_prologue_kernel (the transposed W2 and W3 streams of the backward, the statistics partials of
//                     step 0), then per step s
//   A  bc_rows_kernel     one 16-row tile per workgroup (8 waves): gather idx[s] rows, standardise with the statistics
//                         that include them (networks.py:68-81), the forward on the f32 matrix cores
//                         (v_mfma_f32_16x16x4_f32) in the forward kernel's chain order (ilmlp_common.h) with relu, the
//                         output layer's one or two column tiles by waves 0 / 1 as one chain over k < 256 each, the
//                         loss terms and dZ3 per element in fp64, dH2 = dZ3 W3 (matrix cores, transposed W3 stream),
//                         dZ2 = dH2 [h2 > 0], dH1 = dZ2 W2 (transposed W2 stream), dZ1 = dH1 [h1 > 0].  Activations and
//                         deltas go to the workspace in row quads ([row / 4][column][row % 4]); the tile's three loss
//                         sums to fixed slots.
//   B  bc_weights_kernel  one 16 x 16 weight tile per workgroup over W1, W2 and W3: dW = sum over the minibatch's rows of
//                         delta^T a (4 waves x a quarter of the 16-row steps each, added in wave order), weight decay,
//                         Adam, the stepped values into param, the moments, the packed stream and the transposed
//                         streams.  Workgroup 0 adds the loss partials, writes out[s] and colstats += minibatch s;
//                         workgroups 1 .. 16 sum step s+1's rows into the statistics partials launch A of s+1 reads.
// Every reduction has a fixed order and there are no atomics: two runs give identical bits, and a call of n steps
// leaves the bits of n calls of one step (the prologue rebuilds from param exactly what launch B keeps current).
// Adam, the statistics fold and the weights kernel's tail are fit_common.h's, shared with K15, K16 and K18; the two
// launches' common phases (the Standardizer's head, the rows' staging, the activation and its gradient, the row-quad
// stores, dZ1, the W2T build, the dW chain, the waves' meeting, the halving tree, the rows kernel's dispatch) are
// ilmlp_fit.h's, shared with K18, K26 and K27.
//
//   oly_bc_fit_steps_log  the same with the whole of logging() (:82-94): on a logging step, after launch B,
//   L  K25's kernel (k25_sg_act.hip) on the rows idx[s] with the stepped stream and the statistics that hold them twice
//   F  bc_log_fold_kernel  -mean(log_prob) into the step's fourth scalar; colstats += minibatch s a second time.
//
// With oly_bc_fit.pair (K28: the inverse action model's fit on a replay ring) the rows are (states[i, :d1] | x2[i, :d2])
// of two indexed tables and the target is un-squashed from the ring's raw actions in launch A.  The prologue and launch A
// are then the instantiations of the templates below over PairFitArgs (bc_fit.h), launch B is k28_iam.hip's kernel and
// launch L K25's over oly_sg::PairArgs; a call without a pair runs the FitArgs instantiations and bc_weights_kernel,
// which compile to the code they had.
#include <cstdlib>
#include <type_traits>

#include "bc_fit.h"
#include "ilmlp_fit.h"
#include "oly_common.h"
#include "sg_act.h"

namespace {
using namespace oly_ilfit;
using oly_fit::adam1;
using oly_fit::row_at;
using oly_fit::stats_slice;
using namespace oly_bc;

// grid PRO_BLOCKS: the transposed streams from param (grid-stride) and, workgroups 0 .. NSP-1, step 0's partials
template <class KA>
__global__ __launch_bounds__(THREADS) void bc_prologue_kernel(KA a) {
  __shared__ double part[8 * IN_MAX];
  build_w2t(a);
  for (int e = blockIdx.x * THREADS + threadIdx.x; e < OUTP * H2; e += PRO_BLOCKS * THREADS)
    a.ws[a.W.w3t + pt_index(OUTP, e / H2, e % H2)] = e / H2 < a.out_dim ? a.param[a.P.w3 + e] : 0.f;
  if (a.colstats && blockIdx.x < NSP) {
    if constexpr (PAIRED<KA>)
      pair_stats_slice(a, a.off, a.R, blockIdx.x, part);
    else
      stats_slice(a, a.off, a.R, blockIdx.x, part);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Launch A.  RTHREADS = 512 threads = 8 waves, two per SIMD (as K18: at the batches of this fit a CU holds one workgroup, so the
// second wave per SIMD is what covers the other's weight loads).  Chains: layer 1 wave w -> column tiles 4w .. 4w+3,
// layer 2 -> 2w, 2w+1, the output layer's tile t by wave t.  Backward: dH2 (wave w -> tiles 2w, 2w+1, the chain over the
// 32 padded outputs) and dH1 (wave w -> tiles 4w .. 4w+3, the chain over the 256 layer-2 units).
constexpr size_t ROWS_LDS_FLOATS = (size_t)(IN_MAX + H1 + 2 * H2) * 16 + 2 * OUTP * 16;
constexpr size_t ROWS_LDS = sizeof(float) * ROWS_LDS_FLOATS + sizeof(double) * (2 * IN_MAX + 3 * 256 + 48);
static_assert(ROWS_LDS_FLOATS % 4 == 0, "the fp64 arrays must be 8-byte aligned");

template <int G1, class KA>
__global__ __launch_bounds__(RTHREADS) void bc_rows_kernel(KA a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xT = lds;                       // [64 x 16]   standardised input (act16 images, mlp_tiles.h)
  float* hA = xT + IN_MAX * 16;          // [512 x 16]  h1
  float* hB = hA + H1 * 16;              // [256 x 16]  h2
  float* gz = hB + H2 * 16;              // [256 x 16]  dZ2
  float* z3 = gz + H2 * 16;              // [16][32]    the raw outputs by row
  float* gz3 = z3 + 16 * OUTP;           // [32 x 16]   dZ3
  double* st = reinterpret_cast<double*>(lds + ROWS_LDS_FLOATS);   // [2][IN_MAX] mean, std
  double* red = st + 2 * IN_MAX;         // [3][16][16] nll, clamped log_sigma, squared error by (row, action)
  double* rsum = red + 3 * 256;          // [3][16]     their sums by row
  __shared__ int rows_x[16];             // the tile's data rows (-1 beyond the minibatch)
  const float* P = a.packed;
  const float4* P4 = reinterpret_cast<const float4*>(P);
  const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, h4 = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row0 = blockIdx.x * 16, R = a.R, in_dim = a.in_dim, A = a.act_dim;
  const bool standardise = a.colstats != nullptr;
  float* ws = a.ws;
  float4* ws4 = reinterpret_cast<float4*>(ws);
  const size_t quad = (size_t)(row0 >> 2) + h4;      // this lane's accumulator rows: 4 h4 + i = one row quad

  if (standardise && tid < in_dim) {   // Standardizer.update_mean_std with the minibatch's rows (networks.py:76-81), as K18
    const double* sp = reinterpret_cast<const double*>(ws + a.W.statp);
    double s, ss;
    slice_sums(sp, tid, s, ss);
    double mean, sd;
    col_moments(a.colstats[tid] + (double)R, a.colstats[in_dim + tid] + s, a.colstats[2 * in_dim + tid] + ss, mean, sd);
    st[tid] = mean;
    st[IN_MAX + tid] = sd;
    if (blockIdx.x == 0) {
      double* d = reinterpret_cast<double*>(ws + a.W.delta);
      d[tid] = s;
      d[IN_MAX + tid] = ss;
    }
  }
  if (tid < 16) rows_x[tid] = row0 + tid < R ? row_at(a, a.off + row0 + tid) : -1;
  __syncthreads();
  if constexpr (PAIRED<KA>)
    stage_rows(xT, in_dim, standardise, st, [&](int m) { return rows_x[m] >= 0; },
               [&](int m, int k) { return pair_at(a, (size_t)rows_x[m], k); }, true, ws + a.W.xs, row0);
  else
    stage_rows(xT, in_dim, standardise, st, [&](int m) { return rows_x[m] >= 0; },
               [&](int m, int k) { return a.x[(size_t)rows_x[m] * in_dim + k]; }, true, ws + a.W.xs, row0);
  __syncthreads();
  {  // ---- layer 1: [16, in] x [in, 512]
    f32x4 acc[1][4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[0][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float4* a4[1] = {reinterpret_cast<const float4*>(xT)};
    tiles<G1, 4, 1>(a4, P4 + P_W1 / 4 + (size_t)(4 * wave) * (IN_MAX / 16) * 64, (IN_MAX / 16) * 64, lane, acc);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int col = 16 * (4 * wave + t) + c;
      const float bv = P[P_B1 + col];
      float4 h;
      h.x = Relu::f(acc[0][t][0] + bv);
      h.y = Relu::f(acc[0][t][1] + bv);
      h.z = Relu::f(acc[0][t][2] + bv);
      h.w = Relu::f(acc[0][t][3] + bv);
      hA[act16_index(col, 4 * h4)] = h.x;
      hA[act16_index(col, 4 * h4 + 1)] = h.y;
      hA[act16_index(col, 4 * h4 + 2)] = h.z;
      hA[act16_index(col, 4 * h4 + 3)] = h.w;
      ws4[(a.W.h1 >> 2) + quad * H1 + col] = h;
    }
  }
  __syncthreads();
  float4 h2r[2];
  {  // ---- layer 2: [16, 512] x [512, 256]
    f32x4 acc[1][2];
#pragma unroll
    for (int t = 0; t < 2; ++t) acc[0][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float4* a4[1] = {reinterpret_cast<const float4*>(hA)};
    tiles<H1 / 16, 2, 1>(a4, P4 + P_W2 / 4 + (size_t)(2 * wave) * (H1 / 16) * 64, (H1 / 16) * 64, lane, acc);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int col = 16 * (2 * wave + t) + c;
      const float bv = P[P_B2 + col];
      float4 h;
      h.x = Relu::f(acc[0][t][0] + bv);
      h.y = Relu::f(acc[0][t][1] + bv);
      h.z = Relu::f(acc[0][t][2] + bv);
      h.w = Relu::f(acc[0][t][3] + bv);
      hB[act16_index(col, 4 * h4)] = h.x;
      hB[act16_index(col, 4 * h4 + 1)] = h.y;
      hB[act16_index(col, 4 * h4 + 2)] = h.z;
      hB[act16_index(col, 4 * h4 + 3)] = h.w;
      h2r[t] = h;
      ws4[(a.W.h2 >> 2) + quad * H2 + col] = h;
    }
  }
  __syncthreads();
  if (wave < (a.out_dim > 16 ? 2 : 1)) {  // ---- the output layer's column tile `wave`: one chain over k < 256, as the forward kernel
    f32x4 acc[1][1] = {{f32x4{0.f, 0.f, 0.f, 0.f}}};
    const float4* a4[1] = {reinterpret_cast<const float4*>(hB)};
    tiles<H2 / 16, 1, 1>(a4, P4 + P_W3 / 4 + (size_t)wave * (H2 / 16) * 64, 0, lane, acc);
    const int col = 16 * wave + c;
    const float bv = P[P_B3 + col];
#pragma unroll
    for (int i = 0; i < 4; ++i) z3[(4 * h4 + i) * OUTP + col] = acc[0][0][i] + bv;
  }
  __syncthreads();
  {  // ---- GaussianNLLLoss(full=False, eps, 'mean')'s terms and dZ3, thread (row m, output column col)
    const int m = tid >> 5, col = tid & (OUTP - 1), row = rows_x[m];
    float g = 0.f;
    if (col < 2 * A) {
      const int j = col < A ? col : col - A;
      double t0 = 0.0, t1 = 0.0;
      if (row >= 0) {
        const float raw = z3[m * OUTP + A + j];
        const float ls = fminf(fmaxf(raw, a.ls_min), a.ls_max);                 // iq_sac.py:146
        const double sg = exp((double)ls), var = sg * sg, vc = fmax(var, (double)a.nll_eps);
        float target;
        if constexpr (PAIRED<KA>)
          target = pair_target(a, (size_t)row, A, j);
        else
          target = a.targets[(size_t)row * A + j];
        const double d = (double)z3[m * OUTP + j] - (double)target;
        const double r = d * d / vc, invn = 1.0 / ((double)R * (double)A);
        if (col < A) {
          g = (float)(d / vc * invn);
          t0 = 0.5 * (log(vc) + r);
          t1 = d * d;
        } else {
          // the variance floor is applied under no_grad, so the gradient passes through it: var / vc; the clamp's
          // mask is inclusive
          g = (raw >= a.ls_min && raw <= a.ls_max) ? (float)((1.0 - r) * (var / vc) * invn) : 0.f;
          t0 = (double)ls;
        }
      }
      if (col < A) {
        red[m * 16 + j] = t0;
        red[512 + m * 16 + j] = t1;
      } else {
        red[256 + m * 16 + j] = t0;
      }
    }
    gz3[act16_index(col, m)] = g;
    ws[a.W.dz3 + ((size_t)((row0 + m) >> 2) * OUTP + col) * 4 + (m & 3)] = g;
  }
  __syncthreads();
  if (tid < 48) {       // the three sums of row tid & 15, actions in order
    double s = 0.0;
    for (int j = 0; j < A; ++j) s += red[tid * 16 + j];
    rsum[tid] = s;
  }
  {  // ---- dZ2 = (dZ3 W3) [h2 > 0]
    f32x4 acc[1][2];
#pragma unroll
    for (int t = 0; t < 2; ++t) acc[0][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float4* a4[1] = {reinterpret_cast<const float4*>(gz3)};
    tiles<OUTP / 16, 2, 1>(a4, reinterpret_cast<const float4*>(ws) + (a.W.w3t >> 2) + (size_t)(2 * wave) * (OUTP / 16) * 64,
                           (OUTP / 16) * 64, lane, acc);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int col = 16 * (2 * wave + t) + c;
      float4 g;
      g.x = Relu::back(acc[0][t][0], h2r[t].x);
      g.y = Relu::back(acc[0][t][1], h2r[t].y);
      g.z = Relu::back(acc[0][t][2], h2r[t].z);
      g.w = Relu::back(acc[0][t][3], h2r[t].w);
      put_quad(gz, col, h4, g);
      ws4[(a.W.dz2 >> 2) + quad * H2 + col] = g;
    }
  }
  __syncthreads();
  if (tid < 3) {        // this tile's loss partials, rows in order
    double s = 0.0;
    for (int r = 0; r < 16; ++r) s += rsum[tid * 16 + r];
    double* lp = reinterpret_cast<double*>(ws + a.W.lossp);
    const size_t tiles_n = (size_t)gridDim.x;
    if (tid < 2) {
      lp[2 * blockIdx.x + tid] = s;
    } else {
      lp[2 * tiles_n + 2 * blockIdx.x] = s;
      lp[2 * tiles_n + 2 * blockIdx.x + 1] = 0.0;
    }
  }
  // ---- dZ1 = (dZ2 W2) [h1 > 0]
  dz1_tiles<Relu>(gz, reinterpret_cast<const float4*>(ws) + (a.W.w2t >> 2),
                  [&](int col) { return get_quad(hA, col, h4); }, ws4, a.W.dz1, quad);
}

// ---------------------------------------------------------------------------------------------------------------
// Launch B (the tiles: weight_tiles, ilmlp_fit.h; W3 is (1 or 2) x 16).  The decode and the step keep their own text here,
// which is ilmlp_fit.h's weight_tile and tile_step with the W2 / W3 mirrors in the step: through the two functions a step
// of the fit ran 0.2 to 0.4 us (0.5 to 0.8 %) longer in each of three alternating runs at batch 32 and 256 (HIP events).
__global__ __launch_bounds__(THREADS) void bc_weights_kernel(FitArgs a) {
  __shared__ float red[4 * 256];
  __shared__ float bred[4 * 64];
  __shared__ double dred[2 * THREADS];
  const int tid = threadIdx.x;
  const WsL& W = a.W;
  const ParamLayout& PL = a.P;
  const int kt0 = (a.in_dim + 15) / 16;
  int t = blockIdx.x, layer, nt, kt;
  if (t < 32 * kt0) {
    layer = 0, nt = t / kt0, kt = t % kt0;
  } else if ((t -= 32 * kt0) < 512) {
    layer = 1, nt = t / 32, kt = t % 32;
  } else {
    layer = 2, nt = (t - 512) / 16, kt = (t - 512) % 16;
  }
  // delta [R][dw] (N columns used) and activation [R][aw] (K columns used) of the layer, both in row quads
  const int dw = layer == 0 ? H1 : layer == 1 ? H2 : OUTP;
  const int N = layer == 2 ? a.out_dim : dw;
  const int aw = layer == 0 ? IN_MAX : layer == 1 ? H1 : H2;
  const int K = layer == 0 ? a.in_dim : aw;
  const float4* dl = reinterpret_cast<const float4*>(a.ws + (layer == 0 ? W.dz1 : layer == 1 ? W.dz2 : W.dz3));
  const float4* al = reinterpret_cast<const float4*>(a.ws + (layer == 0 ? W.xs : layer == 1 ? W.h1 : W.h2));
  const int n0 = 16 * nt, k0 = 16 * kt, R = a.R, steps = (R + 15) / 16;
  f32x4 acc;
  float bsum;
  dw_accumulate(dl, al, dw, aw, n0, N, k0, K, steps, acc, bsum);
  meet_waves(red, bred, acc, bsum);
  {
    const int nn = tid >> 4, kk = tid & 15, ne = n0 + nn, ke = k0 + kk;
    if (ne < N && ke < K) {
      const float g = ((red[tid] + red[256 + tid]) + red[512 + tid]) + red[768 + tid];
      if (layer == 0) {
        a.packed[pk_index(P_W1, IN_MAX / 16, ne, ke)] = adam1(a, PL.w1 + (size_t)ne * a.in_dim + ke, g);
      } else if (layer == 1) {
        const float p = adam1(a, PL.w2 + (size_t)ne * H1 + ke, g);
        a.packed[pk_index(P_W2, H1 / 16, ne, ke)] = p;
        a.ws[W.w2t + pt_index(H2, ne, ke)] = p;
      } else {
        const float p = adam1(a, PL.w3 + (size_t)ne * H2 + ke, g);
        a.packed[pk_index(P_W3, H2 / 16, ne, ke)] = p;
        a.ws[W.w3t + pt_index(OUTP, ne, ke)] = p;
      }
    }
    if (kt == 0 && tid < 16 && n0 + tid < N) {   // the bias: the column sums of delta, lane groups then waves in order
      const float gb = oly_fit::bias_colsum(bred, tid);
      const size_t pb = layer == 0 ? PL.b1 : layer == 1 ? PL.b2 : PL.b3;
      const size_t kb = layer == 0 ? P_B1 : layer == 1 ? P_B2 : P_B3;
      a.packed[kb + n0 + tid] = adam1(a, pb + n0 + tid, gb);
    }
  }
  if (blockIdx.x == 0) {   // ---- the step's three scalars (logging(), behavioral_cloning.py:82-94); colstats += minibatch s
    const double* lp = reinterpret_cast<const double*>(a.ws + W.lossp);
    oly_fit::loss_tree(steps, lp, dred);
    const double nll = dred[0], lsum = dred[THREADS];
    __syncthreads();
    oly_fit::loss_tree(steps, lp + 2 * (size_t)steps, dred);
    if (tid == 0) {
      const double n = (double)R * (double)a.act_dim;
      a.out[0] = nll / n;                                                       // GaussianNLLLoss
      a.out[1] = (double)a.act_dim * HALF_LOG_2PI_P1 + lsum / (double)R;         // entropy_from_logsigma, mean over rows
      a.out[2] = dred[0] / n;                                                   // F.mse_loss(mu, target)
    }
    if (a.colstats) oly_fit::colstats_add(a, R);
  } else if (blockIdx.x <= NSP && a.colstats && a.Rn > 0) {
    stats_slice(a, a.off_next, a.Rn, blockIdx.x - 1, dred);
  }
}

// targets = atanhf(clip((a - central) / delta, -+f32(1 - 1e-7)))   (behavioral_cloning.py:63-66, float32 as torch)
__global__ __launch_bounds__(256) void bc_targets_kernel(long n, int A, const float* __restrict__ act,
                                                         const float* __restrict__ central, const float* __restrict__ delta,
                                                         float* __restrict__ out) {
  const float hi = 0x1.fffffcp-1f;    // float32(1 - 1e-7) = 1 - 2^-23 = 0.99999988
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n * A; e += (long)gridDim.x * 256) {
    const int j = (int)(e % A);
    float u = (act[e] - central[j]) / delta[j];
    u = u < -hi ? -hi : u > hi ? hi : u;     // NaN passes through, as torch.clip
    out[e] = (float)atanh((double)u);        // correctly rounded: one launch per demonstration table, not per step
  }
}

// The logged fit's fourth scalar and the Standardizer's second take of the minibatch (logging(), behavioral_cloning.py:90-92).
// One workgroup: thread t adds the log-probabilities of rows 16 t .. 16 t + 15 in order (K25 left them after the
// workspace), the partials meet by loss_tree's halving tree, out[3] = -sum / R; colstats += the minibatch's sums again.
__global__ __launch_bounds__(THREADS) void bc_log_fold_kernel(FitArgs a) {
  __shared__ double dred[THREADS];
  const int tid = threadIdx.x, R = a.R;
  const float* lp = a.ws + a.W.total;
  double s = 0.0;
  for (int r = 16 * tid; r < min(R, 16 * tid + 16); ++r) s += (double)lp[r];
  const double sum = tree_sum(dred, s);
  if (tid == 0) a.out[3] = -sum / (double)R;      // "Squashed Gaussian Entropy (Empirical)"
  if (a.colstats) oly_fit::colstats_add(a, R);
}

}  // namespace

extern "C" int64_t oly_bc_fit_ws(int batch, int in_dim, int act_dim) {
  if (batch <= 0 || batch > MAX_BATCH || in_dim <= 0 || in_dim > IN_MAX || act_dim <= 0 || act_dim > MAX_ACT) return -1;
  return (int64_t)ws_layout(batch).total;
}

extern "C" int oly_bc_targets(oly_ctx* ctx, int64_t n, int act_dim, const float* actions, const float* central,
                              const float* delta, float* targets, oly_stream stream) {
  if (!ctx) return OLY_EINVAL;
  if (n < 0 || n > 0x7fffffffL || act_dim <= 0 || act_dim > MAX_ACT)
    OLY_FAIL(ctx, OLY_EINVAL, "oly_bc_targets: bad shape (n %ld, act_dim %d; 1 <= act_dim <= %d)", (long)n, act_dim, MAX_ACT);
  if (!actions || !central || !delta || !targets) OLY_FAIL(ctx, OLY_EINVAL, "oly_bc_targets: NULL argument");
  if (n == 0) return OLY_OK;
  const long total = (long)n * act_dim;
  const long blocks = (total + 255) / 256;
  const unsigned grid = (unsigned)(blocks < 1024 ? blocks : 1024);
  hipLaunchKernelGGL(bc_targets_kernel, dim3(grid), dim3(256), 0, oly_s(stream), (long)n, act_dim, actions, central, delta,
                     targets);
  OLY_LAUNCH_CHECK(ctx, "behavioural cloning targets kernel");
  return OLY_OK;
}

template <class KA>
static int run_steps(oly_ctx* ctx, const oly_bc_fit* f, int n_steps, const oly_bc_fit_log* lg, oly_stream stream, KA a,
                     unsigned bit);

// What oly_bc_fit_steps and oly_bc_fit_steps_log share. lg == NULL: oly_bc_fit_steps (out [n_steps, 3], its launches
// alone).  lg: out [n_steps, 4], and a step s with (iter0 + s) % logging_iter == 0 runs two more launches after launch B.
static int fit_steps(oly_ctx* ctx, const char* name, const oly_bc_fit* f, int n_steps, const oly_bc_fit_log* lg,
                     oly_stream stream) {
  const int in_dim = f->in_dim, A = f->act_dim, batch = f->batch;
  if (n_steps < 0 || f->n_rows <= 0 || oly_bc_fit_ws(batch, in_dim, A) < 0)
    OLY_FAIL(ctx, OLY_EINVAL,
             "%s: supported: 0 < batch <= %d, 0 < in_dim <= %d, 0 < act_dim <= %d, n_rows > 0, n_steps >= 0 "
             "(got batch %d, in %d, act %d, n_rows %d, n_steps %d)",
             name, MAX_BATCH, IN_MAX, MAX_ACT, batch, in_dim, A, f->n_rows, n_steps);
  if (const oly_bc_pair* pr = f->pair) {
    if (f->targets)
      OLY_FAIL(ctx, OLY_EINVAL, "%s: with pair the targets are formed from pair->actions (targets must be NULL)", name);
    if (!pr->x2 || !pr->actions || !pr->central || !pr->delta)
      OLY_FAIL(ctx, OLY_EINVAL, "%s: NULL x2 / actions / central / delta in pair", name);
    if (pr->d1 < 1 || pr->d2 < 1 || (long)pr->d1 + pr->d2 != in_dim)
      OLY_FAIL(ctx, OLY_EINVAL, "%s: pair needs d1 >= 1, d2 >= 1, d1 + d2 == in_dim (got %d, %d, in %d)", name, pr->d1, pr->d2,
               in_dim);
    if (pr->stride1 < pr->d1 || pr->stride2 < pr->d2)
      OLY_FAIL(ctx, OLY_EINVAL, "%s: a stride of pair below its width (stride1 %d, d1 %d; stride2 %d, d2 %d)", name,
               pr->stride1, pr->d1, pr->stride2, pr->d2);
  }
  if (!f->states || (!f->targets && !f->pair) || !f->idx || !f->param || !f->m || !f->v || !f->packed || !f->ws || !f->out)
    OLY_FAIL(ctx, OLY_EINVAL, "%s: NULL pointer in the argument block", name);
  if (!(f->log_std_min <= f->log_std_max) || !(f->nll_eps > 0.f))
    OLY_FAIL(ctx, OLY_EINVAL, "%s: log_std_min <= log_std_max and nll_eps > 0 are required", name);
  const WsL W = ws_layout(batch);
  const size_t ws_need = lg ? (size_t)oly_bc_fit_log_ws(batch, in_dim, A) : W.total;
  int rc = oly_fit::refuse_buffers(ctx, name, f->ws_floats, ws_need, f->ws, f->packed, f->step, n_steps);
  if (rc != OLY_OK) return rc;
  if ((reinterpret_cast<uintptr_t>(f->out) & 7) != 0 || (reinterpret_cast<uintptr_t>(f->colstats) & 7) != 0)
    OLY_FAIL(ctx, OLY_EINVAL, "%s: out and colstats must be 8-byte aligned", name);
  if (lg) {
    if (lg->logging_iter < 1 || lg->iter0 < 0 || (long)lg->iter0 + n_steps > 0x7fffffffL)
      OLY_FAIL(ctx, OLY_EINVAL, "%s: logging_iter >= 1 and iter0 >= 0 are required (got %d, %d)", name, lg->logging_iter,
               lg->iter0);
    // the first logging step of the call, if it has one
    const long first = ((long)lg->logging_iter - lg->iter0 % lg->logging_iter) % lg->logging_iter;
    if (first < n_steps && !lg->eps) OLY_FAIL(ctx, OLY_EINVAL, "%s: a step of the call logs and eps is NULL", name);
  }
  if (n_steps == 0) return OLY_OK;
  PairFitArgs pa{};
  FitArgs& a = pa;
  a.in_dim = a.ds = in_dim;
  a.n_rows = f->n_rows;
  a.act_dim = A;
  a.out_dim = 2 * A;
  a.perm = f->idx;
  a.x = f->states;
  a.targets = f->targets;
  a.colstats = f->colstats;
  a.param = f->param;
  a.m = f->m;
  a.v = f->v;
  a.packed = f->packed;
  a.ws = f->ws;
  a.ls_min = f->log_std_min;
  a.ls_max = f->log_std_max;
  a.nll_eps = f->nll_eps;
  a.wd = f->weight_decay;
  a.P = param_layout(in_dim, 2 * A);
  a.W = W;
  a.R = batch;
  if (!f->pair) return run_steps<FitArgs>(ctx, f, n_steps, lg, stream, a, 1u);
  pa.d1 = f->pair->d1;
  pa.d2 = f->pair->d2;
  pa.stride1 = f->pair->stride1;
  pa.stride2 = f->pair->stride2;
  pa.x2 = f->pair->x2;
  pa.actions = f->pair->actions;
  pa.central = f->pair->central;
  pa.delta = f->pair->delta;
  return run_steps<PairFitArgs>(ctx, f, n_steps, lg, stream, pa, 4u);
}

// The launches of a call over the argument block KA: FitArgs, or PairFitArgs with oly_bc_fit.pair (`bit`: the rows
// kernel's first flag in the context's bcfit_attr_done).
template <class KA>
static int run_steps(oly_ctx* ctx, const oly_bc_fit* f, int n_steps, const oly_bc_fit_log* lg, oly_stream stream, KA a,
                     unsigned bit) {
  const int in_dim = f->in_dim, A = f->act_dim, batch = f->batch;
  const WsL& W = a.W;
  const float* p = f->param;
  const ParamLayout& P = a.P;
  int rc = oly_ilmlp_pack(ctx, in_dim, H1, H2, 2 * A, p + P.w1, p + P.b1, p + P.w2, p + P.b2, p + P.w3, p + P.b3, f->packed,
                      stream);
  if (rc != OLY_OK) return rc;
  a.off = 0;
  hipLaunchKernelGGL(bc_prologue_kernel<KA>, dim3(PRO_BLOCKS), dim3(THREADS), 0, oly_s(stream), a);
  const dim3 grid_a((unsigned)((batch + 15) / 16)), grid_b((unsigned)weight_tiles(in_dim, 2 * A));
  const size_t out_w = lg ? 4 : 3;
  long logged = 0;
  for (int s = 0; s < n_steps; ++s) {
    a.off = (long)s * batch;
    a.off_next = a.off + batch;
    a.Rn = s + 1 < n_steps ? batch : 0;
    a.ad = oly_fit::adam_scalars(f->beta1, f->beta2, f->eps, f->lr, (long)f->step + s + 1);
    a.out = f->out + out_w * (size_t)s;
    rc = launch_rows(ctx, ctx->bcfit_attr_done, bit, bc_rows_kernel<2, KA>, bc_rows_kernel<4, KA>, in_dim, grid_a, ROWS_LDS,
                     stream, a);
    if (rc != OLY_OK) return rc;
    if constexpr (PAIRED<KA>)
      oly_bc::launch_weights_pair(a, grid_b, stream);
    else
      hipLaunchKernelGGL(bc_weights_kernel, grid_b, dim3(THREADS), 0, oly_s(stream), a);
    if (lg && ((long)lg->iter0 + s) % lg->logging_iter == 0) {
      // logging() (behavioral_cloning.py:82-94): compute_action_and_log_prob on the minibatch.  colstats holds idx[s] once
      // (launch B) and the workspace's delta its column sums (launch A): the forward standardises with colstats + delta,
      // the fold adds delta to colstats.
      std::conditional_t<PAIRED<KA>, oly_sg::PairArgs, oly_sg::Args> g{};
      if constexpr (PAIRED<KA>) {
        g.d1 = a.d1;
        g.stride1 = a.stride1;
        g.stride2 = a.stride2;
        g.x2 = a.x2;
      }
      g.N = batch;
      g.in_dim = in_dim;
      g.act_dim = A;
      g.x = f->states;
      g.rows = f->idx + a.off;
      g.n_rows = f->n_rows;
      g.colstats = f->colstats;
      g.extra = f->colstats ? reinterpret_cast<const double*>(f->ws + W.delta) : nullptr;
      g.extra_cnt = (double)batch;
      g.packed = f->packed;
      g.ls_min = f->log_std_min;
      g.ls_max = f->log_std_max;
      g.eps = lg->eps + (size_t)logged * batch * A;
      g.log_prob = f->ws + W.total;
      rc = oly_sg::launch(ctx, g, stream);
      if (rc != OLY_OK) return rc;
      hipLaunchKernelGGL(bc_log_fold_kernel, dim3(1), dim3(THREADS), 0, oly_s(stream), static_cast<const FitArgs&>(a));
      ++logged;
    }
  }
  OLY_LAUNCH_CHECK(ctx, "behavioural cloning fit kernels");
  return OLY_OK;
}

extern "C" int oly_bc_fit_steps(oly_ctx* ctx, const oly_bc_fit* f, int n_steps, oly_stream stream) {
  if (!ctx) return OLY_EINVAL;
  if (!f) OLY_FAIL(ctx, OLY_EINVAL, "oly_bc_fit_steps: NULL argument");
  return fit_steps(ctx, "oly_bc_fit_steps", f, n_steps, nullptr, stream);
}

// the logged fit's workspace: oly_bc_fit_steps' and the minibatch's log-probabilities [batch rounded up to 16] f32
extern "C" int64_t oly_bc_fit_log_ws(int batch, int in_dim, int act_dim) {
  const int64_t n = oly_bc_fit_ws(batch, in_dim, act_dim);
  return n < 0 ? n : n + (batch + 15) / 16 * 16;
}

extern "C" int oly_bc_fit_steps_log(oly_ctx* ctx, const oly_bc_fit_log* f, int n_steps, oly_stream stream) {
  if (!ctx) return OLY_EINVAL;
  if (!f) OLY_FAIL(ctx, OLY_EINVAL, "oly_bc_fit_steps_log: NULL argument");
  return fit_steps(ctx, "oly_bc_fit_steps_log", &f->fit, n_steps, f, stream);
}
