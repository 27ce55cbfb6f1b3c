// K15: one epoch of the VAIL discriminator's fit (_fit_discriminator, imitation_lib/imitation/gail_TRPO.py:167-220,
// states only) in one call: mushroom's minibatch loop over the concatenated policy + demonstration rows, per minibatch
// Standardizer.forward (networks.py:68-81), VariationalNet.forward (:258-284), VDBLoss (utils/math.py:52-81, beta's
// dual update included), backward and torch.optim.Adam.  Network: in <= 64 -> 256 -> 128 (relu, relu), mu / logvar
// 128 -> 128, decoder 128 -> 1, the shape K12 serves.
//
// Launches per call: oly_disc_pack (the K12 stream from param), fitd_prologue_kernel (the transposed weight streams of
// the backward, the statistics partials of minibatch 0), then per minibatch b
//   A  fitd_rows_kernel     one 16-row tile per workgroup: gather perm rows, standardise with the statistics that
//                           include minibatch b, the forward on the f32 matrix cores (v_mfma_f32_16x16x4_f32) from the
//                           K12 stream with K12's chain order and exp32, the per-row loss terms, and every data
//                           gradient (dd, dmu, dlogvar, dEnc, dH1, also on the matrix cores).  Activations and deltas go
//                           to the workspace row-major; per-tile loss partials to fixed slots.
//   B  fitd_weights_kernel  one 16 x 16 weight tile per workgroup: dW = sum over the minibatch's rows of delta^T a
//                           (4 waves x a quarter of the rows each, added in wave order), weight decay, Adam, and the
//                           stepped values into param, the moments, both layouts of the K12 stream and the transposed
//                           streams.  Workgroup 0 adds the loss partials, steps beta and writes the per-minibatch
//                           outputs and colstats += minibatch b; workgroups 1 .. 16 sum minibatch b+1's rows into the
//                           statistics partials launch A of b+1 reads.
// Every reduction has a fixed order and there are no atomics: two runs give identical bits.  What this fit shares with
// K16 and K18 (Adam, the statistics fold, the weights kernel's tail, the epoch driver's host side) is in fit_common.h.
//
// oly_disc_fit_epoch_pair is the same epoch on a paired input (oly_disc_pair: (s, s') with use_next_states, (s, a) with
// actions; VariationalNet.forward, networks.py:258-278): launch A gathers perm rows from both sources, standardises the
// states with colstats + the minibatch's states and the next states with that + the minibatch's next states (actions
// raw); the statistics partials carry both sets of column sums and workgroup 0's colstats += adds both.  The states-only
// entry point is the paired one with no second part.
#include <cstdlib>

#include "disc_common.h"
#include "fit_common.h"
#include "mlp_tiles.h"
#include "oly_common.h"

namespace {
using oly_disc::DiscLayout;
using oly_disc::disc_layout;
using oly_disc::exp32;
using oly_disc::G1N16;
using oly_disc::H1;
using oly_disc::H2;
using oly_disc::MAX_IN;
using oly_disc::ZD;
using oly_fit::adam1;
using oly_fit::NSP;
using oly_fit::pt_index;
using oly_fit::row_at;
using oly_fit::stats_slice;
using oly_fit::THREADS;
using oly_mlp::act16_index;
using oly_mlp::f32x4;
using oly_mlp::layer_tiles16;

constexpr int MAX_BATCH = 4096;

// flat parameters, oly_disc_pack's argument order
struct ParamL {
  size_t w0, b0, w1, b1, wmu, bmu, wlv, blv, wd, bd, total;
};
__host__ __device__ inline ParamL param_layout(int in_dim) {
  ParamL P;
  P.w0 = 0;
  P.b0 = (size_t)H1 * in_dim;
  P.w1 = P.b0 + H1;
  P.b1 = P.w1 + (size_t)H2 * H1;
  P.wmu = P.b1 + H2;
  P.bmu = P.wmu + (size_t)ZD * H2;
  P.wlv = P.bmu + ZD;
  P.blv = P.wlv + (size_t)ZD * H2;
  P.wd = P.blv + ZD;
  P.bd = P.wd + ZD;
  P.total = P.bd + 1;
  return P;
}

// workspace (floats), BP = batch rounded up to 16 rows:
//   xs [BP][64] standardised rows | h1 [BP][256] | h2 [BP][128] | z [BP][128] | dmu, dlv, dEnc (relu-masked) [BP][128]
//   | dH1 (relu-masked) [BP][256] | dd [BP] | loss partials [BP / 16][2] f64 | statistics partials [NSP][2][64] f64 |
//   the minibatch's column sums [2][64] f64 | transposed streams W1T, WmuT, WlvT
struct WsL {
  size_t xs, h1, h2, z, dmu, dlv, denc, dh1, dd, lossp, statp, delta, w1t, wmut, wlvt, total;
};
__host__ __device__ inline WsL ws_layout(int batch) {
  const size_t BP = (size_t)(batch + 15) / 16 * 16;
  WsL W;
  W.xs = 0;
  W.h1 = W.xs + BP * MAX_IN;
  W.h2 = W.h1 + BP * H1;
  W.z = W.h2 + BP * H2;
  W.dmu = W.z + BP * ZD;
  W.dlv = W.dmu + BP * ZD;
  W.denc = W.dlv + BP * ZD;
  W.dh1 = W.denc + BP * H2;
  W.dd = W.dh1 + BP * H1;
  W.lossp = W.dd + BP;
  W.statp = W.lossp + BP / 16 * 4;
  W.delta = W.statp + (size_t)NSP * 2 * MAX_IN * 2;
  W.w1t = W.delta + 2 * MAX_IN * 2;
  W.wmut = W.w1t + (size_t)H2 * H1;
  W.wlvt = W.wmut + (size_t)ZD * H2;
  W.total = W.wlvt + (size_t)ZD * H2;
  return W;
}

// offsets of W[n][k] in the K12 stream: the 32-column-tile layout (packed_weight) and the 16-column one (packed_weight16)
__device__ __forceinline__ size_t p32_index(size_t base, int groups, int n, int k) {
  const int lane = (n & 31) | ((k & 1) << 5), q = (k >> 1) & 3;
  return base + ((size_t)((n >> 5) * groups + (k >> 3)) * 64 + lane) * 4 + q;
}
__device__ __forceinline__ size_t p16_index(size_t base, int groups, int n, int k) {
  const int lane = (n & 15) | ((k & 3) << 4), q = (k >> 2) & 3;
  return base + ((size_t)((n >> 4) * groups + (k >> 4)) * 64 + lane) * 4 + q;
}
// W1T, WmuT and WlvT are B operands of the data gradients dX = dY W (pt_index, fit_common.h)

struct FitArgs {
  int in_dim, n_rows, n_plcy;
  int ds, d2, std2, stride2; // x [n_rows, ds] | x2 [n_rows, stride2]'s first d2 columns (d2 = in_dim - ds, 0: none);
  const float* x2;           // std2: x2 goes through the Standardizer (next states), else raw (actions)
  int R, Rn;                 // rows of minibatch b / b+1 (0: none)
  long off, off_next;        // first position of minibatch b / b+1 in perm and eps
  const int32_t* perm;
  const float *x, *targets, *eps;
  double* colstats;
  float *param, *m, *v, *packed, *ws, *beta;
  float info_c, lr_beta;
  oly_fit::AdamK ad;
  float wd;                  // weight_decay
  double *loss_out, *bce_out, *kl_out;   // + b, or NULL
  float* beta_out;
  DiscLayout L;
  ParamL P;
  WsL W;
};

// grid PRO_BLOCKS: the transposed streams from param (grid-stride) and, workgroups 0 .. NSP-1, minibatch 0's partials
constexpr int PRO_BLOCKS = 64;
__global__ __launch_bounds__(THREADS) void fitd_prologue_kernel(FitArgs a) {
  __shared__ double part[8 * MAX_IN];
  const int n1 = H2 * H1, nm = ZD * H2;
  for (int e = blockIdx.x * THREADS + threadIdx.x; e < n1 + 2 * nm; e += PRO_BLOCKS * THREADS) {
    if (e < n1) {
      a.ws[a.W.w1t + pt_index(H2, e / H1, e % H1)] = a.param[a.P.w1 + e];
    } else {
      const int i = (e - n1) % nm;
      const bool mu = e < n1 + nm;
      a.ws[(mu ? a.W.wmut : a.W.wlvt) + pt_index(ZD, i / H2, i % H2)] = a.param[(mu ? a.P.wmu : a.P.wlv) + i];
    }
  }
  if (blockIdx.x < NSP) stats_slice(a, a.off, a.R, blockIdx.x, part);
}

// ---------------------------------------------------------------------------------------------------------------
// Launch A.  256 threads = 4 waves.  Forward as disc_forward16_kernel (K12): layer 1 wave w -> column tiles 4w .. 4w+3,
// layer 2 -> 2w, 2w+1, mu / logvar -> 2w, 2w+1 of both; the decoder by wave 0 as two 64-long chains added.  Backward:
// dEnc (wave w -> tiles 2w, 2w+1: the chain over z for dmu W_mu, continued over dlogvar W_lv) and dH1 (wave w -> tiles
// 4w .. 4w+3, the chain over the 128 encoder outputs).
constexpr size_t ROWS_LDS_FLOATS = (size_t)(MAX_IN + H1 + H2 + 4 * ZD) * 16 + 16 * ZD + ZD + 4 + 16;
constexpr size_t ROWS_LDS = sizeof(float) * ROWS_LDS_FLOATS + sizeof(double) * (2 * MAX_IN + 2 * 16);
static_assert(ROWS_LDS_FLOATS % 2 == 0, "the fp64 arrays must be 8-byte aligned");

template <int G1>
__global__ __launch_bounds__(THREADS) void fitd_rows_kernel(FitArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xT = lds;                       // [64 x 16]   standardised input (act16 images, mlp_tiles.h)
  float* hA = xT + MAX_IN * 16;          // [256 x 16]  h1
  float* hB = hA + H1 * 16;              // [128 x 16]  h2
  float* zT = hB + H2 * 16;              // [128 x 16]  z
  float* gmu = zT + ZD * 16;             // [128 x 16]  dmu
  float* glv = gmu + ZD * 16;            // [128 x 16]  dlogvar
  float* gen = glv + ZD * 16;            // [128 x 16]  dEnc (relu-masked)
  float* klt = gen + H2 * 16;            // [16][128]   the KL terms by row
  float* wd = klt + 16 * ZD;             // [ZD + 4]    decoder row + bias
  float* dds = wd + ZD + 4;              // [16]        dd by row
  double* st = reinterpret_cast<double*>(lds + ROWS_LDS_FLOATS);   // [2][MAX_IN] mean, std
  double* red = st + 2 * MAX_IN;         // [2][16] bce, KL by row
  __shared__ int rows_x[16];              // the tile's data rows (-1 beyond the minibatch)
  const DiscLayout& L = a.L;
  const float* P = a.packed;
  const float4* P4 = reinterpret_cast<const float4*>(P);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, h4 = lane >> 4;
  const int row0 = blockIdx.x * 16, R = a.R, in_dim = a.in_dim;
  float* ws = a.ws;

  if (tid < in_dim) {   // Standardizer.update_mean_std with the minibatch's rows (networks.py:76-81), as K16
    const double* sp = reinterpret_cast<const double*>(ws + a.W.statp);
    const int ds = a.ds;
    double s = 0.0, ss = 0.0;
    for (int p = 0; p < NSP; ++p) {
      s += sp[p * 2 * MAX_IN + tid];
      ss += sp[p * 2 * MAX_IN + MAX_IN + tid];
    }
    double mean = 0.0, sd = 1.0;        // an action column passes through: f32((f64(a) - 0) / 1) is a
    if (tid < ds) {
      const double cnt = a.colstats[tid] + (double)R + 1e-2;
      mean = (a.colstats[ds + tid] + s) / cnt;
      sd = sqrt(fmax((a.colstats[2 * ds + tid] + ss + 1e-2) / cnt - mean * mean, 1e-2));
    } else if (a.std2) {
      // a next-state column: the Standardizer has taken the minibatch's states in, then its next states
      // (VariationalNet.forward, networks.py:266-270), so column j's statistics hold both sets of sums
      const int j = tid - ds;
      double s1 = 0.0, ss1 = 0.0;
      for (int p = 0; p < NSP; ++p) {
        s1 += sp[p * 2 * MAX_IN + j];
        ss1 += sp[p * 2 * MAX_IN + MAX_IN + j];
      }
      const double cnt = a.colstats[j] + (double)R + (double)R + 1e-2;
      mean = ((a.colstats[ds + j] + s1) + s) / cnt;
      sd = sqrt(fmax(((a.colstats[2 * ds + j] + ss1) + ss + 1e-2) / cnt - mean * mean, 1e-2));
    }
    st[tid] = mean;
    st[MAX_IN + tid] = sd;
    if (blockIdx.x == 0) {
      double* d = reinterpret_cast<double*>(ws + a.W.delta);
      d[tid] = s;
      d[MAX_IN + tid] = ss;
    }
  }
  if (tid < ZD + 4) wd[tid] = P[L.wd + tid];
  if (tid < 16) rows_x[tid] = row0 + tid < R ? row_at(a, a.off + row0 + tid) : -1;
  __syncthreads();
  for (int e = tid; e < 16 * MAX_IN; e += THREADS) {
    const int m = e / MAX_IN, k = e & (MAX_IN - 1), row = rows_x[m];
    float v = 0.f;
    // f32((f64(x) - mean) / std): the reference subtracts fp64 statistics and narrows afterwards (networks.py:68-74)
    if (row >= 0 && k < in_dim) {
      const float* src = k < a.ds ? a.x + ((size_t)row * a.ds + k) : a.x2 + ((size_t)row * a.stride2 + (k - a.ds));
      v = (float)(((double)*src - st[k]) / st[MAX_IN + k]);
    }
    xT[act16_index(k, m)] = v;
    if (row >= 0) ws[a.W.xs + (size_t)(row0 + m) * MAX_IN + k] = v;
  }
  __syncthreads();
  // this lane's accumulator rows: 4 h4 + i
  auto store_act = [&](const f32x4& acc, float bias, int col, float* img, size_t wofs, int width) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = 4 * h4 + i;
      float v = acc[i] + bias;
      v = (v > 0.f || v != v) ? v : 0.f;     // relu, NaN kept like torch
      img[act16_index(col, m)] = v;
      if (row0 + m < R) ws[wofs + (size_t)(row0 + m) * width + col] = v;
    }
  };
  {  // ---- layer 1: [16, in] x [in, 256]
    f32x4 acc[4] = {{0}, {0}, {0}, {0}};
    const float4* const base = P4 + (L.w0n >> 2) + (size_t)(4 * wave) * G1N16 * 64;
    const float4* const w[4] = {base, base + G1N16 * 64, base + 2 * G1N16 * 64, base + 3 * G1N16 * 64};
    layer_tiles16<G1, 4>(reinterpret_cast<const float4*>(xT), w, lane, acc);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int col = 16 * (4 * wave + t) + c;
      store_act(acc[t], P[L.b0 + col], col, hA, a.W.h1, H1);
    }
  }
  __syncthreads();
  {  // ---- layer 2: [16, 256] x [256, 128]
    f32x4 acc[2] = {{0}, {0}};
    const float4* const base = P4 + (L.w1n >> 2) + (size_t)(2 * wave) * (H1 / 16) * 64;
    const float4* const w[2] = {base, base + (H1 / 16) * 64};
    layer_tiles16<H1 / 16, 2>(reinterpret_cast<const float4*>(hA), w, lane, acc);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int col = 16 * (2 * wave + t) + c;
      store_act(acc[t], P[L.b1 + col], col, hB, a.W.h2, H2);
    }
  }
  float ev[2][4];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = 4 * h4 + i;
      ev[t][i] = row0 + m < R ? a.eps[(size_t)(a.off + row0 + m) * ZD + 16 * (2 * wave + t) + c] : 0.f;
    }
  __syncthreads();
  float mu_r[2][4], lv_r[2][4], se_r[2][4];
  {  // ---- mu and logvar: [16, 128] x [128, 128] each; z = mu + exp(logvar / 2) eps (reparameterize)
    f32x4 acc[4] = {{0}, {0}, {0}, {0}};
    const float4* const bm = P4 + (L.wmun >> 2) + (size_t)(2 * wave) * (H2 / 16) * 64;
    const float4* const bl = P4 + (L.wlvn >> 2) + (size_t)(2 * wave) * (H2 / 16) * 64;
    const float4* const w[4] = {bm, bm + (H2 / 16) * 64, bl, bl + (H2 / 16) * 64};
    layer_tiles16<H2 / 16, 4>(reinterpret_cast<const float4*>(hB), w, lane, acc);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int col = 16 * (2 * wave + t) + c;
      const float bmu = P[L.bmu + col], blv = P[L.blv + col];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = 4 * h4 + i;
        const float mu = acc[t][i] + bmu, lv = acc[2 + t][i] + blv;
        const float se = exp32(lv / 2.0f) * ev[t][i];
        const float z = mu + se;
        mu_r[t][i] = mu;
        lv_r[t][i] = lv;
        se_r[t][i] = se;
        zT[act16_index(col, m)] = z;
        // kl_divergence's terms (math.py:88-89): mu^2 + exp(logvar) - logvar - 1
        klt[m * ZD + col] = row0 + m < R ? ((mu * mu + exp32(lv)) - lv) - 1.0f : 0.f;
        if (row0 + m < R) ws[a.W.z + (size_t)(row0 + m) * ZD + col] = z;
      }
    }
  }
  __syncthreads();
  const float invR = 1.0f / (float)R;
  if (wave == 0) {  // ---- decoder, BCEWithLogits and dd = (sigmoid(d) - t) / R: lane (row r, half) chains k in [64 half, +64)
    const int r = lane & 15, half = (lane >> 4) & 1;
    float s = 0.f;
#pragma unroll 16
    for (int k = 0; k < 64; ++k) s = fmaf(zT[act16_index(64 * half + k, r)], wd[64 * half + k], s);
    const float o = __shfl_xor(s, 16, 64);
    if (lane < 16) {
      const int row = rows_x[r];
      double bce = 0.0;
      float dd = 0.f;
      if (row >= 0) {
        const float d = (s + o) + wd[ZD];
        const float t = a.targets ? a.targets[row] : (row < a.n_plcy ? 0.f : 1.f);
        const double dv = d;
        bce = fmax(dv, 0.0) - dv * (double)t + log1p(exp(-fabs(dv)));
        dd = (float)(1.0 / (1.0 + exp(-dv)) - (double)t) * invR;
        ws[a.W.dd + row0 + r] = dd;
      }
      red[r] = bce;
      dds[r] = dd;
    }
  } else if (wave == 1 && lane < 16) {   // 0.5 * sum over the 128 latent columns, in order
    double s = 0.0;
    for (int j = 0; j < ZD; ++j) s += (double)klt[lane * ZD + j];
    red[16 + lane] = 0.5 * s;
  }
  __syncthreads();
  if (tid == 0) {       // this tile's loss partials, rows in order
    double b = 0.0, k = 0.0;
    for (int r = 0; r < 16; ++r) {
      b += red[r];
      k += red[16 + r];
    }
    double* lp = reinterpret_cast<double*>(ws + a.W.lossp) + 2 * blockIdx.x;
    lp[0] = b;
    lp[1] = k;
  }
  {  // ---- dmu = dz + beta mu / R, dlogvar = dz exp(logvar / 2) eps / 2 + beta (exp(logvar) - 1) / (2 R); dz = dd wd
    const float bR = a.beta[0] * invR;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int col = 16 * (2 * wave + t) + c;
      const float wdc = wd[col];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = 4 * h4 + i;
        float gm = 0.f, gl = 0.f;
        if (row0 + m < R) {
          const float dz = dds[m] * wdc;
          gm = dz + bR * mu_r[t][i];
          gl = dz * 0.5f * se_r[t][i] + bR * 0.5f * (exp32(lv_r[t][i]) - 1.0f);
          ws[a.W.dmu + (size_t)(row0 + m) * ZD + col] = gm;
          ws[a.W.dlv + (size_t)(row0 + m) * ZD + col] = gl;
        }
        gmu[act16_index(col, m)] = gm;
        glv[act16_index(col, m)] = gl;
      }
    }
  }
  __syncthreads();
  const float4* T4 = reinterpret_cast<const float4*>(ws);
  {  // ---- dEnc = (dmu W_mu + dlogvar W_lv) * [h2 > 0]
    f32x4 acc[2] = {{0}, {0}};
    const float4* const bm = T4 + (a.W.wmut >> 2) + (size_t)(2 * wave) * (ZD / 16) * 64;
    const float4* const bl = T4 + (a.W.wlvt >> 2) + (size_t)(2 * wave) * (ZD / 16) * 64;
    const float4* const wm[2] = {bm, bm + (ZD / 16) * 64};
    const float4* const wl[2] = {bl, bl + (ZD / 16) * 64};
    layer_tiles16<ZD / 16, 2>(reinterpret_cast<const float4*>(gmu), wm, lane, acc);
    layer_tiles16<ZD / 16, 2>(reinterpret_cast<const float4*>(glv), wl, lane, acc);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int col = 16 * (2 * wave + t) + c;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = 4 * h4 + i;
        const float v = hB[act16_index(col, m)] > 0.f ? acc[t][i] : 0.f;    // threshold_backward on the output
        gen[act16_index(col, m)] = v;
        if (row0 + m < R) ws[a.W.denc + (size_t)(row0 + m) * H2 + col] = v;
      }
    }
  }
  __syncthreads();
  {  // ---- dH1 = dEnc W1 * [h1 > 0]
    f32x4 acc[4] = {{0}, {0}, {0}, {0}};
    const float4* const base = T4 + (a.W.w1t >> 2) + (size_t)(4 * wave) * (H2 / 16) * 64;
    const float4* const w[4] = {base, base + (H2 / 16) * 64, base + 2 * (H2 / 16) * 64, base + 3 * (H2 / 16) * 64};
    layer_tiles16<H2 / 16, 4>(reinterpret_cast<const float4*>(gen), w, lane, acc);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int col = 16 * (4 * wave + t) + c;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = 4 * h4 + i;
        if (row0 + m < R) ws[a.W.dh1 + (size_t)(row0 + m) * H1 + col] = hA[act16_index(col, m)] > 0.f ? acc[t][i] : 0.f;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Launch B.  Tiles: W0 16 x ceil(in / 16), W1 8 x 16, W_mu 8 x 8, W_lv 8 x 8, decoder 1 x 8 (n-tile x k-tile); the
// k-tile 0 of each layer also steps the layer's bias.
__host__ __device__ inline int weight_tiles(int in_dim) { return 16 * ((in_dim + 15) / 16) + 128 + 64 + 64 + 8; }

constexpr int RB_UNROLL = 8;
__global__ __launch_bounds__(THREADS) void fitd_weights_kernel(FitArgs a) {
  __shared__ float red[4 * 256];
  __shared__ float bred[4 * 64];
  __shared__ double dred[2 * THREADS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, h4 = lane >> 4;
  const WsL& W = a.W;
  const ParamL& Pl = a.P;
  const DiscLayout& L = a.L;
  const int kt0 = (a.in_dim + 15) / 16;
  int t = blockIdx.x, layer, nt, kt;
  if (t < 16 * kt0) {
    layer = 0, nt = t / kt0, kt = t % kt0;
  } else if ((t -= 16 * kt0) < 128) {
    layer = 1, nt = t / 16, kt = t % 16;
  } else if ((t -= 128) < 128) {
    layer = 2 + t / 64, nt = (t % 64) / 8, kt = t % 8;
  } else {
    layer = 4, nt = 0, kt = t - 128;
  }
  // delta [R][N] and activation [R][aw] (K columns used) of the layer
  const int N = layer == 0 ? H1 : layer == 1 ? H2 : layer == 4 ? 1 : ZD;
  const int aw = layer == 0 ? MAX_IN : layer == 1 ? H1 : layer == 4 ? ZD : H2;
  const int K = layer == 0 ? a.in_dim : aw, dw = N;
  const size_t dofs = layer == 0 ? W.dh1 : layer == 1 ? W.denc : layer == 2 ? W.dmu : layer == 3 ? W.dlv : W.dd;
  const size_t aofs = layer == 0 ? W.xs : layer == 1 ? W.h1 : layer == 4 ? W.z : W.h2;
  const float* dl = a.ws + dofs;
  const float* al = a.ws + aofs;
  const int n0 = 16 * nt, k0 = 16 * kt, R = a.R;
  const int n = n0 + c, k = k0 + c;
  // wave w: rows [w Q, min(R, (w + 1) Q)), Q a multiple of 4
  const int Q = (((R + 3) / 4) + 3) & ~3, rs = wave * Q, re = min(R, rs + Q);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;
  for (int r = rs; r < re; r += 4 * RB_UNROLL) {
    float dv[RB_UNROLL], av[RB_UNROLL];
#pragma unroll
    for (int u = 0; u < RB_UNROLL; ++u) {
      const int row = r + 4 * u + h4;
      dv[u] = (row < re && n < N) ? dl[(size_t)row * dw + n] : 0.f;
      av[u] = (row < re && k < K) ? al[(size_t)row * aw + k] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < RB_UNROLL; ++u) {
      // A[i = lane & 15][r = lane >> 4] = delta[row][n0 + i], B[r][j = lane & 15] = a[row][k0 + j]
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(dv[u], av[u], acc, 0, 0, 0);
      bsum += dv[u];
    }
  }
  // D[n = 4 (lane >> 4) + i][k = lane & 15]
#pragma unroll
  for (int i = 0; i < 4; ++i) red[wave * 256 + (4 * h4 + i) * 16 + c] = acc[i];
  bred[wave * 64 + lane] = bsum;
  __syncthreads();
  {
    const int nn = tid >> 4, kk = tid & 15, ne = n0 + nn, ke = k0 + kk;
    if (ne < N && ke < K) {
      const float g = ((red[tid] + red[256 + tid]) + red[512 + tid]) + red[768 + tid];
      switch (layer) {
        case 0: {
          const float p = adam1(a, Pl.w0 + (size_t)ne * a.in_dim + ke, g);
          a.packed[p32_index(L.w0, L.g1, ne, ke)] = p;
          a.packed[p16_index(L.w0n, G1N16, ne, ke)] = p;
          break;
        }
        case 1: {
          const float p = adam1(a, Pl.w1 + (size_t)ne * H1 + ke, g);
          a.packed[p32_index(L.w1, H1 / 8, ne, ke)] = p;
          a.packed[p16_index(L.w1n, H1 / 16, ne, ke)] = p;
          a.ws[W.w1t + pt_index(H2, ne, ke)] = p;
          break;
        }
        case 2:
        case 3: {
          const bool mu = layer == 2;
          const float p = adam1(a, (mu ? Pl.wmu : Pl.wlv) + (size_t)ne * H2 + ke, g);
          a.packed[p32_index(mu ? L.wmu : L.wlv, H2 / 8, ne, ke)] = p;
          a.packed[p16_index(mu ? L.wmun : L.wlvn, H2 / 16, ne, ke)] = p;
          a.ws[(mu ? W.wmut : W.wlvt) + pt_index(ZD, ne, ke)] = p;
          break;
        }
        default:
          a.packed[L.wd + ke] = adam1(a, Pl.wd + ke, g);
      }
    }
    if (kt == 0 && tid < 16 && n0 + tid < N) {   // the bias: the column sums of delta, lane groups then waves in order
      const float gb = oly_fit::bias_colsum(bred, tid);
      const size_t pb = layer == 0 ? Pl.b0 : layer == 1 ? Pl.b1 : layer == 2 ? Pl.bmu : layer == 3 ? Pl.blv : Pl.bd;
      const size_t kb = layer == 0 ? L.b0 : layer == 1 ? L.b1 : layer == 2 ? L.bmu : layer == 3 ? L.blv : L.bd;
      a.packed[kb + n0 + tid] = adam1(a, pb + n0 + tid, gb);
    }
  }
  if (blockIdx.x == 0) {   // ---- VDBLoss's value and beta's dual update; colstats += minibatch b
    oly_fit::loss_tree((R + 15) / 16, reinterpret_cast<const double*>(a.ws + W.lossp), dred);
    if (tid == 0) {
      const double bce = dred[0] / R, kl = dred[THREADS] / R;
      const float beta = a.beta[0];
      const float bottleneck = (float)kl - a.info_c;       // kld.mean() - I_c in float32
      float nb = beta + a.lr_beta * bottleneck;
      nb = nb > 0.f ? nb : 0.f;                            // max(0, .) : NaN gives 0 as Python's max does
      a.beta[0] = nb;
      if (a.loss_out) a.loss_out[0] = bce + (double)beta * (double)bottleneck;
      if (a.bce_out) a.bce_out[0] = bce;
      if (a.kl_out) a.kl_out[0] = kl;
      if (a.beta_out) a.beta_out[0] = nb;
    }
    oly_fit::colstats_add(a, R);
  } else if (blockIdx.x <= NSP && a.Rn > 0) {
    stats_slice(a, a.off_next, a.Rn, blockIdx.x - 1, dred);
  }
}

}  // namespace

extern "C" int64_t oly_disc_fit_ws_floats(int batch, int in_dim) {
  if (batch <= 0 || batch > MAX_BATCH || in_dim <= 0 || in_dim > MAX_IN) return -1;
  return (int64_t)ws_layout(batch).total;
}

extern "C" int64_t oly_disc_fit_pair_ws_floats(int batch, int ds, int d2, int standardise) {
  if (ds <= 0 || d2 <= 0 || ds > MAX_IN || d2 > MAX_IN || (standardise && d2 != ds)) return -1;
  return oly_disc_fit_ws_floats(batch, ds + d2);
}

extern "C" int oly_disc_fit_epoch(oly_ctx* ctx, const oly_disc_fit* f, const int32_t* perm, int n_rows, int batch,
                                  oly_stream stream) {
  return oly_disc_fit_epoch_pair(ctx, f, nullptr, perm, n_rows, batch, stream);
}

extern "C" int oly_disc_fit_epoch_pair(oly_ctx* ctx, const oly_disc_fit* f, const oly_disc_pair* pair, const int32_t* perm,
                                       int n_rows, int batch, oly_stream stream) {
  if (!ctx) return OLY_EINVAL;
  if (!f || !perm) OLY_FAIL(ctx, OLY_EINVAL, "oly_disc_fit_epoch: NULL argument");
  const char* const name = "oly_disc_fit_epoch";
  int rc = oly_fit::refuse_shape(ctx, name, pair, f->in_dim, oly_disc_fit_ws_floats(batch, f->in_dim) >= 0, OLY_ERANGE, MAX_BATCH,
                                 n_rows, batch, f->n_plcy);
  if (rc != OLY_OK) return rc;
  if (!f->x || !f->eps || !f->colstats || !f->param || !f->exp_avg || !f->exp_avg_sq || !f->packed || !f->beta || !f->ws)
    OLY_FAIL(ctx, OLY_EINVAL, "oly_disc_fit_epoch: NULL pointer in the argument block");
  const WsL W = ws_layout(batch);
  const int nb = (n_rows + batch - 1) / batch;
  rc = oly_fit::refuse_buffers(ctx, name, f->ws_floats, W.total, f->ws, f->packed, f->step, nb);
  if (rc != OLY_OK) return rc;
  if (nb == 0) return OLY_OK;
  const int in_dim = f->in_dim;
  FitArgs a{};
  oly_fit::set_pair_cols(a, in_dim, pair);
  a.n_rows = n_rows;
  a.n_plcy = f->n_plcy;
  a.perm = perm;
  a.x = f->x;
  a.targets = f->targets;
  a.eps = f->eps;
  a.colstats = f->colstats;
  a.param = f->param;
  a.m = f->exp_avg;
  a.v = f->exp_avg_sq;
  a.packed = f->packed;
  a.ws = f->ws;
  a.beta = f->beta;
  a.info_c = f->info_constraint;
  a.lr_beta = f->lr_beta;
  a.wd = f->weight_decay;
  a.L = disc_layout(in_dim);
  a.P = param_layout(in_dim);
  a.W = W;
  const float* p = f->param;
  const ParamL& P = a.P;
  rc = oly_disc_pack(ctx, in_dim, H1, H2, ZD, p + P.w0, p + P.b0, p + P.w1, p + P.b1, p + P.wmu, p + P.bmu,
                         p + P.wlv, p + P.blv, p + P.wd, p + P.bd, f->packed, stream);
  if (rc != OLY_OK) return rc;
  const unsigned bit = in_dim <= 32 ? 1u : 2u;
  if (!(ctx->discfit_attr_done & bit)) {
    OLY_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(in_dim <= 32 ? fitd_rows_kernel<2> : fitd_rows_kernel<4>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)ROWS_LDS));
    ctx->discfit_attr_done |= bit;
  }
  oly_fit::set_minibatch(a, 0, nb, n_rows, batch);
  hipLaunchKernelGGL(fitd_prologue_kernel, dim3(PRO_BLOCKS), dim3(THREADS), 0, oly_s(stream), a);
  for (int b = 0; b < nb; ++b) {
    oly_fit::set_minibatch(a, b, nb, n_rows, batch);
    a.ad = oly_fit::adam_scalars(f->beta1, f->beta2, f->adam_eps, f->lr, (long)f->step + b + 1);
    a.loss_out = f->loss_out ? f->loss_out + b : nullptr;
    a.bce_out = f->bce_out ? f->bce_out + b : nullptr;
    a.kl_out = f->kl_out ? f->kl_out + b : nullptr;
    a.beta_out = f->beta_out ? f->beta_out + b : nullptr;
    const dim3 grid_a((unsigned)((a.R + 15) / 16));
    if (in_dim <= 32) hipLaunchKernelGGL(fitd_rows_kernel<2>, grid_a, dim3(THREADS), ROWS_LDS, oly_s(stream), a);
    else hipLaunchKernelGGL(fitd_rows_kernel<4>, grid_a, dim3(THREADS), ROWS_LDS, oly_s(stream), a);
    hipLaunchKernelGGL(fitd_weights_kernel, dim3(weight_tiles(in_dim)), dim3(THREADS), 0, oly_s(stream), a);
  }
  OLY_LAUNCH_CHECK(ctx, "disc fit kernels");
  return OLY_OK;
}
