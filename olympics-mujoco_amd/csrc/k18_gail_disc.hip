// K18: GAIL's discriminator (create_gail_agent, examples/imitation_learning/utils.py:79-97):
// DiscriminatorNetwork(masked obs -> [512, 256] -> 1, tanh / tanh / identity) (imitation_lib/utils/networks.py:194-225)
// on its own Standardizer, trained by Adam over GailDiscriminatorLoss (imitation_lib/utils/math.py:11-36).
//
//   oly_gail_disc_forward    make_discrim_reward (imitation_lib/imitation/gail_TRPO.py:320-327) in ONE launch: K16's
//                            forward kernel (ilmlp_common.h) instantiated with tanh32 hidden layers, the state mask
//                            (prepare_discrim_inputs, gail_TRPO.py:297-313) applied while the rows are staged, the
//                            reward formula (reward_of, disc_common.h) on the logit.
//   oly_gail_reward_step     the Standardizer's update with the masked rows (networks.py:68-81), then that forward.
//   oly_gail_disc_fit_epoch  one epoch of _fit_discriminator's minibatch loop (gail_TRPO.py:167-220, states only).
//   oly_gail_*_pair          the same three on a paired input (oly_disc_pair: (s, s') with use_next_states, (s, a) with
//                            actions; DiscriminatorNetwork.preprocess_inputs, networks.py:216-234).  A row is staged from
//                            two sources; the states' half is standardised with the statistics after the states went in,
//                            the next states' half with those after the next states went in as well (two updates per
//                            forward, networks.py:224-227), actions raw.  The states-only entry points are the paired
//                            ones with no second part.
//
// The fit, per call: oly_ilmlp_pack (the stream from param), gfit_prologue_kernel (the transposed W2 stream of the
// backward, the statistics partials of minibatch 0), then per minibatch b
//   A  gfit_rows_kernel     one 16-row tile per workgroup (8 waves): gather perm rows, standardise with the
//                           statistics that include minibatch b, the forward on the f32 matrix cores (v_mfma_f32_16x16x4_f32) in the forward
//                           kernel's chain order with tanh32, the per-row loss terms, dd, dZ2 = dd w3 (1 - h2^2),
//                           dH1 = dZ2 W2 (matrix cores, transposed stream), dZ1 = dH1 (1 - h1^2).  Activations and
//                           deltas go to the workspace in row quads ([row / 4][column][row % 4]: the accumulator's four
//                           rows are one 16-byte store, and one 16-byte load in launch B); loss partials to fixed slots.
//   B  gfit_weights_kernel  one 16 x 16 weight tile per workgroup: dW = sum over the minibatch's rows of delta^T a
//                           (4 waves x a quarter of the 16-row steps each, added in wave order; 16-byte loads of four
//                           rows per lane, four steps of loads in flight), weight decay, Adam, the stepped values into
//                           param, the moments, the packed stream and the transposed stream.  Workgroup 0 adds the loss
//                           partials and writes the per-minibatch outputs and colstats += minibatch b; workgroups
//                           1 .. 16 sum minibatch b+1's rows into the statistics partials launch A of b+1 reads.
// Every reduction has a fixed order and there are no atomics: two runs give identical bits.  What the fit shares with
// K15 and K16 (Adam, the statistics fold, the weights kernel's tail, the epoch driver's host side) is in fit_common.h;
// what the two launches share with K24 and K26 (the Standardizer's head, the activation and its gradient, the row-quad
// stores, dZ1, the W2T build, the tile count, the rows kernel's dispatch) is in ilmlp_fit.h, taken here with Tanh.
#include <cstdlib>

#include "disc_common.h"
#include "ilmlp_fit.h"
#include "oly_common.h"

namespace {
using namespace oly_ilfit;
using oly_fit::adam1;
using oly_fit::row_at;
using oly_fit::stats_slice;
static_assert(IN_MAX == oly_fit::MAX_IN, "fit_common.h's statistics arrays have this file's pitch");

constexpr int MAX_BATCH = 4096;

// workspace (floats), BP = batch rounded up to 16 rows; [BP][W] arrays in row quads, element (row, col) at
// ((row / 4) W + col) 4 + row % 4:
//   xs [BP][64] standardised rows | h1 [BP][512] | h2 [BP][256] | dZ1 [BP][512] | dZ2 [BP][256] | dd [BP] |
//   loss partials [BP / 16][2] f64 | statistics partials [NSP][2][64] f64 | the minibatch's column sums [2][64] f64 |
//   the transposed stream W2T
struct WsL {
  size_t xs, h1, h2, dz1, dz2, dd, lossp, statp, delta, w2t, total;
};
__host__ __device__ inline WsL ws_layout(int batch) {
  const size_t BP = (size_t)(batch + 15) / 16 * 16;
  WsL W;
  W.xs = 0;
  W.h1 = W.xs + BP * IN_MAX;
  W.h2 = W.h1 + BP * H1;
  W.dz1 = W.h2 + BP * H2;
  W.dz2 = W.dz1 + BP * H1;
  W.dd = W.dz2 + BP * H2;
  W.lossp = W.dd + BP;
  W.statp = W.lossp + BP / 16 * 4;
  W.delta = W.statp + (size_t)NSP * 2 * IN_MAX * 2;
  W.w2t = W.delta + 2 * IN_MAX * 2;
  W.total = W.w2t + (size_t)H2 * H1;
  return W;
}

// W2T is the B operand of the data gradient dH1 = dZ2 W2 (pt_index, fit_common.h; N = 256 outputs)
struct FitArgs {
  int in_dim, n_rows, n_plcy;
  int ds, d2, std2, stride2; // x [n_rows, ds] | x2 [n_rows, stride2]'s first d2 columns (d2 = in_dim - ds, 0: none);
  const float* x2;           // std2: x2 goes through the Standardizer (next states), else raw (actions)
  int R, Rn;                 // rows of minibatch b / b+1 (0: none)
  long off, off_next;        // first position of minibatch b / b+1 in perm
  const int32_t* perm;
  const float *x, *targets;
  double* colstats;
  float *param, *m, *v, *packed, *ws;
  float entcoeff;
  oly_fit::AdamK ad;
  float wd;                  // weight_decay
  double *loss_out, *bce_out, *ent_out;   // + b, or NULL
  ParamLayout P;
  WsL W;
};

// grid PRO_BLOCKS: the transposed stream from param (grid-stride) and, workgroups 0 .. NSP-1, minibatch 0's partials
__global__ __launch_bounds__(THREADS) void gfit_prologue_kernel(FitArgs a) {
  __shared__ double part[8 * IN_MAX];
  build_w2t(a);
  if (blockIdx.x < NSP) stats_slice(a, a.off, a.R, blockIdx.x, part);
}

// ---------------------------------------------------------------------------------------------------------------
// Launch A.  RTHREADS = 512 threads = 8 waves, two per SIMD: at 2048 rows the 128 workgroups leave every CU at most one, so a
// second wave per SIMD is what covers the other's weight loads and tanh32.  The forward kernel's chains: layer 1 wave w ->
// column tiles 4w .. 4w+3, layer 2 -> 2w, 2w+1, the logit by wave 0 as one chain over k < 256 (column 0 of W3's first
// tile).  Backward: dZ2 (wave w -> tiles 2w, 2w+1) and dH1 (wave w -> tiles 4w .. 4w+3, the chain over the 256 layer-2
// units).
constexpr size_t ROWS_LDS_FLOATS = (size_t)(IN_MAX + H1 + 2 * H2) * 16 + H2 + 16;
constexpr size_t ROWS_LDS = sizeof(float) * ROWS_LDS_FLOATS + sizeof(double) * (2 * IN_MAX + 2 * 16);
static_assert(ROWS_LDS_FLOATS % 4 == 0, "the fp64 arrays must be 8-byte aligned");

// waves_per_eu(7, 8) holds the allocator to the register budget of seven waves per SIMD (72 VGPRs), which both
// instantiations fit without a spill.  Left to itself it gives both 74 with the two-source staging (six waves in the
// compiler's report; the 32-column instantiation had 72 before).  A 512-thread workgroup with this kernel's LDS never has
// seven waves resident on a SIMD, so the attribute bounds registers and nothing else.
template <int G1>
__global__ __launch_bounds__(RTHREADS) __attribute__((amdgpu_waves_per_eu(7, 8))) void gfit_rows_kernel(FitArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xT = lds;                       // [64 x 16]   standardised input (act16 images, mlp_tiles.h)
  float* hA = xT + IN_MAX * 16;          // [512 x 16]  h1
  float* hB = hA + H1 * 16;              // [256 x 16]  h2
  float* gz = hB + H2 * 16;              // [256 x 16]  dZ2
  float* w3 = gz + H2 * 16;              // [256]       the output row
  float* dds = w3 + H2;                  // [16]        dd by row
  double* st = reinterpret_cast<double*>(lds + ROWS_LDS_FLOATS);   // [2][IN_MAX] mean, std
  double* red = st + 2 * IN_MAX;         // [2][16] bce, entropy by row
  __shared__ int rows_x[16];             // the tile's data rows (-1 beyond the minibatch)
  const ParamLayout& PL = a.P;
  const float* P = a.packed;
  const float4* P4 = reinterpret_cast<const float4*>(P);
  const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, h4 = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row0 = blockIdx.x * 16, R = a.R, in_dim = a.in_dim;
  float* ws = a.ws;
  float4* ws4 = reinterpret_cast<float4*>(ws);
  const size_t quad = (size_t)(row0 >> 2) + h4;      // this lane's accumulator rows: 4 h4 + i = one row quad

  if (tid < in_dim) {   // Standardizer.update_mean_std with the minibatch's rows (networks.py:76-81), as K15
    const double* sp = reinterpret_cast<const double*>(ws + a.W.statp);
    const int ds = a.ds;
    double s, ss;
    slice_sums(sp, tid, s, ss);
    double mean = 0.0, sd = 1.0;        // an action column passes through: f32((f64(a) - 0) / 1) is a
    if (tid < ds) {
      col_moments(a.colstats[tid] + (double)R, a.colstats[ds + tid] + s, a.colstats[2 * ds + tid] + ss, mean, sd);
    } else if (a.std2) {
      // a next-state column: the Standardizer has taken the minibatch's states in, then its next states
      // (preprocess_inputs, networks.py:224-227), so column j's statistics hold both sets of sums
      const int j = tid - ds;
      double s1, ss1;
      slice_sums(sp, j, s1, ss1);
      col_moments(a.colstats[j] + (double)R + (double)R, (a.colstats[ds + j] + s1) + s, (a.colstats[2 * ds + j] + ss1) + ss,
                  mean, sd);
    }
    st[tid] = mean;
    st[IN_MAX + tid] = sd;
    if (blockIdx.x == 0) {
      double* d = reinterpret_cast<double*>(ws + a.W.delta);
      d[tid] = s;
      d[IN_MAX + tid] = ss;
    }
  }
  if (tid < H2) w3[tid] = a.param[PL.w3 + tid];
  if (tid < 16) rows_x[tid] = row0 + tid < R ? row_at(a, a.off + row0 + tid) : -1;
  __syncthreads();
  for (int e = tid; e < 16 * IN_MAX; e += RTHREADS) {
    const int m = e / IN_MAX, k = e & (IN_MAX - 1), row = rows_x[m];
    float v = 0.f;
    // f32((f64(x) - mean) / std): the reference subtracts fp64 statistics and narrows afterwards (networks.py:68-74)
    if (row >= 0 && k < in_dim) {
      const float* src = k < a.ds ? a.x + ((size_t)row * a.ds + k) : a.x2 + ((size_t)row * a.stride2 + (k - a.ds));
      v = (float)(((double)*src - st[k]) / st[IN_MAX + k]);
    }
    xT[act16_index(k, m)] = v;
    ws[a.W.xs + ((size_t)((row0 + m) >> 2) * IN_MAX + k) * 4 + (m & 3)] = v;
  }
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
      h.x = Tanh::f(acc[0][t][0] + bv);
      h.y = Tanh::f(acc[0][t][1] + bv);
      h.z = Tanh::f(acc[0][t][2] + bv);
      h.w = Tanh::f(acc[0][t][3] + bv);
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
      h.x = Tanh::f(acc[0][t][0] + bv);
      h.y = Tanh::f(acc[0][t][1] + bv);
      h.z = Tanh::f(acc[0][t][2] + bv);
      h.w = Tanh::f(acc[0][t][3] + bv);
      hB[act16_index(col, 4 * h4)] = h.x;
      hB[act16_index(col, 4 * h4 + 1)] = h.y;
      hB[act16_index(col, 4 * h4 + 2)] = h.z;
      hB[act16_index(col, 4 * h4 + 3)] = h.w;
      h2r[t] = h;
      ws4[(a.W.h2 >> 2) + quad * H2 + col] = h;
    }
  }
  __syncthreads();
  const float invR = 1.0f / (float)R;
  if (wave == 0) {  // ---- the logit (one chain over k < 256, as the forward kernel), GailDiscriminatorLoss's terms and dd
    f32x4 acc[1][1] = {{f32x4{0.f, 0.f, 0.f, 0.f}}};
    const float4* a4[1] = {reinterpret_cast<const float4*>(hB)};
    tiles<H2 / 16, 1, 1>(a4, P4 + P_W3 / 4, 0, lane, acc);
    if (c == 0) {
      const float bv = P[P_B3];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = 4 * h4 + i, row = rows_x[m];
        double bce = 0.0, ent = 0.0;
        float dd = 0.f;
        if (row >= 0) {
          const float d = acc[0][0][i] + bv;
          const float t = a.targets ? a.targets[row] : (row < a.n_plcy ? 0.f : 1.f);
          const double dv = d, sp = log1p(exp(-fabs(dv))), sig = 1.0 / (1.0 + exp(-dv));
          bce = fmax(dv, 0.0) - dv * (double)t + sp;                  // math.py:25
          ent = (1.0 - sig) * dv + (fmax(-dv, 0.0) + sp);             // math.py:36: (1 - sigmoid) x - logsigmoid(x)
          dd = (float)(sig - (double)t + (double)a.entcoeff * sig * (1.0 - sig) * dv) * invR;
        }
        red[m] = bce;
        red[16 + m] = ent;
        dds[m] = dd;
        ws[a.W.dd + row0 + m] = dd;
      }
    }
  }
  __syncthreads();
  if (tid == 0) {       // this tile's loss partials, rows in order
    double b = 0.0, e = 0.0;
    for (int r = 0; r < 16; ++r) {
      b += red[r];
      e += red[16 + r];
    }
    double* lp = reinterpret_cast<double*>(ws + a.W.lossp) + 2 * blockIdx.x;
    lp[0] = b;
    lp[1] = e;
  }
  {  // ---- dZ2 = dd w3 (1 - h2^2)  (tanh backward from the stored output)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int col = 16 * (2 * wave + t) + c;
      const float wc = w3[col];
      float4 g;
      g.x = Tanh::back(dds[4 * h4] * wc, h2r[t].x);
      g.y = Tanh::back(dds[4 * h4 + 1] * wc, h2r[t].y);
      g.z = Tanh::back(dds[4 * h4 + 2] * wc, h2r[t].z);
      g.w = Tanh::back(dds[4 * h4 + 3] * wc, h2r[t].w);
      put_quad(gz, col, h4, g);
      ws4[(a.W.dz2 >> 2) + quad * H2 + col] = g;
    }
  }
  __syncthreads();
  // ---- dZ1 = (dZ2 W2) (1 - h1^2)
  dz1_tiles<Tanh>(gz, reinterpret_cast<const float4*>(ws) + (a.W.w2t >> 2),
                  [&](int col) { return get_quad(hA, col, h4); }, ws4, a.W.dz1, quad);
}

// ---------------------------------------------------------------------------------------------------------------
// Launch B (the tiles: weight_tiles, ilmlp_fit.h; W3 is 1 x 16).  The dW chain and the waves' meeting are spelt out here,
// not taken from ilmlp_fit.h as in K24 and K26: with the shared functions this kernel ran 1 to 3 % longer at 2048 rows.
__global__ __launch_bounds__(THREADS) void gfit_weights_kernel(FitArgs a) {
  __shared__ float red[4 * 256];
  __shared__ float bred[4 * 64];
  __shared__ double dred[2 * THREADS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, h4 = lane >> 4;
  const WsL& W = a.W;
  const ParamLayout& PL = a.P;
  const int kt0 = (a.in_dim + 15) / 16;
  int t = blockIdx.x, layer, nt, kt;
  if (t < 32 * kt0) {
    layer = 0, nt = t / kt0, kt = t % kt0;
  } else if ((t -= 32 * kt0) < 512) {
    layer = 1, nt = t / 32, kt = t % 32;
  } else {
    layer = 2, nt = 0, kt = t - 512;
  }
  // delta [R][N] and activation [R][aw] (K columns used) of the layer, both in row quads
  const int N = layer == 0 ? H1 : layer == 1 ? H2 : 1;
  const int aw = layer == 0 ? IN_MAX : layer == 1 ? H1 : H2;
  const int K = layer == 0 ? a.in_dim : aw;
  const float4* dl = reinterpret_cast<const float4*>(a.ws + (layer == 0 ? W.dz1 : layer == 1 ? W.dz2 : W.dd));
  const float4* al = reinterpret_cast<const float4*>(a.ws + (layer == 0 ? W.xs : layer == 1 ? W.h1 : W.h2));
  const int n0 = 16 * nt, k0 = 16 * kt, R = a.R;
  const bool n_ok = n0 + c < N, k_ok = k0 + c < K;
  // a step = the 16 rows of one tile of launch A (which wrote all 16: zeros in the deltas beyond the minibatch); lane
  // group h4 takes the step's row quad h4.  Wave w: steps [w Q, min(steps, (w + 1) Q))
  const int steps = (R + 15) / 16, Q = (steps + 3) / 4, s0 = wave * Q, s1 = min(steps, s0 + Q);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int s = s0; s < s1; s += STEP_UNROLL) {
    float4 dv[STEP_UNROLL], av[STEP_UNROLL];
#pragma unroll
    for (int u = 0; u < STEP_UNROLL; ++u) {
      const size_t q = (size_t)4 * (s + u) + h4;
      const bool in = s + u < s1;
      dv[u] = (in && n_ok) ? dl[q * N + n0 + c] : zero4;
      av[u] = (in && k_ok) ? al[q * aw + k0 + c] : zero4;
    }
#pragma unroll
    for (int u = 0; u < STEP_UNROLL; ++u) {
      // A[i = lane & 15][r = lane >> 4] = delta[row 4 q + j][n0 + i], B[r][j = lane & 15] = a[row 4 q + j][k0 + j]
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(dv[u].x, av[u].x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(dv[u].y, av[u].y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(dv[u].z, av[u].z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(dv[u].w, av[u].w, acc, 0, 0, 0);
      bsum += ((dv[u].x + dv[u].y) + dv[u].z) + dv[u].w;
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
      if (layer == 0) {
        a.packed[pk_index(P_W1, IN_MAX / 16, ne, ke)] = adam1(a, PL.w1 + (size_t)ne * a.in_dim + ke, g);
      } else if (layer == 1) {
        const float p = adam1(a, PL.w2 + (size_t)ne * H1 + ke, g);
        a.packed[pk_index(P_W2, H1 / 16, ne, ke)] = p;
        a.ws[W.w2t + pt_index(H2, ne, ke)] = p;
      } else {
        a.packed[pk_index(P_W3, H2 / 16, 0, ke)] = adam1(a, PL.w3 + ke, g);
      }
    }
    if (kt == 0 && tid < 16 && n0 + tid < N) {   // the bias: the column sums of delta, lane groups then waves in order
      const float gb = oly_fit::bias_colsum(bred, tid);
      const size_t pb = layer == 0 ? PL.b1 : layer == 1 ? PL.b2 : PL.b3;
      const size_t kb = layer == 0 ? P_B1 : layer == 1 ? P_B2 : P_B3;
      a.packed[kb + n0 + tid] = adam1(a, pb + n0 + tid, gb);
    }
  }
  if (blockIdx.x == 0) {   // ---- GailDiscriminatorLoss's value; colstats += minibatch b
    oly_fit::loss_tree((R + 15) / 16, reinterpret_cast<const double*>(a.ws + W.lossp), dred);
    if (tid == 0) {
      const double bce = dred[0] / R, ent = dred[THREADS] / R;
      if (a.loss_out) a.loss_out[0] = bce - (double)a.entcoeff * ent;      // math.py:28-29
      if (a.bce_out) a.bce_out[0] = bce;
      if (a.ent_out) a.ent_out[0] = ent;
    }
    oly_fit::colstats_add(a, R);
  } else if (blockIdx.x <= NSP && a.Rn > 0) {
    stats_slice(a, a.off_next, a.Rn, blockIdx.x - 1, dred);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// The Standardizer's running sums over the masked columns of x [B, Dx]: STAT_BLOCKS row ranges, in each four
// row-strided chains added in order, the ranges added in order by the finishing workgroup.
constexpr int STAT_BLOCKS = 256;
__global__ __launch_bounds__(THREADS) void gail_stats_partial_kernel(long B, int Dx, int D, const float* __restrict__ x,
                                                                     const int* __restrict__ mask, double* __restrict__ part_out) {
  __shared__ double part[8 * IN_MAX];
  const int tid = threadIdx.x, k = tid & (IN_MAX - 1), grp = tid >> 6;
  const long per = (B + STAT_BLOCKS - 1) / STAT_BLOCKS, r0 = blockIdx.x * per, r1 = min(B, r0 + per);
  double sum = 0.0, ss = 0.0;
  if (k < D) {
    const int col = mask ? mask[k] : k;
    for (long r = r0 + grp; r < r1; r += 4) {
      const double v = x[r * Dx + col];
      sum += v;
      ss += v * v;
    }
  }
  oly_fit::fold_chains(sum, ss, D, part, part_out + (size_t)blockIdx.x * 2 * IN_MAX);
}

__global__ __launch_bounds__(64) void gail_stats_finish_kernel(long B, int D, const double* __restrict__ part,
                                                               double* __restrict__ colstats, int accumulate,
                                                               double* __restrict__ copy_out) {
  const int k = threadIdx.x;
  if (k >= D) return;
  double s = 0.0, ss = 0.0;
  for (int b = 0; b < STAT_BLOCKS; ++b) {
    s += part[(size_t)b * 2 * IN_MAX + k];
    ss += part[(size_t)b * 2 * IN_MAX + IN_MAX + k];
  }
  if (accumulate) {
    colstats[k] += (double)B; colstats[D + k] += s; colstats[2 * D + k] += ss;
  } else {
    colstats[k] = (double)B; colstats[D + k] = s; colstats[2 * D + k] = ss;
  }
  if (copy_out) {      // the statistics as they stand now, for a forward that runs after a later update
    copy_out[k] = colstats[k]; copy_out[D + k] = colstats[D + k]; copy_out[2 * D + k] = colstats[2 * D + k];
  }
}
static_assert(sizeof(double) * STAT_BLOCKS * 2 * IN_MAX <= sizeof(double) * OLY_STATS_MAX_BLOCKS * 2 * OLY_MAX_OBS,
              "the partials fit ctx->stats_ws");

template <int RS>
int launch_forward(oly_ctx* ctx, const FwdArgs& a, oly_stream stream) {
  const unsigned bit = 1u << (4 * (RS - 1) + (a.in_dim + 15) / 16);
  const dim3 grid((unsigned)((a.N + 16 * RS - 1) / (16 * RS)));
  const size_t lds = fwd_lds<RS>();
  switch ((a.in_dim + 15) / 16) {
#define OLY_GAIL_CASE(G)                                                                                              \
  case G:                                                                                                             \
    if (!(ctx->gail_attr_done & bit)) {                                                                               \
      OLY_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(ilmlp_forward_kernel<RS, G, true>),              \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                        \
      ctx->gail_attr_done |= bit;                                                                                     \
    }                                                                                                                 \
    hipLaunchKernelGGL((ilmlp_forward_kernel<RS, G, true>), grid, dim3(FWD_THREADS), lds, oly_s(stream), a);          \
    break;
    OLY_GAIL_CASE(1)
    OLY_GAIL_CASE(2)
    OLY_GAIL_CASE(3)
    OLY_GAIL_CASE(4)
#undef OLY_GAIL_CASE
  }
  OLY_LAUNCH_CHECK(ctx, "gail discriminator forward");
  return OLY_OK;
}

}  // namespace

int oly_masked_col_stats(oly_ctx* ctx, long B, int Dx, int D, const float* x, const int32_t* mask, double* colstats,
                         int accumulate, double* copy_out, oly_stream stream) {
  hipLaunchKernelGGL(gail_stats_partial_kernel, dim3(STAT_BLOCKS), dim3(THREADS), 0, oly_s(stream), B, Dx, D, x, mask,
                     ctx->stats_ws);
  hipLaunchKernelGGL(gail_stats_finish_kernel, dim3(1), dim3(64), 0, oly_s(stream), B, D, ctx->stats_ws, colstats,
                     accumulate, copy_out);
  OLY_LAUNCH_CHECK(ctx, "gail statistics kernels");
  return OLY_OK;
}

extern "C" int oly_gail_disc_forward_pair(oly_ctx* ctx, int64_t B, int Dx, int Ds, const float* x, const int32_t* mask,
                                          const oly_disc_pair* pair, const double* stats_a, const double* stats_b,
                                          const float* packed, float* reward, float* logits, oly_stream stream) {
  if (!ctx) return OLY_EINVAL;
  if (B < 0 || B > 0x7fffffffL || Dx <= 0 || Ds <= 0 || Ds > IN_MAX || (!mask && Ds != Dx))
    OLY_FAIL(ctx, OLY_EINVAL, "oly_gail_disc_forward_pair: bad shape (B %ld, Dx %d, Ds %d; Ds <= %d)", (long)B, Dx, Ds, IN_MAX);
  if (pair) {
    const char* why = oly_disc::pair_error(pair, Ds);
    if (why) OLY_FAIL(ctx, OLY_EINVAL, "oly_gail_disc_forward_pair: %s (Ds %d, d2 %d)", why, Ds, pair->d2);
    if (pair->standardise && (stats_a == nullptr) != (stats_b == nullptr))
      OLY_FAIL(ctx, OLY_EINVAL, "oly_gail_disc_forward_pair: a standardised second part takes both stats_a and stats_b, or neither");
  }
  if (!x || !packed || (!reward && !logits)) OLY_FAIL(ctx, OLY_EINVAL, "oly_gail_disc_forward_pair: NULL input or no output");
  if ((reinterpret_cast<uintptr_t>(packed) & 15) != 0)
    OLY_FAIL(ctx, OLY_EINVAL, "oly_gail_disc_forward_pair: packed must be 16-byte aligned");
  if (B == 0) return OLY_OK;
  FwdArgs a{(long)B, Ds, 1, OLY_ACT_IDENTITY, Dx, x, mask, nullptr, nullptr, stats_a, packed, logits, reward};
  if (pair) {
    a.in_dim = Ds + pair->d2;
    a.d2 = pair->d2;
    a.std2 = pair->standardise != 0;
    a.stride2 = pair->stride2;
    a.x2 = pair->x2;
    a.mask2 = pair->mask2;
    a.colstats2 = stats_b;
  }
  // 16-row tiles while the 32-row tiles would leave CUs without a second workgroup (as K16)
  const long slots = 2L * (ctx->num_cu > 0 ? ctx->num_cu : 256);
  if ((B + 31) / 32 < slots) return launch_forward<1>(ctx, a, stream);
  return launch_forward<2>(ctx, a, stream);
}

extern "C" int oly_gail_disc_forward(oly_ctx* ctx, int64_t B, int Dx, int D, const float* x, const int32_t* mask,
                                     const double* mean, const double* sd, const double* colstats, const float* packed,
                                     float* reward, float* logits, oly_stream stream) {
  if (!ctx) return OLY_EINVAL;
  if (B < 0 || B > 0x7fffffffL || Dx <= 0 || D <= 0 || D > IN_MAX || (!mask && D != Dx) || (mean == nullptr) != (sd == nullptr) ||
      (mean && colstats))
    OLY_FAIL(ctx, OLY_EINVAL, "oly_gail_disc_forward: bad shape (B %ld, Dx %d, D %d; D <= %d), only one of mean / std, or both mean / std and colstats given",
             (long)B, Dx, D, IN_MAX);
  if (!x || !packed || (!reward && !logits)) OLY_FAIL(ctx, OLY_EINVAL, "oly_gail_disc_forward: NULL input or no output");
  if ((reinterpret_cast<uintptr_t>(packed) & 15) != 0) OLY_FAIL(ctx, OLY_EINVAL, "oly_gail_disc_forward: packed must be 16-byte aligned");
  if (B == 0) return OLY_OK;
  if (!mean) return oly_gail_disc_forward_pair(ctx, B, Dx, D, x, mask, nullptr, colstats, nullptr, packed, reward, logits, stream);
  const FwdArgs a{(long)B, D, 1, OLY_ACT_IDENTITY, Dx, x, mask, mean, sd, colstats, packed, logits, reward};
  // 16-row tiles while the 32-row tiles would leave CUs without a second workgroup (as K16)
  const long slots = 2L * (ctx->num_cu > 0 ? ctx->num_cu : 256);
  if ((B + 31) / 32 < slots) return launch_forward<1>(ctx, a, stream);
  return launch_forward<2>(ctx, a, stream);
}

extern "C" int oly_gail_reward_step_pair(oly_ctx* ctx, int64_t B, int Dx, int Ds, const float* x, const int32_t* mask,
                                         const oly_disc_pair* pair, double* colstats, double* stats_a, int accumulate,
                                         const float* const* weights, float* packed, float* reward, float* logits,
                                         oly_stream stream) {
  if (!ctx) return OLY_EINVAL;
  if (B < 0 || B > 0x7fffffffL || Dx <= 0 || Ds <= 0 || Ds > IN_MAX || (!mask && Ds != Dx))
    OLY_FAIL(ctx, OLY_EINVAL, "oly_gail_reward_step_pair: bad shape (B %ld, Dx %d, Ds %d; Ds <= %d)", (long)B, Dx, Ds, IN_MAX);
  if (pair) {
    const char* why = oly_disc::pair_error(pair, Ds);
    if (why) OLY_FAIL(ctx, OLY_EINVAL, "oly_gail_reward_step_pair: %s (Ds %d, d2 %d)", why, Ds, pair->d2);
    if (pair->standardise && !stats_a)
      OLY_FAIL(ctx, OLY_EINVAL, "oly_gail_reward_step_pair: stats_a (the scratch block [3, Ds]) is NULL for a standardised second part");
    if (pair->standardise && stats_a == colstats)
      OLY_FAIL(ctx, OLY_EINVAL, "oly_gail_reward_step_pair: stats_a must not be colstats (S1 is kept apart from the running sums)");
  }
  if (!x || !colstats || !packed || (!reward && !logits))
    OLY_FAIL(ctx, OLY_EINVAL, "oly_gail_reward_step_pair: NULL x / colstats / packed, or no output");
  if ((reinterpret_cast<uintptr_t>(packed) & 15) != 0)
    OLY_FAIL(ctx, OLY_EINVAL, "oly_gail_reward_step_pair: packed must be 16-byte aligned");
  const int D = Ds + (pair ? pair->d2 : 0);
  if (weights) {
    for (int i = 0; i < 6; ++i)
      if (!weights[i]) OLY_FAIL(ctx, OLY_EINVAL, "oly_gail_reward_step_pair: NULL weight pointer");
    const int rc = oly_ilmlp_pack(ctx, D, H1, H2, 1, weights[0], weights[1], weights[2], weights[3], weights[4], weights[5],
                                  packed, stream);
    if (rc != OLY_OK) return rc;
  }
  const bool two = pair && pair->standardise;
  // _stand(states): the running sums take the states in; S1 is what the states' half is standardised with
  int rc = oly_masked_col_stats(ctx, (long)B, Dx, Ds, x, mask, colstats, accumulate, two ? stats_a : nullptr, stream);
  if (rc != OLY_OK) return rc;
  if (two) {  // _stand(next_states): a second update, S2 = S1 + the next states (networks.py:226-227)
    rc = oly_masked_col_stats(ctx, (long)B, pair->stride2, Ds, pair->x2, pair->mask2, colstats, 1, nullptr, stream);
    if (rc != OLY_OK) return rc;
  }
  return oly_gail_disc_forward_pair(ctx, B, Dx, Ds, x, mask, pair, two ? stats_a : colstats, colstats, packed, reward, logits,
                                    stream);
}

extern "C" int oly_gail_reward_step(oly_ctx* ctx, int64_t B, int Dx, int D, const float* x, const int32_t* mask,
                                    double* colstats, int accumulate, const float* const* weights, float* packed,
                                    float* reward, float* logits, oly_stream stream) {
  if (!ctx) return OLY_EINVAL;
  if (B < 0 || B > 0x7fffffffL || Dx <= 0 || D <= 0 || D > IN_MAX || (!mask && D != Dx))
    OLY_FAIL(ctx, OLY_EINVAL, "oly_gail_reward_step: bad shape (B %ld, Dx %d, D %d; D <= %d)", (long)B, Dx, D, IN_MAX);
  if (!x || !colstats || !packed || (!reward && !logits))
    OLY_FAIL(ctx, OLY_EINVAL, "oly_gail_reward_step: NULL x / colstats / packed, or no output");
  if ((reinterpret_cast<uintptr_t>(packed) & 15) != 0) OLY_FAIL(ctx, OLY_EINVAL, "oly_gail_reward_step: packed must be 16-byte aligned");
  if (weights)
    for (int i = 0; i < 6; ++i)
      if (!weights[i]) OLY_FAIL(ctx, OLY_EINVAL, "oly_gail_reward_step: NULL weight pointer");
  return oly_gail_reward_step_pair(ctx, B, Dx, D, x, mask, nullptr, colstats, nullptr, accumulate, weights, packed, reward,
                                   logits, stream);
}

extern "C" int64_t oly_gail_disc_fit_ws_floats(int batch, int in_dim) {
  if (batch <= 0 || batch > MAX_BATCH || in_dim <= 0 || in_dim > IN_MAX) return -1;
  return (int64_t)ws_layout(batch).total;
}

extern "C" int64_t oly_gail_disc_fit_pair_ws_floats(int batch, int ds, int d2, int standardise) {
  if (ds <= 0 || d2 <= 0 || ds > IN_MAX || d2 > IN_MAX || (standardise && d2 != ds)) return -1;
  return oly_gail_disc_fit_ws_floats(batch, ds + d2);
}

extern "C" int oly_gail_disc_fit_epoch(oly_ctx* ctx, const oly_gail_disc_fit* f, const int32_t* perm, int n_rows,
                                       int batch, oly_stream stream) {
  return oly_gail_disc_fit_epoch_pair(ctx, f, nullptr, perm, n_rows, batch, stream);
}

extern "C" int oly_gail_disc_fit_epoch_pair(oly_ctx* ctx, const oly_gail_disc_fit* f, const oly_disc_pair* pair,
                                            const int32_t* perm, int n_rows, int batch, oly_stream stream) {
  if (!ctx) return OLY_EINVAL;
  if (!f || !perm) OLY_FAIL(ctx, OLY_EINVAL, "oly_gail_disc_fit_epoch: NULL argument");
  const char* const name = "oly_gail_disc_fit_epoch";
  int rc = oly_fit::refuse_shape(ctx, name, pair, f->in_dim, oly_gail_disc_fit_ws_floats(batch, f->in_dim) >= 0, OLY_EINVAL,
                                 MAX_BATCH, n_rows, batch, f->n_plcy);
  if (rc != OLY_OK) return rc;
  if (!f->x || !f->colstats || !f->param || !f->exp_avg || !f->exp_avg_sq || !f->packed || !f->ws)
    OLY_FAIL(ctx, OLY_EINVAL, "oly_gail_disc_fit_epoch: NULL pointer in the argument block");
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
  a.colstats = f->colstats;
  a.param = f->param;
  a.m = f->exp_avg;
  a.v = f->exp_avg_sq;
  a.packed = f->packed;
  a.ws = f->ws;
  a.entcoeff = f->entcoeff;
  a.wd = f->weight_decay;
  a.P = param_layout(in_dim, 1);
  a.W = W;
  const float* p = f->param;
  const ParamLayout& P = a.P;
  rc = oly_ilmlp_pack(ctx, in_dim, H1, H2, 1, p + P.w1, p + P.b1, p + P.w2, p + P.b2, p + P.w3, p + P.b3, f->packed,
                                stream);
  if (rc != OLY_OK) return rc;
  oly_fit::set_minibatch(a, 0, nb, n_rows, batch);
  hipLaunchKernelGGL(gfit_prologue_kernel, dim3(PRO_BLOCKS), dim3(THREADS), 0, oly_s(stream), a);
  for (int b = 0; b < nb; ++b) {
    oly_fit::set_minibatch(a, b, nb, n_rows, batch);
    a.ad = oly_fit::adam_scalars(f->beta1, f->beta2, f->adam_eps, f->lr, (long)f->step + b + 1);
    a.loss_out = f->loss_out ? f->loss_out + b : nullptr;
    a.bce_out = f->bce_out ? f->bce_out + b : nullptr;
    a.ent_out = f->ent_out ? f->ent_out + b : nullptr;
    const dim3 grid_a((unsigned)((a.R + 15) / 16));
    rc = launch_rows(ctx, ctx->gail_attr_done, 1u << 16, gfit_rows_kernel<2>, gfit_rows_kernel<4>, in_dim, grid_a, ROWS_LDS,
                     stream, a);
    if (rc != OLY_OK) return rc;
    hipLaunchKernelGGL(gfit_weights_kernel, dim3(weight_tiles(in_dim, 1)), dim3(THREADS), 0, oly_s(stream), a);
  }
  OLY_LAUNCH_CHECK(ctx, "gail discriminator fit kernels");
  return OLY_OK;
}
