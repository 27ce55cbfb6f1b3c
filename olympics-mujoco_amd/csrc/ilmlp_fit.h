// The phases that the two-launch minibatch fits of the  in -> 512 -> 256 -> out  network share: K18
// (csrc/k18_gail_disc.hip, GAIL's discriminator, tanh hidden layers), K24 (csrc/k24_bc_fit.hip, behavioural cloning, relu),
// K26 (csrc/k26_iq_critic.hip, the soft-Q critic, relu) and K27 (csrc/k27_iq_policy.hip, the SAC family's policy update,
// whose launch A is cut in two where the critic's statistics need every row's action).  Launch A ("rows") takes one 16-row tile per 512-thread
// workgroup through the forward and the data gradients on the f32 matrix cores; launch B ("weights") takes one 16 x 16
// weight tile per 256-thread workgroup through dW, Adam and the re-pack.  The loss, the Standardizer's accounting and what
// a step stores beside the parameter (a target, the transposed streams) are each kernel's own.  As in fit_common.h, the order of every addition is what the tests
// pin, and every function performs its users' float operations in their order.  These kernels' register allocation and
// load scheduling turn on small things, so a kernel takes a function from here only where it then ran no longer than with
// its own text (HIP events, 2048 rows); where one does not, the comment at the function says which and why.
#pragma once
#include "fit_common.h"
#include "ilmlp_common.h"
#include "mlp_tiles.h"

namespace oly_ilfit {
using namespace oly_ilmlp;
using oly_fit::NSP;
using oly_fit::pt_index;
using oly_fit::THREADS;

constexpr int RTHREADS = 512;       // launch A's workgroup: 8 waves, two per SIMD
constexpr int PRO_BLOCKS = 64;      // the prologue's grid
constexpr int STEP_UNROLL = 4;      // launch B: 16-row steps whose loads are issued together

// ---- the hidden layers' activations: f on the pre-activation, back = the gradient g through the STORED output h
struct Relu {
  static __device__ __forceinline__ float f(float z) { return (z > 0.f || z != z) ? z : 0.f; }   // NaN kept like torch
  static __device__ __forceinline__ float back(float g, float h) { return h > 0.f ? g : 0.f; }
};
struct Tanh {
  static __device__ __forceinline__ float f(float z) { return oly_disc::tanh32(z); }
  static __device__ __forceinline__ float back(float g, float h) { return g * (1.0f - h * h); }
};

// ---- the Standardizer's head (Standardizer.update_mean_std, networks.py:76-81)
// column `col`'s sum and sum of squares over the NSP slice partials sp [NSP][2][IN_MAX], slices in order
__device__ __forceinline__ void slice_sums(const double* sp, int col, double& s, double& ss) {
  s = ss = 0.0;
  for (int p = 0; p < NSP; ++p) {
    s += sp[p * 2 * IN_MAX + col];
    ss += sp[p * 2 * IN_MAX + IN_MAX + col];
  }
}

// mean and std of a column from its running count, sum and sum of squares
__device__ __forceinline__ void col_moments(double cnt, double sum, double sq, double& mean, double& sd) {
  const double n = cnt + 1e-2;
  mean = sum / n;
  sd = sqrt(fmax((sq + 1e-2) / n - mean * mean, 1e-2));
}

// ---- launch A
// A lane's four accumulator rows 4 h4 .. 4 h4 + 3 of column `col` in an act16 image (mlp_tiles.h)
__device__ __forceinline__ void put_quad(float* img, int col, int h4, const float4& v) {
  img[act16_index(col, 4 * h4)] = v.x;
  img[act16_index(col, 4 * h4 + 1)] = v.y;
  img[act16_index(col, 4 * h4 + 2)] = v.z;
  img[act16_index(col, 4 * h4 + 3)] = v.w;
}
__device__ __forceinline__ float4 get_quad(const float* img, int col, int h4) {
  return make_float4(img[act16_index(col, 4 * h4)], img[act16_index(col, 4 * h4 + 1)], img[act16_index(col, 4 * h4 + 2)],
                     img[act16_index(col, 4 * h4 + 3)]);
}

// One hidden layer forward for this wave's NT column tiles (NT wave .. NT wave + NT - 1): the forward kernel's chain over
// G k-groups of the image `in` against the packed section at P + PW (GS groups per tile), the bias at P + PB, Act, the
// result into the image `out`.  With `keep` the lane's row quad of each column also goes to the workspace array at float
// `off` ([rows][128 NT] in row quads, this lane's quad `quad`).
// K26 and K27 call it.  K18 and K24 keep their own text of the two layers: with this function their rows kernels need
// eight registers fewer, the compiler then schedules the whole kernel for one more wave per SIMD (which a 512-thread
// workgroup with this much LDS never has) and stops issuing dZ1's weight loads ahead: launch A ran 2.3 % (K18) and 3.7 %
// (K24) longer at 2048 rows.  The lane and wave indices are re-derived from threadIdx: as parameters their signs are
// unknown where this function is simplified, and the index arithmetic comes out longer.
template <class Act, int G, int GS, int NT, size_t PW, size_t PB>
__device__ __forceinline__ void hidden_layer(const float* in, const float* P, float* out, bool keep, float4* ws4, size_t off,
                                             size_t quad) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  f32x4 acc[1][NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[0][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float4* a4[1] = {reinterpret_cast<const float4*>(in)};
  tiles<G, NT, 1>(a4, reinterpret_cast<const float4*>(P) + PW / 4 + (size_t)(NT * wave) * GS * 64, GS * 64, lane, acc);
  const int c = lane & 15, h4 = lane >> 4;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int col = 16 * (NT * wave + t) + c;
    const float bv = P[PB + col];
    float4 h;
    h.x = Act::f(acc[0][t][0] + bv);
    h.y = Act::f(acc[0][t][1] + bv);
    h.z = Act::f(acc[0][t][2] + bv);
    h.w = Act::f(acc[0][t][3] + bv);
    put_quad(out, col, h4, h);
    if (keep) ws4[(off >> 2) + quad * (128 * NT) + col] = h;
  }
}

// dZ1 = (dZ2 W2) act'(h1) for this wave's column tiles 4 wave .. 4 wave + 3: the chain over the 256 layer-2 units of the
// image gz against the transposed stream w2t (pt_index), the lane's stored h1 quad of a column from h1_at(col), the row
// quad `quad` to the workspace array at float `off`.
template <class Act, class H1At>
__device__ __forceinline__ void dz1_tiles(const float* gz, const float4* w2t, H1At h1_at, float4* ws4, size_t off,
                                          size_t quad) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  f32x4 acc[1][4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[0][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float4* a4[1] = {reinterpret_cast<const float4*>(gz)};
  tiles<H2 / 16, 4, 1>(a4, w2t + (size_t)(4 * wave) * (H2 / 16) * 64, (H2 / 16) * 64, lane, acc);
  const int c = lane & 15;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int col = 16 * (4 * wave + t) + c;
    const float4 h = h1_at(col);
    float4 g;
    g.x = Act::back(acc[0][t][0], h.x);
    g.y = Act::back(acc[0][t][1], h.y);
    g.z = Act::back(acc[0][t][2], h.z);
    g.w = Act::back(acc[0][t][3], h.w);
    ws4[(off >> 2) + quad * H1 + col] = g;
  }
}

// Stage the tile's 16 rows: value_at(m, k) of a row the pass takes (takes(m)) in columns k < D, with `standardise` through
// the column's mean st[k] and std st[IN_MAX + k] in LDS, a row or column beyond them as zero, into the image xT and, with
// `keep`, into the workspace's xs array (ws + W.xs) in row quads from row srow0, in the caller's index type (an int; a
// size_t where slots make it one).  K24's and K26's rows kernels and K27's two call it.
template <class Takes, class ValueAt, class Row>
__device__ __forceinline__ void stage_rows(float* xT, int D, bool standardise, const double* st, Takes takes, ValueAt value_at,
                                           bool keep, float* xs, Row srow0) {
  for (int e = threadIdx.x; e < 16 * IN_MAX; e += RTHREADS) {
    const int m = e / IN_MAX, k = e & (IN_MAX - 1);
    float v = 0.f;
    if (takes(m) && k < D) {
      v = value_at(m, k);
      // f32((f64(x) - mean) / std): the reference subtracts fp64 statistics and narrows afterwards (networks.py:68-74)
      if (standardise) v = (float)(((double)v - st[k]) / st[IN_MAX + k]);
    }
    xT[act16_index(k, m)] = v;
    if (keep) xs[((size_t)((srow0 + m) >> 2) * IN_MAX + k) * 4 + (m & 3)] = v;
  }
}

// The one-unit output layer by wave 0: one chain over k < 256 of the image hB against the packed section P + P_W3, as
// the forward kernel's, plus the bias; row r's value to z[r] and qv[r].  K27's launch A2 calls it for each critic.  K26's
// rows kernel keeps its own text of it: with this function it is allocated two to four registers fewer and scheduled for
// one more wave per SIMD (which it never has), and its call ran 0.4 to 1.1 us longer at 512 rows without a target.
__device__ __forceinline__ void output_unit(const float* hB, const float* P, float* z, float* qv) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (wave != 0) return;
  f32x4 acc[1][1] = {{f32x4{0.f, 0.f, 0.f, 0.f}}};
  const float4* a4[1] = {reinterpret_cast<const float4*>(hB)};
  tiles<H2 / 16, 1, 1>(a4, reinterpret_cast<const float4*>(P) + P_W3 / 4, 0, lane, acc);
  if ((lane & 15) == 0) {
    const int h4 = lane >> 4;
    const float bv = P[P_B3];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float q = acc[0][0][i] + bv;
      z[4 * h4 + i] = q;
      qv[4 * h4 + i] = q;
    }
  }
}

// ---- the prologue: W2T, the B operand of dH1 = dZ2 W2 (pt_index, N = 256 outputs), from param; grid PRO_BLOCKS x THREADS
template <class A>
__device__ __forceinline__ void build_w2t(const A& a) {
  for (int e = blockIdx.x * THREADS + threadIdx.x; e < H2 * H1; e += PRO_BLOCKS * THREADS)
    a.ws[a.W.w2t + pt_index(H2, e / H1, e % H1)] = a.param[a.P.w2 + e];
}

// ---- launch B.  Tiles (n-tile x k-tile): W1 32 x ceil(in / 16), W2 16 x 32, W3 ceil(out / 16) x 16; the k-tile 0 of each
// layer also steps the layer's bias.  K26 and K27 take the decode, the step and the gradient-norm partial from here; K18
// keeps its own text of all of launch B, K24 of the decode and the step (through them its step ran 0.5 to 0.8 % longer).
// weight_tile returns its struct from a function on purpose: filled by a constructor instead, the three kernels lost the
// 32 bytes of scratch they have had and launch B ran 8 us longer per 512 rows of a slot.
__host__ __device__ inline int weight_tiles(int in_dim, int out_dim) {
  return 32 * ((in_dim + 15) / 16) + 512 + 16 * ((out_dim + 15) / 16);
}

// The workgroup's tile: layer, n-tile nt and k-tile kt from blockIdx.x, the tile's first output n0 and input k0, and the
// layer's delta dl [rows][dw] (N columns used) and activation al [rows][aw] (K columns used), both in row quads, from
// the workspace layout's xs / h1 / h2 / dz1 / dz2 / dz3.  in_dim: the network's inputs; the output layer has out_dim
// units in a delta of pitch out_pitch (K26: 1 and 1; K24 and K27: 2A and OUT_MAX).
struct WeightTile {
  int layer, nt, kt, n0, k0, dw, N, aw, K;
  const float4 *dl, *al;
};
template <class A>
__device__ __forceinline__ WeightTile weight_tile(const A& a, int in_dim, int out_dim, int out_pitch) {
  WeightTile T;
  const int kt0 = (in_dim + 15) / 16;
  int t = blockIdx.x;
  if (t < 32 * kt0) {
    T.layer = 0, T.nt = t / kt0, T.kt = t % kt0;
  } else if ((t -= 32 * kt0) < 512) {
    T.layer = 1, T.nt = t / 32, T.kt = t % 32;
  } else {
    T.layer = 2, T.nt = (t - 512) / 16, T.kt = (t - 512) % 16;
  }
  const int layer = T.layer;
  T.dw = layer == 0 ? H1 : layer == 1 ? H2 : out_pitch;
  T.N = layer == 2 ? out_dim : T.dw;
  T.aw = layer == 0 ? IN_MAX : layer == 1 ? H1 : H2;
  T.K = layer == 0 ? in_dim : T.aw;
  T.dl = reinterpret_cast<const float4*>(a.ws + (layer == 0 ? a.W.dz1 : layer == 1 ? a.W.dz2 : a.W.dz3));
  T.al = reinterpret_cast<const float4*>(a.ws + (layer == 0 ? a.W.xs : layer == 1 ? a.W.h1 : a.W.h2));
  T.n0 = 16 * T.nt, T.k0 = 16 * T.kt;
  return T;
}

// The tile's dW and the column sums of delta over this wave's share of the rows (K24, K26 and K27; K18 keeps its own text of
// this loop and of meet_waves, with which its launch B ran 1 to 3 % shorter).  delta dl [rows][dw] (N columns used) and
// activation al [rows][aw] (K columns used) are in row quads.  A step = the 16 rows of one tile of launch A (which wrote
// all 16: zeros in the deltas beyond the minibatch); lane group h4 takes the step's row quad h4.  Wave w: steps
// [w Q, min(steps, (w + 1) Q)).
__device__ __forceinline__ void dw_accumulate(const float4* dl, const float4* al, int dw, int aw, int n0, int N, int k0, int K,
                                              int steps, f32x4& acc, float& bsum) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, h4 = lane >> 4;
  const bool n_ok = n0 + c < N, k_ok = k0 + c < K;
  const int Q = (steps + 3) / 4, s0 = wave * Q, s1 = min(steps, s0 + Q);
  acc = f32x4{0.f, 0.f, 0.f, 0.f};
  bsum = 0.f;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int s = s0; s < s1; s += STEP_UNROLL) {
    float4 dv[STEP_UNROLL], av[STEP_UNROLL];
#pragma unroll
    for (int u = 0; u < STEP_UNROLL; ++u) {
      const size_t q = (size_t)4 * (s + u) + h4;
      const bool in = s + u < s1;
      dv[u] = (in && n_ok) ? dl[q * dw + n0 + c] : zero4;
      av[u] = (in && k_ok) ? al[q * aw + k0 + c] : zero4;
    }
#pragma unroll
    for (int u = 0; u < STEP_UNROLL; ++u) {
      // A[i = lane & 15][r = lane >> 4] = delta[row 4 q + r][n0 + i], B[r][j = lane & 15] = a[row 4 q + r][k0 + j]
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(dv[u].x, av[u].x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(dv[u].y, av[u].y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(dv[u].z, av[u].z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(dv[u].w, av[u].w, acc, 0, 0, 0);
      bsum += ((dv[u].x + dv[u].y) + dv[u].z) + dv[u].w;
    }
  }
}

// the waves meet: red [4 waves][16 n][16 k] (D[n = 4 (lane >> 4) + i][k = lane & 15]) and bred [4 waves][64 lanes]
__device__ __forceinline__ void meet_waves(float* red, float* bred, const f32x4& acc, float bsum) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, h4 = lane >> 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) red[wave * 256 + (4 * h4 + i) * 16 + c] = acc[i];
  bred[wave * 64 + lane] = bsum;
  __syncthreads();
}

// The tile's step after meet_waves.  Thread (n = tid >> 4, k = tid & 15): the element's gradient g, the waves' four
// partials in order, its flat parameter index i (layout a.P, in_dim columns in W1) and its packed index pk, handed to
// step(layer, ne, ke, i, pk, g), which makes the Adam step and the caller's stores.  With the layer's k-tile 0, threads
// < 16 the same for the bias of output n0 + tid (fit_common.h's bias_colsum; ke = -1).  g2, b2: the squares of the two
// gradients in fp64, 0 where the thread has none.
template <class A, class Step>
__device__ __forceinline__ void tile_step(const WeightTile& T, const A& a, int in_dim, const float* red, const float* bred,
                                          Step step, double& g2, double& b2) {
  const int tid = threadIdx.x, ne = T.n0 + (tid >> 4), ke = T.k0 + (tid & 15);
  g2 = b2 = 0.0;
  if (ne < T.N && ke < T.K) {
    const float g = ((red[tid] + red[256 + tid]) + red[512 + tid]) + red[768 + tid];
    g2 = (double)g * (double)g;
    size_t i, pk;
    if (T.layer == 0) i = a.P.w1 + (size_t)ne * in_dim + ke, pk = pk_index(P_W1, IN_MAX / 16, ne, ke);
    else if (T.layer == 1) i = a.P.w2 + (size_t)ne * H1 + ke, pk = pk_index(P_W2, H1 / 16, ne, ke);
    else i = a.P.w3 + (size_t)ne * H2 + ke, pk = pk_index(P_W3, H2 / 16, ne, ke);
    step(T.layer, ne, ke, i, pk, g);
  }
  if (T.kt == 0 && tid < 16 && T.n0 + tid < T.N) {   // the bias: the column sums of delta, lane groups then waves in order
    const float gb = oly_fit::bias_colsum(bred, tid);
    b2 = (double)gb * (double)gb;
    const size_t pb = (T.layer == 0 ? a.P.b1 : T.layer == 1 ? a.P.b2 : a.P.b3) + T.n0 + tid;
    const size_t kb = (T.layer == 0 ? P_B1 : T.layer == 1 ? P_B2 : P_B3) + T.n0 + tid;
    step(T.layer, T.n0 + tid, -1, pb, kb, gb);
  }
}

// The sum of the workgroup's THREADS values v by a halving tree in dred [THREADS]; every thread calls it and gets the sum.
__device__ __forceinline__ double tree_sum(double* dred, double v) {
  const int tid = threadIdx.x;
  dred[tid] = v;
  __syncthreads();
  for (int h = THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) dred[tid] += dred[tid + h];
    __syncthreads();
  }
  return dred[0];
}

// The tile's sum of squared gradients (tile_step's g2 and b2) to its slot of gnp: the tree over the elements, then the 16
// bias squares in order (bsq [16]).  Launch F's total of the `tiles` slots: thread t adds t, t + THREADS, ..., then the tree.
__device__ __forceinline__ void gradnorm_partial(double* dred, double* bsq, double g2, double b2, double* gnp) {
  if (threadIdx.x < 16) bsq[threadIdx.x] = b2;
  double s = tree_sum(dred, g2);
  if (threadIdx.x == 0) {
    for (int j = 0; j < 16; ++j) s += bsq[j];
    gnp[blockIdx.x] = s;
  }
}
__device__ __forceinline__ double gradnorm_total(double* dred, const double* gnp, int tiles) {
  double s = 0.0;
  for (int t = threadIdx.x; t < tiles; t += THREADS) s += gnp[t];
  return tree_sum(dred, s);
}

// ---- the host side: launch A for in_dim columns (<2> k-groups in layer 1 up to 32, else <4>), its dynamic LDS allowed on
// the instantiation's first use (`done`: the context's flags, bit / bit << 1 the two instantiations')
template <class A>
inline int launch_rows(oly_ctx* ctx, unsigned& done, unsigned bit, void (*kernel2)(A), void (*kernel4)(A), int in_dim,
                       dim3 grid, size_t lds, oly_stream stream, const A& a) {
  void (*const kernel)(A) = in_dim <= 32 ? kernel2 : kernel4;
  if (in_dim > 32) bit <<= 1;
  if (!(done & bit)) {
    OLY_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    done |= bit;
  }
  hipLaunchKernelGGL(kernel, grid, dim3(RTHREADS), lds, oly_s(stream), a);
  return OLY_OK;
}

}  // namespace oly_ilfit
