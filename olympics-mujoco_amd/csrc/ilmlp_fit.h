// The phases that the two-launch minibatch fits of the  in -> 512 -> 256 -> out  network share: K18
// (csrc/k18_gail_disc.hip, GAIL's discriminator, tanh hidden layers), K24 (csrc/k24_bc_fit.hip, behavioural cloning, relu),
// K26 (csrc/k26_iq_critic.hip, the soft-Q critic, relu) and K27 (csrc/k27_iq_policy.hip, the SAC family's policy update,
// whose launch A is cut in two where the critic's statistics need every row's action).  Launch A ("rows") takes one 16-row tile per 512-thread
// workgroup through the forward and the data gradients on the f32 matrix cores; launch B ("weights") takes one 16 x 16
// weight tile per 256-thread workgroup through dW, Adam and the re-pack.  The loss, the output layer, the Standardizer's
// accounting and the Adam stores are each kernel's own.  As in fit_common.h, the order of every addition is what the tests
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

// ---- the prologue: W2T, the B operand of dH1 = dZ2 W2 (pt_index, N = 256 outputs), from param; grid PRO_BLOCKS x THREADS
template <class A>
__device__ __forceinline__ void build_w2t(const A& a) {
  for (int e = blockIdx.x * THREADS + threadIdx.x; e < H2 * H1; e += PRO_BLOCKS * THREADS)
    a.ws[a.W.w2t + pt_index(H2, e / H1, e % H1)] = a.param[a.P.w2 + e];
}

// ---- launch B.  Tiles (n-tile x k-tile): W1 32 x ceil(in / 16), W2 16 x 32, W3 ceil(out / 16) x 16; the k-tile 0 of each
// layer also steps the layer's bias.  The decode of the workgroup's (layer, n-tile, k-tile) and the layer's shapes stay in
// each kernel: behind a function the compiler stops threading the three layers' branches through the loop below, and
// launch B's code changes (it loses the 32 bytes of scratch it has had and its flat loads: a speed change).  So do the
// per-layer Adam stores: with one indexed store behind a helper the layer's offsets are fetched after the barrier, and
// launch B ran about 1 % longer.
__host__ __device__ inline int weight_tiles(int in_dim, int out_dim) {
  return 32 * ((in_dim + 15) / 16) + 512 + 16 * ((out_dim + 15) / 16);
}

// The tile's dW and the column sums of delta over this wave's share of the rows (K24 and K26; K18 keeps its own text of
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
