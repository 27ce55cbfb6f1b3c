// Pieces of the imitation-learning MLP  in -> 512 -> 256 -> out  that its kernels share: the packed operand stream's
// layout, the flat parameter order and the forward kernel on the f32 matrix cores.  The forward kernel is K16's
// (csrc/k16_il_critic.hip: relu hidden layers, the critic and the policy mean) and K18's (csrc/k18_gail_disc.hip: tanh
// hidden layers, GAIL's discriminator); the layout and the chain `tiles` are also those of K21 and K25 and, through
// ilmlp_fit.h, of the fits K18, K24 (csrc/k24_bc_fit.hip) and K26 (csrc/k26_iq_critic.hip), whose rows kernels keep the
// forward kernel's chain order.
#pragma once
#include "disc_common.h"
#include "mlp_tiles.h"
#include "oly_common.h"

namespace oly_ilmlp {
using oly_mlp::act16_index;
using oly_mlp::f32x4;
using oly_mlp::store_relu16v;

constexpr int IN_MAX = 64, H1 = 512, H2 = 256, OUT_MAX = 32;

// Packed stream (floats), the B operand of v_mfma_f32_16x16x4_f32 for every layer:
//   P[tile][group g][lane][q] = W[n = 16 tile + (lane & 15)][k = 16 g + 4 q + (lane >> 4)]   (zero outside the shape)
// W1: 32 tiles x 4 groups (k padded to 64), W2: 16 x 32, W3: 2 x 16 (n padded to 32); biases b1 [512], b2 [256],
// b3 [32] (padded with zeros).
constexpr size_t P_W1 = 0, P_B1 = P_W1 + (size_t)(H1 / 16) * (IN_MAX / 16) * 256, P_W2 = P_B1 + H1,
                 P_B2 = P_W2 + (size_t)(H2 / 16) * (H1 / 16) * 256, P_W3 = P_B2 + H2,
                 P_B3 = P_W3 + (size_t)(OUT_MAX / 16) * (H2 / 16) * 256, P_TOTAL = P_B3 + OUT_MAX;
static_assert(P_B1 % 4 == 0 && P_W2 % 4 == 0 && P_W3 % 4 == 0 && P_TOTAL % 4 == 0, "16-byte aligned sections");

// offset of W[n][k] in a packed section of `groups` k-groups
__host__ __device__ inline size_t pk_index(size_t base, int groups, int n, int k) {
  const int lane = (n & 15) | ((k & 3) << 4), q = (k >> 2) & 3;
  return base + ((size_t)((n >> 4) * groups + (k >> 4)) * 64 + lane) * 4 + q;
}

// torch parameter order: W1 [512,in] | b1 [512] | W2 [256,512] | b2 [256] | W3 [out,256] | b3 [out]
struct ParamLayout {
  int in_dim, out_dim;
  size_t w1, b1, w2, b2, w3, b3, total;
};
__host__ __device__ inline ParamLayout param_layout(int in_dim, int out_dim) {
  ParamLayout L;
  L.in_dim = in_dim;
  L.out_dim = out_dim;
  L.w1 = 0;
  L.b1 = (size_t)H1 * in_dim;
  L.w2 = L.b1 + H1;
  L.b2 = L.w2 + (size_t)H2 * H1;
  L.w3 = L.b2 + H2;
  L.b3 = L.w3 + (size_t)out_dim * H2;
  L.total = L.b3 + out_dim;
  return L;
}

// where parameter i (torch order) lives in the packed stream
__device__ inline size_t packed_of_param(const ParamLayout& L, size_t i) {
  if (i < L.b1) return pk_index(P_W1, IN_MAX / 16, (int)(i / L.in_dim), (int)(i % L.in_dim));
  if (i < L.w2) return P_B1 + (i - L.b1);
  if (i < L.b2) return pk_index(P_W2, H1 / 16, (int)((i - L.w2) / H1), (int)((i - L.w2) % H1));
  if (i < L.w3) return P_B2 + (i - L.b2);
  if (i < L.b3) return pk_index(P_W3, H2 / 16, (int)((i - L.w3) / H2), (int)((i - L.w3) % H2));
  return P_B3 + (i - L.b3);
}

// bias + activation of a 16 x 16 accumulator tile into the activation image of the next layer
template <bool HT>
__device__ __forceinline__ void store_act16v(const f32x4& acc, float bv, int tile, int lane, float* __restrict__ img) {
  if (!HT) {
    store_relu16v(acc, bv, tile, lane, img);
  } else {
    const int c = lane & 15, h2 = lane >> 4;
    float* dst = img + ((tile * 4 + (c & 3)) * 16 + 4 * h2) * 4 + (c >> 2);
#pragma unroll
    for (int i = 0; i < 4; ++i) dst[4 * i] = oly_disc::tanh32(acc[i] + bv);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Forward.  256 threads = 4 waves; RS 16-row sub-tiles per workgroup.  Layer 1: wave w owns column tiles 8 w .. 8 w + 7,
// layer 2: 4 w .. 4 w + 3; the output layer: wave w runs (sub-tile, column tile) pair w as ONE chain over k < 256.
constexpr int FWD_THREADS = 256;

struct FwdArgs {
  long N;
  int in_dim, out_dim, act;
  int stride;               // floats between the rows of x
  const float* x;
  const int* mask;          // [in_dim] columns of x, or NULL (identity)
  const double *mean, *sd, *colstats;
  const float* packed;
  float* y;
  float* reward;            // [N] reward_of(y) (out_dim == 1), or NULL
  // The discriminator's second part (DiscriminatorNetwork.preprocess_inputs, networks.py:216-234), d2 == 0: none.
  // Columns [in_dim - d2, in_dim) of the input are x2[row, mask2[k - ds]]: next states standardised with colstats2
  // (std2, the statistics after the Standardizer's SECOND update of the forward) or actions taken raw.
  int d2, std2, stride2;
  const float* x2;
  const int* mask2;         // [d2] columns of x2, or NULL (identity)
  const double* colstats2;  // [3, in_dim - d2], as colstats
};

template <int RS>
constexpr size_t fwd_lds() { return sizeof(float) * (size_t)RS * (IN_MAX + H1 + H2) * 16 + 2 * sizeof(double) * IN_MAX; }

// NT column tiles of one wave x RS row sub-tiles, G k-groups in order; w: this wave's first tile, tstride float4s
// between tiles
template <int G, int NT, int RS>
__device__ __forceinline__ void tiles(const float4* const (&a4)[RS], const float4* __restrict__ w, size_t tstride, int lane,
                                      f32x4 (&acc)[RS][NT]) {
#pragma unroll 2
  for (int g = 0; g < G; ++g) {
    float4 b[NT], a[RS];
#pragma unroll
    for (int t = 0; t < NT; ++t) b[t] = w[t * tstride + (size_t)g * 64 + lane];
#pragma unroll
    for (int s = 0; s < RS; ++s) a[s] = a4[s][g * 64 + lane];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const float bq = q == 0 ? b[t].x : q == 1 ? b[t].y : q == 2 ? b[t].z : b[t].w;
#pragma unroll
        for (int s = 0; s < RS; ++s) {
          const float aq = q == 0 ? a[s].x : q == 1 ? a[s].y : q == 2 ? a[s].z : a[s].w;
          acc[s][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq, bq, acc[s][t], 0, 0, 0);
        }
      }
    }
  }
}

// HT: tanh32 hidden layers (GAIL's discriminator, K18) instead of relu (K16)
template <int RS, int G1, bool HT>
__global__ __launch_bounds__(FWD_THREADS) void ilmlp_forward_kernel(FwdArgs p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xT = lds;                                   // [RS][64 x 16]   input images (act16 layout)
  float* hA = xT + (size_t)RS * IN_MAX * 16;         // [RS][512 x 16]  layer-1 images
  float* hB = hA + (size_t)RS * H1 * 16;             // [RS][256 x 16]  layer-2 images
  double* s_mean = reinterpret_cast<double*>(hB + (size_t)RS * H2 * 16);
  double* s_sd = s_mean + IN_MAX;
  const float* __restrict__ P = p.packed;
  const float4* P4 = reinterpret_cast<const float4*>(P);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long row0 = (long)blockIdx.x * (16 * RS);
  const int in_dim = p.in_dim, ds = in_dim - p.d2;     // ds: the Standardizer's columns (the first part)
  const bool standardise = p.mean || p.colstats;

  if (tid < in_dim && standardise) {
    double mean, sd;
    if (p.colstats && tid >= ds && !p.std2) {   // actions pass through: f32((f64(a) - 0) / 1) is a
      mean = 0.0;
      sd = 1.0;
    } else if (p.colstats) {    // Standardizer.update_mean_std's derivation (networks.py:54-56,76-81), as K12
      const double* cs = tid < ds ? p.colstats : p.colstats2;
      const int j = tid < ds ? tid : tid - ds;
      const double cnt = cs[j] + 1e-2;
      mean = cs[ds + j] / cnt;
      sd = sqrt(fmax((cs[2 * ds + j] + 1e-2) / cnt - mean * mean, 1e-2));
    } else {
      mean = p.mean[tid];
      sd = p.sd[tid];
    }
    s_mean[tid] = mean;
    s_sd[tid] = sd;
  }
  __syncthreads();
  for (int e = tid; e < RS * 16 * IN_MAX; e += FWD_THREADS) {
    const int s = e / (16 * IN_MAX), m = (e / IN_MAX) & 15, k = e & (IN_MAX - 1);
    const long row = row0 + 16 * s + m;
    float v = 0.f;
    if (row < p.N && k < in_dim) {
      const float xv = k < ds ? p.x[row * p.stride + (p.mask ? p.mask[k] : k)]
                              : p.x2[row * p.stride2 + (p.mask2 ? p.mask2[k - ds] : k - ds)];
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
      for (int s = 0; s < RS; ++s) store_act16v<HT>(acc[s][t], bv, 8 * wave + t, lane, hA + (size_t)s * H1 * 16);
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
      for (int s = 0; s < RS; ++s) store_act16v<HT>(acc[s][t], bv, 4 * wave + t, lane, hB + (size_t)s * H2 * 16);
    }
  }
  __syncthreads();
  // ---- output layer: [16, 256] x [256, 16] per (sub-tile, column tile) pair
  const int nt3 = p.out_dim > 16 ? 2 : 1;
  if (wave < RS * nt3) {
    const int s = wave / nt3, t = wave - s * nt3;
    f32x4 acc[1][1] = {{f32x4{0.f, 0.f, 0.f, 0.f}}};
    const float4* a4[1] = {reinterpret_cast<const float4*>(hB + (size_t)s * H2 * 16)};
    tiles<H2 / 16, 1, 1>(a4, P4 + P_W3 / 4 + (size_t)t * (H2 / 16) * 64, 0, lane, acc);
    const int col = 16 * t + (lane & 15);
    if (col < p.out_dim) {
      const float bv = P[P_B3 + col];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long row = row0 + 16 * s + 4 * (lane >> 4) + i;
        if (row < p.N) {
          float v = acc[0][0][i] + bv;
          if (p.act == OLY_ACT_TANH) v = tanhf(v);
          if (p.y) p.y[row * p.out_dim + col] = v;
          if (p.reward) p.reward[row] = oly_disc::reward_of(v);
        }
      }
    }
  }
}

}  // namespace oly_ilmlp
