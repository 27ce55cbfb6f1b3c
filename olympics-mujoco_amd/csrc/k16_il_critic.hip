// K16: the imitation-learning MLP  in -> 512 -> 256 -> out  (relu, relu, identity | tanh): the critic of
// examples/imitation_learning/utils.py:136-149 (FullyConnectedNetwork, networks.py:88-160, out = 1) and, with tanh and
// out <= 32, the policy mean of :126-134.  Two things in this file:
//
//   oly_ilmlp_forward        the forward on the f32 matrix cores (v_mfma_f32_16x16x4_f32), 16-row tiles for small N,
//                            32-row tiles (two 16-row sub-tiles sharing every weight load) for large N.
//                            The kernel, the stream's layout and the parameter order are in ilmlp_common.h, which
//                            K18 (GAIL's tanh discriminator) shares; this file launches the relu form.
//   oly_il_critic_fit_epoch  one epoch of mushroom's Regressor.fit for the critic (out = 1): per minibatch the
//                            Standardizer update (networks.py:68-81), forward, F.mse_loss, backward and one
//                            torch.optim.Adam step, 3 launches per minibatch split over the weight COLUMNS
//                            (DESIGN.md section 11), plus one closing launch per call.
//
// Numerics.  Forward: every pre-activation is the f32 fma chain over k ascending from 0, bias added after the chain (the
// MFMA is bit-for-bit that chain; the zero-padded k add exact zeros), so both tile sizes give identical values.  The fit
// runs the same chains for layers 1 and 2 on the vector ALU (fmaf, k ascending) and the output layer as one chain over
// k < 256; gradients are fma chains over the minibatch rows in ascending order, dH1 is the sum of 16 partial chains
// (16 layer-2 units each) added in slice order.  Every reduction has a fixed order: two runs give identical bits.
// Adam's scalars and the clamp of a perm entry are the ones K15 and K18 use (fit_common.h).
#include <cstdlib>

#include "fit_common.h"
#include "ilmlp_common.h"
#include "mlp_tiles.h"
#include "oly_common.h"

namespace {
using namespace oly_ilmlp;
using oly_fit::AdamK;
using oly_fit::row_at;

__global__ void ilmlp_pack_kernel(int in_dim, int out_dim, const float* __restrict__ w1, const float* __restrict__ b1,
                                  const float* __restrict__ w2, const float* __restrict__ b2,
                                  const float* __restrict__ w3, const float* __restrict__ b3, float* __restrict__ out) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < P_TOTAL; e += (size_t)gridDim.x * blockDim.x) {
    float v = 0.f;
    if (e < P_B1 || (e >= P_W2 && e < P_B2) || (e >= P_W3 && e < P_B3)) {
      const size_t base = e < P_B1 ? P_W1 : e < P_B2 ? P_W2 : P_W3;
      const int groups = e < P_B1 ? IN_MAX / 16 : e < P_B2 ? H1 / 16 : H2 / 16;
      const size_t r = e - base;
      const int q = (int)(r & 3), lane = (int)((r >> 2) & 63);
      const int g = (int)((r >> 8) % groups), tile = (int)((r >> 8) / groups);
      const int n = 16 * tile + (lane & 15), k = 16 * g + 4 * q + (lane >> 4);
      if (base == P_W1) v = k < in_dim ? w1[(size_t)n * in_dim + k] : 0.f;
      else if (base == P_W2) v = w2[(size_t)n * H1 + k];
      else v = n < out_dim ? w3[(size_t)n * H2 + k] : 0.f;
    } else if (e < P_W2) {
      v = b1[e - P_B1];
    } else if (e < P_W3) {
      v = b2[e - P_B2];
    } else {
      const int n = (int)(e - P_B3);
      v = n < out_dim ? b3[n] : 0.f;
    }
    out[e] = v;
  }
}

template <int RS>
int launch_forward(oly_ctx* ctx, const FwdArgs& a, oly_stream stream) {
  const unsigned bit = 1u << (4 * (RS - 1) + (a.in_dim + 15) / 16);
  const dim3 grid((unsigned)((a.N + 16 * RS - 1) / (16 * RS)));
  const size_t lds = fwd_lds<RS>();
  switch ((a.in_dim + 15) / 16) {
#define OLY_ILMLP_CASE(G)                                                                                             \
  case G:                                                                                                             \
    if (!(ctx->ilmlp_attr_done & bit)) {                                                                              \
      OLY_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(ilmlp_forward_kernel<RS, G, false>),             \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                        \
      ctx->ilmlp_attr_done |= bit;                                                                                    \
    }                                                                                                                 \
    hipLaunchKernelGGL((ilmlp_forward_kernel<RS, G, false>), grid, dim3(FWD_THREADS), lds, oly_s(stream), a);         \
    break;
    OLY_ILMLP_CASE(1)
    OLY_ILMLP_CASE(2)
    OLY_ILMLP_CASE(3)
    OLY_ILMLP_CASE(4)
#undef OLY_ILMLP_CASE
  }
  OLY_LAUNCH_CHECK(ctx, "ilmlp_forward_kernel");
  return OLY_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Fit.  Per minibatch b (R <= 256 rows), three launches:
//   A  fit_l1_kernel   32 workgroups x 16 layer-1 units: [close minibatch b-1: dH1 from the 16 partials, dZ1, dW1 / db1,
//                      Adam on W1 / b1 (and, workgroup 0, on W3 / b3)]; statistics of minibatch b (each workgroup sums
//                      the rows itself, in the same order), standardise, H1 = relu(Xs W1^T + b1) for its 16 units.
//   B  fit_l2_kernel   16 x 16 layer-2 units x 64-row blocks: H2 = relu(H1 W2^T + b2).
//   C  fit_bwd_kernel  16 x 16 layer-2 units x 4 x 128 layer-1 units: y (one chain over k < 256), loss, dy, dZ2,
//                      dW2 for its tile, db2 / dW3 / db3, the dH1 partial of its 16 units over its 128 columns,
//                      Adam on its W2 tile and b2; the running statistics += minibatch b.
// The closing launch A (no minibatch b) finishes the last minibatch.  Every weight is written by the workgroup that
// owns it, after that workgroup has read the old value; nothing reads a weight that another workgroup of the same
// launch writes (W3 / b3, which every workgroup of C reads, are stepped by the next A).
constexpr int FIT_THREADS = 256, MAX_BATCH = 256, NS2 = H2 / 16;   // NS2: layer-2 slices (dH1 partials)
// workspace (floats): colstats delta [2][64] f64 | dW3 [256], db3 | H1 [256][512] | H2 [256][256] | dH1 partials
// [16][256][512] | standardised rows [2][256][64] (by minibatch parity)
constexpr size_t WS_DELTA = 0, WS_G3 = 256, WS_H1 = 768, WS_H2 = WS_H1 + (size_t)MAX_BATCH * H1,
                 WS_DH1 = WS_H2 + (size_t)MAX_BATCH * H2, WS_XS = WS_DH1 + (size_t)NS2 * MAX_BATCH * H1,
                 WS_TOTAL = WS_XS + (size_t)2 * MAX_BATCH * IN_MAX;

struct FitArgs {
  int n_rows, in_dim;
  int r_prev, r_cur;        // rows of minibatch b-1 / b (0: none)
  int par_prev, par_cur;    // parity of b-1 / b (standardised-row buffers)
  const int32_t* perm;      // rows of minibatch b
  const float* x;
  const float* vt;
  double* colstats;
  float *param, *m, *v, *packed, *ws;
  double* loss;             // loss_out + b
  AdamK ad_prev, ad_cur;
};

// torch.optim.Adam.step (amsgrad off, no decay) on one element.  Not oly_fit::adam1: this one reads param after it has
// stored the moments, and the two orders compile to different code.
__device__ __forceinline__ float adam1(const FitArgs& a, const AdamK& k, size_t i, float g) {
  float m = a.m[i], v = a.v[i];
  m = m + (g - m) * k.w1;
  v = v * k.beta2 + (k.w2 * g) * g;
  a.m[i] = m;
  a.v[i] = v;
  const float denom = sqrtf(v) / k.bc2_sqrt + k.eps;
  const float p = a.param[i] + k.neg_step * (m / denom);
  a.param[i] = p;
  return p;
}

__device__ __forceinline__ void adam_store(const FitArgs& a, const AdamK& k, const ParamLayout& L, size_t i, float g,
                                           float* keep) {
  const float p = adam1(a, k, i, g);
  a.packed[packed_of_param(L, i)] = p;
  if (keep) *keep = p;
}

constexpr int XP = IN_MAX + 1;     // LDS pitch of [row][k] images

__global__ __launch_bounds__(FIT_THREADS) void fit_l1_kernel(FitArgs a) {
  __shared__ float xl[MAX_BATCH * XP];        // standardised rows [r][k]
  __shared__ float dz[MAX_BATCH * 17];        // dZ1 of the previous minibatch [r][unit]
  __shared__ float w1s[16 * XP], b1s[16];     // this workgroup's W1 rows / b1 (current values)
  __shared__ double s_mean[IN_MAX], s_sd[IN_MAX], part[8 * IN_MAX];   // part: the column sums' row-strided partials
  __shared__ int rows_s[MAX_BATCH];
  const ParamLayout L = param_layout(a.in_dim, 1);
  const int tid = threadIdx.x, j0 = blockIdx.x * 16, in_dim = a.in_dim;
  const float* ws = a.ws;

  if (a.r_prev > 0) {   // ---- close minibatch b-1 for units j0 .. j0 + 15
    const int R = a.r_prev;
    const float* xsp = ws + WS_XS + (size_t)a.par_prev * MAX_BATCH * IN_MAX;
    for (int e = tid; e < R * 16; e += FIT_THREADS) {
      const int r = e >> 4, c = e & 15;
      const size_t o = (size_t)r * H1 + j0 + c;
      float s = ws[WS_DH1 + o];
      for (int p = 1; p < NS2; ++p) s += ws[WS_DH1 + (size_t)p * MAX_BATCH * H1 + o];
      dz[r * 17 + c] = ws[WS_H1 + o] <= 0.f ? 0.f : s;        // relu backward on the output (threshold_backward)
    }
    for (int e = tid; e < R * in_dim; e += FIT_THREADS) {
      const int r = e / in_dim, k = e - r * in_dim;
      xl[r * XP + k] = xsp[r * IN_MAX + k];
    }
    __syncthreads();
    for (int e = tid; e < 16 * in_dim + 16; e += FIT_THREADS) {
      if (e < 16 * in_dim) {
        const int c = e / in_dim, k = e - c * in_dim;
        float g = 0.f;
        for (int r = 0; r < R; ++r) g = fmaf(dz[r * 17 + c], xl[r * XP + k], g);
        adam_store(a, a.ad_prev, L, L.w1 + (size_t)(j0 + c) * in_dim + k, g, &w1s[c * XP + k]);
      } else {
        const int c = e - 16 * in_dim;
        float g = 0.f;
        for (int r = 0; r < R; ++r) g += dz[r * 17 + c];
        adam_store(a, a.ad_prev, L, L.b1 + j0 + c, g, &b1s[c]);
      }
    }
    if (blockIdx.x == 0) {   // the output layer's step (its gradients came from launch C)
      for (int e = tid; e <= H2; e += FIT_THREADS)
        adam_store(a, a.ad_prev, L, e < H2 ? L.w3 + e : L.b3, ws[WS_G3 + e], nullptr);
    }
  } else {
    for (int e = tid; e < 16 * in_dim; e += FIT_THREADS) {
      const int c = e / in_dim, k = e - c * in_dim;
      w1s[c * XP + k] = a.param[L.w1 + (size_t)(j0 + c) * in_dim + k];
    }
    if (tid < 16) b1s[tid] = a.param[L.b1 + j0 + tid];
  }
  __syncthreads();
  if (a.r_cur <= 0) return;

  // ---- minibatch b: Standardizer.update_mean_std then forward (networks.py:68-81).  The rows are gathered into LDS
  // in one parallel pass; the column sums are four row-strided partial chains (rows g, g + 4, ...) added in order g.
  // (oly_fit::fold_chains' order; that one stores the sums, these stay in registers.)
  const int R = a.r_cur;
  if (tid < R) rows_s[tid] = row_at(a, tid);
  __syncthreads();
  for (int e = tid; e < R * in_dim; e += FIT_THREADS) {
    const int r = e / in_dim, k = e - r * in_dim;
    xl[r * XP + k] = a.x[(size_t)rows_s[r] * in_dim + k];
  }
  __syncthreads();
  {
    const int k = tid & (IN_MAX - 1), grp = tid >> 6;
    double s = 0.0, ss = 0.0;
    if (k < in_dim)
      for (int r = grp; r < R; r += 4) {
        const double v = xl[r * XP + k];
        s += v;
        ss += v * v;
      }
    part[grp * IN_MAX + k] = s;
    part[(4 + grp) * IN_MAX + k] = ss;
  }
  __syncthreads();
  if (tid < in_dim) {
    const double s = ((part[tid] + part[IN_MAX + tid]) + part[2 * IN_MAX + tid]) + part[3 * IN_MAX + tid];
    const double ss = ((part[4 * IN_MAX + tid] + part[5 * IN_MAX + tid]) + part[6 * IN_MAX + tid]) + part[7 * IN_MAX + tid];
    // the same expressions as launch C's update of colstats, so the values used here are the ones it stores
    const double cnt = a.colstats[tid] + (double)R + 1e-2;
    const double mean = (a.colstats[in_dim + tid] + s) / cnt;
    s_mean[tid] = mean;
    s_sd[tid] = sqrt(fmax((a.colstats[2 * in_dim + tid] + ss + 1e-2) / cnt - mean * mean, 1e-2));
    if (blockIdx.x == 0) {
      double* d = reinterpret_cast<double*>(a.ws + WS_DELTA);
      d[tid] = s;
      d[IN_MAX + tid] = ss;
    }
  }
  __syncthreads();
  float* xs_cur = a.ws + WS_XS + (size_t)a.par_cur * MAX_BATCH * IN_MAX;
  for (int e = tid; e < R * in_dim; e += FIT_THREADS) {
    const int r = e / in_dim, k = e - r * in_dim;
    const float v = (float)(((double)xl[r * XP + k] - s_mean[k]) / s_sd[k]);
    xl[r * XP + k] = v;
    if (blockIdx.x == 0) xs_cur[r * IN_MAX + k] = v;
  }
  __syncthreads();
  for (int e = tid; e < R * 16; e += FIT_THREADS) {
    const int r = e >> 4, c = e & 15;
    float z = 0.f;
    for (int k = 0; k < in_dim; ++k) z = fmaf(xl[r * XP + k], w1s[c * XP + k], z);
    z += b1s[c];
    a.ws[WS_H1 + (size_t)r * H1 + j0 + c] = (z > 0.f || z != z) ? z : 0.f;
  }
}

// grid (16 slices of 16 layer-2 units, row blocks of 64)
__global__ __launch_bounds__(FIT_THREADS) void fit_l2_kernel(FitArgs a) {
  __shared__ float hs[64 * XP], w2s[16 * XP];
  const ParamLayout L = param_layout(a.in_dim, 1);
  const int tid = threadIdx.x, n0 = blockIdx.x * 16, r0 = blockIdx.y * 64;
  const int rows = min(64, a.r_cur - r0);
  const int r = tid & 63, cg = tid >> 6;           // row, group of four units
  const float* h1 = a.ws + WS_H1;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int kc = 0; kc < H1; kc += 64) {
    for (int e = tid; e < 64 * 64; e += FIT_THREADS) {
      const int rr = e >> 6, kk = e & 63;
      hs[rr * XP + kk] = rr < rows ? h1[(size_t)(r0 + rr) * H1 + kc + kk] : 0.f;
    }
    for (int e = tid; e < 16 * 64; e += FIT_THREADS) {
      const int nn = e >> 6, kk = e & 63;
      w2s[nn * XP + kk] = a.param[L.w2 + (size_t)(n0 + nn) * H1 + kc + kk];
    }
    __syncthreads();
    for (int kk = 0; kk < 64; ++kk) {
      const float h = hs[r * XP + kk];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = fmaf(h, w2s[(4 * cg + t) * XP + kk], acc[t]);
    }
    __syncthreads();
  }
  if (r < rows) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int n = n0 + 4 * cg + t;
      const float z = acc[t] + a.param[L.b2 + n];
      a.ws[WS_H2 + (size_t)(r0 + r) * H2 + n] = (z > 0.f || z != z) ? z : 0.f;
    }
  }
}

// grid (16 slices of 16 layer-2 units, 4 slices of 128 layer-1 units)
constexpr int KS = 128, KP = KS + 1;
__global__ __launch_bounds__(FIT_THREADS) void fit_bwd_kernel(FitArgs a) {
  __shared__ float tile[MAX_BATCH * 33];       // H2 chunks [256][32] (pitch 33) for y, then H1 chunks [64][128] (pitch KP)
  static_assert(64 * KP <= MAX_BATCH * 33, "the H1 chunks fit the tile");
  __shared__ float w3s[H2], dys[MAX_BATCH], dz2[MAX_BATCH * 17], w2t[16 * KP];
  __shared__ double lsum[FIT_THREADS];
  const ParamLayout L = param_layout(a.in_dim, 1);
  const int tid = threadIdx.x, n0 = blockIdx.x * 16, k0 = blockIdx.y * KS, R = a.r_cur;
  const bool first = blockIdx.x == 0 && blockIdx.y == 0;
  const float* h1 = a.ws + WS_H1;
  const float* h2 = a.ws + WS_H2;
  w3s[tid] = a.param[L.w3 + tid];
  for (int e = tid; e < 16 * KS; e += FIT_THREADS) {          // the OLD W2 tile (dH1 is taken through it)
    const int c = e / KS, kk = e - c * KS;
    w2t[c * KP + kk] = a.param[L.w2 + (size_t)(n0 + c) * H1 + k0 + kk];
  }
  // ---- y = H2 w3 + b3 for every row: one chain over k < 256 (row tid)
  float y = 0.f;
  for (int kc = 0; kc < H2; kc += 32) {
    __syncthreads();
    for (int e = tid; e < R * 32; e += FIT_THREADS) {
      const int rr = e >> 5, kk = e & 31;
      tile[rr * 33 + kk] = h2[(size_t)rr * H2 + kc + kk];
    }
    __syncthreads();
    if (tid < R)
      for (int kk = 0; kk < 32; ++kk) y = fmaf(tile[tid * 33 + kk], w3s[kc + kk], y);
  }
  double d2 = 0.0;
  if (tid < R) {
    y += a.param[L.b3];
    const float d = y - a.vt[row_at(a, tid)];
    dys[tid] = (2.0f / (float)R) * d;     // mse_loss backward: (2 / N) (y - t) * grad_out
    d2 = (double)d * (double)d;
  }
  lsum[tid] = d2;
  __syncthreads();
  if (first && tid == 0) {
    double s = 0.0;
    for (int i = 0; i < R; ++i) s += lsum[i];
    a.loss[0] = s / R;
  }
  // ---- dZ2 of this workgroup's 16 units
  for (int e = tid; e < R * 16; e += FIT_THREADS) {
    const int r = e >> 4, c = e & 15;
    const float dh = dys[r] * w3s[n0 + c];
    dz2[r * 17 + c] = h2[(size_t)r * H2 + n0 + c] <= 0.f ? 0.f : dh;
  }
  __syncthreads();
  // ---- dH1 partial over this slice's 16 units for columns k0 .. k0 + 127 (old W2)
  {
    const int kk = tid & (KS - 1);
    float* out = a.ws + WS_DH1 + (size_t)blockIdx.x * MAX_BATCH * H1 + k0 + kk;
    for (int r = tid >> 7; r < R; r += 2) {
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < 16; ++c) s = fmaf(dz2[r * 17 + c], w2t[c * KP + kk], s);
      out[(size_t)r * H1] = s;
    }
  }
  // ---- dW2 [16 units][128 columns]: thread (kk, 8 units) chains over the rows
  const int kk = tid & (KS - 1), c0 = (tid >> 7) * 8;
  float g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int rc = 0; rc < R; rc += 64) {
    const int rows = min(64, R - rc);
    __syncthreads();
    for (int e = tid; e < rows * KS; e += FIT_THREADS) {
      const int rr = e / KS, k = e - rr * KS;
      tile[rr * KP + k] = h1[(size_t)(rc + rr) * H1 + k0 + k];
    }
    __syncthreads();
    for (int rr = 0; rr < rows; ++rr) {
      const float h = tile[rr * KP + kk];
#pragma unroll
      for (int t = 0; t < 8; ++t) g[t] = fmaf(dz2[(rc + rr) * 17 + c0 + t], h, g[t]);
    }
  }
#pragma unroll
  for (int t = 0; t < 8; ++t) adam_store(a, a.ad_cur, L, L.w2 + (size_t)(n0 + c0 + t) * H1 + k0 + kk, g[t], nullptr);
  if (blockIdx.y == 0 && tid < 16) {
    float gb = 0.f, gw = 0.f;
    for (int r = 0; r < R; ++r) {
      gb += dz2[r * 17 + tid];
      gw = fmaf(dys[r], h2[(size_t)r * H2 + n0 + tid], gw);
    }
    adam_store(a, a.ad_cur, L, L.b2 + n0 + tid, gb, nullptr);
    a.ws[WS_G3 + n0 + tid] = gw;                              // W3 / b3 are stepped by the next launch A
  }
  if (first && tid == 0) {
    float gb = 0.f;
    for (int r = 0; r < R; ++r) gb += dys[r];
    a.ws[WS_G3 + H2] = gb;
  }
  if (first && tid < a.in_dim) {          // Standardizer.update_mean_std: the running sums += this minibatch
    const double* d = reinterpret_cast<const double*>(a.ws + WS_DELTA);
    a.colstats[tid] = a.colstats[tid] + (double)R;
    a.colstats[a.in_dim + tid] = a.colstats[a.in_dim + tid] + d[tid];
    a.colstats[2 * a.in_dim + tid] = a.colstats[2 * a.in_dim + tid] + d[IN_MAX + tid];
  }
}

bool ilmlp_shape_ok(int in_dim, int h1, int h2, int out_dim) {
  return in_dim > 0 && in_dim <= IN_MAX && h1 == H1 && h2 == H2 && out_dim > 0 && out_dim <= OUT_MAX;
}

}  // namespace

extern "C" int64_t oly_ilmlp_packed_floats(int in_dim, int h1, int h2, int out_dim) {
  return ilmlp_shape_ok(in_dim, h1, h2, out_dim) ? (int64_t)P_TOTAL : -1;
}

extern "C" int oly_ilmlp_pack(oly_ctx* ctx, int in_dim, int h1, int h2, int out_dim, const float* w1, const float* b1,
                              const float* w2, const float* b2, const float* w3, const float* b3, float* packed,
                              oly_stream stream) {
  if (!ctx) return OLY_EINVAL;
  if (!ilmlp_shape_ok(in_dim, h1, h2, out_dim))
    OLY_FAIL(ctx, OLY_ERANGE, "oly_ilmlp_pack: supported shape is in <= %d -> %d -> %d -> out <= %d (got %d, %d, %d, %d)",
             IN_MAX, H1, H2, OUT_MAX, in_dim, h1, h2, out_dim);
  if (!w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !packed) OLY_FAIL(ctx, OLY_EINVAL, "oly_ilmlp_pack: NULL pointer");
  if ((reinterpret_cast<uintptr_t>(packed) & 15) != 0) OLY_FAIL(ctx, OLY_EINVAL, "oly_ilmlp_pack: packed must be 16-byte aligned");
  hipLaunchKernelGGL(ilmlp_pack_kernel, dim3(128), dim3(256), 0, oly_s(stream), in_dim, out_dim, w1, b1, w2, b2, w3, b3,
                     packed);
  OLY_LAUNCH_CHECK(ctx, "ilmlp_pack_kernel");
  return OLY_OK;
}

extern "C" int oly_ilmlp_forward(oly_ctx* ctx, int64_t N, int in_dim, int out_dim, int last_act, const float* x,
                                 const double* mean, const double* sd, const double* colstats, const float* packed,
                                 float* y, oly_stream stream) {
  if (!ctx) return OLY_EINVAL;
  if (N < 0 || !ilmlp_shape_ok(in_dim, H1, H2, out_dim) || (last_act != OLY_ACT_IDENTITY && last_act != OLY_ACT_TANH))
    OLY_FAIL(ctx, OLY_ERANGE, "oly_ilmlp_forward: bad N / shape / activation (N %ld, in %d, out %d, act %d)", (long)N,
             in_dim, out_dim, last_act);
  if (N == 0) return OLY_OK;
  if (!x || !packed || !y || (!mean) != (!sd) || (mean && colstats))
    OLY_FAIL(ctx, OLY_EINVAL, "oly_ilmlp_forward: NULL x / packed / y, or not exactly one of mean+std / colstats / none");
  if ((reinterpret_cast<uintptr_t>(packed) & 15) != 0) OLY_FAIL(ctx, OLY_EINVAL, "oly_ilmlp_forward: packed must be 16-byte aligned");
  const FwdArgs a{(long)N, in_dim, out_dim, last_act, in_dim, x, nullptr, mean, sd, colstats, packed, y, nullptr};
  // 16-row tiles while the 32-row tiles would leave CUs without a second workgroup (as K11)
  const long slots = 2L * (ctx->num_cu > 0 ? ctx->num_cu : 256);
  if ((N + 31) / 32 < slots) return launch_forward<1>(ctx, a, stream);
  return launch_forward<2>(ctx, a, stream);
}

extern "C" int64_t oly_il_critic_fit_ws_floats(int batch, int in_dim) {
  if (batch <= 0 || batch > MAX_BATCH || in_dim <= 0 || in_dim > IN_MAX) return -1;
  return (int64_t)WS_TOTAL;
}

extern "C" int oly_il_critic_fit_epoch(oly_ctx* ctx, const oly_il_critic_fit* f, const int32_t* perm, int n_rows,
                                       int batch, oly_stream stream) {
  if (!ctx) return OLY_EINVAL;
  if (!f || !perm) OLY_FAIL(ctx, OLY_EINVAL, "oly_il_critic_fit_epoch: NULL argument");
  if (n_rows < 0 || oly_il_critic_fit_ws_floats(batch, f->in_dim) < 0)
    OLY_FAIL(ctx, OLY_ERANGE, "oly_il_critic_fit_epoch: supported: 0 < batch <= %d, 0 < in_dim <= %d (got n %d, batch %d, in %d)",
             MAX_BATCH, IN_MAX, n_rows, batch, f->in_dim);
  if (!f->x || !f->v_target || !f->colstats || !f->param || !f->exp_avg || !f->exp_avg_sq || !f->packed || !f->ws ||
      !f->loss_out)
    OLY_FAIL(ctx, OLY_EINVAL, "oly_il_critic_fit_epoch: NULL pointer in the argument block");
  if (f->ws_floats < (int64_t)WS_TOTAL || (reinterpret_cast<uintptr_t>(f->ws) & 15) != 0)
    OLY_FAIL(ctx, OLY_EINVAL, "oly_il_critic_fit_epoch: ws must be 16-byte aligned and hold %ld floats", (long)WS_TOTAL);
  const int nb = (n_rows + batch - 1) / batch;
  if (f->step < 0 || (long)f->step + nb > 0x7fffffffL) OLY_FAIL(ctx, OLY_EINVAL, "oly_il_critic_fit_epoch: bad step");
  if (nb == 0) return OLY_OK;
  FitArgs a{};
  a.n_rows = n_rows;
  a.in_dim = f->in_dim;
  a.x = f->x;
  a.vt = f->v_target;
  a.colstats = f->colstats;
  a.param = f->param;
  a.m = f->exp_avg;
  a.v = f->exp_avg_sq;
  a.packed = f->packed;
  a.ws = f->ws;
  for (int b = 0; b <= nb; ++b) {
    a.r_prev = b > 0 ? min(batch, n_rows - (b - 1) * batch) : 0;
    a.r_cur = b < nb ? min(batch, n_rows - b * batch) : 0;
    a.par_prev = (b + 1) & 1;
    a.par_cur = b & 1;
    a.perm = perm + (size_t)min(b, nb - 1) * batch;
    a.loss = f->loss_out + min(b, nb - 1);
    a.ad_prev = a.ad_cur;
    a.ad_cur = oly_fit::adam_scalars(f->beta1, f->beta2, f->eps, f->lr, (long)f->step + b + 1);
    hipLaunchKernelGGL(fit_l1_kernel, dim3(H1 / 16), dim3(FIT_THREADS), 0, oly_s(stream), a);
    if (b == nb) break;
    hipLaunchKernelGGL(fit_l2_kernel, dim3(H2 / 16, (a.r_cur + 63) / 64), dim3(FIT_THREADS), 0, oly_s(stream), a);
    hipLaunchKernelGGL(fit_bwd_kernel, dim3(H2 / 16, H1 / KS), dim3(FIT_THREADS), 0, oly_s(stream), a);
  }
  OLY_LAUNCH_CHECK(ctx, "il critic fit kernels");
  return OLY_OK;
}
