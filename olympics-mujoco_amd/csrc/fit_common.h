// Pieces that the minibatch fits share: K15 (csrc/k15_disc_fit.hip, the VAIL discriminator), K16 (csrc/k16_il_critic.hip,
// the imitation critic), K18 (csrc/k18_gail_disc.hip, GAIL's discriminator), K24 (csrc/k24_bc_fit.hip, behavioural
// cloning) and K26 (csrc/k26_iq_critic.hip, the soft-Q critic); oly_ppo_adam_step (K14) takes its bias corrections from
// adam_scalars.  What only K18, K24 and K26 share (one network, one two-launch design) is one level up, in ilmlp_fit.h.
// The order of every addition here is what makes a fit deterministic and what the tests
// pin: a change to it is a change to all of its users.  The functions that take an argument block `a` are templates
// over the kernels' own FitArgs (the networks differ; the members named here do not).  The device functions are written
// so that their users compile to the code they had with their own copies; how an index is spelt can matter to that.
#pragma once
#include <cmath>

#include "disc_common.h"
#include "oly_common.h"

namespace oly_fit {
using oly_disc::MAX_IN;          // widest input, the pitch of every statistics array
constexpr int THREADS = 256;     // the workgroup of every kernel that calls fold_chains, stats_slice or loss_tree
constexpr int NSP = 16;          // slices of the statistics partials (fixed: their sum order does not depend on a grid)

// ---- Adam
// The scalars of one torch.optim.Adam step (amsgrad off).  Weight decay is not among them: K16 has none, and its
// argument block holds two of these.
struct AdamK {
  float w1, beta2, w2, eps, neg_step, bc2_sqrt;
};

// the step-dependent scalars in fp64 as torch's default (non-capturable) Adam forms them, narrowed to float
inline AdamK adam_scalars(float beta1, float beta2, float eps, float lr, long step) {
  const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
  AdamK k;
  k.w1 = 1.0f - beta1;
  k.beta2 = beta2;
  k.w2 = 1.0f - beta2;
  k.eps = eps;
  k.neg_step = (float)(-((double)lr / bc1));
  k.bc2_sqrt = (float)sqrt(bc2);
  return k;
}

// torch.optim.Adam.step on element i of a.param / a.m / a.v, float32 in K14's order (adam_step_kernel); weight decay
// `wd` as L2 on the gradient.  Returns the stepped parameter.
template <class A>
__device__ __forceinline__ float adam1(const A& a, const AdamK& k, float wd, size_t i, float g) {
  float p = a.param[i], m = a.m[i], v = a.v[i];
  if (wd != 0.f) g = fmaf(wd, p, g);
  m = m + (g - m) * k.w1;
  v = v * k.beta2 + (k.w2 * g) * g;
  a.m[i] = m;
  a.v[i] = v;
  const float denom = sqrtf(v) / k.bc2_sqrt + k.eps;
  p = p + k.neg_step * (m / denom);
  a.param[i] = p;
  return p;
}
template <class A>
__device__ __forceinline__ float adam1(const A& a, size_t i, float g) {
  return adam1(a, a.ad, a.wd, i, g);
}

// ---- indexing
// The B operand of a data gradient dX = dY W (a sum over the layer's OUTPUT index n, N outputs):
//   T[tile][group g][lane][q] = W[n = 16 g + 4 q + (lane >> 4)][k = 16 tile + (lane & 15)]
__device__ __forceinline__ size_t pt_index(int N, int n, int k) {
  const int lane = (k & 15) | ((n & 3) << 4), q = (n >> 2) & 3;
  return ((size_t)((k >> 4) * (N / 16) + (n >> 4)) * 64 + lane) * 4 + q;
}

// the data row at position pos of a.perm, clamped for memory safety only: perm is a permutation of [0, n_rows)
template <class A>
__device__ __forceinline__ int row_at(const A& a, long pos) {
  const int i = a.perm[pos];
  return i < 0 ? 0 : i >= a.n_rows ? a.n_rows - 1 : i;
}

// ---- the Standardizer's column sums
// A 256-thread workgroup's thread (column k = tid & 63, chain g = tid >> 6) brings the sum and the sum of squares of its
// row-strided chain (rows g, g + 4, ...): they meet in part [8][MAX_IN] and, after a barrier, threads tid < cols add
// them in order g into out [2][MAX_IN].  Every thread of the workgroup calls it.
__device__ __forceinline__ void fold_chains(double sum, double sq, int cols, double* part, double* out) {
  const int tid = threadIdx.x, k = tid & (MAX_IN - 1), grp = tid >> 6;
  part[grp * MAX_IN + k] = sum;
  part[(4 + grp) * MAX_IN + k] = sq;
  __syncthreads();
  if (tid < cols) {
    out[tid] = ((part[tid] + part[MAX_IN + tid]) + part[2 * MAX_IN + tid]) + part[3 * MAX_IN + tid];
    out[MAX_IN + tid] = ((part[4 * MAX_IN + tid] + part[5 * MAX_IN + tid]) + part[6 * MAX_IN + tid]) + part[7 * MAX_IN + tid];
  }
}

// Statistics partial `s` (at a.ws + a.W.statp) of the minibatch at perm[off .. off + R): its rows split into NSP slices;
// in each, the four chains over the gathered rows of x | x2.  Every thread of the workgroup calls it.
template <class A>
__device__ void stats_slice(const A& a, long off, int R, int s, double* part) {
  const int tid = threadIdx.x, k = tid & (MAX_IN - 1), grp = tid >> 6;
  const int per = (R + NSP - 1) / NSP, r0 = s * per, r1 = min(R, r0 + per);
  double sum = 0.0, ss = 0.0;
  if (k < a.ds || (k < a.in_dim && a.std2))
    for (int r = r0 + grp; r < r1; r += 4) {
      const size_t row = row_at(a, off + r);
      const double v = k < a.ds ? a.x[row * a.ds + k] : a.x2[row * a.stride2 + (k - a.ds)];
      sum += v;
      ss += v * v;
    }
  fold_chains(sum, ss, a.in_dim, part, reinterpret_cast<double*>(a.ws + a.W.statp) + (size_t)s * 2 * MAX_IN);
}

// ---- the tail of a weights kernel (launch B of K15, K18, K24 and K26)
// the bias gradient of the tile's column tid < 16: the column sums of delta in bred [4 waves][64 lanes], lane groups
// then waves in order
__device__ __forceinline__ float bias_colsum(const float* bred, int tid) {
  float gb = 0.f;
  for (int w = 0; w < 4; ++w) {
    const float s = ((bred[w * 64 + tid] + bred[w * 64 + 16 + tid]) + bred[w * 64 + 32 + tid]) + bred[w * 64 + 48 + tid];
    gb = w == 0 ? s : gb + s;
  }
  return gb;
}

// The minibatch's two loss sums from launch A's per-tile partials lp [tiles][2], by a fixed tree (the same order on
// every run) in dred [2][THREADS]: they end in dred[0] and dred[THREADS].  Every thread of the workgroup calls it.
__device__ __forceinline__ void loss_tree(int tiles, const double* lp, double* dred) {
  const int tid = threadIdx.x;
  dred[tid] = tid < tiles ? lp[2 * tid] : 0.0;
  dred[THREADS + tid] = tid < tiles ? lp[2 * tid + 1] : 0.0;
  __syncthreads();
  for (int s = THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
      dred[tid] += dred[tid + s];
      dred[THREADS + tid] += dred[THREADS + tid + s];
    }
    __syncthreads();
  }
}

// colstats += the minibatch's R rows: launch A left their column sums at a.ws + a.W.delta, the states' in the first ds
// columns and (std2) the next states' in the following ds.  Every thread calls it; threads tid < ds do it.
template <class A>
__device__ __forceinline__ void colstats_add(const A& a, int R) {
  const int tid = threadIdx.x;
  if (tid < a.ds) {
    const double* d = reinterpret_cast<const double*>(a.ws + a.W.delta);
    const int ds = a.ds, tq = MAX_IN + tid;     // tq: column tid of the sums of squares
    double cnt = a.colstats[tid] + (double)R;
    double sum = a.colstats[ds + tid] + d[tid];
    double sq = a.colstats[2 * ds + tid] + d[tq];
    if (a.std2) {       // the minibatch's next states, taken in after its states
      cnt += (double)R;
      sum += d[ds + tid];
      sq += d[tq + ds];
    }
    a.colstats[tid] = cnt;
    a.colstats[ds + tid] = sum;
    a.colstats[2 * ds + tid] = sq;
  }
}

// ---- the host side of oly_disc_fit_epoch_pair and oly_gail_disc_fit_epoch_pair
// `name` is the states-only entry point's, which the messages have always carried.
// What comes before the argument block's pointers are looked at: the pair, the shape (shape_ok; K15 answers
// OLY_ERANGE, K18 OLY_EINVAL), n_plcy.
inline int refuse_shape(oly_ctx* ctx, const char* name, const oly_disc_pair* pair, int in_dim, bool shape_ok, int shape_code,
                        int max_batch, int n_rows, int batch, int n_plcy) {
  if (pair) {
    const char* why = in_dim - pair->d2 <= 0 ? "d2 leaves the first part no column" : oly_disc::pair_error(pair, in_dim - pair->d2);
    if (!why && pair->mask2) why = "the fit takes the second part already gathered (mask2 NULL)";
    if (why) OLY_FAIL(ctx, OLY_EINVAL, "%s_pair: %s (in_dim %d, d2 %d)", name, why, in_dim, pair->d2);
  }
  if (n_rows < 0 || !shape_ok)
    OLY_FAIL(ctx, shape_code, "%s: supported: 0 < batch <= %d, 0 < in_dim <= %d (got n %d, batch %d, in %d)", name, max_batch,
             MAX_IN, n_rows, batch, in_dim);
  if (n_plcy < 0 || n_plcy > n_rows) OLY_FAIL(ctx, OLY_EINVAL, "%s: n_plcy %d outside [0, %d]", name, n_plcy, n_rows);
  return OLY_OK;
}

// ... and after: the workspace's size, the alignment of ws and packed, the range of the nb steps from `step`
inline int refuse_buffers(oly_ctx* ctx, const char* name, int64_t ws_floats, size_t ws_need, const float* ws,
                          const float* packed, int step, int nb) {
  if (ws_floats < (int64_t)ws_need || (reinterpret_cast<uintptr_t>(ws) & 15) != 0 || (reinterpret_cast<uintptr_t>(packed) & 15) != 0)
    OLY_FAIL(ctx, OLY_EINVAL, "%s: ws (%ld floats) and packed must be 16-byte aligned", name, (long)ws_need);
  if (step < 0 || (long)step + nb > 0x7fffffffL) OLY_FAIL(ctx, OLY_EINVAL, "%s: bad step", name);
  return OLY_OK;
}

// the columns of the two sources: x [n_rows, ds] | the first d2 of x2 [n_rows, stride2] (none without a pair)
template <class A>
inline void set_pair_cols(A& a, int in_dim, const oly_disc_pair* pair) {
  a.in_dim = in_dim;
  a.ds = in_dim - (pair ? pair->d2 : 0);
  if (pair) {
    a.d2 = pair->d2;
    a.std2 = pair->standardise != 0;
    a.stride2 = pair->stride2;
    a.x2 = pair->x2;
  }
}

// minibatch b of nb: its rows are perm[off .. off + R), those of b + 1 perm[off_next .. off_next + Rn) (Rn 0: none)
template <class A>
inline void set_minibatch(A& a, int b, int nb, int n_rows, int batch) {
  a.off = (long)b * batch;
  a.R = min(batch, n_rows - b * batch);
  a.off_next = a.off + a.R;
  a.Rn = b + 1 < nb ? min(batch, n_rows - (b + 1) * batch) : 0;
}

}  // namespace oly_fit
