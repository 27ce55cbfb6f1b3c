// K20: the agent's iteration diagnostics (_logging_sw, imitation_lib/imitation/gail_TRPO.py:163, 251-272), which every run
// of the reference's launcher executes at the end of a trained iteration because it passes a SummaryWriter:
//
//   vf_loss        F.mse_loss(self._V(x), v_target)                                   :254-256   the critic's forward
//   entropy        self.policy.entropy(x)                                             :258       no forward
//   kl             mean kl_divergence(old_pol_dist, self.policy.distribution(x))      :259-262   the policy's forward
//   EpTrueRewMean  np.mean(compute_J(dataset))                                        :263       the environment's reward
//   EpRewMean      np.mean(compute_J(new_data_set))                                   :264       the reward trained on
//   EpLenMean      int(np.round(np.mean(compute_episodes_length(dataset))))           :265
//
// Both forwards go through Standardizer.forward (networks.py:68-81), which adds the batch to the running sums first: with
// S the live statistics and c the batch's (count, sum, sumsq), the critic standardises with S + c, the policy with
// S + 2c, and the live statistics end at S + 2c.
//
//   episode_kernel      a lane per environment walks its column of [T, N] in step order (coalesced across N): float64
//                       returns sum gamma^k r_k per episode, lengths at `last`; an episode still open at the end of the
//                       column counts among the returns and not among the lengths.  One wave per workgroup, wave
//                       shuffles, one slot per workgroup.
//   episode_finish      adds the slots in block order and forms the means.
//   iter_chain_kernel   S + c and S + 2c by sequential float64 addition; the second replaces colstats.
//   forwards            K16's launcher (oly_ilmlp_forward, kernels untouched) on chunks of at most 16 384 rows.
//   iter_metric_kernel  the float32 row terms of the squared error or of the KL, float64 partials per thread, wave
//                       shuffles, LDS in wave order, one slot per workgroup.
//   iter_finish_kernel  adds the slots in block order within chunk order and writes the scalars.
// No atomics, no scratch, no allocation, no host synchronisation; two runs give identical bits.
#include "ilmlp_common.h"
#include "oly_common.h"

namespace {

using oly_ilmlp::IN_MAX;
using oly_ilmlp::OUT_MAX;

constexpr int EP_THREADS = 64;                  // one wave per workgroup: [400, 4096] is 64 workgroups
constexpr int EP_MAX_BLOCKS = 1024;
constexpr int EP_Q = 5;                         // sum J, sum J2, returns, sum lengths, lengths
constexpr int THREADS = 256;
constexpr int CHUNK = 16384;                    // rows per forward launch
constexpr int CHUNK_BLOCKS = CHUNK / THREADS;   // partial slots per chunk
constexpr int SW = 3 * IN_MAX;                  // doubles reserved per statistics block ([3, D] dense inside)

template <typename R>
__global__ __launch_bounds__(EP_THREADS) void episode_kernel(int T, int N, double gamma, const R* __restrict__ rew,
                                                            const float* __restrict__ rew2,
                                                            const uint8_t* __restrict__ last, double* __restrict__ slots) {
  double q[EP_Q] = {0.0, 0.0, 0.0, 0.0, 0.0};
  const long stride = (long)gridDim.x * EP_THREADS;
  for (long e = (long)blockIdx.x * EP_THREADS + threadIdx.x; e < N; e += stride) {
    double j1 = 0.0, j2 = 0.0, g = 1.0;
    int len = 0;
    for (int t = 0; t < T; ++t) {
      const size_t i = (size_t)t * (size_t)N + (size_t)e;
      j1 += g * (double)rew[i];
      if (rew2) j2 += g * (double)rew2[i];
      g *= gamma;
      ++len;
      if (last[i]) {
        q[0] += j1;
        q[1] += j2;
        q[2] += 1.0;
        q[3] += (double)len;
        q[4] += 1.0;
        j1 = j2 = 0.0;
        g = 1.0;
        len = 0;
      }
    }
    if (len > 0) {      // compute_J's `i == len(dataset) - 1`: the open episode is a return, not a length
      q[0] += j1;
      q[1] += j2;
      q[2] += 1.0;
    }
  }
#pragma unroll
  for (int i = 0; i < EP_Q; ++i) {
    const double v = wave_sum(q[i]);
    if (threadIdx.x == 0) slots[(size_t)blockIdx.x * EP_Q + i] = v;
  }
}

// out [OLY_EPISODE_STATS]: mean return, mean return of the second block, mean length (NaN without a completed episode),
// returns, lengths, and the three sums
__global__ __launch_bounds__(64) void episode_finish_kernel(int nblocks, int two, const double* __restrict__ slots,
                                                           double* __restrict__ out) {
  __shared__ double S[EP_Q];
  const int tid = threadIdx.x;
  if (tid < EP_Q) {
    double s = 0.0;
    for (int b = 0; b < nblocks; ++b) s += slots[(size_t)b * EP_Q + tid];
    S[tid] = s;
  }
  __syncthreads();
  if (tid != 0) return;
  out[0] = S[0] / S[2];
  out[1] = two ? S[1] / S[2] : 0.0;
  out[2] = S[3] / S[4];        // 0 / 0 = NaN when no episode was completed
  out[3] = S[2];
  out[4] = S[4];
  out[5] = S[0];
  out[6] = two ? S[1] : 0.0;
  out[7] = S[3];
}

inline int ep_blocks(int N) {
  const long b = ((long)N + EP_THREADS - 1) / EP_THREADS;
  return (int)(b < EP_MAX_BLOCKS ? b : EP_MAX_BLOCKS);
}

int run_episode_stats(oly_ctx* ctx, const char* who, int T, int N, int rew_f64, double gamma, const void* rew,
                      const float* rew2, const uint8_t* last, double* slots, double* out, oly_stream stream) {
  if (T < 1 || N < 1 || (long)T * (long)N > 2147483647L)
    OLY_FAIL(ctx, OLY_EINVAL, "%s: supported: T >= 1, N >= 1, T N < 2^31 (got T %d, N %d)", who, T, N);
  if (!rew || !last || !out || !slots) OLY_FAIL(ctx, OLY_EINVAL, "%s: NULL reward / last / out", who);
  if (!(gamma >= 0.0 && gamma <= 1.0)) OLY_FAIL(ctx, OLY_EINVAL, "%s: gamma %g outside [0, 1]", who, gamma);
  const int nb = ep_blocks(N);
  if (rew_f64)
    hipLaunchKernelGGL(episode_kernel<double>, dim3(nb), dim3(EP_THREADS), 0, oly_s(stream), T, N, gamma,
                       static_cast<const double*>(rew), rew2, last, slots);
  else
    hipLaunchKernelGGL(episode_kernel<float>, dim3(nb), dim3(EP_THREADS), 0, oly_s(stream), T, N, gamma,
                       static_cast<const float*>(rew), rew2, last, slots);
  hipLaunchKernelGGL(episode_finish_kernel, dim3(1), dim3(64), 0, oly_s(stream), nb, rew2 ? 1 : 0, slots, out);
  OLY_LAUNCH_CHECK(ctx, "episode statistics kernels");
  return OLY_OK;
}

// workspace (floats): chain [2][SW] f64 (S + c, S + 2c) | c [SW] f64 | episode slots [EP_MAX_BLOCKS][EP_Q] f64 |
// episode out [OLY_EPISODE_STATS] f64 | partial slots [2][chunks * CHUNK_BLOCKS] f64 | y [C, 32] (the chunk's critic
// values, then its policy means), C = min(n, CHUNK) rounded up to four rows
struct WsL {
  size_t chain, c, epslots, ep, slots, y, total;
  int chunks;
};
inline WsL ws_layout(long n) {
  WsL W;
  W.chunks = (int)((n + CHUNK - 1) / CHUNK);
  const size_t C = (size_t)((n < CHUNK ? n : CHUNK) + 3) / 4 * 4;
  W.chain = 0;
  W.c = W.chain + (size_t)2 * SW * 2;
  W.epslots = W.c + (size_t)SW * 2;
  W.ep = W.epslots + (size_t)EP_MAX_BLOCKS * EP_Q * 2;
  W.slots = W.ep + (size_t)OLY_EPISODE_STATS * 2;
  W.y = W.slots + (size_t)2 * W.chunks * CHUNK_BLOCKS * 2;
  W.total = W.y + C * OUT_MAX;
  return W;
}

// One thread per column, the three rows (count, sum, sumsq) each two float64 additions in sequence, as two
// Standardizer.forward calls (and two accumulating oly_col_stats calls) leave them.
__global__ __launch_bounds__(64) void iter_chain_kernel(int D, double* __restrict__ colstats, const double* __restrict__ c,
                                                        double* __restrict__ chain) {
  const int j = threadIdx.x;
  if (j >= D) return;
  for (int r = 0; r < 3; ++r) {
    const int e = r * D + j;
    double s = colstats[e];
    s += c[e];
    chain[e] = s;
    s += c[e];
    chain[SW + e] = s;
    colstats[e] = s;
  }
}

struct MetArgs {
  int kl;                   // 0: squared error of the values; 1: KL(old || new) of the means
  int R, A;
  long row0;                // the chunk's first row in the batch
  const float* y;           // [R] values or [R, A] means of the chunk
  const float* v_target;    // [n]
  const float* mu_old;      // [n, A]
  const float *ls_old, *ls; // [A]
  double* slots;            // [gridDim.x]
};

// Row terms in float32 (F.mse_loss; kl_divergence of two MultivariateNormals with diagonal scale_tril: half_term1 +
// (term2 + term3 - A) / 2, with term2 - A summed as (s_old / s)^2 - 1 per action), summed in float64.
__global__ __launch_bounds__(THREADS) void iter_metric_kernel(MetArgs a) {
  __shared__ double red[THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = blockIdx.x * THREADS + tid;
  double q = 0.0;
  if (r < a.R) {
    const long g = a.row0 + r;
    if (!a.kl) {
      const float d = a.y[r] - a.v_target[g];
      q = (double)(d * d);
    } else {
      const float* mu = a.y + (size_t)r * a.A;
      const float* mo = a.mu_old + (size_t)g * a.A;
      float half = 0.f, t2 = 0.f, t3 = 0.f;
      for (int d = 0; d < a.A; ++d) {
        const float sg = expf(a.ls[d]), so = expf(a.ls_old[d]);
        half += a.ls[d] - a.ls_old[d];
        const float u = so / sg, w = (mu[d] - mo[d]) / sg;
        t2 += u * u - 1.f;      // term2 - A, element by element: A - A never cancels a KL of 1e-3's digits
        t3 += w * w;
      }
      q = (double)(half + 0.5f * (t2 + t3));
    }
  }
  q = wave_sum(q);
  if (lane == 0) red[wave] = q;
  __syncthreads();
  if (tid == 0) a.slots[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

struct FinArgs {
  long n;
  int A, chunks;
  const float* ls;          // [A] the new policy's log_sigma
  const double* slots;      // [2][chunks * CHUNK_BLOCKS]
  const double* ep;         // [OLY_EPISODE_STATS]
  double* out;              // [OLY_ITER_LOG_SCALARS]
};

__global__ __launch_bounds__(64) void iter_finish_kernel(FinArgs a) {
  __shared__ double S[2];
  const int tid = threadIdx.x;
  if (tid < 2) {
    const double* sl = a.slots + (size_t)tid * a.chunks * CHUNK_BLOCKS;
    double s = 0.0;
    for (long c0 = 0, c = 0; c0 < a.n; c0 += CHUNK, ++c) {      // chunks in order, their workgroups in order
      const long rc = a.n - c0 < CHUNK ? a.n - c0 : CHUNK;
      const int nb = (int)((rc + THREADS - 1) / THREADS);
      for (int b = 0; b < nb; ++b) s += sl[(size_t)c * CHUNK_BLOCKS + b];
    }
    S[tid] = s;
  }
  __syncthreads();
  if (tid != 0) return;
  double lsum = 0.0;     // entropy_t: A / 2 log(2 pi e) + sum(log_sigma)
  for (int d = 0; d < a.A; ++d) lsum += (double)a.ls[d];
  a.out[0] = a.ep[0];                                   // EpTrueRewMean
  a.out[1] = a.ep[1];                                   // EpRewMean
  a.out[2] = rint(a.ep[2]);                             // EpLenMean: half to even, as np.round; NaN stays NaN
  a.out[3] = S[0] / (double)a.n;                        // vf_loss
  a.out[4] = 0.5 * (double)a.A * 2.8378770664093453 + lsum;   // entropy, log(2 pi e)
  a.out[5] = S[1] / (double)a.n;                        // kl
  a.out[6] = a.ep[2];                                   // the mean length before rounding
  a.out[7] = a.ep[4];                                   // completed episodes
}

}  // namespace

extern "C" int oly_episode_stats(oly_ctx* ctx, int T, int N, int rew_f64, double gamma, const void* rew, const float* rew2,
                                 const uint8_t* last, double* out, oly_stream stream) {
  if (!ctx) return OLY_EINVAL;
  if (ctx->stats_ws_bytes < sizeof(double) * EP_MAX_BLOCKS * EP_Q)
    OLY_FAIL(ctx, OLY_EINVAL, "oly_episode_stats: the context's partial-sum buffer is too small");
  return run_episode_stats(ctx, "oly_episode_stats", T, N, rew_f64, gamma, rew, rew2, last, ctx->stats_ws, out, stream);
}

extern "C" int64_t oly_iter_log_ws_floats(int n) {
  if (n < 1) return -1;
  return (int64_t)ws_layout(n).total;
}

extern "C" int oly_iter_log(oly_ctx* ctx, const oly_iter_log_args* f, oly_stream stream) {
  if (!ctx) return OLY_EINVAL;
  if (!f) OLY_FAIL(ctx, OLY_EINVAL, "oly_iter_log: NULL argument");
  if (f->T < 1 || f->N < 1 || (long)f->T * (long)f->N > 2147483647L || (long)f->T * (long)f->N != (long)f->n)
    OLY_FAIL(ctx, OLY_EINVAL, "oly_iter_log: n >= 1 rows are the [T, N] blocks' T N (got n %d, T %d, N %d)", f->n, f->T, f->N);
  if (f->in_dim <= 0 || f->in_dim > IN_MAX || f->act_dim <= 0 || f->act_dim > OUT_MAX)
    OLY_FAIL(ctx, OLY_EINVAL, "oly_iter_log: supported: 0 < in_dim <= %d, 0 < act_dim <= %d (got %d, %d)", IN_MAX, OUT_MAX,
             f->in_dim, f->act_dim);
  if (!f->x || !f->v_target || !f->mu_old || !f->log_sigma_old || !f->log_sigma || !f->critic_packed || !f->policy_packed ||
      !f->rew_env || !f->rew || !f->last || !f->colstats || !f->ws || !f->out)
    OLY_FAIL(ctx, OLY_EINVAL, "oly_iter_log: NULL pointer in the argument block");
  const WsL W = ws_layout(f->n);
  if (f->ws_floats < (int64_t)W.total || (reinterpret_cast<uintptr_t>(f->ws) & 15) != 0 ||
      (reinterpret_cast<uintptr_t>(f->critic_packed) & 15) != 0 || (reinterpret_cast<uintptr_t>(f->policy_packed) & 15) != 0)
    OLY_FAIL(ctx, OLY_EINVAL, "oly_iter_log: ws (%ld floats for %d rows, got %ld) and the packed streams must be 16-byte aligned",
             (long)W.total, f->n, (long)f->ws_floats);
  const int n = f->n, D = f->in_dim, A = f->act_dim;
  double* chain = reinterpret_cast<double*>(f->ws + W.chain);
  double* c = reinterpret_cast<double*>(f->ws + W.c);
  double* epslots = reinterpret_cast<double*>(f->ws + W.epslots);
  double* ep = reinterpret_cast<double*>(f->ws + W.ep);
  double* slots = reinterpret_cast<double*>(f->ws + W.slots);
  float* y = f->ws + W.y;

  int rc = run_episode_stats(ctx, "oly_iter_log", f->T, f->N, f->rew_f64, 1.0, f->rew_env, f->rew, f->last, epslots, ep,
                             stream);
  if (rc != OLY_OK) return rc;
  rc = oly_col_stats(ctx, n, D, f->x, c, 0, stream);      // c, once
  if (rc != OLY_OK) return rc;
  hipLaunchKernelGGL(iter_chain_kernel, dim3(1), dim3(64), 0, oly_s(stream), D, f->colstats, c, chain);
  OLY_LAUNCH_CHECK(ctx, "iteration diagnostics: statistics chain");

  for (int k = 0; k < 2; ++k) {      // 0: self._V(x) at S + c; 1: self.policy.distribution(x) at S + 2c
    const int od = k == 0 ? 1 : A;
    const float* packed = k == 0 ? f->critic_packed : f->policy_packed;
    for (long c0 = 0, ci = 0; c0 < n; c0 += CHUNK, ++ci) {
      const long rows = n - c0 < CHUNK ? n - c0 : CHUNK;
      rc = oly_ilmlp_forward(ctx, rows, D, od, OLY_ACT_IDENTITY, f->x + (size_t)c0 * D, nullptr, nullptr,
                             chain + (size_t)k * SW, packed, y, stream);
      if (rc != OLY_OK) return rc;
      MetArgs m{k, (int)rows, A, c0, y, f->v_target, f->mu_old, f->log_sigma_old, f->log_sigma,
                slots + ((size_t)k * W.chunks + ci) * CHUNK_BLOCKS};
      hipLaunchKernelGGL(iter_metric_kernel, dim3((unsigned)((rows + THREADS - 1) / THREADS)), dim3(THREADS), 0,
                         oly_s(stream), m);
    }
  }
  FinArgs fa{n, A, W.chunks, f->log_sigma, slots, ep, f->out};
  hipLaunchKernelGGL(iter_finish_kernel, dim3(1), dim3(64), 0, oly_s(stream), fa);
  OLY_LAUNCH_CHECK(ctx, "iteration diagnostics kernels");
  return OLY_OK;
}
