// K19: the discriminator's diagnostics (_discriminator_logging, imitation_lib/imitation/gail_TRPO.py:222-249, extended by
// vail_TRPO.py:23-32), which every run of the reference's launcher executes after each discriminator epoch because it
// passes a SummaryWriter.  The call runs six forwards through _D (seven for VAIL):
//
//   1  all rows           DiscrimLoss                                  :226
//   2  demonstration half D_Expert_Accuracy, D_Out_Expert              :230
//   3  policy half        D_Generator_Accuracy, D_Out_Generator        :231
//   4  all rows           Bernoulli Ent., Neg. Bernoulli Ent. Loss     :240-241
//   5  demonstration half Expert_Loss (halved)                         :244
//   6  policy half        Generator_loss (halved)                      :245
//   7  all rows (VAIL)    Bottleneck_Loss, Beta, their product         vail_TRPO.py:28-32
//
// and every forward first adds its rows to the discriminator's Standardizer (networks.py:68-81; with next states twice,
// :224-227), so each one standardises with other statistics and the live statistics end four (five) c_all later.
//
//   log_chain_kernel   the statistics blocks S1 .. S6 (S7) from the live colstats and the parts' column sums, by
//                      sequential float64 addition in the reference's order; the last block is the new colstats.
//   forwards           the existing launchers (oly_gail_disc_forward_pair, K18; oly_disc_forward_pair, K12) on chunks of
//                      at most 16 384 rows with stats_a / stats_b pointing into the chain.
//   log_metric_kernel  one pass over a chunk's logits (and mu / logvar): float64 partials of the sums every scalar needs,
//                      wave shuffles, then LDS, the waves added in order; one slot per workgroup.
//   log_finish_kernel  adds the slots in block order within chunk order and forms the 12 scalars.
// No atomics, no allocation, no host synchronisation; two runs give identical bits.
#include "disc_common.h"
#include "oly_common.h"

namespace {

constexpr int THREADS = 256;
constexpr int CHUNK = 16384;                    // rows per forward launch
constexpr int CHUNK_BLOCKS = CHUNK / THREADS;   // partial slots per chunk
constexpr int NQ = 6;                           // partial sums per slot
enum { Q_BCE = 0, Q_ENT, Q_SIG, Q_GT, Q_LT, Q_KL };
constexpr int MAX_FWD = 7;
constexpr int CHAIN_BLOCKS = 2 * MAX_FWD;       // two blocks per forward: after the states, after the next states
constexpr int SW = 3 * oly_disc::MAX_IN;        // doubles reserved per statistics block ([3, Ds] dense inside)

// workspace (floats): chain [CHAIN_BLOCKS][SW] f64 | parts [4][SW] f64 (policy states, demonstration states, policy next
// states, demonstration next states) | partial slots [MAX_FWD][chunks * CHUNK_BLOCKS][NQ] f64 | logits [C] |
// mu [C][128] | logvar [C][128] (VAIL), C = min(n_rows, CHUNK) rounded up to four rows
struct WsL {
  size_t chain, parts, slots, logits, mu, logvar, total;
  int chunks;
};
inline WsL ws_layout(long n_rows, bool vail) {
  WsL W;
  W.chunks = (int)((n_rows + CHUNK - 1) / CHUNK);
  const size_t C = (size_t)((n_rows < CHUNK ? n_rows : CHUNK) + 3) / 4 * 4;
  W.chain = 0;
  W.parts = W.chain + (size_t)CHAIN_BLOCKS * SW * 2;
  W.slots = W.parts + (size_t)4 * SW * 2;
  W.logits = W.slots + (size_t)MAX_FWD * W.chunks * CHUNK_BLOCKS * NQ * 2;
  W.mu = W.logits + C;
  W.logvar = W.mu + (vail ? C * oly_disc::ZD : 0);
  W.total = W.logvar + (vail ? C * oly_disc::ZD : 0);
  return W;
}

// Forward k (0-based) covers: 0, 3, 6 all rows; 1, 4 the demonstration half; 2, 5 the policy half.
__host__ __device__ inline int fwd_kind(int k) { return k % 3; }    // 0 all, 1 demo, 2 plcy

// One thread per column, the three rows (count, sum, sumsq) each a chain of float64 additions in the order the
// reference's forwards add them.  Block 2 k is what forward k standardises the states with, block 2 k + 1 its next states
// (the same values when there are none).
__global__ __launch_bounds__(64) void log_chain_kernel(int ds, int two, int n_fwd, double* __restrict__ colstats,
                                                       const double* __restrict__ parts, double* __restrict__ chain) {
  const int j = threadIdx.x;
  if (j >= ds) return;
  for (int r = 0; r < 3; ++r) {
    const int e = r * ds + j;
    const double cp = parts[e], cd = parts[SW + e];
    const double call = cp + cd;
    double np = 0.0, nd = 0.0, nall = 0.0;
    if (two) {
      np = parts[2 * SW + e];
      nd = parts[3 * SW + e];
      nall = np + nd;
    }
    double s = colstats[e];
    for (int k = 0; k < n_fwd; ++k) {
      const int kind = fwd_kind(k);
      s += kind == 0 ? call : kind == 1 ? cd : cp;
      chain[(size_t)(2 * k) * SW + e] = s;
      if (two) s += kind == 0 ? nall : kind == 1 ? nd : np;
      chain[(size_t)(2 * k + 1) * SW + e] = s;
    }
    colstats[e] = s;
  }
}

struct MetArgs {
  const float* logits;      // [R] the chunk's logits, or NULL (forward 7: mu / logvar only)
  const float* mu;          // [R, 128] or NULL
  const float* logvar;
  const float* targets;     // [n_rows] or NULL (0 below n_plcy, 1 from there)
  long row0;                // the chunk's first row in the concatenated batch
  int R, n_plcy;
  double* slots;            // [gridDim.x][NQ]
};

// LOG1P: F.binary_cross_entropy_with_logits' softplus (VAIL); else GailDiscriminatorLoss's literal log(1 + exp(-|d|))
// (math.py:25).  Per-row terms in float32 as the reference evaluates them, summed in float64.
template <bool LOG1P>
__global__ __launch_bounds__(THREADS) void log_metric_kernel(MetArgs a) {
  __shared__ double red[THREADS / 64][NQ];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = blockIdx.x * THREADS + tid;
  double q[NQ] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (a.logits && r < a.R) {
    const long row = a.row0 + r;
    const float d = a.logits[r];
    const float t = a.targets ? a.targets[row] : (row < a.n_plcy ? 0.f : 1.f);
    const float e = expf(-fabsf(d));
    const float l1p = log1pf(e);
    const float sp = LOG1P ? l1p : logf(1.0f + e);
    const float sig = 1.0f / (1.0f + expf(-d));
    const float logsig = -(fmaxf(-d, 0.f) + l1p);               // torch's LogSigmoid
    q[Q_BCE] = (double)(fmaxf(d, 0.f) - d * t + sp);
    q[Q_ENT] = (double)((1.0f - sig) * d - logsig);             // math.py:36
    q[Q_SIG] = (double)sig;
    q[Q_GT] = sig > 0.5f ? 1.0 : 0.0;
    q[Q_LT] = sig < 0.5f ? 1.0 : 0.0;
  }
  if (a.mu) {   // VDBLoss.kl_divergence (math.py:84-86) over the workgroup's rows, elements strided over the threads
    const int r0 = blockIdx.x * THREADS, r1 = min(a.R, r0 + THREADS);
    if (r1 > r0) {
      const float4* m4 = reinterpret_cast<const float4*>(a.mu + (size_t)r0 * oly_disc::ZD);
      const float4* l4 = reinterpret_cast<const float4*>(a.logvar + (size_t)r0 * oly_disc::ZD);
      const int n4 = (r1 - r0) * (oly_disc::ZD / 4);
      double s = 0.0;
      for (int i = tid; i < n4; i += THREADS) {
        const float4 m = m4[i], l = l4[i];
        const double m0 = m.x, m1 = m.y, m2 = m.z, m3 = m.w, l0 = l.x, l1 = l.y, l2 = l.z, l3 = l.w;
        s += m0 * m0 + exp(l0) - l0 - 1.0;
        s += m1 * m1 + exp(l1) - l1 - 1.0;
        s += m2 * m2 + exp(l2) - l2 - 1.0;
        s += m3 * m3 + exp(l3) - l3 - 1.0;
      }
      q[Q_KL] = 0.5 * s;
    }
  }
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    const double v = wave_sum(q[i]);
    if (lane == 0) red[wave][i] = v;
  }
  __syncthreads();
  if (tid < NQ) a.slots[(size_t)blockIdx.x * NQ + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

struct FinArgs {
  int n_rows, n_plcy, n_fwd, vail, chunks;
  float entcoeff, info_constraint, lr_beta;
  const float* beta;        // device scalar (VAIL)
  const double* slots;      // [MAX_FWD][chunks * CHUNK_BLOCKS][NQ]
  double* out;              // [OLY_DISC_LOG_SCALARS]
};

__global__ __launch_bounds__(64) void log_finish_kernel(FinArgs a) {
  __shared__ double S[MAX_FWD][NQ];
  const int tid = threadIdx.x;
  if (tid < a.n_fwd * NQ) {
    const int k = tid / NQ, i = tid % NQ, kind = fwd_kind(k);
    const long R = kind == 0 ? a.n_rows : kind == 1 ? a.n_rows - a.n_plcy : a.n_plcy;
    const double* sl = a.slots + (size_t)k * a.chunks * CHUNK_BLOCKS * NQ;
    double s = 0.0;
    for (long c0 = 0, c = 0; c0 < R; c0 += CHUNK, ++c) {      // chunks in order, their workgroups in order
      const long rc = R - c0 < CHUNK ? R - c0 : CHUNK;
      const int nb = (int)((rc + THREADS - 1) / THREADS);
      for (int b = 0; b < nb; ++b) s += sl[((size_t)c * CHUNK_BLOCKS + b) * NQ + i];
    }
    S[k][i] = s;
  }
  __syncthreads();
  if (tid != 0) return;
  const double n = a.n_rows, np = a.n_plcy, nd = n - np;
  double o[OLY_DISC_LOG_SCALARS];
  for (int i = 0; i < OLY_DISC_LOG_SCALARS; ++i) o[i] = 0.0;
  o[1] = S[2][Q_LT] / np;      // D_Generator_Accuracy
  o[2] = S[2][Q_SIG] / np;     // D_Out_Generator
  o[3] = S[1][Q_GT] / nd;      // D_Expert_Accuracy
  o[4] = S[1][Q_SIG] / nd;     // D_Out_Expert
  o[5] = S[3][Q_ENT] / n;      // Bernoulli Ent.
  o[6] = -(double)a.entcoeff * o[5];
  if (!a.vail) {               // GailDiscriminatorLoss.forward (math.py:22-29): bce - entcoeff ent
    o[0] = S[0][Q_BCE] / n - (double)a.entcoeff * (S[0][Q_ENT] / n);
    o[7] = (S[5][Q_BCE] / np - (double)a.entcoeff * (S[5][Q_ENT] / np)) / 2.0;
    o[8] = (S[4][Q_BCE] / nd - (double)a.entcoeff * (S[4][Q_ENT] / nd)) / 2.0;
  } else {
    // VDBLoss.forward (math.py:52-72): bce + beta (mean KL - I_c).  The three calls go through ONE deepcopy of the loss
    // (gail_TRPO.py:225), whose _update_beta (math.py:80-81, float32) therefore moves the copy's beta between them:
    // forward 5 sees the update of forward 1, forward 6 that of 5 as well.  The copy is dropped afterwards, so the
    // trainer's beta is read and never written; forward 7 uses a fresh copy (vail_TRPO.py:27), i.e. the trainer's beta.
    const float ic = a.info_constraint, lrb = a.lr_beta, beta0 = a.beta[0];
    const double bl1 = S[0][Q_KL] / n - (double)ic, bl5 = S[4][Q_KL] / nd - (double)ic, bl6 = S[5][Q_KL] / np - (double)ic;
    const double bl7 = S[6][Q_KL] / n - (double)ic;
    const float beta1 = fmaxf(0.f, beta0 + lrb * (float)bl1);
    const float beta2 = fmaxf(0.f, beta1 + lrb * (float)bl5);
    o[0] = S[0][Q_BCE] / n + (double)beta0 * bl1;
    o[8] = (S[4][Q_BCE] / nd + (double)beta1 * bl5) / 2.0;
    o[7] = (S[5][Q_BCE] / np + (double)beta2 * bl6) / 2.0;
    o[9] = bl7;
    o[10] = (double)beta0;
    o[11] = (double)beta0 * bl7;
  }
  for (int i = 0; i < OLY_DISC_LOG_SCALARS; ++i) a.out[i] = o[i];
}

struct LogCall {
  const char* name;
  bool vail;
  int in_dim, n_rows, n_plcy;
  float entcoeff, info_constraint, lr_beta;
  const float *x, *targets, *eps, *beta;
  double* colstats;
  const float* packed;
  float* ws;
  int64_t ws_floats;
  double* out;
};

int run_log(oly_ctx* ctx, const LogCall& f, const oly_disc_pair* pair, oly_stream stream) {
  using namespace oly_disc;
  const int d2 = pair ? pair->d2 : 0, ds = f.in_dim - d2;
  if (pair) {
    const char* why = ds <= 0 ? "d2 leaves the first part no column" : pair_error(pair, ds);
    if (!why && pair->mask2) why = "the diagnostics take the second part already gathered (mask2 NULL)";
    if (why) OLY_FAIL(ctx, OLY_EINVAL, "%s: %s (in_dim %d, d2 %d)", f.name, why, f.in_dim, d2);
  }
  if (f.in_dim <= 0 || f.in_dim > MAX_IN || ds <= 0 || f.n_rows <= 0)
    OLY_FAIL(ctx, OLY_EINVAL, "%s: supported: 0 < in_dim <= %d, n_rows > 0 (got in %d, n %d)", f.name, MAX_IN, f.in_dim, f.n_rows);
  if (f.n_plcy <= 0 || f.n_plcy >= f.n_rows)
    OLY_FAIL(ctx, OLY_EINVAL, "%s: n_plcy %d outside (0, %d): both halves need a row", f.name, f.n_plcy, f.n_rows);
  if (!f.x || !f.colstats || !f.packed || !f.ws || !f.out || (f.vail && !f.beta))
    OLY_FAIL(ctx, OLY_EINVAL, "%s: NULL pointer in the argument block", f.name);
  const WsL W = ws_layout(f.n_rows, f.vail);
  if (f.ws_floats < (int64_t)W.total || (reinterpret_cast<uintptr_t>(f.ws) & 15) != 0 ||
      (reinterpret_cast<uintptr_t>(f.packed) & 15) != 0 || (reinterpret_cast<uintptr_t>(f.eps) & 15) != 0)
    OLY_FAIL(ctx, OLY_EINVAL, "%s: ws (%ld floats for %d rows, got %ld), packed and eps must be 16-byte aligned", f.name,
             (long)W.total, f.n_rows, (long)f.ws_floats);
  const bool two = pair && pair->standardise;
  const int n = f.n_rows, np = f.n_plcy, nd = n - np, n_fwd = f.vail ? 7 : 6;
  double* chain = reinterpret_cast<double*>(f.ws + W.chain);
  double* parts = reinterpret_cast<double*>(f.ws + W.parts);
  double* slots = reinterpret_cast<double*>(f.ws + W.slots);
  float* logits = f.ws + W.logits;
  float* mu = f.vail ? f.ws + W.mu : nullptr;
  float* logvar = f.vail ? f.ws + W.logvar : nullptr;

  // the column sums of each part, once
  int rc = oly_col_stats(ctx, np, ds, f.x, parts, 0, stream);
  if (rc != OLY_OK) return rc;
  rc = oly_col_stats(ctx, nd, ds, f.x + (size_t)np * ds, parts + SW, 0, stream);
  if (rc != OLY_OK) return rc;
  if (two) {
    rc = oly_masked_col_stats(ctx, np, pair->stride2, ds, pair->x2, nullptr, parts + 2 * SW, 0, nullptr, stream);
    if (rc != OLY_OK) return rc;
    rc = oly_masked_col_stats(ctx, nd, pair->stride2, ds, pair->x2 + (size_t)np * pair->stride2, nullptr, parts + 3 * SW, 0,
                              nullptr, stream);
    if (rc != OLY_OK) return rc;
  }
  hipLaunchKernelGGL(log_chain_kernel, dim3(1), dim3(64), 0, oly_s(stream), ds, two ? 1 : 0, n_fwd, f.colstats, parts, chain);
  OLY_LAUNCH_CHECK(ctx, "discriminator diagnostics: statistics chain");

  size_t eps_row = 0;      // the noise blocks follow each other in forward order
  for (int k = 0; k < n_fwd; ++k) {
    const int kind = fwd_kind(k);
    const long r0 = kind == 1 ? np : 0, R = kind == 0 ? n : kind == 1 ? nd : np;
    const double* sa = chain + (size_t)(2 * k) * SW;
    const double* sb = chain + (size_t)(2 * k + 1) * SW;
    const bool want_lat = f.vail && (k == 0 || k == 4 || k == 5 || k == 6);   // the forwards whose loss has the KL term
    const bool want_logit = k < 6;
    const float* eps_k = (f.eps && k < 6) ? f.eps + eps_row * ZD : nullptr;
    for (long c0 = 0, c = 0; c0 < R; c0 += CHUNK, ++c) {
      const long rc_rows = R - c0 < CHUNK ? R - c0 : CHUNK;
      const float* xc = f.x + (size_t)(r0 + c0) * ds;
      oly_disc_pair pc;
      if (pair) {
        pc = *pair;
        pc.x2 = pair->x2 + (size_t)(r0 + c0) * pair->stride2;
      }
      if (f.vail)
        rc = oly_disc_forward_pair(ctx, rc_rows, ds, ds, xc, nullptr, pair ? &pc : nullptr, sa, two ? sb : sa, f.packed,
                                   eps_k ? eps_k + (size_t)c0 * ZD : nullptr, nullptr, want_logit ? logits : nullptr,
                                   want_lat ? mu : nullptr, want_lat ? logvar : nullptr, stream);
      else
        rc = oly_gail_disc_forward_pair(ctx, rc_rows, ds, ds, xc, nullptr, pair ? &pc : nullptr, sa, two ? sb : sa, f.packed,
                                        nullptr, logits, stream);
      if (rc != OLY_OK) return rc;
      MetArgs m{want_logit ? logits : nullptr, want_lat ? mu : nullptr, want_lat ? logvar : nullptr, f.targets,
                r0 + c0, (int)rc_rows, np, slots + ((size_t)k * W.chunks + c) * CHUNK_BLOCKS * NQ};
      const dim3 grid((unsigned)((rc_rows + THREADS - 1) / THREADS));
      if (f.vail) hipLaunchKernelGGL(log_metric_kernel<true>, grid, dim3(THREADS), 0, oly_s(stream), m);
      else hipLaunchKernelGGL(log_metric_kernel<false>, grid, dim3(THREADS), 0, oly_s(stream), m);
    }
    if (k < 6) eps_row += (size_t)R;
  }
  FinArgs fa{n, np, n_fwd, f.vail ? 1 : 0, W.chunks, f.entcoeff, f.info_constraint, f.lr_beta, f.beta, slots, f.out};
  hipLaunchKernelGGL(log_finish_kernel, dim3(1), dim3(64), 0, oly_s(stream), fa);
  OLY_LAUNCH_CHECK(ctx, "discriminator diagnostics kernels");
  return OLY_OK;
}

}  // namespace

extern "C" int64_t oly_gail_disc_log_ws_floats(int n_rows) {
  if (n_rows <= 1) return -1;
  return (int64_t)ws_layout(n_rows, false).total;
}

extern "C" int64_t oly_disc_log_ws_floats(int n_rows) {
  if (n_rows <= 1) return -1;
  return (int64_t)ws_layout(n_rows, true).total;
}

extern "C" int oly_gail_disc_log(oly_ctx* ctx, const oly_gail_disc_log_args* f, const oly_disc_pair* pair, oly_stream stream) {
  if (!ctx) return OLY_EINVAL;
  if (!f) OLY_FAIL(ctx, OLY_EINVAL, "oly_gail_disc_log: NULL argument");
  const LogCall c{"oly_gail_disc_log", false, f->in_dim, f->n_rows, f->n_plcy, f->entcoeff, 0.f, 0.f, f->x, f->targets,
                  nullptr, nullptr, f->colstats, f->packed, f->ws, f->ws_floats, f->out};
  return run_log(ctx, c, pair, stream);
}

extern "C" int oly_disc_log(oly_ctx* ctx, const oly_disc_log_args* f, const oly_disc_pair* pair, oly_stream stream) {
  if (!ctx) return OLY_EINVAL;
  if (!f) OLY_FAIL(ctx, OLY_EINVAL, "oly_disc_log: NULL argument");
  const LogCall c{"oly_disc_log", true, f->in_dim, f->n_rows, f->n_plcy, f->entcoeff, f->info_constraint, f->lr_beta, f->x,
                  f->targets, f->eps, f->beta, f->colstats, f->packed, f->ws, f->ws_floats, f->out};
  return run_log(ctx, c, pair, stream);
}
