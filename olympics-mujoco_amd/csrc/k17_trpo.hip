// K17: TRPO's policy step for the imitation policy GaussianTorchPolicy(FullyConnectedNetwork(in -> 512 -> 256 -> out,
// relu, relu, identity), state-independent log_sigma) (examples/imitation_learning/utils.py:126-134), as
// GAIL_TRPO.fit runs it (imitation_lib/imitation/gail_TRPO.py:131-149) through mushroom-rl's TRPO.  mushroom-rl is
// not part of the reference: what this file restates (_compute_loss, _fisher_vector_product_t, _conjugate_gradient,
// _line_search) is a READING of mushroom-rl >= 1.10.  Three entries:
//
//   oly_trpo_grad   J = mean(exp(logp - old_logp) adv) + ent_coeff entropy and its gradient (_compute_loss + backward)
//   oly_trpo_fvp    the exact Hessian-vector product of mean KL(old || pi_theta), plus cg_damping p
//                   (_fisher_vector_product_t), written as forward-over-reverse (R-op) - see DESIGN.md section 13
//   oly_trpo_step   the whole step: old distribution, gradient, CG, step size, line search, restore; no host
//                   synchronisation (CG's early stop and the line search's acceptance are device predicates)
//
// Every forward standardises with S + k c (S the live Standardizer on entry, c the batch's (count, sum, sumsq),
// added k times in sequence as Standardizer.forward would, networks.py:68-81); k is an argument.
//
// Launch plan.  The rows are cut into chunks of at most CHUNK rows (the row-side workspace is bounded by CHUNK).
// Per chunk, every layer is one launch of gemm_kernel: 64 x 64 output tiles, fmaf chains over k ascending on the
// vector ALU; a second term (the tangent's two products) continues the same chain.  The weight-side products
// (sums over rows) are split into row blocks of RB rows: each block writes a partial, reduce_kernel adds the
// partials in block order and the chunks in chunk order.  No atomics, no data-dependent order: two runs give
// identical bits.  Per row and product: about 2.0 MFLOP at in = 32, out = 11.
#include <cmath>
#include <initializer_list>

#include "oly_common.h"

namespace {

constexpr int IN_MAX = 64, H1 = 512, H2 = 256, OUT_MAX = 32;
constexpr int CHUNK = 16384, RB = 256;
constexpr int GT = 64, GK = 16, GTH = 256, MAXJ = 3;
constexpr int CG_THREADS = 1024;

// control ints (device) and f32 scalars
enum { C_KRUN = 0, C_CGDONE, C_LSDONE, C_JACC, C_JRUN, C_N };
enum { F_R2 = 0, F_SHS, F_N };

// flat parameter layout (mushroom's order: the network's parameters, then log_sigma)
struct Layout {
  int D, A;
  long w1, b1, w2, b2, w3, b3, ls, np;
};
__host__ __device__ inline Layout layout(int D, int A) {
  Layout L;
  L.D = D;
  L.A = A;
  L.w1 = 0;
  L.b1 = (long)H1 * D;
  L.w2 = L.b1 + H1;
  L.b2 = L.w2 + (long)H2 * H1;
  L.w3 = L.b2 + H2;
  L.b3 = L.w3 + (long)A * H2;
  L.ls = L.b3 + A;
  L.np = L.ls + A;
  return L;
}
inline long al4(long v) { return (v + 3) & ~3L; }

// ---------------------------------------------------------------------------------------------------------------
// gemm_kernel: C[M,N] = epilogue(sum over terms of op(A) op(B)), A(m,k) = A[m sam + k sak], B(k,n) = B[k sbk + n sbn].
// Up to MAXJ independent jobs per launch (blockIdx.x enumerates their tiles); blockIdx.y is the k block (kblock
// values of k each), whose result goes to C + y cz.  Epilogue in this order: + bias[n]; relu; zero where
// mask[m ldm + n] <= 0 (torch's relu backward on the saved output).
struct GemmJob {
  const float* A[2];
  const float* B[2];
  long sam[2], sak[2], sbk[2], sbn[2];
  const float* bias;
  const float* mask;
  float* C;
  long ldm, ldc, cz;
  int M, N, K, nterms, relu, kblock, tiles_n, tile0;
};
struct GemmLaunch {
  GemmJob job[MAXJ];
  int njobs;
  const int* gate;   // non-zero *gate: the launch is a no-op
};

__global__ __launch_bounds__(GTH) void gemm_kernel(const GemmLaunch L) {
  if (L.gate && *L.gate) return;
  const int bid = blockIdx.x;
  int j = 0;
#pragma unroll
  for (int q = 1; q < MAXJ; ++q)
    if (q < L.njobs && bid >= L.job[q].tile0) j = q;
  const GemmJob& J = L.job[j];
  const int t = bid - J.tile0, tm = t / J.tiles_n, tn = t - tm * J.tiles_n;
  const int m0 = tm * GT, n0 = tn * GT;
  const long kb0 = (long)blockIdx.y * J.kblock;
  if (kb0 >= J.K) return;
  const long kb1 = min((long)J.K, kb0 + J.kblock);
  __shared__ float As[GK][GT + 4], Bs[GK][GT + 4];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[i][q] = 0.f;
  for (int term = 0; term < J.nterms; ++term) {
    const float* __restrict__ A = J.A[term];
    const float* __restrict__ B = J.B[term];
    const long sam = J.sam[term], sak = J.sak[term], sbk = J.sbk[term], sbn = J.sbn[term];
    const bool a_kfast = sak == 1, b_nfast = sbn == 1;
    for (long k0 = kb0; k0 < kb1; k0 += GK) {
      __syncthreads();
      for (int e = tid; e < GT * GK; e += GTH) {
        int mm, kk;
        if (a_kfast) {
          mm = e >> 4;
          kk = e & 15;
        } else {
          kk = e >> 6;
          mm = e & 63;
        }
        const long m = m0 + mm, k = k0 + kk;
        As[kk][mm] = (m < J.M && k < kb1) ? A[m * sam + k * sak] : 0.f;
        int nn, kq;
        if (b_nfast) {
          kq = e >> 6;
          nn = e & 63;
        } else {
          nn = e >> 4;
          kq = e & 15;
        }
        const long n = n0 + nn, k2 = k0 + kq;
        Bs[kq][nn] = (n < J.N && k2 < kb1) ? B[k2 * sbk + n * sbn] : 0.f;
      }
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < GK; ++kk) {
        float a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          a[i] = As[kk][ty + 16 * i];
          b[i] = Bs[kk][tx + 16 * i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[i][q] = fmaf(a[i], b[q], acc[i][q]);
      }
    }
  }
  float* C = J.C + (long)blockIdx.y * J.cz;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long m = m0 + ty + 16 * i;
    if (m >= J.M) continue;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const long n = n0 + tx + 16 * q;
      if (n >= J.N) continue;
      float z = acc[i][q];
      if (J.bias) z += J.bias[n];
      if (J.relu) z = (z > 0.f || z != z) ? z : 0.f;
      if (J.mask && !(J.mask[m * J.ldm + n] > 0.f)) z = 0.f;
      C[m * J.ldc + n] = z;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Standardise rows [r0, r0 + rows) of obs with S + k c, k = k0 (+ *krun): f32((f64(x) - mean) / std) as K16.
struct StdArgs {
  const float* obs;
  const double *S, *c;
  const int *gate, *krun;
  float* xh;
  long r0;
  int rows, D, k0;
};

__device__ inline void stats_k(const double* S, const double* c, int D, int col, int k, double& mean, double& sd) {
  double cnt = S[col], s = S[D + col], ss = S[2 * D + col];
  for (int i = 0; i < k; ++i) {   // the running sums take the batch once per forward, in sequence
    cnt += c[col];
    s += c[D + col];
    ss += c[2 * D + col];
  }
  const double n = cnt + 1e-2;
  mean = s / n;
  sd = sqrt(fmax((ss + 1e-2) / n - mean * mean, 1e-2));
}

__global__ __launch_bounds__(256) void std_kernel(const StdArgs a) {
  if (a.gate && *a.gate) return;
  __shared__ double s_mean[IN_MAX], s_sd[IN_MAX];
  const int k = a.k0 + (a.krun ? *a.krun : 0);
  if ((int)threadIdx.x < a.D) stats_k(a.S, a.c, a.D, threadIdx.x, k, s_mean[threadIdx.x], s_sd[threadIdx.x]);
  __syncthreads();
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long)a.rows * a.D) return;
  const int col = (int)(e % a.D);
  const float xv = a.obs[a.r0 * a.D + e];
  a.xh[e] = (float)(((double)xv - s_mean[col]) / s_sd[col]);
}

// ---------------------------------------------------------------------------------------------------------------
// Per-row terms of the Gaussian head.  sigma = exp(log_sigma); torch's MultivariateNormal with a diagonal
// scale_tril: log_prob = -(A log(2 pi) + sum u^2) / 2 - sum log(sigma), u = (a - mu) / sigma.
enum { R_MU_OLD = 0, R_LOGP_OLD, R_GRAD, R_FVP, R_EVAL_J, R_EVAL_KL };
struct RowArgs {
  int mode, rows, A, n;
  long r0;
  const int* gate;
  const float *mu, *mud;            // chunk [rows, A]: the mean and its tangent
  const float *act, *adv;           // global [n, A], [n]
  const float *ls, *ls_old, *vls;   // log_sigma, the old one, the tangent's log_sigma part
  float *mu_old, *logp_old;         // global [n, A], [n]
  float *d3, *dd3;                  // chunk [rows, A]
  float* rowv;                      // chunk [rows, A + 2]: log_sigma terms | J term | KL term
};

__global__ __launch_bounds__(256) void row_kernel(const RowArgs a) {
  if (a.gate && *a.gate) return;
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.rows) return;
  const long g = a.r0 + r;
  const int A = a.A;
  const float* mu = a.mu + (long)r * A;
  if (a.mode == R_MU_OLD) {
    for (int d = 0; d < A; ++d) a.mu_old[g * A + d] = mu[d];
    return;
  }
  float* rv = a.rowv + (long)r * (A + 2);
  if (a.mode == R_FVP || a.mode == R_EVAL_KL) {
    const float* mo = a.mu_old + g * A;
    float half = 0.f, t2 = 0.f, t3 = 0.f;
    for (int d = 0; d < A; ++d) {
      const float sg = expf(a.ls[d]), so = expf(a.ls_old[d]);
      const float s = sg * sg, s_old = so * so, dl = mu[d] - mo[d];
      if (a.mode == R_FVP) {
        const float mdot = a.mud[(long)r * A + d], vl = a.vls[d], sn = s * (float)a.n;
        a.d3[(long)r * A + d] = dl / sn;
        a.dd3[(long)r * A + d] = (mdot - 2.f * dl * vl) / sn;
        rv[d] = (-2.f * dl * mdot + 2.f * (s_old + dl * dl) * vl) / sn;
      } else {
        half += a.ls[d] - a.ls_old[d];
        const float q = so / sg, w = dl / sg;
        t2 += q * q;
        t3 += w * w;
      }
    }
    // kl_divergence(MVN, MVN): half_term1 + (term2 + term3 - A) / 2
    if (a.mode == R_EVAL_KL) rv[A + 1] = half + 0.5f * (t2 + t3 - (float)A);
    return;
  }
  const float* ac = a.act + g * A;
  float m2 = 0.f, hld = 0.f;
  for (int d = 0; d < A; ++d) {
    const float sg = expf(a.ls[d]), u = (ac[d] - mu[d]) / sg;
    m2 += u * u;
    hld += logf(sg);
  }
  const float logp = -0.5f * ((float)A * 1.8378770664093453f + m2) - hld;
  if (a.mode == R_LOGP_OLD) {
    a.logp_old[g] = logp;
    return;
  }
  const float ratio = expf(logp - a.logp_old[g]), ra = ratio * a.adv[g];
  if (a.mode == R_EVAL_J) {
    rv[A] = ra;
    return;
  }
  // R_GRAD: dJ/dmu = ratio adv (a - mu) / s / n; dJ/dlog_sigma = ratio adv (u^2 - 1) / n (+ ent_coeff later)
  const float w = ra / (float)a.n;
  for (int d = 0; d < A; ++d) {
    const float sg = expf(a.ls[d]), u = (ac[d] - mu[d]) / sg;
    a.d3[(long)r * A + d] = w * u / sg;
    rv[d] = w * (u * u - 1.f);
  }
  rv[A] = ra;
}

// ---------------------------------------------------------------------------------------------------------------
// Column sums over row blocks: partial[y][dst + c] = sum over the rows of block y (ascending) of src[r ld + c].
struct ColJob {
  const float* src;
  long ld;
  int ncols, dst, col0;
};
struct ColLaunch {
  ColJob job[4];
  int njobs, total, rows;
  long pstride;
  float* partial;
  const int* gate;
};

__global__ __launch_bounds__(256) void colsum_kernel(const ColLaunch L) {
  if (L.gate && *L.gate) return;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= L.total) return;
  int j = 0;
#pragma unroll
  for (int q = 1; q < 4; ++q)
    if (q < L.njobs && c >= L.job[q].col0) j = q;
  const ColJob& J = L.job[j];
  const int cl = c - J.col0;
  const int r0 = blockIdx.y * RB, r1 = min(L.rows, r0 + RB);
  float s = 0.f;
  for (int r = r0; r < r1; ++r) s += J.src[(long)r * J.ld + cl];
  L.partial[(long)blockIdx.y * L.pstride + J.dst + cl] = s;
}

// ---------------------------------------------------------------------------------------------------------------
// acc[i] (=, or += after the first chunk) the partials of the chunk's nb blocks in block order, i in [lo, hi).
// On the last chunk: RED_FVP writes out[i] = acc[i] + damping p[i]; RED_GRAD writes out[i] = acc[i] (+ ent_coeff
// on log_sigma) and J to *jout.
enum { RED_ACC = 0, RED_FVP, RED_GRAD };
struct RedArgs {
  const float* partial;
  long pstride, lo, hi, ls, np;
  int nb, first, last, mode, A, n;
  float damping, ent_coeff;
  const float *p, *theta_ls;
  float *acc, *out;
  double* jout;
  const int* gate;
};

__device__ inline float entropy_of(const float* ls, int A) {
  // GaussianTorchPolicy.entropy_t: A / 2 log(2 pi e) + sum(log_sigma)
  float s = 0.f;
  for (int d = 0; d < A; ++d) s += ls[d];
  return 0.5f * (float)A * 2.8378770664093453f + s;
}

__global__ __launch_bounds__(256) void reduce_kernel(const RedArgs a) {
  if (a.gate && *a.gate) return;
  for (long i = a.lo + (long)blockIdx.x * blockDim.x + threadIdx.x; i < a.hi; i += (long)gridDim.x * blockDim.x) {
    float s = a.partial[i];
    for (int b = 1; b < a.nb; ++b) s += a.partial[(long)b * a.pstride + i];
    const float v = a.first ? s : a.acc[i] + s;
    a.acc[i] = v;
    if (!a.last) continue;
    if (a.mode == RED_FVP && i < a.np) a.out[i] = v + a.damping * a.p[i];
    if (a.mode == RED_GRAD) {
      if (i < a.ls) a.out[i] = v;
      else if (i < a.np) a.out[i] = v + a.ent_coeff;
      else *a.jout = (double)(v / (float)a.n + a.ent_coeff * entropy_of(a.theta_ls, a.A));
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// _conjugate_gradient (numpy float32 in the reference): one workgroup.  Dot products: per-thread f64 partials over
// i = t, t + 1024, ..., then a fixed tree; rounded to f32 as numpy's float32 dot returns them.
struct CgArgs {
  int np, n_cg, phase;   // phase 0: start (x = 0, r = p = g); 1: one iteration after z = Fvp(p)
  float tol;
  const float* g;
  float *x, *r, *p, *z, *fs;
  int* ctl;
};

__device__ float block_dot(const float* a, const float* b, int n, double* sh) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += CG_THREADS) s += (double)a[i] * (double)b[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = CG_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  const double t = sh[0];
  __syncthreads();
  return (float)t;
}

__global__ __launch_bounds__(CG_THREADS) void cg_kernel(const CgArgs a) {
  __shared__ double sh[CG_THREADS];
  const int n = a.np;
  if (a.phase == 0) {
    for (int i = threadIdx.x; i < n; i += CG_THREADS) {
      a.x[i] = 0.f;
      a.r[i] = a.g[i];
      a.p[i] = a.g[i];
    }
    const float r2 = block_dot(a.g, a.g, n, sh);
    if (threadIdx.x == 0) {
      a.fs[F_R2] = r2;
      a.ctl[C_KRUN] = 0;
      a.ctl[C_CGDONE] = 0;
      a.ctl[C_LSDONE] = 0;
      a.ctl[C_JACC] = -1;
      a.ctl[C_JRUN] = 0;
    }
    return;
  }
  if (a.ctl[C_CGDONE]) return;
  const float r2 = a.fs[F_R2];
  const float v = r2 / block_dot(a.p, a.z, n, sh);
  for (int i = threadIdx.x; i < n; i += CG_THREADS) {
    a.x[i] = a.x[i] + v * a.p[i];
    a.r[i] = a.r[i] - v * a.z[i];
  }
  __syncthreads();
  const float r2n = block_dot(a.r, a.r, n, sh);
  const float mu = r2n / r2;
  for (int i = threadIdx.x; i < n; i += CG_THREADS) a.p[i] = a.r[i] + mu * a.p[i];
  __syncthreads();
  if (threadIdx.x == 0) {
    a.fs[F_R2] = r2n;
    const int k = a.ctl[C_KRUN] + 1;
    a.ctl[C_KRUN] = k;
    if (r2n < a.tol || k >= a.n_cg) a.ctl[C_CGDONE] = 1;
  }
}

// _line_search's step size: shs = stepdir . Fvp(stepdir) / 2, lm = sqrt(shs / max_kl), full_step = stepdir / lm
__global__ __launch_bounds__(CG_THREADS) void shs_kernel(int np, float max_kl, const float* x, const float* dir, float* fs,
                                                         float* full, double* scal) {
  __shared__ double sh[CG_THREADS];
  const float shs = 0.5f * block_dot(x, dir, np, sh);
  const float lm = sqrtf(shs / max_kl);
  for (int i = threadIdx.x; i < np; i += CG_THREADS) full[i] = x[i] / lm;
  if (threadIdx.x == 0) {
    fs[F_SHS] = shs;
    scal[2] = (double)shs;
  }
}

// theta_j = theta_0 + full_step 2^-j (skipped once a step was accepted)
__global__ __launch_bounds__(256) void ls_set_kernel(long np, float stepsize, const float* th0, const float* full,
                                                     float* th, const int* ctl) {
  if (ctl[C_LSDONE]) return;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < np; i += (long)gridDim.x * blockDim.x)
    th[i] = th0[i] + full[i] * stepsize;
}

// accept when (kl <= 1.5 max_kl) OR / AND (J - prev_loss >= 0), every value finite
__global__ void ls_decide_kernel(int j, int rule, int A, int n, float max_kl, float ent_coeff, const float* acc_j,
                                 const float* acc_kl, const float* theta_ls, const float* fs, int* ctl, double* scal) {
  if (threadIdx.x != 0 || ctl[C_LSDONE]) return;
  const float J = *acc_j / (float)n + ent_coeff * entropy_of(theta_ls, A);
  const float kl = *acc_kl / (float)n;
  const float improve = J - (float)scal[0];
  const bool fin = isfinite(J) && isfinite(kl) && isfinite(fs[F_SHS]);
  const bool kl_ok = kl <= 1.5f * max_kl, up = improve >= 0.f;
  const bool ok = fin && (rule == OLY_TRPO_ACCEPT_AND ? (kl_ok && up) : (kl_ok || up));
  ctl[C_JRUN] = j + 1;
  scal[4] = (double)kl;
  scal[5] = (double)J;
  if (ok) {
    ctl[C_JACC] = j;
    ctl[C_LSDONE] = 1;
  }
}

// restore theta_0 when nothing was accepted; the live statistics take the batch (2 + k_run + 2 j_run) times
__global__ __launch_bounds__(256) void finish_kernel(long np, int D, const float* th0, float* th, double* S, const double* c,
                                                     const int* ctl, const float* fs, const float* x, const float* full,
                                                     float* stepdir_out, float* full_out, double* scal) {
  const bool restore = ctl[C_JACC] < 0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < np; i += (long)gridDim.x * blockDim.x) {
    if (restore) th[i] = th0[i];
    if (stepdir_out) stepdir_out[i] = x[i];
    if (full_out) full_out[i] = full[i];
  }
  if (blockIdx.x != 0) return;
  const int k = 2 + ctl[C_KRUN] + 2 * ctl[C_JRUN];
  if ((int)threadIdx.x < D) {
    const int col = threadIdx.x;
    double cnt = S[col], s = S[D + col], ss = S[2 * D + col];
    for (int i = 0; i < k; ++i) {
      cnt += c[col];
      s += c[D + col];
      ss += c[2 * D + col];
    }
    S[col] = cnt;
    S[D + col] = s;
    S[2 * D + col] = ss;
  }
  if (threadIdx.x == 0) {
    scal[1] = (double)ctl[C_KRUN];
    scal[3] = (double)ctl[C_JACC];
    scal[6] = (double)ctl[C_JRUN];
    scal[7] = (double)fs[F_R2];
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Host side.
struct Ws {   // offsets (floats) into the workspace
  long ctl, fs, c, mu_old, logp_old, th0, g, x, r, p, z, full, acc, xh, h1, hd1, d1, h2, hd2, d2, dd2, mu, mud, d3, dd3,
      rowv, part, total;
  long pstride;
  int ch;
};

Ws ws_layout(long n, int D, int A) {
  const Layout L = layout(D, A);
  Ws w;
  w.ch = (int)(n < CHUNK ? n : CHUNK);
  const long ch = w.ch, np4 = al4(L.np + 2);
  w.pstride = np4;
  long o = 0;
  auto take = [&](long f) {
    const long at = o;
    o += al4(f);
    return at;
  };
  w.ctl = take(C_N);
  w.fs = take(F_N);
  w.c = take(2 * 3 * IN_MAX);   // doubles
  w.mu_old = take(n * A);
  w.logp_old = take(n);
  w.th0 = take(L.np);
  w.g = take(L.np);
  w.x = take(L.np);
  w.r = take(L.np);
  w.p = take(L.np);
  w.z = take(L.np);
  w.full = take(L.np);
  w.acc = take(L.np + 2);
  w.xh = take(ch * D);
  w.h1 = take(ch * H1);
  w.hd1 = take(ch * H1);
  w.d1 = take(ch * H1);
  w.h2 = take(ch * H2);
  w.hd2 = take(ch * H2);
  w.d2 = take(ch * H2);
  w.dd2 = take(ch * H2);
  w.mu = take(ch * A);
  w.mud = take(ch * A);
  w.d3 = take(ch * A);
  w.dd3 = take(ch * A);
  w.rowv = take(ch * (A + 2));
  w.part = take(((ch + RB - 1) / RB) * np4);
  w.total = o;
  return w;
}

bool shape_ok(int D, int h1, int h2, int A, int act) {
  return D > 0 && D <= IN_MAX && h1 == H1 && h2 == H2 && A > 0 && A <= OUT_MAX && act == OLY_ACT_IDENTITY;
}

// C = X W^T: a row-side layer, X [rows, K] row-major (ldx), W [N, K] row-major
GemmJob job_xwt(const float* X, long ldx, const float* W, int rows, int N, int K) {
  GemmJob j{};
  j.A[0] = X;
  j.sam[0] = ldx;
  j.sak[0] = 1;
  j.B[0] = W;
  j.sbk[0] = 1;
  j.sbn[0] = K;
  j.nterms = 1;
  j.M = rows;
  j.N = N;
  j.K = K;
  j.kblock = K;
  return j;
}
// the same chain continued: + X2 W2^T
void add_xwt(GemmJob& j, const float* X, long ldx, const float* W) {
  j.A[1] = X;
  j.sam[1] = ldx;
  j.sak[1] = 1;
  j.B[1] = W;
  j.sbk[1] = 1;
  j.sbn[1] = j.K;
  j.nterms = 2;
}
// C = X W: back through a layer, X [rows, K] (K = the layer's outputs), W [K, N] row-major
GemmJob job_xw(const float* X, long ldx, const float* W, int rows, int N, int K) {
  GemmJob j = job_xwt(X, ldx, W, rows, N, K);
  j.sbk[0] = N;
  j.sbn[0] = 1;
  return j;
}
void add_xw(GemmJob& j, const float* X, long ldx, const float* W) {
  add_xwt(j, X, ldx, W);
  j.sbk[1] = j.N;
  j.sbn[1] = 1;
}
// weight side: C[M,N] = sum_r Dm[r, m] Hm[r, n], in row blocks of RB (block y's partial at C + y cz)
GemmJob job_dth(const float* Dm, int M, const float* Hm, int N, int rows, float* C, long cz) {
  GemmJob j{};
  j.A[0] = Dm;
  j.sam[0] = 1;
  j.sak[0] = M;
  j.B[0] = Hm;
  j.sbk[0] = N;
  j.sbn[0] = 1;
  j.nterms = 1;
  j.M = M;
  j.N = N;
  j.K = rows;
  j.kblock = RB;
  j.C = C;
  j.ldc = N;
  j.cz = cz;
  return j;
}
void add_dth(GemmJob& j, const float* Dm, const float* Hm) {
  j.A[1] = Dm;
  j.sam[1] = 1;
  j.sak[1] = j.M;
  j.B[1] = Hm;
  j.sbk[1] = j.N;
  j.sbn[1] = 1;
  j.nterms = 2;
}

struct Runner {
  hipStream_t s;
  int D, A;
  long n;
  Layout L;
  Ws w;
  float* ws;
  const float *obs, *act, *adv;
  double *S, *c;
  float ent_coeff;

  float* f(long off) const { return ws + off; }
  int rows_of(long r0) const { return (int)(n - r0 < w.ch ? n - r0 : w.ch); }

  void gemm(std::initializer_list<GemmJob> jobs, const int* gate, int ysplit) {
    GemmLaunch g{};
    int tiles = 0, i = 0;
    for (GemmJob j : jobs) {
      j.tiles_n = (j.N + GT - 1) / GT;
      j.tile0 = tiles;
      if (!j.ldc) j.ldc = j.N;
      tiles += ((j.M + GT - 1) / GT) * j.tiles_n;
      g.job[i++] = j;
    }
    g.njobs = i;
    g.gate = gate;
    hipLaunchKernelGGL(gemm_kernel, dim3(tiles, ysplit), dim3(GTH), 0, s, g);
  }

  // forward of rows [r0, r0 + rows) with the statistics S + k c (k = k0 + *krun): xh, H1, H2, mu
  void forward(const float* th, long r0, int rows, int k0, const int* krun, const int* gate) {
    StdArgs sa{obs, S, c, gate, krun, f(w.xh), r0, rows, D, k0};
    hipLaunchKernelGGL(std_kernel, dim3((unsigned)(((long)rows * D + 255) / 256)), dim3(256), 0, s, sa);
    GemmJob j1 = job_xwt(f(w.xh), D, th + L.w1, rows, H1, D);
    j1.bias = th + L.b1;
    j1.relu = 1;
    j1.C = f(w.h1);
    gemm({j1}, gate, 1);
    GemmJob j2 = job_xwt(f(w.h1), H1, th + L.w2, rows, H2, H1);
    j2.bias = th + L.b2;
    j2.relu = 1;
    j2.C = f(w.h2);
    gemm({j2}, gate, 1);
    GemmJob j3 = job_xwt(f(w.h2), H2, th + L.w3, rows, A, H2);
    j3.bias = th + L.b3;
    j3.C = f(w.mu);
    gemm({j3}, gate, 1);
  }

  RowArgs row_args(int mode, long r0, int rows, const float* th, const float* ls_old, const float* mu_old,
                   const float* logp_old, const int* gate) const {
    RowArgs r{};
    r.mode = mode;
    r.rows = rows;
    r.A = A;
    r.n = (int)n;
    r.r0 = r0;
    r.gate = gate;
    r.mu = f(w.mu);
    r.mud = f(w.mud);
    r.act = act;
    r.adv = adv;
    r.ls = th + L.ls;
    r.ls_old = ls_old;
    r.mu_old = const_cast<float*>(mu_old);
    r.logp_old = const_cast<float*>(logp_old);
    r.d3 = f(w.d3);
    r.dd3 = f(w.dd3);
    r.rowv = f(w.rowv);
    return r;
  }
  void rows_launch(const RowArgs& r) {
    hipLaunchKernelGGL(row_kernel, dim3((r.rows + 255) / 256), dim3(256), 0, s, r);
  }

  void colsum(std::initializer_list<ColJob> jobs, int rows, const int* gate) {
    ColLaunch c{};
    int tot = 0, i = 0;
    for (ColJob j : jobs) {
      j.col0 = tot;
      tot += j.ncols;
      c.job[i++] = j;
    }
    c.njobs = i;
    c.total = tot;
    c.rows = rows;
    c.pstride = w.pstride;
    c.partial = f(w.part);
    c.gate = gate;
    hipLaunchKernelGGL(colsum_kernel, dim3((tot + 255) / 256, (rows + RB - 1) / RB), dim3(256), 0, s, c);
  }

  void reduce(long lo, long hi, int rows, bool first, bool last, int mode, const float* p, const float* th, float* out,
              double* jout, float damping, const int* gate) {
    RedArgs r{};
    r.partial = f(w.part);
    r.pstride = w.pstride;
    r.lo = lo;
    r.hi = hi;
    r.ls = L.ls;
    r.np = L.np;
    r.nb = (rows + RB - 1) / RB;
    r.first = first;
    r.last = last;
    r.mode = mode;
    r.A = A;
    r.n = (int)n;
    r.damping = damping;
    r.ent_coeff = ent_coeff;
    r.p = p;
    r.theta_ls = th + L.ls;
    r.acc = f(w.acc);
    r.out = out;
    r.jout = jout;
    r.gate = gate;
    const long cnt = (hi - lo + 255) / 256;
    hipLaunchKernelGGL(reduce_kernel, dim3((unsigned)(cnt < 1024 ? cnt : 1024)), dim3(256), 0, s, r);
  }

  // one old-policy pass over the rows: mu_old (k = 1) or old_log_prob (k = 2)
  void old_pass(int mode, const float* th, int k) {
    for (long r0 = 0; r0 < n; r0 += w.ch) {
      const int rows = rows_of(r0);
      forward(th, r0, rows, k, nullptr, nullptr);
      rows_launch(row_args(mode, r0, rows, th, th + L.ls, f(w.mu_old), f(w.logp_old), nullptr));
    }
  }

  // g = dJ/dtheta at the statistics S + k c, J to *jout (_compute_loss, backward, get_gradient)
  void grad(const float* th, int k, const float* logp_old, float* g, double* jout) {
    for (long r0 = 0; r0 < n; r0 += w.ch) {
      const int rows = rows_of(r0);
      forward(th, r0, rows, k, nullptr, nullptr);
      rows_launch(row_args(R_GRAD, r0, rows, th, th + L.ls, nullptr, logp_old, nullptr));
      GemmJob b1 = job_xw(f(w.d3), A, th + L.w3, rows, H2, A);           // delta2 = m2 (W3^T delta3)
      b1.mask = f(w.h2);
      b1.ldm = H2;
      b1.C = f(w.d2);
      gemm({b1}, nullptr, 1);
      GemmJob b3 = job_xw(f(w.d2), H2, th + L.w2, rows, H1, H2);         // delta1 = m1 (W2^T delta2)
      b3.mask = f(w.h1);
      b3.ldm = H1;
      b3.C = f(w.d1);
      gemm({b3}, nullptr, 1);
      float* P = f(w.part);
      gemm({job_dth(f(w.d3), A, f(w.h2), H2, rows, P + L.w3, w.pstride),
            job_dth(f(w.d2), H2, f(w.h1), H1, rows, P + L.w2, w.pstride),
            job_dth(f(w.d1), H1, f(w.xh), D, rows, P + L.w1, w.pstride)},
           nullptr, (rows + RB - 1) / RB);
      colsum({{f(w.d3), A, A, (int)L.b3, 0}, {f(w.d2), H2, H2, (int)L.b2, 0}, {f(w.d1), H1, H1, (int)L.b1, 0},
              {f(w.rowv), A + 2, A + 1, (int)L.ls, 0}},
             rows, nullptr);
      reduce(0, L.np + 1, rows, r0 == 0, r0 + rows >= n, RED_GRAD, nullptr, th, g, jout, 0.f, nullptr);
    }
  }

  // out = Fvp(p) + damping p at the statistics S + (k0 + *krun) c; mu_old / ls_old: the old distribution
  void fvp(const float* th, int k0, const int* krun, const float* mu_old, const float* ls_old, const float* p,
           float* out, float damping, const int* gate) {
    for (long r0 = 0; r0 < n; r0 += w.ch) {
      const int rows = rows_of(r0);
      forward(th, r0, rows, k0, krun, gate);
      // tangent forward
      GemmJob t1 = job_xwt(f(w.xh), D, p + L.w1, rows, H1, D);            // Hd1 = m1 (V1 x + vb1)
      t1.bias = p + L.b1;
      t1.mask = f(w.h1);
      t1.ldm = H1;
      t1.C = f(w.hd1);
      gemm({t1}, gate, 1);
      GemmJob t2 = job_xwt(f(w.h1), H1, p + L.w2, rows, H2, H1);          // Hd2 = m2 (V2 H1 + W2 Hd1 + vb2)
      add_xwt(t2, f(w.hd1), H1, th + L.w2);
      t2.bias = p + L.b2;
      t2.mask = f(w.h2);
      t2.ldm = H2;
      t2.C = f(w.hd2);
      gemm({t2}, gate, 1);
      GemmJob t3 = job_xwt(f(w.h2), H2, p + L.w3, rows, A, H2);           // mud = V3 H2 + W3 Hd2 + vb3
      add_xwt(t3, f(w.hd2), H2, th + L.w3);
      t3.bias = p + L.b3;
      t3.C = f(w.mud);
      gemm({t3}, gate, 1);
      RowArgs ra = row_args(R_FVP, r0, rows, th, ls_old, mu_old, nullptr, gate);
      ra.vls = p + L.ls;
      rows_launch(ra);
      // backward chains
      GemmJob b1 = job_xw(f(w.d3), A, th + L.w3, rows, H2, A);            // delta2 = m2 (W3^T delta3)
      b1.mask = f(w.h2);
      b1.ldm = H2;
      b1.C = f(w.d2);
      GemmJob b2 = job_xw(f(w.d3), A, p + L.w3, rows, H2, A);             // dd2 = m2 (V3^T delta3 + W3^T dd3)
      add_xw(b2, f(w.dd3), A, th + L.w3);
      b2.mask = f(w.h2);
      b2.ldm = H2;
      b2.C = f(w.dd2);
      gemm({b1, b2}, gate, 1);
      GemmJob b3 = job_xw(f(w.d2), H2, p + L.w2, rows, H1, H2);           // dd1 = m1 (V2^T delta2 + W2^T dd2)
      add_xw(b3, f(w.dd2), H2, th + L.w2);
      b3.mask = f(w.h1);
      b3.ldm = H1;
      b3.C = f(w.d1);
      gemm({b3}, gate, 1);
      // products: Hv_W3 = dd3 H2^T + delta3 Hd2^T, Hv_W2 = dd2 H1^T + delta2 Hd1^T, Hv_W1 = dd1 x^T
      float* P = f(w.part);
      GemmJob w3 = job_dth(f(w.dd3), A, f(w.h2), H2, rows, P + L.w3, w.pstride);
      add_dth(w3, f(w.d3), f(w.hd2));
      GemmJob w2 = job_dth(f(w.dd2), H2, f(w.h1), H1, rows, P + L.w2, w.pstride);
      add_dth(w2, f(w.d2), f(w.hd1));
      gemm({w3, w2, job_dth(f(w.d1), H1, f(w.xh), D, rows, P + L.w1, w.pstride)}, gate, (rows + RB - 1) / RB);
      colsum({{f(w.dd3), A, A, (int)L.b3, 0}, {f(w.dd2), H2, H2, (int)L.b2, 0}, {f(w.d1), H1, H1, (int)L.b1, 0},
              {f(w.rowv), A + 2, A, (int)L.ls, 0}},
             rows, gate);
      reduce(0, L.np, rows, r0 == 0, r0 + rows >= n, RED_FVP, p, th, out, nullptr, damping, gate);
    }
  }

  // J's row sum (acc slot np) at S + (k0 + *krun) c, or KL's (slot np + 1)
  void eval(int mode, const float* th, int k0, const int* krun, const float* ls_old, const int* gate) {
    const int slot = mode == R_EVAL_J ? 0 : 1;
    for (long r0 = 0; r0 < n; r0 += w.ch) {
      const int rows = rows_of(r0);
      forward(th, r0, rows, k0, krun, gate);
      rows_launch(row_args(mode, r0, rows, th, ls_old, f(w.mu_old), f(w.logp_old), gate));
      colsum({{f(w.rowv) + A + slot, A + 2, 1, (int)(L.np + slot), 0}}, rows, gate);
      reduce(L.np + slot, L.np + slot + 1, rows, r0 == 0, false, RED_ACC, nullptr, th, nullptr, nullptr, 0.f, gate);
    }
  }
};

int check_args(oly_ctx* ctx, const oly_trpo_step_args* a, const char* who) {
  if (!a) OLY_FAIL(ctx, OLY_EINVAL, "%s: NULL argument block", who);
  if (a->n <= 0 || !shape_ok(a->in_dim, a->hidden1, a->hidden2, a->out_dim, a->last_act))
    OLY_FAIL(ctx, OLY_ERANGE,
             "%s: supported: n > 0, in <= %d -> %d -> %d -> out <= %d, identity last activation (got n %d, %d -> %d -> "
             "%d -> %d, act %d)",
             who, IN_MAX, H1, H2, OUT_MAX, a->n, a->in_dim, a->hidden1, a->hidden2, a->out_dim, a->last_act);
  if (!a->obs || !a->act || !a->adv || !a->colstats || !a->theta || !a->ws || !a->scal_out)
    OLY_FAIL(ctx, OLY_EINVAL, "%s: NULL pointer in the argument block", who);
  const Ws w = ws_layout(a->n, a->in_dim, a->out_dim);
  if (a->ws_floats < w.total || (reinterpret_cast<uintptr_t>(a->ws) & 15) != 0)
    OLY_FAIL(ctx, OLY_EINVAL, "%s: ws must be 16-byte aligned and hold %ld floats", who, (long)w.total);
  return OLY_OK;
}

Runner make_runner(const oly_trpo_step_args* a, oly_stream stream) {
  Runner R;
  R.s = oly_s(stream);
  R.D = a->in_dim;
  R.A = a->out_dim;
  R.n = a->n;
  R.L = layout(a->in_dim, a->out_dim);
  R.w = ws_layout(a->n, a->in_dim, a->out_dim);
  R.ws = a->ws;
  R.obs = a->obs;
  R.act = a->act;
  R.adv = a->adv;
  R.S = a->colstats;
  R.c = reinterpret_cast<double*>(a->ws + R.w.c);
  R.ent_coeff = a->ent_coeff;
  return R;
}
}  // namespace

extern "C" int64_t oly_trpo_param_count(int in_dim, int h1, int h2, int out_dim) {
  return shape_ok(in_dim, h1, h2, out_dim, OLY_ACT_IDENTITY) ? (int64_t)layout(in_dim, out_dim).np : -1;
}

extern "C" int64_t oly_trpo_ws_floats(int n, int in_dim, int h1, int h2, int out_dim) {
  if (n <= 0 || !shape_ok(in_dim, h1, h2, out_dim, OLY_ACT_IDENTITY)) return -1;
  return (int64_t)ws_layout(n, in_dim, out_dim).total;
}

extern "C" int oly_trpo_old_offsets(int n, int in_dim, int h1, int h2, int out_dim, int64_t* mu_old_off,
                                    int64_t* log_sigma_old_off) {
  if (n <= 0 || !shape_ok(in_dim, h1, h2, out_dim, OLY_ACT_IDENTITY) || !mu_old_off || !log_sigma_old_off) return OLY_EINVAL;
  const Ws w = ws_layout(n, in_dim, out_dim);
  *mu_old_off = (int64_t)w.mu_old;
  *log_sigma_old_off = (int64_t)(w.th0 + layout(in_dim, out_dim).ls);
  return OLY_OK;
}

extern "C" int oly_trpo_grad(oly_ctx* ctx, const oly_trpo_step_args* a, int k_stats, const float* logp_old,
                             float* grad_out, double* j_out, oly_stream stream) {
  if (!ctx) return OLY_EINVAL;
  const int rc = check_args(ctx, a, "oly_trpo_grad");
  if (rc != OLY_OK) return rc;
  if (!logp_old || !grad_out || !j_out || k_stats < 0)
    OLY_FAIL(ctx, OLY_EINVAL, "oly_trpo_grad: NULL logp_old / grad_out / j_out, or k_stats < 0");
  Runner R = make_runner(a, stream);
  const int c_rc = oly_col_stats(ctx, a->n, a->in_dim, a->obs, R.c, 0, stream);
  if (c_rc != OLY_OK) return c_rc;
  R.grad(a->theta, k_stats, logp_old, grad_out, j_out);
  OLY_LAUNCH_CHECK(ctx, "trpo grad kernels");
  return OLY_OK;
}

extern "C" int oly_trpo_fvp(oly_ctx* ctx, const oly_trpo_step_args* a, int k_stats, const float* mu_old,
                            const float* log_sigma_old, const float* p, float* out, oly_stream stream) {
  if (!ctx) return OLY_EINVAL;
  const int rc = check_args(ctx, a, "oly_trpo_fvp");
  if (rc != OLY_OK) return rc;
  if (!mu_old || !log_sigma_old || !p || !out || k_stats < 0)
    OLY_FAIL(ctx, OLY_EINVAL, "oly_trpo_fvp: NULL mu_old / log_sigma_old / p / out, or k_stats < 0");
  Runner R = make_runner(a, stream);
  const int c_rc = oly_col_stats(ctx, a->n, a->in_dim, a->obs, R.c, 0, stream);
  if (c_rc != OLY_OK) return c_rc;
  R.fvp(a->theta, k_stats, nullptr, mu_old, log_sigma_old, p, out, a->cg_damping, nullptr);
  OLY_LAUNCH_CHECK(ctx, "trpo fvp kernels");
  return OLY_OK;
}

extern "C" int oly_trpo_step(oly_ctx* ctx, const oly_trpo_step_args* a, oly_stream stream) {
  if (!ctx) return OLY_EINVAL;
  const int rc = check_args(ctx, a, "oly_trpo_step");
  if (rc != OLY_OK) return rc;
  if (a->n_epochs_cg < 1 || a->n_epochs_line_search < 0 || a->n_epochs_cg > 1000 || a->n_epochs_line_search > 60 ||
      (a->accept_rule != OLY_TRPO_ACCEPT_OR && a->accept_rule != OLY_TRPO_ACCEPT_AND))
    OLY_FAIL(ctx, OLY_ERANGE, "oly_trpo_step: bad n_epochs_cg %d / n_epochs_line_search %d / accept_rule %d",
             a->n_epochs_cg, a->n_epochs_line_search, a->accept_rule);
  Runner R = make_runner(a, stream);
  const Layout& L = R.L;
  const Ws& w = R.w;
  float* th = a->theta;
  int* ctl = reinterpret_cast<int*>(a->ws + w.ctl);
  float* fs = a->ws + w.fs;
  double* scal = a->scal_out;
  const int c_rc = oly_col_stats(ctx, a->n, a->in_dim, a->obs, R.c, 0, stream);   // c, once per step
  if (c_rc != OLY_OK) return c_rc;
  OLY_HIP(ctx, hipMemcpyAsync(R.f(w.th0), th, sizeof(float) * L.np, hipMemcpyDeviceToDevice, R.s));
  const float* th0 = R.f(w.th0);
  // 1-2: the deep copy's distribution (S + c) and log-probabilities (S + 2c); its statistics are discarded
  R.old_pass(R_MU_OLD, th0, 1);
  R.old_pass(R_LOGP_OLD, th0, 2);
  // 3: J = prev_loss and g at the live S + c
  R.grad(th, 1, R.f(w.logp_old), R.f(w.g), scal);
  // 4: CG; the k-th product at S + (1 + k) c, a no-op on the device after the early stop
  CgArgs cg{(int)L.np, a->n_epochs_cg, 0, a->cg_residual_tol, R.f(w.g), R.f(w.x), R.f(w.r), R.f(w.p), R.f(w.z), fs, ctl};
  hipLaunchKernelGGL(cg_kernel, dim3(1), dim3(CG_THREADS), 0, R.s, cg);
  cg.phase = 1;
  for (int k = 1; k <= a->n_epochs_cg; ++k) {
    R.fvp(th, 1 + k, nullptr, R.f(w.mu_old), th0 + L.ls, R.f(w.p), R.f(w.z), a->cg_damping, ctl + C_CGDONE);
    hipLaunchKernelGGL(cg_kernel, dim3(1), dim3(CG_THREADS), 0, R.s, cg);
  }
  // 5: direction = Fvp(stepdir) at S + (2 + k_run) c; shs, lm, full_step
  R.fvp(th, 2, ctl + C_KRUN, R.f(w.mu_old), th0 + L.ls, R.f(w.x), R.f(w.z), a->cg_damping, nullptr);
  hipLaunchKernelGGL(shs_kernel, dim3(1), dim3(CG_THREADS), 0, R.s, (int)L.np, a->max_kl, R.f(w.x), R.f(w.z), fs,
                     R.f(w.full), scal);
  // 6: line search, J at S + (3 + k_run + 2j) c and KL at S + (4 + k_run + 2j) c, no-ops after an acceptance
  const long pbl = (L.np + 255) / 256;
  const unsigned pb = (unsigned)(pbl < 1024 ? pbl : 1024);
  float stepsize = 1.f;
  for (int j = 0; j < a->n_epochs_line_search; ++j, stepsize *= 0.5f) {
    hipLaunchKernelGGL(ls_set_kernel, dim3(pb), dim3(256), 0, R.s, L.np, stepsize, th0, R.f(w.full), th, ctl);
    R.eval(R_EVAL_J, th, 3 + 2 * j, ctl + C_KRUN, th0 + L.ls, ctl + C_LSDONE);
    R.eval(R_EVAL_KL, th, 4 + 2 * j, ctl + C_KRUN, th0 + L.ls, ctl + C_LSDONE);
    hipLaunchKernelGGL(ls_decide_kernel, dim3(1), dim3(64), 0, R.s, j, a->accept_rule, R.A, a->n, a->max_kl,
                       a->ent_coeff, R.f(w.acc) + L.np, R.f(w.acc) + L.np + 1, th + L.ls, fs, ctl, scal);
  }
  // 7: restore theta_0 when nothing was accepted; the live statistics end at S + (2 + k_run + 2 j_run) c
  hipLaunchKernelGGL(finish_kernel, dim3(pb), dim3(256), 0, R.s, L.np, R.D, th0, th, a->colstats, R.c, ctl, fs,
                     R.f(w.x), R.f(w.full), a->stepdir_out, a->full_step_out, scal);
  OLY_LAUNCH_CHECK(ctx, "trpo step kernels");
  if (a->packed) {
    const int p_rc = oly_ilmlp_pack(ctx, R.D, H1, H2, R.A, th + L.w1, th + L.b1, th + L.w2, th + L.b2, th + L.w3,
                                    th + L.b3, a->packed, stream);
    if (p_rc != OLY_OK) return p_rc;
  }
  return OLY_OK;
}
