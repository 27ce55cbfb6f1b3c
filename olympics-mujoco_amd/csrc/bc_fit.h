// What K24 (csrc/k24_bc_fit.hip, behavioural cloning) shares with K28 (csrc/k28_iam.hip, launch B of the fit on two
// indexed tables, oly_bc_fit.pair): the argument blocks, the workspace layout and the paired rows' device functions.
// K28's kernel is in a file of its own because beside it in one translation unit the unpaired launch B was allocated and
// scheduled differently; alone, K24's kernels compile to the code they had.
#pragma once
#include <type_traits>

#include "ilmlp_fit.h"
#include "oly_common.h"

namespace oly_bc {
using namespace oly_ilfit;
using oly_fit::row_at;
static_assert(IN_MAX == oly_fit::MAX_IN, "fit_common.h's statistics arrays have this file's pitch");

constexpr int MAX_BATCH = OLY_BC_MAX_BATCH;   // loss_tree folds at most THREADS = 256 tiles of 16 rows
constexpr int MAX_ACT = OLY_BC_MAX_ACT;
constexpr int OUTP = OUT_MAX;                 // pitch of the output layer's delta: two column tiles
static_assert(MAX_BATCH <= 16 * THREADS && 2 * MAX_ACT <= OUTP, "one loss partial per thread; 2A output columns");

// workspace (floats), BP = batch rounded up to 16 rows; [BP][W] arrays in row quads, element (row, col) at
// ((row / 4) W + col) 4 + row % 4:
//   xs [BP][64] standardised rows | h1 [BP][512] | h2 [BP][256] | dZ1 [BP][512] | dZ2 [BP][256] | dZ3 [BP][32] |
//   loss partials [2][BP / 16][2] f64 ((nll, sum log_sigma), (squared error, 0)) | statistics partials [NSP][2][64] f64 |
//   the minibatch's column sums [2][64] f64 | the transposed streams W2T, W3T
struct WsL {
  size_t xs, h1, h2, dz1, dz2, dz3, lossp, statp, delta, w2t, w3t, total;
};
__host__ __device__ inline WsL ws_layout(int batch) {
  const size_t BP = (size_t)(batch + 15) / 16 * 16;
  WsL W;
  W.xs = 0;
  W.h1 = W.xs + BP * IN_MAX;
  W.h2 = W.h1 + BP * H1;
  W.dz1 = W.h2 + BP * H2;
  W.dz2 = W.dz1 + BP * H1;
  W.dz3 = W.dz2 + BP * H2;
  W.lossp = W.dz3 + BP * OUTP;
  W.statp = W.lossp + BP / 16 * 8;
  W.delta = W.statp + (size_t)NSP * 2 * IN_MAX * 2;
  W.w2t = W.delta + 2 * IN_MAX * 2;
  W.w3t = W.w2t + (size_t)H2 * H1;
  W.total = W.w3t + (size_t)OUTP * H2;
  return W;
}

// W2T / W3T are the B operands of the data gradients dH1 = dZ2 W2 (N = 256 outputs) and dH2 = dZ3 W3 (N = 32, rows
// n >= 2A zero) in pt_index's layout (fit_common.h)
struct FitArgs {
  int in_dim, n_rows, act_dim, out_dim;
  int ds, d2, std2, stride2;   // fit_common.h's two-source members: one source here (ds = in_dim, no x2)
  const float* x2;
  int R, Rn;                   // rows of step s / s+1 (0: none)
  long off, off_next;          // first position of step s / s+1 in perm
  const int32_t* perm;         // idx [n_steps, batch]
  const float *x, *targets;
  double* colstats;            // or NULL: the rows go in as they are
  float *param, *m, *v, *packed, *ws;
  float ls_min, ls_max, nll_eps;
  oly_fit::AdamK ad;
  float wd;                    // weight_decay
  double* out;                 // + 3 s
  ParamLayout P;
  WsL W;
};

// oly_bc_fit.pair (K28, the inverse action model's fit): the rows of two tables and the raw actions.  K24's prologue and
// rows kernel are templates over their argument block and are instantiated over this one for a paired call alone: a
// call without a pair runs the FitArgs instantiations, which compile to the kernels as they were.  Here ds = in_dim (ONE
// Standardizer over the concatenated row, so colstats_add and the layout [3, in_dim] stay), the first table's width is
// d1, the second's d2.
struct PairFitArgs : FitArgs {
  int d1, stride1;             // x [n_rows, stride1], its first d1 columns; x2 [n_rows, stride2], its first d2
  const float *actions, *central, *delta;   // [n_rows, A], [A], [A]: the target is formed from them in launch A
};
template <class KA>
constexpr bool PAIRED = std::is_same<KA, PairFitArgs>::value;

// column k of the concatenated data row `row`
__device__ __forceinline__ float pair_at(const PairFitArgs& a, size_t row, int k) {
  return k < a.d1 ? a.x[row * a.stride1 + k] : a.x2[row * a.stride2 + (k - a.d1)];
}

// fit_common.h's stats_slice on the two tables: the same chains over the same values in the same order, so the
// partials have the bits of stats_slice on the materialised table
__device__ inline void pair_stats_slice(const PairFitArgs& a, long off, int R, int s, double* part) {
  const int tid = threadIdx.x, k = tid & (IN_MAX - 1), grp = tid >> 6;
  const int per = (R + NSP - 1) / NSP, r0 = s * per, r1 = min(R, r0 + per);
  double sum = 0.0, ss = 0.0;
  if (k < a.in_dim)
    for (int r = r0 + grp; r < r1; r += 4) {
      const double v = pair_at(a, (size_t)row_at(a, off + r), k);
      sum += v;
      ss += v * v;
    }
  oly_fit::fold_chains(sum, ss, a.in_dim, part, reinterpret_cast<double*>(a.ws + a.W.statp) + (size_t)s * 2 * IN_MAX);
}

// oly_bc_targets' value for element (row, j): its float operations in its order (bc_targets_kernel, k24_bc_fit.hip)
__device__ __forceinline__ float pair_target(const PairFitArgs& a, size_t row, int A, int j) {
  const float hi = 0x1.fffffcp-1f;
  float u = (a.actions[row * A + j] - a.central[j]) / a.delta[j];
  u = u < -hi ? -hi : u > hi ? hi : u;
  return (float)atanh((double)u);
}

constexpr double HALF_LOG_2PI_P1 = 0.5 + 0.5 * 1.8378770664093454835606594728112;   // 0.5 + 0.5 log(2 pi)

// launch B of a paired step (k28_iam.hip): ONE launch on `grid` = weight_tiles(in_dim, 2A) workgroups
void launch_weights_pair(const PairFitArgs& a, dim3 grid, oly_stream stream);

}  // namespace oly_bc
