// K25's launch as K24's logged fit (oly_bc_fit_steps_log) calls it: oly_sg_act's kernel on gathered rows, with
// statistics that hold a minibatch's sums once more than colstats does.
#pragma once
#include "oly_common.h"

namespace oly_sg {

struct Args {
  long N;
  int in_dim, act_dim;
  const float* x;              // [*, in_dim]
  const int32_t* rows;         // [N] rows of x, clamped to [0, n_rows) for memory safety only; NULL: row r is x's row r
  int n_rows;
  const double* colstats;      // [3, in_dim], or NULL: the rows go in as they are
  const double* extra;         // [2][64] column sums and sums of squares added to colstats' with extra_cnt rows, or NULL
  double extra_cnt;
  const float* packed;
  float ls_min, ls_max;
  const float *central, *delta, *eps;
  float *action, *log_prob, *mu, *log_sigma;   // each may be NULL here
  void* ctrl;                  // NULL: no controls
  int ctrl64;
  const IlDev* md;             // the configured model (read only when ctrl is given)
};

// The rows of two tables (oly_sg_act_args' trailing fields, oly_bc_fit.pair's logged step): row i of x in its first d1
// columns (rows of stride1 floats), row i of x2 in the next in_dim - d1 (rows of stride2), i = rows[r] or r.  Its
// kernels are instantiations of their own, so that a call without them runs what it ran before.
struct PairArgs : Args {
  int d1, stride1, stride2;
  const float* x2;             // NULL with d1 == in_dim
  const double *clip_lo, *clip_hi;   // [A] or both NULL: action = f32(min(max(f64(action), lo), hi))
};

// ONE launch; the shape was checked by the caller
int launch(oly_ctx* ctx, const Args& a, oly_stream stream);
int launch(oly_ctx* ctx, const PairArgs& a, oly_stream stream);

// colstats [3, d1 + d2] += (n, sum, sumsq) of the n rows (x[i, 0 .. d1) | x2[i, 0 .. d2)), i = rows[r] clamped to
// [0, n_rows) or r: oly_col_stats' two launches in accumulate mode and its bits on the materialised 16-byte aligned rows
// (k7_stats.hip)
int col_stats_pair(oly_ctx* ctx, int n, const PairArgs& a, double* colstats, oly_stream stream);

}  // namespace oly_sg
