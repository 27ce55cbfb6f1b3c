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

// ONE launch; the shape was checked by the caller
int launch(oly_ctx* ctx, const Args& a, oly_stream stream);

}  // namespace oly_sg
