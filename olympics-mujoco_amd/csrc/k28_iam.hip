// K28: launch B of K24's fit on the rows of two indexed tables (oly_bc_fit.pair: the inverse action model,
// GaussianInvActionModel, imitation_lib/utils/action_models.py:257-528).  Everything else of a paired call (the prologue,
// launch A, the host side) is k24_bc_fit.hip's, instantiated over PairFitArgs; the paired act is k25_sg_act.hip's.
#include "bc_fit.h"

namespace {
using namespace oly_bc;
using oly_fit::adam1;

// Launch B of a paired call: the same tile, the same additions in the same order and the same stores, written with
// ilmlp_fit.h's weight_tile and tile_step (whose 0.5 to 0.8 % the kernel above does not pay); workgroups 1 .. 16 sum step
// s+1's rows from the two tables.  As a template instantiation of the kernel above its FitArgs twin was allocated and
// scheduled differently, so the unpaired call keeps that kernel as it is.
__global__ __launch_bounds__(THREADS) void bc_weights_pair_kernel(PairFitArgs a) {
  __shared__ float red[4 * 256];
  __shared__ float bred[4 * 64];
  __shared__ double dred[2 * THREADS];
  const int tid = threadIdx.x, R = a.R, steps = (R + 15) / 16;
  const WsL& W = a.W;
  const WeightTile T = weight_tile(a, a.in_dim, a.out_dim, OUTP);
  f32x4 acc;
  float bsum;
  dw_accumulate(T.dl, T.al, T.dw, T.aw, T.n0, T.N, T.k0, T.K, steps, acc, bsum);
  meet_waves(red, bred, acc, bsum);
  double g2, b2;
  tile_step(T, a, a.in_dim, red, bred,
            [&](int layer, int ne, int ke, size_t i, size_t pk, float g) {
              const float p = adam1(a, i, g);
              a.packed[pk] = p;
              if (ke >= 0 && layer == 1) a.ws[W.w2t + pt_index(H2, ne, ke)] = p;
              if (ke >= 0 && layer == 2) a.ws[W.w3t + pt_index(OUTP, ne, ke)] = p;
            },
            g2, b2);
  if (blockIdx.x == 0) {
    const double* lp = reinterpret_cast<const double*>(a.ws + W.lossp);
    oly_fit::loss_tree(steps, lp, dred);
    const double nll = dred[0], lsum = dred[THREADS];
    __syncthreads();
    oly_fit::loss_tree(steps, lp + 2 * (size_t)steps, dred);
    if (tid == 0) {
      const double n = (double)R * (double)a.act_dim;
      a.out[0] = nll / n;
      a.out[1] = (double)a.act_dim * HALF_LOG_2PI_P1 + lsum / (double)R;
      a.out[2] = dred[0] / n;
    }
    if (a.colstats) oly_fit::colstats_add(a, R);
  } else if (blockIdx.x <= NSP && a.colstats && a.Rn > 0) {
    pair_stats_slice(a, a.off_next, a.Rn, blockIdx.x - 1, dred);
  }
}

}  // namespace

void oly_bc::launch_weights_pair(const PairFitArgs& a, dim3 grid, oly_stream stream) {
  hipLaunchKernelGGL(bc_weights_pair_kernel, grid, dim3(THREADS), 0, oly_s(stream), a);
}
