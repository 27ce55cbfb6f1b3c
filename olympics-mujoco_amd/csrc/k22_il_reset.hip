// K22: reset of the imitation-learning environments whose episode ended, for all N in one launch and without a host
// read-back (the masked half of LocoEnvBase.reset, which the launcher's loop used to drive from the host):
//   oly_il_reset_where   reset / setup                    loco_env_base.py:568-657
//                        set_sim_state                    loco_env_base.py:659-684
//                        Trajectory.reset_trajectory      utils/trajectory.py:289-323
//                        mean_grf.reset()                 loco_env_base.py:584
// One wave per environment, its lanes over the row's columns like K4: the table row is read coalesced and every store is
// to consecutive addresses.  The wave of an environment whose mask byte is clear leaves after that one byte load (and,
// when obs_out is a separate buffer, after copying its observation row).  A masked wave writes, in this order of
// outputs, the trajectory cursor + origin + sample (traj_reset_kernel's expression: the same bits), the physics state
// (a zero row with the sample's entries at qpos_adr / qvel_adr, found through the INVERSE tables address -> spec slot, so
// one lane owns each element and nothing is zeroed first and scattered after), the created observation of that state
// (K1's gather and narrowing; the ground-force columns are 0 because mean_grf was just reset), the reward's carried
// value and the step counter.  Nothing is read that the same launch writes.  Bound: launch latency; at N = 4096 a row
// copy of about 1.4 KB per masked environment.
#include "oly_common.h"

namespace {
constexpr int THREADS = 256;
constexpr int WAVE = 64;
constexpr int ENVS_PER_BLOCK = THREADS / WAVE;

struct ResetArgs {
  int N;
  const IlDev* md;
  TrajDev tj;                 // tj.rows == nullptr: no trajectory, the state rows are zeroed
  const uint8_t* mask;
  const int* traj_no;
  const int* step;
  int* cur_traj;
  int* cur_step;
  double* origin;
  double* sample;
  double* qpos;
  double* qvel;
  const int* qpos_slot;       // [nq]  address -> slot among the first n_pos sample entries, or -1
  const int* qvel_slot;       // [nv]  address -> slot among the next n_vel sample entries, or -1
  const void* obs_in;
  void* obs_out;
  double* prev;
  int* episode_steps;
};

template <bool OBS64>
__global__ __launch_bounds__(THREADS) void il_reset_where_kernel(ResetArgs p) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int n = blockIdx.x * ENVS_PER_BLOCK + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (n >= p.N) return;
  const IlDev* __restrict__ md = p.md;
  const int n_obs = md->n_obs;
  if (p.mask && !p.mask[n]) {                       // wave-uniform: one byte per wave
    if (p.obs_in != p.obs_out) {
      for (int c = lane; c < n_obs; c += WAVE) {
        const size_t o = (size_t)n * n_obs + c;
        if (OBS64)
          static_cast<double*>(p.obs_out)[o] = static_cast<const double*>(p.obs_in)[o];
        else
          static_cast<float*>(p.obs_out)[o] = static_cast<const float*>(p.obs_in)[o];
      }
    }
    return;
  }
  const int nq = md->nq, nv = md->nv, n_pos = md->n_pos, n_vel = md->n_vel;
  const double* row = nullptr;
  if (p.tj.rows) {
    // out-of-range indices are clamped exactly as traj_reset_kernel clamps them
    int j = p.traj_no[n], s = p.step[n];
    j = min(max(j, 0), p.tj.n_traj - 1);
    s = min(max(s, 0), p.tj.len - 1);
    row = p.tj.rows + ((size_t)j * p.tj.len + s) * p.tj.n_keys;
    for (int k = lane; k < p.tj.n_keys; k += WAVE) {
      double v = row[k];
      if (k == 0) v -= row[0];
      if (k == 1) v -= row[1];
      p.sample[(size_t)n * p.tj.n_keys + k] = v;
    }
    if (lane == 0) { p.cur_traj[n] = j; p.cur_step[n] = s; }
    if (lane < 2) p.origin[2 * n + lane] = row[lane];
  }
  // sample entry k as traj_reset_kernel stores it, read from the table (never from the sample row this launch writes)
  auto entry = [&](int k) -> double {
    double v = row[k];
    if (k == 0) v -= row[0];
    if (k == 1) v -= row[1];
    return v;
  };
  // staged-row element sidx of the reset state: [qpos (nq) | qvel (nv) | mean_grf (n_grf, zero after its reset)]
  auto staged = [&](int sidx) -> double {
    if (!row) return 0.0;
    if (sidx < nq) {
      const int slot = p.qpos_slot[sidx];
      return (slot >= 0 && slot < n_pos) ? entry(slot) : 0.0;
    }
    if (sidx < nq + nv) {
      const int slot = p.qvel_slot[sidx - nq];
      return (slot >= 0 && slot < n_vel) ? entry(n_pos + slot) : 0.0;
    }
    return 0.0;
  };
  for (int a = lane; a < nq; a += WAVE) p.qpos[(size_t)n * nq + a] = staged(a);
  for (int a = lane; a < nv; a += WAVE) p.qvel[(size_t)n * nv + a] = staged(nq + a);
  for (int c = lane; c < n_obs; c += WAVE) {
    const double x = staged(md->src[c]);
    const size_t o = (size_t)n * n_obs + c;
    if (OBS64)
      static_cast<double*>(p.obs_out)[o] = x;
    else
      static_cast<float*>(p.obs_out)[o] = (float)x;
  }
  if (lane == 0) {
    p.episode_steps[n] = 0;
    if (md->reward_type != OLY_REWARD_NONE) p.prev[n] = staged(md->reward_sidx);   // self._obs of the reset
  }
}
}  // namespace

extern "C" int oly_il_reset_where(oly_ctx* ctx, const oly_il_reset_args* f, oly_stream stream) {
  if (!ctx) return OLY_EINVAL;
  if (!f) OLY_FAIL(ctx, OLY_EINVAL, "oly_il_reset_where: NULL argument block");
  if (!ctx->il_ok) OLY_FAIL(ctx, OLY_EINVAL, "oly_il_reset_where before oly_il_configure");
  const IlDev& h = ctx->il_host;
  if (f->n < 0) OLY_FAIL(ctx, OLY_EINVAL, "oly_il_reset_where: n = %d", f->n);
  if (f->traj_no) {
    if (!ctx->traj_ok) OLY_FAIL(ctx, OLY_EINVAL, "oly_il_reset_where: traj_no given before oly_traj_upload");
    if (ctx->traj.n_keys < h.n_pos + h.n_vel)
      OLY_FAIL(ctx, OLY_EINVAL, "oly_il_reset_where: the uploaded table has %d keys, the model needs n_pos + n_vel = %d",
               ctx->traj.n_keys, h.n_pos + h.n_vel);
    if (!f->step || !f->cur_traj || !f->cur_step || !f->origin || !f->sample)
      OLY_FAIL(ctx, OLY_EINVAL, "oly_il_reset_where: NULL step / cur_traj / cur_step / origin / sample with traj_no given");
  }
  if (!f->qpos || !f->qvel || !f->qpos_slot || !f->qvel_slot || !f->obs_in || !f->obs_out || !f->episode_steps)
    OLY_FAIL(ctx, OLY_EINVAL, "oly_il_reset_where: NULL qpos / qvel / qpos_slot / qvel_slot / obs_in / obs_out / episode_steps");
  if (h.reward_type != OLY_REWARD_NONE && !f->prev) OLY_FAIL(ctx, OLY_EINVAL, "oly_il_reset_where: prev required by the reward");
  if (f->n == 0) return OLY_OK;
  ResetArgs a;
  a.N = f->n; a.md = ctx->il_dev;
  a.tj = ctx->traj;
  if (!f->traj_no) a.tj.rows = nullptr;
  a.mask = f->mask; a.traj_no = f->traj_no; a.step = f->step; a.cur_traj = f->cur_traj; a.cur_step = f->cur_step;
  a.origin = f->origin; a.sample = f->sample; a.qpos = f->qpos; a.qvel = f->qvel; a.qpos_slot = f->qpos_slot;
  a.qvel_slot = f->qvel_slot; a.obs_in = f->obs_in; a.obs_out = f->obs_out; a.prev = f->prev;
  a.episode_steps = f->episode_steps;
  const dim3 grid((unsigned)((f->n + ENVS_PER_BLOCK - 1) / ENVS_PER_BLOCK));
  if (f->out_flags & OLY_OUT_OBS_F64)
    hipLaunchKernelGGL(il_reset_where_kernel<true>, grid, dim3(THREADS), 0, oly_s(stream), a);
  else
    hipLaunchKernelGGL(il_reset_where_kernel<false>, grid, dim3(THREADS), 0, oly_s(stream), a);
  OLY_LAUNCH_CHECK(ctx, "il_reset_where_kernel");
  return OLY_OK;
}
