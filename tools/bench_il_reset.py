#!/usr/bin/env python3
"""K22: resetting the ended imitation-learning episodes on the device, against the host-driven reset, at UnitreeH1's
shape on KinematicPhysics.  Times are HIP events on the kernels' stream (the host's enqueue time and, on the host path,
its read-backs are inside the interval whenever the device waits for them), warm-up first, the median of the
repetitions.  Run the tool twice and compare the two JSON lines before quoting a number.

    windows   one ILCore.learn collection [T, N] (default [100, 4096]) with a fit that does nothing, for
              device_reset=False (host: bool(last.any()) per step, reset(env_mask=) when set) and device_reset=True
              (one oly_il_reset_where launch per step), in three regimes:
                no_reset    horizon 1000 > T: no episode ends inside the window
                reset_all   horizon 10: every environment is reset on every tenth step
                one_percent about 1 % of the environments end per step: episodes of 100 steps whose counters start
                            staggered (n mod 100), a per-environment offset applied here, not in the library
    launch    oly_il_reset_where alone at N environments with 0 %, 1 % and 100 % of the mask set, beside
              VecLocoEnv.reset(env_mask=) with the same masks

    python tools/bench_il_reset.py [--learn 100x4096] [--reps 20] [--launch-reps 300]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "olympics-mujoco_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

D, A = 32, 11


def event_median(fn, reps, warmup, eng):
    """Median milliseconds of fn() between two HIP events on the engine's stream."""
    from olympic_hip._ffi import HipTimer
    tm = HipTimer()
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        tm.start(eng._s())
        fn()
        tm.stop(eng._s())
        out.append(tm.elapsed_ms())
    return statistics.median(out), min(out), max(out)


class NoFit:
    def fit(self, dataset, generator=None):
        return None


class Staggered:
    """The environment with episodes of `length` steps that end at different times: `last` is recomputed from the
    environment's own step counters, which start at n mod length."""

    def __init__(self, vec, length):
        self._vec, self._length = vec, length

    def __getattr__(self, name):
        return getattr(self._vec, name)

    def reset(self, env_mask=None):
        obs = self._vec.reset(env_mask=env_mask)
        if env_mask is None:
            self._vec.episode_steps.copy_(torch.arange(self._vec.num_envs, device=obs.device) % self._length)
        return obs

    def step(self, actions, ctrl=None):
        obs, reward, absorbing, info = self._vec.step(actions, ctrl=ctrl)
        info["last"] = absorbing | (self._vec.episode_steps >= self._length)
        return obs, reward, absorbing, info


def window(regime, device_reset, T, N, reps, warmup):
    from olympic_hip.envs import LocoEnvBase
    from olympic_hip.gail import DeviceStandardizer
    from olympic_hip.il_agent import DeviceGaussianPolicy
    from olympic_hip.il_core import ILCore
    vec = LocoEnvBase.make("UnitreeH1.walk.real", num_envs=N, seed=0).vec
    env = vec
    if regime == "reset_all":
        vec.spec.horizon = vec.info.horizon = 10
    elif regime == "one_percent":
        vec.spec.horizon = vec.info.horizon = 10 ** 9
        env = Staggered(vec, 100)
    else:
        assert vec.info.horizon > T
    torch.manual_seed(0)
    lins = [torch.nn.Linear(D, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, A)]
    pol = DeviceGaussianPolicy(vec.eng, lins, DeviceStandardizer(vec.eng, D), std_0=0.8)
    core = ILCore(NoFit(), env, pol, generator=torch.Generator(device="cuda").manual_seed(0), device_reset=device_reset)
    med, lo, hi = event_median(lambda: core.learn(T, T), reps, warmup, vec.eng)
    last = core.blocks["last"]
    row = dict(collection_ms=med, min_ms=lo, max_ms=hi, per_step_ms=med / T, steps_with_a_reset=int(last.any(1).sum()),
               resets=int(last.sum()))
    torch.cuda.synchronize()
    vec.eng.ctx.close()
    return row


def launch_alone(N, reps, warmup):
    from olympic_hip.envs import LocoEnvBase
    vec = LocoEnvBase.make("UnitreeH1.walk.real", num_envs=N, seed=0).vec
    vec.obs_f64 = False
    vec.reset()
    vec.step(torch.zeros((N, A), device="cuda"))
    J, L = vec.trajectories.number_of_trajectories, vec.trajectories.trajectory_length
    g = np.random.default_rng(0)
    tn = torch.as_tensor(g.integers(0, J, N).astype(np.int32)).cuda()
    st = torch.as_tensor(g.integers(0, L, N).astype(np.int32)).cuda()
    obs_in, obs_out = vec._obs.clone(), torch.empty_like(vec._obs)
    res = {}
    for name, frac in (("0", 0.0), ("1", 0.01), ("100", 1.0)):
        m = torch.as_tensor(g.uniform(size=N) < frac).cuda()

        def call():
            vec.eng.il_reset_where(m, vec.physics.qpos, vec.physics.qvel, obs_in, obs_out, vec._prev, vec.episode_steps,
                                   traj_no=tn, step=st, cur_traj=vec._cur_traj, cur_step=vec._cur_step, origin=vec._origin,
                                   sample=vec._sample)
        row = dict(set=int(m.sum()))
        row["il_reset_where_ms"] = event_median(call, reps, warmup, vec.eng)[0]
        row["reset_where_ms"] = event_median(lambda: vec.reset_where(m), reps, warmup, vec.eng)[0]       # + the draws
        row["host_reset_ms"] = event_median(lambda: vec.reset(env_mask=m), reps, warmup, vec.eng)[0]
        row["host_over_device"] = row["host_reset_ms"] / row["reset_where_ms"]
        res[f"mask_{name}_percent"] = row
        print(f"# launch N={N} {name} %: {row}", file=sys.stderr)
    torch.cuda.synchronize()
    vec.eng.ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--learn", default="100x4096")
    ap.add_argument("--reps", type=int, default=20, help="collections per median")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launch-reps", type=int, default=300)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_il_reset needs the GPU: nothing is measured without one")
    T, N = (int(v) for v in args.learn.split("x"))
    res = dict(metric="il_reset", T=T, N=N, reps=args.reps, launch_reps=args.launch_reps)
    for regime in ("no_reset", "reset_all", "one_percent"):
        row = {}
        for name, device_reset in (("host", False), ("device", True), ("host_again", False), ("device_again", True)):
            row[name] = window(regime, device_reset, T, N, args.reps, args.warmup)
        row["host_over_device"] = (min(row["host"]["collection_ms"], row["host_again"]["collection_ms"])
                                   / min(row["device"]["collection_ms"], row["device_again"]["collection_ms"]))
        res[regime] = row
        print(f"# window {regime}: {row}", file=sys.stderr)
    res["launch"] = launch_alone(N, args.launch_reps, 30)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
