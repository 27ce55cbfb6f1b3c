#!/usr/bin/env python3
"""The cost of a PPO checkpoint at config 3's sizes: ppo_checkpoint.state_dict (clones on the device),
one ppo_checkpoint.save to disk (the copies to the host, torch.save, the rename) with the file's size, and one
ppo_checkpoint.load into the same objects (read, compare, the in-place copies), for the run bench.py's config-3 iteration
trains: 4096 environments, T = 400, the mirror loss on, the K13 rollout and the K14 update.  Wall-clock with a device
synchronisation on both sides of every repetition, warm-up first, the median of the repetitions; the file goes to a
temporary directory.  Nothing here is on the per-step path: the numbers are reported, not bounded.

    python tools/bench_ppo_checkpoint.py [--num_envs 4096] [--T 400] [--reps 10]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "olympics-mujoco_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=statistics.median(out), min_ms=min(out), max_ms=max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--T", type=int, default=400)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    from olympic_hip import ppo_checkpoint, specs
    from olympic_hip.a3 import ReplayA3Physics, VecA3Env
    from olympic_hip.engine import Engine
    from olympic_hip.ppo import PPO, MLPCritic, MLPGaussianActor
    from olympic_hip.synthetic import A3_FLOOR_BODY, A3_GEOM_BODYID, A3_LFOOT_BODY, A3_RFOOT_BODY, a3_synthetic_blocks
    from olympic_hip.wrappers import SymmetricEnv
    N, T = args.num_envs, args.T
    spec = specs.A3Spec(mass=41.5)
    blocks = {k: torch.as_tensor(np.ascontiguousarray(v)).cuda() for k, v in a3_synthetic_blocks(N, 32, seed=1).items()}
    vec = VecA3Env(spec, N, Engine(0), ReplayA3Physics(blocks), A3_GEOM_BODYID, A3_FLOOR_BODY, A3_RFOOT_BODY, A3_LFOOT_BODY,
                   rs=np.random.RandomState(0))
    vec.device = vec.eng.device
    env = SymmetricEnv(lambda: vec, mirrored_obs=list(spec.mirrored_obs), mirrored_act=list(spec.mirrored_acts),
                       clock_inds=list(spec.clock_inds))
    hp = dict(gamma=0.99, lam=0.95, lr=1e-4, eps=1e-5, entropy_coeff=0.0, clip=0.2, minibatch_size=65536, epochs=3,
              max_traj_len=T, use_gae=False, num_procs=N, max_grad_norm=0.05, mirror_coeff=0.4, eval_freq=10 ** 9)
    with tempfile.TemporaryDirectory() as tmp:
        ppo = PPO(hp, tmp)
        torch.manual_seed(0)
        pi, vf = MLPGaussianActor(41, 12).cuda(), MLPCritic(41).cuda()
        pi.obs_mean, pi.obs_std = torch.zeros(41, device="cuda"), torch.ones(41, device="cuda")
        ppo.train(lambda: env, pi, vf, n_itr=2, verbose=False)        # every buffer live, the reset stream started
        path = os.path.join(tmp, ppo_checkpoint.FILE)
        out = dict(num_envs=N, T=T, reps=args.reps, update=ppo._run["update"],
                   state_dict=timed(lambda: ppo_checkpoint.state_dict(ppo, env), args.reps),
                   save=timed(lambda: ppo_checkpoint.save(path, ppo, env), args.reps))
        out["file_bytes"] = os.path.getsize(path)
        out["load"] = timed(lambda: ppo_checkpoint.load(path, ppo, env), args.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
