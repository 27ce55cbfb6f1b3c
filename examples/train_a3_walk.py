#!/usr/bin/env python3
"""PPO on StickFigureA3 with the reference's command line
(reference: examples/reinforcement_learning_ppo/a3/train_a3_walk.py).

    python examples/train_a3_walk.py train --num_procs 4096 --n_itr 10 --logdir ./logs_dir/
    python examples/train_a3_walk.py train ... --checkpoint_every 100        # LOGDIR/checkpoint.pt, replaced every 100 iterations
    python examples/train_a3_walk.py train ... --resume ./logs_dir/          # the stopped run goes on, bit for bit
    python examples/train_a3_walk.py train ... --continued ./logs_dir/       # its weights, a new run from iteration 0
    python examples/train_a3_walk.py train ... --reset_draw device           # reset records drawn on the device (K23)

--resume continues a run exactly (weights, Adam, environment, random streams, logs: olympic_hip.ppo_checkpoint) and needs the
same command line as the run that wrote the file.  --continued has the reference's meaning (train_a3_walk.py:54-64): the
weights and input-normalisation tables of an earlier run, a fresh optimiser, iteration 0; it reads checkpoint.pt (a file, or
the one in a directory), never a pickled module.  Either one skips the normalisation pre-pass, as the reference does.

`--num_procs` is the number of environments stepped in lock step on the GPU (the reference starts
that many ray workers).  MuJoCo is not part of this repository: `make_physics(num_envs)` below
returns the synthetic readback used by the tests; plug a MuJoCo-backed object with the same
four members (see olympic_hip.a3.StickFigureA3) to train for real."""
import argparse
import os
import sys
from functools import partial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "olympics-mujoco_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from olympic_hip.a3 import AlgorithmType, ReplayA3Physics, StickFigureA3  # noqa: E402
from olympic_hip.ppo import PPO, MLPCritic, MLPGaussianActor  # noqa: E402
from olympic_hip.rollout import get_normalization_params  # noqa: E402
from olympic_hip.wrappers import SymmetricEnv  # noqa: E402


def make_physics(num_envs, seed=1):
    from bench_ppo_iter import synthetic_blocks
    return ReplayA3Physics(synthetic_blocks(num_envs, 32, torch.Generator(device="cuda").manual_seed(seed)))


def run_experiment(args):
    env_fn = partial(StickFigureA3, algorithm_type=AlgorithmType.REINFORCEMENT_LEARNING, num_envs=args.num_procs,
                     physics=make_physics(args.num_procs), reset_draw=getattr(args, "reset_draw", "host"),
                     reset_pool_depth=getattr(args, "reset_pool_depth", None))
    if not args.no_mirror:
        probe = env_fn()
        env_fn = partial(SymmetricEnv, env_fn, mirrored_obs=probe.robot.mirrored_obs,
                         mirrored_act=probe.robot.mirrored_acts, clock_inds=probe.robot.clock_inds)
    obs_dim = env_fn().observation_space.shape[0]
    action_dim = env_fn().action_space.shape[0]
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    policy = MLPGaussianActor(obs_dim, action_dim, fixed_std=torch.exp(torch.tensor(float(args.std_dev)))).cuda()
    critic = MLPCritic(obs_dim).cuda()
    if args.continued:
        from olympic_hip import ppo_checkpoint
        ppo_checkpoint.load_policy(args.continued, policy, critic)
    if args.input_norm_steps > 0 and not (args.resume or args.continued):
        env = env_fn()
        mean, std = get_normalization_params(args.input_norm_steps, policy, env, 1.0)
        policy.obs_mean = torch.as_tensor(mean, dtype=torch.float32, device="cuda")
        policy.obs_std = torch.as_tensor(std, dtype=torch.float32, device="cuda")
    algo = PPO(vars(args), args.logdir)
    algo.use_graph = algo.use_graph_rollout = not args.no_graph
    return algo.train(env_fn, policy, critic, args.n_itr, anneal_rate=args.anneal, resume=args.resume,
                      checkpoint_every=args.checkpoint_every)


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    if len(sys.argv) < 2 or sys.argv[1] != "train":
        raise SystemExit("usage: train_a3_walk.py train [options]")
    sys.argv.remove(sys.argv[1])
    parser.add_argument("--seed", default=0, type=int)
    parser.add_argument("--logdir", type=str, default="./logs_dir/")
    parser.add_argument("--input_norm_steps", type=int, default=100000)
    parser.add_argument("--n_itr", type=int, default=20000)
    parser.add_argument("--lr", type=float, default=1e-4)
    parser.add_argument("--eps", type=float, default=1e-5)
    parser.add_argument("--lam", type=float, default=0.95)
    parser.add_argument("--gamma", type=float, default=0.99)
    parser.add_argument("--anneal", default=1.0, type=float)
    parser.add_argument("--std_dev", type=float, default=-1.5)
    parser.add_argument("--entropy_coeff", type=float, default=0.0)
    parser.add_argument("--clip", type=float, default=0.2)
    parser.add_argument("--minibatch_size", type=int, default=64)
    parser.add_argument("--epochs", type=int, default=3)
    parser.add_argument("--use_gae", type=bool, default=True)
    parser.add_argument("--num_procs", type=int, default=12)
    parser.add_argument("--max_grad_norm", type=float, default=0.05)
    parser.add_argument("--max_traj_len", type=int, default=400)
    parser.add_argument("--no_mirror", action="store_true")
    parser.add_argument("--mirror_coeff", default=0.4, type=float)
    parser.add_argument("--eval_freq", default=100, type=int)
    parser.add_argument("--no_graph", action="store_true", help="op-by-op PyTorch update / rollout instead of HIP graphs")
    parser.add_argument("--continued", default=None, type=str,
                        help="checkpoint.pt (or its directory) to take weights and normalisation tables from")
    parser.add_argument("--resume", default=None, type=str, help="checkpoint.pt (or its directory) to continue exactly")
    parser.add_argument("--reset_draw", default="host", choices=["host", "device"],
                        help="where the walking task's reset records are drawn: numpy on the host, or K23 on the device")
    parser.add_argument("--reset_pool_depth", default=None, type=lambda v: v if v == "rollout" else int(v),
                        help="reset records kept per environment (default 4 on the host, 32 on the device); with "
                             "--reset_draw device, 'rollout' keeps one per step so that none is used twice")
    parser.add_argument("--checkpoint_every", default=None, type=int, help="write LOGDIR/checkpoint.pt every K iterations")
    args = parser.parse_args()
    if args.resume and args.continued:
        raise SystemExit("--resume continues a run, --continued starts a new one from its weights: give one of them")
    hist = run_experiment(args)
    if hist:
        print("done:", len(hist), "iterations; last return", hist[-1]["ep_return"], "fps", round(hist[-1]["fps"]))
    else:
        print("done: the checkpoint already holds iteration", args.n_itr - 1, "or later; nothing left to run")
