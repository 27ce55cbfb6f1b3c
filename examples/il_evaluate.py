#!/usr/bin/env python3
"""Evaluate a saved imitation-learning agent (examples/imitation_learning/evaluate_save_npz.py:93-104 without the
recording): build the agent as examples/il_experiment.py does, load a file il_checkpoint wrote into it,
core.evaluate(n_episodes), print the launcher's three scalars.

    python examples/il_evaluate.py results/agent_epoch_3_J_12.500000.pt --algo gail --num_envs 256 --n_episodes 50

Only the agent is taken from the file: the evaluation starts from a full reset with this script's own seed, as the
reference's does from Agent.load.  --algo, and the environment's sizes, must be those of the run that wrote the file; a
mismatch is refused with the field's name.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "olympics-mujoco_amd"))
import torch  # noqa: E402

from il_experiment import build_agent  # noqa: E402  (the example beside this one)
from olympic_hip import il_checkpoint  # noqa: E402
from olympic_hip.envs import LocoEnvBase  # noqa: E402
from olympic_hip.il_core import ILCore  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("path", help="a file written by il_checkpoint.save / BestAgentSaver")
    ap.add_argument("--algo", choices=("gail", "vail"), default="gail")
    ap.add_argument("--num_envs", type=int, default=256)
    ap.add_argument("--n_episodes", type=int, default=50)
    ap.add_argument("--horizon", type=int, default=0, help="replace the environment's horizon (0: keep the spec's 1000)")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    torch.manual_seed(args.seed)
    env = LocoEnvBase.make("UnitreeH1.walk.real", num_envs=args.num_envs, seed=args.seed)
    vec = env.vec
    if args.horizon > 0:
        vec.spec.horizon = vec.info.horizon = args.horizon
    agent, policy = build_agent(args.algo, env, False)
    meta = il_checkpoint.load(args.path, agent)
    print(f"loaded {args.path}: iteration {agent.iter}, meta {meta}")
    core = ILCore(agent, vec, policy, generator=torch.Generator(device="cuda").manual_seed(args.seed))
    ev = core.evaluate(n_episodes=args.n_episodes)
    print(f"evaluated {ev['n_episodes']} episodes, {ev['n_steps']} steps")
    print(f"Eval_R-stochastic: {ev['R_mean']:.6g}")
    print(f"Eval_J-stochastic: {ev['J_mean']:.6g}")
    print(f"Eval_L-stochastic: {ev['L']:.6g}")


if __name__ == "__main__":
    main()
