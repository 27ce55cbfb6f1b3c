#!/usr/bin/env python3
"""Behavioural cloning (imitation_lib/imitation/offline/behavioral_cloning.py) on UnitreeH1's observations: a teacher
policy acts in the environment, its (state, action) blocks become the demonstrations, and a fresh squashed-Gaussian
student (IQ_Learn_Policy, imitation_lib/imitation/iq_sac.py) is fitted to them by DeviceBehavioralCloning, every step of
a fit_offline call on the GPU (K24, oly_bc_fit_steps).  Both are then scored by ILCore.evaluate, as the reference's
launcher scores an agent (Eval_R / Eval_J / Eval_L).

The teacher is a DeviceGaussianPolicy with random weights (there is no trained walker in the repository), and the physics
is the kinematic stand-in, so the returns say nothing about walking: what the example shows is the student's loss falling
and the whole pipeline running on the device.

    python examples/bc_fit.py --envs 1024 --collect 20 --steps 1000 [--batch 32] [--log] [--json FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "olympics-mujoco_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from olympic_hip.bc import DeviceBehavioralCloning, DeviceSquashedGaussianPolicy  # noqa: E402
from olympic_hip.envs import LocoEnvBase  # noqa: E402
from olympic_hip.gail import DeviceStandardizer  # noqa: E402
from olympic_hip.il_agent import DeviceGaussianPolicy  # noqa: E402
from olympic_hip.il_core import ILCore  # noqa: E402
from vail_fit import PrintingWriter  # noqa: E402  (the example beside this one)


class Collector:
    """The `agent` of the collection loop: its fit keeps the [T,N] blocks ILCore hands over."""

    def __init__(self):
        self.blocks = []

    def fit(self, dataset, generator=None):
        self.blocks.append(dict(state=dataset["state"].clone(), action=dataset["action"].clone()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--collect", type=int, default=20, help="vec steps the teacher acts for: the demonstrations are [T,N] blocks")
    ap.add_argument("--steps", type=int, default=1000, help="fit_offline iterations")
    ap.add_argument("--batch", type=int, default=32, help="the reference's default batch_size")
    ap.add_argument("--calls", type=int, default=4, help="fit_offline calls the iterations are cut into")
    ap.add_argument("--eval-episodes", type=int, default=0, help="episodes per ILCore.evaluate (default: one per environment)")
    ap.add_argument("--horizon", type=int, default=20, help="the environment's horizon for this example (0: the spec's 1000)")
    ap.add_argument("--log", action="store_true", help="print the trainer's scalars under the reference's names")
    ap.add_argument("--fused-act", action="store_true", help="the student acts through one oly_sg_act call per vec step (K25)")
    ap.add_argument("--empirical-entropy", action="store_true",
                    help="the whole of the reference's logging(): the sampled second forward of the logged iterations (K25)")
    ap.add_argument("--json", default=None, metavar="FILE", help="write the run's figures to FILE")
    args = ap.parse_args()
    torch.manual_seed(0)
    env = LocoEnvBase.make("UnitreeH1.walk.real", num_envs=args.envs, seed=0)
    vec, eng = env.vec, env.vec.eng
    if args.horizon > 0:
        vec.spec.horizon = vec.info.horizon = args.horizon
    gen = torch.Generator(device="cuda").manual_seed(0)
    n_obs, n_act = vec.spec.n_obs, vec.spec.n_act
    space = vec.info.action_space
    # ---- the teacher acts; its blocks are the demonstrations
    t_lins = [torch.nn.Linear(n_obs, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, n_act)]
    teacher = DeviceGaussianPolicy(eng, t_lins, DeviceStandardizer(eng, n_obs), std_0=0.3)
    collector = Collector()
    ILCore(collector, vec, teacher, generator=gen).learn(n_steps=args.collect, n_steps_per_fit=args.collect)
    blk = collector.blocks[0]
    demo = dict(states=blk["state"].reshape(-1, n_obs), actions=blk["action"].reshape(-1, n_act))
    print(f"demonstrations: {demo['states'].shape[0]} rows from {args.collect} steps of {args.envs} environments")
    # ---- the student: in -> [512, 256] -> 2A with its own Standardizer, the reference's defaults
    s_lins = [torch.nn.Linear(n_obs, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 2 * n_act)]
    student = DeviceSquashedGaussianPolicy(eng, s_lins, np.asarray(space.low), np.asarray(space.high),
                                           standardizer=DeviceStandardizer(eng, n_obs), fused_act=args.fused_act)
    bc = DeviceBehavioralCloning(eng, student, demo, lr=1e-3, batch_size=args.batch,
                                 logging_iter=max(1, args.steps // 10), sw=PrintingWriter() if args.log else None,
                                 empirical_entropy=args.empirical_entropy)
    calls = max(1, min(args.calls, args.steps))
    outs = [bc.fit_offline(args.steps // calls + (i < args.steps % calls), generator=gen) for i in range(calls)]
    out = torch.cat(outs).cpu().numpy()
    k = max(1, len(out) // 10)
    first, last = float(out[:k, 0].mean()), float(out[-k:, 0].mean())
    print(f"student: {bc.step} Adam steps at batch {bc.batch}; GaussianNLLLoss {first:.4f} -> {last:.4f} (means of {k}), "
          f"mse {float(out[:k, 2].mean()):.4f} -> {float(out[-k:, 2].mean()):.4f}")
    # ---- both through the launcher's evaluation
    n_eval = args.eval_episodes or args.envs
    rec = dict(rows=int(demo["states"].shape[0]), steps=int(bc.step), batch=int(bc.batch), loss_first=first, loss_last=last)
    for name, pol in (("teacher", teacher), ("student", student)):
        ev = ILCore(collector, vec, pol, generator=gen).evaluate(n_episodes=n_eval)
        print(f"{name}: Eval_R {ev['R_mean']:.4f}  Eval_J {ev['J_mean']:.4f}  Eval_L {ev['L']:.2f} over {ev['n_episodes']} episodes")
        rec[name] = dict(R=ev["R_mean"], J=ev["J_mean"], L=ev["L"])
    student.sync_to_torch()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rec, f)


if __name__ == "__main__":
    main()
