#!/usr/bin/env python3
"""VAILAgent.fit on UnitreeH1: one GAIL_TRPO.fit (imitation_lib/imitation/gail_TRPO.py:105-165) per call with the
discriminator reward (K12), GAE + advantage normalisation (K6 + K7) and the critic's evaluation and fit (K16) on the
GPU.  The policy step is the caller's.  By default it is a stand-in that only reports the advantages it was handed, and
the policy is a random one on the kinematic stand-in physics.  With --policy device the actions come from a
DeviceGaussianPolicy (obs -> [512, 256] -> act, std_0 0.5) and DeviceTRPO (K17) trains it with UnitreeH1's confs.yaml
values (max_kl 5e-3, ent_coeff 1e-3, n_epochs_cg 25).

    python examples/vail_fit.py --num_envs 4096 --steps 100 --iters 3 [--disc-fit device] [--policy device] [--log]
                                [--disc_use_next_states] [--disc_only_states False]

--disc_use_next_states gives the discriminator (state, next state) (64 columns for H1's 32-column kinematic mask),
--disc_only_states False gives it (state, action); both need --disc-fit device (K15), and the agent then hands
next_state or action to the reward and the trainer by itself.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "olympics-mujoco_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from olympic_hip.envs import LocoEnvBase  # noqa: E402
from olympic_hip.gail import (DeviceStandardizer, DiscriminatorReward, DiscriminatorTrainer,  # noqa: E402
                              VariationalDiscriminator, VDBLoss)
from olympic_hip.il_agent import (DeviceDiscriminatorTrainer, DeviceGaussianPolicy, DeviceILCritic,  # noqa: E402
                                  DeviceTRPO, VAILAgent, episode_stats)


def policy_step(obs, act, adv, agent):
    """The caller's TRPO step would go here; this one only looks at its inputs."""
    print(f"  policy_step: {obs.shape[0]} rows, advantage mean {float(adv.mean()):+.2e} "
          f"std {float(adv.std(unbiased=False)):.4f}")


class PrintingWriter:
    """The part of a SummaryWriter the agent uses: add_scalar, printed."""

    def add_scalar(self, tag, value, step):
        print(f"    [{step}] {tag}: {value:.6g}")


def paired_inputs(args, env, mask, n_act):
    """(pair, act_mask, demonstrations, network width) for the two switches.  Both together is the reference's refused
    three-part combination (gail_TRPO.py:195-196): the reward's constructor raises OlyError for it."""
    pair = "next_state" if args.disc_use_next_states else (None if args.disc_only_states else "action")
    act_mask = None if args.disc_only_states else np.arange(n_act)
    ds = env.create_dataset()
    if pair is None:
        return None, None, ds["states"], len(mask)
    key = "next_states" if pair == "next_state" else "actions"
    if ds.get(key) is None:
        raise SystemExit(f"the dataset of this task holds no `{key}`")
    width = 2 * len(mask) if pair == "next_state" else len(mask) + n_act
    return pair, act_mask, {"states": ds["states"], key: ds[key]}, width


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--disc-fit", choices=("torch", "device"), default="torch",
                    help="the discriminator's training: DiscriminatorTrainer (torch) or DeviceDiscriminatorTrainer (K15)")
    ap.add_argument("--policy", choices=("random", "device"), default="random",
                    help="random actions and a stand-in policy step, or DeviceGaussianPolicy trained by DeviceTRPO (K17)")
    ap.add_argument("--disc_use_next_states", action="store_true",
                    help="the discriminator sees (state, next state), as confs.yaml sets for UnitreeA1 (disc_use_next_states)")
    ap.add_argument("--disc_only_states", type=lambda s: s.lower() in ("1", "true", "yes"), default=True,
                    help="False: the discriminator sees (state, action) (disc_only_states of the reference's launcher); needs a "
                         "dataset with `actions`, which the bundled task's trajectory does not hold")
    ap.add_argument("--log", action="store_true",
                    help="give the agent a writer, as the reference's launcher does: the discriminator's diagnostics "
                         "(_discriminator_logging, K19) run after every discriminator epoch and are printed; needs "
                         "--disc-fit device.  With --policy device the iteration's diagnostics (_logging_sw, K20: the "
                         "episode means, vf_loss, entropy, kl) run and are printed as well")
    args = ap.parse_args()
    if args.log and args.disc_fit != "device":
        raise SystemExit("--log needs --disc-fit device (the torch trainer has no diagnostics)")
    torch.manual_seed(0)
    env = LocoEnvBase.make("UnitreeH1.walk.real", num_envs=args.num_envs, seed=0)
    vec, eng = env.vec, env.vec.eng
    gen = torch.Generator(device="cuda").manual_seed(0)
    n_obs, n_act = vec.spec.n_obs, vec.spec.n_act
    mask = vec.get_kinematic_obs_mask()
    pair, act_mask, demo, width = paired_inputs(args, env, mask, n_act)
    if pair is None:
        disc = DiscriminatorReward(eng, VariationalDiscriminator(n_obs).cuda(), state_mask=mask)
    else:
        if args.disc_fit != "device":
            raise SystemExit("a paired discriminator input is fitted by --disc-fit device (K15)")
        disc = DiscriminatorReward(eng, VariationalDiscriminator(width).cuda(), state_mask=mask, pair=pair,
                                   act_mask=act_mask)
    if args.disc_fit == "device":     # the reference's minibatch loop, disc_batch_size 2048 (confs.yaml)
        trainer = DeviceDiscriminatorTrainer(disc, demo, VDBLoss(info_constraint=0.1, lr_beta=1e-5), lr=5e-5,
                                             batch_size=2048)
    else:
        trainer = DiscriminatorTrainer(disc, demo, VDBLoss(info_constraint=0.1, lr_beta=1e-5), lr=5e-5)
    # the critic of examples/imitation_learning/utils.py:136-149: obs -> [512, 256] -> 1, the policy's standardizer
    lins = [torch.nn.Linear(n_obs, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 1)]
    trpo_standardizer = DeviceStandardizer(eng, n_obs)
    critic = DeviceILCritic(eng, lins, trpo_standardizer, lr=1e-4)
    step, policy = policy_step, None
    if args.policy == "device":     # the policy of utils.py:126-134 with UnitreeH1's confs.yaml values
        pol_lins = [torch.nn.Linear(n_obs, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, n_act)]
        policy = DeviceGaussianPolicy(eng, pol_lins, trpo_standardizer, std_0=0.5)
        step = DeviceTRPO(policy, max_kl=5e-3, ent_coeff=1e-3, n_epochs_cg=25)
    agent = VAILAgent(eng, disc, trainer, critic, step, gamma=0.99, lam=0.97, env_reward_frac=0.0,
                      train_D_n_th_epoch=3, critic_fit_params=dict(n_epochs=3, batch_size=256),
                      sw=PrintingWriter() if args.log else None, iteration_log=args.log and policy is not None)
    T, N = args.steps, args.num_envs
    x = torch.empty((T + 1, N, n_obs), dtype=torch.float32, device="cuda")
    act = torch.empty((T, N, n_act), dtype=torch.float32, device="cuda")
    r_env = torch.empty((T, N), dtype=torch.float32, device="cuda")
    absorbing = torch.empty((T, N), dtype=torch.bool, device="cuda")
    last = torch.empty((T, N), dtype=torch.bool, device="cuda")
    x[0] = vec.reset().to(torch.float32)
    for it in range(args.iters):
        for t in range(T):
            if policy is None:
                act[t].uniform_(-1, 1, generator=gen)
            else:
                act[t] = policy.draw_action(x[t], generator=gen)
            o, r, a, info = vec.step(act[t])
            x[t + 1], r_env[t], absorbing[t], last[t] = o.to(torch.float32), r, a, info["last"]
        last[-1] = True
        ep = episode_stats(eng, r_env, last).tolist()      # compute_J / compute_episodes_length of the rollout (K20)
        print(f"rollout {it}: {ep[3]:.0f} episodes, mean return {ep[0]:.4f}, mean length {ep[2]:.2f} over {ep[4]:.0f} completed")
        out = agent.fit(dict(state=x[:-1], action=act, reward=r_env, next_state=x[1:], absorbing=absorbing, last=last),
                        generator=gen)
        loss = out["critic_loss"]
        print(f"iter {it}: reward mean {float(out['reward'].mean()):.4f}; critic loss {float(loss[0, 0]):.4f} -> "
              f"{float(loss[-1, -1]):.4f} over {loss.numel()} minibatches; discriminator trained: {out['disc_trained']}")
        if policy is not None:
            sc = step.scalars()
            improve = sc["J"] - sc["prev_loss"]
            ok = sc["kl"] <= 1.5 * 5e-3 or improve >= 0
            print(f"  TRPO: CG iterations {sc['cg_iters']:.0f}, accepted j {sc['accepted_j']:.0f}, kl {sc['kl']:.3e}, "
                  f"improvement {improve:+.3e}" + ("" if sc["accepted_j"] < 0 or ok else "  (acceptance rule violated)"))
        x[0] = x[-1]
    critic.sync_to_torch()
    if policy is not None:
        policy.sync_to_torch()


if __name__ == "__main__":
    main()
