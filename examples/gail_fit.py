#!/usr/bin/env python3
"""GAILAgent.fit on UnitreeH1's observations with GAIL's own discriminator: one GAIL_TRPO.fit
(imitation_lib/imitation/gail_TRPO.py:105-165) per call with the discriminator reward (K18: in -> 512 -> 256 -> 1, tanh),
GAE + advantage normalisation (K6 + K7) and the critic's evaluation and fit (K16) on the GPU.  The hyperparameters are
HumanoidMuscle's of confs.yaml, the environment the reference configures for GAIL: lr_disc 5e-6, d_entr_coef 1e-3,
max_kl 1e-2, std_0 0.8.  The policy step is the caller's.  By default it is a stand-in that only reports the advantages
it was handed, and the policy is a random one on the kinematic stand-in physics.  With --policy device the actions come
from a DeviceGaussianPolicy (obs -> [512, 256] -> act) and DeviceTRPO (K17) trains it.

    python examples/gail_fit.py --num_envs 4096 --steps 100 --iters 3 [--disc-fit device] [--policy device] [--log]
                                [--disc_use_next_states] [--disc_only_states False]

--disc_use_next_states gives the discriminator (state, next state) (64 columns for H1's 32-column kinematic mask),
--disc_only_states False gives it (state, action); the agent then hands next_state or action to the reward and the
trainer by itself.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "olympics-mujoco_amd"))
import torch  # noqa: E402

from olympic_hip.envs import LocoEnvBase  # noqa: E402
from olympic_hip.gail import DeviceStandardizer, GAILDiscriminator, GAILDiscriminatorReward  # noqa: E402
from olympic_hip.il_agent import (DeviceGAILDiscriminatorTrainer, DeviceGaussianPolicy, DeviceILCritic,  # noqa: E402
                                  DeviceTRPO, GAILAgent, episode_stats)
from vail_fit import PrintingWriter, paired_inputs  # noqa: E402  (the example beside this one: the two switches mean the same there)


def policy_step(obs, act, adv, agent):
    """The caller's TRPO step would go here; this one only looks at its inputs."""
    print(f"  policy_step: {obs.shape[0]} rows, advantage mean {float(adv.mean()):+.2e} "
          f"std {float(adv.std(unbiased=False)):.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--disc-fit", choices=("none", "device"), default="device",
                    help="the discriminator's training: DeviceGAILDiscriminatorTrainer (K18), or none (a frozen discriminator)")
    ap.add_argument("--policy", choices=("random", "device"), default="random",
                    help="random actions and a stand-in policy step, or DeviceGaussianPolicy trained by DeviceTRPO (K17)")
    ap.add_argument("--disc_use_next_states", action="store_true",
                    help="the discriminator sees (state, next state), as confs.yaml sets for UnitreeA1 (disc_use_next_states)")
    ap.add_argument("--disc_only_states", type=lambda s: s.lower() in ("1", "true", "yes"), default=True,
                    help="False: the discriminator sees (state, action) (disc_only_states of the reference's launcher); needs a "
                         "dataset with `actions`, which the bundled task's trajectory does not hold")
    ap.add_argument("--log", action="store_true",
                    help="give the agent a writer, as the reference's launcher does: the discriminator's diagnostics "
                         "(_discriminator_logging, K19) run after every discriminator epoch and are printed.  With "
                         "--policy device the iteration's diagnostics (_logging_sw, K20: the episode means, vf_loss, "
                         "entropy, kl) run and are printed as well")
    args = ap.parse_args()
    torch.manual_seed(0)
    env = LocoEnvBase.make("UnitreeH1.walk.real", num_envs=args.num_envs, seed=0)
    vec, eng = env.vec, env.vec.eng
    gen = torch.Generator(device="cuda").manual_seed(0)
    n_obs, n_act = vec.spec.n_obs, vec.spec.n_act
    mask = vec.get_kinematic_obs_mask()
    pair, act_mask, demo, width = paired_inputs(args, env, mask, n_act)
    disc = GAILDiscriminatorReward(eng, GAILDiscriminator(width).cuda(), state_mask=mask, pair=pair, act_mask=act_mask)
    # the reference's minibatch loop, disc_batch_size 2048 (confs.yaml); the trainer exists either way, "none" never calls it
    trainer = DeviceGAILDiscriminatorTrainer(disc, demo, entcoeff=1e-3, lr=5e-6, batch_size=2048)
    # the critic of examples/imitation_learning/utils.py:136-149: obs -> [512, 256] -> 1, the policy's standardizer
    lins = [torch.nn.Linear(n_obs, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 1)]
    trpo_standardizer = DeviceStandardizer(eng, n_obs)
    critic = DeviceILCritic(eng, lins, trpo_standardizer, lr=1e-4)
    step, policy = policy_step, None
    if args.policy == "device":     # the policy of utils.py:126-134 with HumanoidMuscle's confs.yaml values
        pol_lins = [torch.nn.Linear(n_obs, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, n_act)]
        policy = DeviceGaussianPolicy(eng, pol_lins, trpo_standardizer, std_0=0.8)
        step = DeviceTRPO(policy, max_kl=1e-2, ent_coeff=1e-3, n_epochs_cg=25)
    agent = GAILAgent(eng, disc, trainer, critic, step, gamma=0.99, lam=0.97, env_reward_frac=0.0,
                      train_D_n_th_epoch=3 if args.disc_fit == "device" else 10 ** 9,
                      critic_fit_params=dict(n_epochs=3, batch_size=256), sw=PrintingWriter() if args.log else None,
                      iteration_log=args.log and policy is not None)
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
              f"{float(loss[-1, -1]):.4f} over {loss.numel()} minibatches; discriminator trained: {out['disc_trained']}"
              + (f", loss {float(out['disc_loss'][0, 0]):.4f} -> {float(out['disc_loss'][-1, -1]):.4f}"
                 if out["disc_trained"] else ""))
        if policy is not None:
            sc = step.scalars()
            improve = sc["J"] - sc["prev_loss"]
            ok = sc["kl"] <= 1.5 * 1e-2 or improve >= 0
            print(f"  TRPO: CG iterations {sc['cg_iters']:.0f}, accepted j {sc['accepted_j']:.0f}, kl {sc['kl']:.3e}, "
                  f"improvement {improve:+.3e}" + ("" if sc["accepted_j"] < 0 or ok else "  (acceptance rule violated)"))
        x[0] = x[-1]
    critic.sync_to_torch()
    if policy is not None:
        policy.sync_to_torch()


if __name__ == "__main__":
    main()
