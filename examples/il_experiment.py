#!/usr/bin/env python3
"""The imitation-learning launcher's loop (examples/imitation_learning/experiment.py:51-67) on UnitreeH1 with ILCore:

    for epoch: core.learn(n_steps, n_steps_per_fit); core.evaluate(n_episodes) -> Eval_R / Eval_J / Eval_L
               agent_saver.save(core.agent, R_mean)
    agent_saver.save_curr_best_agent()

Collection acts through DeviceGaussianPolicy.act (K21: statistics update, mean network, Gaussian sample and the control
vector in one call), resets every environment whose episode ended (one launch, K22: VecLocoEnv.reset_where; --host-reset
selects the former host-driven reset with its flag read-back per step), and hands separate state / next_state blocks to
GAILAgent.fit or VAILAgent.fit (K12 / K18, K6 + K7, K16, K17, K15 / K18, K19 / K20).  The networks and hyperparameters
are those of examples/gail_fit.py (--algo gail) and examples/vail_fit.py (--algo vail) with --policy device and
--disc-fit device.  The physics is the kinematic stand-in.

With --results_dir the best agent since the last write is kept by il_checkpoint.BestAgentSaver, the reference's schedule
(--n_epochs_save, default 500 as experiment.py:25; -1: never), as agent_epoch_%d_J_%f.pt; the files hold the core as well,
so --resume FILE continues such a run bit for bit at the epoch after the file's (same --algo, --num_envs and --horizon).

    python examples/il_experiment.py --algo gail --num_envs 256 --steps_per_fit 20 --fits_per_epoch 3 --eval_episodes 50
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "olympics-mujoco_amd"))
import torch  # noqa: E402

from olympic_hip.envs import LocoEnvBase  # noqa: E402
from olympic_hip.gail import (DeviceStandardizer, DiscriminatorReward, GAILDiscriminator,  # noqa: E402
                              GAILDiscriminatorReward, VariationalDiscriminator, VDBLoss)
from olympic_hip.il_agent import (DeviceDiscriminatorTrainer, DeviceGAILDiscriminatorTrainer,  # noqa: E402
                                  DeviceGaussianPolicy, DeviceILCritic, DeviceTRPO, GAILAgent, VAILAgent)
from olympic_hip import il_checkpoint  # noqa: E402
from olympic_hip.il_core import ILCore  # noqa: E402
from vail_fit import PrintingWriter, paired_inputs  # noqa: E402  (the examples beside this one)


def build_agent(algo, env, log, sw=None):
    """(agent, policy) as examples/gail_fit.py / examples/vail_fit.py build them for --policy device --disc-fit device.
    log: the agent gets a writer (sw, or a PrintingWriter) and runs its diagnostics."""
    vec, eng = env.vec, env.vec.eng
    n_obs, n_act = vec.spec.n_obs, vec.spec.n_act
    mask = vec.get_kinematic_obs_mask()
    switches = argparse.Namespace(disc_use_next_states=False, disc_only_states=True)
    _, _, demo, width = paired_inputs(switches, env, mask, n_act)
    lins = [torch.nn.Linear(n_obs, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 1)]
    trpo_standardizer = DeviceStandardizer(eng, n_obs)
    critic = DeviceILCritic(eng, lins, trpo_standardizer, lr=1e-4)
    pol_lins = [torch.nn.Linear(n_obs, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, n_act)]
    sw = (sw or PrintingWriter()) if log else None
    common = dict(gamma=0.99, lam=0.97, env_reward_frac=0.0, train_D_n_th_epoch=3,
                  critic_fit_params=dict(n_epochs=3, batch_size=256), sw=sw, iteration_log=log)
    if algo == "gail":       # HumanoidMuscle's confs.yaml values, as examples/gail_fit.py
        disc = GAILDiscriminatorReward(eng, GAILDiscriminator(width).cuda(), state_mask=mask)
        trainer = DeviceGAILDiscriminatorTrainer(disc, demo, entcoeff=1e-3, lr=5e-6, batch_size=2048)
        policy = DeviceGaussianPolicy(eng, pol_lins, trpo_standardizer, std_0=0.8)
        step = DeviceTRPO(policy, max_kl=1e-2, ent_coeff=1e-3, n_epochs_cg=25)
        return GAILAgent(eng, disc, trainer, critic, step, **common), policy
    disc = DiscriminatorReward(eng, VariationalDiscriminator(n_obs).cuda(), state_mask=mask)   # UnitreeH1's, as vail_fit.py
    trainer = DeviceDiscriminatorTrainer(disc, demo, VDBLoss(info_constraint=0.1, lr_beta=1e-5), lr=5e-5, batch_size=2048)
    policy = DeviceGaussianPolicy(eng, pol_lins, trpo_standardizer, std_0=0.5)
    step = DeviceTRPO(policy, max_kl=5e-3, ent_coeff=1e-3, n_epochs_cg=25)
    return VAILAgent(eng, disc, trainer, critic, step, **common), policy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--algo", choices=("gail", "vail"), default="gail")
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--steps_per_fit", type=int, default=100, help="vec steps per fit: every environment adds that many samples")
    ap.add_argument("--fits_per_epoch", type=int, default=3)
    ap.add_argument("--eval_episodes", type=int, default=50)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--horizon", type=int, default=0, help="replace the environment's horizon (0: keep the spec's 1000)")
    ap.add_argument("--host-reset", action="store_true",
                    help="reset ended episodes from the host (one read-back per vec step) instead of one launch (K22)")
    ap.add_argument("--log", action="store_true", help="print the agent's own diagnostics (K19 / K20) as well")
    ap.add_argument("--results_dir", default=None, help="where BestAgentSaver writes agent_epoch_%%d_J_%%f.pt (default: nothing "
                                                        "is written)")
    ap.add_argument("--n_epochs_save", type=int, default=500,
                    help="write the best agent since the last write once this many epochs have passed (-1: never)")
    ap.add_argument("--resume", default=None, metavar="PATH",
                    help="a file this launcher wrote: load agent and core and continue at the epoch after the file's")
    args = ap.parse_args()
    torch.manual_seed(0)
    env = LocoEnvBase.make("UnitreeH1.walk.real", num_envs=args.num_envs, seed=0)
    vec = env.vec
    if args.horizon > 0:
        vec.spec.horizon = vec.info.horizon = args.horizon
    gen = torch.Generator(device="cuda").manual_seed(0)
    agent, policy = build_agent(args.algo, env, args.log)
    core = ILCore(agent, vec, policy, generator=gen, device_reset=False if args.host_reset else None)
    saver = il_checkpoint.BestAgentSaver(args.results_dir, args.n_epochs_save) if args.results_dir else None
    first = 0
    if args.resume:
        meta = il_checkpoint.load(args.resume, agent, core)
        first = int(meta["epoch"]) + 1
        print(f"resumed from {args.resume}: epoch {meta['epoch']}, J {meta['J']:.6f}; continuing at epoch {first}")
        if saver is not None:           # the epochs before `first` belong to the run that wrote the file
            saver.epoch_counter = saver.last_save = first
    sw = PrintingWriter()
    for epoch in range(first, args.epochs):
        outs = core.learn(n_steps=args.steps_per_fit * args.fits_per_epoch, n_steps_per_fit=args.steps_per_fit)
        for i, out in enumerate(outs):
            loss = out["critic_loss"]
            print(f"epoch {epoch} fit {i}: reward mean {float(out['reward'].mean()):.4f}; critic loss "
                  f"{float(loss[0, 0]):.4f} -> {float(loss[-1, -1]):.4f}; discriminator trained: {out['disc_trained']}")
        ev = core.evaluate(n_episodes=args.eval_episodes)
        print(f"epoch {epoch}: evaluated {ev['n_episodes']} episodes, {ev['n_steps']} steps")
        sw.add_scalar("Eval_R-stochastic", ev["R_mean"], epoch)
        sw.add_scalar("Eval_J-stochastic", ev["J_mean"], epoch)
        sw.add_scalar("Eval_L-stochastic", ev["L"], epoch)
        if saver is not None:           # experiment.py:65
            path = saver.save(agent, ev["R_mean"], core=core)
            if path:
                print(f"epoch {epoch}: wrote {path}")
    if saver is not None:               # experiment.py:67
        path = saver.save_curr_best_agent()
        if path:
            print(f"wrote {path}")


if __name__ == "__main__":
    main()
