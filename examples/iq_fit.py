#!/usr/bin/env python3
"""IQ-Learn (imitation_lib/imitation/iq_sac.py), SQIL (imitation_lib/imitation/sqil_sac.py) or LSIQ
(imitation_lib/imitation/lsiq.py) whole on synthetic
transitions (olympic_hip.synthetic, as examples/iq_q_fit.py): DeviceIQSAC.fit runs iq_update on the GPU, the critic update
(the policy passes of K25 and one oly_iq_q_update, K26) and the policy update (one oly_iq_pi_update, K27; with
--learnable-alpha one oly_iq_alpha_update after it).  The expert's and the policy's transitions are seeded stand-ins; the
policy that is trained does not collect them.

    python examples/iq_fit.py --algo iq|sqil|lsiq [--learnable-alpha] [--log] [--updates 200] [--batch 32] [--json FILE]
    python examples/iq_fit.py --algo iqfo|lsiqfo|lsiqfo_h|lsiqfo_hc [--am-lr] [--am-batch] [--am-fits-per-step] [--interpolate C]
    python examples/iq_fit.py --algo lsiq_h|lsiq_hc --q-exp-loss MSE [--h-loss-mode MSE|Huber] [--h-tau 0.005]
        (LSIQ_H / LSIQ_HC, lsiq_h.py / lsiq_hc.py: a second critic H learns the entropy, the actor follows Q + H)
    python examples/iq_fit.py --algo lsiq --q-exp-loss MSE|Huber [--lossq-type iq_like|sqil_like]
        [--loss-mode-exp fix|bootstrap] [--q-min -1] [--q-max 1] [--no-target-clipping] [--plcy-loss-mode MODE]
    python examples/iq_fit.py --algo lsiq_offline --n-steps K --q-exp-loss MSE|Huber [--regularizer-mode off|exp|exp_and_plcy]
        (LSIQ_Offline, imitation_lib/imitation/offline/lsiq_offline.py: DeviceLSIQOffline.fit_offline trains from the
        demonstrations alone, K26 with plcy_loss_mode v0 on all-expert batches of --batch rows)
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "olympics-mujoco_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from olympic_hip import _abi  # noqa: E402
from olympic_hip.bc import DeviceSquashedGaussianPolicy  # noqa: E402
from olympic_hip.engine import Engine  # noqa: E402
from olympic_hip.gail import DeviceStandardizer  # noqa: E402
from olympic_hip.iq import (DeviceIQSAC, DeviceLSIQHCSAC, DeviceLSIQHSAC, DeviceLSIQSAC, DeviceSoftQCritic,  # noqa: E402
                            DeviceSQILSAC)
from olympic_hip.synthetic import il_synthetic_transitions  # noqa: E402


class PrintingWriter:
    def add_scalar(self, name, value, it):
        print(f"  [{it}] {name} = {value:.6g}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--algo", choices=("iq", "sqil", "lsiq", "lsiq_h", "lsiq_hc", "iqfo", "lsiqfo", "lsiqfo_h", "lsiqfo_hc",
                                       "lsiq_offline"),
                    default="iq", help="the *fo agents learn from (s, s') alone: an inverse action model draws the expert's actions")
    ap.add_argument("--am-lr", type=float, default=1e-4, help="*fo: the action model's Adam learning rate")
    ap.add_argument("--am-batch", type=int, default=64, help="*fo: rows of one action-model fit")
    ap.add_argument("--am-fits-per-step", type=int, default=1, help="*fo: action-model fits per iteration")
    ap.add_argument("--interpolate", type=float, default=None, metavar="C",
                    help="*fo: interpolate_expert_states with interpolation_coef C")
    ap.add_argument("--h-loss-mode", choices=("MSE", "Huber"), default="Huber", help="lsiq_hc: H_loss_mode")
    ap.add_argument("--h-tau", type=float, default=0.005, help="lsiq_hc: H_tau, the H target's own rate")
    ap.add_argument("--lossq-type", choices=("iq_like", "sqil_like"), default="iq_like", help="lsiq: lossQ_type")
    ap.add_argument("--loss-mode-exp", choices=("fix", "bootstrap"), default="fix", help="lsiq: loss_mode_exp")
    ap.add_argument("--q-exp-loss", choices=("MSE", "Huber"), default=None, help="lsiq: Q_exp_loss (fix and sqil_like need one)")
    ap.add_argument("--q-min", type=float, default=-1.0, help="lsiq: Q_min")
    ap.add_argument("--q-max", type=float, default=1.0, help="lsiq: Q_max")
    ap.add_argument("--no-target-clipping", action="store_true", help="lsiq: target_clipping=False")
    ap.add_argument("--plcy-loss-mode", default=None, help="plcy_loss_mode (default: the algorithm's)")
    ap.add_argument("--n-steps", type=int, default=200, help="lsiq_offline: fit_offline's steps")
    ap.add_argument("--regularizer-mode", choices=("off", "exp", "exp_and_plcy"), default="off", help="lsiq_offline")
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--batch", type=int, default=32, help="policy rows per update; as many expert rows are added")
    ap.add_argument("--in-dim", type=int, default=32)
    ap.add_argument("--act-dim", type=int, default=11)
    ap.add_argument("--learnable-alpha", action="store_true", help="train the temperature (one 4-byte read-back per update)")
    ap.add_argument("--log", action="store_true", help="print the logged scalars under the reference's names")
    ap.add_argument("--json", default=None, metavar="FILE", help="write the run's figures to FILE")
    args = ap.parse_args()
    torch.manual_seed(0)
    eng = Engine(0)
    gen = torch.Generator(device="cuda").manual_seed(0)
    D, A = args.in_dim, args.act_dim
    p_lins = [torch.nn.Linear(D, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 2 * A)]
    with torch.no_grad():
        p_lins[2].weight.mul_(0.1)
    policy = DeviceSquashedGaussianPolicy(eng, p_lins, -np.ones(A), np.ones(A), standardizer=DeviceStandardizer(eng, D))
    c_lins = [torch.nn.Linear(D + A, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 1)]
    critic = DeviceSoftQCritic(eng, c_lins, standardizer=DeviceStandardizer(eng, D + A), lr=3e-4, tau=0.005)
    demo = il_synthetic_transitions(20000, D, A, seed=1)
    if args.algo == "lsiq_offline":
        return offline(args, eng, gen, policy, critic, demo)
    kw = dict(gamma=0.99, batch_size=args.batch, use_target=True, logging_iter=max(1, args.updates // 4),
              sw=PrintingWriter() if args.log else None, max_replay_size=50000, actor_optimizer=dict(lr=3e-4),
              warmup_transitions=1024, learnable_alpha=args.learnable_alpha, lr_alpha=3e-4, init_alpha=0.1)
    if args.plcy_loss_mode is not None:
        kw["plcy_loss_mode"] = args.plcy_loss_mode
    fo = args.algo.endswith("fo") or "fo_" in args.algo
    base = args.algo.replace("fo", "")
    if base in ("lsiq_h", "lsiq_hc"):      # the second critic: the same shape, its own optimiser
        h_lins = [torch.nn.Linear(D + A, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 1)]
        kw["h_critic"] = DeviceSoftQCritic(eng, h_lins, standardizer=DeviceStandardizer(eng, D + A), lr=3e-4, tau=0.005)
        if base == "lsiq_hc":
            kw.update(H_tau=args.h_tau, H_loss_mode=args.h_loss_mode)
    if base.startswith("lsiq"):
        kw.update(lossQ_type=args.lossq_type, loss_mode_exp=args.loss_mode_exp, Q_exp_loss=args.q_exp_loss, Q_min=args.q_min,
                  Q_max=args.q_max, target_clipping=not args.no_target_clipping)
    classes = dict(iq=DeviceIQSAC, sqil=DeviceSQILSAC, lsiq=DeviceLSIQSAC, lsiq_h=DeviceLSIQHSAC, lsiq_hc=DeviceLSIQHCSAC)
    if fo:      # the demonstrations lose their actions; the model on (s | s') draws them
        from olympic_hip import iqfo
        classes = dict(iq=iqfo.DeviceIQfOSAC, lsiq=iqfo.DeviceLSIQfOSAC, lsiq_h=iqfo.DeviceLSIQfOHSAC,
                       lsiq_hc=iqfo.DeviceLSIQfOHCSAC)
        demo = {k: v for k, v in demo.items() if k != "actions"}
        a_lins = [torch.nn.Linear(2 * D, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 2 * A)]
        kw["action_model"] = iqfo.DeviceGaussianInvActionModel(eng, a_lins, -np.ones(A), np.ones(A), args.am_lr,
                                                               batch_size=args.am_batch,
                                                               standardizer=DeviceStandardizer(eng, 2 * D))
        kw["action_model_fit_params"] = dict(fits_per_step=args.am_fits_per_step, init_epochs=0)
        if args.interpolate is not None:
            kw.update(interpolate_expert_states=True, interpolation_coef=args.interpolate)
    agent = classes[base](eng, policy, critic, demo, **kw)
    w0 = policy.param.clone()
    first_pi = last_q = last_pi = None
    for u in range(args.updates):
        # what the collection loop would hand over: the transitions of one vec step of 256 environments
        dataset = {k: torch.as_tensor(v).cuda() for k, v in il_synthetic_transitions(256, D, A, seed=100 + u, drift=0.5).items()}
        out_q, out_pi = agent.fit(dataset, generator=gen)
        last_q = out_q if out_q is not None else last_q
        if out_pi is not None:
            last_pi = out_pi.clone()
            first_pi = last_pi if first_pi is None else first_pi
    if last_pi is None:
        sys.exit("no policy update ran: --updates too small for the warm-up of 1024 transitions")
    first_pi, last_pi, last_q = first_pi.cpu().numpy(), last_pi.cpu().numpy(), last_q.cpu().numpy()
    moved = float((policy.param - w0).abs().max())
    print(f"{args.algo}: {critic.step} critic and {agent.pi_step} policy updates at batch {2 * args.batch}; Actor/Loss "
          f"{first_pi[0]:.5f} -> {last_pi[0]:.5f}; mean log_prob {first_pi[2]:.4f} -> {last_pi[2]:.4f}; mean Q(s, pi(s)) "
          f"{first_pi[3]:.4f} -> {last_pi[3]:.4f}; policy gradient norm {last_pi[1]:.4f}; the policy moved by {moved:.4f}; "
          f"alpha {agent.alpha:.5f} ({agent.alpha_step} temperature steps)")
    policy.sync_to_torch()
    critic.sync_to_torch()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(algo=args.algo, critic_updates=int(critic.step), policy_updates=int(agent.pi_step),
                           alpha=agent.alpha, first={t: float(v) for t, v in zip(_abi.IQ_PI_TAGS, first_pi)},
                           last={t: float(v) for t, v in zip(_abi.IQ_PI_TAGS, last_pi)},
                           critic_last={t: float(v) for t, v in zip(_abi.IQ_Q_TAGS, last_q)}), f)


def offline(args, eng, gen, policy, critic, demo):
    from olympic_hip.iq_offline import DeviceLSIQOffline
    agent = DeviceLSIQOffline(eng, policy, critic, demo, gamma=0.99, batch_size=args.batch, use_target=True, Q_max=args.q_max,
                              Q_min=args.q_min, loss_mode_exp=args.loss_mode_exp, Q_exp_loss=args.q_exp_loss,
                              regularizer_mode=args.regularizer_mode, actor_optimizer=dict(lr=3e-4),
                              learnable_alpha=args.learnable_alpha, lr_alpha=3e-4, init_alpha=0.1,
                              logging_iter=max(1, args.n_steps // 4), sw=PrintingWriter() if args.log else None)
    w0 = policy.param.clone()
    first_q, _ = agent.fit_offline(1, generator=gen)
    first_q = first_q.cpu().numpy()
    last_q, last_pi = agent.fit_offline(args.n_steps - 1, generator=gen) if args.n_steps > 1 else (None, None)
    last_q = first_q if last_q is None else last_q.cpu().numpy()
    moved = float((policy.param - w0).abs().max())
    print(f"lsiq_offline: {critic.step} critic and {agent.pi_step} policy updates at batch {args.batch}; Loss1 "
          f"{first_q[0]:.5f} -> {last_q[0]:.5f}; Q for expert {first_q[4]:.4f} -> {last_q[4]:.4f} (Q_max {args.q_max}); "
          f"the policy moved by {moved:.4f}; alpha {agent.alpha:.5f} ({agent.alpha_step} temperature steps)")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(algo=args.algo, critic_updates=int(critic.step), policy_updates=int(agent.pi_step),
                           alpha=agent.alpha, critic_first={t: float(v) for t, v in zip(_abi.IQ_Q_TAGS, first_q)},
                           critic_last={t: float(v) for t, v in zip(_abi.IQ_Q_TAGS, last_q)}), f)


if __name__ == "__main__":
    main()
