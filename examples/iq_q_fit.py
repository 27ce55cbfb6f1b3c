#!/usr/bin/env python3
"""The critic side of IQ-Learn (imitation_lib/imitation/iq_sac.py), SQIL (imitation_lib/imitation/sqil_sac.py), LSIQ
(imitation_lib/imitation/lsiq.py) or LSIQ_H / LSIQ_HC (lsiq_h.py, lsiq_hc.py: a second critic H learns the entropy) on
synthetic transitions (olympic_hip.synthetic): a squashed-Gaussian policy with random weights supplies the actions the
critic's loss needs, the expert's and the policy's transitions are seeded stand-ins, and DeviceIQLearn.fit_Q runs
update_Q_function and the soft target update on the GPU: three oly_sg_act calls at most (K25) and one oly_iq_q_update
(K26) per update.  The policy is not trained here: examples/iq_fit.py runs the whole agent (DeviceIQSAC, K27).

    python examples/iq_q_fit.py --algo iq|sqil|lsiq [--updates 200] [--batch 32] [--no-target] [--log] [--json FILE]
    python examples/iq_q_fit.py --algo lsiq --q-exp-loss MSE|Huber [--lossq-type iq_like|sqil_like]
        [--loss-mode-exp fix|bootstrap] [--q-min -1] [--q-max 1] [--no-target-clipping] [--plcy-loss-mode MODE]
    python examples/iq_q_fit.py --algo lsiq_h|lsiq_hc --q-exp-loss MSE [--h-loss-mode MSE|Huber] [--h-tau 0.005]
        [--alpha 0.2] and LSIQ's options (lossq-type iq_like)
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
from olympic_hip.iq import DeviceIQLearn, DeviceLSIQ, DeviceLSIQH, DeviceLSIQHC, DeviceSoftQCritic, DeviceSQIL  # noqa: E402
from olympic_hip.synthetic import il_synthetic_transitions  # noqa: E402


class PrintingWriter:
    def add_scalar(self, name, value, it):
        print(f"  [{it}] {name} = {value:.6g}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--algo", choices=("iq", "sqil", "lsiq", "lsiq_h", "lsiq_hc"), default="iq")
    ap.add_argument("--h-loss-mode", choices=("MSE", "Huber"), default="Huber", help="lsiq_hc: H_loss_mode")
    ap.add_argument("--h-tau", type=float, default=0.005, help="lsiq_hc: H_tau, the H target's own rate")
    ap.add_argument("--alpha", type=float, default=None, help="init_alpha (default: the agents' 1e-3)")
    ap.add_argument("--lossq-type", choices=("iq_like", "sqil_like"), default="iq_like", help="lsiq: lossQ_type")
    ap.add_argument("--loss-mode-exp", choices=("fix", "bootstrap"), default="fix", help="lsiq: loss_mode_exp")
    ap.add_argument("--q-exp-loss", choices=("MSE", "Huber"), default=None, help="lsiq: Q_exp_loss (fix and sqil_like need one)")
    ap.add_argument("--q-min", type=float, default=-1.0, help="lsiq: Q_min")
    ap.add_argument("--q-max", type=float, default=1.0, help="lsiq: Q_max")
    ap.add_argument("--no-target-clipping", action="store_true", help="lsiq: target_clipping=False")
    ap.add_argument("--plcy-loss-mode", default=None, help="plcy_loss_mode (default: the algorithm's)")
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--batch", type=int, default=32, help="policy rows per update; as many expert rows are added")
    ap.add_argument("--in-dim", type=int, default=32)
    ap.add_argument("--act-dim", type=int, default=11)
    ap.add_argument("--no-target", action="store_true", help="use_target=False: the next-state pass carries a gradient")
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
    kw = dict(gamma=0.99, batch_size=args.batch, use_target=not args.no_target, logging_iter=max(1, args.updates // 4),
              sw=PrintingWriter() if args.log else None, max_replay_size=50000)
    if args.plcy_loss_mode is not None:
        kw["plcy_loss_mode"] = args.plcy_loss_mode
    if args.alpha is not None:
        kw["init_alpha"] = args.alpha
    h_critic = None
    if args.algo in ("lsiq_h", "lsiq_hc"):      # the second critic: the same shape, its own optimiser
        h_lins = [torch.nn.Linear(D + A, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 1)]
        h_critic = DeviceSoftQCritic(eng, h_lins, standardizer=DeviceStandardizer(eng, D + A), lr=3e-4, tau=0.005)
        kw["h_critic"] = h_critic
        if args.algo == "lsiq_hc":
            kw.update(H_tau=args.h_tau, H_loss_mode=args.h_loss_mode)
    if args.algo != "iq" and args.algo != "sqil":
        kw.update(lossQ_type=args.lossq_type, loss_mode_exp=args.loss_mode_exp, Q_exp_loss=args.q_exp_loss, Q_min=args.q_min,
                  Q_max=args.q_max, target_clipping=not args.no_target_clipping)
    agent = dict(iq=DeviceIQLearn, sqil=DeviceSQIL, lsiq=DeviceLSIQ, lsiq_h=DeviceLSIQH,
                 lsiq_hc=DeviceLSIQHC)[args.algo](eng, policy, critic, demo, **kw)
    first = last = h_first = None
    for u in range(args.updates):
        # what the collection loop would hand over: the transitions of one vec step of 256 environments
        dataset = {k: torch.as_tensor(v).cuda() for k, v in il_synthetic_transitions(256, D, A, seed=100 + u, drift=0.5).items()}
        out = agent.fit_Q(dataset, generator=gen)
        if u == 0:
            first = out.clone()
            h_first = agent.h_out.clone() if h_critic is not None else None
        last = out
    first, last = first.cpu().numpy(), last.cpu().numpy()
    name = "IQ-Loss/LossQ" if args.algo == "sqil" else "Loss1 + Loss2 + Chi2"      # LSIQ's sqil_like: Chi2 is 0
    tot = lambda o: float(o[0]) if args.algo == "sqil" else float(o[0] + o[1] + o[2])
    print(f"{args.algo}: {critic.step} critic updates at batch {2 * args.batch} ({'a target' if not args.no_target else 'no target'}); "
          f"{name} {tot(first):.5f} -> {tot(last):.5f}; Q for expert {first[4]:.4f} -> {last[4]:.4f}, "
          f"Q for policy {first[6]:.4f} -> {last[6]:.4f}; gradient norm {last[15]:.4f}")
    q = critic.predict(torch.as_tensor(demo["states"][:256]).cuda(), torch.as_tensor(demo["actions"][:256]).cuda())
    print(f"Q on 256 expert rows: mean {float(q.mean()):.4f}; target mean "
          f"{float(critic.predict_target(torch.as_tensor(demo['states'][:256]).cuda(), torch.as_tensor(demo['actions'][:256]).cuda()).mean()):.4f}")
    if h_critic is not None:
        h0, h1 = h_first.cpu().numpy(), agent.h_out.cpu().numpy()
        print(f"H: {h_critic.step} updates; H function/Loss {h0[0]:.5f} -> {h1[0]:.5f}; H expert {h0[3]:.4f} -> {h1[3]:.4f}, "
              f"H plcy {h0[2]:.4f} -> {h1[2]:.4f}; running maximum of -log pi {float(agent.h_max_state[0]):.4f}")
    critic.sync_to_torch()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(algo=args.algo, updates=int(critic.step), first={t: float(v) for t, v in zip(_abi.IQ_Q_TAGS, first)},
                           last={t: float(v) for t, v in zip(_abi.IQ_Q_TAGS, last)}), f)


if __name__ == "__main__":
    main()
