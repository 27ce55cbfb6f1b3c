#!/usr/bin/env python3
"""LSIQ's critic update beside IQ's, one JSON line: at in = 32, A = 11 and B = 64 and 512 rows, with a target and both
Standardizers, one update of
  iq         IQ-Learn, plcy_loss_mode value, regularizer exp_and_plcy (tools/bench_iq_q.py's case)
  lsiq_fix   LSIQ iq_like, target_clipping, loss_mode_exp fix with Q_exp_loss MSE, the same mode and regularizer
  lsiq_sqil  LSIQ sqil_like, plcy_loss_mode value_plcy (the third pass on the policy's rows alone), bootstrap / Huber
in the same process: the agent's update_Q_function (the policy passes of K25 and one oly_iq_q_update) and the
oly_iq_q_update call alone, each timed in TWO runs (both shown: `*_us_*` is [run 1, run 2], the median of REPS windows
each), and the two LSIQ updates in torch eager on the same GPU (tools/bench_iq_q.py's lines with LSIQ's loss).

    python tools/bench_lsiq_q.py [--out FILE] [--kernel-only]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "olympics-mujoco_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bench_iq_q import ACT_DIM, IN_DIM, MANY, REPS, D, Stand, launches, mlp, timed  # noqa: E402

Q_MIN, Q_MAX = -1.0, 1.0
CASES = dict(iq=None,
             lsiq_fix=dict(lossQ_type="iq_like", loss_mode_exp="fix", Q_exp_loss="MSE", plcy_loss_mode="value"),
             lsiq_sqil=dict(lossQ_type="sqil_like", loss_mode_exp="bootstrap", Q_exp_loss="Huber", plcy_loss_mode="value_plcy"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-only", action="store_true", help="time the device path alone")
    args = ap.parse_args()
    from olympic_hip.bc import DeviceSquashedGaussianPolicy
    from olympic_hip.engine import Engine
    from olympic_hip.gail import DeviceStandardizer
    from olympic_hip.iq import DeviceIQLearn, DeviceLSIQ, DeviceSoftQCritic
    from olympic_hip.synthetic import il_synthetic_transitions
    eng = Engine(0)
    torch.manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "in_dim": IN_DIM, "act_dim": ACT_DIM, "reps": REPS, "runs": 2}
    demo = il_synthetic_transitions(64, IN_DIM, ACT_DIM, seed=1)
    twice = lambda fn, many: [timed(lambda: [fn() for _ in range(many)], REPS) * 1e3 / many for _ in range(2)]
    for B in (64, 512):
        n_p = B // 2
        t = {k: torch.as_tensor(v).cuda() for k, v in il_synthetic_transitions(B, IN_DIM, ACT_DIM, seed=2, absorbing_frac=0.2).items()}
        obs, act, nxt, ab = t["states"], t["actions"], t["next_states"], t["absorbing"]
        for name, ls in CASES.items():
            tag = f"{name}_b{B}"
            n_pi = n_p if name == "lsiq_sqil" else B
            eps = dict(next=torch.randn((B, ACT_DIM), device="cuda"), pi=torch.randn((n_pi, ACT_DIM), device="cuda"),
                       expert=torch.randn((B - n_p, ACT_DIM), device="cuda"))
            p_lins = [torch.nn.Linear(IN_DIM, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 2 * ACT_DIM)]
            pol = DeviceSquashedGaussianPolicy(eng, p_lins, -np.ones(ACT_DIM), np.ones(ACT_DIM),
                                               standardizer=DeviceStandardizer(eng, IN_DIM))
            c_lins = [torch.nn.Linear(D, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 1)]
            cr = DeviceSoftQCritic(eng, c_lins, standardizer=DeviceStandardizer(eng, D), lr=3e-4, tau=0.005)
            kw = dict(gamma=0.99, batch_size=n_p, use_target=True, logging_iter=10 ** 9, max_replay_size=8)
            if ls is None:
                ag = DeviceIQLearn(eng, pol, cr, demo, **kw)
            else:
                ag = DeviceLSIQ(eng, pol, cr, demo, Q_min=Q_MIN, Q_max=Q_MAX, target_clipping=True, **ls, **kw)
            upd = lambda: ag.update_Q_function(obs, act, nxt, ab, n_p, eps=eps)
            res[f"update_us_{tag}"] = twice(upd, MANY)
            res[f"launches_{tag}"] = launches(upd)
            a_n, lp_n = ag._policy_pass(nxt, eps["next"], None)
            a_p, lp_p = ag._policy_pass(obs[:n_pi], eps["pi"], None)
            ws = ag._workspace(B)

            def k26():
                eng.iq_q_update(obs, act, nxt, ab, a_n, lp_n, a_p, lp_p, n_p, cr.stand.colstats, cr.target_stand.colstats,
                                cr.param, cr.exp_avg, cr.exp_avg_sq, cr.packed, cr.target_param, cr.target_packed, ws, cr.step,
                                cr.lr, algo=ag.ALGO, plcy_loss_mode=ag.plcy_loss_mode, use_target=True, alpha=ag.alpha,
                                tau=cr.tau, **ag._algo_block())
                cr.step += 1
            res[f"k26_us_{tag}"] = twice(k26, MANY)
            res[f"k26_launches_{tag}"] = launches(k26)
            if args.kernel_only or ls is None:
                continue
            # torch eager: the reference's lines on the same GPU
            pnet, cnet, tnet = mlp(IN_DIM, 2 * ACT_DIM), mlp(D, 1), mlp(D, 1)
            tnet.load_state_dict(cnet.state_dict())
            ps, cs, ts = Stand(IN_DIM), Stand(D), Stand(D)
            opt = torch.optim.Adam(cnet.parameters(), lr=3e-4)
            alpha, gamma, tau, reg = 1e-3, 0.99, 0.005, 0.5
            is_exp = torch.arange(B, device="cuda") >= n_p
            sqil_like = ls["lossQ_type"] == "sqil_like"

            def act_logp(x, e):
                with torch.no_grad():
                    y = pnet(ps(x))
                    mu, lsg = y[:, :ACT_DIM], torch.clamp(y[:, ACT_DIM:], -20.0, 2.0)
                    raw = mu + lsg.exp() * e
                    a = torch.tanh(raw)
                    lp = torch.distributions.Normal(mu, lsg.exp()).log_prob(raw).sum(1) - torch.log(1.0 - a.pow(2) + 1e-6).sum(1)
                return a, lp.unsqueeze(1)

            def torch_update():
                q = cnet(cs(torch.cat([obs, act], 1)))
                a1, lp1 = act_logp(nxt, eps["next"])
                with torch.no_grad():
                    nv = tnet(ts(torch.cat([nxt, a1], 1))) - alpha * lp1
                y = (1 - ab.unsqueeze(1)) * gamma * torch.clip(nv, Q_MIN, Q_MAX)
                reward = q - y
                if sqil_like:
                    r = torch.ones_like(y) * (1 / reg)
                    a2, lp2 = act_logp(obs[:n_p], eps["pi"])
                    v = cnet(cs(torch.cat([obs[:n_p], a2], 1))) - alpha * lp2
                    loss = F.huber_loss(q[is_exp], r[is_exp] + y[is_exp]) + F.huber_loss(v, -r[~is_exp] + y[~is_exp])
                else:
                    a2, lp2 = act_logp(obs, eps["pi"])
                    v = cnet(cs(torch.cat([obs, a2], 1))) - alpha * lp2
                    loss = F.mse_loss(q[is_exp], torch.ones_like(q[is_exp]) * Q_MAX) + (v - y).mean() + \
                        (reg * torch.square(reward)).mean()
                opt.zero_grad()
                loss.backward()
                opt.step()
                with torch.no_grad():
                    for p, q_ in zip(cnet.parameters(), tnet.parameters()):
                        q_.copy_(tau * p + (1 - tau) * q_)
            res[f"torch_us_{tag}"] = twice(torch_update, 50)
            res[f"torch_launches_{tag}"] = launches(torch_update)
            res[f"speedup_{tag}"] = min(res[f"torch_us_{tag}"]) / min(res[f"update_us_{tag}"])
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
