#!/usr/bin/env python3
"""Offline LS-IQ's updates, one JSON line: at in = 32, A = 11 and B = 64 and 512 rows, with a target and both
Standardizers, in the same process
  k26_plain   one oly_iq_q_update of LSIQ iq_like fix / MSE, plcy_loss_mode value, n_policy = B / 2 (tools/bench_lsiq_q.py's
              lsiq_fix call: three passes, the existing instantiation)
  k26_v0      the same call with plcy_loss_mode v0 (four passes, the v0 instantiation; the same number of gradient slots)
  k26_offline the offline call: v0 on an all-expert batch (n_policy = 0, the fourth pass takes all B rows), regularizer off
  iq_update   one whole DeviceLSIQOffline.iq_update: four policy passes (K25), the critic update (K26), the policy update
              (K27), no logging
  torch       LSIQ_Offline's iq_update in torch eager on the same GPU (the reference's lines under _Q_Q_multiplier =
              _abs_mult = 1)
each timed with HIP events in TWO runs (both shown: `*_us_*` is [run 1, run 2], the median of REPS windows each; see
tools/bench_iq_q.py's timed).

    python tools/bench_iq_offline.py [--out FILE] [--kernel-only]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-only", action="store_true", help="time the device path alone")
    args = ap.parse_args()
    from olympic_hip.bc import DeviceSquashedGaussianPolicy
    from olympic_hip.engine import Engine
    from olympic_hip.gail import DeviceStandardizer
    from olympic_hip.iq import DeviceSoftQCritic
    from olympic_hip.iq_offline import DeviceLSIQOffline
    from olympic_hip.synthetic import il_synthetic_transitions
    eng = Engine(0)
    torch.manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "in_dim": IN_DIM, "act_dim": ACT_DIM, "reps": REPS, "runs": 2}
    twice = lambda fn, many: [timed(lambda: [fn() for _ in range(many)], REPS) * 1e3 / many for _ in range(2)]
    block = dict(lossQ_type="iq_like", loss_mode_exp="fix", Q_exp_loss="MSE", target_clipping=True, Q_min=Q_MIN, Q_max=Q_MAX)
    for B in (64, 512):
        t = {k: torch.as_tensor(v).cuda() for k, v in il_synthetic_transitions(B, IN_DIM, ACT_DIM, seed=2, absorbing_frac=0.2).items()}
        obs, act, nxt, ab = t["states"], t["actions"], t["next_states"], t["absorbing"]
        demo = {k: v for k, v in t.items()}
        p_lins = [torch.nn.Linear(IN_DIM, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 2 * ACT_DIM)]
        pol = DeviceSquashedGaussianPolicy(eng, p_lins, -np.ones(ACT_DIM), np.ones(ACT_DIM),
                                           standardizer=DeviceStandardizer(eng, IN_DIM))
        c_lins = [torch.nn.Linear(D, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 1)]
        cr = DeviceSoftQCritic(eng, c_lins, standardizer=DeviceStandardizer(eng, D), lr=3e-4, tau=0.005)
        ag = DeviceLSIQOffline(eng, pol, cr, demo, gamma=0.99, batch_size=B, use_target=True, Q_max=Q_MAX, Q_min=Q_MIN,
                               Q_exp_loss="MSE", logging_iter=10 ** 9, actor_optimizer=dict(lr=3e-4))
        eps = {k: torch.randn((B, ACT_DIM), device="cuda") for k in ("next", "pi", "v0", "ppi")}
        a_n, lp_n = ag._policy_pass(nxt, eps["next"], None)
        a_p, lp_p = ag._policy_pass(obs, eps["pi"], None)
        a_0, lp_0 = ag._policy_pass(obs, eps["v0"], None)
        ws = ag._workspace(B)

        def k26(n_p, mode, reg, **more):
            def call():
                eng.iq_q_update(obs, act, nxt, ab, a_n, lp_n, a_p, lp_p, n_p, cr.stand.colstats, cr.target_stand.colstats,
                                cr.param, cr.exp_avg, cr.exp_avg_sq, cr.packed, cr.target_param, cr.target_packed, ws, cr.step,
                                cr.lr, algo="lsiq", plcy_loss_mode=mode, regularizer_mode=reg, use_target=True, alpha=ag.alpha,
                                tau=cr.tau, lsiq=block, **more)
                cr.step += 1
            return call
        half = B // 2
        cases = dict(k26_plain=k26(half, "value", "exp_and_plcy"),
                     k26_v0=k26(half, "v0", "exp_and_plcy", v0=(a_0[half:].contiguous(), lp_0[half:].contiguous())),
                     k26_offline=k26(0, "v0", "off", treat_absorbing=True, v0=(a_0, lp_0), all_expert=True))
        # alternate the cases within each run, so that a drift of the clock shows in all of them alike
        for name, fn in cases.items():
            res[f"{name}_us_b{B}"] = []
        for _ in range(2):
            for name, fn in cases.items():
                res[f"{name}_us_b{B}"].append(timed(lambda: [fn() for _ in range(MANY)], REPS) * 1e3 / MANY)
        for name, fn in cases.items():
            res[f"{name}_launches_b{B}"] = launches(fn)
        upd = lambda: ag.iq_update(obs, act, nxt, ab, eps=dict(q=eps, pi=dict(pi=eps["ppi"])))
        res[f"iq_update_us_b{B}"] = twice(upd, MANY)
        res[f"iq_update_launches_b{B}"] = launches(upd)
        if args.kernel_only:
            continue
        # torch eager: the reference's lines on the same GPU
        pnet, cnet, tnet = mlp(IN_DIM, 2 * ACT_DIM), mlp(D, 1), mlp(D, 1)
        tnet.load_state_dict(cnet.state_dict())
        ps, cs, ts = Stand(IN_DIM), Stand(D), Stand(D)
        opt = torch.optim.Adam(cnet.parameters(), lr=3e-4)
        popt = torch.optim.Adam(pnet.parameters(), lr=3e-4)
        alpha, gamma, tau = 1e-3, 0.99, 0.005

        def act_logp(x, e, grad=False):
            with torch.enable_grad() if grad else torch.no_grad():
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
            loss = F.mse_loss(q, torch.ones_like(q) * Q_MAX)
            a2, lp2 = act_logp(obs, eps["pi"])
            v = cnet(cs(torch.cat([obs, a2], 1))) - alpha * lp2                 # getV(obs): logged only
            a3, lp3 = act_logp(obs, eps["v0"])
            v0 = cnet(cs(torch.cat([obs, a3], 1))) - alpha * lp3
            loss = loss + ((1 - gamma) * v0).mean()
            opt.zero_grad()
            loss.backward()
            opt.step()
            a4, lp4 = act_logp(obs, eps["ppi"], grad=True)
            xa = torch.cat([obs, a4], 1)
            cs(xa.detach())                         # the Standardizer takes the rows (numpy in the reference: no gradient)
            cnt = cs.cs[0] + 1e-2
            mean = cs.cs[1] / cnt
            sd = torch.sqrt(torch.clamp((cs.cs[2] + 1e-2) / cnt - mean * mean, min=1e-2))
            ploss = (alpha * lp4.squeeze(1) - cnet(((xa.double() - mean) / sd).float())).mean()
            popt.zero_grad()
            ploss.backward()
            popt.step()
            with torch.no_grad():
                for p, q_ in zip(cnet.parameters(), tnet.parameters()):
                    q_.copy_(tau * p + (1 - tau) * q_)
            return nv, v
        res[f"torch_us_b{B}"] = twice(torch_update, 50)
        res[f"torch_launches_b{B}"] = launches(torch_update)
        res[f"speedup_b{B}"] = min(res[f"torch_us_b{B}"]) / min(res[f"iq_update_us_b{B}"])
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
