#!/usr/bin/env python3
"""The inverse action model's measurements (olympic_hip.iqfo, K24 / K25 / K28 on two indexed tables), one JSON line:
at in = 32 (16 + 16), A = 11, a replay ring of 20 000 rows and a Standardizer,

  one action-model fit step at batch 64 and 512, a one-step call as an iteration makes it:
      paired     DeviceGaussianInvActionModel.fit on (ring, idx): ONE oly_bc_fit_steps call with oly_bc_fit.pair
      composed   what the entry points without the pair compose: three torch gathers, a cat, oly_bc_targets, then
                 oly_bc_fit_steps on the materialised table
      torch      the reference's loop restated in torch eager on the same GPU (gathers, cat, un-squashing, the
                 Standardizer's update, GaussianNLLLoss, backward, torch.optim.Adam)
  one expert draw of 64 and 512 rows: paired (ONE oly_sg_act call with its two-table fields and the clip) against
  composed (two gathers, a cat, oly_sg_act on the materialised rows, then LSIQfO's clip as torch makes it: to float64,
  maximum, minimum, to float32).
  one whole DeviceIQfOSAC.fit against one DeviceIQSAC.fit at batch 64 (fits_per_step 1, action-model batch 64, no
  logging iteration in the windows, datasets of 64 transitions).

Same process, the variants alternating, RUNS runs each; every figure is the median of REPS timed windows of MANY calls
after a warm-up, HIP events on the stream, microseconds per call.  The launch counts beside the times are those of the
library's calls (the header's); torch's own kernels for a gather or a cat are counted as one each.

    python tools/bench_iam.py [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "olympics-mujoco_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

REPS, RUNS, MANY = 7, 2, 100
D1 = D2 = 16
ACT_DIM, N_ROWS = 11, 20000
LAUNCHES = {"fit_paired": 4, "fit_composed": 9, "draw_paired": 3, "draw_composed": 10}


def timed(fn, reps=REPS, warmup=2):
    """Median microseconds per call over `reps` windows of MANY fn() each."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(MANY):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / MANY)
    return statistics.median(out)


def agents(eng, res, gen):
    """One whole fit of the from-observations agent against one of its base agent, alternating."""
    from olympic_hip.bc import DeviceSquashedGaussianPolicy
    from olympic_hip.gail import DeviceStandardizer
    from olympic_hip.iq import DeviceIQSAC, DeviceSoftQCritic
    from olympic_hip.iqfo import DeviceGaussianInvActionModel, DeviceIQfOSAC
    from olympic_hip.synthetic import il_synthetic_transitions
    D, A, batch = D1, ACT_DIM, 64
    lin = torch.nn.Linear
    demo = il_synthetic_transitions(20000, D, A, seed=1)
    data = {k: torch.as_tensor(v).cuda() for k, v in il_synthetic_transitions(64, D, A, seed=2, drift=0.5).items()}
    made = {}
    for name in ("iqfo", "iq"):
        policy = DeviceSquashedGaussianPolicy(eng, [lin(D, 512), lin(512, 256), lin(256, 2 * A)], -np.ones(A), np.ones(A),
                                              standardizer=DeviceStandardizer(eng, D))
        critic = DeviceSoftQCritic(eng, [lin(D + A, 512), lin(512, 256), lin(256, 1)], standardizer=DeviceStandardizer(eng, D + A),
                                   lr=3e-4, tau=0.005)
        kw = dict(gamma=0.99, batch_size=batch, use_target=True, logging_iter=10 ** 9, max_replay_size=50000,
                  actor_optimizer=dict(lr=3e-4), init_alpha=0.1)
        if name == "iqfo":
            am = DeviceGaussianInvActionModel(eng, [lin(2 * D, 512), lin(512, 256), lin(256, 2 * A)], -np.ones(A), np.ones(A),
                                              1e-4, batch_size=64, standardizer=DeviceStandardizer(eng, 2 * D))
            made[name] = DeviceIQfOSAC(eng, policy, critic, {k: v for k, v in demo.items() if k != "actions"},
                                       action_model=am, **kw)
        else:
            made[name] = DeviceIQSAC(eng, policy, critic, demo, **kw)
    for run in range(RUNS):
        for name, agent in made.items():
            res.setdefault(f"agent_fit_{name}_us_b{batch}", []).append(round(timed(lambda: agent.fit(data, generator=gen)), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from olympic_hip.engine import Engine
    from olympic_hip.gail import DeviceStandardizer
    from olympic_hip.iqfo import DeviceGaussianInvActionModel
    eng = Engine(0)
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    D = D1 + D2
    up = lambda a: torch.as_tensor(a.astype(np.float32)).cuda()
    S = up(rng.standard_normal((N_ROWS, D1)) * rng.uniform(0.3, 3, D1))
    NS = up(rng.standard_normal((N_ROWS, D2)) * rng.uniform(0.3, 3, D2))
    ACT = up(1.05 * np.tanh(rng.standard_normal((N_ROWS, ACT_DIM))))
    lo, hi = -np.ones(ACT_DIM), np.ones(ACT_DIM)
    clip = (torch.as_tensor(lo).cuda(), torch.as_tensor(hi).cuda())
    res = {"device": torch.cuda.get_device_name(0), "in_dim": D, "act_dim": ACT_DIM, "rows": N_ROWS, "reps": REPS,
           "calls_per_window": MANY, "launches": LAUNCHES}
    gen = torch.Generator(device="cuda").manual_seed(0)

    def model(batch):
        lins = [torch.nn.Linear(D, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 2 * ACT_DIM)]
        return DeviceGaussianInvActionModel(eng, lins, lo, hi, 1e-4, batch_size=batch, standardizer=DeviceStandardizer(eng, D))

    for batch in (64, 512):
        idx = torch.randint(N_ROWS, (1, batch), device="cuda", generator=gen).to(torch.int32)
        rows, own = idx[0].long(), torch.arange(batch, device="cuda", dtype=torch.int32).reshape(1, batch)
        m1, m2 = model(batch), model(batch)
        ws = eng.bc_fit_ws(batch, D, ACT_DIM)

        def fit_paired():
            m1.fit(S, NS, ACT, idx)

        def fit_composed():
            table = torch.cat([S[rows], NS[rows]], dim=1)
            targets = eng.bc_targets(ACT[rows], m2.central, m2.delta)
            eng.bc_fit_steps(table, targets, own, m2._colstats(), m2.param, m2.exp_avg, m2.exp_avg_sq, m2.packed, ws, m2.step,
                             m2.lr, log_std_min=m2.log_std_min, log_std_max=m2.log_std_max)
            m2.stand._fresh = False
            m2.step += 1

        net = torch.nn.Sequential(torch.nn.Linear(D, 512), torch.nn.ReLU(), torch.nn.Linear(512, 256), torch.nn.ReLU(),
                                  torch.nn.Linear(256, 2 * ACT_DIM)).cuda()
        opt = torch.optim.Adam(net.parameters(), lr=1e-4)
        loss_fn = torch.nn.GaussianNLLLoss()
        cs = torch.zeros((3, D), dtype=torch.float64, device="cuda")

        def fit_torch():
            xd = torch.cat([S[rows], NS[rows]], dim=1).double()
            t = torch.arctanh(torch.clip((ACT[rows] - m2.central) / m2.delta, -1.0 + 1e-7, 1.0 - 1e-7))
            cs[0] += batch
            cs[1] += xd.sum(0)
            cs[2] += (xd * xd).sum(0)
            cnt = cs[0] + 1e-2
            mean = cs[1] / cnt
            sd = torch.sqrt(torch.clamp((cs[2] + 1e-2) / cnt - mean * mean, min=1e-2))
            y = net(((xd - mean) / sd).float())
            mu, log_sigma = y[:, :ACT_DIM], torch.clamp(y[:, ACT_DIM:], -5.0, 2.0)
            loss = loss_fn(input=mu, target=t, var=torch.square(log_sigma.exp()))
            opt.zero_grad()
            loss.backward()
            opt.step()

        eps = torch.randn((batch, ACT_DIM), device="cuda", generator=gen)

        def draw_paired():
            m1.draw_action(S, NS, idx=idx[0], eps=eps, clip=clip)

        def draw_composed():
            x = torch.cat([S[rows], NS[rows]], dim=1)
            o = eng.sg_act(x, m2.packed, m2.central, m2.delta, colstats=m2.stand.colstats, eps=eps,
                           log_std_min=m2.log_std_min, log_std_max=m2.log_std_max, want=())
            torch.minimum(torch.maximum(o["action"].double(), clip[0]), clip[1]).float()

        for run in range(RUNS):
            for name, fn in (("fit_paired", fit_paired), ("fit_composed", fit_composed), ("fit_torch", fit_torch),
                             ("draw_paired", draw_paired), ("draw_composed", draw_composed)):
                res.setdefault(f"{name}_us_b{batch}", []).append(round(timed(fn), 2))
    agents(eng, res, gen)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
