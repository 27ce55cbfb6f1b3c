#!/usr/bin/env python3
"""K16 measurements, one JSON line: the forward at 409 600 rows, the critic-fit epoch call per minibatch of 256
against a torch eager loop doing the same work on the same GPU (standardise, forward, F.mse_loss, backward,
torch.optim.Adam), and one whole VAILAgent.fit for [100, 4096] with a no-op policy_step.  HIP events on the stream.

    python tools/bench_il_critic.py [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "olympics-mujoco_amd"))

import torch  # noqa: E402


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from olympic_hip.engine import Engine
    from olympic_hip.gail import DeviceStandardizer, DiscriminatorReward, VariationalDiscriminator
    from olympic_hip.il_agent import DeviceILCritic, VAILAgent
    eng = Engine(0)
    torch.manual_seed(0)
    lins = [torch.nn.Linear(32, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 1)]
    res = {"device": torch.cuda.get_device_name(0)}

    # ---- forward at 409 600 rows
    stand = DeviceStandardizer(eng, 32)
    critic = DeviceILCritic(eng, lins, stand)
    x = torch.randn((409600, 32), device="cuda")
    stand.update_mean_std(x)
    y = torch.empty((409600, 1), device="cuda")
    ms = timed(lambda: eng.ilmlp_forward(x, critic.packed, 1, colstats=stand.colstats, y=y), 50)
    res["forward_409600_us"] = ms * 1e3
    res["forward_409600_tflops"] = 2 * (32 * 512 + 512 * 256 + 256) * 409600 / (ms * 1e-3) / 1e12

    # ---- the fit: one epoch call over 409 600 rows (1600 minibatches of 256)
    vt = torch.randn(409600, device="cuda")
    perm = torch.randperm(409600, device="cuda").to(torch.int32)
    ws = eng.il_critic_fit_ws(256, 32)
    nb = 1600
    step = [0]

    def epoch():
        eng.il_critic_fit_epoch(x, vt, perm, 256, stand.colstats, critic.param, critic.exp_avg, critic.exp_avg_sq,
                                critic.packed, ws, step[0], 1e-4)
        step[0] += nb
    ms = timed(epoch, 3, warmup=1)
    res["fit_us_per_minibatch"] = ms * 1e3 / nb

    # torch eager: the same work per minibatch (statistics update, standardise, forward, mse, backward, Adam)
    net = torch.nn.Sequential(torch.nn.Linear(32, 512), torch.nn.ReLU(), torch.nn.Linear(512, 256), torch.nn.ReLU(),
                              torch.nn.Linear(256, 1)).cuda()
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    cs = torch.zeros((3, 32), dtype=torch.float64, device="cuda")
    vt2 = vt.reshape(-1, 1)
    p64 = perm.long()
    n_torch = 200

    def torch_loop():
        for b in range(n_torch):
            idx = p64[b * 256:(b + 1) * 256]
            xb = x[idx]
            xd = xb.double()
            cs[0] += 256
            cs[1] += xd.sum(0)
            cs[2] += (xd * xd).sum(0)
            cnt = cs[0] + 1e-2
            mean = cs[1] / cnt
            sd = torch.sqrt(torch.clamp((cs[2] + 1e-2) / cnt - mean * mean, min=1e-2))
            loss = torch.nn.functional.mse_loss(net(((xd - mean) / sd).float()), vt2[idx])
            opt.zero_grad()
            loss.backward()
            opt.step()
    ms = timed(torch_loop, 3, warmup=1)
    res["torch_us_per_minibatch"] = ms * 1e3 / n_torch
    res["fit_speedup"] = res["torch_us_per_minibatch"] / res["fit_us_per_minibatch"]

    # ---- whole VAILAgent.fit, [T=100, N=4096], no-op policy step, a no-op discriminator trainer
    class NoTrain:
        def fit(self, x, generator=None):
            return []
    dnet = VariationalDiscriminator(in_dim=32).cuda()
    stand2 = DeviceStandardizer(eng, 32)
    agent = VAILAgent(eng, DiscriminatorReward(eng, dnet), NoTrain(), DeviceILCritic(eng, lins, stand2),
                      lambda o, a, adv, ag: None, train_D_n_th_epoch=10 ** 9)
    T, N = 100, 4096
    s = torch.randn((T + 1, N, 32), device="cuda")
    last = torch.zeros((T, N), dtype=torch.bool, device="cuda")
    last[-1] = True
    ds = dict(state=s[:-1], action=torch.randn((T, N, 11), device="cuda"), reward=torch.randn((T, N), device="cuda"),
              next_state=s[1:], absorbing=torch.zeros((T, N), dtype=torch.bool, device="cuda"), last=last)
    agent.fit(ds)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps = 3
    for _ in range(reps):
        agent.fit(ds)
    torch.cuda.synchronize()
    res["vail_fit_100x4096_ms"] = (time.perf_counter() - t0) * 1e3 / reps
    res["vail_fit_minibatches"] = 3 * ((T * N + 255) // 256)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
