#!/usr/bin/env python3
"""K18 measurements, one JSON line: GAIL's discriminator-fit epoch call per minibatch of 2048 at the H1 kinematic width
(32) against the same loop in torch on the same GPU, written as the reference runs it (Standardizer update, forward,
GailDiscriminatorLoss, backward, torch.optim.Adam, loss.item()), two runs of each; DeviceGAILDiscriminatorTrainer.fit at
the reference launcher's size (n = 1000: one minibatch of 2000 rows) and at [100, 4096] (400 minibatches); GAILAgent.fit
on [100, 4096] with and without a discriminator call; the reward forward at 4096 and 409 600 rows against K16's relu
forward on the same shapes.  HIP events on the stream; every shape is warmed up first.

    python tools/bench_gail_disc_fit.py [--out FILE]

--in-dim D (states only at another width) and --pair next_state | action (the paired input, (s, s') at 32 + 32 or (s, a)
at 32 + 11, through oly_gail_disc_fit_epoch_pair) measure the epoch call alone, two runs:

    python tools/bench_gail_disc_fit.py --in-dim 64
    python tools/bench_gail_disc_fit.py --pair next_state
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "olympics-mujoco_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

IN, BATCH = 32, 2048
FLOP_PER_ROW = 3 * 2 * (IN * 512 + 512 * 256 + 256) - 2 * IN * 512   # forward, weight and data grads (no dX)


def timed(fn, reps, warmup=2):
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


def wall(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--epoch-only", action="store_true", help="only the epoch call (for a kernel trace)")
    ap.add_argument("--in-dim", type=int, default=IN, help="states-only input width; != 32: only the epoch call")
    ap.add_argument("--pair", choices=("next_state", "action"), default=None, help="the paired input: (s, s') at 32 + 32 or (s, a) at 32 + 11; only the epoch call is measured")
    args = ap.parse_args()
    ds, d2 = (32, 32 if args.pair == "next_state" else 11) if args.pair else (args.in_dim, 0)
    width = ds + d2
    args.epoch_only = args.epoch_only or width != IN or args.pair is not None
    from olympic_hip.engine import Engine
    from olympic_hip.gail import (DeviceStandardizer, GAILDiscriminator, GAILDiscriminatorReward,
                                  gail_discriminator_loss)
    from olympic_hip.il_agent import DeviceGAILDiscriminatorTrainer, DeviceILCritic, GAILAgent
    eng = Engine(0)
    torch.manual_seed(0)
    flop_per_row = 3 * 2 * (width * 512 + 512 * 256 + 256) - 2 * width * 512
    res = {"device": torch.cuda.get_device_name(0), "flop_per_row": flop_per_row, "in_dim": width, "pair": args.pair}

    # ---- the epoch call: 131 072 rows, 64 minibatches of 2048
    n = 131072
    nb = n // BATCH
    net = GAILDiscriminator(width).cuda()
    x = (torch.randn((n, ds), device="cuda") * 1.3 + 0.2).contiguous()
    x2 = (torch.randn((n, d2), device="cuda") * 0.8 + 0.5).contiguous() if args.pair else None
    perm = torch.randperm(n, device="cuda").to(torch.int32)
    ps = [t.detach() for lin in net._linears for t in (lin.weight, lin.bias)]
    flat = torch.cat([p.reshape(-1) for p in ps]).contiguous()
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    packed = eng.ilmlp_pack(*[p.contiguous() for p in ps])
    cs = eng.col_stats(x)
    ns = args.pair == "next_state"
    ws = eng.gail_disc_fit_pair_ws(BATCH, ds, d2, ns) if args.pair else eng.gail_disc_fit_ws(BATCH, width)
    step = [0]

    def epoch():
        if args.pair:
            eng.gail_disc_fit_epoch_pair(x, x2, ns, n // 2, perm, BATCH, cs, flat, m, v, packed, ws, step[0], 5e-6,
                                         entcoeff=1e-3)
        else:
            eng.gail_disc_fit_epoch(x, n // 2, perm, BATCH, cs, flat, m, v, packed, ws, step[0], 5e-6, entcoeff=1e-3)
        step[0] += nb
    runs = [timed(epoch, 5) for _ in range(2)]
    res["fit_us_per_minibatch_2048_runs"] = [ms * 1e3 / nb for ms in runs]
    res["fit_us_per_minibatch_2048"] = max(runs) * 1e3 / nb
    res["fit_tflops"] = flop_per_row * n / (max(runs) * 1e-3) / 1e12
    if args.epoch_only:
        print(json.dumps(res))
        return

    # torch: the reference's loop on the same GPU (statistics on the device instead of numpy)
    tnet = GAILDiscriminator(IN).cuda()
    opt = torch.optim.Adam(tnet.parameters(), lr=5e-6, weight_decay=0.0)
    tcs = torch.zeros((3, IN), dtype=torch.float64, device="cuda")
    p64 = perm.long()
    target = (torch.arange(n, device="cuda") >= n // 2).float()[:, None]
    n_torch = 32

    def torch_loop():
        for b in range(n_torch):
            idx = p64[b * BATCH:(b + 1) * BATCH]
            xd = x[idx].double()
            tcs[0] += BATCH
            tcs[1] += xd.sum(0)
            tcs[2] += (xd * xd).sum(0)
            cnt = tcs[0] + 1e-2
            mean = tcs[1] / cnt
            sd = torch.sqrt(torch.clamp((tcs[2] + 1e-2) / cnt - mean * mean, min=1e-2))
            loss = gail_discriminator_loss(tnet(((xd - mean) / sd).float()), target[idx], 1e-3)
            opt.zero_grad()
            loss.backward()
            opt.step()
            loss.item()
    truns = [timed(torch_loop, 3, warmup=1) for _ in range(2)]
    res["torch_us_per_minibatch_2048_runs"] = [ms * 1e3 / n_torch for ms in truns]
    res["torch_us_per_minibatch_2048"] = min(truns) * 1e3 / n_torch
    # the slower device run against the faster torch run
    res["fit_speedup"] = res["torch_us_per_minibatch_2048"] / res["fit_us_per_minibatch_2048"]

    # ---- the reward forward against K16's relu forward (the same stream, the same shapes)
    for B in (4096, 409600):
        xb = (torch.randn((B, IN), device="cuda") * 1.3 + 0.2).contiguous()
        y = torch.empty((B, 1), device="cuda")
        out = dict(reward=torch.empty(B, device="cuda"))
        reps = 200 if B == 4096 else 20
        t_relu = timed(lambda: eng.ilmlp_forward(xb, packed, 1, colstats=cs, y=y), reps)
        t_tanh = timed(lambda: eng.gail_disc_forward(xb, packed, colstats=cs, want=("reward",), out=out), reps)
        res[f"reward_forward_{B}_ms"] = t_tanh
        res[f"relu_forward_{B}_ms"] = t_relu
        res[f"reward_over_relu_{B}"] = t_tanh / t_relu

    # ---- DeviceGAILDiscriminatorTrainer.fit: n = 1000 (one minibatch of 2000) and [100, 4096] (400 minibatches)
    # as many demonstration rows as policy rows at [100, 4096], so that every fit draws m = n of them
    demo = np.random.default_rng(0).normal(0.2, 1.0, (100 * 4096, IN)).astype(np.float32)
    r = GAILDiscriminatorReward(eng, GAILDiscriminator(IN).cuda())
    tr = DeviceGAILDiscriminatorTrainer(r, demo)
    g = torch.Generator(device="cuda").manual_seed(0)
    small = torch.randn((1000, IN), device="cuda")
    res["trainer_fit_n1000_ms"] = wall(lambda: tr.fit(small, generator=g), 20, warmup=3)
    big = torch.randn((100 * 4096, IN), device="cuda")
    res["trainer_fit_100x4096_ms"] = wall(lambda: tr.fit(big, generator=g), 3)
    res["trainer_fit_100x4096_minibatches"] = (2 * 100 * 4096 + BATCH - 1) // BATCH

    # ---- GAILAgent.fit, [T=100, N=4096], no-op policy step, with and without the discriminator's fit
    T, N = 100, 4096
    s = torch.randn((T + 1, N, IN), device="cuda")
    last = torch.zeros((T, N), dtype=torch.bool, device="cuda")
    last[-1] = True
    ds = dict(state=s[:-1], action=torch.randn((T, N, 11), device="cuda"), reward=torch.randn((T, N), device="cuda"),
              next_state=s[1:], absorbing=torch.zeros((T, N), dtype=torch.bool, device="cuda"), last=last)
    for key, every in (("gail_fit_100x4096_with_disc_ms", 1), ("gail_fit_100x4096_without_disc_ms", 10 ** 9)):
        lins = [torch.nn.Linear(IN, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 1)]
        rr = GAILDiscriminatorReward(eng, GAILDiscriminator(IN).cuda())
        agent = GAILAgent(eng, rr, DeviceGAILDiscriminatorTrainer(rr, demo),
                          DeviceILCritic(eng, lins, DeviceStandardizer(eng, IN)), lambda o, a, adv, ag: None,
                          train_D_n_th_epoch=every)
        res[key] = wall(lambda: agent.fit(ds, generator=g), 2)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
