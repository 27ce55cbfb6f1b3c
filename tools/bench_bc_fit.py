#!/usr/bin/env python3
"""K24 measurements, one JSON line: one step of oly_bc_fit_steps at batch 32 and 256 (in = 32, A = 11, 20 000
demonstration rows, a Standardizer) as the mean over a 1000-step call and as a 1-step call, against the reference's loop
restated in torch eager on the same GPU (the same network, the Standardizer's update on the device, GaussianNLLLoss,
backward, torch.optim.Adam).  Every figure is the median of REPS timed windows after a warm-up; HIP events on the stream.

    python tools/bench_bc_fit.py [--out FILE] [--kernel-only]

--kernel-only leaves the torch loop out (a kernel trace of the run then holds K24's launches alone).
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

REPS = 7
IN_DIM, ACT_DIM, N_ROWS = 32, 11, 20000


def timed(fn, reps, warmup=2):
    """Median milliseconds of `reps` windows of one fn() each."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-only", action="store_true", help="time the device path alone")
    args = ap.parse_args()
    from olympic_hip.bc import DeviceBehavioralCloning, DeviceSquashedGaussianPolicy
    from olympic_hip.engine import Engine
    from olympic_hip.gail import DeviceStandardizer
    eng = Engine(0)
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    states = torch.as_tensor((rng.standard_normal((N_ROWS, IN_DIM)) * rng.uniform(0.3, 3, IN_DIM)).astype(np.float32)).cuda()
    actions = torch.as_tensor(np.tanh(rng.standard_normal((N_ROWS, ACT_DIM))).astype(np.float32)).cuda()
    res = {"device": torch.cuda.get_device_name(0), "in_dim": IN_DIM, "act_dim": ACT_DIM, "rows": N_ROWS, "reps": REPS}
    gen = torch.Generator(device="cuda").manual_seed(0)
    for batch in (32, 256):
        lins = [torch.nn.Linear(IN_DIM, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 2 * ACT_DIM)]
        pol = DeviceSquashedGaussianPolicy(eng, lins, -np.ones(ACT_DIM), np.ones(ACT_DIM),
                                           standardizer=DeviceStandardizer(eng, IN_DIM))
        bc = DeviceBehavioralCloning(eng, pol, dict(states=states, actions=actions), lr=1e-4, batch_size=batch)
        idx1000, idx1 = bc.draw_idx(1000, gen), bc.draw_idx(1, gen)
        ms = timed(lambda: bc.fit_offline(1000, idx=idx1000), REPS)
        res[f"kernel_us_per_step_b{batch}_call1000"] = ms  # ms per 1000 steps = us per step
        many = 200
        ms = timed(lambda: [bc.fit_offline(1, idx=idx1) for _ in range(many)], REPS)
        res[f"kernel_us_per_step_b{batch}_call1"] = ms * 1e3 / many

        if args.kernel_only:
            continue
        # torch eager: the reference's loop on the same GPU
        net = torch.nn.Sequential(torch.nn.Linear(IN_DIM, 512), torch.nn.ReLU(), torch.nn.Linear(512, 256), torch.nn.ReLU(),
                                  torch.nn.Linear(256, 2 * ACT_DIM)).cuda()
        opt = torch.optim.Adam(net.parameters(), lr=1e-4)
        loss_fn = torch.nn.GaussianNLLLoss()
        cs = torch.zeros((3, IN_DIM), dtype=torch.float64, device="cuda")
        targets = bc.targets
        rows = idx1000.long()
        n_torch = 200

        def torch_loop():
            for s in range(n_torch):
                r = rows[s]
                xd = states[r].double()
                cs[0] += batch
                cs[1] += xd.sum(0)
                cs[2] += (xd * xd).sum(0)
                cnt = cs[0] + 1e-2
                mean = cs[1] / cnt
                sd = torch.sqrt(torch.clamp((cs[2] + 1e-2) / cnt - mean * mean, min=1e-2))
                y = net(((xd - mean) / sd).float())
                mu, log_sigma = y[:, :ACT_DIM], torch.clamp(y[:, ACT_DIM:], -20.0, 2.0)
                loss = loss_fn(input=mu, target=targets[r], var=torch.square(log_sigma.exp()))
                opt.zero_grad()
                loss.backward()
                opt.step()
        ms = timed(torch_loop, REPS, warmup=1)
        res[f"torch_us_per_step_b{batch}"] = ms * 1e3 / n_torch
        res[f"speedup_b{batch}_call1000"] = res[f"torch_us_per_step_b{batch}"] / res[f"kernel_us_per_step_b{batch}_call1000"]
        res[f"speedup_b{batch}_call1"] = res[f"torch_us_per_step_b{batch}"] / res[f"kernel_us_per_step_b{batch}_call1"]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
