#!/usr/bin/env python3
"""K17: one TRPO policy step on the device (oly_trpo_step) against the float32 torch restatement of the same step on
the same GPU (tests/trpo_restate.py: autograd double backward for every Fisher-vector product; CG on device tensors,
and CG through the host every iteration as mushroom's numpy CG does), at n = 1000 and n = 409 600 rows (D = 32,
act = 11, UnitreeH1's max_kl / ent_coeff / n_epochs_cg).  Also one oly_trpo_fvp call alone: its time and TFLOP/s at
2.0 MFLOP per row.  Prints one JSON line.

    python tools/bench_trpo.py [--reps 5] [--sizes 1000,409600]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "olympics-mujoco_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import trpo_restate as tr  # noqa: E402
from test_trpo_cpu import make_case  # noqa: E402

D, A = 32, 11
CONF = dict(max_kl=5e-3, ent_coeff=1e-3, n_epochs_cg=25)


def flop_per_row(D=D, A=A):
    fwd = 2 * (512 * D + 512 * 256 + 256 * A)
    tangent = 2 * (512 * D + 2 * 512 * 256 + 2 * 256 * A)
    back = 2 * 256 * A + 4 * 256 * A + 4 * 512 * 256
    weights = 4 * 256 * A + 4 * 512 * 256 + 2 * 512 * D
    return fwd + tangent + back + weights


def timed(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        r = fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1000,409600")
    args = ap.parse_args()
    from olympic_hip.engine import Engine
    eng = Engine(0)
    res = dict(metric="trpo_step", D=D, act=A, **CONF, flop_per_row_fvp=flop_per_row())
    for n in (int(s) for s in args.sizes.split(",")):
        case = make_case(n=n, seed=9, prior=10000, device="cuda")
        ws = torch.empty(int(__import__("olympic_hip._ffi", fromlist=["lib"]).lib().oly_trpo_ws_floats(n, D, 512, 256, A)),
                         device="cuda")
        th, S = case["theta"].clone(), case["S"].clone()

        def dev():
            th.copy_(case["theta"])
            S.copy_(case["S"])
            return eng.trpo_step(case["x"], case["act"], case["adv"], S, th, ws=ws, **CONF)
        dev()
        t_dev, scal = timed(dev, args.reps)
        sc = scal.cpu().tolist()
        # one product alone
        c = tr.batch_stats(case["x"])
        mu_old = tr.forward(case["theta"], tr.standardise(case["x"], case["S"], c, 1, torch.float32), A)[2].contiguous()
        ls = case["theta"][-A:].contiguous()
        p = torch.randn_like(case["theta"])
        out = torch.empty_like(p)
        fvp = lambda: eng.trpo_fvp(case["x"], case["S"], case["theta"], mu_old, ls, p, k_stats=3, out=out, ws=ws)  # noqa: E731
        fvp()
        t_fvp, _ = timed(fvp, args.reps)
        row = dict(device_ms=t_dev, cg_iters=int(sc[1]), accepted_j=int(sc[3]), fvp_ms=t_fvp,
                   fvp_tflops=n * flop_per_row() / (t_fvp * 1e-3) / 1e12)
        reps_t = 1 if n > 100000 else args.reps
        for name, kw in (("torch_f32", dict(fvp=tr.fvp_autograd)), ("torch_f32_host_cg", dict(fvp=tr.fvp_autograd,
                                                                                               host_cg=True))):
            run = lambda: tr.trpo_step(case["theta"], case["S"], case["x"], case["act"], case["adv"],   # noqa: E731
                                       dtype=torch.float32, **kw, **CONF)
            run()
            t, r = timed(run, reps_t)
            row[f"{name}_ms"] = t
            row[f"{name}_cg_iters"] = r["k_run"]
            row[f"speedup_vs_{name}"] = t / t_dev
        res[f"n{n}"] = row
        print(f"# n={n}: {row}", file=sys.stderr)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
