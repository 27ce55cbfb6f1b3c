#!/usr/bin/env python3
"""K20: one _logging_sw call on the device (oly_iter_log) including the read-back of its scalars, against the same
sequence in torch on the same GPU written the way the reference runs it: the Standardizer's sums on the host from a copy
of the batch for each of the two forwards (networks.py:68-81), the forwards in float32 torch, F.mse_loss and torch's
kl_divergence of two MultivariateNormals, and compute_J / compute_episodes_length as Python loops over host copies of the
[T, N] blocks.  obs 32, act 11.  Also oly_episode_stats alone at the same blocks.  Prints one JSON line.

    python tools/bench_iter_log.py [--reps 5] [--shapes 100x4096,250x4]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "olympics-mujoco_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import iter_log_restate as rs  # noqa: E402

D, A = 32, 11


def timed(fn, reps):
    """Host clock around the call, its read-back included; the median of `reps`."""
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), r


def case(T, N, seed=3):
    rng = np.random.default_rng(seed)
    n = T * N
    scale, shift = rng.uniform(0.3, 3.0, D), rng.normal(0, 2, D)
    x = (rng.normal(0, 1, (n, D)) * scale + shift).astype(np.float32)

    def net(out_dim):
        shapes = ((512, D), (512,), (256, 512), (256,), (out_dim, 256), (out_dim,))
        return [(rng.standard_normal(s) * (1.4, 1.4, 0.5)[i // 2] / np.sqrt(s[1])).astype(np.float32) if i % 2 == 0
                else (rng.uniform(-1, 1, s) * 0.1).astype(np.float32) for i, s in enumerate(shapes)]
    last = rng.random((T, N)) < 1 / 40
    last[-1] = True
    cs = np.stack([np.full(D, 10000.0), 10000.0 * shift, 10000.0 * (scale ** 2 + shift ** 2)])
    return dict(critic=net(1), policy=net(A), log_sigma=np.full(A, -0.7, dtype=np.float32),
                mu_old=rng.normal(0, 0.3, (n, A)).astype(np.float32), ls_old=np.full(A, -0.69, dtype=np.float32), colstats=cs,
                x=x, v_target=rng.normal(0, 1, n).astype(np.float32), r_env=rng.uniform(0.2, 1.2, (T, N)).astype(np.float32),
                r=rng.uniform(0.05, 2.0, (T, N)).astype(np.float32), last=last)


def torch_sequence(t, nets):
    """_logging_sw as the reference runs it, on the GPU where it can and through the host where the reference does."""
    cnt, s, sq = (v.copy() for v in t["host_stats"])
    outs = []
    for net in nets:
        xh = t["x"].cpu().numpy()                                     # Standardizer.forward: inputs.detach().cpu().numpy()
        s, sq, cnt = s + xh.sum(axis=0), sq + np.square(xh).sum(axis=0), cnt + len(xh)
        mean = s / cnt
        std = np.sqrt(np.maximum(sq / cnt - np.square(mean), 1e-2))
        z = ((t["x"] - torch.tensor(mean).to("cuda")) / torch.tensor(std).to("cuda")).float()
        outs.append(net(z))
    v_err = torch.nn.functional.mse_loss(torch.tensor(outs[0].cpu().numpy()), torch.tensor(t["vt"].cpu().numpy()))
    old = torch.distributions.MultivariateNormal(loc=t["mo"], scale_tril=torch.diag(torch.exp(t["lo"])))
    new = torch.distributions.MultivariateNormal(loc=outs[1], scale_tril=torch.diag(torch.exp(t["ls"])))
    kl = torch.mean(torch.distributions.kl.kl_divergence(old, new))
    ent = A / 2 * np.log(2 * np.pi * np.e) + torch.sum(t["ls"])
    ep = rs.episode_stats(t["re"].cpu().numpy(), t["last"].cpu().numpy(), 1.0, reward2=t["r"].cpu().numpy())
    return [ep[0], ep[1], float(np.round(ep[2])), float(v_err), float(ent), float(kl)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="100x4096,250x4")
    args = ap.parse_args()
    from olympic_hip.engine import Engine
    eng = Engine(0)
    dev = lambda a, dt=None: torch.as_tensor(np.asarray(a)).to(device="cuda", dtype=dt).contiguous()   # noqa: E731
    res = dict(metric="iter_log", D=D, act=A)
    for T, N in (tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")):
        a = case(T, N)
        n = T * N
        t = dict(x=dev(a["x"]), vt=dev(a["v_target"]), mo=dev(a["mu_old"]), lo=dev(a["ls_old"]), ls=dev(a["log_sigma"]),
                 pc=eng.ilmlp_pack(*[dev(p) for p in a["critic"]]), pp=eng.ilmlp_pack(*[dev(p) for p in a["policy"]]),
                 re=dev(a["r_env"]), r=dev(a["r"]), last=dev(a["last"]), ws=eng.iter_log_ws(n),
                 host_stats=(np.array([a["colstats"][0, 0] + 1e-2]), a["colstats"][1].astype(np.float32),
                             (a["colstats"][2] + 1e-2).astype(np.float32)))
        cs0, cs, out = dev(a["colstats"]), dev(a["colstats"]), torch.empty(8, dtype=torch.float64, device="cuda")

        def device_call():
            cs.copy_(cs0)
            return eng.iter_log(t["x"], t["vt"], t["mo"], t["lo"], t["ls"], t["pc"], t["pp"], t["re"], t["r"], t["last"], cs,
                                t["ws"], out=out).cpu().tolist()

        def enqueue_only():
            cs.copy_(cs0)
            t0 = time.perf_counter()
            eng.iter_log(t["x"], t["vt"], t["mo"], t["lo"], t["ls"], t["pc"], t["pp"], t["re"], t["r"], t["last"], cs, t["ws"],
                         out=out)
            return (time.perf_counter() - t0) * 1e3
        device_call()
        t_dev, got = timed(device_call, args.reps)
        t_enq = statistics.median(timed(enqueue_only, 1)[1] for _ in range(args.reps))
        t_ep, _ = timed(lambda: eng.episode_stats(t["re"], t["last"], reward2=t["r"]).cpu().tolist(), args.reps)

        def mlp(params):
            lins = [torch.nn.Linear(p.shape[1], p.shape[0]) for p in params[::2]]
            with torch.no_grad():
                for lin, w, b in zip(lins, params[::2], params[1::2]):
                    lin.weight.copy_(torch.as_tensor(w))
                    lin.bias.copy_(torch.as_tensor(b))
            return torch.nn.Sequential(lins[0], torch.nn.ReLU(), lins[1], torch.nn.ReLU(), lins[2]).cuda()
        nets = (mlp(a["critic"]), mlp(a["policy"]))
        with torch.no_grad():
            torch_sequence(t, nets)
            t_torch, want = timed(lambda: torch_sequence(t, nets), 1 if n > 100000 else args.reps)
        chunks = (n + 16383) // 16384
        row = dict(rows=n, launches=2 + 2 + 1 + 4 * chunks + 1, device_ms=t_dev, enqueue_ms=t_enq, episode_stats_ms=t_ep,
                   torch_ms=t_torch, speedup=t_torch / t_dev,
                   max_rel_diff=float(np.max(np.abs(np.array(got[:6]) - np.array(want)) / np.abs(np.array(want)))))
        res[f"{T}x{N}"] = row
        print(f"# [{T}, {N}]: {row}", file=sys.stderr)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
