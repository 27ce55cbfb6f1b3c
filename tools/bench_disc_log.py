#!/usr/bin/env python3
"""K19 measurements, one JSON line: one diagnostics call (oly_gail_disc_log / oly_disc_log through the engine) at the
reference launcher's size with disc_batch_size rows (2 x 2048) and at [100, 4096] policy rows (2 x 409 600), against the
same sequence written in torch on the same GPU the way the reference runs it: the Standardizer's sums on the host from a
copy of every forward's rows, the statistics sent back, the network's forward on the device, its output brought to the
host, the scalars formed there (gail_TRPO.py:222-249, vail_TRPO.py:23-32; networks.py:68-81).

Per size and algorithm: the device call's time by a host clock around work that ends in a synchronise, two runs, the
slower one reported; the torch sequence's likewise, the FASTER one reported; their ratio; the time the host needs to
enqueue the device call (it returns long before the device finishes at the large size: there is no synchronisation
inside); and the launch count, computed from the shapes.  Every shape is warmed up first.

    python tools/bench_disc_log.py [--out FILE] [--small-only]
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
import torch.nn.functional as F  # noqa: E402

DS, CHUNK = 32, 16384


def wall(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def launches(n, n_plcy, vail, next_states=False):
    chunks = lambda r: (r + CHUNK - 1) // CHUNK
    per_triple = chunks(n) + chunks(n - n_plcy) + chunks(n_plcy)
    fwd_chunks = 2 * per_triple + (chunks(n) if vail else 0)
    return dict(statistics=2 * (4 if next_states else 2), chain=1, forwards=fwd_chunks, reductions=fwd_chunks, finish=1,
                total=2 * (4 if next_states else 2) + 1 + 2 * fwd_chunks + 1)


class HostStandardizer:
    """The reference's Standardizer as it runs with the network on a GPU: every forward copies its rows to the host, adds
    their column sums there and sends mean and std back."""

    def __init__(self, dim):
        self.sum, self.sumsq, self.count = np.zeros(dim), np.full(dim, 1e-2), 1e-2

    def __call__(self, x):
        h = x.detach().cpu().numpy()
        self.sum = self.sum + h.sum(axis=0)
        self.sumsq = self.sumsq + np.square(h).sum(axis=0)
        self.count += len(h)
        mean = self.sum / self.count
        std = np.sqrt(np.maximum(self.sumsq / self.count - np.square(mean), 1e-2))
        return ((x - torch.tensor(mean).to(x.device)) / torch.tensor(std).to(x.device)).float()


def torch_log(net, stand, vail, x, n_plcy, targets, entcoeff=1e-3, beta=0.1, info_c=0.1, lr_beta=1e-5):
    """The logging sequence: six (seven) forwards whose outputs go to the host, scalars from host tensors."""
    def D(rows):
        with torch.no_grad():
            xs = stand(rows)
            if not vail:
                return net(xs).cpu()
            mu, lv = net.encode(xs)
            z = mu + torch.exp(lv / 2) * torch.randn_like(lv)
            return net.decoder(z).cpu(), mu.cpu(), lv.cpu()

    def ent(d):
        return (1.0 - torch.sigmoid(d)) * d - F.logsigmoid(d)

    def kl(mu, lv):
        return (0.5 * torch.sum(mu * mu + torch.exp(lv) - lv - 1, dim=1)).mean() - info_c

    def loss(out, t, b):
        if not vail:
            d = out
            bce = torch.mean(torch.clamp(d, min=0) - d * t + torch.log(1 + torch.exp(-torch.abs(d))))
            return bce - entcoeff * torch.mean(ent(d)), b
        d, mu, lv = out
        bl = kl(mu, lv)
        return F.binary_cross_entropy_with_logits(d.squeeze(), t.squeeze()) + b * bl, max(0.0, float(b + lr_beta * bl))
    first = (lambda o: o[0]) if vail else (lambda o: o)
    plcy, demo = x[:n_plcy], x[n_plcy:]
    o = []
    l0, b1 = loss(D(x), targets, beta)
    o.append(float(l0))
    d_exp, d_pl = torch.sigmoid(first(D(demo))), torch.sigmoid(first(D(plcy)))
    o += [float((d_pl < 0.5).float().mean()), float(d_pl.mean()), float((d_exp > 0.5).float().mean()), float(d_exp.mean())]
    e = float(torch.mean(ent(first(D(x)))))
    o += [e, -entcoeff * e]
    le, b2 = loss(D(demo), targets[n_plcy:], b1)
    lg, _ = loss(D(plcy), targets[:n_plcy], b2)
    o += [float(lg) / 2, float(le) / 2]
    if vail:
        _, mu, lv = D(x)
        bl = float(kl(mu, lv))
        o += [bl, beta, beta * bl]
    return o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small-only", action="store_true", help="only 2 x 2048 rows")
    args = ap.parse_args()
    from olympic_hip.engine import Engine
    from olympic_hip.gail import GAILDiscriminator, VariationalDiscriminator
    eng = Engine(0)
    torch.manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "in_dim": DS}
    sizes = [("2x2048", 2048)] + ([] if args.small_only else [("2x409600", 100 * 4096)])
    for algo in ("gail", "vail"):
        vail = algo == "vail"
        net = (VariationalDiscriminator(in_dim=DS) if vail else GAILDiscriminator(DS)).cuda()
        if vail:
            ps = [net.encoder[0].weight, net.encoder[0].bias, net.encoder[1].weight, net.encoder[1].bias, net.mu_out.weight,
                  net.mu_out.bias, net.logvar_out.weight, net.logvar_out.bias, net.decoder.weight, net.decoder.bias]
            packed = eng.disc_pack(*[p.detach().contiguous() for p in ps])
        else:
            packed = eng.ilmlp_pack(*[t.detach().contiguous() for lin in net._linears for t in (lin.weight, lin.bias)])
        for label, n_plcy in sizes:
            n = 2 * n_plcy
            x = (torch.randn((n, DS), device="cuda") * 1.3 + 0.2).contiguous()
            cs = eng.col_stats(x)
            ws = eng.disc_log_ws(n) if vail else eng.gail_disc_log_ws(n)
            out = torch.zeros(12, dtype=torch.float64, device="cuda")
            beta = torch.full((1,), 0.1, device="cuda")
            eps = torch.randn((4 * n, 128), device="cuda") if vail else None

            def dev():
                if vail:
                    eng.disc_log(x, n_plcy, cs, packed, beta, ws, eps=eps, out=out)
                else:
                    eng.gail_disc_log(x, n_plcy, cs, packed, ws, out=out)

            def dev_read():
                dev()
                return out.cpu()                                  # the one read-back of the 12 doubles
            reps = 50 if n_plcy == 2048 else 3
            druns = [wall(dev_read, reps) for _ in range(2)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dev()
            enqueue = (time.perf_counter() - t0) * 1e3
            torch.cuda.synchronize()
            stand = HostStandardizer(DS)
            stand(x)
            targets = (torch.arange(n) >= n_plcy).float()[:, None]
            treps = 10 if n_plcy == 2048 else 2
            truns = [wall(lambda: torch_log(net, stand, vail, x, n_plcy, targets), treps, warmup=1) for _ in range(2)]
            key = f"{algo}_{label}"
            res[key] = dict(device_ms_runs=druns, device_ms=max(druns), torch_ms_runs=truns, torch_ms=min(truns),
                            torch_over_device=min(truns) / max(druns), enqueue_ms=enqueue,
                            launches=launches(n, n_plcy, vail))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
