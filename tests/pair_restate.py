"""A float64 restatement of the discriminators on PAIRED inputs, (s, s') with use_next_states and (s, a) with actions:
the reward (make_discrim_reward, gail_TRPO.py:320-327) and _fit_discriminator's epochs (gail_TRPO.py:174-218) for
GAIL's DiscriminatorNetwork and VAIL's VariationalNet (networks.py:216-234, 258-284).  No tests here:
tests/test_disc_pair_cpu.py holds it to the reference-run fixtures of tests/golden/disc_pair_fit/, and
tests/test_gpu_disc_pair.py compares the kernels with it.

The rule the fixtures pin (networks.py:224-227 / 266-270): one forward updates the Standardizer TWICE in next-state
mode.  _stand(states) adds the states' rows and standardises them with the result S1; _stand(next_states) adds the next
states' rows and standardises them with S2 = S1 + s'.  The halves of a row use different statistics and the count rises
by 2 B.  With actions there is one update and the actions go in as they are.  `variant` selects a deliberately WRONG
reading, for the test that shows the fixtures tell them apart:
    "two"      the reference's rule
    "shared"   both halves standardised with S2
    "count_b"  the next states' sums are added but the count rises by B only
"""
import os
import sys

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import gen_disc_pair_fit as gen  # noqa: E402  (inputs / init_params: the parts of the fixtures rebuilt from seeds)

FIXTURE_DIR = os.path.join(GOLDEN, "disc_pair_fit")
CASES = tuple(gen.CASES)
VARIANTS = ("two", "shared", "count_b")


def fixture(case):
    return os.path.join(FIXTURE_DIR, f"{case}.npz")


def moments_of(cs):
    cnt = cs[0] + 1e-2
    mean = cs[1] / cnt
    return mean, torch.sqrt(torch.clamp((cs[2] + 1e-2) / cnt - mean * mean, min=1e-2))


def add_rows(cs, x, count=True):
    """Standardizer.update_mean_std (networks.py:76-81) on the float64 running (count, sum, sumsq) rows."""
    xd = x.to(torch.float64)
    if count:
        cs[0] += xd.shape[0]
    cs[1] += xd.sum(0)
    cs[2] += (xd * xd).sum(0)


def network_input(cs, s, second, standardise, dtype, variant="two"):
    """preprocess_inputs (networks.py:216-234): updates cs in place, returns [standardise(s) | second] as
    f32((f64(x) - mean) / std) values in `dtype`."""
    assert variant in VARIANTS
    add_rows(cs, s)
    m1, d1 = moments_of(cs)
    if standardise:
        add_rows(cs, second, count=variant != "count_b")
        m2, d2 = moments_of(cs)
        if variant == "shared":
            m1, d1 = m2, d2
        b = ((second.to(torch.float64) - m2) / d2).to(torch.float32)
    else:
        b = second.to(torch.float32)
    a = ((s.to(torch.float64) - m1) / d1).to(torch.float32)
    return torch.cat([a, b], dim=1).to(dtype)


def gail_forward(P, xs):
    h1 = torch.tanh(xs @ P[0].T + P[1])
    h2 = torch.tanh(h1 @ P[2].T + P[3])
    return (h2 @ P[4].T + P[5]).reshape(-1)


def vail_forward(P, xs, noise):
    h1 = torch.relu(xs @ P[0].T + P[1])
    h2 = torch.relu(h1 @ P[2].T + P[3])
    mu, lv = h2 @ P[4].T + P[5], h2 @ P[6].T + P[7]
    z = mu if noise is None else mu + torch.exp(lv / 2) * noise
    return (z @ P[8].T + P[9]).reshape(-1), mu, lv


def gail_loss(d, t, entcoeff):
    """GailDiscriminatorLoss.forward (imitation_lib/utils/math.py:22-36) -> (loss, bce, ent)."""
    bce = torch.mean(torch.clamp(d, min=0) - d * t + torch.log1p(torch.exp(-torch.abs(d))))
    ent = torch.mean((1.0 - torch.sigmoid(d)) * d - torch.nn.functional.logsigmoid(d))
    return bce - entcoeff * ent, bce, ent


def _t(a, device, dtype=None):
    a = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
    return a.to(device) if dtype is None else a.to(device=device, dtype=dtype)


def restate_reward(algo, params, colstats, s, second, standardise, noise=None, dtype=torch.float64, device="cpu",
                   variant="two"):
    """make_discrim_reward on masked s [B,Ds], second [B,D2] -> (logits, reward, colstats after)."""
    P = [_t(p, device, dtype) for p in params]
    cs = _t(colstats, device, torch.float64).clone()
    xs = network_input(cs, _t(s, device), _t(second, device), standardise, dtype, variant)
    d = gail_forward(P, xs) if algo == "gail" else vail_forward(P, xs, None if noise is None else _t(noise, device, dtype))[0]
    return d, -torch.log(1.0 - torch.sigmoid(d) + 1e-8), cs


def restate_fit(algo, epochs, n_plcy, params, colstats, standardise, lr, batch, wd=0.0, entcoeff=1e-3, info_c=0.1,
                lr_beta=1e-3, beta=0.1, step0=0, moments=None, dtype=torch.float64, device="cpu", betas=(0.9, 0.999),
                eps=1e-8, variant="two"):
    """_fit_discriminator's epochs on a paired input.  epochs: [(s [n,Ds] f32, second [n,D2] f32, both masked and
    concatenated policy rows first; perm; targets or None; noise [n,128] in minibatch order or None (GAIL))].  Per epoch
    the explicit update_mean_std of the STATES (gail_TRPO.py:206), then per minibatch network_input (the Standardizer's
    one or two updates), the forward, the loss and torch's Adam step with L2 weight decay.
    Returns (params, moments, colstats, records, step[, beta])."""
    P = [_t(p, device, dtype).clone() for p in params]
    M = [torch.zeros_like(p) for p in P] if moments is None else [m.clone() for m in moments[0]]
    V = [torch.zeros_like(p) for p in P] if moments is None else [v.clone() for v in moments[1]]
    cs = _t(colstats, device, torch.float64).clone()
    rec = {k: [] for k in (("loss", "bce", "ent") if algo == "gail" else ("loss", "bce", "kl", "beta"))}
    step = step0
    for s, second, perm, targets, noise in epochs:
        s, second = _t(s, device), _t(second, device)
        n = s.shape[0]
        t_all = (_t(targets, device) if targets is not None else
                 (torch.arange(n, device=device) >= n_plcy).to(torch.float32)).to(dtype)
        perm = torch.as_tensor(np.asarray(perm, dtype=np.int64), device=device)
        noise = None if noise is None else _t(noise, device, dtype)
        add_rows(cs, s)
        for b in range((n + batch - 1) // batch):
            idx = perm[b * batch:min(n, (b + 1) * batch)]
            xs = network_input(cs, s[idx], second[idx], standardise, dtype, variant)
            for p in P:
                p.requires_grad_(True)
            if algo == "gail":
                loss, bce, ent = gail_loss(gail_forward(P, xs), t_all[idx], entcoeff)
                vals = dict(loss=loss, bce=bce, ent=ent)
            else:
                d, mu, lv = vail_forward(P, xs, noise[b * batch:b * batch + idx.shape[0]])
                bce = torch.nn.functional.binary_cross_entropy_with_logits(d, t_all[idx])
                kl = (0.5 * torch.sum(mu * mu + torch.exp(lv) - lv - 1, dim=1)).mean()
                loss = bce + beta * (kl - info_c)
                vals = dict(loss=loss, bce=bce, kl=kl)
            grads = torch.autograd.grad(loss, P)
            for k, v in vals.items():
                rec[k].append(float(v.detach()))
            if algo != "gail":
                beta = max(0.0, beta + lr_beta * (float(kl.detach()) - info_c))
                rec["beta"].append(beta)
            step += 1
            bc1, bc2 = 1 - betas[0] ** step, 1 - betas[1] ** step
            with torch.no_grad():
                for i in range(len(P)):
                    p, gr = P[i].detach(), grads[i]
                    if wd:
                        gr = gr + wd * p
                    M[i] = M[i] + (gr - M[i]) * (1 - betas[0])
                    V[i] = V[i] * betas[1] + (1 - betas[1]) * gr * gr
                    P[i] = p - (lr / bc1) * (M[i] / (torch.sqrt(V[i]) / bc2 ** 0.5 + eps))
    out = ([p.detach() for p in P], (M, V), cs, {k: np.array(v) for k, v in rec.items()}, step)
    return out if algo == "gail" else out + (beta,)


# ------------------------------------------------------------------------------ the fixtures' cases
def case_algo(case):
    return gen.CASES[case]["algo"]


def case_standardise(case):
    return gen.CASES[case]["pair"] == "next_state"


def case_epochs(g, case, data=None):
    """Per epoch (s, second, perm, targets or None, noise or None) as the fixture's run drew them."""
    data = gen.inputs() if data is None else data
    ns = case_standardise(case)
    m2 = g["state_mask"] if ns else g["act_mask"]
    plcy = data["plcy_obs"][:, g["state_mask"]]
    plcy2 = (data["plcy_next"] if ns else data["plcy_act"])[:, m2]
    noise = None if case_algo(case) == "gail" else gen.noise(case)
    out = []
    for e in range(g["perms"].shape[0]):
        idx = g["demo_idx"][e]
        demo = data["demo_states"][idx][:, g["state_mask"]]
        demo2 = (data["demo_next_states"] if ns else data["demo_actions"])[idx][:, m2]
        t = g["targets"][e] if "targets" in g.files else None
        n = 2 * plcy.shape[0]
        out.append((np.concatenate([plcy, demo]), np.concatenate([plcy2, demo2]), g["perms"][e], t,
                    None if noise is None else noise[e * n:(e + 1) * n]))
    return out


def case_hold(g, case, data=None):
    """(s, second, noise or None) of the held-out reward evaluation, masked."""
    data = gen.inputs() if data is None else data
    ns = case_standardise(case)
    second = (data["hold_next"][:, g["state_mask"]] if ns else data["hold_act"][:, g["act_mask"]])
    noise = None if case_algo(case) == "gail" else gen.noise(case)[-gen.N_HOLD:]
    return np.ascontiguousarray(data["hold_obs"][:, g["state_mask"]]), np.ascontiguousarray(second), noise


def case_hyper(g, case):
    h = dict(lr=float(g["lr"]), batch=int(g["batch"]), wd=float(g["wd"]))
    for k in ("entcoeff", "info_c", "lr_beta"):
        if k in g.files:
            h[k] = float(g[k])
    return h


def restate_case(case, g=None, dtype=torch.float64, device="cpu", variant="two"):
    """The whole fixture run: the fit from the initial parameters and zero statistics, then the held-out reward.
    Returns dict(params, colstats_fit, rec, step, logits, reward, colstats)."""
    g = np.load(fixture(case)) if g is None else g
    algo, ns = case_algo(case), case_standardise(case)
    data = gen.inputs()
    out = restate_fit(algo, case_epochs(g, case, data), gen.N_PLCY, gen.init_params(case), np.zeros((3, gen.DS)), ns,
                      dtype=dtype, device=device, variant=variant, **case_hyper(g, case))
    s, second, noise = case_hold(g, case, data)
    d, r, cs = restate_reward(algo, out[0], out[2], s, second, ns, noise=noise, dtype=dtype, device=device, variant=variant)
    return dict(params=out[0], moments=out[1], colstats_fit=out[2], rec=out[3], step=out[4], logits=d, reward=r, colstats=cs)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def check_statistics(cs, g, prefix="st"):
    """The fp64 running (count, sum, sumsq) against the reference Standardizer's own sums (float32 in numpy), with
    test_disc_fit_cpu.check_statistics' bounds."""
    cs = np.asarray(cs)
    np.testing.assert_allclose(cs[0] + 1e-2, np.full(cs.shape[1], g[f"{prefix}_count"][0]), rtol=0, atol=1e-9)
    np.testing.assert_allclose(cs[1], g[f"{prefix}_sum"], rtol=1e-5, atol=1e-2)
    np.testing.assert_allclose(cs[2] + 1e-2, g[f"{prefix}_sumsq"], rtol=1e-5)
