"""A restatement of K17's TRPO policy step in torch, in any dtype and on any device: the float64
yardstick of tests/test_trpo_cpu.py and tests/test_gpu_trpo.py, and the float32 torch step tools/bench_trpo.py times.

It follows the table of the step (the k-th forward standardises with S + k c, c added k times in sequence) and
mushroom-rl's TRPO as this project reads it (>= 1.10; mushroom-rl is not part of the reference).  The Fisher-vector
product is written as forward-over-reverse (fvp_rop); fvp_autograd is torch's double backward of the same KL, and
fvp_rop(..., gauss_newton=True) drops the second-order term sum (Delta / s) d2mu, which the drift of the statistics
makes non-zero at theta_0."""
import math

import torch

H1, H2 = 512, 256
LOG2PI = math.log(2 * math.pi)
LOG2PIE = math.log(2 * math.pi * math.e)


def n_params(D, A):
    return H1 * D + H1 + H2 * H1 + H2 + A * H2 + A + A


def split(theta, D, A):
    """W1, b1, W2, b2, W3, b3, log_sigma views of a flat vector in mushroom's order."""
    shapes = [(H1, D), (H1,), (H2, H1), (H2,), (A, H2), (A,), (A,)]
    out, o = [], 0
    for s in shapes:
        k = math.prod(s)
        out.append(theta[o:o + k].view(s))
        o += k
    return out


def batch_stats(x):
    """c = the batch's (count, sum, sumsq) per column, float64."""
    xd = x.double()
    return torch.stack([torch.full((x.shape[1],), float(x.shape[0]), dtype=torch.float64, device=x.device),
                        xd.sum(0), (xd * xd).sum(0)])


def add_k(S, c, k):
    """S + c + c + ... (k times, in sequence), as k Standardizer.forward calls leave it."""
    S = S.clone()
    for _ in range(k):
        S = S + c
    return S


def standardise(x, S, c, k, dtype):
    Sk = add_k(S, c, k)
    cnt = Sk[0] + 1e-2
    mean = Sk[1] / cnt
    sd = torch.sqrt(torch.clamp((Sk[2] + 1e-2) / cnt - mean * mean, min=1e-2))
    return ((x.double() - mean) / sd).to(dtype)


def forward(theta, xh, A):
    W1, b1, W2, b2, W3, b3, _ = split(theta, xh.shape[1], A)
    h1 = torch.relu(xh @ W1.T + b1)
    h2 = torch.relu(h1 @ W2.T + b2)
    return h1, h2, h2 @ W3.T + b3


def log_prob(mu, act, ls):
    sigma = torch.exp(ls)
    u = (act - mu) / sigma
    return -0.5 * (mu.shape[1] * LOG2PI + (u * u).sum(1)) - torch.log(sigma).sum()


def entropy(ls):
    return 0.5 * ls.shape[0] * LOG2PIE + ls.sum()


def kl_rows(mu_old, ls_old, mu, ls):
    """kl_divergence(N(mu_old, exp(ls_old)^2), N(mu, exp(ls)^2)) per row, diagonal covariances."""
    half = (ls - ls_old).sum()
    t2 = ((torch.exp(ls_old) / torch.exp(ls)) ** 2).sum()
    t3 = (((mu - mu_old) / torch.exp(ls)) ** 2).sum(1)
    return half + 0.5 * (t2 + t3 - mu.shape[1])


def surrogate(theta, xh, act, adv, logp_old, ent_coeff):
    A = act.shape[1]
    mu = forward(theta, xh, A)[2]
    ls = split(theta, xh.shape[1], A)[6]
    ratio = torch.exp(log_prob(mu, act, ls) - logp_old)
    return torch.mean(ratio * adv) + ent_coeff * entropy(ls)


def grad(theta, xh, act, adv, logp_old, ent_coeff):
    """(J, dJ/dtheta) by autograd (first order)."""
    th = theta.detach().clone().requires_grad_(True)
    J = surrogate(th, xh, act, adv, logp_old, ent_coeff)
    g, = torch.autograd.grad(J, th)
    return J.detach(), g


def fvp_autograd(theta, xh, mu_old, ls_old, p, damping):
    """torch's double backward: grad(grad(mean KL) . p) + damping p (_fisher_vector_product_t)."""
    A = mu_old.shape[1]
    th = theta.detach().clone().requires_grad_(True)
    mu = forward(th, xh, A)[2]
    kl = kl_rows(mu_old, ls_old, mu, split(th, xh.shape[1], A)[6]).mean()
    g, = torch.autograd.grad(kl, th, create_graph=True)
    hv, = torch.autograd.grad((g * p).sum(), th)
    return hv + damping * p


def fvp_rop(theta, xh, mu_old, ls_old, p, damping, gauss_newton=False):
    """The same product written out: tangent forward, both backward chains, outer products."""
    n, D = xh.shape
    A = mu_old.shape[1]
    W1, b1, W2, b2, W3, b3, ls = split(theta, D, A)
    V1, vb1, V2, vb2, V3, vb3, vl = split(p, D, A)
    z1 = xh @ W1.T + b1
    m1 = (z1 > 0).to(xh.dtype)
    h1 = z1 * m1
    z2 = h1 @ W2.T + b2
    m2 = (z2 > 0).to(xh.dtype)
    h2 = z2 * m2
    mu = h2 @ W3.T + b3
    s, s_old = torch.exp(ls) ** 2, torch.exp(ls_old) ** 2
    dl = mu - mu_old
    hd1 = m1 * (xh @ V1.T + vb1)
    hd2 = m2 * (h1 @ V2.T + hd1 @ W2.T + vb2)
    mud = h2 @ V3.T + hd2 @ W3.T + vb3
    d3 = dl / (s * n)
    dd3 = (mud - 2 * dl * vl) / (s * n)
    if gauss_newton:
        d3 = torch.zeros_like(d3)
    d2 = m2 * (d3 @ W3)
    dd2 = m2 * (d3 @ V3 + dd3 @ W3)
    dd1 = m1 * (d2 @ V2 + dd2 @ W2)
    hv = [dd1.T @ xh, dd1.sum(0), dd2.T @ h1 + d2.T @ hd1, dd2.sum(0), dd3.T @ h2 + d3.T @ hd2, dd3.sum(0),
          ((-2 * dl * mud + 2 * (s_old + dl * dl) * vl) / s).mean(0)]
    return torch.cat([t.reshape(-1) for t in hv]) + damping * p


def trpo_step(theta, S, x, act, adv, max_kl, ent_coeff, n_epochs_cg, cg_damping=1e-1, cg_residual_tol=1e-10,
              n_epochs_line_search=10, accept_rule="or", dtype=torch.float64, fvp=fvp_rop, host_cg=False):
    """One step (gail_TRPO.py:131-149 with mushroom's TRPO, this project's reading).  theta [n_par], S [3, D] f64 (the
    live statistics), x [n, D], act [n, A], adv [n].  host_cg: the CG vectors go through the host every iteration, as
    mushroom's numpy CG does.  Returns a dict: theta, S, prev_loss, k_run, shs, j (-1: restored), kl, J, j_run,
    stepdir, full_step."""
    A = act.shape[1]
    D = x.shape[1]
    th0 = theta.detach().to(dtype)
    act, adv = act.to(dtype), adv.reshape(-1).to(dtype)
    c = batch_stats(x)
    xs = lambda k: standardise(x, S, c, k, dtype)       # noqa: E731
    ls0 = split(th0, D, A)[6]
    with torch.no_grad():
        mu_old = forward(th0, xs(1), A)[2]
        logp_old = log_prob(forward(th0, xs(2), A)[2], act, ls0)
    prev_loss, g = grad(th0, xs(1), act, adv, logp_old, ent_coeff)
    with torch.no_grad() if fvp is fvp_rop else torch.enable_grad():
        F = lambda k, v: fvp(th0, xs(k), mu_old, ls0, v, cg_damping)    # noqa: E731
        p, r = g.clone(), g.clone()
        xv = torch.zeros_like(g)
        r2 = r.dot(r).cpu() if host_cg else r.dot(r)
        k_run = 0
        for i in range(n_epochs_cg):
            z = F(2 + i, p).detach()
            if host_cg:
                p, z, r, xv = p.cpu(), z.cpu(), r.cpu(), xv.cpu()
            v = r2 / p.dot(z)
            xv = xv + v * p
            r = r - v * z
            r2n = r.dot(r)
            p = r + (r2n / r2) * p
            r2 = r2n
            if host_cg:
                p, r, xv = p.to(g.device), r.to(g.device), xv.to(g.device)
            k_run += 1
            if float(r2) < cg_residual_tol:
                break
        direction = F(2 + k_run, xv).detach()
    with torch.no_grad():
        shs = 0.5 * xv.dot(direction)
        full = xv / torch.sqrt(shs / max_kl)
        j_acc, j_run, kl, J, th = -1, 0, float("nan"), float("nan"), th0
        for j in range(n_epochs_line_search):
            th = th0 + full * (0.5 ** j)
            J = float(surrogate(th, xs(3 + k_run + 2 * j), act, adv, logp_old, ent_coeff))
            kl = float(kl_rows(mu_old, ls0, forward(th, xs(4 + k_run + 2 * j), A)[2], split(th, D, A)[6]).mean())
            j_run = j + 1
            fin = math.isfinite(J) and math.isfinite(kl) and math.isfinite(float(shs))
            kl_ok, up = kl <= 1.5 * max_kl, J - float(prev_loss) >= 0
            if fin and ((kl_ok and up) if accept_rule == "and" else (kl_ok or up)):
                j_acc = j
                break
        th_new = th if j_acc >= 0 else th0
    return dict(theta=th_new, S=add_k(S, c, 2 + k_run + 2 * j_run), prev_loss=float(prev_loss), k_run=k_run,
                shs=float(shs), j=j_acc, kl=kl, J=J, j_run=j_run, stepdir=xv, full_step=full)
