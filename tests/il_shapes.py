"""The shapes at which the imitation-learning fit kernels (K15 oly_disc_fit_epoch, K16 oly_il_critic_fit_epoch, K17
oly_trpo_*) are compared with their float64 restatements, and the builders of those cases.  No tests here:
tests/test_il_shapes_cpu.py checks the tables and the yardstick without a GPU, tests/test_gpu_il_shapes.py runs the
kernels.

Every case is rebuilt from its seed.  The inputs have a scale and a shift per column, so a standardiser that is wrong
in one column changes the numbers; the parameters are nn.Linear's default initialisation at the case's own in_dim (K15,
K16: what VariationalDiscriminator and the critic's network start from) or test_trpo_cpu.make_case(D=, A=) (K17)."""
from collections import namedtuple

import numpy as np
import torch

import trpo_restate as tr
from test_trpo_cpu import make_case

TOL = 2e-5            # what the GPU tests allow per tensor against float64 (test_gpu_disc_fit.py, test_gpu_il_critic.py,
                      # test_gpu_trpo.py): the float32 restatement has to sit within TOL / 10, the fit has to move every
                      # tensor by 10 TOL

# ------------------------------------------------------------------------------ the tables
K15Case = namedtuple("K15Case", "in_dim batch n_rows n_plcy targets weight_decay seed lr")
K16Case = namedtuple("K16Case", "in_dim batch n seed lr")
K17Case = namedtuple("K17Case", "D A n seed prior")

K15_EPOCHS = K16_EPOCHS = 2
K15_HYPER = dict(info_c=0.1, lr_beta=1e-3)

K15_CASES = (   # minibatches per epoch in the comment
    K15Case(1, 7, 20, 10, False, 0.0, 1, 1e-3),            # 7, 7, 6: every 16-row tile partly empty, one column
    K15Case(17, 3, 10, 5, False, 0.0, 2, 1e-3),            # 3, 3, 3, 1: fewer rows than the weight kernel's split
    K15Case(17, 256, 257, 128, False, 0.0, 3, 1e-3),       # 256, 1
    K15Case(33, 4096, 4097, 2048, False, 0.0, 4, 1e-3),    # 4096 (256 loss partials), 1
    K15Case(33, 64, 199, 99, True, 0.0, 5, 1e-3),          # 64, 64, 64, 7
    K15Case(45, 100, 250, 125, False, 0.0, 6, 1e-3),       # 100, 100, 50
    K15Case(45, 512, 300, 300, False, 0.0, 7, 1e-3),       # batch > n_rows: 300 = 16 * 18 + 12; policy rows only
    K15Case(64, 255, 513, 200, True, 1e-3, 8, 1e-3),       # 255, 255, 3; explicit targets and weight decay
    K15Case(64, 333, 1022, 0, False, 0.0, 9, 1e-3),        # 333, 333, 333, 23 = 16 + 7; demonstration rows only
)

K16_CASES = (
    K16Case(1, 7, 20, 1, 1e-3),          # 7, 7, 6
    K16Case(17, 256, 257, 2, 1e-3),      # 256, 1
    K16Case(33, 100, 250, 3, 1e-3),      # 100, 100, 50
    K16Case(33, 100, 37, 4, 1e-3),       # batch > n
    K16Case(45, 255, 511, 23, 1e-3),     # 255, 255, 1
    K16Case(45, 255, 320, 6, 1e-3),      # 255, 65 = 64 + 1
    K16Case(64, 256, 385, 7, 1e-3),      # 256, 129 = 2 * 64 + 1
    K16Case(64, 1, 5, 8, 1e-3),          # five minibatches of one row
)

# The seeds of the two cases above 16 384 rows were chosen on the CPU (test_il_shapes_cpu.py holds them to it): with
# 16 000 rows x 768 hidden units some pre-activation lies within 1e-8 of zero, float32 cannot tell its sign, and one
# flipped ReLU mask moves the gradient by about 1 / (16 sqrt(n)) = 5e-4 of its norm, since the rows' contributions cancel
# to 1 / sqrt(n) of their sum.  Most seeds do that to torch's own float32 run; these are seeds where it does not, and
# where the smallest |pre-activation| relative to its terms is among the largest of 60 seeds tried.
K17_CASES = (
    K17Case(1, 1, 65, 1, 500),
    K17Case(1, 32, 63, 2, 0),
    K17Case(17, 1, 1, 21, 400),           # one row: the advantage is set by hand (its normalisation gives 0)
    K17Case(17, 12, 257, 20, 1000),
    K17Case(32, 11, 1, 5, 400),
    K17Case(45, 11, 63, 6, 0),
    K17Case(45, 12, 16384 + 300, 126, 5000),
    K17Case(64, 32, 257, 8, 0),
    K17Case(64, 32, 16385, 113, 20000),    # the second chunk holds one row
    K17Case(64, 12, 65, 10, 300),
)
K17_STEP = dict(max_kl=5e-3, ent_coeff=1e-3, n_epochs_cg=10)
K17_STEP_MIN_ROWS = 63                    # the whole step is run for the cases with at least this many rows


def case_id(c):
    return "-".join(f"{k}{int(v) if isinstance(v, bool) else v}" for k, v in zip(c._fields, c)
                    if k not in ("seed", "lr", "prior"))


def required_shapes_present():
    """The shapes the tables exist for; raises AssertionError naming the first one that is missing."""
    def last(n, batch):
        return n - ((n - 1) // batch) * batch
    k15, k16, k17 = K15_CASES, K16_CASES, K17_CASES
    assert len(set(k15)) == len(k15) and len(set(k16)) == len(k16) and len(set(k17)) == len(k17), "a case is listed twice"
    for d in (1, 17, 33, 45, 64):
        assert any(c.in_dim == d for c in k15), f"K15 in_dim {d}"
        assert any(c.in_dim == d for c in k16), f"K16 in_dim {d}"
    for c in k15 + k16:
        assert 0 < c.in_dim <= 64 and c.batch > 0
    assert all(0 <= c.n_plcy <= c.n_rows and c.batch <= 4096 for c in k15)
    assert all(c.batch <= 256 for c in k16)
    assert any(last(c.n_rows, c.batch) == 1 for c in k15), "K15 last minibatch of 1 row"
    assert any(last(c.n_rows, c.batch) == 3 for c in k15), "K15 last minibatch of 3 rows"
    assert any(last(c.n_rows, c.batch) % 16 == 7 and last(c.n_rows, c.batch) > 16 for c in k15), "K15 last of 16k + 7"
    assert any(c.batch > c.n_rows for c in k15), "K15 batch > n_rows"
    assert any(c.batch == 4096 and c.n_rows == 4097 for c in k15), "K15 batch 4096, 4097 rows"
    assert any(c.batch == 100 for c in k15), "K15 batch 100"
    assert any(c.n_plcy == 0 for c in k15) and any(c.n_plcy == c.n_rows for c in k15), "K15 n_plcy 0 and n_rows"
    assert any(c.targets and c.weight_decay == 1e-3 and c.in_dim > 32 for c in k15), "K15 targets + weight decay"
    for b in (1, 7, 100, 255, 256):
        assert any(c.batch == b for c in k16), f"K16 batch {b}"
    assert any(last(c.n, c.batch) == 1 and c.batch > 1 for c in k16), "K16 last minibatch of 1 row"
    assert any(last(c.n, c.batch) % 64 == 1 and last(c.n, c.batch) > 64 for c in k16), "K16 last of 64k + 1"
    for d in (1, 17, 45, 64):
        assert any(c.D == d for c in k17), f"K17 D {d}"
    for a in (1, 11, 12, 32):
        assert any(c.A == a for c in k17), f"K17 A {a}"
    for n in (1, 63, 65, 257, 16385, 16384 + 300):
        assert any(c.n == n for c in k17), f"K17 n {n}"
    assert all(0 < c.D <= 64 and 0 < c.A <= 32 and 0 < c.n <= 17000 for c in k17)
    assert K15_EPOCHS == 2 and K16_EPOCHS == 2


# ------------------------------------------------------------------------------ builders
def linear_params(dims, seed):
    """nn.Linear's default initialisation for the chain of (in, out) pairs, as float32 numpy [w, b, w, b, ...]."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        lins = [torch.nn.Linear(i, o) for i, o in dims]
    return [t.detach().numpy().copy() for lin in lins for t in (lin.weight, lin.bias)]


def disc_params(in_dim, seed):
    """VariationalDiscriminator(in_dim)'s parameters in oly_disc_pack's order (encoder 0, encoder 1, mu, logvar,
    decoder), drawn in the module's own construction order."""
    return linear_params([(in_dim, 256), (256, 128), (128, 128), (128, 128), (128, 1)], seed)


def critic_params(in_dim, seed, out_dim=1):
    return linear_params([(in_dim, 512), (512, 256), (256, out_dim)], seed)


def _columns(rng, in_dim):
    return rng.uniform(0.3, 3.0, in_dim), rng.standard_normal(in_dim) * 2.0


def disc_case(c, epochs=K15_EPOCHS):
    """(params, [(x [n,in] f32 policy rows first, perm, targets or None, noise [n,128] f32) per epoch], hyper)."""
    rng = np.random.default_rng(1000 + c.seed)
    scale, shift = _columns(rng, c.in_dim)
    out = []
    for _ in range(epochs):
        plcy = rng.standard_normal((c.n_plcy, c.in_dim)) * scale + shift
        demo = rng.standard_normal((c.n_rows - c.n_plcy, c.in_dim)) * scale * 0.8 + shift + 0.4 * scale
        t = None
        if c.targets:      # use_noisy_targets' ranges (gail_TRPO.py:209-211)
            t = np.concatenate([rng.uniform(0.01, 0.10, c.n_plcy),
                                rng.uniform(0.80, 0.99, c.n_rows - c.n_plcy)]).astype(np.float32)
        out.append((np.concatenate([plcy, demo]).astype(np.float32), rng.permutation(c.n_rows), t,
                    rng.standard_normal((c.n_rows, 128)).astype(np.float32)))
    hyper = dict(K15_HYPER, lr=c.lr, batch=c.batch, wd=c.weight_decay)
    return disc_params(c.in_dim, c.seed), out, hyper


def disc_restate(c, dtype=torch.float64, device="cpu", **kw):
    from test_disc_fit_cpu import restate_fit
    params, epochs, h = disc_case(c)
    args = dict(params=params, colstats=np.zeros((3, c.in_dim)))
    args.update(kw)
    return restate_fit(epochs, c.n_plcy, args.pop("params"), args.pop("colstats"), h["info_c"], h["lr_beta"], h["lr"],
                       h["batch"], wd=h["wd"], dtype=dtype, device=device, **args)


def critic_case(c, epochs=K16_EPOCHS):
    """(params, x [n,in] f32, v_target [n] f32, perms [epochs, n], colstats [3,in] f64: the statistics after one
    update_mean_std(x), as VAILAgent.fit leaves them before the critic's fit)."""
    rng = np.random.default_rng(2000 + c.seed)
    scale, shift = _columns(rng, c.in_dim)
    x = (rng.standard_normal((c.n, c.in_dim)) * scale + shift).astype(np.float32)
    vt = (0.5 * (x[:, 0] - shift[0]) / scale[0] + 0.3 * rng.standard_normal(c.n) + 0.2).astype(np.float32)
    perms = np.stack([rng.permutation(c.n) for _ in range(epochs)])
    xd = x.astype(np.float64)
    cs = np.stack([np.full(c.in_dim, float(c.n)), xd.sum(0), (xd * xd).sum(0)])
    return critic_params(c.in_dim, c.seed), x, vt, perms, cs


def critic_restate(c, dtype=torch.float64, device="cpu"):
    from test_il_critic_cpu import restate_fit
    params, x, vt, perms, cs = critic_case(c)
    return restate_fit(x, vt, perms, params, cs, c.lr, c.batch, dtype=dtype, device=device)


def trpo_case(c, device="cpu"):
    case = make_case(n=c.n, seed=c.seed, prior=c.prior, D=c.D, A=c.A, device=device)
    if c.n == 1:
        case["adv"] = torch.full((1,), 0.7, dtype=torch.float32, device=device)
    return case


def trpo_old_dist(case, D, A):
    """c, mu_old (S + c), log_sigma and old_log_prob (S + 2c) of the case's policy in float64."""
    th = case["theta"].double()
    c = tr.batch_stats(case["x"])
    mu_old = tr.forward(th, tr.standardise(case["x"], case["S"], c, 1, torch.float64), A)[2]
    mu2 = tr.forward(th, tr.standardise(case["x"], case["S"], c, 2, torch.float64), A)[2]
    ls = tr.split(th, D, A)[6]
    return c, mu_old, ls, tr.log_prob(mu2, case["act"].double(), ls)


def trpo_grad_fvp_reference(c, case, k, dtype=torch.float64):
    """(J, g, product, the float32 inputs the device is given) at S + k c.  The inputs (old_log_prob, mu_old, p) are
    rounded to float32 first, so both sides start from the same numbers; dtype is the arithmetic of the reference."""
    cc, mu_old, ls_old, logp_old = trpo_old_dist(case, c.D, c.A)
    th = case["theta"].to(dtype)
    xh = tr.standardise(case["x"], case["S"], cc, k, dtype)
    lp, mu32 = logp_old.float(), mu_old.float().contiguous()
    J, g = tr.grad(th, xh, case["act"].to(dtype), case["adv"].to(dtype), lp.to(dtype), K17_STEP["ent_coeff"])
    p = torch.randn(th.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(100 * c.seed + k))
    p = p.float().to(th.device)
    prod = tr.fvp_autograd(th, xh, mu32.to(dtype), ls_old.float().to(dtype), p.to(dtype), 0.1)
    return J, g, prod.detach(), dict(logp_old=lp.contiguous(), mu_old=mu32, log_sigma_old=ls_old.float().contiguous(), p=p)


def views(flat, shapes):
    out, o = [], 0
    for s in shapes:
        k = int(np.prod(s))
        out.append(flat[o:o + k].view(*s))
        o += k
    assert o == flat.numel()
    return out


# ------------------------------------------------------------------------------ guarded buffers
MARGIN = 64          # elements on each side; keeps the interior's alignment (256 bytes for float32)


class Guarded:
    """A tensor allocated as the interior of a larger one whose margins hold a sentinel.  `t` is the tensor to hand to
    a kernel; intact() says whether both margins still hold the sentinel."""
    SENTINEL = -7.0e33

    def __init__(self, shape, dtype, device="cuda", init=None):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        self.n = int(np.prod(shape))
        self.big = torch.full((self.n + 2 * MARGIN,), self.SENTINEL, dtype=dtype, device=device)
        self.t = self.big[MARGIN:MARGIN + self.n].view(shape)
        if init is None:
            self.t.zero_()
        else:
            self.t.copy_(torch.as_tensor(init).to(device=device, dtype=dtype).reshape(shape))

    def intact(self):
        lo, hi = self.big[:MARGIN], self.big[MARGIN + self.n:]
        s = self.big.new_tensor(self.SENTINEL)
        return bool((lo == s).all()) and bool((hi == s).all())


def guarded(shape, dtype, device="cuda", init=None):
    return Guarded(shape, dtype, device, init)


def all_intact(bufs):
    """bufs: {name: Guarded}; returns the names whose margins were written."""
    return [k for k, g in bufs.items() if not g.intact()]
