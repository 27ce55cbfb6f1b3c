"""A float64 restatement of _discriminator_logging (imitation_lib/imitation/gail_TRPO.py:222-249, extended by
vail_TRPO.py:23-32): the chain of statistics its six (VAIL: seven) forwards leave in the discriminator's Standardizer and
the scalars it hands to the writer.  No tests here: tests/test_disc_log_cpu.py holds it to the reference-run fixtures of
tests/golden/disc_log/, and tests/test_gpu_disc_log.py compares K19 (oly_gail_disc_log, oly_disc_log) with it.

The forwards, in the reference's order, and what each adds to the Standardizer before it standardises (networks.py:68-81;
with next states the states' rows, then the next states' rows, :224-227):

    1 all rows   2 demonstration half   3 policy half   4 all rows   5 demonstration half   6 policy half   (7 all rows)

`chain` selects the reading:
    "sequence"   the reference's: every forward adds its own rows
    "single"     a deliberately WRONG one: the batch is added once and every forward standardises with that (S1)
    "all_each"   a deliberately WRONG one: every forward adds the whole batch (c_all once per forward, whichever rows it
                 evaluates), which is what a replay by `S + k c` would do
`stats` selects the arithmetic of the running sums: "f64" (what the device keeps) or "ref" (the reference's own: numpy's
float32 column sums added to float32 running sums, networks.py:76-79, so that the final statistics can be compared with
the fixture's to the last bit).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
FIXTURE_DIR = os.path.join(GOLDEN, "disc_log")
CASES = ("gail_s", "gail_ns", "vail_s", "vail_sa")
CHAINS = ("sequence", "single", "all_each")
NAMES = ("DiscrimLoss", "D_Generator_Accuracy", "D_Out_Generator", "D_Expert_Accuracy", "D_Out_Expert", "Bernoulli Ent.",
         "Neg. Bernoulli Ent. Loss (incl. in DiscrimLoss)", "Generator_loss", "Expert_Loss", "Bottleneck_Loss", "Beta",
         "Bottleneck_Loss_times_Beta")
ACCURACIES = (1, 3)           # step functions of the logits: compared exactly
TOL = 2e-5                    # the project's device tolerance, relative to max(1, |value|)
BAND = 1e-4                   # no float64 logit of a fixture lies within this of 0


def fixture(case):
    return os.path.join(FIXTURE_DIR, f"{case}.npz")


def tolerances(spread):
    """The device tolerance per scalar from the measured float32-fixture-versus-float64 spread (relative to
    max(1, |value|)): the project's 2e-5 wherever the spread is below a tenth of it, else four times the spread."""
    spread = np.asarray(spread, dtype=np.float64)
    return np.where(spread < TOL / 10, TOL, 4 * spread)


class Stats:
    """The Standardizer's running (count, sum, sumsq), offsets included (networks.py:54-56)."""

    def __init__(self, count, s, sq, ref=False):
        self.ref = ref
        dt = np.float32 if ref else np.float64
        self.count, self.sum, self.sumsq = float(count), np.asarray(s, dtype=dt).copy(), np.asarray(sq, dtype=dt).copy()

    @classmethod
    def from_colstats(cls, cs, ref=False):
        cs = np.asarray(cs, dtype=np.float64)
        return cls(cs[0, 0] + 1e-2, cs[1], cs[2] + 1e-2, ref)

    def colstats(self):
        d = self.sum.shape[0]
        return np.stack([np.full(d, self.count - 1e-2), self.sum.astype(np.float64), self.sumsq.astype(np.float64) - 1e-2])

    def add(self, x):
        x = np.asarray(x, dtype=np.float32)
        if not self.ref:
            x = x.astype(np.float64)
        self.sum = self.sum + x.sum(axis=0).ravel()
        self.sumsq = self.sumsq + np.square(x).sum(axis=0).ravel()
        self.count += len(x)

    def moments(self):
        count = np.array([self.count])                          # a float64 array, as the reference's _count
        mean = self.sum / count
        return mean, np.sqrt(np.maximum(self.sumsq / count - np.square(mean), 1e-2))

    def standardise(self, x):
        mean, std = self.moments()
        return ((np.asarray(x, dtype=np.float32) - mean) / std).astype(np.float32)      # float64 statistics, then narrowed


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


def forward_rows(n, n_plcy, vail):
    """(first row, rows) of each forward."""
    parts = [(0, n), (n_plcy, n - n_plcy), (0, n_plcy)]
    return parts + parts + ([(0, n)] if vail else [])


def restate_log(algo, params, colstats, x, n_plcy, x2=None, pair=None, targets=None, entcoeff=1e-3, beta=0.1, info_c=0.1,
                lr_beta=1e-5, noise=None, chain="sequence", stats="f64", dtype=torch.float64, device="cpu"):
    """_discriminator_logging on the masked concatenated rows x [n,Ds] (policy rows first) and the second part x2
    [n,D2] (pair "next_state" or "action") from the raw colstats [3,Ds].  noise: VAIL's six blocks in forward order, or
    None (z = mu).  device: where the networks' float64 forwards run (the statistics stay in numpy).  Returns dict(scalars [12] f64, colstats [3,Ds] f64 after the call, logits: one array per forward,
    blocks: the statistics each forward used as (after the states, after the next states))."""
    assert chain in CHAINS and stats in ("f64", "ref") and algo in ("gail", "vail") and pair in (None, "next_state", "action")
    vail = algo == "vail"
    P = [torch.as_tensor(np.asarray(p)).to(device=device, dtype=dtype) for p in params]
    x = np.asarray(x, dtype=np.float32)
    n = x.shape[0]
    t_all = (np.concatenate([np.zeros(n_plcy), np.ones(n - n_plcy)]) if targets is None
             else np.asarray(targets, dtype=np.float64).reshape(-1))
    st = Stats.from_colstats(colstats, ref=stats == "ref")
    logits, lat, blocks = [], [], []
    for k, (r0, R) in enumerate(forward_rows(n, n_plcy, vail)):
        rows = slice(r0, r0 + R)
        srows = rows if chain == "sequence" else slice(0, n)
        add = chain != "single" or k == 0
        if add:
            st.add(x[srows])
        a = st.standardise(x[rows])
        blk_a = st.colstats()
        if pair == "next_state":
            if add:
                st.add(x2[srows])
            b = st.standardise(x2[rows])
        elif pair == "action":
            b = np.asarray(x2[rows], dtype=np.float32)
        blocks.append((blk_a, st.colstats()))
        xs = torch.as_tensor(a if pair is None else np.concatenate([a, b], axis=1)).to(device=device, dtype=dtype)
        if vail:
            eps = None if (noise is None or k >= 6) else torch.as_tensor(np.asarray(noise[k])).to(device=device, dtype=dtype)
            d, mu, lv = vail_forward(P, xs, eps)
            lat.append((mu.double().cpu().numpy(), lv.double().cpu().numpy()))
        else:
            d = gail_forward(P, xs)
        logits.append(d.double().cpu().numpy())

    def bce(k, t):
        d = logits[k]
        return float(np.mean(np.maximum(d, 0) - d * t + np.log1p(np.exp(-np.abs(d)))))

    def sig(d):
        return 1.0 / (1.0 + np.exp(-d))

    def ent(k):
        d = logits[k]
        logsig = -(np.maximum(-d, 0) + np.log1p(np.exp(-np.abs(d))))
        return float(np.mean((1.0 - sig(d)) * d - logsig))

    def bottleneck(k):
        mu, lv = lat[k]
        return float(np.mean(0.5 * np.sum(mu * mu + np.exp(lv) - lv - 1.0, axis=1)) - info_c)

    o = np.zeros(12)
    t_plcy, t_demo = t_all[:n_plcy], t_all[n_plcy:]
    o[1] = float(np.mean(sig(logits[2]) < 0.5))
    o[2] = float(np.mean(sig(logits[2])))
    o[3] = float(np.mean(sig(logits[1]) > 0.5))
    o[4] = float(np.mean(sig(logits[1])))
    o[5] = ent(3)
    o[6] = -entcoeff * o[5]
    if not vail:
        o[0] = bce(0, t_all) - entcoeff * ent(0)
        o[8] = (bce(4, t_demo) - entcoeff * ent(4)) / 2
        o[7] = (bce(5, t_plcy) - entcoeff * ent(5)) / 2
    else:
        # one deepcopy of the VDBLoss serves the three loss evaluations (gail_TRPO.py:225), and VDBLoss.forward moves its
        # beta every time (math.py:70, 80-81, float32); forward 7 goes through a fresh copy (vail_TRPO.py:27)
        f32 = np.float32
        b0 = f32(beta)
        bl1, bl5, bl6, bl7 = bottleneck(0), bottleneck(4), bottleneck(5), bottleneck(6)
        b1 = max(f32(0), f32(b0 + f32(lr_beta) * f32(bl1)))
        b2 = max(f32(0), f32(b1 + f32(lr_beta) * f32(bl5)))
        o[0] = bce(0, t_all) + float(b0) * bl1
        o[8] = (bce(4, t_demo) + float(b1) * bl5) / 2
        o[7] = (bce(5, t_plcy) + float(b2) * bl6) / 2
        o[9], o[10], o[11] = bl7, float(b0), float(b0) * bl7
    return dict(scalars=o, colstats=st.colstats(), logits=logits, blocks=blocks, stats=st)


def load_case(case):
    """The inputs of a fixture rebuilt from its seeds, as restate_log's keyword arguments, and the fixture itself."""
    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)
    import gen_disc_log as gen
    g = np.load(fixture(case))
    return gen.case_args(case, g), g
