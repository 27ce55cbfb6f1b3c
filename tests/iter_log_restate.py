"""A float64 restatement of _logging_sw (imitation_lib/imitation/gail_TRPO.py:163, 251-272): the six scalars it hands to
the writer and the two batches its forwards add to the policy / critic Standardizer.  No tests here:
tests/test_iter_log_cpu.py holds it to the reference-run fixtures of tests/golden/iter_log/, and tests/test_gpu_iter_log.py
compares K20 (oly_episode_stats, oly_iter_log) with it.

mushroom-rl is not part of the reference tree; compute_J, compute_episodes_length, Regressor.__call__ and
GaussianTorchPolicy.distribution / entropy are READINGS of mushroom-rl >= 1.10 (each marked below).

`reading` selects which statistics the two forwards standardise with (S the live statistics on entry, c the batch's):
    "sequence"    the reference's: self._V(x) adds the batch and sees S + c, self.policy.distribution(x) adds it again
                  and sees S + 2c (networks.py:68-81)
    "live"        a deliberately WRONG one: both forwards standardise with S
    "policy_s1"   a deliberately WRONG one: the policy's forward sees S + c as the critic's does
`count_open_length=True` is a deliberately WRONG reading of compute_episodes_length that appends the trailing open episode.
"""
import os
import sys

import numpy as np
import torch

from disc_log_restate import Stats

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
FIXTURE_DIR = os.path.join(GOLDEN, "iter_log")
CASES = ("a", "b")
NAMES = ("EpTrueRewMean", "EpRewMean", "EpLenMean", "vf_loss", "entropy", "kl")
READINGS = {"sequence": (1, 2), "live": (0, 0), "policy_s1": (1, 1)}
EPISODE = (0, 1)              # float64 on both sides: compared to 1e-12 relative
EP_TOL = 1e-12
FLOOR = 1e-6                  # eight float32 ulps: the floor of DESIGN section 13's rule max(4 spread, 1e-6)
LOG2PIE = float(np.log(2 * np.pi * np.e))


def fixture(case):
    return os.path.join(FIXTURE_DIR, f"{case}.npz")


def rel_err(got, want):
    """Per scalar, relative to the value itself (a max(1, |v|) scale would accept a KL of zero)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.abs(got - want) / np.abs(want)


def tolerances(spread):
    """The device tolerance per scalar from the measured float32-fixture-versus-float64 spread: four times the spread
    (the project's convention, DESIGN section 13, whose floor of 1e-6 stands for the float32 rounding of a result whose
    spread happens to be small), the episode means 1e-12 and EpLenMean exact."""
    tol = np.maximum(4 * np.asarray(spread, dtype=np.float64), FLOOR)
    tol[list(EPISODE)] = EP_TOL
    tol[2] = 0.0
    return tol


# ---- READING of mushroom_rl.utils.dataset.compute_J / compute_episodes_length (>= 1.10), per environment
def column_returns(reward, last, gamma=1.0):
    js, j, k = [], 0.0, 0
    for i in range(len(reward)):
        j += gamma ** k * float(reward[i])
        k += 1
        if last[i] or i == len(reward) - 1:
            js.append(j)
            j, k = 0.0, 0
    return js


def column_lengths(last, count_open_length=False):
    ls, l = [], 0
    for i in range(len(last)):
        l += 1
        if last[i]:
            ls.append(l)
            l = 0
    if count_open_length and l > 0:
        ls.append(l)
    return ls
# ---- end of the reading


def episode_stats(reward, last, gamma=1.0, reward2=None, count_open_length=False):
    """oly_episode_stats' out [8] for [T,N] blocks, every column one dataset: mean return, mean return of reward2, mean
    length (NaN without a completed episode), returns, lengths, and the three sums."""
    reward, last = np.asarray(reward), np.asarray(last).astype(bool)
    T, N = reward.shape
    js, js2, ls = [], [], []
    for e in range(N):
        js += column_returns(reward[:, e], last[:, e], gamma)
        if reward2 is not None:
            js2 += column_returns(np.asarray(reward2)[:, e], last[:, e], gamma)
        ls += column_lengths(last[:, e], count_open_length)
    s1, s2, sl = float(np.sum(js)), float(np.sum(js2)) if js2 else 0.0, float(np.sum(ls)) if ls else 0.0
    return np.array([s1 / len(js), s2 / len(js) if js2 else 0.0, sl / len(ls) if ls else float("nan"), len(js), len(ls),
                     s1, s2, sl])


def forward(P, xs, device="cpu"):
    """The relu MLP in -> 512 -> 256 -> out in float64 (P: W1, b1, W2, b2, W3, b3)."""
    P = [torch.as_tensor(np.asarray(p)).to(device=device, dtype=torch.float64) for p in P]
    h = torch.as_tensor(np.asarray(xs)).to(device=device, dtype=torch.float64)
    h = torch.relu(h @ P[0].T + P[1])
    h = torch.relu(h @ P[2].T + P[3])
    return (h @ P[4].T + P[5]).cpu().numpy()


def kl_rows(mu_old, ls_old, mu, ls):
    """kl_divergence(MultivariateNormal(mu_old, diag(exp(ls_old))), MultivariateNormal(mu, diag(exp(ls)))) per row."""
    mu_old, ls_old, mu, ls = (np.asarray(a, dtype=np.float64) for a in (mu_old, ls_old, mu, ls))
    half = np.sum(ls - ls_old)
    t2 = np.sum((np.exp(ls_old) / np.exp(ls)) ** 2)
    t3 = np.sum(((mu - mu_old) / np.exp(ls)) ** 2, axis=1)
    return half + 0.5 * (t2 + t3 - mu.shape[1])


def old_means(policy, colstats0, x, device="cpu"):
    """old_pol_dist's means (gail_TRPO.py:132-133): the deep copy's forward adds the batch to ITS Standardizer (colstats0
    + c, then discarded), narrowed to the float32 the tensor is held in."""
    st = Stats.from_colstats(colstats0)
    st.add(x)
    return forward(policy, st.standardise(x), device).astype(np.float32)


def restate_iter_log(critic, policy, log_sigma, mu_old, ls_old, colstats, x, v_target, r_env, r, last, reading="sequence",
                     count_open_length=False, device="cpu"):
    """_logging_sw on x [n,D] (row t N + e), v_target [n], the old distribution, the raw colstats [3,D] on entry and the
    [T,N] blocks r_env (the environment's reward), r (the reward trained on) and last.  Returns dict(scalars [8] f64 in
    oly_iter_log's order, colstats [3,D] f64 after the call, v, mu)."""
    k_v, k_p = READINGS[reading]
    x = np.asarray(x, dtype=np.float32)
    st = Stats.from_colstats(colstats)
    blocks = [Stats.from_colstats(colstats)]
    for _ in range(2):
        st.add(x)
        blocks.append(Stats.from_colstats(st.colstats()))
    # ---- READING of Regressor.__call__: the network's forward over the whole batch
    v = forward(critic, blocks[k_v].standardise(x), device).reshape(-1)
    # ---- READING of GaussianTorchPolicy.distribution: N(mu(x), diag(exp(log_sigma))^2)
    mu = forward(policy, blocks[k_p].standardise(x), device)
    ep = episode_stats(r_env, last, 1.0, reward2=r, count_open_length=count_open_length)
    ls = np.asarray(log_sigma, dtype=np.float64)
    o = np.zeros(8)
    o[0], o[1] = ep[0], ep[1]
    o[2] = np.round(ep[2])                                     # half to even, as int(np.round(.)); NaN stays NaN
    o[3] = float(np.mean((v - np.asarray(v_target, dtype=np.float64).reshape(-1)) ** 2))
    o[4] = 0.5 * ls.shape[0] * LOG2PIE + float(np.sum(ls))     # ---- READING of GaussianTorchPolicy.entropy
    o[5] = float(np.mean(kl_rows(mu_old, ls_old, mu, ls)))
    o[6], o[7] = ep[2], ep[4]
    return dict(scalars=o, colstats=st.colstats(), v=v, mu=mu)


def load_case(case, device="cpu"):
    """The inputs of a fixture rebuilt from its seeds, as restate_iter_log's keyword arguments, and the fixture itself."""
    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)
    import gen_iter_log as gen
    g = np.load(fixture(case))
    return gen.case_args(case, g, device=device), g
