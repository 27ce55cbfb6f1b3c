"""A float64 restatement of one acting step of the imitation-learning collection loop (K21, oly_il_act):
GaussianTorchPolicy.draw_action through FullyConnectedNetwork.forward (networks.py:68-81) and _preprocess_action's
control vector.  No tests here: tests/test_gpu_il_act.py compares the kernel with it.

    statistics  += (n, sum, sumsq) of x's columns (Standardizer.update_mean_std, the derivation of gail.py:36-43)
    xs           = f32((f64(x) - mean) / std)           float64 statistics, then narrowed (networks.py:68-74)
    mu           = W3 relu(W2 relu(W1 xs + b1) + b2) + b3   in float64
    action       = mu + exp(log_sigma) eps
    ctrl[j]      = clamp(action[k] delta[k] + mean[k], lo[k], hi[k]),  k the action slot of actuator j (spec tables)

mushroom-rl's GaussianTorchPolicy is not part of the reference tree: distribution_t(s) = N(mu(s), diag(exp(log_sigma))^2)
is a READING of mushroom-rl >= 1.10, as in olympic_hip.il_agent.DeviceGaussianPolicy.
"""
import numpy as np

from disc_log_restate import TOL as DEV_TOL   # noqa: F401  (the project's device tolerance, relative to max(1, |value|))
from disc_log_restate import Stats
from iter_log_restate import forward


def restate_act(params, log_sigma, colstats, x, eps=None, update_stats=True, device="cpu"):
    """params: W1, b1, W2, b2, W3, b3 of the mean network; colstats [3,in] the raw running sums on entry; x [n,in] f32.
    Returns dict(mu [n,act] f64, action [n,act] f64, colstats [3,in] f64 after the call)."""
    x = np.asarray(x, dtype=np.float32)
    st = Stats.from_colstats(colstats)
    if update_stats:
        st.add(x)
    mu = forward(params, st.standardise(x), device)
    action = mu if eps is None else mu + np.exp(np.asarray(log_sigma, dtype=np.float64)) * np.asarray(eps, dtype=np.float64)
    return dict(mu=mu, action=action, colstats=st.colstats())


def restate_ctrl(spec, action):
    """clamp(_preprocess_action(action)) in actuator order from the spec's tables, float64; actuators no action slot
    drives stay 0.  Returns (ctrl [n,nu] f64, clamped [n,nu] bool)."""
    a = np.asarray(action, dtype=np.float32).astype(np.float64)
    n = a.shape[0]
    ctrl, clamped = np.zeros((n, spec.nu)), np.zeros((n, spec.nu), bool)
    for k, j in enumerate(np.asarray(spec.act_to_ctrl)):
        u = a[:, k] * float(spec.act_delta[k]) + float(spec.act_mean[k])
        lo, hi = float(spec.ctrl_lo[k]), float(spec.ctrl_hi[k])
        clamped[:, j] = (u < lo) | (u > hi)
        ctrl[:, j] = np.minimum(np.maximum(u, lo), hi)
    return ctrl, clamped
