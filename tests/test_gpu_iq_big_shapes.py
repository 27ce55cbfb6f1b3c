"""K26 and K27 at large batches on the MI355X: oly_iq_q_update (IQ, SQIL, LSIQ, LSIQ_H / LSIQ_HC), oly_iq_pi_update with one
critic and with two, and oly_iq_alpha_update at the shapes, configs and seeds of tests/iq_big_shapes.py (257 to 4096 rows,
two updates each) against the float64 restatements the small sweeps use, in the fenced device state of those sweeps' own
test files with workspaces of exactly the reported size; and at the same shapes the bits across runs, a workspace reused
after a larger batch, Q's bits against the forward kernel and LSIQ_H's running maximum against torch's float32 expression.

The rule is the small sweeps': per tensor |kernel - f64| <= max(TOL, 4 |f32 - f64|) with TOL = 2e-5, the moments relative
to their largest entry, the scalars as tests/test_gpu_iq_q.py compares them (iq_big_shapes.q_errors, pi_errors,
alpha_errors); tests/test_iq_big_shapes_cpu.py holds the float32 run of every case within TOL / 4 and shows that one misread
row misses this rule ten times over.  Every test prints error, tolerance and their ratio before it asserts."""
import gc

import numpy as np
import pytest
import torch

import iq_big_shapes as S
import iq_pi_restate as P
from fences import assert_intact, fenced
from test_gpu_iq_pi import Dev as PiDev, split as pi_split
from test_gpu_iq_q import Dev, check_q_values_have_the_forward_kernels_bits, split
from test_gpu_lsiq_h import HDev
from test_gpu_lsiq_h_actor import HPiDev
from test_gpu_lsiq_q import LDev, same_bits

pytestmark = pytest.mark.gpu
TOL = S.TOL
DEV = dict(iq=Dev, lsiq=LDev, h=HDev)


@pytest.fixture(scope="module")
def eng():
    from olympic_hip.engine import Engine
    e = Engine(0)
    yield e
    torch.cuda.synchronize()
    e.ctx.close()
    gc.collect()


def q_dev(eng, fam, cfg, k, params):
    in_dim, A, B, _ = S.K26_SHAPES[k]
    dev = DEV[fam](eng, params, cfg, in_dim, A, B)
    assert dev.t("ws").numel() == dev.nws
    return dev


def q_updates(dev, fam, cfg, steps, n_policy):
    return torch.stack([dev.update(s, n_policy) for s in S.q_steps(fam, cfg, steps, n_policy)])


def report(who, errs):
    for name, e, t in errs:
        print(f"{who} {name}: |kernel - f64| {e:.3e}, tolerance {t:.3e}, ratio {e / t:.3f}")
    bad = [(n, e, t) for n, e, t in errs if not e <= t]
    assert not bad, (who, bad)


# ------------------------------------------------------------------------------ K26 against the float64 yardstick
@pytest.mark.parametrize("case", S.Q_CASES, ids=S.q_case_id)
def test_q_update_against_float64(eng, case):
    k, j = case
    fam, cfg = S.Q_CONFIGS[j]
    in_dim, A, B, n_policy = S.K26_SHAPES[k]
    steps, params = S.q_case_inputs(fam, k)
    yard = S.q_yardstick(case)
    ref = yard[0]
    dev = q_dev(eng, fam, cfg, k, params)
    out = q_updates(dev, fam, cfg, steps, n_policy).cpu().numpy()
    got = dev.snapshot()
    who = "K26 " + S.q_case_id(case)
    dev.check_fences(who)
    h64 = lambda key: got[key].double().cpu().numpy()
    clip_expert = fam == "h" and cfg.clip_expert
    state = dict(params=h64("param"), target=h64("target_param"), exp_avg=h64("m"), exp_avg_sq=h64("v"),
                 max=float(got["h_max"][0]) if clip_expert else None)
    report(who, S.q_errors(state, out, yard))
    if cfg.standardizer:
        for key, rk in (("colstats", "colstats"), ("target_colstats", "tcolstats")):
            a, r = got[key].cpu().numpy(), ref[rk]
            assert np.array_equal(a[0], r[0]), (who, key, "counts", a[0, 0], r[0, 0])
            assert np.all(np.abs(a - r) <= 1e-12 * np.maximum(1.0, np.abs(r))), (who, key)
    if fam == "h":
        assert np.all(out[:, 9:] == 0.0)
        h_max = got["h_max"].cpu().numpy()
        assert h_max[1] == 1.0 and out[-1, 8] == float(h_max[0]), (who, h_max, out[-1, 8])
    assert torch.equal(got["packed"], eng.ilmlp_pack(*split(got["param"], in_dim + A)))
    assert torch.equal(got["target_packed"], eng.ilmlp_pack(*split(got["target_param"], in_dim + A)))


# ------------------------------------------------------------------------------ K27 against the float64 yardstick
def pi_dev(eng, cfg, two, k, inp):
    in_dim, A, Bp = S.K27_SHAPES[k]
    dev = (HPiDev if two else PiDev)(eng, inp, cfg, in_dim, A, Bp)
    assert dev.t("ws").numel() == dev.nws
    return dev


@pytest.mark.parametrize("case", S.PI_CASES, ids=S.pi_case_id)
def test_pi_update_against_float64(eng, case):
    k, j = case
    cfg, two = S.PI_CONFIGS[j]
    in_dim, A, Bp = S.K27_SHAPES[k]
    inp = S.pi_case_inputs(k)
    yard = S.pi_yardstick(case)
    ref = yard[0]
    dev = pi_dev(eng, cfg, two, k, inp)
    out = np.stack([dev.update(s).cpu().numpy() for s in inp["steps"]])
    got = dev.snapshot()
    who = "K27 " + S.pi_case_id(case)
    dev.check_fences(who)
    h64 = lambda key: got[key].double().cpu().numpy()
    report(who, S.pi_errors(dict(params=h64("param"), exp_avg=h64("m")), out, (h64("action"), h64("log_prob")), yard))
    if cfg.standardizer:
        # the policy's Standardizer takes the inputs' rows: exact counts, float64 sums; the critics' take (x | a_new) with
        # the kernel's float32 a_new, held as the small sweep holds them
        a, want = got["colstats"].cpu().numpy(), ref["policy"]["colstats"]
        assert np.array_equal(a[0], want[0]) and np.all(np.abs(a - want) <= 1e-12 * np.maximum(1.0, np.abs(want))), who
        for key, want in [("critic_colstats", ref["critic"]["colstats"])] + ([("h_colstats", ref["h"]["colstats"])] if two else []):
            a = got[key].cpu().numpy()
            assert np.array_equal(a[0], want[0]), (who, key, "counts")
            assert np.all(np.abs(a - want) <= TOL * np.maximum(1.0, np.abs(want))), (who, key)
    assert torch.equal(got["packed"], eng.ilmlp_pack(*pi_split(got["param"], in_dim, 2 * A)))


@pytest.mark.parametrize("n", S.ALPHA_N)
def test_alpha_update_against_float64(eng, n):
    lps, te, lr, init = S.alpha_case(n)
    state = fenced(np.array([np.float32(np.log(init)), 0, 0], np.float32))
    inputs = []
    for step, lp in enumerate(lps):
        inputs.append(fenced(lp))
        eng.iq_alpha_update(inputs[-1].t, state.t, step, lr, te)
    torch.cuda.synchronize()
    assert_intact(dict(state=state, **{f"lp{i}": f for i, f in enumerate(inputs)}), "alpha")
    report(f"alpha n={n}", S.alpha_errors(state.t.double().cpu().numpy(), P.alpha_adam(lps, te, lr, init=init)))


# ------------------------------------------------------------------------------ bits
def same_snapshots(a, b, what):
    for key, t in a.items():
        assert same_bits(t, b[key]), (what, key)


def test_two_runs_give_the_same_bits(eng):
    """(48, 16, 1040, 520): 65 tiles, 49 steps a wave.  K26 as IQ without a target (three slots) and as LSIQ_H, K27 with two
    critics."""
    k = 2
    in_dim, A, B, n_policy = S.K26_SHAPES[k]
    assert B == 1040
    for j in (0, 6):
        fam, cfg = S.Q_CONFIGS[j]
        assert (fam == "iq" and not cfg.use_target) or (fam == "h" and not cfg.cost)
        steps, params = S.q_case_inputs(fam, k)
        snaps = []
        for _ in range(2):
            dev = q_dev(eng, fam, cfg, k, params)
            outs = q_updates(dev, fam, cfg, steps, n_policy)
            snaps.append((dev.snapshot(), outs))
        same_snapshots(snaps[0][0], snaps[1][0], S.q_cfg_id(j))
        assert torch.equal(snaps[0][1].view(torch.int64), snaps[1][1].view(torch.int64)), S.q_cfg_id(j)
    cfg, two = S.PI_CONFIGS[1]
    assert two
    inp = S.pi_case_inputs(k)
    snaps = []
    for _ in range(2):
        dev = pi_dev(eng, cfg, two, k, inp)
        outs = torch.stack([dev.update(s) for s in inp["steps"]])
        snaps.append((dev.snapshot(), outs))
    same_snapshots(snaps[0][0], snaps[1][0], "K27")
    assert torch.equal(snaps[0][1].view(torch.int64), snaps[1][1].view(torch.int64))


class Front:
    """The first n floats of a larger fenced workspace, in place of a Fenced of its own."""

    def __init__(self, whole, n):
        self.whole, self.t = whole, whole.t[:n]

    def intact(self):
        return self.whole.intact()


def test_workspace_reused_after_a_larger_batch(eng):
    """One update at 4096 rows, nothing poisoned in between, then (17, 6, 257, 1) in the front of the same buffer: the
    smaller call leaves the bits of a run in a fresh (poisoned) workspace of its own size, so it reads nothing of the
    workspace it has not written itself.  K26 as IQ without a target, K27 with two critics (both workspaces)."""
    big, small = 3, 0
    fam, cfg = S.Q_CONFIGS[0]
    steps_b, params_b = S.q_case_inputs(fam, big)
    steps_s, params_s = S.q_case_inputs(fam, small)
    n_policy = S.K26_SHAPES[small][3]
    larger = q_dev(eng, fam, cfg, big, params_b)
    larger.update(steps_b[0], S.K26_SHAPES[big][3])
    snaps = []
    for reuse in (False, True):
        dev = q_dev(eng, fam, cfg, small, params_s)
        if reuse:
            assert dev.nws < larger.nws
            dev.f["ws"] = Front(larger.f["ws"], dev.nws)
        outs = q_updates(dev, fam, cfg, steps_s, n_policy)
        snaps.append((dev.snapshot(), outs))
        dev.check_fences("K26 reuse")
    same_snapshots(snaps[0][0], snaps[1][0], "K26")
    assert torch.equal(snaps[0][1].view(torch.int64), snaps[1][1].view(torch.int64))
    assert bool(torch.isfinite(snaps[0][0]["param"]).all())
    # ---- K27
    pcfg, two = S.PI_CONFIGS[1]
    inp_b, inp_s = S.pi_case_inputs(big), S.pi_case_inputs(small)
    larger = pi_dev(eng, pcfg, two, big, inp_b)
    larger.update(inp_b["steps"][0])
    snaps = []
    for reuse in (False, True):
        dev = pi_dev(eng, pcfg, two, small, inp_s)
        if reuse:
            dev.f["ws"], dev.f["h_ws"] = Front(larger.f["ws"], dev.nws), Front(larger.f["h_ws"], dev.nws)
        outs = torch.stack([dev.update(s) for s in inp_s["steps"]])
        snaps.append((dev.snapshot(), outs))
        dev.check_fences("K27 reuse")
    same_snapshots(snaps[0][0], snaps[1][0], "K27")
    assert torch.equal(snaps[0][1].view(torch.int64), snaps[1][1].view(torch.int64))
    assert bool(torch.isfinite(snaps[0][0]["param"]).all())


@pytest.mark.parametrize("standardizer", (False, True), ids=("nostd", "std"))
def test_q_values_have_the_forward_kernels_bits(eng, standardizer):
    """tests/test_gpu_iq_q.py's test at (32, 11, 300, 150): 19 tiles, the last of 12 rows."""
    assert S.K26_SHAPES[1] == (32, 11, 300, 150)
    check_q_values_have_the_forward_kernels_bits(eng, S.K26_SHAPES[1], standardizer)


# ------------------------------------------------------------------------------ LSIQ_H's running maximum
def running_maximum(eng, k, steps, params):
    """tests/test_gpu_lsiq_h.py's test on the given steps: the [2] block after each update against lsiq_h.py:64-74
    evaluated by torch in float32 on the same log-probabilities, bit for bit."""
    fam, cfg = S.Q_CONFIGS[6]
    assert fam == "h" and cfg.clip_expert and not cfg.cost
    n_policy = S.K26_SHAPES[k][3]
    dev = q_dev(eng, fam, cfg, k, params)
    M = None
    for s in S.q_steps(fam, cfg, steps, n_policy):
        out = dev.update(s, n_policy)
        cur = torch.max(-torch.as_tensor(s["logp_next"])[:n_policy])
        if M is None:
            M = cur
        elif cur > M:
            M = (1 - cfg.tau_up) * M + cfg.tau_up * cur
        else:
            M = (1 - cfg.tau_down) * M + cfg.tau_down * cur
        assert M.dtype == torch.float32
        got = dev.t("h_max").cpu()
        assert got[0].item() == M.item() and got[1].item() == 1.0, (got, M)
        assert out[8].item() == M.item()
    dev.check_fences("running maximum")


def with_logp(steps, row, value_of):
    out = []
    for s in steps:
        lp = s["logp_next"].copy()
        lp[row] = value_of(lp)
        out.append(dict(s, logp_next=lp))
    return out


def test_the_running_maximum_of_one_policy_row_past_the_first_trip(eng):
    """(17, 6, 257, 1): the single policy row's -log pi is the batch's maximum; row 256, an expert's, is the second trip of
    the loop that strides by 256 threads."""
    k = 0
    steps, params = S.q_case_inputs("h", k)
    steps = with_logp(steps, 0, lambda lp: np.float32(lp.min() - 1.0))
    for s in steps:
        assert -s["logp_next"][0] > np.max(-s["logp_next"][1:])
    running_maximum(eng, k, steps, params)


def test_the_running_maximum_at_the_last_policy_row_in_a_later_trip(eng):
    """(48, 16, 1040, 520): the policy rows' maximum sits at row 519, in the third trip of the strided loop, where the
    r < n_policy cut falls; the batch's maximum sits at row 520, the first expert's, and must not be taken."""
    k = 2
    n_policy = S.K26_SHAPES[k][3]
    steps, params = S.q_case_inputs("h", k)
    steps = with_logp(steps, n_policy - 1, lambda lp: np.float32(lp[:n_policy].min() - 0.5))
    steps = with_logp(steps, n_policy, lambda lp: np.float32(lp.min() - 1.0))
    for s in steps:
        neg = -s["logp_next"]
        assert n_policy - 1 > 2 * S.THREADS and neg[n_policy - 1] > neg[:n_policy - 1].max()
        assert neg[n_policy] == neg.max() > neg[n_policy - 1]
    running_maximum(eng, k, steps, params)
