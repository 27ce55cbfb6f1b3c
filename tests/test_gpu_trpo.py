"""K17 on the MI355X: the gradient and the Fisher-vector product against float64 autograd, the whole TRPO step against
the reference-pinned fixture and against the float64 restatement (line-search branches under both acceptance rules,
CG's early stop, size), determinism, refusals, DeviceGaussianPolicy.draw_action, and VAILAgent.fit with DeviceTRPO."""
import gc

import numpy as np
import pytest
import torch

import trpo_restate as tr
from test_gpu_il_critic import _agent_parts, _dataset, _Trainer, make_net
from test_trpo_cpu import A, D, fixture_case, make_case, project, rel

pytestmark = pytest.mark.gpu
FIXTURE = "trpo_step/trpo_step.npz"


@pytest.fixture(scope="module")
def eng():
    from olympic_hip.engine import Engine
    e = Engine(0)
    yield e
    torch.cuda.synchronize()
    e.ctx.close()
    gc.collect()


def cuda_case(**kw):
    return make_case(device="cuda", **kw)


def old_dist(case, dtype=torch.float64):
    """mu_old (S + c) and old_log_prob (S + 2c) of the case's policy, float64."""
    th = case["theta"].double()
    c = tr.batch_stats(case["x"])
    mu_old = tr.forward(th, tr.standardise(case["x"], case["S"], c, 1, torch.float64), A)[2]
    mu2 = tr.forward(th, tr.standardise(case["x"], case["S"], c, 2, torch.float64), A)[2]
    ls = tr.split(th, D, A)[6]
    return c, mu_old, ls, tr.log_prob(mu2, case["act"].double(), ls)


@pytest.mark.parametrize("n", [1000, 16384])
def test_grad_and_fvp_against_float64_autograd(eng, n):
    case = cuda_case(n=n, seed=7, prior=3000)
    c, mu_old, ls_old, logp_old = old_dist(case)
    th = case["theta"].double()
    for k in (1, 4):
        xh = tr.standardise(case["x"], case["S"], c, k, torch.float64)
        lp = logp_old.float()
        J, g = tr.grad(th, xh, case["act"].double(), case["adv"].double(), lp.double(), 1e-3)
        g_dev, J_dev = eng.trpo_grad(case["x"], case["act"], case["adv"], case["S"].clone(), case["theta"], lp,
                                     k_stats=k, ent_coeff=1e-3)
        assert rel(g_dev, g) <= 2e-5, k
        assert abs(float(J_dev) - float(J)) <= 2e-5 * max(1.0, abs(float(J)))
        p = torch.randn(th.shape, device="cuda", dtype=torch.float64, generator=torch.Generator(device="cuda").manual_seed(k))
        ref = tr.fvp_autograd(th, xh, mu_old.float().double(), ls_old, p.float().double(), 0.1)
        got = eng.trpo_fvp(case["x"], case["S"].clone(), case["theta"], mu_old.float().contiguous(),
                           ls_old.float().contiguous(), p.float().contiguous(), k_stats=k, cg_damping=0.1)
        assert rel(got, ref) <= 2e-5, k


def same_stats(a, b):
    """Equal counts; sums equal up to the summation order of the batch's column sums."""
    return torch.equal(a[0], b[0]) and torch.allclose(a, b, rtol=1e-12, atol=0)


def device_step(eng, case, **kw):
    theta, S = case["theta"].clone(), case["S"].clone()
    sd = torch.empty_like(theta)
    scal = eng.trpo_step(case["x"], case["act"], case["adv"], S, theta, stepdir_out=sd, **kw)
    torch.cuda.synchronize()
    v = scal.cpu().tolist()
    return dict(theta=theta, S=S, stepdir=sd, prev_loss=v[0], k_run=int(v[1]), shs=v[2], j=int(v[3]), kl=v[4], J=v[5],
                j_run=int(v[6]))


@pytest.mark.parametrize("name", ["a", "b"])
def test_step_against_fixture(eng, golden, name):
    f = golden(FIXTURE)
    case = {k: v.cuda() for k, v in fixture_case(f, name).items()}
    out = device_step(eng, case, max_kl=float(f["max_kl"]), ent_coeff=float(f["ent_coeff"]),
                      n_epochs_cg=int(f["n_epochs_cg"]))
    assert out["j"] == int(f[f"{name}_j"]) and out["k_run"] == int(f[f"{name}_k_run"])
    assert out["j_run"] == int(f[f"{name}_j_run"])
    assert np.array_equal(out["S"][0].cpu().numpy(), f[f"{name}_S_final"][0]), "the final count"
    assert np.allclose(out["S"].cpu().numpy(), f[f"{name}_S_final"], rtol=1e-6, atol=1e-6)
    tol = float(f[f"{name}_tol"])
    for key in ("prev_loss", "shs", "kl", "J"):
        assert abs(out[key] - float(f[f"{name}_{key}"])) <= tol * max(1.0, abs(float(f[f"{name}_{key}"]))), key
    for key in ("stepdir", "theta"):
        flat, proj = project(f, out[key])
        assert rel(flat, torch.from_numpy(f[f"{name}_{key}_flat"]).double()) <= tol, key
        assert rel(proj, torch.from_numpy(f[f"{name}_{key}_w2proj"]).double()) <= tol, key


@pytest.mark.parametrize("n", [65536, 409600])
def test_step_at_size_no_farther_than_torch_float32(eng, n):
    case = cuda_case(n=n, seed=9, prior=100000)
    kw = dict(max_kl=5e-3, ent_coeff=1e-3, n_epochs_cg=10)
    r64 = tr.trpo_step(case["theta"], case["S"], case["x"], case["act"], case["adv"], **kw)
    r32 = tr.trpo_step(case["theta"], case["S"], case["x"], case["act"], case["adv"], dtype=torch.float32, **kw)
    out = device_step(eng, case, **kw)
    assert out["j"] == r64["j"] == r32["j"] and out["k_run"] == r64["k_run"]
    assert same_stats(out["S"], r64["S"])
    for key in ("stepdir", "theta"):
        e_dev = rel(out[key], r64[key]) if key == "stepdir" else rel(out[key].double() - case["theta"].double(),
                                                                        r64[key] - case["theta"].double())
        e_32 = rel(r32[key], r64[key]) if key == "stepdir" else rel(r32[key].double() - case["theta"].double(),
                                                                       r64[key] - case["theta"].double())
        assert e_dev <= 2 * e_32 + 1e-6, (key, e_dev, e_32)


BRANCHES = [   # (rule, seed, prior rows, max_kl, expected: 0 / "later" / -1), chosen with the float64 restatement
    ("or", 0, 0, 5e-3, 0), ("and", 0, 0, 5e-3, 0),
    ("or", 0, 0, 1e3, "later"), ("and", 1, 5000, 5e-3, "later"),
    ("or", 1, 5000, 1e-8, -1), ("and", 0, 0, 1e-5, -1),
]


@pytest.mark.parametrize("rule,seed,prior,max_kl,expect", BRANCHES)
def test_line_search_branches(eng, rule, seed, prior, max_kl, expect):
    case = cuda_case(n=1000, seed=seed, prior=prior)
    kw = dict(max_kl=max_kl, ent_coeff=1e-3, n_epochs_cg=10, accept_rule=rule)
    r64 = tr.trpo_step(case["theta"], case["S"], case["x"], case["act"], case["adv"], **kw)
    assert (r64["j"] > 0) if expect == "later" else (r64["j"] == expect)
    out = device_step(eng, case, **kw)
    assert out["j"] == r64["j"] and out["j_run"] == r64["j_run"] and out["k_run"] == r64["k_run"]
    assert same_stats(out["S"], r64["S"])
    if out["j"] < 0:
        assert torch.equal(out["theta"], case["theta"]), "theta_0 restored"
        assert out["j_run"] == 10
    else:
        kl_ok, up = out["kl"] <= 1.5 * max_kl, out["J"] - out["prev_loss"] >= 0
        assert (kl_ok and up) if rule == "and" else (kl_ok or up)
        assert rel(out["theta"].double() - case["theta"].double(), r64["theta"] - case["theta"].double()) <= 1e-3


def test_cg_early_stop(eng):
    case = cuda_case(n=1000, seed=3)
    kw = dict(max_kl=5e-3, ent_coeff=1e-3, n_epochs_cg=25, cg_residual_tol=1e30)
    out = device_step(eng, case, **kw)
    r64 = tr.trpo_step(case["theta"], case["S"], case["x"], case["act"], case["adv"], **kw)
    assert out["k_run"] == r64["k_run"] == 1
    assert same_stats(out["S"], r64["S"])
    assert float(out["S"][0, 0] - case["S"][0, 0]) == (3 + 2 * out["j_run"]) * 1000


def test_two_runs_bit_identical(eng):
    case = cuda_case(n=20000, seed=5, prior=1000)    # two chunks
    kw = dict(max_kl=5e-3, ent_coeff=1e-3, n_epochs_cg=25)
    a, b = device_step(eng, case, **kw), device_step(eng, case, **kw)
    for k in ("theta", "S", "stepdir"):
        assert torch.equal(a[k], b[k]), k
    assert [a[k] for k in ("prev_loss", "shs", "kl", "J", "j", "k_run")] == [b[k] for k in ("prev_loss", "shs", "kl", "J",
                                                                                             "j", "k_run")]


def test_refusals_before_launch(eng):
    from olympic_hip._ffi import OlyError
    from olympic_hip.gail import DeviceStandardizer
    from olympic_hip.il_agent import DeviceGaussianPolicy
    case = cuda_case(n=64, seed=1)
    x, act, adv, S, th = case["x"], case["act"], case["adv"], case["S"], case["theta"]
    with pytest.raises(OlyError, match="identity"):
        eng.trpo_step(x, act, adv, S, th, last_act="tanh")
    with pytest.raises(OlyError, match="unsupported"):
        eng.trpo_step(torch.zeros((64, 65), device="cuda"), act, adv, torch.zeros((3, 65), dtype=torch.float64,
                                                                                  device="cuda"), th)
    with pytest.raises(OlyError, match="unsupported"):
        eng.trpo_step(x, torch.zeros((64, 33), device="cuda"), adv, S, th)
    with pytest.raises(OlyError, match="unsupported"):
        eng.trpo_step(x, act, adv, S, th, hidden=(256, 256))
    with pytest.raises(OlyError, match="no rows"):
        eng.trpo_step(x[:0], act[:0], adv[:0], S, th)
    with pytest.raises(OlyError):
        DeviceGaussianPolicy(eng, [torch.nn.Linear(32, 512), torch.nn.Linear(512, 128), torch.nn.Linear(128, 11)],
                             DeviceStandardizer(eng, 32))
    # the C entry refuses on its own, whatever the binding checked
    from olympic_hip import _abi
    a, _ = eng.trpo_args(x, act, adv, S, th)
    a.last_act = _abi.ACT_TANH
    with pytest.raises(OlyError, match="identity last activation"):
        eng.ctx.call("oly_trpo_step", __import__("ctypes").byref(a), eng._s())
    a.last_act, a.n = _abi.ACT_IDENTITY, 0
    with pytest.raises(OlyError, match="n > 0"):
        eng.ctx.call("oly_trpo_step", __import__("ctypes").byref(a), eng._s())


def test_draw_action_against_float64(eng):
    from olympic_hip.gail import DeviceStandardizer
    from olympic_hip.il_agent import DeviceGaussianPolicy
    lins = make_net(D, A, 3)
    stand = DeviceStandardizer(eng, D)
    pol = DeviceGaussianPolicy(eng, lins, stand, std_0=0.5)
    x = torch.randn((777, D), device="cuda") * 2 + 1
    a = pol.draw_action(x, generator=torch.Generator(device="cuda").manual_seed(4))
    eps = torch.randn((777, A), device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
    S = tr.batch_stats(x)
    th = pol.theta.double()
    mu = tr.forward(th, tr.standardise(x, torch.zeros_like(S), S, 1, torch.float64), A)[2]
    ref = mu + 0.5 * eps.double()
    assert float((a.double() - ref).abs().max()) <= 1e-5
    assert same_stats(stand.colstats, S)
    assert abs(float(pol.entropy()) - float(tr.entropy(th[-A:]))) <= 1e-5


def test_vail_agent_fit_with_device_trpo_equals_the_sequence_by_hand(eng):
    from olympic_hip import _abi
    from olympic_hip.il_agent import DeviceGaussianPolicy, DeviceTRPO, VAILAgent
    from olympic_hip.rollout import GAERollout, RolloutBuffer
    T, N = 20, 100
    disc_a, critic_a, stand_a = _agent_parts(eng, 5)
    disc_b, critic_b, stand_b = _agent_parts(eng, 5)
    pol_a = DeviceGaussianPolicy(eng, make_net(32, 11, 8), stand_a, std_0=0.5)
    pol_b = DeviceGaussianPolicy(eng, make_net(32, 11, 8), stand_b, std_0=0.5)
    conf = dict(max_kl=5e-3, ent_coeff=1e-3, n_epochs_cg=25)
    trpo = DeviceTRPO(pol_a, **conf)
    agent = VAILAgent(eng, disc_a, _Trainer(), critic_a, trpo, env_reward_frac=0.25, train_D_n_th_epoch=3)
    post = GAERollout(eng, gamma=0.99, lam=0.97)
    for call in range(2):
        ds = _dataset(T, N, 60 + call)
        eps = torch.randn((T * N, 128), device="cuda", generator=torch.Generator(device="cuda").manual_seed(call))
        agent.fit(ds, eps=eps, generator=torch.Generator(device="cuda").manual_seed(100 + call))
        # ---- by hand: gail_TRPO.py:105-165
        gb = torch.Generator(device="cuda").manual_seed(100 + call)
        x, xn = ds["state"], ds["next_state"]
        flat = x.reshape(T * N, 32)
        stand_b.update_mean_std(flat)
        r = ds["reward"] * 0.25 + disc_b(flat, eps).reshape(T, N) * 0.75
        buf = RolloutBuffer(T, N, 32, 1, x.device)
        buf.rewards.copy_(r)
        buf.values.copy_(critic_b(flat).reshape(T, N))
        buf.next_values.copy_(critic_b(xn.reshape(T * N, 32).contiguous()).reshape(T, N))
        buf.flags.copy_((ds["last"].to(torch.uint8) * _abi.FLAG_LAST) |
                        (ds["absorbing"].to(torch.uint8) * _abi.FLAG_ABSORBING))
        buf.ptr = T
        v_target, adv = post.finish(buf, normalize=True)
        scal = eng.trpo_step(flat.contiguous(), ds["action"].reshape(T * N, 11).contiguous(), adv.reshape(-1).contiguous(),
                             stand_b.colstats, pol_b.theta, packed=pol_b.packed, **conf)
        for _ in range(3):
            stand_b.update_mean_std(flat)
        critic_b.fit(flat, v_target.reshape(-1), n_epochs=3, batch_size=256, generator=gb)
        torch.cuda.synchronize()
        assert torch.equal(trpo.last, scal)
        assert torch.equal(pol_a.theta, pol_b.theta) and torch.equal(pol_a.packed, pol_b.packed)
        assert torch.equal(pol_a.log_sigma, pol_b.log_sigma)
        assert torch.equal(stand_a.colstats, stand_b.colstats)
        assert torch.equal(critic_a.param, critic_b.param)
    assert not torch.equal(pol_a.theta, DeviceGaussianPolicy(eng, make_net(32, 11, 8), stand_b,
                                                                           std_0=0.5).theta), "the policy moved"
    net, log_sigma = pol_a.sync_to_torch()
    assert torch.equal(net[2].bias.detach().cuda(), pol_a.theta[-22:-11]) and torch.equal(log_sigma.cuda(), pol_a.log_sigma)
