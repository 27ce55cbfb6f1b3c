"""K15, K16's fit and K17 on the MI355X at the shapes of tests/il_shapes.py (in_dim 1 .. 64 that is not 32, minibatches
that leave tiles partly empty, row counts one past a tile, a block or a chunk) against the float64 restatements, with
every buffer the kernels write whose size depends on the shape placed between sentinels."""
import gc

import numpy as np
import pytest
import torch

import il_shapes as sh
import trpo_restate as tr
from il_shapes import K15_CASES, K16_CASES, K17_CASES, TOL, case_id, guarded
from test_disc_fit_cpu import rel, restate_fit as disc_restate_fit
from test_il_critic_cpu import restate_fit as critic_restate_fit
from test_trpo_cpu import rel as trel

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def eng():
    from olympic_hip.engine import Engine
    e = Engine(0)
    yield e
    # release the context here (see test_gpu_il_critic.py: a context freed later by the cycle collector could land
    # inside another module's graph capture)
    torch.cuda.synchronize()
    e.ctx.close()
    gc.collect()


def disc_shapes(d):
    return [(256, d), (256,), (128, 256), (128,), (128, 128), (128,), (128, 128), (128,), (1, 128), (1,)]


def critic_shapes(d):
    return [(512, d), (512,), (256, 512), (256,), (1, 256), (1,)]


def _dev(a, dtype=None):
    t = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
    return t.to(device="cuda", dtype=dtype).contiguous()


def _flat(params):
    return np.concatenate([np.asarray(p, dtype=np.float32).reshape(-1) for p in params])


def assert_intact(bufs):
    torch.cuda.synchronize()
    assert sh.all_intact(bufs) == [], "written outside the buffer"


# ------------------------------------------------------------------------------ K15
def disc_state(eng, in_dim, batch, params):
    n_par = sum(int(np.prod(s)) for s in disc_shapes(in_dim))
    g = dict(param=guarded(n_par, F32, init=_flat(params)), exp_avg=guarded(n_par, F32), exp_avg_sq=guarded(n_par, F32),
             colstats=guarded((3, in_dim), F64), beta=guarded(1, F32, init=[0.1]))
    v = sh.views(g["param"].t, disc_shapes(in_dim))
    return dict(g=g, views=v, packed=eng.disc_pack(*v), ws=eng.disc_fit_ws(batch, in_dim), step=0, in_dim=in_dim)


def disc_run(eng, s, epochs, n_plcy, h):
    """update_mean_std(concat) then one oly_disc_fit_epoch per epoch, as test_gpu_disc_fit._run, every output between
    sentinels; returns the per-minibatch outputs."""
    g, rec = s["g"], {k: [] for k in ("loss", "bce", "kl", "beta")}
    for e, (x, perm, t, noise) in enumerate(epochs):
        xg = _dev(x, F32)
        nb = (int(xg.shape[0]) + h["batch"] - 1) // h["batch"]
        eng.col_stats(xg, g["colstats"].t)
        o = {k: guarded(nb, F32 if k == "beta" else F64) for k in rec}
        for k in o:
            g[f"{k}_out{e}_{s['step']}"] = o[k]
        eng.disc_fit_epoch(xg, n_plcy, _dev(noise, F32), _dev(perm, torch.int32), h["batch"], g["colstats"].t,
                           g["param"].t, g["exp_avg"].t, g["exp_avg_sq"].t, s["packed"], g["beta"].t, s["ws"], s["step"],
                           h["lr"], weight_decay=h["wd"], info_constraint=h["info_c"], lr_beta=h["lr_beta"],
                           targets=None if t is None else _dev(t, F32), loss_out=o["loss"].t, bce_out=o["bce"].t,
                           kl_out=o["kl"].t, beta_out=o["beta"].t)
        s["step"] += nb
        for k in rec:
            rec[k].append(o[k].t)
    torch.cuda.synchronize()
    return {k: torch.cat(v).double().cpu().numpy() for k, v in rec.items()}


def disc_check(eng, s, rec, ref, names=None):
    P, _, cs, rec64, step = ref
    assert s["step"] == step
    for i, (a, b) in enumerate(zip(s["views"], P)):
        r = rel(a.cpu().numpy(), b.cpu().numpy())
        print(f"K15 tensor {i}: {r:.2e} from float64")
        assert r <= TOL, (i, r)
    for k in ("loss", "bce", "kl", "beta"):
        np.testing.assert_allclose(rec[k], rec64[k][-len(rec[k]):], rtol=TOL, atol=TOL, err_msg=k)
    assert float(s["g"]["beta"].t) == pytest.approx(rec64["beta"][-1], abs=TOL)
    got, want = s["g"]["colstats"].t.cpu().numpy(), cs.cpu().numpy()
    assert np.array_equal(got[0], want[0]), "the count"
    np.testing.assert_allclose(got, want, rtol=1e-12)
    assert torch.equal(s["packed"], eng.disc_pack(*s["views"])), "the packed stream is the stepped parameters'"
    assert_intact(s["g"])


@pytest.mark.parametrize("c", K15_CASES, ids=case_id)
def test_disc_fit_shapes(eng, c):
    params, epochs, h = sh.disc_case(c)
    s = disc_state(eng, c.in_dim, c.batch, params)
    rec = disc_run(eng, s, epochs, c.n_plcy, h)
    disc_check(eng, s, rec, sh.disc_restate(c, device="cuda"))


# ------------------------------------------------------------------------------ K16
def critic_state(eng, in_dim, batch, params, colstats):
    n_par = sum(int(np.prod(s)) for s in critic_shapes(in_dim))
    g = dict(param=guarded(n_par, F32, init=_flat(params)), exp_avg=guarded(n_par, F32), exp_avg_sq=guarded(n_par, F32),
             colstats=guarded((3, in_dim), F64, init=colstats))
    v = sh.views(g["param"].t, critic_shapes(in_dim))
    return dict(g=g, views=v, packed=eng.ilmlp_pack(*v), ws=eng.il_critic_fit_ws(batch, in_dim), step=0)


def critic_run(eng, s, x, vt, perms, batch, lr):
    g, losses = s["g"], []
    xg, vg = _dev(x, F32), _dev(vt, F32)
    nb = (int(xg.shape[0]) + batch - 1) // batch
    for perm in perms:
        lo = g[f"loss_out_{s['step']}"] = guarded(nb, F64)
        eng.il_critic_fit_epoch(xg, vg, _dev(perm, torch.int32), batch, g["colstats"].t, g["param"].t, g["exp_avg"].t,
                                g["exp_avg_sq"].t, s["packed"], s["ws"], s["step"], lr, loss_out=lo.t)
        s["step"] += nb
        losses.append(lo.t)
    torch.cuda.synchronize()
    return torch.cat(losses).cpu().numpy()


def critic_check(eng, s, losses, ref):
    P, _, cs, losses64, step = ref
    assert s["step"] == step
    for i, (a, b) in enumerate(zip(s["views"], P)):
        r = rel(a.cpu().numpy(), b.cpu().numpy())
        print(f"K16 tensor {i}: {r:.2e} from float64")
        assert r <= TOL, (i, r)
    np.testing.assert_allclose(losses, losses64[-len(losses):], rtol=TOL)
    got, want = s["g"]["colstats"].t.cpu().numpy(), cs.cpu().numpy()
    assert np.array_equal(got[0], want[0]), "the count"
    np.testing.assert_allclose(got, want, rtol=1e-12)
    assert torch.equal(s["packed"], eng.ilmlp_pack(*s["views"])), "the packed stream is the stepped parameters'"
    assert_intact(s["g"])


@pytest.mark.parametrize("c", K16_CASES, ids=case_id)
def test_il_critic_fit_shapes(eng, c):
    params, x, vt, perms, cs = sh.critic_case(c)
    s = critic_state(eng, c.in_dim, c.batch, params, cs)
    losses = critic_run(eng, s, x, vt, perms, c.batch, c.lr)
    critic_check(eng, s, losses, sh.critic_restate(c, device="cuda"))


# ------------------------------------------------------------------------------ K17
@pytest.mark.parametrize("c", K17_CASES, ids=case_id)
def test_trpo_grad_and_fvp_shapes(eng, c):
    case = sh.trpo_case(c, device="cuda")
    n_par = tr.n_params(c.D, c.A)
    for k in (1, 4):
        J, g, prod, inp = sh.trpo_grad_fvp_reference(c, case, k)
        bufs = dict(grad_out=guarded(n_par, F32), out=guarded(n_par, F32),
                    colstats=guarded((3, c.D), F64, init=case["S"]), theta=guarded(n_par, F32, init=case["theta"]))
        g_dev, J_dev = eng.trpo_grad(case["x"], case["act"], case["adv"], bufs["colstats"].t, bufs["theta"].t,
                                     inp["logp_old"], k_stats=k, ent_coeff=sh.K17_STEP["ent_coeff"],
                                     grad_out=bufs["grad_out"].t)
        got = eng.trpo_fvp(case["x"], bufs["colstats"].t, bufs["theta"].t, inp["mu_old"], inp["log_sigma_old"], inp["p"],
                           k_stats=k, cg_damping=0.1, out=bufs["out"].t)
        torch.cuda.synchronize()
        eg, ep = trel(g_dev, g), trel(got, prod)
        print(f"K17 {case_id(c)} k={k}: g {eg:.2e}, product {ep:.2e}, J {abs(float(J_dev) - float(J)):.2e}")
        assert eg <= TOL, (k, eg)
        assert abs(float(J_dev) - float(J)) <= TOL * max(1.0, abs(float(J)))
        assert ep <= TOL, (k, ep)
        assert torch.equal(bufs["theta"].t, case["theta"]) and torch.equal(bufs["colstats"].t, case["S"])
        assert_intact(bufs)


def same_stats(a, b):
    """Equal counts; sums equal up to the summation order of the batch's column sums."""
    return torch.equal(a[0], b[0]) and torch.allclose(a, b, rtol=1e-12, atol=0)


def trpo_device_step(eng, c, case, **kw):
    n_par = tr.n_params(c.D, c.A)
    bufs = dict(theta=guarded(n_par, F32, init=case["theta"]), colstats=guarded((3, c.D), F64, init=case["S"]),
                stepdir_out=guarded(n_par, F32))
    scal = eng.trpo_step(case["x"], case["act"], case["adv"], bufs["colstats"].t, bufs["theta"].t,
                         stepdir_out=bufs["stepdir_out"].t, **kw)
    torch.cuda.synchronize()
    v = scal.cpu().tolist()
    return dict(theta=bufs["theta"].t, S=bufs["colstats"].t, stepdir=bufs["stepdir_out"].t, prev_loss=v[0], k_run=int(v[1]),
                shs=v[2], j=int(v[3]), kl=v[4], J=v[5], j_run=int(v[6]), bufs=bufs)


def trpo_step_check(out, r64, r32, theta0):
    assert out["j"] == r64["j"] and out["j_run"] == r64["j_run"] and out["k_run"] == r64["k_run"]
    assert same_stats(out["S"], r64["S"])
    th0 = theta0.double()
    for key in ("stepdir", "theta"):
        if key == "stepdir":
            e_dev, e_32 = trel(out[key], r64[key]), trel(r32[key], r64[key])
        else:
            e_dev, e_32 = trel(out[key].double() - th0, r64[key] - th0), trel(r32[key].double() - th0, r64[key] - th0)
        print(f"K17 step {key}: device {e_dev:.2e}, float32 restatement {e_32:.2e} from float64")
        assert e_dev <= 2 * e_32 + 1e-6, (key, e_dev, e_32)
    assert_intact(out["bufs"])


@pytest.mark.parametrize("c", [c for c in K17_CASES if c.n >= sh.K17_STEP_MIN_ROWS], ids=case_id)
def test_trpo_step_shapes(eng, c):
    case = sh.trpo_case(c, device="cuda")
    kw = sh.K17_STEP
    r64 = tr.trpo_step(case["theta"], case["S"], case["x"], case["act"], case["adv"], **kw)
    r32 = tr.trpo_step(case["theta"], case["S"], case["x"], case["act"], case["adv"], dtype=F32, **kw)
    trpo_step_check(trpo_device_step(eng, c, case, **kw), r64, r32, case["theta"])


# ------------------------------------------------------------------------------ a workspace that held a larger minibatch
def _f64_state(s, shapes):
    """The device state after a call as the restatement's starting point: parameters, moments, statistics."""
    cut = lambda name: [t.double().clone() for t in sh.views(s["g"][name].t, shapes)]     # noqa: E731
    return [p.cpu().numpy() for p in cut("param")], (cut("exp_avg"), cut("exp_avg_sq")), s["g"]["colstats"].t.cpu().numpy()


def test_workspace_reused_after_a_larger_minibatch(eng):
    """An epoch of full 512-row (K15) / 256-row (K16) minibatches, then on the same workspace a call whose only minibatch
    has 100 / 37 rows: the workspace's rows beyond R still hold the earlier minibatch and must not be summed."""
    in_dim, rng = 45, np.random.default_rng(77)
    big = sh.K15Case(in_dim, 512, 1024, 512, False, 0.0, 31, 1e-3)
    params, epochs, h = sh.disc_case(big, epochs=1)
    s = disc_state(eng, in_dim, 512, params)
    rec = disc_run(eng, s, epochs, big.n_plcy, h)
    disc_check(eng, s, rec, disc_restate_fit(epochs, big.n_plcy, params, np.zeros((3, in_dim)), h["info_c"], h["lr_beta"],
                                             h["lr"], 512, device="cuda"))
    p0, mom, cs0 = _f64_state(s, disc_shapes(in_dim))
    beta0, step0 = float(s["g"]["beta"].t), s["step"]
    _, small, _ = sh.disc_case(sh.K15Case(in_dim, 512, 100, 40, False, 0.0, 32, 1e-3), epochs=1)
    rec = disc_run(eng, s, small, 40, h)
    assert len(rec["loss"]) == 1
    disc_check(eng, s, rec, disc_restate_fit(small, 40, p0, cs0, h["info_c"], h["lr_beta"], h["lr"], 512, beta=beta0,
                                             step0=step0, moments=mom, device="cuda"))
    # ---- K16
    c = sh.K16Case(in_dim, 256, 512, 33, 1e-3)
    params, x, vt, perms, cs = sh.critic_case(c, epochs=1)
    s = critic_state(eng, in_dim, 256, params, cs)
    losses = critic_run(eng, s, x, vt, perms, 256, c.lr)
    critic_check(eng, s, losses, critic_restate_fit(x, vt, perms, params, cs, c.lr, 256, device="cuda"))
    p0, mom, cs0 = _f64_state(s, critic_shapes(in_dim))
    step0 = s["step"]
    _, x2, vt2, perms2, _ = sh.critic_case(sh.K16Case(in_dim, 256, 37, 34, 1e-3), epochs=1)
    x2 = (x2 + rng.standard_normal(x2.shape)).astype(np.float32)
    losses = critic_run(eng, s, x2, vt2, perms2, 256, c.lr)
    assert len(losses) == 1
    critic_check(eng, s, losses, critic_restate_fit(x2, vt2, perms2, p0, cs0, c.lr, 256, step0=step0, moments=mom,
                                                    device="cuda"))


# ------------------------------------------------------------------------------ determinism
def test_odd_shapes_deterministic(eng):
    c15, c16, c17 = K15_CASES[7], K16_CASES[5], K17_CASES[6]
    assert (c15.in_dim, c15.batch) == (64, 255) and (c16.in_dim, c16.n) == (45, 320) and c17.n == 16384 + 300
    runs = []
    for _ in range(2):
        params, epochs, h = sh.disc_case(c15)
        s = disc_state(eng, c15.in_dim, c15.batch, params)
        rec = disc_run(eng, s, epochs, c15.n_plcy, h)
        out = [s["g"][k].t for k in ("param", "exp_avg", "exp_avg_sq", "colstats", "beta")] + [s["packed"]]
        out += [torch.as_tensor(rec[k]) for k in sorted(rec)]
        params, x, vt, perms, cs = sh.critic_case(c16)
        s = critic_state(eng, c16.in_dim, c16.batch, params, cs)
        out.append(torch.as_tensor(critic_run(eng, s, x, vt, perms, c16.batch, c16.lr)))
        out += [s["g"][k].t for k in ("param", "exp_avg", "exp_avg_sq", "colstats")] + [s["packed"]]
        case = sh.trpo_case(c17, device="cuda")
        o = trpo_device_step(eng, c17, case, **sh.K17_STEP)
        out += [o["theta"], o["S"], o["stepdir"], torch.tensor([o[k] for k in ("prev_loss", "shs", "kl", "J", "j", "k_run")])]
        runs.append(out)
    assert len(runs[0]) == len(runs[1])
    for i, (a, b) in enumerate(zip(*runs)):
        assert torch.equal(a, b), i


# ------------------------------------------------------------------------------ through the classes, 45 columns
COLS = 45


def test_device_il_critic_fit_at_45_columns(eng):
    from olympic_hip.gail import DeviceStandardizer
    from olympic_hip.il_agent import DeviceILCritic
    c = sh.K16Case(COLS, 100, 250, 41, 1e-3)
    params, x, vt, _, cs = sh.critic_case(c)
    lins = [torch.nn.Linear(COLS, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 1)]
    with torch.no_grad():
        for lin, w, b in zip(lins, params[0::2], params[1::2]):
            lin.weight.copy_(torch.as_tensor(w))
            lin.bias.copy_(torch.as_tensor(b))
    stand = DeviceStandardizer(eng, COLS)
    xg = _dev(x, F32)
    stand.update_mean_std(xg)
    critic = DeviceILCritic(eng, lins, stand, lr=c.lr)
    losses = critic.fit(xg, _dev(vt, F32), n_epochs=2, batch_size=c.batch,
                        generator=torch.Generator(device="cuda").manual_seed(3))
    torch.cuda.synchronize()
    g2 = torch.Generator(device="cuda").manual_seed(3)
    perms = [torch.randperm(c.n, generator=g2, device="cuda").cpu().numpy() for _ in range(2)]
    P, _, cs64, losses64, step = critic_restate_fit(x, vt, perms, params, cs, c.lr, c.batch, device="cuda")
    assert critic.step == step == 6
    for i, (a, b) in enumerate(zip(critic._views(), P)):
        assert rel(a.cpu().numpy(), b.cpu().numpy()) <= TOL, i
    np.testing.assert_allclose(losses.reshape(-1).cpu().numpy(), losses64, rtol=TOL)
    np.testing.assert_allclose(stand.colstats.cpu().numpy(), cs64.cpu().numpy(), rtol=1e-12)
    assert torch.equal(critic.packed, eng.ilmlp_pack(*critic._views()))


def test_device_discriminator_trainer_fit_at_45_of_50_columns(eng):
    from olympic_hip.gail import DiscriminatorReward, VariationalDiscriminator, VDBLoss
    from olympic_hip.il_agent import DeviceDiscriminatorTrainer
    obs, n, rows, batch, lr = 50, 300, 700, 100, 1e-3
    mask = np.delete(np.arange(obs), [0, 7, 19, 33, 49])
    assert mask.size == COLS
    torch.manual_seed(12)
    net = VariationalDiscriminator(in_dim=COLS).cuda()
    r = DiscriminatorReward(eng, net, state_mask=mask)
    rng = np.random.default_rng(13)
    scale, shift = rng.uniform(0.3, 3.0, obs), rng.standard_normal(obs) * 2
    demo = (rng.standard_normal((rows, obs)) * scale * 0.8 + shift + 0.4 * scale).astype(np.float32)
    plcy = _dev((rng.standard_normal((n, obs)) * scale + shift).astype(np.float32))
    loss = VDBLoss(info_constraint=0.1, lr_beta=1e-3)
    trainer = DeviceDiscriminatorTrainer(r, demo, loss, lr=lr, batch_size=batch, n_epochs=2)
    params0 = [p.detach().cpu().numpy().copy() for p in r._params()]
    losses = trainer.fit(plcy, generator=torch.Generator(device="cuda").manual_seed(5))
    torch.cuda.synchronize()
    # the trainer's draws per epoch, in its order: the demonstration rows, the permutation, the noise
    g2, epochs, demo_g = torch.Generator(device="cuda").manual_seed(5), [], _dev(demo)
    for _ in range(2):
        idx = torch.randperm(rows, generator=g2, device="cuda")[:n]
        x = torch.cat([plcy[:, mask], demo_g[idx][:, mask]]).contiguous()
        perm = torch.randperm(2 * n, generator=g2, device="cuda")
        epochs.append((x, perm.cpu().numpy(), None, torch.randn((2 * n, 128), device="cuda", generator=g2)))
    P, _, cs64, rec64, step = disc_restate_fit(epochs, n, params0, np.zeros((3, COLS)), 0.1, 1e-3, lr, batch,
                                               device="cuda")
    assert trainer.step == step == 12
    for i, (a, b) in enumerate(zip(r._params(), P)):
        assert rel(a.detach().cpu().numpy(), b.cpu().numpy()) <= TOL, i
        assert rel(params0[i], b.cpu().numpy()) >= 10 * TOL, i
    np.testing.assert_allclose(losses.reshape(-1).cpu().numpy(), rec64["loss"], rtol=TOL, atol=TOL)
    assert loss._beta == pytest.approx(rec64["beta"][-1], abs=TOL)
    np.testing.assert_allclose(r.stand.colstats.cpu().numpy(), cs64.cpu().numpy(), rtol=1e-12)
    assert torch.equal(r._packed, eng.disc_pack(*[p.detach() for p in r._params()]))


def test_device_trpo_at_45_columns(eng):
    from olympic_hip.gail import DeviceStandardizer
    from olympic_hip.il_agent import DeviceGaussianPolicy, DeviceTRPO
    c = K17_CASES[6]
    assert (c.D, c.A) == (COLS, 12)
    case = sh.trpo_case(c, device="cuda")
    W = tr.split(case["theta"], c.D, c.A)
    lins = [torch.nn.Linear(c.D, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, c.A)]
    with torch.no_grad():
        for i, lin in enumerate(lins):
            lin.weight.copy_(W[2 * i].cpu())
            lin.bias.copy_(W[2 * i + 1].cpu())
    stand = DeviceStandardizer(eng, c.D)
    stand.colstats, stand._fresh = case["S"].clone(), False
    pol = DeviceGaussianPolicy(eng, lins, stand, log_sigma=W[6].cpu())
    assert torch.equal(pol.theta, case["theta"])
    trpo = DeviceTRPO(pol, **sh.K17_STEP)
    trpo(case["x"], case["act"], case["adv"])
    torch.cuda.synchronize()
    kw = sh.K17_STEP
    r64 = tr.trpo_step(case["theta"], case["S"], case["x"], case["act"], case["adv"], **kw)
    r32 = tr.trpo_step(case["theta"], case["S"], case["x"], case["act"], case["adv"], dtype=F32, **kw)
    v = trpo.scalars()
    assert (int(v["accepted_j"]), int(v["ls_iters"]), int(v["cg_iters"])) == (r64["j"], r64["j_run"], r64["k_run"])
    assert same_stats(stand.colstats, r64["S"])
    th0 = case["theta"].double()
    e_dev, e_32 = trel(pol.theta.double() - th0, r64["theta"] - th0), trel(r32["theta"].double() - th0, r64["theta"] - th0)
    assert e_dev <= 2 * e_32 + 1e-6, (e_dev, e_32)
    assert torch.equal(pol.packed, eng.ilmlp_pack(*pol._views()[:6]))
