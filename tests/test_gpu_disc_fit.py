"""K15 on the MI355X: oly_disc_fit_epoch against the reference-pinned fixture and against torch at size, the
cross-check with K12's forward, determinism, DeviceDiscriminatorTrainer's hand-over to DiscriminatorReward, and
VAILAgent.fit with the device trainer against the same sequence strung by hand."""
import copy
import gc

import numpy as np
import pytest
import torch

from test_disc_fit_cpu import FIXTURE, case_inputs, check_statistics, gen, hyper, rel, restate_fit

pytestmark = pytest.mark.gpu


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


def _state(eng, params, batch):
    flat = torch.cat([torch.as_tensor(np.asarray(p)).reshape(-1) for p in params]).float().cuda().contiguous()
    views, o = [], 0
    for p in params:
        views.append(flat[o:o + p.size].view(p.shape))
        o += p.size
    in_dim = int(params[0].shape[1])
    return dict(param=flat, views=views, m=torch.zeros_like(flat), v=torch.zeros_like(flat),
                packed=eng.disc_pack(*views), beta=torch.full((1,), 0.1, device="cuda"),
                cs=torch.zeros((3, in_dim), dtype=torch.float64, device="cuda"), ws=eng.disc_fit_ws(batch, in_dim),
                step=0)


def _dev(a, dtype=None):
    t = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
    return t.to(device="cuda", dtype=dtype).contiguous()


def _run(eng, s, epochs, n_plcy, h):
    """The explicit update_mean_std(concat) then one oly_disc_fit_epoch per epoch; returns the per-minibatch outputs."""
    rec = {k: [] for k in ("loss", "bce", "kl", "beta")}
    for x, perm, t, noise in epochs:
        xg = _dev(x)
        n, nb = int(xg.shape[0]), (int(xg.shape[0]) + h["batch"] - 1) // h["batch"]
        eng.col_stats(xg, s["cs"])
        o = dict(bce_out=torch.empty(nb, dtype=torch.float64, device="cuda"),
                 kl_out=torch.empty(nb, dtype=torch.float64, device="cuda"),
                 beta_out=torch.empty(nb, dtype=torch.float32, device="cuda"))
        loss = eng.disc_fit_epoch(xg, n_plcy, _dev(noise), _dev(perm, torch.int32), h["batch"], s["cs"],
                                  s["param"], s["m"], s["v"], s["packed"], s["beta"], s["ws"], s["step"], h["lr"],
                                  weight_decay=h["wd"], info_constraint=h["info_c"], lr_beta=h["lr_beta"],
                                  targets=None if t is None else _dev(t),
                                  **o)
        s["step"] += nb
        for k, v in (("loss", loss), ("bce", o["bce_out"]), ("kl", o["kl_out"]), ("beta", o["beta_out"])):
            rec[k].append(v)
    torch.cuda.synchronize()
    return {k: torch.cat(v).double().cpu().numpy() for k, v in rec.items()}


@pytest.mark.parametrize("case", ["a", "b"])
def test_fit_epoch_against_the_reference_fixture(eng, case):
    g = np.load(FIXTURE)
    h = hyper(g, case)
    s = _state(eng, gen.init_params(), h["batch"])
    rec = _run(eng, s, case_inputs(g, case), 640, h)
    for name, v in zip(gen.NAMES, s["views"]):
        assert rel(v.cpu().numpy(), g[f"{case}_final_{name}"]) <= 2e-5, name
    for k in ("loss", "bce", "kl", "beta"):
        np.testing.assert_allclose(rec[k], g[f"{case}_{k}"], rtol=2e-5, atol=2e-5, err_msg=k)
    assert float(s["beta"]) == pytest.approx(g[f"{case}_beta"][-1], abs=2e-5)
    check_statistics(s["cs"].cpu().numpy(), g, case)
    # the packed stream is the one oly_disc_pack makes from the stepped parameters
    assert torch.equal(s["packed"], eng.disc_pack(*s["views"]))


def test_fit_is_deterministic(eng):
    g = np.load(FIXTURE)
    h = hyper(g, "b")
    runs = []
    for _ in range(2):
        s = _state(eng, gen.init_params(), h["batch"])
        rec = _run(eng, s, case_inputs(g, "b"), 640, h)
        runs.append((s, rec))
    (s0, r0), (s1, r1) = runs
    for k in ("param", "m", "v", "packed", "beta", "cs"):
        assert torch.equal(s0[k], s1[k]), k
    for k in r0:
        assert np.array_equal(r0[k], r1[k]), k


def test_fit_at_size_against_torch(eng):
    """65 536 policy rows + as many demonstration rows, minibatches of 2048: one epoch of 64 Adam steps against the
    float64 restatement on the GPU."""
    n, in_dim, batch = 65536, 32, 2048
    gg = torch.Generator(device="cuda").manual_seed(4)
    shift = torch.randn(in_dim, device="cuda", generator=gg)
    plcy = torch.randn((n, in_dim), device="cuda", generator=gg) * 1.5 + shift
    demo = torch.randn((n, in_dim), device="cuda", generator=gg) * 1.2 + shift + 0.4
    x = torch.cat([plcy, demo]).contiguous()
    perm = torch.randperm(2 * n, device="cuda", generator=gg)
    noise = torch.randn((2 * n, 128), device="cuda", generator=gg)
    params = gen.init_params(seed=3)
    h = dict(info_c=0.1, lr_beta=1e-3, wd=0.0, lr=5e-5, batch=batch)
    s = _state(eng, params, batch)
    rec = _run(eng, s, [(x, perm.cpu().numpy(), None, noise)], n, h)
    epochs = [(x, perm.cpu().numpy(), None, noise)]
    P, _, cs_ref, rec64, _ = restate_fit(epochs, n, params, np.zeros((3, in_dim)), 0.1, 1e-3, 5e-5, batch,
                                         device="cuda")
    P32, _, _, rec32, _ = restate_fit(epochs, n, params, np.zeros((3, in_dim)), 0.1, 1e-3, 5e-5, batch,
                                      dtype=torch.float32, device="cuda")
    for name, a, b, c in zip(gen.NAMES, s["views"], P, P32):
        r, r32 = rel(a.cpu().numpy(), b.cpu().numpy()), rel(c.cpu().numpy(), b.cpu().numpy())
        print(f"{name}: rel to float64 {r:.3e}, torch float32 {r32:.3e}")
        assert r <= max(3 * r32, 1e-4), (name, r, r32)
    for k in ("loss", "bce", "kl", "beta"):
        np.testing.assert_allclose(rec[k], rec64[k], rtol=1e-4, atol=1e-5, err_msg=k)
    np.testing.assert_allclose(s["cs"].cpu().numpy(), cs_ref.cpu().numpy(), rtol=1e-12)


def test_first_minibatch_loss_matches_k12(eng):
    """loss_out[0] against the loss recomputed in f64 from oly_disc_forward's logits, mu and logvar for the same rows,
    statistics (those that include the minibatch) and noise."""
    g = np.load(FIXTURE)
    h = hyper(g, "a")
    x, perm, _, noise = case_inputs(g, "a")[0]
    s = _state(eng, gen.init_params(), h["batch"])
    packed0 = s["packed"].clone()
    rec = _run(eng, s, [(x, perm, None, noise)], 640, h)
    R = h["batch"]
    xb = torch.as_tensor(x[perm[:R]]).cuda().contiguous()
    cs = torch.as_tensor(x).cuda().double()
    cs = torch.stack([torch.full((32,), 1280.0 + R, device="cuda", dtype=torch.float64),
                      cs.sum(0) + xb.double().sum(0), (cs * cs).sum(0) + (xb.double() ** 2).sum(0)]).contiguous()
    o = eng.disc_forward(xb, packed0, colstats=cs, eps=torch.as_tensor(noise[:R]).cuda().contiguous(),
                         want=("logits", "mu", "logvar"))
    d, mu, lv = (o[k].double() for k in ("logits", "mu", "logvar"))
    t = (torch.as_tensor(perm[:R]).cuda() >= 640).double()
    bce = torch.nn.functional.binary_cross_entropy_with_logits(d, t)
    kl = (0.5 * (mu * mu + torch.exp(lv) - lv - 1).sum(1)).mean()
    loss = float(bce + 0.1 * (kl - 0.1))
    assert abs(loss - rec["loss"][0]) <= 1e-5, (loss, rec["loss"][0])


# ------------------------------------------------------------------------------ DeviceDiscriminatorTrainer
def _trainer(eng, seed, **kw):
    from olympic_hip.gail import DiscriminatorReward, VariationalDiscriminator, VDBLoss
    from olympic_hip.il_agent import DeviceDiscriminatorTrainer
    torch.manual_seed(seed)
    net = VariationalDiscriminator(in_dim=32).cuda()
    r = DiscriminatorReward(eng, net, state_mask=np.arange(2, 34))
    demo = np.random.default_rng(seed).normal(0.2, 1.0, (3000, 36)).astype(np.float32)
    args = dict(batch_size=1024)
    args.update(kw)
    return r, DeviceDiscriminatorTrainer(r, demo, VDBLoss(info_constraint=0.1, lr_beta=1e-3), **args)


def test_reward_paths_use_the_fitted_weights(eng):
    from olympic_hip.gail import DeviceStandardizer, DiscriminatorReward
    r, tr = _trainer(eng, 1)
    plcy = torch.randn((1500, 36), device="cuda")
    before = [p.detach().clone() for p in r._params()]
    ptrs = [p.data_ptr() for p in r._params()]
    losses = tr.fit(plcy, generator=torch.Generator(device="cuda").manual_seed(0))
    torch.cuda.synchronize()
    assert losses.shape == (1, 3) and torch.isfinite(losses).all()
    assert [p.data_ptr() for p in r._params()] == ptrs
    assert all(not torch.equal(a, b.detach()) for a, b in zip(before, r._params()))
    assert torch.equal(r._packed, eng.disc_pack(*[p.detach() for p in r._params()]))
    assert tr.loss._beta != 0.1
    x = torch.randn((3000, 36), device="cuda")
    eps = torch.randn((3000, 128), device="cuda")
    cs0 = r.stand.colstats.clone()

    def path(run):
        r.stand.colstats.copy_(cs0)
        return run().clone()
    step = r.prepared(x, eps)
    out = [path(lambda: r.forward(x, eps)["reward"]), path(lambda: step()["reward"])]
    r.cache_packed = True
    out.append(path(lambda: r.forward(x, eps)["reward"]))
    r.cache_packed = False
    st = DeviceStandardizer(eng, 32)
    st.colstats, st._fresh = cs0.clone(), False
    fresh = DiscriminatorReward(eng, copy.deepcopy(r.net), state_mask=np.arange(2, 34), standardizer=st)
    out.append(fresh.forward(x, eps)["reward"])
    torch.cuda.synchronize()
    for o in out[1:]:
        assert torch.equal(o, out[0])


def test_a_write_through_data_between_fits_is_used(eng):
    r, tr = _trainer(eng, 2)
    plcy = torch.randn((1000, 36), device="cuda")
    tr.fit(plcy, generator=torch.Generator(device="cuda").manual_seed(0))
    r.net.decoder.bias.data.fill_(5.0)
    r.net.mu_out.weight.data.zero_()
    tr.fit(plcy, generator=torch.Generator(device="cuda").manual_seed(1))
    torch.cuda.synchronize()
    assert abs(float(r.net.decoder.bias.detach()) - 5.0) < 1e-3
    assert float(r.net.mu_out.weight.abs().max()) < 1e-3


def test_vail_agent_fit_with_the_device_trainer_equals_the_sequence_by_hand(eng):
    from olympic_hip.gail import DeviceStandardizer
    from olympic_hip.il_agent import DeviceILCritic, VAILAgent
    T, N = 20, 100

    def parts(seed):
        r, tr = _trainer(eng, seed, batch_size=512)
        torch.manual_seed(seed + 1)
        lins = [torch.nn.Linear(36, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 1)]
        return r, tr, DeviceILCritic(eng, lins, DeviceStandardizer(eng, 36))
    ra, ta, ca = parts(7)
    rb, tb, cb = parts(7)
    agent = VAILAgent(eng, ra, ta, ca, lambda o, a, adv, ag: None, train_D_n_th_epoch=2)
    for call in range(2):
        g = torch.Generator(device="cuda").manual_seed(call)
        s = torch.randn((T + 1, N, 36), device="cuda", generator=g)
        last = torch.zeros((T, N), dtype=torch.bool, device="cuda")
        last[-1] = True
        ds = dict(state=s[:-1].contiguous(), action=torch.randn((T, N, 11), device="cuda", generator=g),
                  reward=torch.randn((T, N), device="cuda", generator=g), next_state=s[1:].contiguous(),
                  absorbing=torch.zeros((T, N), dtype=torch.bool, device="cuda"), last=last)
        eps = torch.randn((T * N, 128), device="cuda", generator=g)
        out = agent.fit(ds, eps=eps, generator=torch.Generator(device="cuda").manual_seed(10 + call))
        # ---- by hand: the agent's steps with the trainer called directly (gail_TRPO.py:105-165)
        gb = torch.Generator(device="cuda").manual_seed(10 + call)
        flat = ds["state"].reshape(T * N, 36)
        cb.stand.update_mean_std(flat)
        rb(flat, eps)
        cb(flat)
        cb(ds["next_state"].reshape(T * N, 36).contiguous())
        for _ in range(3):
            cb.stand.update_mean_std(flat)
        cb.fit(flat, out["v_target"].reshape(-1), n_epochs=3, batch_size=256, generator=gb)
        disc_loss = tb.fit(flat, generator=gb) if call == 1 else None
        torch.cuda.synchronize()
        assert out["disc_trained"] == (call == 1)
        if call == 1:
            assert torch.equal(out["disc_loss"], disc_loss)
        for pa, pb in zip(ra._params(), rb._params()):
            assert torch.equal(pa, pb)
        assert torch.equal(ra.stand.colstats, rb.stand.colstats) and ta.loss._beta == tb.loss._beta
        assert torch.equal(ca.param, cb.param)


def test_refusals(eng):
    from olympic_hip._ffi import OlyError
    from olympic_hip.gail import DiscriminatorReward, VariationalDiscriminator, VDBLoss
    from olympic_hip.il_agent import DeviceDiscriminatorTrainer
    r, tr = _trainer(eng, 3)
    before = [p.detach().clone() for p in r._params()]
    with pytest.raises(OlyError):
        DeviceDiscriminatorTrainer(r, np.zeros((10, 36)), VDBLoss(0.1, 1e-3, use_bernoulli_ent=True))
    with pytest.raises(OlyError):
        DeviceDiscriminatorTrainer(r, np.zeros((10, 36)), lambda *a: 0.0)          # the GAIL loss
    with pytest.raises(OlyError):
        wide = DiscriminatorReward(eng, VariationalDiscriminator(in_dim=32, enc_features=(128,)).cuda())
        DeviceDiscriminatorTrainer(wide, np.zeros((10, 32)), VDBLoss(0.1, 1e-3))

    class GailNet(torch.nn.Module):        # a non-variational discriminator of the same widths
        def __init__(self):
            super().__init__()
            self.encoder = torch.nn.ModuleList([torch.nn.Linear(32, 256), torch.nn.Linear(256, 128)])
            self.mu_out = torch.nn.Linear(128, 128)
            self.decoder = torch.nn.Linear(128, 1)
    with pytest.raises(OlyError):
        DeviceDiscriminatorTrainer(DiscriminatorReward(eng, GailNet().cuda()), np.zeros((10, 32)), VDBLoss(0.1, 1e-3))
    for bad in (4097, 0):
        with pytest.raises(OlyError):
            DeviceDiscriminatorTrainer(r, np.zeros((10, 36)), VDBLoss(0.1, 1e-3), batch_size=bad)
    with pytest.raises(OlyError):
        tr.fit(torch.zeros((0, 36), device="cuda"))
    with pytest.raises(OlyError):
        tr.fit(torch.zeros((10, 30), device="cuda"))
    # the engine: bad shapes never reach a launch
    s = _state(eng, gen.init_params(), 512)
    x = torch.randn((100, 32), device="cuda")
    perm = torch.randperm(100, device="cuda").to(torch.int32)
    noise = torch.randn((100, 128), device="cuda")
    for bad in (dict(batch=4097), dict(batch=0), dict(perm=perm[:10]), dict(n_plcy=101), dict(noise=noise[:50]),
                dict(x=torch.randn((100, 65), device="cuda"))):
        a = dict(x=x, batch=512, perm=perm, n_plcy=50, noise=noise)
        a.update(bad)
        with pytest.raises(OlyError):
            eng.disc_fit_epoch(a["x"], a["n_plcy"], a["noise"], a["perm"], a["batch"], s["cs"], s["param"], s["m"],
                               s["v"], s["packed"], s["beta"], s["ws"], 0, 5e-5)
    torch.cuda.synchronize()
    assert bool((s["cs"] == 0).all()) and float(s["beta"]) == pytest.approx(0.1)
    assert all(torch.equal(a, b.detach()) for a, b in zip(before, r._params()))
