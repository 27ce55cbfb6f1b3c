"""K18 on the MI355X: oly_gail_disc_fit_epoch against the reference-pinned fixtures, against torch at size and across the
accepted shapes; the reward forward (oly_gail_disc_forward / oly_gail_reward_step); DeviceGAILDiscriminatorTrainer's
hand-over to GAILDiscriminatorReward; GAILAgent.fit against the same sequence strung by hand."""
import gc

import numpy as np
import pytest
import torch

import il_shapes as sh
from il_shapes import K15_CASES, TOL, case_id, guarded
from test_gail_disc_cpu import (case_inputs, check_statistics, fixture, forward, gail_loss, gen, hyper, rel, restate_fit)

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


def shapes(d):
    return [(512, d), (512,), (256, 512), (256,), (1, 256), (1,)]


def _dev(a, dtype=None):
    t = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
    return t.to(device="cuda", dtype=dtype).contiguous()


def _state(eng, params, batch):
    """The fit's buffers, those whose size depends on the shape between sentinels."""
    in_dim = int(np.asarray(params[0]).shape[1])
    flat = np.concatenate([np.asarray(p, dtype=np.float32).reshape(-1) for p in params])
    g = dict(param=guarded(flat.size, F32, init=flat), m=guarded(flat.size, F32), v=guarded(flat.size, F32),
             cs=guarded((3, in_dim), F64))
    views = sh.views(g["param"].t, shapes(in_dim))
    return dict(g=g, param=g["param"].t, m=g["m"].t, v=g["v"].t, cs=g["cs"].t, views=views, packed=eng.ilmlp_pack(*views),
                ws=eng.gail_disc_fit_ws(batch, in_dim), step=0)


def _run(eng, s, epochs, n_plcy, h):
    """The explicit update_mean_std(concat) then one oly_gail_disc_fit_epoch per epoch; returns the per-minibatch outputs."""
    rec = {k: [] for k in ("loss", "bce", "ent")}
    for e, (x, perm, t) in enumerate(epochs):
        xg = _dev(x, F32)
        nb = (int(xg.shape[0]) + h["batch"] - 1) // h["batch"]
        eng.col_stats(xg, s["cs"])
        o = {k: guarded(nb, F64) for k in rec}
        for k in o:
            s["g"][f"{k}_out_{s['step']}"] = o[k]
        eng.gail_disc_fit_epoch(xg, n_plcy, _dev(perm, torch.int32), h["batch"], s["cs"], s["param"], s["m"], s["v"],
                                s["packed"], s["ws"], s["step"], h["lr"], weight_decay=h["wd"], entcoeff=h["entcoeff"],
                                targets=None if t is None else _dev(t, F32), loss_out=o["loss"].t, bce_out=o["bce"].t,
                                ent_out=o["ent"].t)
        s["step"] += nb
        for k in rec:
            rec[k].append(o[k].t)
    torch.cuda.synchronize()
    assert sh.all_intact(s["g"]) == [], "written outside the buffer"
    return {k: torch.cat(v).cpu().numpy() for k, v in rec.items()}


# ------------------------------------------------------------------------------ the fit
@pytest.mark.parametrize("case", ["a", "b"])
def test_fit_epoch_against_the_reference_fixture(eng, case):
    g = np.load(fixture(case))
    h = hyper(g)
    s = _state(eng, gen.init_params(), h["batch"])
    rec = _run(eng, s, case_inputs(g), 640, h)
    for name, v in zip(gen.NAMES, s["views"]):
        r = rel(v.cpu().numpy(), g[f"final_{name}"])
        print(f"{case} {name}: rel to the reference {r:.3e}")
        assert r <= 2e-5, name
    for k in ("loss", "bce", "ent"):
        np.testing.assert_allclose(rec[k], g[k], rtol=2e-5, atol=2e-5, err_msg=k)
    check_statistics(s["cs"].cpu().numpy(), g)
    # the packed stream is the one oly_ilmlp_pack makes from the stepped parameters
    assert torch.equal(s["packed"], eng.ilmlp_pack(*s["views"]))


def test_fit_is_deterministic(eng):
    g = np.load(fixture("b"))
    h = hyper(g)
    runs = []
    for _ in range(2):
        s = _state(eng, gen.init_params(), h["batch"])
        rec = _run(eng, s, case_inputs(g), 640, h)
        runs.append((s, rec))
    (s0, r0), (s1, r1) = runs
    for k in ("param", "m", "v", "packed", "cs"):
        assert torch.equal(s0[k], s1[k]), k
    for k in r0:
        assert np.array_equal(r0[k], r1[k]), k


def test_fit_at_size_against_torch(eng):
    """65 536 policy rows + as many demonstration rows, minibatches of 2048: one epoch of 64 Adam steps against the
    float64 restatement on the GPU.  The bar is K15's: rel <= max(3 x torch-float32's rel, 1e-4) per tensor."""
    n, in_dim, batch = 65536, 32, 2048
    gg = torch.Generator(device="cuda").manual_seed(4)
    shift = torch.randn(in_dim, device="cuda", generator=gg)
    plcy = torch.randn((n, in_dim), device="cuda", generator=gg) * 1.5 + shift
    demo = torch.randn((n, in_dim), device="cuda", generator=gg) * 1.2 + shift + 0.4
    x = torch.cat([plcy, demo]).contiguous()
    perm = torch.randperm(2 * n, device="cuda", generator=gg)
    params = gen.init_params(seed=3)
    h = dict(entcoeff=1e-3, wd=0.0, lr=5e-5, batch=batch)
    s = _state(eng, params, batch)
    epochs = [(x, perm.cpu().numpy(), None)]
    rec = _run(eng, s, epochs, n, h)
    P, _, cs_ref, rec64, _ = restate_fit(epochs, n, params, np.zeros((3, in_dim)), 1e-3, 5e-5, batch, device="cuda")
    P32, _, _, _, _ = restate_fit(epochs, n, params, np.zeros((3, in_dim)), 1e-3, 5e-5, batch, dtype=torch.float32,
                                  device="cuda")
    for name, a, b, c in zip(gen.NAMES, s["views"], P, P32):
        r, r32 = rel(a.cpu().numpy(), b.cpu().numpy()), rel(c.cpu().numpy(), b.cpu().numpy())
        print(f"{name}: rel to float64 {r:.3e}, torch float32 {r32:.3e}")
        assert r <= max(3 * r32, 1e-4), (name, r, r32)
    for k in ("loss", "bce", "ent"):
        np.testing.assert_allclose(rec[k], rec64[k], rtol=1e-4, atol=1e-5, err_msg=k)
    np.testing.assert_allclose(s["cs"].cpu().numpy(), cs_ref.cpu().numpy(), rtol=1e-12)


def gail_case(c):
    """il_shapes' K15 case table for GAIL's network: the same rows, permutations and targets (the noise is dropped), the
    default initialisation at the case's in_dim; entcoeff 0.05 where the case carries explicit targets, else 1e-3."""
    _, epochs, h = sh.disc_case(c)
    return (gen.init_params(seed=100 + c.seed, in_dim=c.in_dim), [(x, perm, t) for x, perm, t, _ in epochs],
            dict(entcoeff=0.05 if c.targets else 1e-3, wd=h["wd"], lr=h["lr"], batch=h["batch"]))


def test_the_shape_table_covers_what_the_fit_accepts():
    def last(n, batch):
        return n - ((n - 1) // batch) * batch
    for d in (1, 17, 33, 45, 64):
        assert any(c.in_dim == d for c in K15_CASES), d
    assert any(c.batch > c.n_rows for c in K15_CASES)
    assert any(last(c.n_rows, c.batch) == 1 for c in K15_CASES)
    assert any(c.batch == 4096 and c.n_rows == 4097 for c in K15_CASES)
    assert any(c.n_plcy == c.n_rows for c in K15_CASES) and any(c.n_plcy == 0 for c in K15_CASES)
    assert any(c.targets and c.weight_decay > 0 for c in K15_CASES)


@pytest.mark.parametrize("c", K15_CASES, ids=case_id)
def test_fit_shapes(eng, c):
    params, epochs, h = gail_case(c)
    s = _state(eng, params, c.batch)
    rec = _run(eng, s, epochs, c.n_plcy, h)
    P, _, cs, rec64, step = restate_fit(epochs, c.n_plcy, params, np.zeros((3, c.in_dim)), h["entcoeff"], h["lr"],
                                        h["batch"], wd=h["wd"], device="cuda")
    assert s["step"] == step
    for name, a, b in zip(gen.NAMES, s["views"], P):
        r = rel(a.cpu().numpy(), b.cpu().numpy())
        print(f"{name}: {r:.2e} from float64")
        assert r <= TOL, (name, r)
    for k in ("loss", "bce", "ent"):
        np.testing.assert_allclose(rec[k], rec64[k], rtol=TOL, atol=TOL, err_msg=k)
    got, want = s["cs"].cpu().numpy(), cs.cpu().numpy()
    assert np.array_equal(got[0], want[0]), "the count"
    np.testing.assert_allclose(got, want, rtol=1e-12)
    assert torch.equal(s["packed"], eng.ilmlp_pack(*s["views"])), "the packed stream is the stepped parameters'"


# ------------------------------------------------------------------------------ the reward forward
def _reward_case(eng, B, seed=0, obs=34):
    g = torch.Generator(device="cuda").manual_seed(seed)
    scale = torch.rand(obs, device="cuda", generator=g) * 2.7 + 0.3
    x = (torch.randn((B, obs), device="cuda", generator=g) * scale + torch.randn(obs, device="cuda", generator=g)).contiguous()
    mask = _dev(gen.STATE_MASK, torch.int32)
    params = [_dev(p, F32) for p in gen.init_params(seed=7)]
    xm = x[:, mask.long()].contiguous()
    cs = eng.col_stats(xm)
    return x, xm, mask, params, eng.ilmlp_pack(*params), cs


def _ulps(a, b):
    ia, ib = a.contiguous().view(torch.int32).long(), b.contiguous().view(torch.int32).long()
    return int((ia - ib).abs().max())


def test_reward_forward_against_float64(eng):
    x, xm, mask, params, packed, cs = _reward_case(eng, 5000)
    o = eng.gail_disc_forward(x, packed, mask=mask, colstats=cs, want=("logits", "reward"))
    cnt = cs[0] + 1e-2
    mean = cs[1] / cnt
    sd = torch.sqrt(torch.clamp((cs[2] + 1e-2) / cnt - mean * mean, min=1e-2))
    xs = ((xm.double() - mean) / sd).float().double()
    d64 = forward([p.double() for p in params], xs)
    r = rel(o["logits"].cpu().numpy(), d64.cpu().numpy())
    print(f"logits: rel to float64 {r:.3e}")
    assert r <= 2e-5
    np.testing.assert_allclose(o["logits"].cpu().numpy(), d64.cpu().numpy(), rtol=2e-5, atol=2e-5)
    # the reward is reward_of (K8's oly_disc_reward) on those logits
    assert _ulps(o["reward"], eng.disc_reward(o["logits"])) <= 1
    assert torch.isfinite(o["reward"]).all()
    # mean / std given explicitly: the same values
    o2 = eng.gail_disc_forward(x, packed, mask=mask, mean=mean.contiguous(), std=sd.contiguous(), want=("logits",))
    assert torch.equal(o2["logits"], o["logits"])


def test_masked_in_kernel_equals_the_gathered_copy(eng):
    x, xm, mask, params, packed, cs = _reward_case(eng, 3001, seed=1)
    a = eng.gail_disc_forward(x, packed, mask=mask, colstats=cs, want=("logits", "reward"))
    b = eng.gail_disc_forward(xm, packed, colstats=cs, want=("logits", "reward"))
    assert torch.equal(a["logits"], b["logits"]) and torch.equal(a["reward"], b["reward"])
    # the one-call form: statistics of the masked rows, then the forward on them
    ca, cb = torch.zeros_like(cs), torch.zeros_like(cs)
    pa, pb = torch.empty_like(packed), torch.empty_like(packed)
    ra = eng.gail_reward_step(x, pa, ca, False, mask=mask, want=("logits", "reward"), weights=params)
    rb = eng.gail_reward_step(xm, pb, cb, False, want=("logits", "reward"), weights=params)
    assert torch.equal(ca, cb) and torch.equal(pa, packed) and torch.equal(pb, packed)
    assert torch.equal(ra["logits"], rb["logits"]) and torch.equal(ra["reward"], rb["reward"])
    np.testing.assert_allclose(ca.cpu().numpy(), cs.cpu().numpy(), rtol=1e-12)
    # accumulate: the running sums take the batch a second time
    eng.gail_reward_step(x, pa, ca, True, mask=mask)
    np.testing.assert_allclose(ca.cpu().numpy(), 2 * cs.cpu().numpy(), rtol=1e-12)


def test_16_and_32_row_tiles_identical(eng):
    x, xm, mask, params, packed, cs = _reward_case(eng, 409600, seed=2)
    big = eng.gail_disc_forward(x, packed, mask=mask, colstats=cs, want=("logits", "reward"))          # 32-row tiles
    small = eng.gail_disc_forward(x[:4096].contiguous(), packed, mask=mask, colstats=cs, want=("logits", "reward"))
    assert torch.equal(big["logits"][:4096], small["logits"]) and torch.equal(big["reward"][:4096], small["reward"])
    tail = eng.gail_disc_forward(x[409600 - 37:].contiguous(), packed, mask=mask, colstats=cs, want=("logits",))
    assert torch.equal(big["logits"][409600 - 37:], tail["logits"])


def test_first_minibatch_loss_matches_the_forward(eng):
    """loss_out[0] against the loss recomputed in f64 from oly_gail_disc_forward's logits for the same rows and the
    statistics that include the minibatch."""
    g = np.load(fixture("a"))
    h = hyper(g)
    x, perm, _ = case_inputs(g)[0]
    s = _state(eng, gen.init_params(), h["batch"])
    packed0 = s["packed"].clone()
    rec = _run(eng, s, [(x, perm, None)], 640, h)
    R = h["batch"]
    xb = torch.as_tensor(x[perm[:R]]).cuda().contiguous()
    cs = torch.as_tensor(x).cuda().double()
    cs = torch.stack([torch.full((32,), 1280.0 + R, device="cuda", dtype=torch.float64),
                      cs.sum(0) + xb.double().sum(0), (cs * cs).sum(0) + (xb.double() ** 2).sum(0)]).contiguous()
    d = eng.gail_disc_forward(xb, packed0, colstats=cs, want=("logits",))["logits"].double()
    t = (torch.as_tensor(perm[:R]).cuda() >= 640).double()
    loss = float(gail_loss(d, t, h["entcoeff"])[0])
    assert abs(loss - rec["loss"][0]) <= 1e-5, (loss, rec["loss"][0])


# ------------------------------------------------------------------------------ trainer and agent
def _trainer(eng, seed, **kw):
    from olympic_hip.gail import GAILDiscriminator, GAILDiscriminatorReward
    from olympic_hip.il_agent import DeviceGAILDiscriminatorTrainer
    torch.manual_seed(seed)
    net = GAILDiscriminator(32).cuda()
    r = GAILDiscriminatorReward(eng, net, state_mask=np.arange(2, 34))
    demo = np.random.default_rng(seed).normal(0.2, 1.0, (3000, 36)).astype(np.float32)
    args = dict(batch_size=1024, lr=5e-5)
    args.update(kw)
    return r, DeviceGAILDiscriminatorTrainer(r, demo, **args)


def test_trainer_steps_the_module_in_place(eng):
    from olympic_hip.gail import DeviceStandardizer, GAILDiscriminatorReward
    import copy
    r, tr = _trainer(eng, 1)
    plcy = torch.randn((1500, 36), device="cuda")
    before = [p.detach().clone() for p in r._params()]
    ptrs = [p.data_ptr() for p in r._params()]
    losses = tr.fit(plcy, generator=torch.Generator(device="cuda").manual_seed(0))
    torch.cuda.synchronize()
    assert losses.shape == (1, 3) and losses.dtype == torch.float64 and torch.isfinite(losses).all()
    assert tr.step == 3
    assert [p.data_ptr() for p in r._params()] == ptrs
    assert all(not torch.equal(a, b.detach()) for a, b in zip(before, r._params()))
    assert torch.equal(r._packed, eng.ilmlp_pack(*[p.detach() for p in r._params()]))
    # the reward uses the fitted weights: the same as a fresh reward object around a copy of the module
    x = torch.randn((3000, 36), device="cuda")
    cs0 = r.stand.colstats.clone()
    got = r(x).clone()
    st = DeviceStandardizer(eng, 32)
    st.colstats, st._fresh = cs0.clone(), False
    fresh = GAILDiscriminatorReward(eng, copy.deepcopy(r.net), state_mask=np.arange(2, 34), standardizer=st)
    assert torch.equal(fresh(x), got) and torch.equal(st.colstats, r.stand.colstats)
    # moments and step persist: a second fit continues from them
    m0 = tr.exp_avg.clone()
    tr.fit(plcy, generator=torch.Generator(device="cuda").manual_seed(1))
    torch.cuda.synchronize()
    assert tr.step == 6 and not torch.equal(tr.exp_avg, m0)


def test_a_write_through_data_between_fits_is_used(eng):
    r, tr = _trainer(eng, 2)
    plcy = torch.randn((1000, 36), device="cuda")
    tr.fit(plcy, generator=torch.Generator(device="cuda").manual_seed(0))
    r.net._linears[2].bias.data.fill_(5.0)
    r.net._linears[1].weight.data.zero_()
    tr.fit(plcy, generator=torch.Generator(device="cuda").manual_seed(1))
    torch.cuda.synchronize()
    assert abs(float(r.net._linears[2].bias.detach()) - 5.0) < 1e-2
    assert float(r.net._linears[1].weight.detach().abs().max()) < 1e-2
    # and by the reward: zeroed hidden weights leave the logit at (about) the bias for every row
    d = r.forward(torch.randn((64, 36), device="cuda"), want=("logits",))["logits"]
    assert float((d - 5.0).abs().max()) < 0.5


def test_trainer_draw_order_and_noisy_targets(eng):
    """demo, noisy targets (demo first), perm from the caller's generator: the fit equals the engine call on those draws."""
    r, tr = _trainer(eng, 4, use_noisy_targets=True, weight_decay=1e-3, entcoeff=0.05, batch_size=512)
    r2, _ = _trainer(eng, 4)
    plcy = torch.randn((700, 36), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    losses = tr.fit(plcy, generator=torch.Generator(device="cuda").manual_seed(9))
    g = torch.Generator(device="cuda").manual_seed(9)
    n = 700
    idx = torch.randperm(3000, generator=g, device="cuda")[:n]
    demo = tr.demo[idx][:, 2:34]
    x = torch.cat([plcy[:, 2:34], demo]).contiguous()
    demo_t = torch.empty(n, device="cuda").uniform_(0.80, 0.99, generator=g)
    plcy_t = torch.empty(n, device="cuda").uniform_(0.01, 0.10, generator=g)
    perm = torch.randperm(2 * n, generator=g, device="cuda").to(torch.int32)
    param = torch.cat([p.detach().reshape(-1) for p in r2._params()]).contiguous()
    cs = eng.col_stats(x)
    want = eng.gail_disc_fit_epoch(x, n, perm, 512, cs, param, torch.zeros_like(param), torch.zeros_like(param),
                                   r2.packed(), eng.gail_disc_fit_ws(512, 32), 0, 5e-5, weight_decay=1e-3, entcoeff=0.05,
                                   targets=torch.cat([plcy_t, demo_t]).contiguous())
    torch.cuda.synchronize()
    assert torch.equal(losses[0], want)
    assert torch.equal(torch.cat([p.detach().reshape(-1) for p in r._params()]), param)
    assert torch.equal(r.stand.colstats, cs)


def test_gail_agent_fit_equals_the_sequence_by_hand(eng):
    from olympic_hip.gail import DeviceStandardizer
    from olympic_hip.il_agent import DeviceILCritic, GAILAgent, VAILAgent
    assert issubclass(GAILAgent, VAILAgent)
    T, N = 20, 100

    def parts(seed):
        r, tr = _trainer(eng, seed, batch_size=512)
        torch.manual_seed(seed + 1)
        lins = [torch.nn.Linear(36, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 1)]
        return r, tr, DeviceILCritic(eng, lins, DeviceStandardizer(eng, 36))
    ra, ta, ca = parts(7)
    rb, tb, cb = parts(7)
    agent = GAILAgent(eng, ra, ta, ca, lambda o, a, adv, ag: None, train_D_n_th_epoch=2)
    for call in range(2):
        g = torch.Generator(device="cuda").manual_seed(call)
        s = torch.randn((T + 1, N, 36), device="cuda", generator=g)
        last = torch.zeros((T, N), dtype=torch.bool, device="cuda")
        last[-1] = True
        ds = dict(state=s[:-1].contiguous(), action=torch.randn((T, N, 11), device="cuda", generator=g),
                  reward=torch.randn((T, N), device="cuda", generator=g), next_state=s[1:].contiguous(),
                  absorbing=torch.zeros((T, N), dtype=torch.bool, device="cuda"), last=last)
        out = agent.fit(ds, generator=torch.Generator(device="cuda").manual_seed(10 + call))
        # ---- by hand: the agent's steps with the trainer called directly (gail_TRPO.py:105-165)
        gb = torch.Generator(device="cuda").manual_seed(10 + call)
        flat = ds["state"].reshape(T * N, 36)
        cb.stand.update_mean_std(flat)
        r_disc = rb(flat)
        cb(flat)
        cb(ds["next_state"].reshape(T * N, 36).contiguous())
        for _ in range(3):
            cb.stand.update_mean_std(flat)
        cb.fit(flat, out["v_target"].reshape(-1), n_epochs=3, batch_size=256, generator=gb)
        disc_loss = tb.fit(flat, generator=gb) if call == 1 else None
        torch.cuda.synchronize()
        assert torch.equal(out["reward"].reshape(-1), r_disc)
        assert out["disc_trained"] == (call == 1)
        if call == 1:
            assert torch.equal(out["disc_loss"], disc_loss)
        for pa, pb in zip(ra._params(), rb._params()):
            assert torch.equal(pa, pb)
        assert torch.equal(ra.stand.colstats, rb.stand.colstats)
        assert torch.equal(ca.param, cb.param)


def test_refusals(eng):
    from olympic_hip._ffi import OlyError
    from olympic_hip.gail import DiscriminatorReward, GAILDiscriminator, GAILDiscriminatorReward, VariationalDiscriminator
    from olympic_hip.il_agent import DeviceGAILDiscriminatorTrainer
    r, tr = _trainer(eng, 3)
    before = [p.detach().clone() for p in r._params()]
    with pytest.raises(OlyError):      # VAIL's reward object
        DeviceGAILDiscriminatorTrainer(DiscriminatorReward(eng, VariationalDiscriminator(in_dim=32).cuda()),
                                       np.zeros((10, 32)))
    for bad_net in (GAILDiscriminator(32, n_features=(256, 256)), GAILDiscriminator(65), GAILDiscriminator(32, (512,)),
                    torch.nn.Linear(32, 1)):
        with pytest.raises(OlyError):
            GAILDiscriminatorReward(eng, bad_net.cuda())
    with pytest.raises(OlyError):      # a mask of the wrong width
        GAILDiscriminatorReward(eng, GAILDiscriminator(32).cuda(), state_mask=np.arange(30))
    for bad in (4097, 0):
        with pytest.raises(OlyError):
            DeviceGAILDiscriminatorTrainer(r, np.zeros((10, 36)), batch_size=bad)
    with pytest.raises(OlyError):
        tr.fit(torch.zeros((0, 36), device="cuda"))
    with pytest.raises(OlyError):
        tr.fit(torch.zeros((10, 30), device="cuda"))
    with pytest.raises(OlyError):
        r(torch.zeros((10, 30), device="cuda"))
    # the engine: bad shapes never reach a launch
    s = _state(eng, gen.init_params(), 512)
    p0, m0, packed0 = s["param"].clone(), s["m"].clone(), s["packed"].clone()
    x = torch.randn((100, 32), device="cuda")
    perm = torch.randperm(100, device="cuda").to(torch.int32)
    for bad in (dict(batch=4097), dict(batch=0), dict(perm=perm[:10]), dict(n_plcy=101),
                dict(targets=torch.zeros(50, device="cuda")), dict(x=torch.randn((100, 65), device="cuda"))):
        a = dict(x=x, batch=512, perm=perm, n_plcy=50, targets=None)
        a.update(bad)
        with pytest.raises(OlyError):
            eng.gail_disc_fit_epoch(a["x"], a["n_plcy"], a["perm"], a["batch"], s["cs"], s["param"], s["m"], s["v"],
                                    s["packed"], s["ws"], 0, 5e-5, targets=a["targets"])
    out = dict(reward=torch.full((100,), -3.0, device="cuda"))
    for bad in (dict(x=torch.randn((100, 65), device="cuda")), dict(mask=torch.arange(33, device="cuda", dtype=torch.int32)),
                dict(want=()), dict(want=("mu",)), dict(colstats=torch.zeros((3, 31), dtype=torch.float64, device="cuda"))):
        a = dict(x=x, mask=None, want=("reward",), colstats=s["cs"])
        a.update(bad)
        with pytest.raises(OlyError):
            eng.gail_disc_forward(a["x"], s["packed"], mask=a["mask"], colstats=a["colstats"], want=a["want"], out=out)
        with pytest.raises(OlyError):
            eng.gail_reward_step(a["x"], s["packed"], a["colstats"], False, mask=a["mask"], want=a["want"], out=out)
    # the C entry points themselves refuse with OLY_EINVAL before any launch
    import ctypes as C
    from olympic_hip import _abi, _ffi
    L = _ffi.lib()
    for batch, in_dim, n_plcy in ((0, 32, 50), (4097, 32, 50), (512, 65, 50), (512, 32, 101)):
        f = _abi.GailDiscFit(in_dim=in_dim, n_plcy=n_plcy, step=0, lr=5e-5, beta1=0.9, beta2=0.999, adam_eps=1e-8,
                             weight_decay=0.0, entcoeff=1e-3, x=x.data_ptr(), colstats=s["cs"].data_ptr(),
                             param=s["param"].data_ptr(), exp_avg=s["m"].data_ptr(), exp_avg_sq=s["v"].data_ptr(),
                             packed=s["packed"].data_ptr(), ws=s["ws"].data_ptr(), ws_floats=s["ws"].numel())
        rc = L.oly_gail_disc_fit_epoch(eng.ctx.handle, C.byref(f), perm.data_ptr(), 100, batch, None)
        assert rc == _abi.OLY_EINVAL, (batch, in_dim, n_plcy, rc)
    rc = L.oly_gail_disc_forward(eng.ctx.handle, 100, 65, 65, x.data_ptr(), None, None, None, None, s["packed"].data_ptr(),
                                 out["reward"].data_ptr(), None, None)
    assert rc == _abi.OLY_EINVAL
    torch.cuda.synchronize()
    assert bool((s["cs"] == 0).all()) and torch.equal(s["param"], p0) and torch.equal(s["m"], m0)
    assert torch.equal(s["packed"], packed0) and bool((out["reward"] == -3.0).all())
    assert sh.all_intact(s["g"]) == []
    assert all(torch.equal(a, b.detach()) for a, b in zip(before, r._params()))
