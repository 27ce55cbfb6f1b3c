"""K16 on the MI355X: oly_ilmlp_forward against a float64 restatement, the critic's epoch call against the
reference-pinned fixture and against torch at size, determinism, refusals, and VAILAgent.fit against the same
sequence strung by hand."""
import gc

import numpy as np
import pytest
import torch

from test_il_critic_cpu import NAMES, initial_colstats, initial_params, rel, restate_fit

pytestmark = pytest.mark.gpu
FIXTURE_NAME = "il_critic/il_critic_fit.npz"


@pytest.fixture(scope="module")
def eng():
    from olympic_hip.engine import Engine
    e = Engine(0)
    yield e
    # release the context here: the refusal tests leave tracebacks (reference cycles) that hold the engine, and a
    # context freed later by the cycle collector could land inside another module's graph capture
    torch.cuda.synchronize()
    e.ctx.close()
    gc.collect()


def make_net(in_dim, out_dim, seed):
    torch.manual_seed(seed)
    return [torch.nn.Linear(in_dim, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, out_dim)]


def dev_params(lins):
    return [t.detach().float().cuda().contiguous() for lin in lins for t in (lin.weight, lin.bias)]


def ref_forward(x, lins, act, colstats=None, mean=None, std=None):
    xd = x.double()
    if colstats is not None:
        cnt = colstats[0] + 1e-2
        mean = colstats[1] / cnt
        std = torch.sqrt(torch.clamp((colstats[2] + 1e-2) / cnt - mean * mean, min=1e-2))
    if mean is not None:
        xd = ((xd - mean) / std).float().double()
    w = [t.detach().double().cuda() for lin in lins for t in (lin.weight, lin.bias)]
    y = torch.relu(torch.relu(xd @ w[0].T + w[1]) @ w[2].T + w[3]) @ w[4].T + w[5]
    return torch.tanh(y) if act == "tanh" else y


def close(y, ref, tol=1e-5):
    err = float((y.double() - ref).abs().max())
    scale = float(ref.abs().max()) + 1e-6
    assert err <= tol * scale, (err, scale)


@pytest.mark.parametrize("in_dim", [1, 16, 17, 32, 36, 45, 48, 64])
@pytest.mark.parametrize("out_dim", [1, 11, 32])
@pytest.mark.parametrize("act", ["identity", "tanh"])
def test_forward_against_float64(eng, in_dim, out_dim, act):
    lins = make_net(in_dim, out_dim, 100 * in_dim + out_dim)
    packed = eng.ilmlp_pack(*dev_params(lins))
    g = torch.Generator(device="cuda").manual_seed(in_dim + out_dim)
    big = (torch.randn((65536, in_dim), device="cuda", generator=g) * 2.0 + 0.5).contiguous()
    cs = torch.stack([torch.full((in_dim,), 5000.0, device="cuda", dtype=torch.float64),
                      big[:5000].double().sum(0), (big[:5000].double() ** 2).sum(0)]).contiguous()
    for N in (1, 17, 4096, 65536):
        if N == 65536 and in_dim not in (32, 64):
            continue
        x = big[:N].contiguous()
        for mode in ("none", "colstats"):
            kw = dict(colstats=cs) if mode == "colstats" else {}
            y = eng.ilmlp_forward(x, packed, out_dim, act, **kw)
            torch.cuda.synchronize()
            close(y, ref_forward(x, lins, act, colstats=cs if mode == "colstats" else None))
    # mean / std given directly
    mean = big.double().mean(0).contiguous()
    std = big.double().std(0).contiguous()
    y = eng.ilmlp_forward(big[:4096].contiguous(), packed, out_dim, act, mean=mean, std=std)
    close(y, ref_forward(big[:4096], lins, act, mean=mean, std=std))


def test_16_and_32_row_tiles_identical(eng):
    lins = make_net(32, 11, 3)
    packed = eng.ilmlp_pack(*dev_params(lins))
    x = torch.randn((65536, 32), device="cuda")
    cs = torch.stack([torch.full((32,), 100.0, device="cuda", dtype=torch.float64), x[:100].double().sum(0),
                      (x[:100].double() ** 2).sum(0)]).contiguous()
    for act in ("identity", "tanh"):
        y_big = eng.ilmlp_forward(x, packed, 11, act, colstats=cs)            # 32-row tiles
        y_small = eng.ilmlp_forward(x[:4096].contiguous(), packed, 11, act, colstats=cs)   # 16-row tiles
        torch.cuda.synchronize()
        assert torch.equal(y_big[:4096], y_small)


def _fit_state(eng, g):
    params = torch.cat([torch.as_tensor(p).reshape(-1) for p in initial_params(g)]).cuda().contiguous()
    views, o = [], 0
    for p in initial_params(g):
        views.append(params[o:o + p.size].view(p.shape))
        o += p.size
    packed = eng.ilmlp_pack(*views)
    return dict(param=params, exp_avg=torch.zeros_like(params), exp_avg_sq=torch.zeros_like(params), packed=packed,
                colstats=torch.as_tensor(initial_colstats(g)).cuda().contiguous(), ws=eng.il_critic_fit_ws(256, 32),
                views=views)


def _run_fixture_fit(eng, g):
    s = _fit_state(eng, g)
    x = torch.as_tensor(g["x"]).cuda().contiguous()
    vt = torch.as_tensor(g["v_target"]).reshape(-1).cuda().contiguous()
    losses, step = [], 0
    for perm in g["perms"]:
        p = torch.as_tensor(perm).cuda().contiguous()
        losses.append(eng.il_critic_fit_epoch(x, vt, p, 256, s["colstats"], s["param"], s["exp_avg"], s["exp_avg_sq"],
                                              s["packed"], s["ws"], step, float(g["lr"])))
        step += 4
    torch.cuda.synchronize()
    return s, torch.cat(losses).cpu().numpy()


def test_fit_epoch_against_the_reference_fixture(eng, golden):
    g = golden(FIXTURE_NAME)
    s, losses = _run_fixture_fit(eng, g)
    for n, v in zip(NAMES, s["views"]):
        r = rel(v.cpu().numpy(), g[f"final_{n}"])
        assert r <= 2e-5, (n, r)
    np.testing.assert_allclose(losses, g["losses"], rtol=2e-5)
    cs = s["colstats"].cpu().numpy()
    np.testing.assert_allclose(cs[0] + 1e-2, np.full(32, g["st_count"][0]), rtol=0, atol=1e-9)
    np.testing.assert_allclose(cs[1], g["st_sum"], rtol=1e-6, atol=1e-3)
    np.testing.assert_allclose(cs[2] + 1e-2, g["st_sumsq"], rtol=1e-6)


def test_fit_is_deterministic_and_keeps_the_packed_stream_current(eng, golden):
    g = golden(FIXTURE_NAME)
    a, la = _run_fixture_fit(eng, g)
    b, lb = _run_fixture_fit(eng, g)
    assert torch.equal(a["param"], b["param"]) and torch.equal(a["exp_avg_sq"], b["exp_avg_sq"])
    assert torch.equal(a["colstats"], b["colstats"]) and np.array_equal(la, lb)
    fresh = eng.ilmlp_pack(*a["views"])
    torch.cuda.synchronize()
    assert torch.equal(fresh, a["packed"])


def test_fit_at_size_against_torch(eng):
    """409 600 rows, minibatches of 256, one epoch (1600 Adam steps) against the float64 restatement on the GPU."""
    n, in_dim = 409600, 32
    lins = make_net(in_dim, 1, 11)
    params = [t.detach().numpy().copy() for lin in lins for t in (lin.weight, lin.bias)]
    gen = torch.Generator(device="cuda").manual_seed(4)
    x = (torch.randn((n, in_dim), device="cuda", generator=gen) * 1.5 + 0.3).contiguous()
    vt = (x[:, 0] * 0.5 + torch.randn(n, device="cuda", generator=gen)).contiguous()
    perm = torch.randperm(n, device="cuda", generator=gen).to(torch.int32)
    flat = torch.cat([torch.as_tensor(p).reshape(-1) for p in params]).cuda().contiguous()
    views, o = [], 0
    for p in params:
        views.append(flat[o:o + p.size].view(p.shape))
        o += p.size
    packed = eng.ilmlp_pack(*views)
    cs = torch.zeros((3, in_dim), dtype=torch.float64, device="cuda")
    m, v, ws = torch.zeros_like(flat), torch.zeros_like(flat), eng.il_critic_fit_ws(256, in_dim)
    losses = eng.il_critic_fit_epoch(x, vt, perm, 256, cs, flat, m, v, packed, ws, 0, 1e-4).cpu().numpy()
    P, _, cs_ref, losses_ref, _ = restate_fit(x, vt, [perm.long().cpu().numpy()], params,
                                              np.zeros((3, in_dim)), 1e-4, 256, device="cuda")
    # over 1600 Adam steps float32 and float64 trajectories separate (ReLU-mask flips, Adam's sign-like steps on
    # gradients near zero): the yardstick is how far torch's own float32 run lands from float64
    P32, _, _, losses32, _ = restate_fit(x, vt, [perm.long().cpu().numpy()], params, np.zeros((3, in_dim)), 1e-4, 256,
                                         dtype=torch.float32, device="cuda")
    for n_, a, b, c in zip(NAMES, views, P, P32):
        r, r32 = rel(a.cpu().numpy(), b.cpu().numpy()), rel(c.cpu().numpy(), b.cpu().numpy())
        print(f"{n_}: rel to float64 {r:.3e}, torch float32 {r32:.3e}")
        assert r <= max(3 * r32, 1e-4), (n_, r, r32)
    np.testing.assert_allclose(losses[:8], losses_ref[:8], rtol=1e-4)
    for lo in (losses, losses32):
        assert abs(lo[-200:].mean() / losses_ref[-200:].mean() - 1) < 1e-2
    np.testing.assert_allclose(cs.cpu().numpy(), cs_ref.cpu().numpy(), rtol=1e-12)


def test_unsupported_shapes_refused_before_launch(eng):
    from olympic_hip._ffi import OlyError
    lins = make_net(32, 1, 1)
    packed = eng.ilmlp_pack(*dev_params(lins))
    x = torch.randn((64, 32), device="cuda")
    y = torch.full((64, 1), float("nan"), device="cuda")
    with pytest.raises(OlyError):
        eng.ilmlp_pack(*dev_params(make_net(65, 1, 1)))
    with pytest.raises(OlyError):
        eng.ilmlp_pack(*dev_params(make_net(32, 33, 1)))
    with pytest.raises(OlyError):
        eng.ilmlp_forward(x, packed, 1, "relu", y=y)
    with pytest.raises(OlyError):
        eng.ilmlp_forward(x, packed[:-4], 1, y=y)
    with pytest.raises(OlyError):
        eng.ilmlp_forward(x.double(), packed, 1, y=y)
    with pytest.raises(OlyError):     # mean without std
        eng.ilmlp_forward(x, packed, 1, mean=torch.zeros(32, dtype=torch.float64, device="cuda"), y=y)
    flat = torch.cat([p.reshape(-1) for p in dev_params(lins)])
    cs = torch.zeros((3, 32), dtype=torch.float64, device="cuda")
    perm = torch.arange(64, dtype=torch.int32, device="cuda")
    for bad in (dict(batch=257), dict(batch=0), dict(perm=perm[:10]), dict(x=torch.randn((64, 65), device="cuda"))):
        args = dict(x=x, batch=256, perm=perm)
        args.update(bad)
        with pytest.raises(OlyError):
            eng.il_critic_fit_epoch(args["x"], torch.zeros(64, device="cuda"), args["perm"], args["batch"], cs, flat,
                                    torch.zeros_like(flat), torch.zeros_like(flat), packed,
                                    eng.il_critic_fit_ws(256, 32), 0, 1e-4)
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and bool((cs == 0).all())


# ------------------------------------------------------------------------------ VAILAgent
class _Trainer:
    def __init__(self):
        self.calls = []

    def fit(self, x, generator=None):
        self.calls.append(int(x.shape[0]))
        return [0.0]


def _agent_parts(eng, seed):
    from olympic_hip.gail import DeviceStandardizer, DiscriminatorReward, VariationalDiscriminator
    from olympic_hip.il_agent import DeviceILCritic
    torch.manual_seed(seed)
    dnet = VariationalDiscriminator(in_dim=32).cuda()
    disc = DiscriminatorReward(eng, dnet)
    crit_lins = make_net(32, 1, seed + 1)
    stand = DeviceStandardizer(eng, 32)
    critic = DeviceILCritic(eng, crit_lins, stand, lr=1e-4)
    return disc, critic, stand


def _dataset(T, N, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    s = torch.randn((T + 1, N, 32), device="cuda", generator=g)
    absorbing = torch.rand((T, N), device="cuda", generator=g) < 0.02
    last = (torch.rand((T, N), device="cuda", generator=g) < 0.05) | absorbing
    last[-1] = True
    return dict(state=s[:-1].contiguous(), action=torch.randn((T, N, 11), device="cuda", generator=g),
                reward=torch.randn((T, N), device="cuda", generator=g), next_state=s[1:].contiguous(),
                absorbing=absorbing, last=last)


def test_vail_agent_fit_equals_the_sequence_by_hand(eng):
    from olympic_hip import _abi
    from olympic_hip.il_agent import VAILAgent
    from olympic_hip.rollout import GAERollout, RolloutBuffer
    T, N = 20, 100
    disc_a, critic_a, stand_a = _agent_parts(eng, 5)
    disc_b, critic_b, stand_b = _agent_parts(eng, 5)
    trainer = _Trainer()
    seen = []
    agent = VAILAgent(eng, disc_a, trainer, critic_a, lambda o, a, adv, ag: seen.append(adv.clone()),
                      env_reward_frac=0.25, train_D_n_th_epoch=3)
    post = GAERollout(eng, gamma=0.99, lam=0.97)
    rows_added, it, d_calls = 0, 1, []
    for call in range(3):
        ds = _dataset(T, N, 40 + call)
        eps = torch.randn((T * N, 128), device="cuda", generator=torch.Generator(device="cuda").manual_seed(call))
        ga = torch.Generator(device="cuda").manual_seed(100 + call)
        out = agent.fit(ds, eps=eps, generator=ga)
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
        for _ in range(3):
            stand_b.update_mean_std(flat)
        critic_b.fit(flat, v_target.reshape(-1), n_epochs=3, batch_size=256, generator=gb)
        if it % 3 == 0:
            d_calls.append(call)
        it += 1
        rows_added += T * N * (1 + 2 + 3 + 3)      # update, V(x), V(xn), n_epochs updates, 3 fit epochs
        torch.cuda.synchronize()
        assert torch.equal(out["reward"], r)
        assert torch.equal(out["v_target"], v_target) and torch.equal(out["adv"], adv)
        assert torch.equal(seen[-1], adv.reshape(-1))
        assert torch.equal(critic_a.param, critic_b.param) and torch.equal(critic_a.packed, critic_b.packed)
        assert torch.equal(stand_a.colstats, stand_b.colstats)
        assert out["disc_trained"] == (call in d_calls)
    assert d_calls == [2] and trainer.calls == [T * N]
    assert float(stand_a.colstats[0, 0]) == rows_added
    # sync_to_torch hands the fitted weights back to the module
    critic_a.sync_to_torch()
    assert torch.equal(critic_a.lins[1].weight.detach().cuda().reshape(-1),
                       critic_a.param[512 * 32 + 512:512 * 32 + 512 + 256 * 512])
