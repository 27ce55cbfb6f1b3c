"""The paired discriminator inputs, (s, s') with use_next_states and (s, a) with actions, on the MI355X: K12 / K15 (VAIL)
and K18 (GAIL) through the oly_*_pair entry points against the four reference-run fixtures of
tests/golden/disc_pair_fit/ and the float64 restatement of tests/pair_restate.py; the bit-for-bit properties (masked
sources, tile heights, two runs, states only through the new entry points); the trainers and the agents.

The shape sweep takes (Ds, D2) from (1,1), (17,16), (32,32), (33,31), (45,19), (63,1), (1,63).  All seven run with
actions.  Next states share the state mask, so D2 == Ds there: that mode runs the pairs with equal halves, (1,1) and
(32,32), and (17,17) in place of (17,16)."""
import copy
import gc

import numpy as np
import pytest
import torch

import il_shapes as sh
import pair_restate as pr
from il_shapes import TOL, guarded

pytestmark = pytest.mark.gpu
gen = pr.gen
F32, F64, I32 = torch.float32, torch.float64, torch.int32


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


def _dev(a, dtype=None):
    t = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
    return t.to(device="cuda", dtype=dtype).contiguous()


def shapes(algo, d):
    if algo == "gail":
        return [(512, d), (512,), (256, 512), (256,), (1, 256), (1,)]
    return [(256, d), (256,), (128, 256), (128,), (128, 128), (128,), (128, 128), (128,), (1, 128), (1,)]


def pack(eng, algo, views):
    return (eng.ilmlp_pack if algo == "gail" else eng.disc_pack)(*views)


def _state(eng, algo, params, batch, ds, d2, standardise):
    """The fit's buffers, those whose size depends on the shape between sentinels."""
    flat = np.concatenate([np.asarray(p, dtype=np.float32).reshape(-1) for p in params])
    g = dict(param=guarded(flat.size, F32, init=flat), m=guarded(flat.size, F32), v=guarded(flat.size, F32),
             cs=guarded((3, ds), F64), beta=guarded(1, F32, init=[0.1]))
    views = sh.views(g["param"].t, shapes(algo, ds + d2))
    # the packed stream and the workspace are written by the kernels: both between sentinels too (the margins keep the
    # interiors' 256-byte alignment)
    packed = pack(eng, algo, views)
    g["packed"] = guarded(int(packed.numel()), F32, init=packed)
    ws = (eng.gail_disc_fit_pair_ws if algo == "gail" else eng.disc_fit_pair_ws)(batch, ds, d2, standardise)
    assert ws.dtype == F32
    g["ws"] = guarded(int(ws.numel()), F32)
    return dict(g=g, algo=algo, param=g["param"].t, m=g["m"].t, v=g["v"].t, cs=g["cs"].t, beta=g["beta"].t, views=views,
                packed=g["packed"].t, ws=g["ws"].t, step=0, standardise=standardise)


def _run(eng, s, epochs, n_plcy, h):
    """The explicit update_mean_std of the STATES, then one oly_*_fit_epoch_pair per epoch; every input and output
    between sentinels.  Returns the per-minibatch outputs."""
    algo = s["algo"]
    keys = ("loss", "bce", "ent") if algo == "gail" else ("loss", "bce", "kl", "beta")
    rec = {k: [] for k in keys}
    for e, (x, x2, perm, t, noise) in enumerate(epochs):
        n = int(np.asarray(x).shape[0])
        nb = (n + h["batch"] - 1) // h["batch"]
        tag = f"{s['step']}"
        gi = dict(x=guarded(np.asarray(x).shape, F32, init=x), x2=guarded(np.asarray(x2).shape, F32, init=x2))
        perm_d = _dev(np.asarray(perm), I32)          # read only by the kernels (the sentinel has no int32 value)
        if t is not None:
            gi["t"] = guarded(n, F32, init=t)
        if noise is not None:
            gi["noise"] = guarded((n, 128), F32, init=noise)
        o = {k: guarded(nb, F32 if k == "beta" else F64) for k in keys}
        for k, v in list(gi.items()) + list(o.items()):
            s["g"][f"{k}_{tag}"] = v
        eng.col_stats(gi["x"].t, s["cs"])
        tt = gi["t"].t if t is not None else None
        if algo == "gail":
            eng.gail_disc_fit_epoch_pair(gi["x"].t, gi["x2"].t, s["standardise"], n_plcy, perm_d, h["batch"], s["cs"],
                                         s["param"], s["m"], s["v"], s["packed"], s["ws"], s["step"], h["lr"],
                                         weight_decay=h["wd"], entcoeff=h["entcoeff"], targets=tt, loss_out=o["loss"].t,
                                         bce_out=o["bce"].t, ent_out=o["ent"].t)
        else:
            eng.disc_fit_epoch_pair(gi["x"].t, gi["x2"].t, s["standardise"], n_plcy, gi["noise"].t, perm_d, h["batch"],
                                    s["cs"], s["param"], s["m"], s["v"], s["packed"], s["beta"], s["ws"], s["step"],
                                    h["lr"], weight_decay=h["wd"], info_constraint=h["info_c"], lr_beta=h["lr_beta"],
                                    targets=tt, loss_out=o["loss"].t, bce_out=o["bce"].t, kl_out=o["kl"].t,
                                    beta_out=o["beta"].t)
        s["step"] += nb
        for k in rec:
            rec[k].append(o[k].t.double())
    torch.cuda.synchronize()
    assert sh.all_intact(s["g"]) == [], "written outside the buffer"
    return {k: torch.cat(v).cpu().numpy() for k, v in rec.items()}


def _reward(eng, algo, s_full, x2_full, params, cs, standardise, mask=None, mask2=None, noise=None, accumulate=True,
            bufs=None):
    """oly_*_reward_step_pair with the weights re-packed inside the call, outputs between sentinels.
    Returns (logits, reward, S1 scratch)."""
    ds = int(cs.shape[1])
    B = int(s_full.shape[0])
    d2 = int(x2_full.shape[1]) if mask2 is None else int(mask2.shape[0])
    g = dict(logits=guarded(B, F32), reward=guarded(B, F32), sa=guarded((3, ds), F64))
    views = [_dev(p, F32) for p in params]
    packed = guarded(int(pack(eng, algo, views).numel()), F32)
    g["packed"] = packed
    out = dict(logits=g["logits"].t, reward=g["reward"].t)
    if algo == "gail":
        eng.gail_reward_step_pair(s_full, x2_full, packed.t, cs, g["sa"].t, accumulate, standardise, mask=mask, mask2=mask2,
                                  want=("logits", "reward"), out=out, weights=views)
    else:
        eng.disc_reward_step_pair(s_full, x2_full, packed.t, cs, g["sa"].t, accumulate, standardise, mask=mask, mask2=mask2,
                                  eps=noise, want=("logits", "reward"), out=out, weights=views)
    torch.cuda.synchronize()
    assert sh.all_intact(g) == [], "written outside the buffer"
    assert torch.equal(packed.t, pack(eng, algo, views))
    assert ds + d2 == int(views[0].shape[1])
    if bufs is not None:
        bufs.update(g)
    return g["logits"].t, g["reward"].t, g["sa"].t


# ------------------------------------------------------------------------------ the fixtures
@pytest.mark.parametrize("case", pr.CASES)
def test_fit_and_reward_against_the_reference_fixture(eng, case):
    g = np.load(pr.fixture(case))
    algo, ns = pr.case_algo(case), pr.case_standardise(case)
    ds, d2 = gen.widths(case)
    h = pr.case_hyper(g, case)
    data = gen.inputs()
    s = _state(eng, algo, gen.init_params(case), h["batch"], ds, d2, ns)
    rec = _run(eng, s, pr.case_epochs(g, case, data), gen.N_PLCY, h)
    for name, v in zip(gen.names(case), s["views"]):
        r = pr.rel(v.cpu().numpy(), g[f"final_{name}"])
        print(f"{case} {name}: rel to the reference {r:.3e}")
        assert r <= TOL, name
    for k in rec:
        print(f"{case} {k}: max err {np.abs(rec[k] - g[k]).max():.3e}")
        np.testing.assert_allclose(rec[k], g[k], rtol=TOL, atol=TOL, err_msg=k)
    pr.check_statistics(s["cs"].cpu().numpy(), g, "fit_st")
    assert torch.equal(s["packed"], pack(eng, algo, s["views"])), "the packed stream is the stepped parameters'"
    # ---- the held-out reward with the fitted parameters: full-width sources, both masks applied in the kernels
    ref = pr.restate_case(case, g, device="cuda")
    mask = _dev(g["state_mask"], I32)
    second = data["hold_next"] if ns else data["hold_act"]
    mask2 = mask if ns else _dev(g["act_mask"], I32)
    noise = None if algo == "gail" else _dev(gen.noise(case)[-gen.N_HOLD:], F32)
    cnt0 = float(s["cs"][0, 0])
    d, r, sa = _reward(eng, algo, _dev(data["hold_obs"], F32), _dev(second, F32), [v.clone() for v in s["views"]], s["cs"], ns,
                       mask=mask, mask2=mask2, noise=noise)
    dn, rn = d.cpu().numpy(), r.cpu().numpy()
    e_fix, e_ref = pr.rel(dn, g["reward_logits"]), pr.rel(dn, ref["logits"].cpu().numpy())
    print(f"{case}: logits rel to the fixture {e_fix:.3e}, to float64 {e_ref:.3e}")
    assert e_fix <= TOL and e_ref <= TOL
    np.testing.assert_allclose(dn, g["reward_logits"], rtol=TOL, atol=TOL)
    # r = -log(1 - sigmoid(d) + 1e-8) has |dr / dd| = sigmoid(d) <= 1: a logit within TOL (1 + |d|) gives a reward within
    # that, plus the float32 steps of the formula itself (a few 1e-7 on 1 - p >= e^-4 here)
    bound = TOL * (1 + np.abs(g["reward_logits"])) + 2e-6
    assert np.abs(g["reward_logits"]).max() < 4 and (np.abs(rn - g["reward"]) <= bound).all()
    pr.check_statistics(s["cs"].cpu().numpy(), g, "st")
    # the count: 2 B with next states, B with actions
    assert float(s["cs"][0, 0]) - cnt0 == (2 if ns else 1) * gen.N_HOLD
    if ns:
        assert float(sa[0, 0]) - cnt0 == gen.N_HOLD            # S1: the states are in, the next states not yet


@pytest.mark.parametrize("case", ["gail_ns", "vail_sa"])
def test_fit_is_deterministic(eng, case):
    g = np.load(pr.fixture(case))
    algo, ns = pr.case_algo(case), pr.case_standardise(case)
    h = pr.case_hyper(g, case)
    runs = []
    for _ in range(2):
        s = _state(eng, algo, gen.init_params(case), h["batch"], *gen.widths(case), ns)
        runs.append((s, _run(eng, s, pr.case_epochs(g, case), gen.N_PLCY, h)))
    (s0, r0), (s1, r1) = runs
    for k in ("param", "m", "v", "packed", "cs", "beta"):
        assert torch.equal(s0[k], s1[k]), k
    for k in r0:
        assert np.array_equal(r0[k], r1[k]), k


# ------------------------------------------------------------------------------ the shape sweep
PAIRS_ACTION = ((1, 1), (17, 16), (32, 32), (33, 31), (45, 19), (63, 1), (1, 63))
PAIRS_NEXT = ((1, 1), (17, 17), (32, 32))
ROWS = ((7, 20, 10), (3, 10, 5), (256, 257, 128), (64, 199, 99), (100, 250, 125), (512, 300, 300), (333, 1022, 0))
SWEEP = [(a, "action", p, ROWS[i % len(ROWS)]) for a in ("gail", "vail") for i, p in enumerate(PAIRS_ACTION)] + \
        [(a, "next_state", p, ROWS[(i + 2) % len(ROWS)]) for a in ("gail", "vail") for i, p in enumerate(PAIRS_NEXT)]


def sweep_case(algo, mode, ds, d2, batch, n_rows, n_plcy, seed, epochs=2):
    """(params, epochs, hyper): columns with a scale and a shift each, the second part distributed differently from the
    first; nn.Linear's default initialisation (VAIL, il_shapes.disc_params) or the reference's rule (GAIL)."""
    rng = np.random.default_rng(3000 + seed)
    scale, shift = rng.uniform(0.3, 3.0, ds), rng.standard_normal(ds) * 2.0
    scale2 = scale if mode == "next_state" else rng.uniform(0.2, 1.5, d2)
    out = []
    targets = seed % 2 == 1
    for _ in range(epochs):
        x = rng.standard_normal((n_rows, ds)) * scale + shift
        x[n_plcy:] += 0.4 * scale
        x2 = (0.6 * x + 1.5 * scale + rng.standard_normal((n_rows, ds)) * 0.5 * scale if mode == "next_state"
              else rng.standard_normal((n_rows, d2)) * scale2 + 0.2)
        t = None
        if targets:
            t = np.concatenate([rng.uniform(0.01, 0.10, n_plcy), rng.uniform(0.80, 0.99, n_rows - n_plcy)]).astype(np.float32)
        noise = None if algo == "gail" else rng.standard_normal((n_rows, 128)).astype(np.float32)
        out.append((x.astype(np.float32), x2.astype(np.float32), rng.permutation(n_rows), t, noise))
    params = gen.gail_init(ds + d2, seed=100 + seed) if algo == "gail" else sh.disc_params(ds + d2, seed)
    h = dict(lr=1e-3, batch=batch, wd=1e-3 if targets else 0.0)
    h.update(dict(entcoeff=0.05 if targets else 1e-3) if algo == "gail" else dict(info_c=0.1, lr_beta=1e-3))
    return params, out, h


def test_the_sweep_covers_what_the_issue_lists():
    got = {(m, p) for _, m, p, _ in SWEEP}
    assert {("action", p) for p in PAIRS_ACTION} <= got
    assert {p for m, p in got if m == "next_state"} >= {(1, 1), (32, 32)} and all(a == b for m, (a, b) in got if m == "next_state")
    assert all(a + b <= 64 for _, (a, b) in got) and any(a + b == 64 for _, (a, b) in got)

    def last(n, b):
        return n - ((n - 1) // b) * b
    assert any(last(n, b) == 1 for b, n, _ in ROWS) and any(b > n for b, n, _ in ROWS)
    assert any(p == 0 for _, _, p in ROWS) and any(p == n for _, n, p in ROWS)


@pytest.mark.parametrize("algo,mode,pair,rows", SWEEP, ids=[f"{a}-{m}-{p[0]}+{p[1]}-b{r[0]}n{r[1]}" for a, m, p, r in SWEEP])
def test_fit_and_reward_shapes(eng, algo, mode, pair, rows):
    (ds, d2), (batch, n_rows, n_plcy) = pair, rows
    ns = mode == "next_state"
    seed = SWEEP.index((algo, mode, pair, rows))
    params, epochs, h = sweep_case(algo, mode, ds, d2, batch, n_rows, n_plcy, seed)
    s = _state(eng, algo, params, batch, ds, d2, ns)
    rec = _run(eng, s, epochs, n_plcy, h)
    out = pr.restate_fit(algo, epochs, n_plcy, params, np.zeros((3, ds)), ns, device="cuda", **h)
    P, cs, rec64, step = out[0], out[2], out[3], out[4]
    assert s["step"] == step
    for i, (a, b) in enumerate(zip(s["views"], P)):
        r = pr.rel(a.cpu().numpy(), b.cpu().numpy())
        print(f"tensor {i}: {r:.2e} from float64")
        assert r <= TOL, (i, r)
    for k in rec:
        np.testing.assert_allclose(rec[k], rec64[k], rtol=TOL, atol=TOL, err_msg=k)
    got, want = s["cs"].cpu().numpy(), cs.cpu().numpy()
    assert np.array_equal(got[0], want[0]), "the count"
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-9)
    assert torch.equal(s["packed"], pack(eng, algo, s["views"]))
    # ---- the reward on the fitted state, both tile heights' worth of rows left to the entry point's choice
    x, x2 = _dev(epochs[0][0], F32), _dev(epochs[0][1], F32)
    noise = None if algo == "gail" else _dev(epochs[0][4], F32)
    d64, r64, cs64 = pr.restate_reward(algo, P, cs, x, x2, ns, noise=noise, device="cuda")
    d, r, _ = _reward(eng, algo, x, x2, [v.clone() for v in s["views"]], s["cs"], ns, noise=noise)
    np.testing.assert_allclose(d.cpu().numpy(), d64.cpu().numpy(), rtol=TOL, atol=TOL)
    np.testing.assert_allclose(s["cs"].cpu().numpy(), cs64.cpu().numpy(), rtol=1e-12, atol=1e-9)
    assert float(s["cs"][0, 0]) == float(cs64[0, 0])


# ------------------------------------------------------------------------------ bit for bit
def _reward_inputs(B, seed, obs=36, act=13):
    g = torch.Generator(device="cuda").manual_seed(seed)
    scale = torch.rand(obs, device="cuda", generator=g) * 2.7 + 0.3
    s = (torch.randn((B, obs), device="cuda", generator=g) * scale + torch.randn(obs, device="cuda", generator=g)).contiguous()
    sn = (0.6 * s + 1.5 * scale + torch.randn((B, obs), device="cuda", generator=g) * 0.5 * scale).contiguous()
    a = torch.randn((B, act), device="cuda", generator=g).contiguous()
    noise = torch.randn((B, 128), device="cuda", generator=g).contiguous()
    return s, sn, a, noise


@pytest.mark.parametrize("algo", ["gail", "vail"])
@pytest.mark.parametrize("mode", ["next_state", "action"])
def test_masked_sources_equal_pregathered_copies(eng, algo, mode):
    ns = mode == "next_state"
    s, sn, a, noise = _reward_inputs(3001, 1)
    mask = _dev(np.arange(2, 34), I32)
    mask2 = mask if ns else _dev(gen.ACT_MASK, I32)
    x2 = sn if ns else a
    d2 = int(mask2.numel())
    params = gen.gail_init(32 + d2, seed=7) if algo == "gail" else sh.disc_params(32 + d2, 7)
    ca, cb = torch.zeros((3, 32), dtype=F64, device="cuda"), torch.zeros((3, 32), dtype=F64, device="cuda")
    nz = None if algo == "gail" else noise
    for acc in (False, True):
        da, ra, sa = _reward(eng, algo, s, x2, params, ca, ns, mask=mask, mask2=mask2, noise=nz, accumulate=acc)
        db, rb, sb = _reward(eng, algo, s[:, mask.long()].contiguous(), x2[:, mask2.long()].contiguous(), params, cb, ns,
                             noise=nz, accumulate=acc)
        assert torch.equal(da, db) and torch.equal(ra, rb) and torch.equal(ca, cb)
        if ns:
            assert torch.equal(sa, sb)
    assert float(ca[0, 0]) == (4 if ns else 2) * 3001


@pytest.mark.parametrize("algo", ["gail", "vail"])
def test_16_and_32_row_tiles_identical(eng, algo):
    """The entry points choose the tile height from the batch: 409 600 rows take 32-row tiles, 4096 rows and the ragged
    tail 16-row tiles, in both modes."""
    B = 409600
    s, sn, a, noise = _reward_inputs(B, 2)
    mask = _dev(np.arange(2, 34), I32)
    for ns, x2, mask2 in ((True, sn, mask), (False, a, _dev(gen.ACT_MASK, I32))):
        d2 = int(mask2.numel())
        params = [_dev(p, F32) for p in (gen.gail_init(32 + d2, seed=8) if algo == "gail" else sh.disc_params(32 + d2, 8))]
        packed = pack(eng, algo, params)
        sa = eng.col_stats(s[:4096, mask.long()].contiguous())
        sb = eng.col_stats(sn[:4096, mask.long()].contiguous(), sa.clone())

        def fwd(lo, hi):
            kw = dict(mask=mask, mask2=mask2, stats_a=sa, stats_b=sb, want=("logits", "reward"))
            if algo == "gail":
                return eng.gail_disc_forward_pair(s[lo:hi].contiguous(), x2[lo:hi].contiguous(), packed, ns, **kw)
            return eng.disc_forward_pair(s[lo:hi].contiguous(), x2[lo:hi].contiguous(), packed, ns,
                                         eps=noise[lo:hi].contiguous(), **kw)
        big, small, tail = fwd(0, B), fwd(0, 4096), fwd(B - 37, B)
        torch.cuda.synchronize()
        for k in ("logits", "reward"):
            assert torch.equal(big[k][:4096], small[k]) and torch.equal(big[k][B - 37:], tail[k]), (ns, k)


@pytest.mark.parametrize("algo", ["gail", "vail"])
def test_states_only_through_the_new_entry_points_equals_the_old(eng, algo):
    """pair NULL: the paired entry points are the existing ones, bit for bit (reward step, forward, fit)."""
    import ctypes as C
    from olympic_hip import _abi, _ffi
    from olympic_hip.engine import ptr
    L, h = _ffi.lib(), eng.ctx.handle
    s, _, _, noise = _reward_inputs(5000, 3)
    mask = _dev(np.arange(2, 34), I32)
    params = [_dev(p, F32) for p in (gen.gail_init(32, seed=9) if algo == "gail" else sh.disc_params(32, 9))]
    packed = pack(eng, algo, params)
    xm = s[:, mask.long()].contiguous()
    cs_old, cs_new = torch.zeros((3, 32), dtype=F64, device="cuda"), torch.zeros((3, 32), dtype=F64, device="cuda")
    d_new, r_new = torch.empty(5000, device="cuda"), torch.empty(5000, device="cuda")
    if algo == "gail":
        old = eng.gail_reward_step(s, packed, cs_old, False, mask=mask, want=("logits", "reward"))
        rc = L.oly_gail_reward_step_pair(h, 5000, 36, 32, ptr(s), ptr(mask), None, ptr(cs_new), None, 0, None, ptr(packed),
                                         ptr(r_new), ptr(d_new), eng._s())
    else:
        old = eng.disc_reward_step(xm, packed, cs_old, False, eps=noise, want=("logits", "reward"))
        rc = L.oly_disc_reward_step_pair(h, 5000, 32, 32, ptr(xm), None, None, ptr(cs_new), None, 0, None, ptr(packed),
                                         ptr(noise), ptr(r_new), ptr(d_new), None, None, eng._s())
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(old["logits"], d_new) and torch.equal(old["reward"], r_new)
    assert torch.equal(cs_new, cs_old)
    if algo == "vail":
        # states only WITH a mask is a path of its own (K18's statistics launches, then oly_disc_forward with the mask),
        # which the call above, forwarded whole to oly_disc_reward_step, does not reach.  Against the existing entry
        # point on the gathered copy the statistics are sums of the same float64 terms in another order (5000 terms of
        # magnitude below 1e3: well inside 1e-12 relative + 1e-9) and the logits agree to the device tolerance; against
        # the same path on the gathered copy under an identity mask everything is equal bit for bit.
        ident = _dev(np.arange(32), I32)
        got = []
        for src, dx, mk in ((s, 36, mask), (xm, 32, ident)):
            cs_m = guarded((3, 32), F64)
            d_m, r_m = guarded(5000, F32), guarded(5000, F32)
            rc = L.oly_disc_reward_step_pair(h, 5000, dx, 32, ptr(src), ptr(mk), None, ptr(cs_m.t), None, 0, None, ptr(packed),
                                             ptr(noise), ptr(r_m.t), ptr(d_m.t), None, None, eng._s())
            assert rc == 0
            torch.cuda.synchronize()
            assert sh.all_intact(dict(cs=cs_m, d=d_m, r=r_m)) == []
            got.append((cs_m.t, d_m.t, r_m.t))
        for a, b in zip(*got):
            assert torch.equal(a, b)
        cs_m, d_m, r_m = got[0]
        assert float(cs_m[0, 0]) == 5000.0
        e_cs = float((cs_m - cs_old).abs().max())
        e_d = pr.rel(d_m.cpu().numpy(), old["logits"].cpu().numpy())
        print(f"masked states only: statistics differ by {e_cs:.3e}, logits rel {e_d:.3e}")
        np.testing.assert_allclose(cs_m.cpu().numpy(), cs_old.cpu().numpy(), rtol=1e-12, atol=1e-9)
        assert e_d <= TOL
        # |dr / dd| = sigmoid(d) <= 1, plus the float32 steps of the reward formula (as in the fixture test above)
        d_old = old["logits"].cpu().numpy()
        assert (np.abs(r_m.cpu().numpy() - old["reward"].cpu().numpy()) <= TOL * (1 + np.abs(d_old)) + 2e-6).all()
    # the forward on given statistics
    d2n = torch.empty(5000, device="cuda")
    if algo == "gail":
        o = eng.gail_disc_forward(s, packed, mask=mask, colstats=cs_old, want=("logits",))
        rc = L.oly_gail_disc_forward_pair(h, 5000, 36, 32, ptr(s), ptr(mask), None, ptr(cs_old), None, ptr(packed), None,
                                          ptr(d2n), eng._s())
    else:
        o = eng.disc_forward(s, packed, mask=mask, colstats=cs_old, eps=noise, want=("logits",))
        rc = L.oly_disc_forward_pair(h, 5000, 36, 32, ptr(s), ptr(mask), None, ptr(cs_old), None, ptr(packed), ptr(noise),
                                     None, ptr(d2n), None, None, eng._s())
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(o["logits"], d2n)
    # the fit: the existing call (which now forwards) against the paired one with a NULL second part
    n, batch = 1300, 512
    x = xm[:n].contiguous()
    perm = torch.randperm(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)).to(I32)
    flat = torch.cat([p.reshape(-1) for p in params]).contiguous()
    res = []
    for new in (False, True):
        p_, m_, v_ = flat.clone(), torch.zeros_like(flat), torch.zeros_like(flat)
        cs = eng.col_stats(x)
        pk = packed.clone()
        loss = torch.zeros(3, dtype=F64, device="cuda")
        if algo == "gail":
            ws = eng.gail_disc_fit_ws(batch, 32)
            f = _abi.GailDiscFit(in_dim=32, n_plcy=600, step=0, lr=1e-3, beta1=0.9, beta2=0.999, adam_eps=1e-8,
                                 weight_decay=0.0, entcoeff=1e-3, x=x.data_ptr(), colstats=cs.data_ptr(), param=p_.data_ptr(),
                                 exp_avg=m_.data_ptr(), exp_avg_sq=v_.data_ptr(), packed=pk.data_ptr(), ws=ws.data_ptr(),
                                 ws_floats=ws.numel(), loss_out=loss.data_ptr())
            rc = (L.oly_gail_disc_fit_epoch_pair(h, C.byref(f), None, ptr(perm), n, batch, eng._s()) if new else
                  L.oly_gail_disc_fit_epoch(h, C.byref(f), ptr(perm), n, batch, eng._s()))
            keep = (ws,)
        else:
            ws = eng.disc_fit_ws(batch, 32)
            beta = torch.full((1,), 0.1, device="cuda")
            nz = noise[:n].contiguous()
            f = _abi.DiscFit(in_dim=32, n_plcy=600, step=0, lr=1e-3, beta1=0.9, beta2=0.999, adam_eps=1e-8, weight_decay=0.0,
                             info_constraint=0.1, lr_beta=1e-3, x=x.data_ptr(), eps=nz.data_ptr(), colstats=cs.data_ptr(),
                             param=p_.data_ptr(), exp_avg=m_.data_ptr(), exp_avg_sq=v_.data_ptr(), packed=pk.data_ptr(),
                             beta=beta.data_ptr(), ws=ws.data_ptr(), ws_floats=ws.numel(), loss_out=loss.data_ptr())
            rc = (L.oly_disc_fit_epoch_pair(h, C.byref(f), None, ptr(perm), n, batch, eng._s()) if new else
                  L.oly_disc_fit_epoch(h, C.byref(f), ptr(perm), n, batch, eng._s()))
            keep = (ws, beta, nz)
        assert rc == 0
        torch.cuda.synchronize()
        res.append((p_, m_, v_, cs, pk, loss, keep))
    for a, b in zip(res[0][:6], res[1][:6]):
        assert torch.equal(a, b)
    assert not torch.equal(res[0][0], flat)


# ------------------------------------------------------------------------------ trainers and agents
OBS, ACT = 36, 13
ACT_MASK = np.array([i for i in range(ACT) if i not in (2, 9)])


def _trainer(eng, algo, mode, seed, demo_as="dict", **kw):
    from olympic_hip.gail import (DiscriminatorReward, GAILDiscriminator, GAILDiscriminatorReward, VariationalDiscriminator,
                                  VDBLoss)
    from olympic_hip.il_agent import DeviceDiscriminatorTrainer, DeviceGAILDiscriminatorTrainer
    torch.manual_seed(seed)
    ns = mode == "next_state"
    dim = 64 if ns else 32 + len(ACT_MASK)
    rng = np.random.default_rng(seed)
    demo = dict(states=rng.normal(0.2, 1.0, (3000, OBS)).astype(np.float32))
    if ns:
        demo["next_states"] = (0.6 * demo["states"] + 1.0 + rng.normal(0, 0.5, (3000, OBS))).astype(np.float32)
    else:
        demo["actions"] = rng.normal(0.1, 0.7, (3000, ACT)).astype(np.float32)
    mk = dict(state_mask=np.arange(2, 34), pair=mode, act_mask=None if ns else ACT_MASK)
    args = dict(batch_size=1024, lr=5e-5)
    args.update(kw)
    if algo == "gail":
        r = GAILDiscriminatorReward(eng, GAILDiscriminator(dim).cuda(), **mk)
        return r, DeviceGAILDiscriminatorTrainer(r, demo, **args), demo
    r = DiscriminatorReward(eng, VariationalDiscriminator(in_dim=dim).cuda(), **mk)
    return r, DeviceDiscriminatorTrainer(r, demo, VDBLoss(0.1, 1e-3), **args), demo


def _policy(n, seed, mode):
    g = torch.Generator(device="cuda").manual_seed(seed)
    s = torch.randn((n, OBS), device="cuda", generator=g)
    x2 = (0.6 * s + 1.0 + 0.5 * torch.randn((n, OBS), device="cuda", generator=g) if mode == "next_state"
          else torch.randn((n, ACT), device="cuda", generator=g))
    return s.contiguous(), x2.contiguous()


@pytest.mark.parametrize("algo", ["gail", "vail"])
@pytest.mark.parametrize("mode", ["next_state", "action"])
def test_trainer_steps_the_module_in_place_and_matches_the_engine(eng, algo, mode):
    """The fit equals the engine call on the same draws (demo rows of both parts from ONE draw, then perm, then VAIL's
    noise); the module is stepped in place and the reward then uses the fitted weights."""
    ns = mode == "next_state"
    r, tr, demo = _trainer(eng, algo, mode, 4, batch_size=512)
    r2, _, _ = _trainer(eng, algo, mode, 4, batch_size=512)
    n = 700
    plcy, plcy2 = _policy(n, 3, mode)
    ptrs = [p.data_ptr() for p in r._params()]
    before = [p.detach().clone() for p in r._params()]
    losses = tr.fit(plcy, generator=torch.Generator(device="cuda").manual_seed(9), x2=plcy2)
    torch.cuda.synchronize()
    assert losses.shape == (1, 3) and torch.isfinite(losses).all() and tr.step == 3
    assert [p.data_ptr() for p in r._params()] == ptrs
    assert all(not torch.equal(a, b.detach()) for a, b in zip(before, r._params()))
    assert torch.equal(r._packed, pack(eng, algo, [p.detach() for p in r._params()]))
    # ---- by hand
    g = torch.Generator(device="cuda").manual_seed(9)
    idx = torch.randperm(3000, generator=g, device="cuda")[:n]
    m2 = torch.arange(2, 34, device="cuda") if ns else torch.as_tensor(ACT_MASK, device="cuda")
    x = torch.cat([plcy[:, 2:34], _dev(demo["states"], F32)[idx][:, 2:34]]).contiguous()
    xb = torch.cat([plcy2[:, m2], _dev(demo["next_states" if ns else "actions"], F32)[idx][:, m2]]).contiguous()
    perm = torch.randperm(2 * n, generator=g, device="cuda").to(I32)
    param = torch.cat([p.detach().reshape(-1) for p in r2._params()]).contiguous()
    cs = eng.col_stats(x)
    zeros = (torch.zeros_like(param), torch.zeros_like(param))
    if algo == "gail":
        want = eng.gail_disc_fit_epoch_pair(x, xb, ns, n, perm, 512, cs, param, *zeros, r2.packed(),
                                            eng.gail_disc_fit_pair_ws(512, 32, int(m2.numel()), ns), 0, 5e-5)
    else:
        noise = torch.randn((2 * n, 128), device="cuda", generator=g)
        want = eng.disc_fit_epoch_pair(x, xb, ns, n, noise, perm, 512, cs, param, *zeros, r2.packed(),
                                       torch.full((1,), 0.1, device="cuda"),
                                       eng.disc_fit_pair_ws(512, 32, int(m2.numel()), ns), 0, 5e-5, info_constraint=0.1,
                                       lr_beta=1e-3)
    torch.cuda.synchronize()
    assert torch.equal(losses[0], want)
    assert torch.equal(torch.cat([p.detach().reshape(-1) for p in r._params()]), param)
    assert torch.equal(r.stand.colstats, cs)
    assert float(cs[0, 0]) == 2 * n * (3 if ns else 2)
    # ---- the reward uses the fitted weights and updates the statistics once or twice
    s, s2 = _policy(900, 5, mode)
    eps = torch.randn((900, 128), device="cuda")
    got = r(s, eps, x2=s2).clone()
    assert float(r.stand.colstats[0, 0]) - float(cs[0, 0]) == 900 * (2 if ns else 1)
    d64, r64, _ = pr.restate_reward(algo, [p.detach() for p in r._params()], cs, s[:, 2:34], s2[:, m2], ns,
                                    noise=None if algo == "gail" else eps, device="cuda")
    assert (np.abs(got.cpu().numpy() - r64.cpu().numpy()) <= TOL * (1 + np.abs(d64.cpu().numpy())) + 2e-6).all()
    # predict: the same statistics for both halves, nothing updated
    c0 = r.stand.colstats.clone()
    o = r.predict(s, x2=s2) if algo == "gail" else r.predict(s, eps, x2=s2)
    assert torch.equal(r.stand.colstats, c0) and torch.isfinite(o["logits"]).all()


def test_the_prepared_paired_reward_equals_forward(eng):
    r, _, _ = _trainer(eng, "vail", "next_state", 6)
    r2, _, _ = _trainer(eng, "vail", "next_state", 6)
    s, s2 = _policy(4096, 7, "next_state")
    eps = torch.randn((4096, 128), device="cuda")
    step = r.prepared(s, eps, want=("reward", "logits"), x2=s2)
    for _ in range(2):
        a = {k: v.clone() for k, v in step().items()}
        b = r2.forward(s, eps, want=("reward", "logits"), x2=s2)
        assert torch.equal(a["reward"], b["reward"]) and torch.equal(a["logits"], b["logits"])
        assert torch.equal(r.stand.colstats, r2.stand.colstats)
    assert float(r.stand.colstats[0, 0]) == 4 * 4096


@pytest.mark.parametrize("algo", ["gail", "vail"])
@pytest.mark.parametrize("mode", ["next_state", "action"])
def test_agent_fit_with_a_paired_reward_equals_the_sequence_by_hand(eng, algo, mode):
    from olympic_hip.gail import DeviceStandardizer
    from olympic_hip.il_agent import DeviceILCritic, GAILAgent, VAILAgent
    T, N = 20, 100

    def parts(seed):
        r, tr, _ = _trainer(eng, algo, mode, seed, batch_size=512)
        torch.manual_seed(seed + 1)
        lins = [torch.nn.Linear(OBS, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 1)]
        return r, tr, DeviceILCritic(eng, lins, DeviceStandardizer(eng, OBS))
    ra, ta, ca = parts(7)
    rb, tb, cb = parts(7)
    agent = (GAILAgent if algo == "gail" else VAILAgent)(eng, ra, ta, ca, lambda o, a, adv, ag: None, train_D_n_th_epoch=2)
    for call in range(2):
        g = torch.Generator(device="cuda").manual_seed(call)
        s = torch.randn((T + 1, N, OBS), device="cuda", generator=g)
        last = torch.zeros((T, N), dtype=torch.bool, device="cuda")
        last[-1] = True
        ds = dict(state=s[:-1].contiguous(), action=torch.randn((T, N, ACT), device="cuda", generator=g),
                  reward=torch.randn((T, N), device="cuda", generator=g), next_state=s[1:].contiguous(),
                  absorbing=torch.zeros((T, N), dtype=torch.bool, device="cuda"), last=last)
        out = agent.fit(ds, generator=torch.Generator(device="cuda").manual_seed(10 + call))
        # ---- by hand: the agent's steps with the reward and the trainer called directly (gail_TRPO.py:105-165)
        gb = torch.Generator(device="cuda").manual_seed(10 + call)
        flat = ds["state"].reshape(T * N, OBS)
        second = (ds["next_state"].reshape(T * N, OBS) if mode == "next_state" else ds["action"].reshape(T * N, ACT)).contiguous()
        cb.stand.update_mean_std(flat)
        r_disc = rb(flat, None, generator=gb, x2=second)
        cb(flat)
        cb(ds["next_state"].reshape(T * N, OBS).contiguous())
        for _ in range(3):
            cb.stand.update_mean_std(flat)
        cb.fit(flat, out["v_target"].reshape(-1), n_epochs=3, batch_size=256, generator=gb)
        disc_loss = tb.fit(flat, generator=gb, x2=second) if call == 1 else None
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
    from olympic_hip.gail import GAILDiscriminator, GAILDiscriminatorReward
    from olympic_hip.il_agent import DeviceGAILDiscriminatorTrainer
    r, tr, demo = _trainer(eng, "gail", "next_state", 3)
    before = [p.detach().clone() for p in r._params()]
    s, s2 = _policy(100, 1, "next_state")
    with pytest.raises(OlyError):                 # the second tensor is missing
        tr.fit(s)
    with pytest.raises(OlyError):
        r(s)
    with pytest.raises(OlyError):                 # a mask that reads past the source's columns
        r(s, x2=s2[:, :30].contiguous())
    with pytest.raises(OlyError):
        tr.fit(s, x2=s2[:, :30].contiguous())
    with pytest.raises(OlyError):                 # demonstrations that lack the second array
        DeviceGAILDiscriminatorTrainer(r, dict(states=demo["states"]))
    with pytest.raises(OlyError):
        DeviceGAILDiscriminatorTrainer(r, dict(states=demo["states"], actions=np.zeros((3000, ACT), np.float32)))
    with pytest.raises(OlyError):                 # an array has no second part
        DeviceGAILDiscriminatorTrainer(r, demo["states"])
    with pytest.raises(OlyError):                 # the three-part combination
        GAILDiscriminatorReward(eng, GAILDiscriminator(64).cuda(), state_mask=np.arange(32), pair="next_state",
                                act_mask=np.arange(3))
    # the engine: bad shapes never reach a launch
    cs = torch.zeros((3, 32), dtype=F64, device="cuda")
    sa = torch.zeros((3, 32), dtype=F64, device="cuda")
    packed = r.packed()
    p0 = packed.clone()
    out = dict(reward=torch.full((100,), -3.0, device="cuda"))
    mask = _dev(np.arange(2, 34), I32)
    for bad in (dict(x2=torch.zeros((100, 0), device="cuda"), mask2=None),                      # D2 == 0
                dict(x2=torch.zeros((100, 33), device="cuda"), mask2=None),                    # D > 64
                dict(x2=s2, mask2=_dev(np.arange(31), I32)),                                   # next states narrower than the states
                dict(x2=s2[:50].contiguous()),                                                 # rows differ
                dict(x2=s2.double())):
        a = dict(x2=s2, mask2=mask)
        a.update(bad)
        with pytest.raises(OlyError):
            eng.gail_reward_step_pair(s, a["x2"], packed, cs, sa, False, True, mask=mask, mask2=a["mask2"], out=out)
        with pytest.raises(OlyError):
            eng.gail_disc_forward_pair(s, a["x2"], packed, True, mask=mask, mask2=a["mask2"], stats_a=cs, stats_b=cs, out=out)
    with pytest.raises(OlyError):                 # S1's scratch block is required with next states
        eng.gail_reward_step_pair(s, s2, packed, cs, None, False, True, mask=mask, mask2=mask, out=out)
    # the C entry points themselves refuse with OLY_EINVAL before any launch
    from olympic_hip import _abi, _ffi
    from olympic_hip.engine import ptr
    import ctypes as C
    L = _ffi.lib()
    for d2, std, stride in ((0, 1, 36), (33, 0, 36), (31, 1, 36), (32, 1, 0)):
        pair = _abi.DiscPair(x2=s2.data_ptr(), mask2=mask.data_ptr(), stride2=stride, d2=d2, standardise=std)
        rc = L.oly_gail_reward_step_pair(eng.ctx.handle, 100, 36, 32, ptr(s), ptr(mask), C.byref(pair), ptr(cs), ptr(sa), 0, None,
                                         ptr(packed), ptr(out["reward"]), None, None)
        assert rc == _abi.OLY_EINVAL, (d2, std, stride, rc)
        rc = L.oly_disc_forward_pair(eng.ctx.handle, 100, 36, 32, ptr(s), ptr(mask), C.byref(pair), ptr(cs), ptr(cs), ptr(packed),
                                     None, ptr(out["reward"]), None, None, None, None)
        assert rc == _abi.OLY_EINVAL, (d2, std, stride, rc)
    torch.cuda.synchronize()
    assert bool((cs == 0).all()) and bool((sa == 0).all()) and torch.equal(packed, p0) and bool((out["reward"] == -3.0).all())
    assert all(torch.equal(a, b.detach()) for a, b in zip(before, r._params()))


def test_refusals_of_statistics_blocks_standardizers_and_trainers(eng):
    """One statistics block without the other, S1's scratch block aliasing the running sums, a standardizer that is no
    DeviceStandardizer, and an agent whose trainer cannot fit a paired reward: each refused before any launch."""
    import ctypes as C
    from olympic_hip import _abi, _ffi
    from olympic_hip._ffi import OlyError
    from olympic_hip.engine import ptr
    from olympic_hip.gail import (DeviceStandardizer, DiscriminatorReward, DiscriminatorTrainer, GAILDiscriminator,
                                  GAILDiscriminatorReward, VariationalDiscriminator, VDBLoss)
    from olympic_hip.il_agent import DeviceILCritic, GAILAgent, VAILAgent
    L, h = _ffi.lib(), eng.ctx.handle
    s, s2 = _policy(100, 1, "next_state")
    mask = _dev(np.arange(2, 34), I32)
    cs = torch.zeros((3, 32), dtype=F64, device="cuda")
    sa = torch.zeros((3, 32), dtype=F64, device="cuda")
    out = torch.full((100,), -3.0, device="cuda")
    pair = _abi.DiscPair(x2=s2.data_ptr(), mask2=mask.data_ptr(), stride2=OBS, d2=32, standardise=1)
    for algo in ("gail", "vail"):
        params = [_dev(p, F32) for p in (gen.gail_init(64, seed=4) if algo == "gail" else sh.disc_params(64, 4))]
        packed = pack(eng, algo, params)
        p0 = packed.clone()
        for a, b in ((None, cs), (cs, None)):         # one block alone
            if algo == "gail":
                rc = L.oly_gail_disc_forward_pair(h, 100, OBS, 32, ptr(s), ptr(mask), C.byref(pair), ptr(a), ptr(b), ptr(packed),
                                                  ptr(out), None, eng._s())
            else:
                rc = L.oly_disc_forward_pair(h, 100, OBS, 32, ptr(s), ptr(mask), C.byref(pair), ptr(a), ptr(b), ptr(packed), None,
                                             ptr(out), None, None, None, eng._s())
            assert rc == _abi.OLY_EINVAL, (algo, a is None, rc)
        # S1's scratch block must not be the running sums themselves
        if algo == "gail":
            rc = L.oly_gail_reward_step_pair(h, 100, OBS, 32, ptr(s), ptr(mask), C.byref(pair), ptr(cs), ptr(cs), 0, None,
                                             ptr(packed), ptr(out), None, eng._s())
        else:
            rc = L.oly_disc_reward_step_pair(h, 100, OBS, 32, ptr(s), ptr(mask), C.byref(pair), ptr(cs), ptr(cs), 0, None,
                                             ptr(packed), None, ptr(out), None, None, None, eng._s())
        assert rc == _abi.OLY_EINVAL, (algo, rc)
        torch.cuda.synchronize()
        assert bool((cs == 0).all()) and bool((out == -3.0).all()) and torch.equal(packed, p0)

    class HostStandardizer:                             # the right shape, but not the device class
        colstats = sa
    for cls, net in ((GAILDiscriminatorReward, GAILDiscriminator(64)), (DiscriminatorReward, VariationalDiscriminator(64))):
        with pytest.raises(OlyError):
            cls(eng, net.cuda(), state_mask=np.arange(2, 34), pair="next_state", standardizer=HostStandardizer())
    # the torch DiscriminatorTrainer fits states only: an agent with a paired reward refuses it at construction
    lins = [torch.nn.Linear(OBS, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 1)]
    critic = DeviceILCritic(eng, lins, DeviceStandardizer(eng, OBS))
    r = DiscriminatorReward(eng, VariationalDiscriminator(64).cuda(), state_mask=np.arange(2, 34), pair="next_state")
    demo = np.zeros((10, OBS), np.float32)
    torch_trainer = DiscriminatorTrainer(r, demo, loss=VDBLoss(0.5, 1e-4))
    with pytest.raises(OlyError):
        VAILAgent(eng, r, torch_trainer, critic, lambda o, a, adv, ag: None)
    rg = GAILDiscriminatorReward(eng, GAILDiscriminator(64).cuda(), state_mask=np.arange(2, 34), pair="next_state")
    with pytest.raises(OlyError):
        GAILAgent(eng, rg, object(), critic, lambda o, a, adv, ag: None)
