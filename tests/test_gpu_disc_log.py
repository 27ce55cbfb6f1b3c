"""K19 on the GPU: the discriminator's diagnostics (oly_gail_disc_log, oly_disc_log) against the reference-run fixtures of
tests/golden/disc_log/ and the float64 restatement of tests/disc_log_restate.py, through the C entry points, the trainers'
fit(log=True) and the agents' writer.

Tolerances: tests/test_disc_log_cpu.py measures the float32-fixture-versus-float64 spread of every scalar below a tenth of
2e-5, so the device tolerance is the project's 2e-5 relative to max(1, |value|) throughout (rs.tolerances states the
rule).  The two accuracies are step functions of the logits: they are compared exactly wherever no float64 logit of the
restatement lies within 1e-4 of zero (true of every fixture), and otherwise may differ by the rows inside that band."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import disc_log_restate as rs
from il_shapes import guarded

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
gen = None


@pytest.fixture(scope="module")
def eng():
    from olympic_hip.engine import Engine
    e = Engine(0)
    yield e
    torch.cuda.synchronize()
    e.ctx.close()
    gc.collect()


def _gen():
    global gen
    if gen is None:
        rs.load_case("gail_s")
        import gen_disc_log
        gen = gen_disc_log
    return gen


def _dev(a, dtype=None):
    t = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
    return t.to(device="cuda", dtype=dtype).contiguous()


def pack(eng, algo, params):
    return (eng.ilmlp_pack if algo == "gail" else eng.disc_pack)(*[_dev(p, F32) for p in params])


def device_log(eng, a, ws=None, bufs=None):
    """restate_log's arguments through the engine's call (one C call) -> (scalars [12], colstats [3,Ds]) as numpy.  bufs:
    a dict that receives the guarded buffers."""
    n = a["x"].shape[0]
    cs = guarded((3, a["x"].shape[1]), F64, init=a["colstats"])
    out = guarded(12, F64, init=np.full(12, 7.0))
    need = eng.gail_disc_log_ws(n) if a["algo"] == "gail" else eng.disc_log_ws(n)
    wsg = guarded(int(need.numel()), F32) if ws is None else None
    kw = dict(x2=None if a["x2"] is None else _dev(a["x2"], F32), standardise=a["pair"] == "next_state",
              targets=None if a["targets"] is None else _dev(a["targets"], F32), out=out.t, entcoeff=a["entcoeff"])
    packed = pack(eng, a["algo"], a["params"])
    if a["algo"] == "gail":
        eng.gail_disc_log(_dev(a["x"], F32), a["n_plcy"], cs.t, packed, wsg.t if ws is None else ws, **kw)
    else:
        eps = None if a["noise"] is None else _dev(np.concatenate(a["noise"]), F32)
        eng.disc_log(_dev(a["x"], F32), a["n_plcy"], cs.t, packed, _dev(np.array([a["beta"]]), F32),
                     wsg.t if ws is None else ws, info_constraint=a["info_c"], lr_beta=a["lr_beta"], eps=eps, **kw)
    torch.cuda.synchronize()
    if bufs is not None:
        bufs.update(cs=cs, out=out, **({} if wsg is None else dict(ws=wsg)))
    return out.t.cpu().numpy().copy(), cs.t.cpu().numpy().copy()


def check_scalars(got, want, logits, n_plcy, label=""):
    """got against float64 `want`: 2e-5 relative to max(1, |value|); accuracies exact up to the rows inside the band."""
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    for name, g, w, e in zip(rs.NAMES, got, want, err):
        print(f"{label:28s} {name:48s} device {g:+.9e} float64 {w:+.9e} err {e:.2e}")
    for i, k in ((1, 2), (3, 1)):
        d = logits[k]
        assert abs(got[i] - want[i]) <= (np.sum(np.abs(d) < rs.BAND) + 1e-9) / len(d), (rs.NAMES[i], got[i], want[i])
    rest = [i for i in range(12) if i not in rs.ACCURACIES]
    assert np.all(err[rest] <= rs.TOL), {rs.NAMES[i]: err[i] for i in rest if err[i] > rs.TOL}


# ------------------------------------------------------------------------------ the fixtures, through the C entry points
@pytest.mark.parametrize("case", rs.CASES)
def test_fixture_through_the_entry_point(eng, case):
    a, g = rs.load_case(case)
    bufs = {}
    got, cs = device_log(eng, a, bufs=bufs)
    assert not [k for k, b in bufs.items() if not b.intact()]
    want = np.zeros(12)
    want[:len(g["values"])] = g["values"]
    ref = rs.restate_log(**a)
    spread = np.abs(ref["scalars"] - want) / np.maximum(1.0, np.abs(want))
    tol = rs.tolerances(spread)
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    for name, x, w, e, t in zip(rs.NAMES, got, want, err, tol):
        print(f"{case:8s} {name:48s} device {x:+.9e} fixture {w:+.9e} err {e:.2e} tol {t:.1e}")
    assert np.all(tol == rs.TOL)
    assert np.all(err <= tol)
    for i in rs.ACCURACIES:
        assert got[i] == want[i]
    if case.startswith("gail"):
        assert np.all(got[9:] == 0)
    # the live statistics end where the reference's Standardizer does
    assert cs[0, 0] + 1e-2 == pytest.approx(float(g["st_count"][0]), rel=1e-12) and np.all(cs[0] == cs[0, 0])
    assert np.all(np.abs(cs[1] - g["st_sum"]) <= rs.TOL * np.maximum(1, np.abs(g["st_sum"])))
    assert np.all(np.abs(cs[2] + 1e-2 - g["st_sumsq"]) <= rs.TOL * np.maximum(1, np.abs(g["st_sumsq"])))
    assert np.all(np.abs(cs - ref["colstats"]) <= 1e-12 * np.maximum(1, np.abs(ref["colstats"])))
    # two runs are bit-identical
    got2, cs2 = device_log(eng, a)
    assert np.array_equal(got, got2) and np.array_equal(cs, cs2)


# ------------------------------------------------------------------------------ shapes where the kernels can go wrong
#        algo    Ds  D2 pair          n_plcy n_demo targets
SHAPES = (("gail", 1, 0, None, 1, 1, False),                    # one column, one row in each half
          ("vail", 1, 0, None, 33, 20, False),
          ("gail", 17, 0, None, 33, 20, True),
          ("vail", 17, 0, None, 257, 257, False),               # 257: a partial reduction block after a full one
          ("gail", 64, 0, None, 257, 130, False),
          ("vail", 64, 0, None, 1, 1, True),
          ("gail", 32, 32, "next_state", 257, 100, False),      # the 64-column limit, two statistics blocks per forward
          ("vail", 32, 32, "next_state", 33, 20, False),
          ("vail", 20, 7, "action", 257, 31, True),
          ("gail", 32, 0, None, 16385, 40, False),              # two chunks, the last of one row (policy half and all rows)
          ("vail", 17, 0, None, 40, 16385, False))              # the same in the demonstration half


def shape_case(algo, ds, d2, pair, n_plcy, n_demo, targets, seed):
    g = _gen()
    rng = np.random.default_rng(seed)
    n = n_plcy + n_demo
    scale, shift = rng.uniform(0.3, 3.0, ds), rng.normal(0, 2, ds)
    x = (np.concatenate([rng.normal(0, 1, (n_plcy, ds)), rng.normal(0.4, 1.2, (n_demo, ds))]) * scale + shift).astype(np.float32)
    x2 = None
    if pair == "next_state":
        x2 = (0.6 * x + 1.5 * scale + rng.normal(0, 0.5, (n, ds)) * scale).astype(np.float32)
    elif pair == "action":
        x2 = rng.normal(0.1, 0.8, (n, d2)).astype(np.float32)
    st = rs.Stats(1e-2, np.zeros(ds), np.full(ds, 1e-2))
    st.add((rng.normal(1.0, 1.0, (500, ds)) * scale * 1.5 + shift).astype(np.float32))
    t = None
    if targets:
        t = np.concatenate([rng.uniform(0.01, 0.10, n_plcy), rng.uniform(0.80, 0.99, n_demo)]).astype(np.float32)
    in_dim = ds + d2
    params = g.gp.gail_init(in_dim, seed) if algo == "gail" else g.vail_params(in_dim, seed)
    noise = None
    if algo == "vail":
        noise = [rng.standard_normal((r, 128)).astype(np.float32) for r in (n, n_demo, n_plcy) * 2]
    return dict(algo=algo, params=params, colstats=st.colstats(), x=x, n_plcy=n_plcy, x2=x2, pair=pair, targets=t,
                entcoeff=0.02, beta=0.2, info_c=0.4, lr_beta=4e-3, noise=noise)


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{s[0]}-{s[1]}+{s[2]}-p{s[4]}d{s[5]}" for s in SHAPES])
def test_shapes_against_the_restatement(eng, shape):
    a = shape_case(*shape, seed=11 + SHAPES.index(shape))
    bufs = {}
    got, cs = device_log(eng, a, bufs=bufs)
    assert not [k for k, b in bufs.items() if not b.intact()]
    ref = rs.restate_log(device="cuda", **a)
    check_scalars(got, ref["scalars"], ref["logits"], a["n_plcy"], label="-".join(str(v) for v in shape[:6]))
    assert np.all(np.abs(cs - ref["colstats"]) <= 1e-12 * np.maximum(1, np.abs(ref["colstats"])))
    k = (5 if shape[0] == "vail" else 4) * (2 if shape[3] == "next_state" else 1)
    assert cs[0, 0] - a["colstats"][0, 0] == k * a["x"].shape[0]


def test_z_equals_mu_without_noise(eng):
    a = shape_case("vail", 17, 0, None, 33, 20, False, seed=5)
    a["noise"] = None
    got, _ = device_log(eng, a)
    ref = rs.restate_log(**a)
    check_scalars(got, ref["scalars"], ref["logits"], a["n_plcy"], label="eps NULL")


def test_a_larger_workspace_is_reused(eng):
    for algo in ("gail", "vail"):
        a = shape_case(algo, 17, 0, None, 200, 100, False, seed=3)
        big = eng.gail_disc_log_ws(4096) if algo == "gail" else eng.disc_log_ws(4096)
        big.fill_(float("nan"))
        got, cs = device_log(eng, a, ws=big)
        want, cs2 = device_log(eng, a)
        assert np.array_equal(got, want) and np.array_equal(cs, cs2)


# ------------------------------------------------------------------------------ trainers
OBS, ACT = 34, 13


def _trainer(eng, case, seed=0, **kw):
    """A device trainer on the fixture's network, masks, demonstrations (the 640 drawn rows) and start statistics, with
    lr = 0 so that the minibatch loop leaves the weights where the fixture has them."""
    from olympic_hip.gail import (DiscriminatorReward, GAILDiscriminator, GAILDiscriminatorReward, VariationalDiscriminator,
                                  VDBLoss)
    from olympic_hip.il_agent import DeviceDiscriminatorTrainer, DeviceGAILDiscriminatorTrainer
    g = _gen()
    c = g.CASES[case]
    fx = np.load(rs.fixture(case))
    data = g.gp.inputs()
    idx = fx["demo_idx"]
    demo = dict(states=data["demo_states"][idx])
    if c["pair"] == "next_state":
        demo["next_states"] = data["demo_next_states"][idx]
    elif c["pair"] == "action":
        demo["actions"] = data["demo_actions"][idx]
    mk = dict(state_mask=g.gp.STATE_MASK)
    if c["pair"] is not None:
        mk.update(pair=c["pair"], act_mask=g.gp.ACT_MASK if c["pair"] == "action" else None)
    dim = sum(g.widths(case))
    args = dict(batch_size=512, lr=0.0, use_noisy_targets=c["noisy"])
    args.update(kw)
    torch.manual_seed(seed)
    if c["algo"] == "gail":
        r = GAILDiscriminatorReward(eng, GAILDiscriminator(dim).cuda(), **mk)
        tr = DeviceGAILDiscriminatorTrainer(r, demo if c["pair"] else demo["states"], entcoeff=c["entcoeff"], **args)
    else:
        r = DiscriminatorReward(eng, VariationalDiscriminator(in_dim=dim).cuda(), **mk)
        tr = DeviceDiscriminatorTrainer(r, demo if c["pair"] else demo["states"],
                                        VDBLoss(c["info_c"], c["lr_beta"], entcoeff=c["entcoeff"]), **args)
        tr.loss._beta = c["beta"]
    with torch.no_grad():
        for p, w in zip(r._params(), g.params(case, int(fx["param_seed"]))):
            p.copy_(_dev(w, F32))
    second = None if c["pair"] is None else _dev(data["plcy_next" if c["pair"] == "next_state" else "plcy_act"], F32)
    return r, tr, _dev(data["plcy_obs"], F32), second, fx


def _fit(tr, plcy, second, **kw):
    if second is not None:
        kw["x2"] = second
    return tr.fit(plcy, **kw)


@pytest.mark.parametrize("case", rs.CASES)
def test_trainer_fit_with_log(eng, case):
    """fit(log=True) on the fixture's network and rows.  The trainer draws its own demonstration order, targets and noise
    and its minibatch loop has moved the statistics (and VAIL's beta) before the diagnostics run, so the expected values
    are the restatement's on the replayed draws; for gail_s, where none of that reaches the scalars, the start statistics
    are set so that the diagnostics start from the fixture's, and the fixture's scalars and final statistics are
    asserted as well."""
    g = _gen()
    c = g.CASES[case]
    r, tr, plcy, second, fx = _trainer(eng, case)
    a, _ = rs.load_case(case)
    n = g.N_PLCY
    seed = 77
    # replay the draws: demo order, noisy targets (demo first), perm, VAIL's noise, then the diagnostics' noise
    gr = torch.Generator(device="cuda").manual_seed(seed)
    p = torch.randperm(n, generator=gr, device="cuda")[:n].cpu().numpy()
    x = np.concatenate([a["x"][:n], a["x"][n:][p]])
    x2 = None if a["x2"] is None else np.concatenate([a["x2"][:n], a["x2"][n:][p]])
    targets = None
    if c["noisy"]:
        demo_t = torch.empty(n, device="cuda").uniform_(0.80, 0.99, generator=gr)
        plcy_t = torch.empty(n, device="cuda").uniform_(0.01, 0.10, generator=gr)
        targets = torch.cat([plcy_t, demo_t]).cpu().numpy()
    torch.randperm(2 * n, generator=gr, device="cuda")
    noise = None
    if c["algo"] == "vail":
        torch.randn((2 * n, 128), device="cuda", generator=gr)
        leps = torch.randn((8 * n, 128), device="cuda", generator=gr).cpu().numpy()
        noise = [leps[o:o + k] for o, k in zip(np.cumsum([0, 2 * n, n, n, 2 * n, n]), (2 * n, n, n, 2 * n, n, n))]
    # the statistics the diagnostics start from: the start, the explicit update (:206), the minibatches' own updates
    k_fit = 3 if c["pair"] == "next_state" else 2
    sums = rs.Stats.from_colstats(np.zeros((3, 32)))
    for _ in range(2):
        sums.add(x)
    if c["pair"] == "next_state":
        sums.add(x2)
    start = a["colstats"] - sums.colstats() if case == "gail_s" else a["colstats"]
    r.stand.colstats = _dev(start, F64)
    r.stand._fresh = False
    losses, logs = _fit(tr, plcy, second, generator=torch.Generator(device="cuda").manual_seed(seed), log=True)
    torch.cuda.synchronize()
    assert logs.shape == (1, 12) and logs.dtype == F64 and losses.shape == (1, 3)
    for pp, w in zip(r._params(), a["params"]):
        assert torch.equal(pp.detach().cpu(), torch.as_tensor(w))                    # lr = 0: the fixture's weights
    s0 = rs.Stats.from_colstats(start)
    for _ in range(2):
        s0.add(x)
    if c["pair"] == "next_state":
        s0.add(x2)
    assert s0.count - 1e-2 - start[0, 0] == k_fit * 2 * n
    ref = rs.restate_log(**dict(a, x=x, x2=x2, targets=targets, noise=noise, colstats=s0.colstats(),
                                beta=float(tr.beta) if c["algo"] == "vail" else 0.0))
    got = logs[0].cpu().numpy()
    check_scalars(got, ref["scalars"], ref["logits"], n, label=f"trainer {case}")
    cs = r.stand.colstats.cpu().numpy()
    assert np.all(np.abs(cs - ref["colstats"]) <= 1e-9 * np.maximum(1, np.abs(ref["colstats"])))
    if case == "gail_s":
        want = np.zeros(12)
        want[:9] = fx["values"]
        assert np.all(np.abs(got - want) / np.maximum(1, np.abs(want)) <= rs.TOL)
        assert got[1] == want[1] and got[3] == want[3]
        assert np.all(np.abs(cs[1] - fx["st_sum"]) <= rs.TOL * np.maximum(1, np.abs(fx["st_sum"])))
        assert np.all(np.abs(cs[2] + 1e-2 - fx["st_sumsq"]) <= rs.TOL * np.maximum(1, np.abs(fx["st_sumsq"])))
    if c["algo"] == "vail":
        assert tr.loss._beta == float(tr.beta)                                       # the diagnostics leave beta alone


@pytest.mark.parametrize("case", ["gail_ns", "vail_s"])
def test_log_false_is_the_trainer_without_diagnostics(eng, case):
    """fit() and fit(log=False) against the engine's calls by hand (the sequence of a trainer that never heard of
    logging): losses, parameters and statistics bit for bit."""
    g = _gen()
    c = g.CASES[case]
    res = []
    for mode in ("default", "false", "hand"):
        r, tr, plcy, second, fx = _trainer(eng, case, lr=1e-4)
        gg = torch.Generator(device="cuda").manual_seed(5)
        if mode != "hand":
            out = _fit(tr, plcy, second, generator=gg, **({} if mode == "default" else dict(log=False)))
            assert torch.is_tensor(out)
            torch.cuda.synchronize()
            res.append((out.clone(), torch.cat([p.detach().reshape(-1) for p in r._params()]), r.stand.colstats.clone()))
            continue
        a, _ = rs.load_case(case)
        n = g.N_PLCY
        p = torch.randperm(n, generator=gg, device="cuda")[:n].cpu().numpy()
        x = _dev(np.concatenate([a["x"][:n], a["x"][n:][p]]), F32)
        perm = torch.randperm(2 * n, generator=gg, device="cuda").to(torch.int32)
        param = torch.cat([q.detach().reshape(-1) for q in r._params()]).contiguous()
        zeros = (torch.zeros_like(param), torch.zeros_like(param))
        cs = eng.col_stats(x)
        if c["algo"] == "gail":
            xb = _dev(np.concatenate([a["x2"][:n], a["x2"][n:][p]]), F32)
            want = eng.gail_disc_fit_epoch_pair(x, xb, True, n, perm, 512, cs, param, *zeros, r.packed(),
                                                eng.gail_disc_fit_pair_ws(512, 32, 32, True), 0, 1e-4, entcoeff=c["entcoeff"])
        else:
            noise = torch.randn((2 * n, 128), device="cuda", generator=gg)
            want = eng.disc_fit_epoch(x, n, noise, perm, 512, cs, param, *zeros, r.packed(),
                                      torch.full((1,), c["beta"], device="cuda"), eng.disc_fit_ws(512, 32), 0, 1e-4,
                                      info_constraint=c["info_c"], lr_beta=c["lr_beta"])
        torch.cuda.synchronize()
        res.append((want.reshape(1, -1).clone(), param, cs))
    for other in res[1:]:
        for u, v in zip(res[0], other):
            assert torch.equal(u, v)


@pytest.mark.parametrize("case", ["gail_s", "vail_sa"])
def test_two_epochs_equal_two_one_epoch_fits(eng, case):
    """The diagnostics run inside the epoch loop (gail_TRPO.py:220), so the second epoch starts from the statistics they
    left: n_epochs = 2 equals two fits of one epoch on one generator."""
    ra, ta, plcy, second, _ = _trainer(eng, case, lr=1e-4, n_epochs=2)
    rb, tb, _, _, _ = _trainer(eng, case, lr=1e-4, n_epochs=1)
    la, ga = _fit(ta, plcy, second, generator=torch.Generator(device="cuda").manual_seed(3), log=True)
    gb = torch.Generator(device="cuda").manual_seed(3)
    outs = [_fit(tb, plcy, second, generator=gb, log=True) for _ in range(2)]
    torch.cuda.synchronize()
    assert ga.shape == (2, 12)
    assert torch.equal(la, torch.cat([o[0] for o in outs])) and torch.equal(ga, torch.cat([o[1] for o in outs]))
    assert not torch.equal(ga[0], ga[1])
    assert torch.equal(ra.stand.colstats, rb.stand.colstats)
    for pa, pb in zip(ra._params(), rb._params()):
        assert torch.equal(pa, pb)
    # and the diagnostics did shift what the second epoch saw
    rc, tc, _, _, _ = _trainer(eng, case, lr=1e-4, n_epochs=2)
    lc = _fit(tc, plcy, second, generator=torch.Generator(device="cuda").manual_seed(3))
    assert torch.equal(lc[0], la[0]) and (not torch.equal(lc[1], la[1]) or case.startswith("vail"))


# ------------------------------------------------------------------------------ agents
class Recorder:
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, step):
        self.rows.append((tag, float(value), int(step)))


def _dataset(T, N, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    s = torch.randn((T + 1, N, OBS), device="cuda", generator=g)
    last = torch.zeros((T, N), dtype=torch.bool, device="cuda")
    last[-1] = True
    return dict(state=s[:-1].contiguous(), action=torch.randn((T, N, ACT), device="cuda", generator=g),
                reward=torch.randn((T, N), device="cuda", generator=g), next_state=s[1:].contiguous(),
                absorbing=torch.zeros((T, N), dtype=torch.bool, device="cuda"), last=last)


@pytest.mark.parametrize("case", ["gail_ns", "vail_s"])
def test_agent_writes_the_reference_s_tags(eng, case):
    from olympic_hip.gail import DeviceStandardizer
    from olympic_hip.il_agent import DISC_LOG_NAMES, DeviceILCritic, GAILAgent, VAILAgent
    algo = case[:4]
    names = DISC_LOG_NAMES[algo]
    assert names == rs.NAMES[:9 if algo == "gail" else 12]

    def agent(sw):
        r, tr, _, _, _ = _trainer(eng, case, lr=1e-4)
        torch.manual_seed(2)
        lins = [torch.nn.Linear(OBS, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 1)]
        critic = DeviceILCritic(eng, lins, DeviceStandardizer(eng, OBS))
        cls = GAILAgent if algo == "gail" else VAILAgent
        return cls(eng, r, tr, critic, lambda o, a, adv, ag: None, train_D_n_th_epoch=3, start_iter=5, sw=sw), r
    sw = Recorder()
    with_sw, r1 = agent(sw)
    without, r2 = agent(None)
    for call, it in enumerate((5, 6, 7)):
        ds = _dataset(8, 40, call)
        before = len(sw.rows)
        o1 = with_sw.fit(ds, generator=torch.Generator(device="cuda").manual_seed(call))
        o2 = without.fit(ds, generator=torch.Generator(device="cuda").manual_seed(call))
        assert "disc_log" not in o2 and set(o2) == {"reward", "v_target", "adv", "critic_loss", "disc_loss", "disc_trained"}
        assert o1["disc_trained"] == o2["disc_trained"] == (it % 3 == 0)
        if it % 3 != 0:
            assert "disc_log" not in o1 and len(sw.rows) == before
            continue
        assert [t for t, _, _ in sw.rows] == list(names)                               # the reference's tags in its order
        assert all(step == it // 3 for _, _, step in sw.rows)
        assert o1["disc_log"] == {t: v for t, v, _ in sw.rows}
        assert all(np.isfinite(v) for _, v, _ in sw.rows)
        assert 0.0 <= o1["disc_log"]["D_Expert_Accuracy"] <= 1.0
        assert torch.is_tensor(o1["disc_loss"]) and o1["disc_loss"].shape == o2["disc_loss"].shape
        # the diagnostics moved the discriminator's Standardizer four (five) batches further, twice with next states
        k = (5 if algo == "vail" else 4) * (2 if case.endswith("_ns") else 1)
        assert float(r1.stand.colstats[0, 0]) - float(r2.stand.colstats[0, 0]) == k * 2 * 320
    assert len(sw.rows) == len(names)


# ------------------------------------------------------------------------------ refusals
def test_refusals(eng):
    from olympic_hip import _abi
    from olympic_hip._ffi import OlyError, lib
    from olympic_hip.il_agent import GAILAgent
    a = shape_case("gail", 17, 0, None, 33, 20, False, seed=1)
    n = 53
    x, cs = _dev(a["x"], F32), _dev(a["colstats"], F64)
    packed = pack(eng, "gail", a["params"])
    ws = eng.gail_disc_log_ws(n)
    for bad in (0, n, -1, n + 1):
        with pytest.raises(OlyError):
            eng.gail_disc_log(x, bad, cs, packed, ws)
    with pytest.raises(OlyError):
        eng.gail_disc_log(x, 33, cs, packed, ws[:-1])
    with pytest.raises(OlyError):
        eng.disc_log_ws(1)
    # the C entry points themselves, before any launch: the outputs keep their sentinels
    out = guarded(12, F64, init=np.full(12, 7.0))
    keep = cs.clone()

    def call(n_plcy, ws_floats, in_dim=17):
        f = _abi.GailDiscLog(in_dim=in_dim, n_rows=n, n_plcy=n_plcy, entcoeff=1e-3, x=x.data_ptr(), targets=None,
                             colstats=cs.data_ptr(), packed=packed.data_ptr(), ws=ws.data_ptr(), ws_floats=ws_floats,
                             out=out.t.data_ptr())
        return lib().oly_gail_disc_log(eng.ctx.handle, C.byref(f), None, eng._s())
    full = int(ws.numel())
    assert call(0, full) == _abi.OLY_EINVAL and call(n, full) == _abi.OLY_EINVAL
    assert call(33, full - 1) == _abi.OLY_EINVAL and call(33, full, in_dim=65) == _abi.OLY_EINVAL
    av = shape_case("vail", 17, 0, None, 33, 20, False, seed=1)
    pv, wv, beta = pack(eng, "vail", av["params"]), eng.disc_log_ws(n), torch.full((1,), 0.1, device="cuda")
    for n_plcy, wsf in ((0, int(wv.numel())), (n, int(wv.numel())), (33, int(wv.numel()) - 1)):
        f = _abi.DiscLog(in_dim=17, n_rows=n, n_plcy=n_plcy, entcoeff=1e-3, info_constraint=0.1, lr_beta=1e-3,
                         x=x.data_ptr(), targets=None, eps=None, beta=beta.data_ptr(), colstats=cs.data_ptr(),
                         packed=pv.data_ptr(), ws=wv.data_ptr(), ws_floats=wsf, out=out.t.data_ptr())
        assert lib().oly_disc_log(eng.ctx.handle, C.byref(f), None, eng._s()) == _abi.OLY_EINVAL
    torch.cuda.synchronize()
    assert out.intact() and bool((out.t == 7.0).all()) and torch.equal(cs, keep)
    assert call(33, full) == _abi.OLY_OK
    torch.cuda.synchronize()
    assert not torch.equal(cs, keep) and out.intact()

    # a writer needs a trainer whose fit takes log=
    class OldTrainer:
        def fit(self, x, generator=None):
            return None
    r, tr, _, _, _ = _trainer(eng, "gail_s")
    with pytest.raises(OlyError, match="log"):
        GAILAgent(eng, r, OldTrainer(), None, lambda *k: None, sw=Recorder())
    with pytest.raises(OlyError, match="add_scalar"):
        GAILAgent(eng, r, tr, None, lambda *k: None, sw=object())
    GAILAgent(eng, r, OldTrainer(), None, lambda *k: None)                              # without a writer nothing is asked of it
