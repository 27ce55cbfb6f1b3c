"""K24 on the MI355X: oly_bc_fit_steps against the float64 restatement of tests/bc_restate.py at every case of its table
and against the reference-run fixture, its bits across runs and across the way a fit is cut into calls, oly_bc_targets,
DeviceSquashedGaussianPolicy, checkpoint / resume of DeviceBehavioralCloning, and examples/bc_fit.py."""
import gc
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bc_restate as br

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = br.TOL
NAMES = ("w1", "b1", "w2", "b2", "w3", "b3")
IDS = [br.case_id(c) for c in br.CASES]


@pytest.fixture(scope="module")
def eng():
    from olympic_hip.engine import Engine
    e = Engine(0)
    yield e
    torch.cuda.synchronize()
    e.ctx.close()
    gc.collect()


def d(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def split(flat, in_dim, A):
    out, o = [], 0
    for s in br.param_shapes(in_dim, A):
        n = int(np.prod(s))
        out.append(flat[o:o + n].reshape(s))
        o += n
    return out


def run_kernel(eng, c, k, cuts=None, lr=None):
    """The fit of case c on the device, cut into calls of `cuts` steps (None: one call).  Returns the device state."""
    A, b = c.A, k["batch"]
    param = d(br.flat(k["params"]).astype(np.float32))
    st = dict(param=param, m=torch.zeros_like(param), v=torch.zeros_like(param),
              colstats=torch.zeros((3, c.in_dim), dtype=torch.float64, device="cuda") if c.standardizer else None,
              out=torch.zeros((c.steps, 3), dtype=torch.float64, device="cuda"))
    st["packed"] = eng.ilmlp_pack(*split(param, c.in_dim, A))
    ws = eng.bc_fit_ws(b, c.in_dim, A)
    states, targets, idx = d(k["states"]), d(k["targets"]), d(k["idx"])
    s = 0
    for n in (cuts or (c.steps,)):
        eng.bc_fit_steps(states, targets, idx[s:s + n].contiguous(), st["colstats"], param, st["m"], st["v"], st["packed"],
                         ws, s, c.lr if lr is None else lr, log_std_min=br.LOG_STD_MIN, log_std_max=br.LOG_STD_MAX,
                         nll_eps=br.NLL_EPS, out=st["out"][s:s + n])
        s += n
    assert s == c.steps
    torch.cuda.synchronize()
    return st


def same_state(a, b):
    for key in ("param", "m", "v", "packed", "colstats", "out"):
        if a[key] is None:
            assert b[key] is None
        else:
            assert torch.equal(a[key], b[key]), key


# ------------------------------------------------------------------------------ against the float64 yardstick
@pytest.mark.parametrize("c", br.CASES, ids=IDS)
def test_fit_against_float64(eng, c):
    k, ref = br.yardstick(c)
    assert_fit_matches_float64(eng, c, run_kernel(eng, c, k), ref)


def assert_fit_matches_float64(eng, c, st, ref):
    """The device state `st` of case c after the fit (run_kernel's keys) against the float64 restatement `ref`."""
    got = [t.double().cpu().numpy() for t in split(st["param"], c.in_dim, c.A)]
    for name, a, r in zip(NAMES, got, ref["params"][-1]):
        err = float(np.abs(a - r).max())
        print(f"{br.case_id(c)} {name}: |kernel - f64| max {err:.3e}")
        assert err <= TOL, (name, err)
    for key, refs in (("m", ref["exp_avg"]), ("v", ref["exp_avg_sq"])):
        for name, a, r in zip(NAMES, split(st[key], c.in_dim, c.A), refs):
            err = float(np.abs(a.double().cpu().numpy() - r).max()) / max(float(np.abs(r).max()), 1e-300)
            print(f"{br.case_id(c)} {key} {name}: relative to the largest entry {err:.3e}")
            assert err <= TOL, (key, name, err)
    if c.standardizer:
        err = float(np.abs(st["colstats"].cpu().numpy() - ref["colstats"]).max())
        print(f"{br.case_id(c)} colstats: {err:.3e}")
        assert err <= TOL
    out = st["out"].cpu().numpy()
    rel = np.abs(out - ref["out"]) / np.abs(ref["out"])
    print(f"{br.case_id(c)} scalars: relative {rel.max(axis=0)}")
    assert rel.max() <= TOL, rel
    # the packed stream after the fit is ilmlp_pack of param
    assert torch.equal(st["packed"], eng.ilmlp_pack(*split(st["param"], c.in_dim, c.A)))


def test_fit_against_the_reference_run_fixture(eng, golden):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import gen_bc_fit as gen
    g = golden("bc_fit/bc_fit.npz")
    states, actions, min_a, max_a = gen.inputs()
    params = gen.initial_params(g)
    A, in_dim, steps = gen.ACT_DIM, gen.IN_DIM, gen.N_STEPS
    central, delta = (0.5 * (max_a + min_a)).astype(np.float32), (0.5 * (max_a - min_a)).astype(np.float32)
    targets = eng.bc_targets(d(actions), d(central), d(delta))
    param = d(br.flat(params).astype(np.float32))
    m, v = torch.zeros_like(param), torch.zeros_like(param)
    colstats = torch.zeros((3, in_dim), dtype=torch.float64, device="cuda")
    packed = eng.ilmlp_pack(*split(param, in_dim, A))
    ws = eng.bc_fit_ws(gen.BATCH, in_dim, A)
    idx = d(g["idx"].astype(np.int32))
    out = torch.zeros((steps, 3), dtype=torch.float64, device="cuda")
    done = 0
    for upto in gen.SNAPSHOTS:
        eng.bc_fit_steps(d(states), targets, idx[done:upto].contiguous(), colstats, param, m, v, packed, ws, done, gen.LR,
                         out=out[done:upto])
        done = upto
        got = split(param, in_dim, A)
        for i, name in enumerate(NAMES):
            if name == "w2":
                continue
            err = float(np.abs(got[i].cpu().numpy().astype(np.float64) - g[f"{name}_step{upto}"]).max())
            assert err <= TOL, (upto, name, err)
    rel = np.abs(out.cpu().numpy() - g["scalars"]) / np.abs(g["scalars"])
    assert rel.max() <= TOL, rel
    # The statistics.  The reference's Standardizer sums the float32 minibatch with numpy in float32 before it adds to its
    # float64 totals (networks.py:77-78), so its sums carry float32 rounding in proportion to their size; the kernel sums in
    # float64.  The count is exact; the sums within TOL of their own size, as the other fixture tests of the fits hold them.
    cs = colstats.cpu().numpy()
    assert np.all(cs[0] + 1e-2 == g["st_count"][0])
    assert np.all(np.abs(cs[1] - g["st_sum"]) <= TOL * np.maximum(1, np.abs(g["st_sum"])))
    assert np.all(np.abs(cs[2] + 1e-2 - g["st_sumsq"]) <= TOL * np.maximum(1, np.abs(g["st_sumsq"])))


# ------------------------------------------------------------------------------ bits
BITS = br.CASES[3]._replace(steps=6)       # 33 rows (16 + 16 + 1), 22 output columns, a Standardizer


def test_two_runs_give_the_same_bits_and_cuts_do_not_matter(eng):
    k = br.build(BITS)
    one = run_kernel(eng, BITS, k)
    same_state(one, run_kernel(eng, BITS, k))
    same_state(one, run_kernel(eng, BITS, k, cuts=(1,) * 6))
    same_state(one, run_kernel(eng, BITS, k, cuts=(2, 4)))
    assert torch.equal(one["packed"], eng.ilmlp_pack(*split(one["param"], BITS.in_dim, BITS.A)))
    assert float(one["out"][:, 0].abs().min()) > 0


def test_bits_without_a_standardizer(eng):
    c = br.CASES[5]._replace(steps=3)
    k = br.build(c)
    one = run_kernel(eng, c, k)
    same_state(one, run_kernel(eng, c, k, cuts=(1, 2)))


def test_refusals(eng):
    from olympic_hip._ffi import OlyError
    c = br.CASES[1]
    k = br.build(c)
    param = d(br.flat(k["params"]).astype(np.float32))
    z = torch.zeros_like(param)
    packed = eng.ilmlp_pack(*split(param, c.in_dim, c.A))
    ws = eng.bc_fit_ws(32, c.in_dim, c.A)
    states, targets = d(k["states"]), d(k["targets"])
    big = torch.zeros((1, 4097), dtype=torch.int32, device="cuda")
    with pytest.raises(OlyError, match="unsupported batch"):
        eng.bc_fit_steps(states, targets, big, None, param, z, z.clone(), packed, ws, 0, 1e-3)
    with pytest.raises(OlyError, match="ws"):
        eng.bc_fit_steps(states, targets, d(k["idx"]), None, param, z, z.clone(), packed, ws[:-4].contiguous(), 0, 1e-3)
    with pytest.raises(OlyError):
        eng.bc_fit_ws(32, 65, 4)
    torch.cuda.synchronize()
    assert torch.equal(param, d(br.flat(k["params"]).astype(np.float32))), "a refused call writes nothing"


# ------------------------------------------------------------------------------ oly_bc_targets
def test_targets_against_torch(eng):
    rng = np.random.default_rng(11)
    A, n = 5, 301
    min_a, max_a = -rng.uniform(0.5, 2.0, A), rng.uniform(0.5, 3.0, A)
    central, delta = (0.5 * (max_a + min_a)).astype(np.float32), (0.5 * (max_a - min_a)).astype(np.float32)
    a = (central + delta * np.tanh(rng.standard_normal((n, A)))).astype(np.float32)
    a[0], a[1] = np.float32(max_a), np.float32(min_a)                # on the bounds
    a[2], a[3] = np.float32(max_a) + 0.5, np.float32(min_a) - 0.5    # beyond
    a[4] = central                                                   # the centre: atanh(0) = 0
    got = eng.bc_targets(d(a), d(central), d(delta)).cpu().numpy()
    u = torch.clip((torch.as_tensor(a) - torch.as_tensor(central)) / torch.as_tensor(delta), -1.0 + 1e-7, 1.0 - 1e-7)
    ref64 = torch.arctanh(u.double()).numpy()
    top = np.float32(np.arctanh(np.float64(br.CLIP)))
    assert abs(float(top) - 8.3177662) < 1e-6
    assert np.all(got[2] == top) and np.all(got[3] == -top), "beyond the bounds: exactly the clipped value"
    on = np.abs(u.numpy()) == np.float32(br.CLIP)
    assert on[2].all() and on[3].all() and np.all(got[on] == np.sign(u.numpy()[on]) * top)
    assert np.all(got[4] == 0.0)
    ulp = np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(got.astype(np.float64) - ref64) <= 2 * ulp)
    ref32 = torch.arctanh(u).numpy()
    assert np.all(np.abs(got.astype(np.float64) - ref32.astype(np.float64)) <= 2 * np.maximum(ulp, np.spacing(np.abs(ref32))))


# ------------------------------------------------------------------------------ DeviceSquashedGaussianPolicy
def make_policy(eng, in_dim, A, seed, standardizer=True, rng=None):
    from olympic_hip.bc import DeviceSquashedGaussianPolicy
    from olympic_hip.gail import DeviceStandardizer
    torch.manual_seed(seed)
    lins = [torch.nn.Linear(in_dim, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 2 * A)]
    rng = rng or np.random.default_rng(seed)
    min_a, max_a = -rng.uniform(0.5, 2.0, A), rng.uniform(0.5, 3.0, A)
    st = DeviceStandardizer(eng, in_dim) if standardizer else None
    return DeviceSquashedGaussianPolicy(eng, lins, min_a, max_a, standardizer=st), lins, min_a, max_a


def test_policy_forward_act_and_log_prob(eng):
    in_dim, A, n = 19, 7, 45
    pol, lins, min_a, max_a = make_policy(eng, in_dim, A, 21)
    with torch.no_grad():
        lins[2].bias[A] = -25.0      # below log_std_min
        lins[2].bias[A + 1] = 3.0    # above log_std_max
    pol.set_weights(torch.cat([t.detach().reshape(-1) for lin in lins for t in (lin.weight, lin.bias)]))
    rng = np.random.default_rng(5)
    x = d((rng.standard_normal((n, in_dim)) * rng.uniform(0.3, 3, in_dim) + rng.standard_normal(in_dim)).astype(np.float32))
    eps = d(rng.standard_normal((n, A)).astype(np.float32))
    mu, ls = pol.get_mu_log_sigma(x)
    cs = pol.stand.colstats
    assert float(cs[0, 0]) == n, "the forward added the rows to the statistics"
    y = eng.ilmlp_forward(x, pol.packed, 2 * A, "identity", colstats=cs)
    assert torch.equal(mu, y[:, :A]) and torch.equal(ls, torch.clamp(y[:, A:], -20.0, 2.0))
    assert float(ls.min()) == -20.0 and float(ls.max()) == 2.0
    # float64 evaluation with the statistics after the rows went in (one more forward adds them again: rebuild)
    cnt = cs[0] + 1e-2
    mean = cs[1] / cnt
    std = torch.sqrt(torch.clamp((cs[2] + 1e-2) / cnt - mean * mean, min=1e-2))
    xs = ((x.double() - mean) / std).float().double()
    w = [t.detach().double().cuda() for lin in lins for t in (lin.weight, lin.bias)]
    y64 = torch.relu(torch.relu(xs @ w[0].T + w[1]) @ w[2].T + w[3]) @ w[4].T + w[5]
    mu64, ls64 = y64[:, :A], torch.clamp(y64[:, A:], -20.0, 2.0)
    central, delta = d(0.5 * (max_a + min_a)), d(0.5 * (max_a - min_a))
    pol.stand.colstats = cs.clone()
    pol.stand.colstats[0] -= n                      # act() adds the same rows again: leave it the statistics above
    pol.stand.colstats[1] -= x.double().sum(0)
    pol.stand.colstats[2] -= (x.double() ** 2).sum(0)
    keep = pol.stand.colstats.clone()
    act, ctrl = pol.act(x, eps=eps)
    assert ctrl is None
    raw64 = mu64 + ls64.exp() * eps.double()
    a64 = torch.tanh(raw64) * delta + central
    assert float((act.double() - a64).abs().max()) <= TOL
    pol.stand.colstats = keep.clone()
    det, _ = pol.act(x, deterministic=True)
    assert float((det.double() - (torch.tanh(mu64) * delta + central)).abs().max()) <= TOL
    pol.stand.colstats = keep.clone()
    mu_again, _ = pol.get_mu_log_sigma(x)
    assert torch.equal(det, (torch.tanh(mu_again) * pol.delta + pol.central))
    pol.stand.colstats = keep.clone()
    a2, _ = pol.compute_action_and_log_prob(x, eps=eps)
    assert torch.equal(a2, act)
    ent = pol.entropy_from_logsigma(ls)
    assert torch.allclose(ent.double(), A * (0.5 + 0.5 * np.log(2 * np.pi)) + ls64.sum(-1), rtol=TOL, atol=0)
    c2, d2 = pol.get_central_delta()
    assert torch.equal(c2, central.float()) and torch.equal(d2, delta.float())
    w0 = pol.get_weights()
    pol.sync_to_torch()
    assert torch.equal(torch.cat([t.detach().reshape(-1) for lin in lins for t in (lin.weight, lin.bias)]).cuda(), w0)


def test_policy_log_prob_against_float64(eng):
    """compute_action_and_log_prob at nn.Linear's default initialisation (log_sigma within -+0.5, |mu + sigma eps| < 4).
    The reference's float32 formula is ill-conditioned beyond that, in torch as here: at log_sigma = -20 the sample
    mu + 2e-9 eps rounds to mu, which moves the Gaussian term by eps^2 / 2, and log(1 - a^2 + 1e-6) carries the rounding
    of a^2 (6e-8) over 1 - a^2; at these values the latter stays under 1e-5 per row against |log_prob| of about 10."""
    in_dim, A, n = 19, 7, 45
    pol, lins, min_a, max_a = make_policy(eng, in_dim, A, 22)
    rng = np.random.default_rng(6)
    x = d((rng.standard_normal((n, in_dim)) * rng.uniform(0.3, 3, in_dim) + rng.standard_normal(in_dim)).astype(np.float32))
    eps = d(np.clip(rng.standard_normal((n, A)), -2.5, 2.5).astype(np.float32))
    act, lp = pol.compute_action_and_log_prob(x, eps=eps)
    cs = pol.stand.colstats
    cnt = cs[0] + 1e-2
    mean = cs[1] / cnt
    std = torch.sqrt(torch.clamp((cs[2] + 1e-2) / cnt - mean * mean, min=1e-2))
    xs = ((x.double() - mean) / std).float().double()
    w = [t.detach().double().cuda() for lin in lins for t in (lin.weight, lin.bias)]
    y64 = torch.relu(torch.relu(xs @ w[0].T + w[1]) @ w[2].T + w[3]) @ w[4].T + w[5]
    mu64, ls64 = y64[:, :A], torch.clamp(y64[:, A:], -20.0, 2.0)
    assert float(ls64.abs().max()) < 1.0
    raw64 = mu64 + ls64.exp() * eps.double()
    assert float(raw64.abs().max()) < 4.0
    t64 = torch.tanh(raw64)
    assert float((act.double() - (t64 * d(0.5 * (max_a - min_a)) + d(0.5 * (max_a + min_a)))).abs().max()) <= TOL
    lp64 = torch.distributions.Normal(mu64, ls64.exp()).log_prob(raw64).sum(1) - torch.log(1.0 - t64 ** 2 + 1e-6).sum(1)
    err = float(((lp.double() - lp64).abs() / lp64.abs().clamp(min=1.0)).max())
    print(f"log_prob: relative {err:.3e}")
    assert lp.shape == (n,) and err <= TOL


# ------------------------------------------------------------------------------ the trainer: resume, logging
class Writer:
    def __init__(self):
        self.rows = []

    def add_scalar(self, name, value, it):
        self.rows.append((name, value, it))


def make_trainer(eng, seed, demo, standardizer=True, **kw):
    from olympic_hip.bc import DeviceBehavioralCloning
    in_dim, A = demo["states"].shape[1], demo["actions"].shape[1]
    pol, _, _, _ = make_policy(eng, in_dim, A, seed, standardizer, rng=np.random.default_rng(77))
    return DeviceBehavioralCloning(eng, pol, demo, lr=1e-3, **kw)


def trainer_state(tr):
    st = tr.policy.stand
    return [tr.policy.param, tr.policy.packed, tr.exp_avg, tr.exp_avg_sq] + ([] if st is None else [st.colstats])


def test_resume_and_logging(eng, tmp_path):
    from olympic_hip import il_checkpoint
    c = br.CASES[1]
    k = br.build(c)
    demo = dict(states=k["states"], actions=k["actions"], next_states=k["states"], absorbing=np.zeros(c.n_rows))
    tr = make_trainer(eng, 1, demo, batch_size=c.batch)
    idx = tr.draw_idx(6, generator=torch.Generator(device="cuda").manual_seed(3))
    assert idx.shape == (6, 32) and all(len(set(r)) == 32 for r in idx.cpu().tolist())
    assert int(idx.min()) >= 0 and int(idx.max()) < c.n_rows
    sw = Writer()
    straight = make_trainer(eng, 1, demo, batch_size=c.batch, logging_iter=2, sw=sw)
    out = straight.fit_offline(6, idx=idx)
    assert straight.step == 6 and straight.iter == 6 and out.shape == (6, 3)
    host = out.cpu().numpy()
    assert [r[2] for r in sw.rows] == [0, 0, 0, 2, 2, 2, 4, 4, 4]
    assert [r[0] for r in sw.rows[:3]] == ["GaussianNLLLoss", "Squashed Gaussian Entropy",
                                           "MSELoss (between mean & target actions)"]
    assert [r[1] for r in sw.rows[3:6]] == [float(v) for v in host[2]]
    assert host[-1, 0] < host[0, 0]
    tr.fit_offline(3, idx=idx[:3].contiguous())
    for how in ("state_dict", "file"):
        fresh = make_trainer(eng, 2, demo, batch_size=c.batch)          # other seeds: every buffer differs
        assert not torch.equal(fresh.policy.param, tr.policy.param)
        if how == "state_dict":
            fresh.load_state_dict(tr.state_dict())
        else:
            path = il_checkpoint.save(str(tmp_path / "bc.pt"), tr, note="three steps")
            assert il_checkpoint.load(path, fresh)["note"] == "three steps"
        assert fresh.step == 3 and fresh.iter == 3
        out2 = fresh.fit_offline(3, idx=idx[3:].contiguous())
        for a, b in zip(trainer_state(fresh), trainer_state(straight)):
            assert torch.equal(a, b)
        assert torch.equal(out2, out[3:])
    # batch_size > n: the batch is cut to n; fit() raises as the reference's
    small = make_trainer(eng, 1, dict(states=k["states"][:30], actions=k["actions"][:30]), batch_size=40, standardizer=False)
    assert small.batch == 30 and small.fit_offline(2).shape == (2, 3) and small.policy.stand is None
    with pytest.raises(AttributeError):
        small.fit(None)


def test_example_runs_and_the_student_learns(tmp_path):
    log = tmp_path / "bc.json"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "bc_fit.py"), "--envs", "64", "--collect", "8",
                        "--steps", "40", "--eval-episodes", "64", "--horizon", "5", "--log", "--json", str(log)], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    import json
    rec = json.loads(log.read_text())
    assert rec["rows"] == 8 * 64 and rec["steps"] == 40 and "GaussianNLLLoss" in p.stdout
    assert rec["loss_last"] < rec["loss_first"], rec
