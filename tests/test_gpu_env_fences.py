"""K1-K9, the expert-data entries and the two host batchers on fenced and poisoned operands (tests/fences.py), at the
smallest shapes that still reach every path of their dispatchers.

Every device operand of every call is a Fenced tensor: inputs are fenced copies (tables read through an index with
gathered=True), outputs the caller may pass are poisoned Fenced tensors, and what the Engine allocates itself goes
through fence_engine.  Every case compares with the reference and at the bar of the entry point's parity test in
tests/test_gpu_parity.py (named in each docstring; no bar is new), and then asserts that
  * every margin is intact (no store outside a buffer),
  * every output the header documents as stored whole holds no poisoned element (no store forgotten),
  * no compared output holds a NaN (a load outside an input brings a NaN or an index -1 out of a margin).
The kernels that pick a vector path by the alignment of their pointers run a second time with their operands skewed
(Fenced(..., skew=)), which sends them down their scalar / generic path on the same fences.

uint8 outputs: 255 is no legal value of absorbing, done, at_end, bad and overflow (0 / 1), of fall_code (0 .. n_fall)
or of the cut flags (0 .. 3), so unwritten() counts their forgotten stores.  idx_r / idx_l of oly_contact_reduce are
padded with -1, the int32 poison: they are held through the oracle comparison alone."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from fences import Bufs, assert_untouched, fence_engine
from helpers import a3_fixture_arrays, h1_synthetic_block, ulp_diff
from olympic_hip import _abi, specs
from olympic_hip._ffi import OlyError, lib, ptr
from test_gpu_parity import _cmp_il, _ppo_case

pytestmark = pytest.mark.gpu
F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8


@pytest.fixture(scope="module")
def eng():
    from olympic_hip.engine import Engine
    e = Engine(0)
    yield e
    torch.cuda.synchronize()
    e.ctx.close()


def host(t):
    return t.cpu().numpy()


def engine_done(ef, what, padded=()):
    """What the Engine allocated inside fence_engine: margins intact, every allocation stored whole but for the tensors in
    `padded` (outputs that may legally hold the poison value)."""
    torch.cuda.synchronize()
    ef.check(what)
    skip = {t.data_ptr() for t in padded if t is not None}
    left = [(i, shape, n) for (i, shape, n), f in zip(ef.unwritten(), ef.bufs) if n and f.t.data_ptr() not in skip]
    assert not left, f"{what}: elements never stored in (allocation, shape, count) {left}"


def engine_untouched(ef, what):
    torch.cuda.synchronize()
    ef.check(what)
    hit = [(i, f.shape) for i, f in enumerate(ef.bufs) if f.unwritten() != f.n]
    assert not hit, f"{what}: a refused call stored into {hit}"


# ------------------------------------------------------------------------------ K1
K1_SPECS = dict(h1=lambda: specs.unitree_h1("walk"), h1_arms=lambda: specs.unitree_h1("walk", disable_arms=False),
                h1_foot_forces=lambda: specs.unitree_h1("walk").with_foot_forces("UnitreeH1"), atlas=lambda: specs.atlas("walk"))
K1_SHAPES = ((1, 1), (1, 127), (1, 128), (3, 129))
K1_OUT = ("obs", "reward", "absorbing", "fall_code", "ctrl", "prev_out")


def _k1_call(eng, sp, b, qpos, qvel, act, prev, grf, f64, skewed, **kw):
    T, N = qpos.shape[:2]
    od = F64 if f64 else F32
    q = b.inp("qpos", qpos, skew=8 if skewed else 0)
    v = b.inp("qvel", qvel, skew=8 if skewed else 0)
    a = b.inp("action", act, skew=4 if skewed else 0)
    out = dict(obs=b.out("obs", (T, N, sp.n_obs), od), reward=b.out("reward", (T, N), F32),
               absorbing=b.out("absorbing", (T, N), U8), fall_code=b.out("fall_code", (T, N), U8),
               ctrl=b.out("ctrl", (T, N, sp.nu), od))
    o = eng.il_step(q, v, a, b.inp("prev_in", prev), prev_out=b.out("prev_out", (N,), F64), grf_mean=b.inp("grf_mean", grf),
                    out=out, obs_f64=f64, ctrl_f64=f64, **kw)
    return {k: (None if t is None else host(t)) for k, t in o.items()}


@pytest.mark.parametrize("skewed", [False, True], ids=["aligned", "skewed"])
@pytest.mark.parametrize("robot", list(K1_SPECS))
def test_k1_il_step(eng, oracle, robot, skewed):
    """oly_il_step against oracle.il_step with _cmp_il of tests/test_gpu_parity.py (test_h1_vs_oracle_shapes: obs,
    absorbing, fall_code, prev and ctrl bit-exact, reward within 1 ulp of float32).

    Dispatch (k1_il_step.hip, oly_il_step): all four robots have a compile-time instantiation of the persistent tile
    kernel, taken when every pointer is 16-byte aligned; it runs the full 128-row tiles and hands the last R % 128 rows
    to the generic kernel.  R = T * N = 1 and 127: the generic remainder alone; 128: one full tile and no remainder; 387:
    three tiles and three rows.  Skewed (qpos, qvel by one double, action by one float): `fast` is off and the
    runtime-shape path (launch_dyn) takes every row.  obs / reward / absorbing / fall_code / ctrl are stored for every row
    and prev_out for every environment (the reward reads the previous observation), so all six are held to `written`."""
    sp = K1_SPECS[robot]()
    eng.il_configure(sp)
    rng = np.random.default_rng(17)
    for T, N in K1_SHAPES:
        qpos, qvel, act = h1_synthetic_block(sp, T, N, seed=T * 1000 + N, fall_frac="wide")
        act = np.ascontiguousarray(act, dtype=np.float32)
        prev = rng.normal(1.25, 0.5, N)
        grf = rng.normal(0, 400, (T, N, sp.n_grf)) if sp.n_grf else None
        okw = dict(grf_mean=grf) if sp.n_grf else {}
        for f64 in (False, True):
            what = f"il_step {robot} T={T} N={N} f64={f64} skewed={skewed}"
            b = Bufs()
            o = _k1_call(eng, sp, b, qpos, qvel, act, prev, grf, f64, skewed)
            b.done(what, written=K1_OUT, finite=("obs", "reward", "ctrl", "prev_out"))
            ref = oracle.il_step(sp, qpos, qvel, act, prev, obs_f64=f64, ctrl_f64=f64, **okw)
            _cmp_il(o, ref, f64)
        # the optional outputs switched off: their buffers stay as they were, the others do not change
        b2 = Bufs()
        o2 = _k1_call(eng, sp, b2, qpos, qvel, act, prev, grf, True, skewed, want_fall_code=False, want_ctrl=False)
        b2.done(what + " without fall_code / ctrl", written=("obs", "reward", "absorbing", "prev_out"), finite=("obs", "reward"))
        assert_untouched(dict(fall_code=b2["fall_code"], ctrl=b2["ctrl"]), what)
        assert o2["fall_code"] is None and o2["ctrl"] is None
        for k in ("obs", "reward", "absorbing", "prev"):
            assert o2[k].tobytes() == o[k].tobytes(), (k, what)


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("N", [1, 17])
def test_k1_il_ctrl(eng, oracle, N, f64):
    """oly_il_ctrl, bit-exact against the ctrl of oracle.il_step as test_il_ctrl_matches_il_step
    (tests/test_gpu_facade.py) holds it; one kernel (il_ctrl_kernel<f64>), every row stored."""
    sp = specs.unitree_h1("walk")
    eng.il_configure(sp)
    qpos, qvel, act = h1_synthetic_block(sp, 1, N, seed=2 + N)
    a = np.ascontiguousarray(act[0] * 1.4, dtype=np.float32)
    b = Bufs()
    eng.il_ctrl(b.inp("action", a), ctrl_f64=f64, out=b.out("ctrl", (N, sp.nu), F64 if f64 else F32))
    b.done(f"il_ctrl N={N}", written=("ctrl",), finite=("ctrl",))
    ref = oracle.il_step(sp, qpos, qvel, a[None], np.zeros(N), ctrl_f64=f64)
    assert np.array_equal(b.host("ctrl"), ref["ctrl"][0])


def test_k1_refusals_store_nothing(eng):
    """The refusals of test_il_argument_errors (tests/test_gpu_parity.py), with poisoned outputs: nothing is stored."""
    sp = specs.unitree_h1("walk")
    eng.il_configure(sp)
    b = Bufs()
    q = b.inp("q", np.zeros((2, 8, 17)))
    p = b.inp("p", np.zeros(8))
    out = lambda tag: dict(obs=b.out(tag + ".obs", (2, 8, 32), F32), reward=b.out(tag + ".reward", (2, 8), F32),
                           absorbing=b.out(tag + ".absorbing", (2, 8), U8), fall_code=b.out(tag + ".fall_code", (2, 8), U8))
    with fence_engine(eng) as ef:
        with pytest.raises(OlyError):
            eng.il_step(q, b.inp("q16", np.zeros((2, 8, 16))), None, p, out=out("nv"))         # wrong nv
        with pytest.raises(OlyError):
            eng.il_step(q, q, None, p, prev_out=p, out=out("alias"))                            # aliasing with T > 1
        with pytest.raises(OlyError):
            eng.il_step(b.inp("q32", np.zeros((2, 8, 17), np.float32)), q, None, p, out=out("dtype"))   # wrong dtype
        with pytest.raises(OlyError):
            eng.il_step(q.cpu(), q, None, p, out=out("host"))                                   # host tensor
        engine_untouched(ef, "il_step refusals")
    b.done("il_step refusals")
    assert_untouched({k: f for k, f in b.items() if "." in k}, "il_step refusals")


# ------------------------------------------------------------------------------ K2 / K5
@pytest.mark.parametrize("lanes", [1, 16])
@pytest.mark.parametrize("obs_f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("N", [1, 15, 16, 17])
def test_k2_a3_step(eng, golden, oracle, monkeypatch, N, obs_f64, lanes):
    """oly_a3_step over three steps against oracle.a3_step at the bars of test_a3_many_envs_vs_oracle
    (tests/test_gpu_parity.py): integer state and done bit-exact, goal and float64 obs 1e-12 / 1e-13, reward 2e-6 /
    1e-7; the float32 observation is the float64 one's rounding within the same bar in float32 (2e-6 / 1e-7, the bar
    that test gives float32 outputs).

    Dispatch (k2_a3_step.hip): a3_step16_kernel, sixteen lanes per environment in groups of 16 environments, or
    a3_step_kernel, one lane per environment; OLY_K2_LANES (read on every call) forces either, as the k2_lanes fixture
    of the parity tests does.  N = 15, 16, 17: a ragged group, a full one, one environment over.  Every state tensor is
    fenced and updated in place; `sequence` is read through the state's own index t1 (gathered=True).  obs, rew6,
    reward and done are stored for every environment."""
    monkeypatch.setenv("OLY_K2_LANES", str(lanes))
    g = golden("a3_task.npz")
    spec = specs.A3Spec(mass=41.5)
    eng.a3_configure(spec, g["clock_lut"])
    rng = np.random.default_rng(12 + N)
    pick = rng.integers(0, g["phase"].shape[0], N)
    st_h, _ = a3_fixture_arrays(g, 0)
    st_h = {k: np.ascontiguousarray(v[pick]) for k, v in st_h.items()}
    st_h["phase"] = rng.integers(0, 88, N).astype(np.int32)
    tgt = st_h["sequence"][np.arange(N), np.minimum(st_h["t1"], st_h["seq_len"] - 1), :3]
    inp = dict(qpos=np.concatenate([rng.normal(0, 1, (N, 3)), rng.normal(0, 1, (N, 4)), rng.uniform(-1, 1, (N, 18))], 1),
               qvel=rng.normal(0, 1, (N, 24)), act_len=rng.uniform(-1, 1, (N, 12)), act_vel=rng.normal(0, 2, (N, 12)),
               lf_pos=tgt + rng.normal(0, 0.15, (N, 3)), rf_pos=tgt + rng.normal(0, 0.3, (N, 3)),
               lf_vel=rng.normal(0, 0.2, (N, 3)), rf_vel=rng.normal(0, 0.2, (N, 3)),
               root_pos=tgt + np.array([0, 0, 0.7]) + rng.normal(0, 0.2, (N, 3)),
               root_quat=rng.normal(0, 1, (N, 4)), head_pos=tgt + np.array([0, 0, 1.2]) + rng.normal(0, 0.1, (N, 3)),
               grf_l=rng.uniform(0, 400, N), grf_r=rng.uniform(0, 400, N), min_z=rng.uniform(-0.01, 0.03, N),
               n_r=rng.integers(0, 3, N).astype(np.int32), n_l=rng.integers(0, 3, N).astype(np.int32),
               bad=(rng.uniform(size=N) < 0.2).astype(np.uint8))
    b = Bufs()
    st_d = {k: b.inp("st." + k, v, gathered=(k == "sequence")) for k, v in st_h.items()}
    st_o = {k: v.copy() for k, v in st_h.items()}
    od = F64 if obs_f64 else F32
    for s in range(3):
        d_in = {k: b.inp(f"in{s}.{k}", v) for k, v in inp.items()}
        names = [f"{k}{s}" for k in ("obs", "rew6", "reward", "done")]
        out = dict(obs=b.out(names[0], (N, spec.n_obs), od), rew6=b.out(names[1], (N, 6), F32),
                   reward=b.out(names[2], (N,), F32), done=b.out(names[3], (N,), U8))
        eng.a3_step(d_in, st_d, obs_f64=obs_f64, out=out)
        b.done(f"a3_step N={N} step {s}", written=names, finite=names[:3] + ["st.goal", "st.sequence"])
        eo = oracle.a3_step(spec, g["clock_lut"], inp, st_o)
        for k in ("phase", "t1", "t2", "reached_frames", "target_reached"):
            assert np.array_equal(b.host("st." + k), st_o[k]), (k, s)
        for k in ("mode", "seq_len", "sequence"):
            assert np.array_equal(b.host("st." + k), st_h[k]), (k, s)                   # inputs: as they were
        assert np.array_equal(b.host(names[3]), eo["done"])
        np.testing.assert_allclose(b.host("st.goal"), st_o["goal"], rtol=1e-12, atol=1e-13)
        if obs_f64:
            np.testing.assert_allclose(b.host(names[0]), eo["obs"], rtol=1e-12, atol=1e-13)
        else:
            np.testing.assert_allclose(b.host(names[0]), eo["obs"].astype(np.float32), rtol=2e-6, atol=1e-7)
        np.testing.assert_allclose(b.host(names[2]), eo["reward"], rtol=2e-6, atol=1e-7)
        np.testing.assert_allclose(b.host(names[1]), eo["rew6"], rtol=2e-6, atol=1e-7)
        inp["lf_pos"] = inp["lf_pos"] + rng.normal(0, 0.02, (N, 3))


@pytest.mark.parametrize("N", [1, 17])
def test_k5_a3_pd(eng, golden, oracle, N):
    """oly_a3_pd_target bit-exact against oracle.a3_pd_target and oly_a3_pd_torque bit-exact against the reference's
    torques of a3_task.npz, as test_a3_pd (tests/test_gpu_parity.py); one element-wise kernel each, every element
    stored (the Engine allocates both outputs)."""
    g = golden("a3_task.npz")
    spec = specs.A3Spec()
    eng.a3_configure(spec, g["clock_lut"])
    rows = np.arange(N) % len(g["pd_action"])
    a32 = np.ascontiguousarray(g["pd_action"][rows].astype(np.float32))
    b = Bufs()
    with fence_engine(eng) as ef:
        tgt = eng.a3_pd_target(b.inp("action", a32))
        engine_done(ef, "a3_pd_target")
        assert np.array_equal(host(tgt), oracle.a3_pd_target(spec, a32))
        kp, kd, t = b.inp("kp", spec.kp), b.inp("kd", spec.kd), b.inp("target", g["pd_target"][rows])
        for s in range(g["pd_q"].shape[1]):
            tau = eng.a3_pd_torque(kp, kd, t, b.inp(f"q{s}", g["pd_q"][rows, s]), b.inp(f"qd{s}", g["pd_qd"][rows, s]))
            engine_done(ef, f"a3_pd_torque {s}")
            assert np.array_equal(host(tau), g["pd_tau"][rows, s])
    b.done("a3_pd")


# ------------------------------------------------------------------------------ K3
GEOM_BODY = np.array([0, 1, 2, 3, 4, 5, 6, 7, 7, 8, 9, 10, 10], np.int32)
K3_SHAPES = ((1, 16), (5, 7), (33, 40))


def _ncon(rng, shape, C):
    """Counts that hold 0, C and values above C (every one of them where there is room)."""
    n = rng.integers(0, C + 4, shape).astype(np.int32)
    flat = n.reshape(-1)
    for i, v in enumerate((C, 0, C + 3)[:flat.size]):
        flat[i] = v
    return n


@pytest.mark.parametrize("N,Cc", K3_SHAPES)
def test_k3_contact_reduce_and_csr(eng, oracle, N, Cc):
    """oly_contact_reduce: every output bit-exact against oracle.contact_reduce (test_contacts_shapes,
    tests/test_gpu_parity.py).  The oracle refuses ncon > C, so such an environment is compared with the oracle's result
    for ncon = C (the staged slots are still counted) and must come back bad, which is what
    test_contacts_more_than_the_staged_slots holds.  oly_contact_reduce_csr: bit-identical to the padded form on the
    same contacts (test_contact_reduce_csr_equals_the_padded_form); its records are a uint8 table read through coff.

    One kernel per form, one lane per environment walking its slots; C = 40 is more than the 16 slots staged at a time.
    n_r, n_l, grf_r, grf_l, min_z and bad are stored for every environment; idx_r / idx_l are -1 padded (the poison)."""
    rng = np.random.default_rng(N + Cc)
    eng.contact_configure(GEOM_BODY, 0, 7, 10)
    ncon = _ncon(rng, N, Cc)
    g1 = rng.choice([0, 0, 0, 8, 3], (N, Cc)).astype(np.int32)
    g2 = rng.choice([8, 12, 8, 12, 0, 5], (N, Cc)).astype(np.int32)
    f6 = rng.normal(0, 100, (N, Cc, 6))
    pz = rng.uniform(-0.05, 0.05, (N, Cc))
    b = Bufs()
    d = [b.inp("ncon", ncon), b.inp("geom1", g1), b.inp("geom2", g2), b.inp("force6", f6), b.inp("pos_z", pz)]
    with fence_engine(eng) as ef:
        o = eng.contact_reduce(*d)
        engine_done(ef, f"contact_reduce N={N} Cc={Cc}", padded=(o["idx_r"], o["idx_l"]))
        used = np.minimum(ncon, Cc)
        e = oracle.contact_reduce(GEOM_BODY, 0, 7, 10, used, g1, g2, f6, pz)
        over = ncon > Cc
        assert over.any() or N == 1
        for k in e:
            if k == "bad":
                assert np.array_equal(host(o[k])[~over], e[k][~over]) and (host(o[k])[over] == 1).all()
            else:
                assert np.array_equal(host(o[k]), e[k]), k
        ref = eng.contact_reduce(*d, want_idx=False)
        coff = (np.cumsum(used) - used).astype(np.int32)
        rec = np.zeros(int(used.sum()) + 1, np.dtype([("g1", "<i4"), ("g2", "<i4"), ("f", "<f8", 6), ("z", "<f8")]))
        assert rec.dtype.itemsize == C.sizeof(_abi.ContactRecord) == 64
        for n in range(N):
            sl = slice(coff[n], coff[n] + used[n])
            rec["g1"][sl], rec["g2"][sl], rec["f"][sl], rec["z"][sl] = g1[n, :used[n]], g2[n, :used[n]], f6[n, :used[n]], pz[n, :used[n]]
        # one 64-byte record per row of the table, so that gathered=True holds its pitch to the fence
        records = b.inp("records", rec.view(np.uint8).reshape(-1, 64), gathered=True)
        got = eng.contact_reduce_csr(d[0], b.inp("coff", coff), records.view(-1), Cc)
        engine_done(ef, f"contact_reduce_csr N={N} Cc={Cc}", padded=(o["idx_r"], o["idx_l"]))
        for k in ("n_r", "n_l", "grf_r", "grf_l", "min_z", "bad"):
            assert torch.equal(got[k], ref[k]), k
    b.done(f"contacts N={N} Cc={Cc}")


@pytest.mark.parametrize("N,C", K3_SHAPES)
def test_k3_il_ground_forces_and_window(eng, oracle, N, C):
    """oly_il_ground_forces (steps, mean and the overflow flags) and oly_il_grf_window, bit-exact against
    oracle.il_ground_forces as test_il_ground_forces_vs_oracle (tests/test_gpu_parity.py); raw counts of 0, C and above
    C.  One kernel each; grf_step, grf_mean and overflow are stored for every environment and substep."""
    W = 3
    rng = np.random.default_rng(W + N + C)
    ngeom = 30
    gg = np.full(ngeom, -1, np.int32)
    gg[0], gg[[7, 8]], gg[[20]], gg[[21]], gg[[22]] = 0, 1, 2, 3, 4
    pairs = [(0, 1), (0, 2), (0, 3), (0, 4)][:1 + (N % 4)]
    ncon = _ncon(rng, (W, N), C)
    g1 = np.where(rng.uniform(size=(W, N, C)) < 0.5, 0, rng.integers(-1, ngeom + 1, (W, N, C))).astype(np.int32)
    g2 = rng.choice([0, 7, 8, 20, 21, 22, 3, 29, -1, ngeom], size=(W, N, C)).astype(np.int32)
    swap = rng.uniform(size=(W, N, C)) < 0.3
    g1, g2 = np.where(swap, g2, g1).astype(np.int32), np.where(swap, g1, g2).astype(np.int32)
    f6 = rng.normal(0, 200, (W, N, C, 6))
    eng.grf_configure(gg, pairs)
    b = Bufs()
    with fence_engine(eng) as ef:
        o = eng.il_ground_forces(b.inp("ncon", ncon), b.inp("geom1", g1), b.inp("geom2", g2), b.inp("force6", f6),
                                 want_steps=True, check=False)
        engine_done(ef, f"il_ground_forces N={N} C={C}")
        e_step, e_mean, e_over = oracle.il_ground_forces(gg, pairs, ncon, g1, g2, f6, want_overflow=True)
        assert np.array_equal(host(o["steps"]), e_step) and np.array_equal(host(o["mean"]), e_mean)
        assert np.array_equal(host(o["overflow"]), e_over)
        m2 = eng.il_ground_forces(b["ncon"].t, b["geom1"].t, b["geom2"].t, b["force6"].t)["mean"]   # grf_step NULL
        engine_done(ef, "il_ground_forces without steps")
        assert torch.equal(m2, o["mean"])
        mean = b.out("window", (N, 3 * len(pairs)), F64)
        eng.il_grf_window(b.inp("grf_step", e_step), mean)
        b.done(f"il_grf_window N={N}", written=("window",), finite=("window",))
        assert np.array_equal(b.host("window"), e_mean)
    b.done(f"ground forces N={N} C={C}")


# ------------------------------------------------------------------------------ K4 and the expert data
@pytest.mark.parametrize("N", [1, 5, 129])
def test_k4_traj_reset_next_euler(eng, golden, oracle, N):
    """oly_traj_reset / oly_traj_next / oly_traj_euler on the table of trajectory.npz, bit-exact against the oracle as
    test_traj_vs_oracle_many_envs (tests/test_gpu_parity.py); environment 0 starts at the last step of its trajectory,
    so its first oly_traj_next reports at_end and leaves its sample row alone.  One lane per environment in each kernel;
    129 is more than one wave and, with 256 threads, still one block.  reset stores cur_traj, cur_step, origin and sample
    whole, next stores at_end whole; sample and cur_step are otherwise updated in place."""
    table = golden("trajectory.npz")["table"]
    K, J, L = table.shape
    eng.traj_upload(table)
    rng = np.random.default_rng(4 + N)
    tn, st = rng.integers(0, J, N).astype(np.int32), rng.integers(0, L, N).astype(np.int32)
    st[0] = L - 1
    b = Bufs()
    ct, cs = b.out("cur_traj", (N,), I32), b.out("cur_step", (N,), I32)
    origin, sample = b.out("origin", (N, 2), F64), b.out("sample", (N, K), F64)
    eng.traj_reset(b.inp("traj_no", tn), b.inp("step", st), ct, cs, origin, sample)
    b.done(f"traj_reset N={N}", written=("cur_traj", "cur_step", "origin", "sample"), finite=("origin", "sample"))
    e_ct, e_cs, e_or, e_sa = oracle.traj_reset(table, tn, st)
    assert np.array_equal(host(sample), e_sa) and np.array_equal(host(origin), e_or)
    assert np.array_equal(host(ct), e_ct) and np.array_equal(host(cs), e_cs)
    active = (rng.uniform(size=N) < 0.7).astype(np.uint8)
    active[0] = 1
    act_d = b.inp("active", active)
    for i in range(3):
        cur = rng.normal(size=(N, 17))
        eng.traj_euler(17, 0.01, b.inp(f"cur{i}", cur), sample)
        e_sa = oracle.traj_euler(17, 0.01, cur, e_sa)
        b.done(f"traj_euler {i}", finite=("sample",))
        assert np.array_equal(host(sample), e_sa)
        at_end = b.out(f"at_end{i}", (N,), U8)
        eng.traj_next(ct, cs, origin, sample, active=act_d if i else None, at_end=at_end)
        e_cs, e_sa, e_end = oracle.traj_next(table, e_ct, e_cs, e_or, e_sa, active=active if i else None)
        b.done(f"traj_next {i}", written=(f"at_end{i}",), finite=("sample",))
        assert np.array_equal(host(cs), e_cs) and np.array_equal(host(at_end), e_end) and np.array_equal(host(sample), e_sa)
        assert host(at_end)[0] == 1
    assert np.array_equal(host(ct), e_ct) and np.array_equal(host(origin), e_or)


@pytest.mark.parametrize("want_next", [False, True])
@pytest.mark.parametrize("B", [1, 7])
def test_expert_gather_and_dataset(eng, golden, B, want_next):
    """oly_expert_gather and oly_expert_dataset bit-exact against the reference's create_dataset arrays of
    trajectory.npz (ds_*), as test_expert_dataset_and_minibatches_from_the_device_table (tests/test_gpu_expert.py).
    The indices hold row 0 and the last row; idx and cols are fenced (an index read from a margin is -1).  One kernel
    each, one lane per output element; every output is stored whole."""
    from olympic_hip.gail import ExpertDataset
    from test_gpu_expert import _traj_from_golden
    g = golden("trajectory.npz")
    ds = ExpertDataset(eng, _traj_from_golden(g), ignore_keys=["q_pelvis_tx", "q_pelvis_tz"])
    rows = ds.rows
    assert rows == len(g["ds_states"])
    idx = np.array([rows - 1, 0, 5, rows - 1, 17, 0, 42][:B] if B > 1 else [rows - 1], np.int64)
    if B == 1 and want_next:
        idx = np.array([0], np.int64)
    b = Bufs()
    cols = b.inp("cols", host(ds.cols))
    with fence_engine(eng) as ef:
        o = eng.expert_gather(b.inp("idx", idx), cols, want_next=want_next)
        engine_done(ef, f"expert_gather B={B}")
        st, nx = o if want_next else (o, None)
        assert np.array_equal(host(st), g["ds_states"][idx].astype(np.float32))
        if want_next:
            assert np.array_equal(host(nx), g["ds_next_states"][idx].astype(np.float32))
        d = eng.expert_dataset(b.inp("dataset_cols", host(ds.dataset_cols)))
        engine_done(ef, "expert_dataset")
        for k in ("states", "next_states", "absorbing", "last"):
            assert np.array_equal(host(d[k]), g["ds_" + k]), k
    b.done(f"expert data B={B}")


# ------------------------------------------------------------------------------ K6
def _scan_case(T, N, seed=0):
    rng = np.random.default_rng(T * 7 + N + seed)
    r = rng.uniform(-0.3, 1, (T, N))
    v = rng.normal(0, 1, (T, N)).astype(np.float32)
    vn = rng.normal(0, 1, (T, N)).astype(np.float32)
    last = rng.uniform(size=(T, N)) < 1 / 30
    ab = last & (rng.uniform(size=(T, N)) < 0.5)
    return r, v, vn, (last * _abi.FLAG_LAST + ab * _abi.FLAG_ABSORBING).astype(np.uint8)


def _scan_run(eng, mode, rew, v, vn, flags, skew=0, stats=True, plain=False):
    """One fenced oly_return_scan_stats (plain: oly_return_scan itself); -> (ret, adv, stats3 or None) on the host."""
    T, N = v.shape
    b = Bufs()
    d = [b.inp("rew", rew, skew=2 * skew if rew.dtype == np.float64 else skew), b.inp("val", v, skew=skew),
         b.inp("next_val", vn, skew=skew), b.inp("flags", flags, skew=skew)]
    ret, adv = b.out("ret", (T, N), F32, skew=skew), b.out("adv", (T, N), F32, skew=skew)
    written = ["ret", "adv"]
    if plain:
        eng.ctx.call("oly_return_scan", int(mode), T, N, C.c_double(0.99), C.c_double(0.97), *(ptr(t) for t in d), ptr(ret),
                     ptr(adv), eng._s())
    else:
        st = b.out("stats3", (3,), F64, skew=2 * skew) if stats else None
        written += ["stats3"] if stats else []
        eng.return_scan(mode, 0.99, 0.97, *d, ret=ret, adv=adv, stats3=st)
    b.done(f"return_scan mode={mode} T={T} N={N} {rew.dtype} skew={skew}", written=written, finite=written)
    return b.host("ret"), b.host("adv"), (b.host("stats3") if stats and not plain else None)


def _scan_check(eng, oracle, T, N, skew=0):
    r64, v, vn, flags = _scan_case(T, N)
    r32 = r64.astype(np.float32)
    res = {}
    for mode, rew in ((_abi.SCAN_RETURN, r32), (_abi.SCAN_GAE, r32), (_abi.SCAN_RETURN, r64)):
        ret, adv, st = _scan_run(eng, mode, rew, v, vn, flags, skew=skew)
        if rew.dtype == np.float64:
            e_ret, e_adv = oracle.return_scan_r64(0.99, rew, v, vn, flags)
        else:
            e_ret, e_adv = oracle.return_scan(mode, 0.99, 0.97, rew, v, vn, flags)
        assert np.array_equal(ret, e_ret) and np.array_equal(adv, e_adv), (mode, rew.dtype, T, N)
        assert st[0] == T * N
        np.testing.assert_allclose(st[1:], oracle.adv_stats(e_adv)[1:], rtol=1e-12, atol=1e-9)
        res[(mode, str(rew.dtype))] = (ret, adv, st)
        if rew.dtype == np.float32:
            ret2, adv2, _ = _scan_run(eng, mode, rew, v, vn, flags, skew=skew, plain=True)      # oly_return_scan
            assert ret2.tobytes() == ret.tobytes() and adv2.tobytes() == adv.tobytes()
    return res


@pytest.mark.parametrize("T,N", [(1, 1), (5, 3), (1, 4), (33, 257), (7, 260)])
def test_k6_return_scan_small(eng, oracle, T, N):
    """oly_return_scan and oly_return_scan_stats, both modes and float64 rewards: ret / adv bit-exact against the oracle
    (test_scan_vs_oracle, test_scan_float64_rewards_vs_oracle), the statistics at 1e-12 relative, 1e-9 absolute with
    an exact count (test_scan_fused_statistics; all tests/test_gpu_parity.py).

    Dispatch (k6_scan.hip, oly_return_scan_stats): N % 4 != 0, or a pointer off its alignment, takes scan_tile_kernel,
    64 environments per block, and a separate oly_adv_stats: (1, 1), (5, 3) and (33, 257), the last with five blocks
    and one environment in the fifth.  N % 4 == 0 with aligned pointers takes scan_pipe_kernel, below 64 environments
    per CU in its 16-environment workgroups: (1, 4) one ragged workgroup and one step, (7, 260) seventeen workgroups,
    the last with four environments.  ret, adv and stats3 are stored whole by every path."""
    _scan_check(eng, oracle, T, N)


@pytest.mark.parametrize("per_cu", [64, 128, 256])
def test_k6_return_scan_wide(eng, oracle, per_cu):
    """The further kernels the default dispatch picks, each at its threshold, T = 2: N = 64 environments per CU selects
    scan_pipe_kernel's 32-environment workgroups, 128 per CU its 64-environment ones, and 256 per CU the
    lane-per-environment scan_lane_kernel in RETURN mode (GAE stays on the pipelined kernel).  Same bars."""
    N = per_cu * torch.cuda.get_device_properties(0).multi_processor_count
    _scan_check(eng, oracle, 2, N)


def test_k6_return_scan_skewed_fallback(eng, oracle):
    """Every operand 4 bytes off a 256-byte boundary (the float64 ones 8) at N % 4 == 0: wide_ok fails and scan_tile_kernel
    runs (the path of test_scan_unaligned_views_take_the_fallback), on fences, and gives the bytes of the aligned run."""
    T, N = 7, 260
    aligned, skewed = _scan_check(eng, oracle, T, N), _scan_check(eng, oracle, T, N, skew=4)
    for k in aligned:
        assert aligned[k][0].tobytes() == skewed[k][0].tobytes() and aligned[k][1].tobytes() == skewed[k][1].tobytes(), k


def test_k6_lane_kernel_child():
    """OLY_K6_PIPE=7 forces scan_lane_kernel onto every shape and onto GAE, which the default dispatch never sends there;
    the variable is read once per process, hence the child (as test_scan_lane_kernel_on_every_scan_case,
    tests/test_gpu_parity.py).  Like that test it cannot tell whether the variable took effect."""
    env = dict(os.environ, OLY_K6_PIPE="7")
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k",
                          "k6_return_scan_small or k6_return_scan_skewed", "-p", "no:cacheprovider"], capture_output=True,
                         text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert " passed" in out.stdout and "no tests ran" not in out.stdout, out.stdout[-500:]


@pytest.mark.parametrize("N", [1, 63, 65])
def test_rollout_cuts(eng, oracle, N):
    """oly_rollout_cuts bit-exact against oracle.rollout_cuts (test_rollout_cuts_vs_oracle, tests/test_gpu_parity.py):
    one lane per environment, 63 and 65 on either side of a wave.  traj_len is updated in place; flags is stored for
    every environment and n_cut is cleared and counted, so both start poisoned."""
    rng = np.random.default_rng(N)
    tl = rng.integers(0, 12, N).astype(np.int32)
    b = Bufs()
    tl_d = b.inp("traj_len", tl)
    for last in (0, 1):
        done = (rng.uniform(size=N) < 0.1).astype(np.uint8)
        fl_d, nc_d = b.out(f"flags{last}", (N,), U8), b.out(f"n_cut{last}", (1,), I32)
        eng.rollout_cuts(b.inp(f"done{last}", done), tl_d, fl_d, nc_d, 10, last)
        b.done(f"rollout_cuts N={N} last={last}", written=(f"flags{last}", f"n_cut{last}"))
        fl, tl2, nc = oracle.rollout_cuts(done, tl, 10, last)
        assert np.array_equal(host(fl_d), fl) and np.array_equal(host(tl_d), tl2) and int(nc_d) == nc
        tl = tl2


# ------------------------------------------------------------------------------ K7
@pytest.mark.parametrize("skew", [0, 4], ids=["aligned", "skewed"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027])
def test_k7_adv_stats_and_normalize(eng, oracle, n, skew):
    """oly_adv_stats: exact count, sums at 1e-12 against oracle.adv_stats; oly_adv_normalize and
    oly_adv_normalize_parts in place on a fenced x: bit-exact against oracle.adv_normalize / adv_normalize_parts
    (test_adv_stats_normalize, test_adv_normalize_parts; tests/test_gpu_parity.py).  n = 1 is normalised with ddof = 0
    only (ddof = 1 divides by zero, which that test leaves out too); three parts need three elements.

    Both kernels (k7_stats.hip) read float4 groups while x is 16-byte aligned and finish the n % 4 tail by the element:
    n = 1 and 3 are tail alone, 4 one group and no tail, 5 and 1027 a group or 256 of them and a tail of 1 and 3.
    Skewed by one float, the scalar loop takes every element.  stats3 is stored whole."""
    rng = np.random.default_rng(n)
    x = rng.normal(0.3, 2.0, n).astype(np.float32)
    b = Bufs()
    xd = b.inp("x", x, skew=skew)
    st = eng.adv_stats(xd, b.out("stats3", (3,), F64))
    b.done(f"adv_stats n={n}", written=("stats3",), finite=("stats3",))
    s = b.host("stats3")
    assert s[0] == n
    np.testing.assert_allclose(s[1:], oracle.adv_stats(x)[1:], rtol=1e-12)
    for ddof, eps in (((1, 1e-5), (0, 1e-8)) if n > 1 else ((0, 1e-8),)):
        y = b.inp(f"y{ddof}", x, skew=skew)
        eng.adv_normalize(y, st, ddof, eps)
        b.done(f"adv_normalize_parts n={n} ddof={ddof}", finite=(f"y{ddof}",))
        assert np.array_equal(host(y), oracle.adv_normalize(x, s, ddof, eps))
        y1 = b.inp(f"y1{ddof}", x, skew=skew)
        eng.ctx.call("oly_adv_normalize", C.c_int64(n), ptr(y1), ptr(st), ddof, C.c_double(eps), eng._s())
        b.done(f"adv_normalize n={n} ddof={ddof}", finite=(f"y1{ddof}",))
        assert torch.equal(y1, y)
        if n >= 3:
            shards = np.array_split(x, 3)
            p3 = np.stack([host(eng.adv_stats(b.inp(f"shard{ddof}.{i}", sh, skew=skew), b.out(f"p3{ddof}.{i}", (3,), F64)))
                           for i, sh in enumerate(shards)])
            y3 = b.inp(f"y3{ddof}", x, skew=skew)
            eng.adv_normalize(y3, b.inp(f"parts{ddof}", p3), ddof, eps)
            b.done(f"adv_normalize_parts n={n} parts=3", finite=(f"y3{ddof}",))
            assert np.array_equal(host(y3), oracle.adv_normalize_parts(x, p3, ddof, eps))


@pytest.mark.parametrize("B,D,skew", [(1, 32, 0), (2, 32, 0), (3, 41, 0), (129, 12, 0), (130, 32, 0), (130, 32, 4), (3, 41, 4)])
def test_k7_col_stats(eng, oracle, B, D, skew):
    """oly_col_stats at 1e-12 against oracle.col_stats, accumulate 0 into a poisoned colstats and then 1 into the same
    (test_col_stats, tests/test_gpu_parity.py).

    Dispatch (k7_stats.hip): D % 4 == 0 with a 16-byte aligned x takes col_partial4_kernel, one float4 per row and lane
    and two rows, r and r + lanes, per trip of its loop, with a guarded single row at the end: D = 32 has 32 rows in
    flight, so B = 1 and 2 leave lanes idle, (130, 32) gives rows 0 .. 31 two trips and a guarded fifth row for rows 0
    and 1, and (129, 12), 85 rows in flight, one trip for rows 0 .. 43 and a guarded row for the rest.  D = 41, or x one
    float off, takes the scalar col_partial_kernel.  colstats is stored whole when accumulate is 0."""
    rng = np.random.default_rng(B + D)
    b = Bufs()
    cs = b.out("colstats", (3, D), F64)
    want = 0
    for acc in (0, 1):
        x = rng.normal(0.5, 1.5, (B, D)).astype(np.float32)
        xd = b.inp(f"x{acc}", x, skew=skew)
        if acc:
            eng.col_stats(xd, cs)
        else:                                           # Engine.col_stats overwrites only a buffer of its own
            eng.ctx.call("oly_col_stats", B, D, ptr(xd), ptr(cs), 0, eng._s())
        b.done(f"col_stats B={B} D={D} accumulate={acc}", written=("colstats",), finite=("colstats",))
        want = want + oracle.col_stats(x)
        np.testing.assert_allclose(b.host("colstats"), want, rtol=1e-12)
    assert (b.host("colstats")[0] == 2 * B).all()
    with fence_engine(eng) as ef:                       # the Engine's own allocation of a fresh colstats
        got = eng.col_stats(b["x1"].t)
        engine_done(ef, "col_stats, engine-allocated")
        np.testing.assert_allclose(host(got), oracle.col_stats(b.host("x1")), rtol=1e-12)


# ------------------------------------------------------------------------------ K8
@pytest.mark.parametrize("B", [1, 65])
@pytest.mark.parametrize("Dx,D,skew", [(32, 32, 0), (32, 11, 0), (11, 11, 0), (36, 32, 0), (32, 32, 4)])
def test_k8_disc_standardize(eng, oracle, B, Dx, D, skew):
    """oly_disc_standardize bit-exact against oracle.disc_standardize (test_disc_golden, tests/test_gpu_parity.py), with
    and without a mask.  Dispatch (k8_disc.hip): no mask, D % 4 == 0 and aligned x / out take standardize4_kernel;
    a mask (D < Dx: 11 of 32 and 32 of 36 columns), D = 11, or x and out one float off take the scalar
    standardize_kernel.  x is read through the mask (gathered=True).  out is stored whole."""
    rng = np.random.default_rng(B + Dx + D)
    x = rng.normal(0.3, 2.0, (B, Dx)).astype(np.float32)
    mask = None if D == Dx else np.sort(rng.choice(Dx, D, replace=False)).astype(np.int32)
    mean, std = rng.normal(0.3, 0.2, D), rng.uniform(0.5, 2.5, D)
    b = Bufs()
    out = b.out("out", (B, D), F32, skew=skew)
    eng.disc_standardize(b.inp("x", x, gathered=True, skew=skew), b.inp("mask", mask), b.inp("mean", mean), b.inp("std", std), out)
    b.done(f"disc_standardize B={B} Dx={Dx} D={D}", written=("out",), finite=("out",))
    assert np.array_equal(b.host("out"), oracle.disc_standardize(x, np.arange(Dx) if mask is None else mask, mean, std))


@pytest.mark.parametrize("in_place", [False, True], ids=["out", "in_place"])
@pytest.mark.parametrize("B,D,skew", [(1, 32, 0), (65, 32, 0), (1, 41, 0), (65, 41, 0), (65, 32, 4)])
def test_k8_obs_filter(eng, oracle, B, D, skew, in_place):
    """oly_obs_filter bit-exact against oracle.obs_filter (test_obs_filter_and_device_running_mean_std,
    tests/test_gpu_parity.py), into a poisoned out and with out = x.  D % 4 == 0 and aligned pointers take
    obs_filter4_kernel, D = 41 or a skew of one float the scalar obs_filter_kernel.  out is stored whole."""
    rng = np.random.default_rng(B + D)
    x = rng.normal(0, 3, (B, D)).astype(np.float32)
    m, v = rng.normal(0, 1, D), rng.uniform(0.1, 4, D)
    b = Bufs()
    xd = b.inp("x", x, skew=skew)
    out = xd if in_place else b.out("out", (B, D), F32, skew=skew)
    eng.obs_filter(xd, b.inp("mean", m), b.inp("var", v), 1e-8, 5.0, out=out)
    b.done(f"obs_filter B={B} D={D}", written=() if in_place else ("out",), finite=("x",) if in_place else ("out",))
    assert np.array_equal(host(out), oracle.obs_filter(x, m, v, 1e-8, 5.0))
    if not in_place:
        assert np.array_equal(b.host("x"), x)


@pytest.mark.parametrize("n", [1, 7, 1028])
def test_k8_disc_reparam(eng, oracle, n):
    """oly_disc_reparam against oracle.disc_reparam at rtol 3e-7, atol 1e-7 (test_disc_golden, tests/test_gpu_parity.py):
    one element-wise kernel, 1028 is four blocks and four elements over.  z is stored whole, both the caller's and the
    one the Engine allocates."""
    rng = np.random.default_rng(n)
    mu, lv, eps = (rng.normal(0, 1, n).astype(np.float32) for _ in range(3))
    b = Bufs()
    d = [b.inp("mu", mu), b.inp("logvar", lv), b.inp("eps", eps)]
    eng.disc_reparam(*d, z=b.out("z", (n,), F32))
    b.done(f"disc_reparam n={n}", written=("z",), finite=("z",))
    np.testing.assert_allclose(b.host("z"), oracle.disc_reparam(mu, lv, eps), rtol=3e-7, atol=1e-7)
    with fence_engine(eng) as ef:
        z = eng.disc_reparam(*d)
        engine_done(ef, "disc_reparam, engine-allocated")
        assert len(ef.bufs) == 1 and torch.equal(z, b["z"].t)
    b.done("disc_reparam")


@pytest.mark.parametrize("skew", [0, 4], ids=["aligned", "skewed"])
@pytest.mark.parametrize("n", [1, 3, 4, 4099])
def test_k8_disc_reward(eng, oracle, n, skew):
    """oly_disc_reward against oracle.disc_reward within the float32 tolerance of
    test_disc_reward_vector_and_scalar_paths (tests/test_gpu_parity.py).  reward_kernel (k8_disc.hip) stores float4
    groups while both pointers are 16-byte aligned and the n % 4 tail by the element: n = 1 and 3 tail alone, 4 one
    group, 4099 = 1024 groups (four full blocks of the five launched) and a tail of 3; one float off, every element by
    the element.  reward is stored whole."""
    rng = np.random.default_rng(n + skew)
    d = np.concatenate([rng.normal(0, 4, n - min(n, 3)), [-30.0, 0.0, 25.0][:min(n, 3)]]).astype(np.float32)
    b = Bufs()
    eng.disc_reward(b.inp("logits", d, skew=skew), b.out("reward", (n,), F32, skew=skew))
    b.done(f"disc_reward n={n} skew={skew}", written=("reward",), finite=("reward",))
    r, want = b.host("reward"), oracle.disc_reward(d)
    p = 1.0 / (1.0 + np.exp(-d.astype(np.float64)))
    tol = 4 * 2.0 ** -24 / (1 - p + 1e-8) + 4e-7 * np.abs(want) + 1e-7
    assert (np.abs(r - want) <= tol).all() and np.isfinite(r).all()


# ------------------------------------------------------------------------------ K12, the paired paths
@pytest.mark.parametrize("mode,pair", [("action", (1, 1)), ("action", (33, 31)), ("next_state", (17, 17))],
                         ids=["action-1+1", "action-33+31", "next_state-17+17"])
@pytest.mark.parametrize("B", [1, 33])
def test_k12_disc_reward_step_and_forward_pair(eng, B, mode, pair):
    """oly_disc_reward_step_pair and oly_disc_forward_pair, the two K8 / K12 entry points the K12 cases of
    tests/test_gpu_fences.py do not call (oly_disc_pack, oly_disc_forward and oly_disc_reward_step run fenced there),
    as test_k18_gail_reward_step_and_forward_pair (tests/test_gpu_il_fences.py) runs their GAIL twins: against
    pair_restate.restate_reward, the logits at il_shapes.TOL (2e-5) relative and absolute and the statistics at 1e-12 /
    1e-9 with an exact count (test_fit_and_reward_shapes, tests/test_gpu_disc_pair.py), the reward within what a logit
    that far off allows plus the float32 steps of the formula, TOL (1 + |d|) + 2e-6
    (test_fit_and_reward_against_the_reference_fixture, same file).  Both sources are masked in the kernel; widths 2, 64 and 34 columns, 16-row tiles with
    one row and with a ragged third tile.  Stored whole: reward, logits, colstats (accumulate 0), stats_a (next states),
    packed."""
    import pair_restate as pr
    from il_shapes import TOL

    def _check_reward(b, tag, d64, what):
        d, r, d64 = b.host(f"{tag}.logits"), b.host(f"{tag}.reward"), d64.cpu().numpy()
        np.testing.assert_allclose(d, d64, rtol=TOL, atol=TOL, err_msg=what)
        r64 = -np.log(1.0 - 1.0 / (1.0 + np.exp(-d64)) + 1e-8)
        assert (np.abs(r - r64) <= TOL * (1 + np.abs(d64)) + 2e-6).all(), what
    (ds, d2), ns = pair, mode == "next_state"
    rng = np.random.default_rng(B + ds)
    Dx, W2 = ds + 3, (ds + 3 if ns else d2 + 2)
    mask = np.sort(rng.choice(Dx, ds, replace=False)).astype(np.int32)
    mask2 = mask if ns else np.sort(rng.choice(W2, d2, replace=False)).astype(np.int32)
    scale = rng.uniform(0.3, 3.0, Dx)
    x = (rng.normal(0, 1, (B, Dx)) * scale + rng.normal(0, 1, Dx)).astype(np.float32)
    x2 = ((0.6 * x + 1.5 * scale + rng.normal(0, 0.5, (B, Dx)) * scale) if ns else rng.normal(0.2, 0.8, (B, W2))).astype(np.float32)
    noise = rng.standard_normal((B, 128)).astype(np.float32)
    params = pr.gen.vail_init(ds + d2, seed=9 + ds)
    b = Bufs()
    xd, x2d, md, nd = b.inp("x", x, gathered=True), b.inp("x2", x2, gathered=True), b.inp("mask", mask), b.inp("eps", noise)
    m2d = md if ns else b.inp("mask2", mask2)
    w = [b.inp(f"w{i}", p) for i, p in enumerate(params)]
    packed = b.out("packed", int(lib().oly_disc_packed_floats(ds + d2, 256, 128, 128)), F32)
    cs, sa = b.out("colstats", (3, ds), F64), b.out("stats_a", (3, ds), F64)
    out = dict(reward=b.out("s.reward", B, F32), logits=b.out("s.logits", B, F32))
    eng.disc_reward_step_pair(xd, x2d, packed, cs, sa, 0, ns, mask=md, mask2=m2d, eps=nd, want=("reward", "logits"), out=out,
                              weights=w)
    names = ("s.reward", "s.logits", "colstats", "packed") + (("stats_a",) if ns else ())
    b.done("disc_reward_step_pair", written=names, finite=names)
    d64, _, cs64 = pr.restate_reward("vail", params, np.zeros((3, ds)), x[:, mask], x2[:, mask2], ns, noise=noise, device="cuda")
    _check_reward(b, "s", d64, "reward step")
    np.testing.assert_allclose(b.host("colstats"), cs64.cpu().numpy(), rtol=1e-12, atol=1e-9)
    assert float(b.host("colstats")[0, 0]) == (2 if ns else 1) * B
    if ns:
        assert float(b.host("stats_a")[0, 0]) == B
    else:
        assert_untouched(dict(stats_a=b["stats_a"]), "actions: stats_a is not touched")
    out = dict(reward=b.out("f.reward", B, F32), logits=b.out("f.logits", B, F32))
    eng.disc_forward_pair(xd, x2d, packed, ns, mask=md, mask2=m2d, stats_a=sa if ns else cs, stats_b=cs if ns else None,
                          eps=nd, want=("reward", "logits"), out=out)
    b.done("disc_forward_pair", written=("f.reward", "f.logits"), finite=("f.reward", "f.logits"))
    _check_reward(b, "f", d64, "forward")


# ------------------------------------------------------------------------------ K9
@pytest.mark.parametrize("B,A,mode,skew", [(1, 3, 1, 0), (64, 12, 0, 0), (65, 16, 2, 0), (5, 64, 1, 0), (64, 12, 0, 4)])
def test_k9_ppo_loss(eng, oracle, B, A, mode, skew):
    """oly_ppo_loss against oracle.ppo_loss at the tolerances of test_ppo_loss_vs_oracle (tests/test_gpu_parity.py): 2e-5
    / 1e-7 on the five scalars, 1e-6 on grad_value, 1e-4 / 1e-9 on grad_mu and grad_std; want_grad and want_grad_std
    both ways.

    Dispatch (k9_ppo_loss.hip): A % 4 == 0, A <= 16 and 16-byte aligned mu / old_mu / action / gradients take
    ppo_loss_rows_kernel<A / 4>, a row in registers: (64, 12) with a scalar std and (65, 16) with a full one, one row
    past a wave.  A = 3 and A = 64 take the generic LDS-tile ppo_loss_kernel (A = 64: 64-row tiles), and so does A = 12
    with mu, old_mu and action one float off.  scal and every requested gradient are stored whole; a gradient that is
    not requested is a NULL pointer, so the Engine allocates nothing for it."""
    rng = np.random.default_rng(B + A + mode)
    c = _ppo_case(rng, B, A, mode)
    names = ("mu", "std", "old_mu", "old_std", "action", "adv", "ret", "value")
    b = Bufs()
    d = [b.inp(k, a, skew=skew if k in ("mu", "old_mu", "action") else 0) for k, a in zip(names, c)]
    scal, gmu, gsd, gv = oracle.ppo_loss(*c, 0.2, 0.5)
    for want_grad in (True, False):
        for want_std in (True, False):
            with fence_engine(eng) as ef:
                r = eng.ppo_loss(*d, 0.2, 0.5, want_grad=want_grad, want_grad_std=want_std)
                engine_done(ef, f"ppo_loss B={B} A={A} grad={want_grad} grad_std={want_std}")
                assert len(ef.bufs) == 1 + 2 * want_grad + want_std
            np.testing.assert_allclose(host(r["scal"]), scal, rtol=2e-5, atol=1e-7)
            assert (r["grad_mu"] is None) == (not want_grad) and (r["grad_std"] is None) == (not want_std)
            if want_grad:
                np.testing.assert_allclose(host(r["grad_value"]), gv, rtol=1e-6, atol=0)
                np.testing.assert_allclose(host(r["grad_mu"]), gmu, rtol=1e-4, atol=1e-9)
            if want_std:
                np.testing.assert_allclose(host(r["grad_std"]), gsd, rtol=1e-4, atol=1e-9)
    b.done(f"ppo_loss B={B} A={A}")


@pytest.mark.parametrize("B,A", [(1, 3), (65, 12)])
def test_k9_mirror_loss_and_signed_perm(eng, oracle, B, A):
    """oly_mirror_loss against oracle.mirror_loss (loss 1e-12 relative, gradients bit-exact) and oly_signed_perm
    bit-exact (+-1 times one input) against oracle.signed_perm, as test_signed_perm_and_mirror_loss
    (tests/test_gpu_parity.py).  One element-wise kernel each; src and sign are fenced, so an index read from a margin
    is -1 and lands in the fenced x's front margin (gathered=True).  loss, both gradients and out are stored whole."""
    rng = np.random.default_rng(B + A)
    src = rng.permutation(A).astype(np.int32)
    sgn = rng.choice([-1.0, 1.0], A).astype(np.float32)
    det, mir = rng.normal(0, 1, (B, A)).astype(np.float32), rng.normal(0, 1, (B, A)).astype(np.float32)
    b = Bufs()
    s_d, g_d = b.inp("src", src), b.inp("sign", sgn)
    with fence_engine(eng) as ef:
        loss, gd, gm = eng.mirror_loss(b.inp("det", det, gathered=True), b.inp("mir", mir, gathered=True), s_d, g_d)
        engine_done(ef, f"mirror_loss B={B} A={A}")
        el, egd, egm = oracle.mirror_loss(det, mir, src, sgn)
        assert float(loss) == pytest.approx(el, rel=1e-12)
        assert np.array_equal(host(gd), egd) and np.array_equal(host(gm), egm)
        l2, n1, n2 = eng.mirror_loss(b["det"].t, b["mir"].t, s_d, g_d, want_grad=False)
        engine_done(ef, "mirror_loss without gradients")
        assert n1 is None and n2 is None and torch.equal(l2, loss)
    out = b.out("out", (B, A), F32)
    eng.signed_perm(b["det"].t, s_d, g_d, out=out)
    b.done(f"signed_perm B={B} A={A}", written=("out",), finite=("out",))
    assert np.array_equal(b.host("out"), oracle.signed_perm(det, src, sgn))


def test_newer_entry_points_refusals_store_nothing(eng):
    """The refusals of test_error_paths_of_the_newer_entry_points (tests/test_gpu_parity.py) that reach an output: the
    caller's poisoned outputs and whatever the Engine allocated before it refused are as they were."""
    z = lambda *s, dt=np.float32: np.zeros(s, dt)
    b = Bufs()
    eng.grf_configure(np.array([0, 1, 2], np.int32), [(0, 1)])
    with fence_engine(eng) as ef:
        with pytest.raises(OlyError, match="force6"):
            eng.il_ground_forces(b.inp("ncon", z(2, 4, dt=np.int32)), b.inp("g1", z(2, 4, 16, dt=np.int32)),
                                 b.inp("g2", z(2, 4, 16, dt=np.int32)), b.inp("f32", z(2, 4, 16, 6)))      # f32 instead of f64
        with pytest.raises(OlyError, match="oly_ppo_loss: bad argument"):
            eng.ppo_loss(b.inp("m65", z(8, 65)), b.inp("s1", z(1)), b["m65"].t, b["s1"].t, b["m65"].t, b.inp("v8", z(8)),
                         b["v8"].t, b["v8"].t, 0.2)                                                          # A > OLY_MAX_ACT
        with pytest.raises(OlyError, match="old_mu"):
            eng.ppo_loss(b.inp("m12", z(8, 12)), b["s1"].t, b.inp("m7", z(7, 12)), b["s1"].t, b["m12"].t, b["v8"].t,
                         b["v8"].t, b["v8"].t, 0.2)
        x = b.inp("x", z(4, 6))
        snap = b["x"].snapshot()
        with pytest.raises(OlyError, match="oly_signed_perm: bad argument"):
            eng.signed_perm(x, b.inp("src", z(6, dt=np.int32)), b.inp("sgn", z(6)), out=x)                   # in place
        assert b["x"].same_as(snap)
        with pytest.raises(OlyError, match="mean"):
            eng.obs_filter(x, b["sgn"].t, b.inp("var", z(6, dt=np.float64)), out=b.out("filtered", (4, 6), F32))   # f32 mean
        with pytest.raises(OlyError, match="parts"):
            eng.adv_normalize(b["v8"].t, b.inp("p65", np.zeros((65, 3))), 1, 1e-5)
        engine_untouched(ef, "refusals")
    # the C layer's own refusals of that test, B = 0 and W = 0, with real (poisoned) output pointers
    L, h = lib(), eng.ctx.handle
    m12, sgn12 = b.inp("c.m12", z(8, 12)), b.inp("c.sgn", z(12))
    outs = [b.out("c.loss", (1,), F64), b.out("c.gd", (8, 12), F32), b.out("c.gm", (8, 12), F32)]
    assert L.oly_mirror_loss(h, 0, 12, ptr(m12), ptr(m12), ptr(b.inp("c.src", z(12, dt=np.int32))), ptr(sgn12),
                             *(ptr(t) for t in outs), eng._s()) == _abi.OLY_EINVAL
    assert b"oly_mirror_loss" in L.oly_last_error(h)
    grf = [b.out("c.steps", (1, 4, 3), F64), b.out("c.mean", (4, 3), F64), b.out("c.over", (4,), U8)]
    assert L.oly_il_ground_forces(h, 0, 4, 16, ptr(b["ncon"].t), ptr(b["g1"].t), ptr(b["g2"].t),
                                  ptr(b.inp("c.f64", z(2, 4, 16, 6, dt=np.float64))), *(ptr(t) for t in grf),
                                  eng._s()) == _abi.OLY_EINVAL
    b.done("refusals")
    assert_untouched({k: b[k] for k in ("filtered", "c.loss", "c.gd", "c.gm", "c.steps", "c.mean", "c.over")}, "refusals")
    assert not b.host("v8").any()


# ------------------------------------------------------------------------------ the host batchers
@pytest.mark.parametrize("N", [1, 33])
def test_host_batcher_step(eng, oracle, N):
    """oly_batcher_set_prev and oly_batcher_step with the built-in kinematic physics against oracle.il_step, as
    test_host_batcher_kinematic_and_callback (tests/test_gpu_facade.py: obs and absorbing bit-exact, reward within
    1 ulp): the device tensors the batcher is handed (prev, action) are fenced, the device outputs it stores (obs,
    reward, absorbing, fall_code) fenced and poisoned, and all four are stored for every environment."""
    from olympic_hip.batcher import HostBatcher
    sp = specs.unitree_h1("walk")
    eng.il_configure(sp)
    qpos, qvel, act = h1_synthetic_block(sp, 3, N, seed=31, fall_frac="wide")
    hb = HostBatcher(eng, N, n_threads=2, dt=0.01, obs_f64=True)
    try:
        hb.qpos[:], hb.qvel[:] = qpos[0], qvel[0]
        prev = np.linspace(0.5, 2.0, N)
        b = Bufs()
        hb.set_prev(b.inp("prev", prev))
        q, v = qpos[0].copy(), qvel[0].copy()
        for t in range(3):
            names = [f"{k}{t}" for k in ("obs", "reward", "absorbing", "fall_code")]
            hb.obs, hb.reward = b.out(names[0], (N, sp.n_obs), F64), b.out(names[1], (N,), F32)
            hb.absorbing, hb.fall_code = b.out(names[2], (N,), U8), b.out(names[3], (N,), U8)
            obs, rew, ab = hb.step(b.inp(f"action{t}", np.ascontiguousarray(act[t], dtype=np.float32)))
            b.done(f"batcher_step N={N} t={t}", written=names, finite=names[:2])
            q = q + 0.01 * v
            assert np.array_equal(hb.qpos, q)
            ref = oracle.il_step(sp, q[None], v[None], None, prev, obs_f64=True)
            assert np.array_equal(host(obs), ref["obs"][0]) and np.array_equal(host(ab), ref["absorbing"][0])
            assert np.array_equal(b.host(names[3]), ref["fall_code"][0])
            assert ulp_diff(host(rew), ref["reward"][0]).max() <= 1
            prev = ref["prev"]
        assert np.array_equal(b.host("prev"), np.linspace(0.5, 2.0, N))
    finally:
        torch.cuda.synchronize()
        hb.close()


@pytest.mark.parametrize("N", [1, 33])
def test_a3_host_batcher_step(eng, golden, N):
    """oly_a3_batcher_step (and oly_a3_batcher_upload with the physics off) replaying the recorded readback of
    a3_task.npz through a Python physics callback, at the bars of test_a3_host_batcher_replays_golden_sequence
    (tests/test_gpu_facade.py: phase and done bit-exact, obs 1e-10 / 1e-11, reward and rew6 2e-6 / 1e-7).  The action
    and every state tensor are fenced, the four outputs fenced and poisoned and stored for every environment."""
    from olympic_hip.batcher import A3HostBatcher
    g = golden("a3_task.npz")
    E, K = g["phase"].shape
    sp = specs.A3Spec(mass=float(g["mass"]))
    eng.a3_configure(sp, g["clock_lut"])
    eng.contact_configure(g["geom_bodyid"], int(g["floor_body"]), int(g["rfoot_body"]), int(g["lfoot_body"]))
    pick = np.arange(N) % E
    st_h, _ = a3_fixture_arrays(g, 0)
    b = Bufs()
    state = {k: b.inp("st." + k, np.ascontiguousarray(v[pick]), gathered=(k == "sequence")) for k, v in st_h.items()}
    C_ = g["geom1"].shape[-1]
    step_no = {"k": 0}

    def physics(e, target, slots):
        k = step_no["k"]
        for n in ("qpos", "qvel", "act_len", "act_vel", "lf_pos", "rf_pos", "lf_vel", "rf_vel", "root_pos", "root_quat",
                  "head_pos", "geom1", "geom2", "force6", "cpos_z"):
            slots[n][...] = g[n][pick[e], k]
        slots["ncon"][0] = g["ncon"][pick[e], k]
    hb = A3HostBatcher(eng, N, C_, physics, n_threads=2, obs_f64=True)
    try:
        act = b.inp("action", np.zeros((N, 12), np.float32))
        for k in range(min(K, 3)):
            step_no["k"] = k
            names = [f"{n}{k}" for n in ("obs", "rew6", "reward", "done")]
            hb.obs, hb.rew6 = b.out(names[0], (N, sp.n_obs), F64), b.out(names[1], (N, 6), F32)
            hb.reward, hb.done = b.out(names[2], (N,), F32), b.out(names[3], (N,), U8)
            obs, rew, done, rew6 = hb.step(act, state)
            b.done(f"a3_batcher_step N={N} k={k}", written=names, finite=names[:3] + ["st.goal"])
            assert np.array_equal(b.host("st.phase"), g["phase"][pick, k])
            assert np.array_equal(host(done).astype(bool), g["done"][pick, k])
            np.testing.assert_allclose(host(obs), g["obs"][pick, k], rtol=1e-10, atol=1e-11)
            np.testing.assert_allclose(host(rew), g["reward"][pick, k], rtol=2e-6, atol=1e-7)
            np.testing.assert_allclose(host(rew6), g["rew6"][pick, k], rtol=2e-6, atol=1e-7)
        # upload() and a step without the physics: the same readback evaluated on a copy of the state
        keep = {n: f.t.clone() for n, f in b.items() if n.startswith("st.")}
        hb.obs = b.out("obs.up", (N, sp.n_obs), F64)
        hb.upload()
        o2, *_ = hb.step(None, state, with_physics=False)
        b.done("a3_batcher_upload", written=("obs.up",), finite=("obs.up",))
        for n, t in keep.items():
            b[n].t.copy_(t)
    finally:
        torch.cuda.synchronize()
        hb.close()
