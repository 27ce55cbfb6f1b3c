"""K10-K14, K23 and K24 on fenced and poisoned buffers (tests/fences.py), at their smallest ragged shapes.

Every case hands every pointer argument as a Fenced tensor (inputs copied in, pure outputs poisoned with 0xFF bytes),
sizes every workspace and packed stream to exactly the number the library reports, compares the results with the
reference and at the tolerance of the kernel's existing test, and then asserts that
  * every margin is intact (no write outside a buffer, the last float of a workspace included),
  * every buffer the header documents as fully written holds no poisoned element (no store forgotten, which a buffer
    from torch's caching allocator can hide behind the previous call's values),
  * no compared output holds a NaN (a read outside an input reads NaN or index -1 from a margin).
Every call is a valid call or a documented refusal that launches nothing."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import a3_reset_draw_restate as R
import bc_log_restate as blr
import bc_restate as br
import fences as fn
from fences import Bufs
from helpers import check_persistent_rollout_against_oracle, ppo_update_case
from olympic_hip import _abi, specs
from olympic_hip._ffi import OlyError, lib
from olympic_hip.synthetic import a3_synthetic_blocks
from olympic_hip.vecstep import REC
from test_gpu_bc_fit import assert_fit_matches_float64
from test_gpu_bc_fit import split as bc_split
from test_gpu_parity import _DISC_KEYS, _disc_weights
from test_gpu_sg_act import assert_logged_fit_matches_float64
from test_gpu_update import oracle_update
from test_gpu_vecstep import CONTACT, _compare, _host_rollout, _to_device
from test_update_cpu import adam_case

pytestmark = pytest.mark.gpu
F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8


@pytest.fixture(scope="module")
def eng():
    from olympic_hip.engine import Engine
    e = Engine(0)
    yield e
    torch.cuda.synchronize()
    e.ctx.close()


def test_the_instrument_on_the_device():
    """Fenced on the GPU as tests/test_fences_cpu.py holds it on the host, through a kernel of torch's."""
    for dtype in (F32, F64, I32, I64, U8):
        f = fn.Fenced((5, 3), dtype)
        assert f.t.is_cuda and f.t.data_ptr() % fn.ALIGN == 0 and f.intact() and f.unwritten() == 15
        f.t[:, :2] = 1
        assert f.intact() and f.unwritten() == 5
        f.buf[fn.MARGIN + f.nbytes:].view(dtype)[0] = 0          # the element behind the last
        assert not f.intact()
    assert bool(torch.isnan(fn.Fenced(3, F32).t).all()) and bool((fn.Fenced(3, I32).t == -1).all())


# ------------------------------------------------------------------------------ K11
def _mlp_net(rng, in_dim, out):
    f = lambda *s: rng.normal(0, 0.4, s).astype(np.float32)
    return [f(256, in_dim), f(256), f(256, 256) * np.float32(0.2), f(256), f(out, 256) * np.float32(0.2), f(out)]


def _pack_fenced(eng, b, tag, net, in_dim, out, mean=None, std=None):
    """oly_mlp_pack of fenced parameters into a fenced, poisoned stream of exactly oly_mlp_packed_floats floats."""
    n = int(lib().oly_mlp_packed_floats(in_dim, 256, out))
    pk = b.out(f"packed_{tag}", n, F32)
    args = [b.inp(f"{tag}.w{i}", a) for i, a in enumerate(net)]
    eng.mlp_pack(*args, b.inp(f"{tag}.mean", mean), b.inp(f"{tag}.std", std), packed=pk)
    return pk


@pytest.mark.parametrize("in_dim,out_a,out_b", [(1, 1, 1), (41, 12, 1), (64, 32, 32)])
def test_k11_pack_and_forward(eng, oracle, in_dim, out_a, out_b):
    """Bit-exact against oracle.mlp_forward, as test_fused_mlp_forward_vs_oracle_and_torch and
    test_fused_mlp_other_dimensions_vs_oracle (tests/test_gpu_vecstep.py) hold it."""
    rng = np.random.default_rng(in_dim * 100 + out_a)
    normalize = in_dim == 41
    na, nb = _mlp_net(rng, in_dim, out_a), _mlp_net(rng, in_dim, out_b)
    mean = rng.normal(0, 0.4, in_dim).astype(np.float32) if normalize else None
    std = rng.uniform(0.5, 1.5, in_dim).astype(np.float32) if normalize else None
    b = Bufs()
    pa = _pack_fenced(eng, b, "a", na, in_dim, out_a, mean, std)
    pb = _pack_fenced(eng, b, "b", nb, in_dim, out_b)
    b.done("mlp_pack", written=("packed_a", "packed_b"), finite=("packed_a", "packed_b"))
    for N in (1, 17, 33):
        x = (rng.normal(0, 1.2, (N, in_dim))).astype(np.float32)
        ya, yb = b.out(f"ya{N}", (N, out_a), F32), b.out(f"yb{N}", (N, out_b), F32)
        eng.mlp_forward2(b.inp(f"x{N}", x), pa, out_a, ya, pb, out_b, yb, normalize_a=normalize)
        b.done(f"mlp_forward2 N={N}", written=(f"ya{N}", f"yb{N}"), finite=(f"ya{N}", f"yb{N}"))
        assert np.array_equal(b.host(f"ya{N}"), oracle.mlp_forward(x, *na, in_mean=mean, in_std=std)), N
        assert np.array_equal(b.host(f"yb{N}"), oracle.mlp_forward(x, *nb)), N
        # one network alone: the second pointer set NULL
        y1 = b.out(f"y1{N}", (N, out_a), F32)
        eng.mlp_forward2(b[f"x{N}"].t, pa, out_a, y1, normalize_a=normalize)
        b.done(f"mlp_forward2 one network N={N}", written=(f"y1{N}",))
        assert torch.equal(y1, ya)


def _child(env_name, rows, select):
    """The selected tests of this file in a fresh pytest process with env_name=rows.  Like the existing tile-height
    children, this holds both settings to the same oracle; it cannot tell whether the variable took effect, and would
    pass twice on the default choice if the library stopped reading it."""
    env = dict(os.environ, **{env_name: str(rows)})
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k", select,
                          "-p", "no:cacheprovider"], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert " passed" in out.stdout and "no tests ran" not in out.stdout, out.stdout[-500:]


@pytest.mark.parametrize("rows", [16, 32])
def test_k11_both_tile_heights(rows):
    """OLY_K11_ROWS forces one tile height onto every K11 case of this file; the variable is read once per process, hence
    the child (as test_fused_mlp_both_tile_heights_on_every_case, tests/test_gpu_vecstep.py)."""
    _child("OLY_K11_ROWS", rows, "k11_pack_and_forward")


# ------------------------------------------------------------------------------ K12, the plain paths
def _disc_pack_fenced(eng, b, w, D):
    n = int(lib().oly_disc_packed_floats(D, 256, 128, 128))
    pk = b.out("packed", n, F32)
    eng.disc_pack(*[b.inp("w." + k, w[k]) for k in _DISC_KEYS], packed=pk)
    b.done("disc_pack", written=("packed",), finite=("packed",))
    return pk


WANT = ("reward", "logits", "mu", "logvar")
SHAPES12 = dict(reward=lambda B: (B,), logits=lambda B: (B,), mu=lambda B: (B, 128), logvar=lambda B: (B, 128))


def _disc_forward_case(eng, oracle, B, Dx, D, stats):
    """One case of test_disc_forward_vs_oracle (tests/test_gpu_parity.py), fenced: every output BIT-EXACT."""
    rng = np.random.default_rng(B * 131 + D)
    w = _disc_weights(rng, D)
    x = rng.normal(0.3, 2.0, (B, Dx)).astype(np.float32)
    mask = None if D == Dx else np.sort(rng.choice(Dx, D, replace=False)).astype(np.int32)
    eps = rng.normal(0, 1, (B, 128)).astype(np.float32)
    b = Bufs()
    kw, okw = {}, {}
    if stats == "meanstd":
        mean, std = rng.normal(0.3, 0.2, D), rng.uniform(0.5, 2.5, D)
        kw, okw = dict(mean=b.inp("mean", mean), std=b.inp("std", std)), dict(mean=mean, std=std)
    elif stats == "colstats":
        xm = x if mask is None else x[:, mask]
        cs = np.stack([np.full(D, float(B)), xm.astype(np.float64).sum(0), (xm.astype(np.float64) ** 2).sum(0)])
        kw, okw = dict(colstats=b.inp("colstats", cs)), dict(colstats=cs)
    packed = _disc_pack_fenced(eng, b, w, D)
    xd, md = b.inp("x", x), b.inp("mask", mask)
    for tag, e in (("noise", eps), ("mean", None)):
        out = {k: b.out(f"{tag}.{k}", SHAPES12[k](B), F32) for k in WANT}
        eng.disc_forward(xd, packed, mask=md, eps=b.inp(f"{tag}.eps", e), want=WANT, out=out, **kw)
        names = [f"{tag}.{k}" for k in WANT]
        b.done(f"disc_forward {tag}", written=names, finite=names)
        ref = oracle.disc_forward(x, w, mask=mask, eps=e, **okw)
        for k in WANT:
            assert np.array_equal(b.host(f"{tag}.{k}"), ref[k]), (k, tag)
    # the reward alone: the three other output pointers NULL
    r = b.out("alone", (B,), F32)
    eng.disc_forward(xd, packed, mask=md, eps=b["noise.eps"].t, out=dict(reward=r), **kw)
    b.done("disc_forward reward alone", written=("alone",))
    assert torch.equal(r, b["noise.reward"].t)


@pytest.mark.parametrize("stats", ["meanstd", "colstats", "none"])
@pytest.mark.parametrize("B", [1, 31, 33])
def test_k12_disc_forward(eng, oracle, B, stats):
    _disc_forward_case(eng, oracle, B, 32, 32, stats)


def test_k12_disc_forward_masked(eng, oracle):
    """Dx > D: 30 of 36 columns through an int32 mask, whose margins hold -1."""
    _disc_forward_case(eng, oracle, 33, 36, 30, "colstats")


@pytest.mark.parametrize("B", [1, 31, 33])
def test_k12_disc_reward_step(eng, oracle, B):
    """oly_disc_reward_step, accumulate 0 then 1, on a fenced float64 colstats: the statistics against oracle.col_stats
    at test_col_stats' 1e-12 (tests/test_gpu_parity.py), the forward on them bit-exact against oracle.disc_forward as
    test_disc_forward_vs_oracle holds it."""
    D = 32
    rng = np.random.default_rng(B + 7)
    w = _disc_weights(rng, D)
    b = Bufs()
    packed = _disc_pack_fenced(eng, b, w, D)
    cs = b.out("colstats", (3, D), F64)              # accumulate = 0 overwrites it: a pure output of the first call
    want_cs = None
    for acc in (0, 1):
        x = rng.normal(0.3, 2.0, (B, D)).astype(np.float32)
        eps = rng.normal(0, 1, (B, 128)).astype(np.float32)
        out = {k: b.out(f"{acc}.{k}", SHAPES12[k](B), F32) for k in WANT}
        eng.disc_reward_step(b.inp(f"{acc}.x", x), packed, cs, acc, eps=b.inp(f"{acc}.eps", eps), want=WANT, out=out)
        names = [f"{acc}.{k}" for k in WANT]
        b.done(f"disc_reward_step accumulate={acc}", written=names + ["colstats"], finite=names + ["colstats"])
        want_cs = oracle.col_stats(x) if want_cs is None else want_cs + oracle.col_stats(x)
        got_cs = b.host("colstats")
        np.testing.assert_allclose(got_cs, want_cs, rtol=1e-12)
        ref = oracle.disc_forward(x, w, colstats=got_cs, eps=eps)
        for k in WANT:
            assert np.array_equal(b.host(f"{acc}.{k}"), ref[k]), (k, acc)
    assert float(b.host("colstats")[0, 0]) == 2 * B


@pytest.mark.parametrize("rows", [16, 32])
def test_k12_both_tile_heights(rows):
    """OLY_K12_ROWS forces one tile height onto every K12 case of this file, in a child process (as
    test_disc_forward_both_tile_heights_on_every_case, tests/test_gpu_parity.py)."""
    _child("OLY_K12_ROWS", rows, "k12_disc")


# ------------------------------------------------------------------------------ K10
# what a RESET_ALL and T steps write whole: poisoned.  Everything else holds _host_rollout's start values.
K10_OUTPUTS = ("ro.buf_states", "ro.buf_actions", "ro.buf_rewards", "ro.buf_values", "ro.buf_flags", "ro.buf_rew6",
               "ro.pd_target")
# the observation: poisoned too, but held to "written whole" after RESET_ALL only, since the step loop then copies the
# oracle's observation over it before every launch (as test_vec_step_vs_oracle does)
K10_RESET_OUTPUTS = ("ro.state",)


def _k10_put(b):
    def put(name, a):
        if name in K10_OUTPUTS + K10_RESET_OUTPUTS:
            return b.out(name, a.shape, torch.as_tensor(a[:0]).dtype)
        return b.inp(name, a)
    return put


def _k10_run(eng, oracle, golden, N, T, max_len, K, det, blocks_of=None, p_bad=0.05):
    spec = specs.A3Spec(mass=41.5)
    lut = golden("a3_task.npz")["clock_lut"]
    eng.a3_configure(spec, lut)
    eng.contact_configure(*CONTACT)
    blocks, state, ro, rng = _host_rollout(spec, N, K, T, max_len, 2, seed=N + T, det=det, p_bad=p_bad)
    if blocks_of is not None:
        blocks = blocks_of(rng)
    b = Bufs()
    d_blocks, d_state, d_ro = _to_device(eng, blocks, state, ro, put=_k10_put(b))
    launch = eng.a3_vec_prepare(d_blocks, d_state, d_ro)
    launch(_abi.VSTEP_RESET_ALL)
    oracle.a3_vec_step(spec, lut, CONTACT, blocks, state, ro, _abi.VSTEP_RESET_ALL)
    b.done("RESET_ALL", written=K10_RESET_OUTPUTS, finite=K10_RESET_OUTPUTS)
    for t in range(T):
        mu = rng.normal(0, 0.3, (N, spec.nu)).astype(np.float32)
        val = rng.normal(0, 1, N).astype(np.float32)
        ro["mu"][...], ro["value"][...] = mu, val
        d_ro["state"].copy_(torch.as_tensor(ro["state"]).cuda())          # both sides on the oracle's observation
        launch(0, b.inp(f"mu{t}", mu), b.inp(f"value{t}", val))
        oracle.a3_vec_step(spec, lut, CONTACT, blocks, state, ro, 0)
        b.done(f"step {t}")
    return b, d_blocks, d_state, d_ro, blocks, state, ro, launch


@pytest.mark.parametrize("det", [False, True], ids=["stochastic", "deterministic"])
@pytest.mark.parametrize("N", [1, 37, 65])
def test_k10_vec_step(eng, oracle, golden, N, det):
    """RESET_ALL + T steps against oracle.a3_vec_step with the comparisons of test_vec_step_vs_oracle
    (tests/test_gpu_vecstep.py: _compare), then one launch past the last row, which the library defines as "writes
    nothing and is reported" (test_a_step_past_the_last_row_writes_nothing_and_is_reported): every fenced buffer,
    margins included, equals its copy from before the launch byte for byte, but for the overrun mark in ctr."""
    T = 3
    b, d_blocks, d_state, d_ro, blocks, state, ro, launch = _k10_run(eng, oracle, golden, N, T, 2, 5, det)
    _compare(d_state, d_ro, state, ro, "end")
    assert ro["ctr"].tolist() == [T, 3 + T]
    b.done("the rollout", written=K10_OUTPUTS, finite=K10_OUTPUTS + ("state.goal", "state.sequence", "ro.side_obs"))
    snap = {k: f.snapshot() for k, f in b.items()}
    launch(0)                                                            # t == T
    torch.cuda.synchronize()
    c = b.host("ro.ctr").reshape(-1, 2)
    assert c[-1, 0] == 1 and (c[:-1, 0] == T).all()
    d_ro["ctr"][-2] = 0
    changed = [k for k, f in b.items() if not f.same_as(snap[k])]
    assert not changed, f"a launch past the last row wrote {changed}"


def test_k10_more_than_sixteen_contact_slots(eng, oracle, golden):
    """C = 20 contact slots, up to all of them in use, as test_vec_step_more_than_sixteen_contact_slots."""
    N, T, C20 = 37, 3, 20

    def blocks_of(rng):
        b20 = a3_synthetic_blocks(N, 3, seed=9, C=C20, p_bad=0.3, p_low=0.02)
        b20["ncon"] = rng.integers(0, C20 + 1, b20["ncon"].shape).astype(np.int32)
        return b20
    b, d_blocks, d_state, d_ro, blocks, state, ro, _ = _k10_run(eng, oracle, golden, N, T, 2, 3, True, blocks_of)
    assert (blocks["ncon"] > 16).any()
    _compare(d_state, d_ro, state, ro, "end")
    b.done("20 contact slots", written=K10_OUTPUTS, finite=K10_OUTPUTS)


# ------------------------------------------------------------------------------ K13
K13_OUTPUTS = ("ro.buf_states", "ro.buf_actions", "ro.buf_rewards", "ro.buf_values", "ro.buf_flags", "ro.buf_mu",
               "ro.pd_target", "ro.state", "packed_actor", "packed_critic", "mu_out", "value_out")


@pytest.mark.parametrize("N,T,max_len,det,normalize", [(16, 5, 3, True, False), (70, 6, 2, False, True)])
def test_k13_persistent_rollout(eng, oracle, N, T, max_len, det, normalize):
    """oly_a3_rollout_persistent: the set-up and the bars of test_persistent_rollout_against_the_oracle_directly
    (helpers.check_persistent_rollout_against_oracle), every buffer fenced and the pure outputs poisoned."""
    b = Bufs()

    def put(name, a):
        if name in K13_OUTPUTS:
            return b.out(name, a.shape, torch.as_tensor(a[:0]).dtype)
        return b.inp(name, a)
    check_persistent_rollout_against_oracle(eng, oracle, N=N, T=T, max_len=max_len, det=det, normalize=normalize,
                                            seed=N + T, put=put)
    assert set(K13_OUTPUTS) <= set(b)
    b.done("persistent rollout", written=K13_OUTPUTS,
           finite=K13_OUTPUTS + ("state.goal", "state.sequence", "ro.side_obs"))


# ------------------------------------------------------------------------------ K14
def _k14_buffers(eng, c, idx, mirror, ws_short=0):
    """Every operand of oly_ppo_update_grads for the case c, fenced; ws of the plan's floats less ws_short."""
    in_dim, act_dim = c["obs"].shape[1], c["action"].shape[1]
    b = Bufs()
    pa = _pack_fenced(eng, b, "actor", c["actor"], in_dim, act_dim, c["a_mean"], c["a_std"])
    pc = _pack_fenced(eng, b, "critic", c["critic"], in_dim, 1)
    B = len(idx) if idx is not None else len(c["obs"])
    ws_n, p_a, p_c = eng.ppo_update_plan(B, in_dim, act_dim, mirror)
    ga = b.out("grad_actor", int(lib().oly_ppo_update_grad_floats(in_dim, 256, act_dim)), F32)
    gc = b.out("grad_critic", int(lib().oly_ppo_update_grad_floats(in_dim, 256, 1)), F32)
    scal, ws, gn = b.out("scal", 6, F64), b.out("ws", ws_n - ws_short, F32), b.out("gnorm_ws", 1024, F64)
    sd, lsd = b.inp("sd", c["sd"]), b.inp("log_sd", c["log_sd"])
    kw = {}
    if mirror:
        kw = dict(mir_obs=b.inp("mir_obs", c["mir_obs"], gathered=True), act_src=b.inp("act_src", c["act_src"]),
                  act_sign=b.inp("act_sign", c["act_sign"]))
    args = (b.inp("obs", c["obs"], gathered=True), b.inp("action", c["action"], gathered=True), b.inp("adv", c["adv"]),
            b.inp("ret", c["ret"]), b.inp("old_mu", c["old_mu"], gathered=True), pa, pc, sd, lsd, sd, lsd, ga, gc, scal, ws)
    kw.update(idx=b.inp("idx", idx), normalize_actor=c["a_mean"] is not None, clip=0.2, vf_coeff=0.5, mirror_coeff=0.4,
              gnorm_ws=gn)
    return b, args, kw, (p_a, p_c)


K14_OUT = ("grad_actor", "grad_critic", "scal")


def _k14_case(eng, oracle, c, idx, mirror, parts):
    """Gradients BIT-EXACT against the oracle twin, the six scalars to 1e-12, as test_ppo_update_kernel_equals_the_oracle
    (tests/test_gpu_update.py)."""
    b, args, kw, plan = _k14_buffers(eng, c, idx, mirror)
    eng.ppo_update_grads(*args, parts=parts, **kw)
    b.done("ppo_update_grads", written=K14_OUT + ("packed_actor", "packed_critic"), finite=K14_OUT)
    oa, oc, os_ = oracle_update(oracle, c, idx, mirror, parts if parts != (0, 0) else plan)
    assert np.array_equal(b.host("grad_actor"), oa), np.abs(b.host("grad_actor") - oa).max()
    assert np.array_equal(b.host("grad_critic"), oc), np.abs(b.host("grad_critic") - oc).max()
    np.testing.assert_allclose(b.host("scal"), os_, rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("n,B,mirror,parts", [(5, None, False, (0, 0)), (96, 50, True, (2, 1)), (200, 131, False, (3, 4))])
def test_k14_update_grads_ragged_and_gathered(eng, oracle, n, B, mirror, parts):
    """The ragged and gathered rows of test_gpu_update.CASES, the workspace of exactly oly_ppo_update_ws_floats floats.
    With explicit parts, (2, 1) and (3, 4), a launch uses less than that plan-sized workspace, so its back fence does not
    sit where these launches end: the exact fit is held by the (5, all) case here, by the widths below and by the epoch."""
    c = ppo_update_case(100 + n, n=n, mirror=mirror, normalize=True)
    idx = None if B is None else np.random.default_rng(n).permutation(n)[:B].astype(np.int32)
    _k14_case(eng, oracle, c, idx, mirror, parts)


@pytest.mark.parametrize("in_dim,act_dim,mirror", [(10, 3, True), (49, 7, False), (64, 16, True)])
def test_k14_update_grads_widths(eng, oracle, in_dim, act_dim, mirror):
    """Three instantiations of the kernel with the plan's own split: the workspace is then exactly what the launch
    asks for.  The statistics partials end 4 floats before its end (the reported size carries 4 floats behind them that
    no launch writes), so a partial stored one slot too far still reaches the fence: a slot is 2 floats per statistic."""
    c = ppo_update_case(in_dim + act_dim, n=70, in_dim=in_dim, act_dim=act_dim, mirror=mirror)
    idx = np.random.default_rng(3).permutation(70)[:53].astype(np.int32)
    _k14_case(eng, oracle, c, idx, mirror, (0, 0))


def test_k14_a_workspace_one_float_short_is_refused_and_nothing_is_launched(eng):
    c = ppo_update_case(1, n=40, mirror=False)
    b, args, kw, _ = _k14_buffers(eng, c, None, False, ws_short=1)
    with pytest.raises(OlyError, match="workspace"):
        eng.ppo_update_grads(*args, **kw)
    torch.cuda.synchronize()
    fn.assert_untouched({k: b[k] for k in K14_OUT + ("ws", "gnorm_ws")}, "refused ppo_update_grads")
    fn.assert_intact(b, "refused ppo_update_grads")


def _flat(arrays):
    return np.concatenate([np.asarray(a, np.float32).reshape(-1) for a in arrays])


def _unflat(p, in_dim, out):
    cuts = np.cumsum([256 * in_dim, 256, 65536, 256, out * 256])
    shapes = [(256, in_dim), (256,), (256, 256), (256,), (out, 256), (out,)]
    return [a.reshape(s) for a, s in zip(np.split(p, cuts), shapes)]


def _fresh_pack(eng, param, in_dim, out, mean=None, std=None):
    parts = [a.contiguous() for a in torch.split(param, [256 * in_dim, 256, 65536, 256, out * 256, out])]
    return eng.mlp_pack(parts[0].view(256, in_dim), parts[1], parts[2].view(256, 256), parts[3], parts[4].view(-1, 256),
                        parts[5], mean, std)


def _adam_nets(eng, b, params, in_dim, outs, mean, std):
    """The two network blocks of oly_ppo_adam_step on fenced buffers: the gradients poisoned, the packed streams poisoned
    and then written by oly_mlp_pack from the same parameters, as KernelUpdate.begin leaves them (the optimiser launch
    writes the stepped weights and the tables to their places and leaves the zero padding alone)."""
    nets = []
    for tag, p0, out in zip(("actor", "critic"), params, outs):
        z = np.zeros_like(p0)
        nt = dict(param=b.inp(tag + ".param", p0), grad=b.out(tag + ".grad", len(p0), F32),
                  exp_avg=b.inp(tag + ".m", z), exp_avg_sq=b.inp(tag + ".v", z), out_dim=out,
                  packed=b.out(tag + ".packed", int(lib().oly_mlp_packed_floats(in_dim, 256, out)), F32),
                  in_mean=b.inp(tag + ".mean", mean if tag == "actor" else None),
                  in_std=b.inp(tag + ".std", std if tag == "actor" else None))
        w = [b.inp(f"{tag}.w{i}", a) for i, a in enumerate(_unflat(p0, in_dim, out))]
        eng.mlp_pack(*w, nt["in_mean"], nt["in_std"], packed=nt["packed"])
        nets.append(nt)
    b.done("mlp_pack", written=("actor.packed", "critic.packed"), finite=("actor.packed", "critic.packed"))
    return nets


ADAM_STATE = tuple(f"{t}.{k}" for t in ("actor", "critic") for k in ("param", "m", "v", "packed"))


def test_k14_adam_step(eng, oracle):
    """oly_ppo_adam_step, four steps: parameters and both moments BIT-EXACT against the oracle twin and the packed
    stream equal to a fresh oly_mlp_pack of the stepped parameters, as test_ppo_adam_step_equals_the_oracle_and_torch
    (tests/test_gpu_update.py); that also shows the zero padding of the streams untouched."""
    sizes = (int(lib().oly_ppo_update_grad_floats(41, 256, 12)), int(lib().oly_ppo_update_grad_floats(41, 256, 1)))
    cases = [adam_case(5 + i, n=n) for i, n in enumerate(sizes)]
    mean, std = np.linspace(-1, 1, 41, dtype=np.float32), np.linspace(0.5, 2, 41, dtype=np.float32)
    b = Bufs()
    nets = _adam_nets(eng, b, [c[0] for c in cases], 41, (12, 1), mean, std)
    ws = b.out("gnorm_ws", 1024, F64)
    ref = [(c[0].copy(), np.zeros_like(c[0]), np.zeros_like(c[0])) for c in cases]
    for t in range(4):
        for nt, c in zip(nets, cases):
            nt["grad"].copy_(torch.as_tensor(c[1][t]))
        eng.ppo_adam_step(41, t + 1, 1e-4, 1e-5, 0.05, nets, ws)
        ref = [oracle.ppo_adam_step(r[0], c[1][t], r[1], r[2], t + 1, 1e-4, eps=1e-5, max_norm=0.05) for r, c in zip(ref, cases)]
        b.done(f"adam step {t + 1}", written=ADAM_STATE, finite=ADAM_STATE)
    for tag, nt, r in zip(("actor", "critic"), nets, ref):
        for k, want in zip(("param", "m", "v"), r):
            assert np.array_equal(b.host(f"{tag}.{k}"), want), (tag, k)
        fresh = _fresh_pack(eng, nt["param"], 41, nt["out_dim"], nt["in_mean"], nt["in_std"])
        assert torch.equal(fresh, nt["packed"]), tag


def test_k14_update_epoch(eng, oracle):
    """oly_ppo_update_epoch, four minibatches of 100 gathered rows with the mirror loss, against the chain of the two
    oracle twins (ppo_update on the parameters as stepped so far, then ppo_adam_step): scalars to 1e-12 and the final
    parameters, moments and gradients BIT-EXACT, the bars of test_ppo_update_kernel_equals_the_oracle and
    test_ppo_adam_step_equals_the_oracle_and_torch; the streams equal a fresh oly_mlp_pack of the stepped parameters.
    perm holds exactly n_batches * B indices: an index read behind them is -1 and gathers NaN from a front margin."""
    B, n_batches, n, in_dim, act_dim = 100, 4, 450, 41, 12
    lr, eps, max_norm = 1e-3, 1e-5, 0.05
    c = ppo_update_case(31, n=n, mirror=True)
    perm = np.random.default_rng(31).permutation(n)[:n_batches * B].astype(np.int32)
    b = Bufs()
    params = [_flat(c["actor"]), _flat(c["critic"])]
    nets = _adam_nets(eng, b, params, in_dim, (act_dim, 1), c["a_mean"], c["a_std"])
    ws_n, p_a, p_c = eng.ppo_update_plan(B, in_dim, act_dim, True)
    ws, gn = b.out("ws", ws_n, F32), b.out("gnorm_ws", 1024, F64)
    scal = b.out("scal", (n_batches, 6), F64)
    pd = b.inp("perm", perm)
    sd, lsd = b.inp("sd", c["sd"]), b.inp("log_sd", c["log_sd"])
    gl = eng.ppo_update_grads(b.inp("obs", c["obs"], gathered=True), b.inp("action", c["action"], gathered=True),
                              b.inp("adv", c["adv"]), b.inp("ret", c["ret"]), b.inp("old_mu", c["old_mu"], gathered=True),
                              nets[0]["packed"], nets[1]["packed"], sd, lsd, sd, lsd, nets[0]["grad"], nets[1]["grad"],
                              scal[0], ws, idx=pd[:B], mir_obs=b.inp("mir_obs", c["mir_obs"], gathered=True),
                              act_src=b.inp("act_src", c["act_src"]), act_sign=b.inp("act_sign", c["act_sign"]),
                              normalize_actor=True, clip=0.2, vf_coeff=0.5, mirror_coeff=0.4, gnorm_ws=gn, prepare=True)
    al = eng.ppo_adam_step(in_dim, 1, lr, eps, max_norm, nets, gn, prepare=True)
    torch.cuda.synchronize()
    fn.assert_untouched({k: b[k] for k in ("actor.grad", "critic.grad", "scal", "ws", "gnorm_ws")}, "prepare launches nothing")
    eng.ppo_update_epoch(gl, al, 1, pd, n_batches, scal)
    state = ADAM_STATE + ("actor.grad", "critic.grad", "scal")
    b.done("ppo_update_epoch", written=state, finite=state)
    ref = [(p.copy(), np.zeros_like(p), np.zeros_like(p)) for p in params]
    for k in range(n_batches):
        cur = dict(c, actor=_unflat(ref[0][0], in_dim, act_dim), critic=_unflat(ref[1][0], in_dim, 1))
        grads = oracle_update(oracle, cur, perm[k * B:(k + 1) * B], True, (p_a, p_c))
        np.testing.assert_allclose(b.host("scal")[k], grads[2], rtol=1e-12, atol=1e-15, err_msg=f"minibatch {k}")
        ref = [oracle.ppo_adam_step(r[0], g, r[1], r[2], 1 + k, lr, eps=eps, max_norm=max_norm) for r, g in zip(ref, grads[:2])]
    for tag, nt, r, g in zip(("actor", "critic"), nets, ref, grads[:2]):
        assert np.array_equal(b.host(tag + ".grad"), g), (tag, "the last minibatch's gradient")
        for k, want in zip(("param", "m", "v"), r):
            assert np.array_equal(b.host(f"{tag}.{k}"), want), (tag, k)
        fresh = _fresh_pack(eng, nt["param"], in_dim, nt["out_dim"], nt["in_mean"], nt["in_std"])
        assert torch.equal(fresh, nt["packed"]), tag
    assert float(np.abs(b.host("scal")[:, 3]).max()) > 0                   # the policy moved between minibatches


# ------------------------------------------------------------------------------ K23
@pytest.mark.parametrize("depth", [1, 33])
@pytest.mark.parametrize("N", [1, 63, 65])
def test_k23_reset_draw(eng, N, depth):
    """Byte for byte against a3_reset_draw_restate, the calls of test_kernel_equals_the_restatement
    (tests/test_gpu_a3_reset_draw.py), into a fenced and poisoned pool."""
    seed, period, isz = 0xC0FFEE1234567891, 88, REC.itemsize
    base0 = np.array([0, 5, 2 ** 32 - 1, 2 ** 32 + 7], dtype=np.int64)[np.arange(N) % 4]
    consumed = ((np.arange(N) * 7) % 5 + (np.arange(N) == 0)).astype(np.int32)
    h = R.step_height(7000)
    b = Bufs()
    pool, base, count = b.out("pool", N * depth * isz, U8), b.inp("base", base0), b.inp("count", consumed)

    def poisoned_records():
        return int((b["pool"].bytes.view(N * depth, isz) == fn.POISON).all(dim=1).sum())
    assert poisoned_records() == N * depth
    eng.a3_reset_draw(pool, base, None, depth, seed, h, period)             # pool_count NULL: base as it is
    b.done("pool_count NULL")
    assert poisoned_records() == 0 and np.array_equal(b.host("base"), base0)
    assert b.host("pool").tobytes() == R.ring(seed, base0, depth, period, h).tobytes()
    pool.fill_(fn.POISON)
    eng.a3_reset_draw(pool, base, count, depth, seed, h, period)            # consumed records: the ring moves on
    b.done("advanced")
    assert poisoned_records() == 0 and np.array_equal(b.host("base"), base0 + consumed) and not b.host("count").any()
    assert b.host("pool").tobytes() == R.ring(seed, base0 + consumed, depth, period, h).tobytes()


# ------------------------------------------------------------------------------ K24
def _bc_buffers(eng, c, k, ws_floats, out_cols, eps=None):
    """The operands of oly_bc_fit_steps(_log) for case c, fenced: ws of exactly ws_floats floats, out poisoned."""
    b = Bufs()
    param = b.inp("param", br.flat(k["params"]).astype(np.float32))
    st = dict(param=param, m=b.inp("m", np.zeros(param.numel(), np.float32)), v=b.inp("v", np.zeros(param.numel(), np.float32)),
              colstats=b.inp("colstats", np.zeros((3, c.in_dim))) if c.standardizer else None,
              out=b.out("out", (c.steps, out_cols), F64))
    npk = int(lib().oly_ilmlp_packed_floats(c.in_dim, 512, 256, 2 * c.A))
    st["packed"] = eng.ilmlp_pack(*bc_split(param, c.in_dim, c.A), packed=b.out("packed", npk, F32))
    args = (b.inp("states", k["states"], gathered=True), b.inp("targets", k["targets"], gathered=True), b.inp("idx", k["idx"]),
            st["colstats"], param, st["m"], st["v"], st["packed"], b.out("ws", ws_floats, F32))
    if eps is not None:
        b.inp("noise", eps)
    b.done("ilmlp_pack", written=("packed",), finite=("packed",))
    return b, st, args


BC_STATE = ("param", "m", "v", "packed")


@pytest.mark.parametrize("c", br.CASES, ids=[br.case_id(c) for c in br.CASES])
def test_k24_fit(eng, c):
    """Every row of bc_restate.CASES against the float64 restatement at bc_restate.TOL, by test_fit_against_float64's
    own comparison (tests/test_gpu_bc_fit.py), with a workspace of exactly oly_bc_fit_ws floats."""
    k, ref = br.yardstick(c)
    b, st, args = _bc_buffers(eng, c, k, int(lib().oly_bc_fit_ws(k["batch"], c.in_dim, c.A)), 3)
    eng.bc_fit_steps(*args, 0, c.lr, log_std_min=br.LOG_STD_MIN, log_std_max=br.LOG_STD_MAX, nll_eps=br.NLL_EPS, out=st["out"])
    state = BC_STATE + ("out",) + (("colstats",) if c.standardizer else ())
    b.done("bc_fit_steps", written=state, finite=state)
    assert_fit_matches_float64(eng, c, st, ref)


@pytest.mark.parametrize("c", blr.RUNS[:2], ids=[br.case_id(c) for c in blr.RUNS[:2]])
def test_k24_logged_fit(eng, golden, c):
    """The two smallest runs of bc_log_restate.RUNS at the tolerances of test_logged_fit_against_float64
    (tests/test_gpu_sg_act.py), the workspace of exactly oly_bc_fit_log_ws floats (the log_prob rows are its last), the
    noise fenced.  Column 3 of a step that does not log is documented as not written: exactly those stay poisoned."""
    k = br.build(c)
    li = blr.logging_iter_of(c)
    eps = blr.noise(c, li)
    ref = blr.restate(c.in_dim, c.A, k, c.steps, c.lr, c.standardizer, eps, li)
    b, st, args = _bc_buffers(eng, c, k, int(lib().oly_bc_fit_log_ws(k["batch"], c.in_dim, c.A)), 4, eps=eps)
    eng.bc_fit_steps_log(*args, 0, c.lr, li, 0, b["noise"].t, log_std_min=br.LOG_STD_MIN, log_std_max=br.LOG_STD_MAX,
                         nll_eps=br.NLL_EPS, out=st["out"])
    state = BC_STATE + (("colstats",) if c.standardizer else ())
    b.done("bc_fit_steps_log", written=state, finite=state)
    logged = blr.logged_steps(c.steps, li)
    assert b["out"].unwritten() == c.steps - len(logged)
    out = b.host("out")
    assert not np.isnan(out[:, :3]).any() and not np.isnan(out[logged, 3]).any()
    assert_logged_fit_matches_float64(c, k, li, st, ref, float(golden("bc_log/bc_log.npz")["ent_spread"]))


def _assert_targets(got, actions, central, delta):
    """oly_bc_targets' table against float64 atanh of the float32 clipped argument, at two float32 ulps: the bound of
    test_targets_against_torch (tests/test_gpu_bc_fit.py), `np.abs(got - ref64) <= 2 * ulp`."""
    u = torch.clip((torch.as_tensor(actions) - torch.as_tensor(central)) / torch.as_tensor(delta), -1.0 + 1e-7, 1.0 - 1e-7)
    ref64 = torch.arctanh(u.double()).numpy()
    ulp = np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(got.astype(np.float64) - ref64) <= 2 * ulp)


@pytest.mark.parametrize("n", [1, 17])
def test_k24_targets(eng, n):
    """oly_bc_targets into a poisoned table, against float64 atanh at two float32 ulps and the exact values on and
    beyond the bounds, as test_targets_against_torch (tests/test_gpu_bc_fit.py)."""
    rng = np.random.default_rng(11 + n)
    A = 5
    min_a, max_a = -rng.uniform(0.5, 2.0, A), rng.uniform(0.5, 3.0, A)
    central, delta = (0.5 * (max_a + min_a)).astype(np.float32), (0.5 * (max_a - min_a)).astype(np.float32)
    a = (central + delta * np.tanh(rng.standard_normal((n, A)))).astype(np.float32)
    a[0, 0], a[0, 1], a[-1, 2], a[-1, 3] = np.float32(max_a[0]) + 0.5, np.float32(min_a[1]) - 0.5, central[2], np.float32(max_a[3])
    b = Bufs()
    got = eng.bc_targets(b.inp("actions", a), b.inp("central", central), b.inp("delta", delta), out=b.out("targets", (n, A), F32))
    b.done("bc_targets", written=("targets",), finite=("targets",))
    got = got.cpu().numpy()
    top = np.float32(np.arctanh(np.float64(br.CLIP)))
    assert got[0, 0] == top and got[0, 1] == -top and got[-1, 2] == 0.0
    _assert_targets(got, a, central, delta)


def test_k24_refusals_launch_nothing(eng):
    """Straight at the C entries, which take the workspace's size from the caller: the unlogged fit's workspace handed
    to the logged entry (as test_logged_fit_refusals, tests/test_gpu_sg_act.py), and one float less than oly_bc_fit_ws
    handed to the unlogged one.  Both are refused for the workspace (the shared check's message, "ws (N floats) ...", so
    that a mistake in the argument block built here cannot pass for it), leave every poisoned float poisoned, the
    parameters as they were and every margin intact."""
    c = br.CASES[1]
    k = br.build(c)
    n_fit, n_log = int(lib().oly_bc_fit_ws(k["batch"], c.in_dim, c.A)), int(lib().oly_bc_fit_log_ws(k["batch"], c.in_dim, c.A))
    assert 0 < n_fit < n_log
    for entry, floats, cols in (("oly_bc_fit_steps_log", n_fit, 4), ("oly_bc_fit_steps", n_fit - 1, 3)):
        eps = blr.noise(c, 1) if cols == 4 else None
        b, st, args = _bc_buffers(eng, c, k, floats, cols, eps=eps)
        snap = {name: b[name].snapshot() for name in BC_STATE}
        fit = _abi.BCFit(in_dim=c.in_dim, act_dim=c.A, batch=k["batch"], n_rows=c.n_rows, step=0, lr=c.lr, beta1=0.9, beta2=0.999,
                         eps=1e-8, weight_decay=0.0, log_std_min=br.LOG_STD_MIN, log_std_max=br.LOG_STD_MAX, nll_eps=br.NLL_EPS,
                         states=args[0].data_ptr(), targets=args[1].data_ptr(), idx=args[2].data_ptr(), colstats=None,
                         param=args[4].data_ptr(), m=args[5].data_ptr(), v=args[6].data_ptr(), packed=args[7].data_ptr(),
                         ws=args[8].data_ptr(), ws_floats=floats, out=st["out"].data_ptr())
        block = fit if cols == 3 else _abi.BCFitLog(fit=fit, logging_iter=1, iter0=0, eps=b["noise"].t.data_ptr())
        with pytest.raises(OlyError, match=rf"{entry}: ws \({n_fit if cols == 3 else n_log} floats\)"):
            eng.ctx.call(entry, C.byref(block), c.steps, eng._s())
        torch.cuda.synchronize()
        fn.assert_untouched(dict(out=b["out"], ws=b["ws"]), entry)
        fn.assert_intact(b, entry)
        assert all(b[name].same_as(snap[name]) for name in BC_STATE), entry
    # the typed front end refuses the same two before the library is reached
    b, st, args = _bc_buffers(eng, c, k, n_fit - 1, 3)
    with pytest.raises(OlyError, match="ws"):
        eng.bc_fit_steps(*args, 0, c.lr, out=st["out"])
    fn.assert_untouched(dict(out=b["out"], ws=b["ws"]), "bc_fit_steps")
    b, st, args = _bc_buffers(eng, c, k, n_fit, 4, eps=blr.noise(c, 1))
    with pytest.raises(OlyError, match="ws"):
        eng.bc_fit_steps_log(*args, 0, c.lr, 1, 0, b["noise"].t, out=st["out"])
    fn.assert_untouched(dict(out=b["out"], ws=b["ws"]), "bc_fit_steps_log")


# ------------------------------------------------------------------------------ what the engine allocates itself
def test_engine_allocated_outputs_of_k11_k12_k14_k24(eng, oracle):
    """One small case each through the Engine methods that allocate their own outputs, every allocation fenced and
    poisoned: what _Guard (tests/test_gpu_parity.py) does for K1-K9, and the poison."""
    d = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a)).cuda()
    rng = np.random.default_rng(77)
    with fn.fence_engine(eng) as ef:
        def returned(what, *tensors):
            torch.cuda.synchronize()
            ef.check(what)
            for t in tensors:
                f = ef.of(t)
                assert f.unwritten() == 0, (what, f.shape, f.unwritten())
                assert not t.dtype.is_floating_point or not bool(torch.isnan(t).any()), (what, f.shape)
        # K11: the packed stream is the engine's
        net = _mlp_net(rng, 41, 12)
        x = rng.normal(0, 1, (17, 41)).astype(np.float32)
        pk = eng.mlp_pack(*[d(a) for a in net])
        returned("mlp_pack", pk)
        y = torch.empty((17, 12), device="cuda")
        eng.mlp_forward2(d(x), pk, 12, y)
        returned("mlp_forward2")
        assert np.array_equal(y.cpu().numpy(), oracle.mlp_forward(x, *net))
        # K12: the stream and every output
        w = _disc_weights(rng, 32)
        x12, eps = rng.normal(0.3, 2.0, (33, 32)).astype(np.float32), rng.normal(0, 1, (33, 128)).astype(np.float32)
        dpk = eng.disc_pack(*[d(w[k]) for k in _DISC_KEYS])
        returned("disc_pack", dpk)
        o = eng.disc_forward(d(x12), dpk, eps=d(eps), want=WANT)
        returned("disc_forward", *o.values())
        ref = oracle.disc_forward(x12, w, eps=eps)
        assert all(np.array_equal(o[k].cpu().numpy(), ref[k]) for k in WANT)
        cs = torch.zeros((3, 32), dtype=F64, device="cuda")
        o = eng.disc_reward_step(d(x12), dpk, cs, False, eps=d(eps), want=WANT)
        returned("disc_reward_step", *o.values())
        ref = oracle.disc_forward(x12, w, colstats=cs.cpu().numpy(), eps=eps)
        assert all(np.array_equal(o[k].cpu().numpy(), ref[k]) for k in WANT)
        # K14: both streams are the engine's, the update runs on them
        c = ppo_update_case(105, n=5, mirror=False, normalize=True)
        pa = eng.mlp_pack(*[d(a) for a in c["actor"]], d(c["a_mean"]), d(c["a_std"]))
        pc = eng.mlp_pack(*[d(a) for a in c["critic"]])
        returned("mlp_pack for the update", pa, pc)
        ws_n, p_a, p_c = eng.ppo_update_plan(5, 41, 12, False)
        ga = fn.Fenced(int(lib().oly_ppo_update_grad_floats(41, 256, 12)), F32)
        gc = fn.Fenced(int(lib().oly_ppo_update_grad_floats(41, 256, 1)), F32)
        scal, ws = fn.Fenced(6, F64), fn.Fenced(ws_n, F32)
        sd, lsd = d(c["sd"]), d(c["log_sd"])
        eng.ppo_update_grads(d(c["obs"]), d(c["action"]), d(c["adv"]), d(c["ret"]), d(c["old_mu"]), pa, pc, sd, lsd, sd, lsd,
                             ga.t, gc.t, scal.t, ws.t, normalize_actor=True, clip=0.2, vf_coeff=0.5)
        returned("ppo_update_grads")
        fn.assert_intact(dict(ga=ga, gc=gc, scal=scal, ws=ws), "ppo_update_grads")
        fn.assert_written(dict(ga=ga, gc=gc, scal=scal), "ppo_update_grads")
        oa, oc, os_ = oracle_update(oracle, c, None, False, (p_a, p_c))
        assert np.array_equal(ga.t.cpu().numpy(), oa) and np.array_equal(gc.t.cpu().numpy(), oc)
        np.testing.assert_allclose(scal.t.cpu().numpy(), os_, rtol=1e-12, atol=1e-15)
        # K24: the targets, the stream, the workspace (exactly the reported floats: the fence makes no allowance) and out
        case = br.CASES[2]
        k, ref = br.yardstick(case)
        targets = eng.bc_targets(d(k["actions"]), d(k["central"]), d(k["delta"]))
        returned("bc_targets", targets)
        _assert_targets(targets.cpu().numpy(), k["actions"], k["central"], k["delta"])
        param = d(br.flat(k["params"]).astype(np.float32))
        st = dict(param=param, m=torch.zeros_like(param), v=torch.zeros_like(param),
                  colstats=torch.zeros((3, case.in_dim), dtype=F64, device="cuda"))
        st["packed"] = eng.ilmlp_pack(*bc_split(param, case.in_dim, case.A))
        returned("ilmlp_pack", st["packed"])
        ws24 = eng.bc_fit_ws(k["batch"], case.in_dim, case.A)
        assert ef.of(ws24).n == int(lib().oly_bc_fit_ws(k["batch"], case.in_dim, case.A))
        st["out"] = eng.bc_fit_steps(d(k["states"]), d(k["targets"]), d(k["idx"]), st["colstats"], param, st["m"], st["v"],
                                     st["packed"], ws24, 0, case.lr, log_std_min=br.LOG_STD_MIN, log_std_max=br.LOG_STD_MAX,
                                     nll_eps=br.NLL_EPS)
        returned("bc_fit_steps", st["out"], st["packed"])
        assert_fit_matches_float64(eng, case, st, ref)
        ef.check("the end")
    assert "_new" not in eng.__dict__
