"""K26's fourth algorithm on the MI355X: oly_iq_q_update with OLY_IQ_ALGO_LSIQ_H, the H update of LSIQ_H / LSIQ_HC, against
the float64 restatement of tests/lsiq_h_restate.py (which keeps the reference's [B, B] broadcast) over iq_restate's shapes
and both classes x MSE / Huber x expert clip on / off x Standardizers on / off; the running maximum's exact float32
expression; its bits (the forward kernel's, across runs, LSIQ's with a tail it does not read); fenced and poisoned
operands; the refusals at the C ABI and the engine; and the agents' critic sides DeviceLSIQH / DeviceLSIQHC: three
update_Q_function calls against lsiq_h_restate's CriticTwin, the deferred target update's bits, the constructors'
refusals, checkpoint and resume.

Tolerances are test_gpu_iq_q.py's: 4 x the float32-against-float64 spread of the same update, never below TOL = 2e-5 (for
the scalars and the running maximum relative to their size from 1 upwards).  lsiq_h_restate.yardstick asserts the margins
of every case's float64 run."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import lsiq_h_restate as H
import lsiq_restate as L
from fences import Fenced, assert_untouched, assert_written, fenced
from test_gpu_iq_q import Dev, split
from test_gpu_lsiq_q import LDev, block_of, same_bits

pytestmark = pytest.mark.gpu
TOL, SHAPES, cat = H.TOL, H.SHAPES, H.cat


@pytest.fixture(scope="module")
def eng():
    from olympic_hip.engine import Engine
    e = Engine(0)
    yield e
    torch.cuda.synchronize()
    e.ctx.close()
    gc.collect()


class HDev(Dev):
    """test_gpu_iq_q.py's fenced critic state carrying H's network, the [2] block of the running maximum fenced at exactly
    two floats, every input of a step fenced at exactly its rows (q_t / v_t at B), and a_pi / logp_pi handed over
    POISONED (NaN all over): the H update must not read them."""

    def __init__(self, eng, params, cfg, in_dim, A, B, target=None):
        super().__init__(eng, params, cfg, in_dim, A, B, target)
        self.f["h_max"] = fenced(np.zeros(2, np.float32))

    def update(self, s, n_policy, **over):
        c = self.cfg
        self.inputs = {k: fenced(np.asarray(v, np.float32)) for k, v in s.items()}
        self.poisoned = dict(a_pi=Fenced((self.B, self.A), torch.float32), logp_pi=Fenced(self.B, torch.float32))
        i = {k: v.t for k, v in self.inputs.items()}
        h = dict(loss=c.loss, cost=c.cost, clip_expert=c.clip_expert, tau_up=c.tau_up, tau_down=c.tau_down,
                 max_state=self.t("h_max") if c.clip_expert else None, q_t=i.get("q_t"), v_t=i.get("v_t"))
        kw = dict(algo="lsiq_h", use_target=True, update_target=c.update_target, gamma=c.gamma, alpha=c.alpha,
                  reg_mult=c.reg_mult, tau=c.tau, weight_decay=c.wd, eps=c.adam_eps,
                  lsiq=dict(Q_min=c.q_min, Q_max=c.q_max, h=h))
        kw.update(over)
        self.eng.iq_q_update(i["obs"], i["act"], i["next_obs"], i["absorbing"], i["a_next"], i["logp_next"],
                             self.poisoned["a_pi"].t, self.poisoned["logp_pi"].t, n_policy, self.t("colstats"),
                             self.t("target_colstats"), self.t("param"), self.t("m"), self.t("v"), self.t("packed"),
                             self.t("target_param"), self.t("target_packed"), self.t("ws"), self.step, c.lr,
                             out=self.t("out"), **kw)
        self.step += 1
        return self.t("out").clone()

    def check_fences(self, what):
        super().check_fences(what)
        assert_untouched(self.poisoned, what)


def compare(eng, who, cfg, dev, out, yard, in_dim, A):
    """The device state and scalars after a case's updates against the float64 run, by the module's rule; prints each
    figure before it asserts."""
    ref, ref_out, f32, f32_out = yard
    got = dev.snapshot()
    dev.check_fences(who)
    for key, rk in (("param", "params"), ("target_param", "target")):
        spread = float(np.abs(cat(f32[rk]) - cat(ref[rk])).max())
        err = float(np.abs(got[key].double().cpu().numpy() - cat(ref[rk])).max())
        print(f"{who} {key}: |kernel - f64| max {err:.3e} (float32 spread {spread:.3e})")
        assert err <= max(TOL, 4 * spread), (who, key, err, spread)
    for key, rk in (("m", "exp_avg"), ("v", "exp_avg_sq")):
        r = cat(ref[rk])
        scale = max(float(np.abs(r).max()), 1e-300)
        spread = float(np.abs(cat(f32[rk]) - r).max()) / scale
        err = float(np.abs(got[key].double().cpu().numpy() - r).max()) / scale
        print(f"{who} {key}: relative to the largest entry {err:.3e} (spread {spread:.3e})")
        assert err <= max(TOL, 4 * spread), (who, key, err, spread)
    if cfg.standardizer:
        for key, rk in (("colstats", "colstats"), ("target_colstats", "tcolstats")):
            a, r = got[key].cpu().numpy(), ref[rk]
            assert np.array_equal(a[0], r[0]), (who, key, "counts", a[0, 0], r[0, 0])
            assert np.all(np.abs(a - r) <= 1e-12 * np.maximum(1.0, np.abs(r))), (who, key)
    tol = np.maximum(TOL * np.maximum(1.0, np.abs(ref_out)), 4 * np.abs(f32_out - ref_out))
    print(f"{who} scalars: worst |kernel - f64| / tolerance {np.max(np.abs(out - ref_out) / tol):.3f}")
    assert np.all(np.abs(out - ref_out) <= tol), (who, np.argwhere(np.abs(out - ref_out) > tol), out, ref_out)
    assert np.all(out[:, 9:] == 0.0)
    h_max = got["h_max"].cpu().numpy()
    if cfg.clip_expert:
        rel = abs(float(h_max[0]) - ref["max"]) / abs(ref["max"])
        spread = abs(f32["max"] - ref["max"]) / abs(ref["max"])
        print(f"{who} running maximum: relative {rel:.3e} (float32 spread {spread:.3e})")
        assert rel <= max(TOL, 4 * spread) and h_max[1] == 1.0, (who, h_max, ref["max"])
        assert out[-1, 8] == float(h_max[0])
    else:
        assert np.array_equal(h_max, np.zeros(2, np.float32)), (who, h_max)
    assert torch.equal(got["packed"], eng.ilmlp_pack(*split(got["param"], in_dim + A)))
    assert torch.equal(got["target_packed"], eng.ilmlp_pack(*split(got["target_param"], in_dim + A)))


# ------------------------------------------------------------------------------ against the float64 yardstick
@pytest.mark.parametrize("cost", (False, True), ids=("lsiq_h", "lsiq_hc"))
@pytest.mark.parametrize("k", range(len(SHAPES)), ids=["-".join(map(str, s)) for s in SHAPES])
def test_update_against_float64(eng, k, cost):
    """Three updates at shape k of one class's eight configs: MSE / Huber x expert clip on / off x Standardizers on / off."""
    in_dim, A, B, n_policy = SHAPES[k]
    steps, params = H.sweep_inputs(k)
    cases = [(j, c) for j, c in enumerate(H.CONFIGS) if c.cost == cost]
    assert len(cases) == 8
    for j, cfg in cases:
        dev = HDev(eng, params, cfg, in_dim, A, B)
        out = np.stack([dev.update(s, n_policy).cpu().numpy() for s in H.case_steps(cfg, steps)])
        compare(eng, f"{SHAPES[k]} {H.cfg_id(cfg)}", cfg, dev, out, H.yardstick(k, j), in_dim, A)


@pytest.mark.parametrize("j", range(len(H.CLIPPED)), ids=[H.cfg_id(c) for c in H.CLIPPED])
def test_targets_beyond_the_upper_clip_bound(eng, j):
    """alpha large enough that at least two rows' targets lie above the target's upper clip bound and two inside, at every
    update (lsiq_h_restate asserts it of the float64 run)."""
    in_dim, A, B, n_policy = SHAPES[1]
    steps, params = H.clipped_inputs()
    cfg = H.CLIPPED[j]
    dev = HDev(eng, params, cfg, in_dim, A, B)
    out = np.stack([dev.update(s, n_policy).cpu().numpy() for s in H.case_steps(cfg, steps)])
    compare(eng, f"clipped {H.cfg_id(cfg)}", cfg, dev, out, H.yardstick("clipped", j), in_dim, A)


def test_the_running_maximum_is_torchs_float32_expression(eng):
    """The [2] block after each of three updates against lsiq_h.py:64-74 evaluated by torch in float32 on the same
    log-probabilities, bit for bit: the first call takes the batch's maximum, a later one (1 - tau) * M + tau * cur with
    the rate of its branch; both branches are taken (lsiq_h_restate asserts it of shape 1's cases)."""
    k = 1
    in_dim, A, B, n_policy = SHAPES[k]
    steps, params = H.sweep_inputs(k)
    cfg = H.CONFIGS[0]
    assert cfg.clip_expert and not cfg.cost
    dev = HDev(eng, params, cfg, in_dim, A, B)
    M, taken = None, set()
    for s in H.case_steps(cfg, steps):
        out = dev.update(s, n_policy)
        neg = -torch.as_tensor(s["logp_next"])
        cur = torch.max(neg[:n_policy])
        if M is None:
            M = cur
        elif cur > M:
            taken.add("up")
            M = (1 - cfg.tau_up) * M + cfg.tau_up * cur
        else:
            taken.add("down")
            M = (1 - cfg.tau_down) * M + cfg.tau_down * cur
        assert M.dtype == torch.float32
        got = dev.t("h_max").cpu()
        assert got[0].item() == M.item() and got[1].item() == 1.0, (got, M)
        assert out[8].item() == M.item()
    assert taken == {"up", "down"}


# ------------------------------------------------------------------------------ bits
@pytest.mark.parametrize("standardizer", (False, True), ids=("nostd", "std"))
def test_h_values_have_the_forward_kernels_bits(eng, standardizer):
    """The raw outputs of both passes, H(obs | act) with the live stream and H'(next_obs | a_next) with the target's, equal
    oly_ilmlp_forward's on the same rows with the statistics each network's Standardizer holds at its pass."""
    from olympic_hip._ffi import lib
    in_dim, A, B, n_policy = SHAPES[1]
    steps, params = H.sweep_inputs(1)
    s = dict(steps[0])
    for key in ("obs", "act", "next_obs", "a_next"):      # a grid of 1/8: the float64 column sums are exact in any order
        s[key] = (np.round(s[key] * 8) / 8).astype(np.float32)
    cfg = H.CONFIGS[12]._replace(standardizer=standardizer)
    target = [p + np.float32(0.01) for p in params]
    dev = HDev(eng, params, cfg, in_dim, A, B, target=target)
    packed0, tpacked0 = dev.t("packed").clone(), dev.t("target_packed").clone()
    dev.update(s, n_policy)
    torch.cuda.synchronize()
    off, BP = int(lib().oly_iq_q_ws_values(B, in_dim, A)), (B + 15) // 16 * 16
    qv = dev.t("ws")[off:off + 3 * BP].view(3, BP)[:, :B]
    x0, x1 = np.concatenate([s["obs"], s["act"]], 1), np.concatenate([s["next_obs"], s["a_next"]], 1)
    st = lambda x: torch.as_tensor(np.stack([np.full(x.shape[1], float(len(x))), x.astype(np.float64).sum(0),
                                             np.square(x.astype(np.float64)).sum(0)])).cuda() if standardizer else None
    assert torch.equal(qv[0], eng.ilmlp_forward(torch.as_tensor(x0).cuda(), packed0, 1, colstats=st(x0)).reshape(-1))
    assert torch.equal(qv[1], eng.ilmlp_forward(torch.as_tensor(x1).cuda(), tpacked0, 1, colstats=st(x1)).reshape(-1))


def test_two_runs_give_the_same_bits(eng):
    k = 3
    in_dim, A, B, n_policy = SHAPES[k]
    steps, params = H.sweep_inputs(k)
    for cfg in (H.CONFIGS[0], H.CONFIGS[12]):
        snaps = []
        for _ in range(2):
            dev = HDev(eng, params, cfg, in_dim, A, B)
            outs = [dev.update(s, n_policy) for s in H.case_steps(cfg, steps)]
            snaps.append((dev.snapshot(), torch.stack(outs)))
        for key, a in snaps[0][0].items():
            assert a is None or torch.equal(a, snaps[1][0][key]), key
        assert torch.equal(snaps[0][1].view(torch.int64), snaps[1][1].view(torch.int64))


def test_the_target_moves_by_the_given_rate_or_not_at_all(eng):
    """update_target = False leaves H's target (the caller of LSIQ_HC updates it with H_tau); with it the target is
    f32(tau) w + f32(1 - tau) t, the other algorithms' expression."""
    in_dim, A, B, n_policy = SHAPES[1]
    steps, params = H.sweep_inputs(1)
    target = [p + np.float32(0.01) for p in params]
    dev = HDev(eng, params, H.CONFIGS[12]._replace(update_target=False), in_dim, A, B, target=target)
    before = dev.snapshot()
    dev.update(steps[0], n_policy)
    after = dev.snapshot()
    assert torch.equal(before["target_param"], after["target_param"])
    assert torch.equal(before["target_packed"], after["target_packed"])
    assert not torch.equal(before["param"], after["param"])
    dev = HDev(eng, params, H.CONFIGS[12]._replace(tau=0.3), in_dim, A, B, target=target)
    t0 = dev.t("target_param").clone()
    dev.update(steps[0], n_policy)
    got = dev.snapshot()
    want = torch.tensor(np.float32(0.3)).cuda() * got["param"] + torch.tensor(np.float32(1 - 0.3)).cuda() * t0
    assert torch.equal(got["target_param"], want)


class LTailDev(LDev):
    """LSIQ's call with the block's h_* tail filled with values the H update refuses and with pointers to poisoned
    buffers (the engine leaves the tail zero, so the block is spoiled as the engine builds it)."""

    def update(self, s, n_policy, tail=False):
        if not tail:
            return super().update(s, n_policy)
        from olympic_hip import _abi
        made = []
        make = _abi.LSIQ
        self.tail = dict(h_max_state=Fenced(2, torch.float32), h_q_t=Fenced(self.B, torch.float32),
                         h_v_t=Fenced(self.B, torch.float32))

        def spoiled(**kw):
            blk = make(**kw)
            blk.h_loss, blk.h_cost, blk.h_clip_expert, blk.h_pad = 7, 5, 1, -1
            blk.h_tau_up, blk.h_tau_down = float("nan"), 3.0
            for k, f in self.tail.items():
                setattr(blk, k, f.t.data_ptr())
            made.append(blk)
            return blk
        _abi.LSIQ = spoiled
        try:
            out = super().update(s, n_policy)
        finally:
            _abi.LSIQ = make
        assert len(made) == 1
        torch.cuda.synchronize()
        assert_untouched(self.tail, "the block's tail")
        return out


def test_lsiq_does_not_read_the_blocks_tail(eng):
    """OLY_IQ_ALGO_LSIQ with the new members zero and with the new members spoiled leaves the same bits: the tail is read
    for the H update alone, so a caller's zero-filled tail is the call as it was."""
    k = 1
    in_dim, A, B, n_policy = SHAPES[k]
    steps, params = L.sweep_inputs(k)
    for cfg in (L.CONFIGS[1], L.CONFIGS[4]):
        snaps = []
        for tail in (False, True):
            dev = LTailDev(eng, params, cfg, in_dim, A, B)
            outs = torch.stack([dev.update(s, n_policy, tail=tail) for s in L.case_steps(cfg, steps, n_policy)])
            snaps.append((dev.snapshot(), outs))
        for key, a in snaps[0][0].items():
            assert same_bits(a, snaps[1][0][key]), (L.cfg_id(cfg), key)
        assert torch.equal(snaps[0][1].view(torch.int64), snaps[1][1].view(torch.int64))


# ------------------------------------------------------------------------------ fenced and poisoned operands
@pytest.mark.parametrize("B,n_policy", ((18, 9), (2, 1)))
def test_fenced_operands_are_written_whole_and_nothing_else(eng, B, n_policy):
    """Every operand in a buffer of exactly its size between poisoned margins: q_t / v_t at exactly B, the [2] block at
    exactly two floats, the workspace at exactly the reported size, a_pi / logp_pi poisoned and left so; out and the [2]
    block are written whole, every parameter moves (weight decay) and stays finite."""
    in_dim, A = 12, 5
    steps, params = H.h_inputs(in_dim, A, B, n_policy, seed=7, updates=1)
    base = H.CONFIGS[12]._replace(wd=1e-3, tau=0.5)
    for cfg in (base, base._replace(cost=False, loss="MSE", reg_mult=0.5)):
        dev = HDev(eng, params, cfg, in_dim, A, B, target=[p + np.float32(0.01) for p in params])
        dev.f["out"] = Fenced(16, torch.float64)              # poisoned again
        before = dev.snapshot()
        s = H.case_steps(cfg, steps)[0]
        assert ("q_t" in s) == cfg.cost and (not cfg.cost or s["q_t"].shape == s["v_t"].shape == (B,))
        dev.update(s, n_policy)
        after = dev.snapshot()
        dev.check_fences(H.cfg_id(cfg))
        assert_written(dict(out=dev.f["out"]), H.cfg_id(cfg))
        for key in ("param", "m", "v", "target_param"):
            assert bool((after[key] != before[key]).all()), key
            assert bool(torch.isfinite(after[key]).all()), key
        assert bool(torch.isfinite(after["out"]).all())
        assert after["h_max"][1].item() == 1.0 and after["h_max"][0].item() == float(np.max(-s["logp_next"][:n_policy]))
        assert float(after["colstats"][0, 0]) == B and float(after["target_colstats"][0, 0]) == B


# ------------------------------------------------------------------------------ refusals
def test_refusals_come_before_any_launch(eng):
    from olympic_hip import _abi
    from olympic_hip._ffi import lib
    in_dim, A, B = 12, 5, 18
    D = in_dim + A
    n_par = 512 * D + 512 + 256 * 512 + 256 + 256 + 1
    npk = int(lib().oly_ilmlp_packed_floats(D, 512, 256, 1))
    nws = int(lib().oly_iq_q_ws(B, in_dim, A))
    f32, f64 = torch.float32, torch.float64
    bufs = dict(obs=Fenced((B, in_dim), f32), act=Fenced((B, A), f32), next_obs=Fenced((B, in_dim), f32),
                absorbing=Fenced(B, f32), a_next=Fenced((B, A), f32), logp_next=Fenced(B, f32), colstats=Fenced((3, D), f64),
                target_colstats=Fenced((3, D), f64), param=Fenced(n_par, f32), m=Fenced(n_par, f32), v=Fenced(n_par, f32),
                packed=Fenced(npk, f32), target_param=Fenced(n_par, f32), target_packed=Fenced(npk, f32),
                ws=Fenced(nws, f32), out=Fenced(16, f64))
    tail = dict(h_max_state=Fenced(2, f32), h_q_t=Fenced(B, f32), h_v_t=Fenced(B, f32))
    keep = []

    def block(ls=None, null_lsiq=False, **over):
        lk = dict(lossQ_type=0, loss_mode_exp=0, Q_exp_loss=1, target_clipping=1, Q_min=-1.0, Q_max=1.0, h_loss=2, h_cost=1,
                  h_clip_expert=1, h_tau_up=1e-2, h_tau_down=1e-4)
        lk.update({k: b.t.data_ptr() for k, b in tail.items()})
        lk.update(ls or {})
        blk = _abi.LSIQ(**lk)
        keep.append(blk)
        kw = dict(in_dim=in_dim, act_dim=A, batch=B, n_policy=9, algo=_abi.IQ_ALGO["lsiq_h"], plcy_loss_mode=0,
                  regularizer_mode=0, treat_absorbing=0, use_target=1, update_target=1, step=0, pad=0, gamma=0.99, alpha=1e-3,
                  reg_mult=0.5, R_min=0.0, R_max=1.0, gradient_penalty_lambda=0.0, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8,
                  weight_decay=0.0, pad2=0.0, tau=0.005, packed_floats=npk, target_packed_floats=npk, ws_floats=nws,
                  a_pi=None, logp_pi=None, lsiq=None if null_lsiq else C.pointer(blk))
        kw.update({k: b.t.data_ptr() for k, b in bufs.items()})
        kw.update(over)
        return _abi.IQQ(**kw)
    nan = float("nan")
    bad = dict(no_block=dict(null_lsiq=True), no_target=dict(use_target=0), mode=dict(plcy_loss_mode=1),
               reg=dict(regularizer_mode=1), loss_none=dict(ls=dict(h_loss=0)), loss_unknown=dict(ls=dict(h_loss=3)),
               cost_unknown=dict(ls=dict(h_cost=2)), tau_up_big=dict(ls=dict(h_tau_up=1.5)), tau_up_neg=dict(ls=dict(h_tau_up=-0.1)),
               tau_up_nan=dict(ls=dict(h_tau_up=nan)), tau_down_big=dict(ls=dict(h_tau_down=2.0)),
               tau_down_nan=dict(ls=dict(h_tau_down=nan)), null_max=dict(ls=dict(h_max_state=None)),
               null_q_t=dict(ls=dict(h_q_t=None)), null_v_t=dict(ls=dict(h_v_t=None)), bounds_equal=dict(ls=dict(Q_min=0.5, Q_max=0.5)),
               q_min_nan=dict(ls=dict(Q_min=nan)),
               null_target=dict(target_param=None), null_target_packed=dict(target_packed=None), null_logp=dict(logp_next=None),
               gp=dict(gradient_penalty_lambda=0.5), tau=dict(tau=1.5), short_ws=dict(ws_floats=nws - 1),
               reg_mult_0=dict(reg_mult=0.0), n_policy_B=dict(n_policy=B))
    Lb = lib()
    for name, over in bad.items():
        rc = Lb.oly_iq_q_update(eng.ctx.handle, C.byref(block(**over)), eng._s())
        assert rc == _abi.OLY_EINVAL, (name, rc)
    torch.cuda.synchronize()
    assert_untouched(bufs, "refused calls")
    assert_untouched(tail, "refused calls")


def test_the_engine_refuses_what_the_library_refuses(eng):
    from olympic_hip._ffi import OlyError
    in_dim, A, B, n_policy = SHAPES[1]
    steps, params = H.sweep_inputs(1)
    cfg = H.CONFIGS[12]
    dev = HDev(eng, params, cfg, in_dim, A, B)
    s = steps[0]
    d = lambda a: torch.as_tensor(a).cuda()
    good = dict(loss="Huber", cost=True, clip_expert=True, tau_up=0.3, tau_down=0.1, max_state=dev.t("h_max"), q_t=d(s["q_t"]),
                v_t=d(s["v_t"]))
    blk = lambda **h: dict(lsiq=dict(Q_min=cfg.q_min, Q_max=cfg.q_max, h=dict(good, **h)))
    before = dev.snapshot()
    for over in (dict(lsiq=None), dict(lsiq=dict(Q_min=cfg.q_min, Q_max=cfg.q_max)), blk(loss=None), blk(loss="L1"),
                 blk(tau_up=1.5), blk(tau_down=-1.0), blk(max_state=None), blk(q_t=None), blk(v_t=d(s["v_t"][:-1])),
                 blk(max_state=torch.zeros(3, device="cuda")), blk(extra=1), dict(use_target=False),
                 dict(plcy_loss_mode="value_expert"), dict(regularizer_mode="off"), dict(reg_mult=0.0),
                 dict(lsiq=dict(Q_min=1.0, Q_max=-1.0, h=good))):
        with pytest.raises(OlyError):
            dev.update(s, n_policy, **over)
    dev.step = 0
    after = dev.snapshot()
    for key, a in before.items():
        assert same_bits(a, after[key]), key
    # and the other algorithms take no h entry
    ldev = LDev(eng, params, L.LCfg(q_min=L.Q_MIN, q_max=L.Q_MAX), in_dim, A, B)
    with pytest.raises(OlyError):
        ldev.update(L.sweep_inputs(1)[0][0], n_policy, lsiq=dict(block_of(ldev.cfg), h=good))


# ------------------------------------------------------------------------------ the agents' critic side
def build_agent(eng, case, sw=None, **more):
    from olympic_hip.bc import DeviceSquashedGaussianPolicy
    from olympic_hip.gail import DeviceStandardizer
    from olympic_hip.iq import DeviceLSIQH, DeviceLSIQHC, DeviceSoftQCritic
    in_dim, A = case["in_dim"], case["A"]
    D, pcfg, lcfg, hcfg = in_dim + A, case["pcfg"], case["lcfg"], case["hcfg"]

    def lins(params, dims):
        out = [torch.nn.Linear(i, o) for i, o in dims]
        with torch.no_grad():
            for j, lin in enumerate(out):
                lin.weight.copy_(torch.as_tensor(params[2 * j]))
                lin.bias.copy_(torch.as_tensor(params[2 * j + 1]))
        return out
    if "min_a" in case:
        min_a, max_a = case["min_a"], case["max_a"]
    else:
        central, delta = case["central"].astype(np.float64), case["delta"].astype(np.float64)
        min_a, max_a = central - delta, central + delta
    policy = DeviceSquashedGaussianPolicy(eng, lins(case["pparams"], [(in_dim, 512), (512, 256), (256, 2 * A)]),
                                          min_a, max_a, standardizer=DeviceStandardizer(eng, in_dim),
                                          log_std_min=pcfg.ls_min, log_std_max=pcfg.ls_max)
    dims = [(D, 512), (512, 256), (256, 1)]
    critic = DeviceSoftQCritic(eng, lins(case["qparams"], dims), standardizer=DeviceStandardizer(eng, D), lr=lcfg.lr,
                               eps=lcfg.adam_eps, tau=lcfg.tau)
    h_critic = DeviceSoftQCritic(eng, lins(case["hparams"], dims), standardizer=DeviceStandardizer(eng, D), lr=hcfg.lr,
                                 eps=hcfg.adam_eps, tau=lcfg.tau)
    demo = dict(states=np.zeros((4, in_dim), np.float32), actions=np.zeros((4, A), np.float32),
                next_states=np.zeros((4, in_dim), np.float32), absorbing=np.zeros(4, np.float32))
    kw = dict(gamma=lcfg.gamma, batch_size=case["n_policy"], use_target=lcfg.use_target,
              init_alpha=case.get("init_alpha", hcfg.alpha), reg_mult=lcfg.reg_mult,
              plcy_loss_mode=lcfg.mode, regularizer_mode=lcfg.reg, Q_max=lcfg.q_max, Q_min=lcfg.q_min,
              loss_mode_exp=lcfg.exp_mode, Q_exp_loss=lcfg.exp_loss, target_clipping=True, lossQ_type=lcfg.type,
              max_replay_size=64, sw=sw, h_critic=h_critic, max_H_policy_tau_up=hcfg.tau_up,
              max_H_policy_tau_down=hcfg.tau_down)
    if hcfg.cost:
        kw.update(H_tau=hcfg.tau, H_loss_mode=hcfg.loss)
    kw.update(more)
    if kw["h_critic"] == "the Q critic":
        kw["h_critic"] = critic
    return (DeviceLSIQHC if hcfg.cost else DeviceLSIQH)(eng, policy, critic, demo, **kw)


def run_agent(agent, case, first, last):
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    outs = []
    for s, e in list(zip(case["steps"], case["noise"]))[first:last]:
        eps = {k: d(v) for k, v in e.items()}
        q = agent.update_Q_function(d(s["obs"]), d(s["act"]), d(s["next_obs"]), d(s["absorbing"]), case["n_policy"], eps=eps)
        outs.append((q.cpu().numpy(), agent.h_out.cpu().numpy()))
        agent._iter += 1
    return outs


@pytest.mark.parametrize("cost", (False, True), ids=("lsiq_h", "lsiq_hc"))
def test_update_Q_function_against_the_twin(eng, cost):
    """Three update_Q_function calls of DeviceLSIQH / DeviceLSIQHC, every iteration logging, against the float64
    CriticTwin on the same batches and noise: both critics' parameters and targets, the running maximum, both blocks
    of scalars, and how many rows each Standardizer has taken."""
    from olympic_hip import _abi
    from test_gpu_iq_q import Recorder
    case = H.agent_case(cost)
    ref, ref_q, ref_h, margins = H.run_agent(case, check=True)
    H.assert_margins(margins, ("agent", cost), counts=False)
    f32, f32_q, f32_h = H.run_agent(case, torch.float32)
    sw = Recorder()
    agent = build_agent(eng, case, sw=sw)
    outs = run_agent(agent, case, 0, len(case["steps"]))
    torch.cuda.synchronize()
    for net, c in (("q", agent.critic), ("h", agent.h_critic)):
        for flat, rk in ((c.param, "params"), (c.target_param, "target")):
            r = cat(ref[net][rk])
            spread = float(np.abs(cat(f32[net][rk]) - r).max())
            err = float(np.abs(flat.double().cpu().numpy() - r).max())
            print(f"{'hc' if cost else 'h'} {net} {rk}: |device - f64| max {err:.3e} (float32 spread {spread:.3e})")
            assert err <= max(TOL, 4 * spread), (net, rk, err, spread)
        for st, rk in ((c.stand, "colstats"), (c.target_stand, "tcolstats")):
            a, r = st.colstats.cpu().numpy(), ref[net][rk]
            assert np.array_equal(a[0], r[0]), (net, rk, a[0, 0], r[0, 0])
            assert np.all(np.abs(a - r) <= np.maximum(TOL * np.maximum(1.0, np.abs(r)), 1e-9)), (net, rk)
    a, r = agent.policy.stand.colstats.cpu().numpy(), ref["policy_colstats"]
    B, n_p = case["B"], case["n_policy"]
    assert np.array_equal(a[0], r[0]) and a[0, 0] == 3 * ((4 if cost else 3) * B + (B - n_p))
    h_max = agent.h_max_state.cpu().numpy()
    rel = abs(float(h_max[0]) - ref["h"]["max"]) / abs(ref["h"]["max"])
    spread = abs(f32["h"]["max"] - ref["h"]["max"]) / abs(ref["h"]["max"])
    print(f"running maximum: relative {rel:.3e} (float32 spread {spread:.3e})")
    assert rel <= max(TOL, 4 * spread) and h_max[1] == 1.0
    for k, (want, want32, name) in enumerate(((ref_q, f32_q, "Q"), (ref_h, f32_h, "H"))):
        got = np.stack([o[k] for o in outs])
        tol = np.maximum(TOL * np.maximum(1.0, np.abs(want)), 4 * np.nan_to_num(np.abs(want32 - want)))
        ok = (np.abs(got - want) <= tol) | (np.isnan(got) & np.isnan(want))
        print(f"{name} scalars: worst |device - f64| / tolerance {np.nanmax(np.abs(got - want) / tol):.3f}")
        assert ok.all(), (name, np.argwhere(~ok), got[~ok], want[~ok])
    for i in range(len(outs)):                     # the writer got the reference's seven H scalars of every iteration
        for k in range(7):
            assert sw.rows[i + 1][_abi.LSIQ_H_TAGS[k]] == outs[i][1][k]
        assert _abi.LSIQ_H_TAGS[7] not in sw.rows[i + 1] and "IQ-Loss/Loss1" in sw.rows[i + 1]
    assert agent.critic.step == agent.h_critic.step == len(outs)


def test_the_deferred_target_update_has_the_in_call_updates_bits(eng):
    """DeviceLSIQHC passes update_target=False to the Q critic's call and updates its target after the H update; the H
    update does not write the Q critic, so after one update_Q_function the Q critic's target and its stream equal,
    bit for bit, what DeviceLSIQH's in-call update leaves from the same start (the Q step itself is the same call)."""
    case = H.agent_case(True)
    a = build_agent(eng, case)
    case_h = dict(case, hcfg=case["hcfg"]._replace(cost=False, loss="MSE"))
    b = build_agent(eng, case_h)
    run_agent(a, case, 0, 1)
    run_agent(b, case_h, 0, 1)
    torch.cuda.synchronize()
    assert torch.equal(a.critic.param, b.critic.param)
    assert not torch.equal(a.critic.target_param, a.critic.param)
    assert torch.equal(a.critic.target_param, b.critic.target_param)
    assert torch.equal(a.critic.target_packed, b.critic.target_packed)


def test_the_constructors_refuse(eng):
    from olympic_hip._ffi import OlyError
    case = H.agent_case(True)
    build_agent(eng, case)
    for more in (dict(h_critic=None), dict(h_critic="the Q critic"), dict(max_H_policy_tau_up=1.5),
                 dict(max_H_policy_tau_down=-0.1), dict(H_tau=None), dict(H_tau=1.5), dict(H_loss_mode="L1"),
                 dict(reg_mult=0.0), dict(learnable_alpha=True), dict(plcy_loss_mode="v0")):
        with pytest.raises(OlyError):
            build_agent(eng, case, **more)
            print("not refused:", more)


@pytest.mark.parametrize("cost", (False, True), ids=("lsiq_h", "lsiq_hc"))
def test_a_saved_run_resumes_to_the_same_bits(eng, tmp_path, cost):
    from olympic_hip._ffi import OlyError
    case = H.agent_case(cost)
    whole = build_agent(eng, case)
    run_agent(whole, case, 0, 3)
    first = build_agent(eng, case)
    run_agent(first, case, 0, 2)
    path = first.save(str(tmp_path / "lsiq_h.pt"), note="after update 2")
    resumed = build_agent(eng, case)
    ptrs = [t.data_ptr() for t in (resumed.h_critic.param, resumed.h_critic.target_packed, resumed.h_max_state)]
    assert resumed.load(path)["note"] == "after update 2"
    assert resumed._iter == 3 and resumed.h_critic.step == 2
    assert ptrs == [t.data_ptr() for t in (resumed.h_critic.param, resumed.h_critic.target_packed, resumed.h_max_state)]
    run_agent(resumed, case, 2, 3)
    torch.cuda.synchronize()
    for a, b in ((whole.critic, resumed.critic), (whole.h_critic, resumed.h_critic)):
        for key in ("param", "target_param", "exp_avg", "exp_avg_sq", "packed", "target_packed"):
            assert torch.equal(getattr(a, key), getattr(b, key)), key
        assert torch.equal(a.stand.colstats, b.stand.colstats) and torch.equal(a.target_stand.colstats, b.target_stand.colstats)
    assert torch.equal(whole.h_max_state, resumed.h_max_state) and float(whole.h_max_state[1]) == 1.0
    assert torch.equal(whole.policy.stand.colstats, resumed.policy.stand.colstats)
    assert whole.state_dict()["kind"] == ("lsiq_hc_critic" if cost else "lsiq_h_critic")
    other = build_agent(eng, dict(case, hcfg=case["hcfg"]._replace(cost=not cost, loss="Huber")))
    with pytest.raises(OlyError):
        other.load(path)
