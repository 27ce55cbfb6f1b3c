"""The two device discriminator trainers (il_agent.DeviceDiscriminatorTrainer for VAIL, DeviceGAILDiscriminatorTrainer for
GAIL) and the two rewards above the C ABI, without a GPU: an Engine on CPU tensors whose context records every entry
point instead of calling it.  What is pinned is the host layer's contract with the library: which entry points a fit
issues and in what order, the scalars and the non-pointer struct fields it hands them, which pointers are NULL, the
draws it takes from the caller's generator, and the trainer's own state afterwards.  The real library serves the
workspace and packed sizes.

Shapes: 9 policy rows of 6 columns, 7 demonstration rows (m < n), the state mask 1..5, 2 epochs.  16 concatenated rows
in minibatches of 4 are four whole minibatches; minibatches of 5 end on a partial one, so both sizes run."""
import ctypes
import os

import numpy as np
import pytest
import torch

from olympic_hip import _abi, _ffi
from olympic_hip._ffi import OlyError
from olympic_hip.engine import Engine
from olympic_hip.gail import (DiscriminatorReward, GAILDiscriminator, GAILDiscriminatorReward, VariationalDiscriminator,
                              VDBLoss)
from olympic_hip.il_agent import DISC_LOG_NAMES, DeviceDiscriminatorTrainer, DeviceGAILDiscriminatorTrainer

N_PLCY, N_DEMO, OBS, ACT, EPOCHS = 9, 7, 6, 3, 2
ROWS = N_PLCY + N_DEMO
MASK = np.arange(1, 6)
DS = int(MASK.size)
PAIRS = (None, "next_state", "action")
HYPER = dict(lr=3e-4, betas=(0.8, 0.95), eps=1e-6, weight_decay=1e-3)
INFO_CONSTRAINT, LR_BETA, ENTCOEFF = 0.2, 1e-4, 2e-3
_POINTERS = (ctypes.c_void_p, ctypes.c_char_p)


def _lib():
    if not os.path.exists(_ffi.LIB_PATH):
        pytest.fail(f"{_ffi.LIB_PATH} missing: run python __graft_entry__.py build")
    return _ffi.lib()


def _plain(a):
    """One argument of a recorded call as plain data: numbers as they are, a pointer as True / False (NULL), a struct
    passed by reference as a dict of its fields (pointers again True / False)."""
    if a is None:
        return False
    if isinstance(a, ctypes.c_void_p):
        return bool(a.value)
    if isinstance(a, ctypes._SimpleCData):
        return a.value
    obj = getattr(a, "_obj", None)                  # ctypes.byref(struct)
    if isinstance(obj, ctypes.Structure):
        return {name: (bool(getattr(obj, name)) if ctype in _POINTERS else getattr(obj, name))
                for name, ctype in obj._fields_ if name != "pad"}
    if isinstance(a, ctypes.Array):
        return [bool(v) for v in a]
    assert isinstance(a, (int, float)), type(a)
    return a


class RecordingContext:
    """Stands where Engine.ctx stands: call() records (name, arguments as plain data) and launches nothing."""

    def __init__(self):
        self.calls = []

    def stream(self):
        return None

    def call(self, name, *args):
        self.calls.append((name, [_plain(a) for a in args]))

    def names(self):
        return [c[0] for c in self.calls]


def cpu_engine():
    _lib()
    eng = Engine.__new__(Engine)
    eng.device = torch.device("cpu")
    eng.ctx = RecordingContext()
    return eng


def widths(pair):
    """(network input, second part) of a mode."""
    return {None: (DS, 0), "next_state": (2 * DS, DS), "action": (DS + ACT, ACT)}[pair]


def make_reward(algo, eng, pair):
    torch.manual_seed(3)
    in_dim = widths(pair)[0]
    if algo == "vail":
        return DiscriminatorReward(eng, VariationalDiscriminator(in_dim=in_dim), state_mask=MASK, pair=pair)
    return GAILDiscriminatorReward(eng, GAILDiscriminator(in_dim), state_mask=MASK, pair=pair)


def make_inputs(pair):
    rng = np.random.default_rng(11)
    f = lambda *sh: rng.normal(0, 1, sh).astype(np.float32)
    plcy, demo = torch.as_tensor(f(N_PLCY, OBS)), f(N_DEMO, OBS)
    if pair is None:
        return plcy, None, demo                                           # an array of full observations
    w2, key = (OBS, "next_states") if pair == "next_state" else (ACT, "actions")
    return plcy, torch.as_tensor(f(N_PLCY, w2)), {"states": demo, key: f(N_DEMO, w2)}   # the reference's dict


def make_trainer(algo, eng, pair, noisy, batch):
    r = make_reward(algo, eng, pair)
    plcy, x2, demo = make_inputs(pair)
    kw = dict(HYPER, batch_size=batch, n_epochs=EPOCHS, use_noisy_targets=noisy)
    if algo == "vail":
        loss = VDBLoss(INFO_CONSTRAINT, LR_BETA, entcoeff=ENTCOEFF)
        return DeviceDiscriminatorTrainer(r, demo, loss, **kw), plcy, x2
    return DeviceGAILDiscriminatorTrainer(r, demo, entcoeff=ENTCOEFF, **kw), plcy, x2


def run_fit(algo, pair, noisy, log, batch, seed=5):
    eng = cpu_engine()
    tr, plcy, x2 = make_trainer(algo, eng, pair, noisy, batch)
    g = torch.Generator().manual_seed(seed)
    kw = dict(generator=g, log=log)
    if pair is not None:
        kw["x2"] = x2
    return eng, tr, g, tr.fit(plcy, **kw)


def expected_draws(algo, noisy, log, seed=5):
    """The draws of one fit, made here in the documented order per epoch."""
    g = torch.Generator().manual_seed(seed)
    for _ in range(EPOCHS):
        torch.randperm(N_DEMO, generator=g)
        if noisy:
            torch.empty(N_PLCY).uniform_(0.80, 0.99, generator=g)
            torch.empty(N_PLCY).uniform_(0.01, 0.10, generator=g)
        torch.randperm(ROWS, generator=g)
        if algo == "vail":
            torch.randn((ROWS, 128), generator=g)
            if log:
                torch.randn((4 * ROWS, 128), generator=g)
    return g


def f32(v):
    return float(np.float32(v))


CASES = [(a, p, n, l, b) for a in ("vail", "gail") for p in PAIRS for n in (False, True) for l in (False, True)
         for b in (4, 5)]


@pytest.mark.parametrize("algo,pair,noisy,log,batch", CASES)
def test_fit_issues_the_entry_points_of_its_mode_with_the_arguments_of_its_inputs(algo, pair, noisy, log, batch):
    L = _lib()
    eng, tr, g, res = run_fit(algo, pair, noisy, log, batch)
    calls = eng.ctx.calls
    vail = algo == "vail"
    in_dim, d2 = widths(pair)
    std = int(pair == "next_state")
    nb = (ROWS + batch - 1) // batch

    # ---- the sequence, written out
    pack = "oly_disc_pack" if vail else "oly_ilmlp_pack"
    epoch = {("vail", False): "oly_disc_fit_epoch", ("vail", True): "oly_disc_fit_epoch_pair",
             ("gail", False): "oly_gail_disc_fit_epoch", ("gail", True): "oly_gail_disc_fit_epoch_pair"}[algo, pair is not None]
    logname = "oly_disc_log" if vail else "oly_gail_disc_log"
    per_epoch = ["oly_col_stats", epoch] + ([logname] if log else [])
    assert eng.ctx.names() == [pack] + per_epoch * EPOCHS
    assert (tr._log_ws is not None) == log

    # ---- the arguments, from the inputs
    if pair is None:
        ws_floats = int((L.oly_disc_fit_ws_floats if vail else L.oly_gail_disc_fit_ws_floats)(batch, in_dim))
    else:
        ws_floats = int((L.oly_disc_fit_pair_ws_floats if vail else L.oly_gail_disc_fit_pair_ws_floats)(batch, DS, d2, std))
    assert ws_floats > 0 and int(tr._ws.numel()) == ws_floats
    log_floats = int((L.oly_disc_log_ws_floats if vail else L.oly_gail_disc_log_ws_floats)(ROWS))
    body = calls[1:]
    for e in range(EPOCHS):
        stats, fit = body[e * len(per_epoch)], body[e * len(per_epoch) + 1]
        assert stats[1] == [ROWS, DS, True, True, 1, False]           # rows, states' columns, x, colstats, accumulate, stream
        s = fit[1][0]
        want = dict(in_dim=in_dim, n_plcy=N_PLCY, step=e * nb, lr=f32(HYPER["lr"]), beta1=f32(HYPER["betas"][0]),
                    beta2=f32(HYPER["betas"][1]), adam_eps=f32(HYPER["eps"]), weight_decay=f32(HYPER["weight_decay"]),
                    ws_floats=ws_floats, x=True, targets=noisy, colstats=True, param=True, exp_avg=True, exp_avg_sq=True,
                    packed=True, ws=True, loss_out=True, bce_out=False)
        if vail:
            want.update(info_constraint=f32(INFO_CONSTRAINT), lr_beta=f32(LR_BETA), eps=True, beta=True, kl_out=False,
                        beta_out=False)
        else:
            want.update(entcoeff=f32(ENTCOEFF), ent_out=False)
        assert s == want
        rest = fit[1][1:]
        if pair is not None:
            assert rest[0] == dict(x2=True, mask2=False, stride2=d2, d2=d2, standardise=std)
            rest = rest[1:]
        assert rest == [True, ROWS, batch, False]                      # perm, n_rows, batch, stream
        if log:
            name, a = body[e * len(per_epoch) + 2]
            want = dict(in_dim=in_dim, n_rows=ROWS, n_plcy=N_PLCY, entcoeff=f32(ENTCOEFF), x=True, targets=noisy,
                        colstats=True, packed=True, ws=True, ws_floats=log_floats, out=True)
            if vail:
                want.update(info_constraint=f32(INFO_CONSTRAINT), lr_beta=f32(LR_BETA), eps=True, beta=True)
            assert a[0] == want
            assert a[1] == (False if pair is None else dict(x2=True, mask2=False, stride2=d2, d2=d2, standardise=std))
            assert a[2] is False                                       # stream

    # ---- the generator, the trainer, the result
    assert torch.equal(g.get_state(), expected_draws(algo, noisy, log).get_state())
    assert tr.step == EPOCHS * nb
    losses, logs = res if log else (res, None)
    assert tuple(losses.shape) == (EPOCHS, nb) and losses.dtype == torch.float64
    if log:
        assert tuple(logs.shape) == (EPOCHS, 12) and logs.dtype == torch.float64
    assert tr.log_names == DISC_LOG_NAMES[algo] and tr.pair == pair
    assert int(tr.param.numel()) == int(tr.exp_avg.numel()) == int(tr.exp_avg_sq.numel()) == sum(
        int(p.numel()) for p in tr.r._params())
    assert tr.expert is None and tuple(tr.demo.shape) == (N_DEMO, OBS)
    if pair is not None:
        assert tuple(tr.demo2.shape) == (N_DEMO, OBS if pair == "next_state" else ACT)


@pytest.mark.parametrize("pair", PAIRS)
def test_vail_takes_its_noise_from_the_caller_when_given(pair):
    """eps [n_epochs, rows, 128] and log_eps [n_epochs, 4 rows, 128] replace draws 4 and 5; GAIL's fit has neither."""
    eng = cpu_engine()
    tr, plcy, x2 = make_trainer("vail", eng, pair, True, 4)
    g = torch.Generator().manual_seed(5)
    kw = dict(x2=x2) if pair is not None else {}
    tr.fit(plcy, generator=g, eps=torch.zeros((EPOCHS, ROWS, 128)), log=True, log_eps=torch.zeros((EPOCHS, 4 * ROWS, 128)), **kw)
    assert torch.equal(g.get_state(), expected_draws("gail", True, True).get_state())
    geng = cpu_engine()
    gtr, plcy, x2 = make_trainer("gail", geng, pair, True, 4)
    with pytest.raises(TypeError):
        gtr.fit(plcy, eps=None, **kw)
    with pytest.raises(TypeError):
        gtr.fit(plcy, log_eps=None, **kw)


@pytest.mark.parametrize("algo", ["vail", "gail"])
def test_a_second_fit_continues_the_step_count_and_keeps_the_state(algo):
    eng = cpu_engine()
    tr, plcy, _ = make_trainer(algo, eng, None, False, 4)
    ptrs = [t.data_ptr() for t in (tr.param, tr.exp_avg, tr.exp_avg_sq)]
    params = [p.data_ptr() for p in tr.r._params()]
    tr.fit(plcy, generator=torch.Generator().manual_seed(1))
    first = len(eng.ctx.calls)
    tr.fit(plcy, generator=torch.Generator().manual_seed(2))
    steps = [c[1][0]["step"] for c in eng.ctx.calls if "fit_epoch" in c[0]]
    assert steps == [0, 4, 8, 12] and tr.step == 16
    assert "pack" in eng.ctx.names()[0] and not any("pack" in n for n in eng.ctx.names()[first:])
    assert ptrs == [t.data_ptr() for t in (tr.param, tr.exp_avg, tr.exp_avg_sq)]
    assert params == [p.data_ptr() for p in tr.r._params()]            # written back in place
    d = tr.state_dict()
    assert sorted(d) == sorted(["n_par", "exp_avg", "exp_avg_sq", "step"] + (["beta"] if algo == "vail" else []))
    assert d["step"] == 16 and d["n_par"] == int(tr.param.numel())
    other, _, _ = make_trainer(algo, cpu_engine(), None, False, 4)
    other.load_state_dict(d)
    assert other.step == 16
    with pytest.raises(OlyError, match=type(tr).__name__):
        other.load_state_dict(dict(d, n_par=d["n_par"] + 1))


@pytest.mark.parametrize("algo", ["vail", "gail"])
def test_the_trainers_refuse_by_their_own_name(algo):
    name = "DeviceDiscriminatorTrainer" if algo == "vail" else "DeviceGAILDiscriminatorTrainer"
    tr, plcy, _ = make_trainer(algo, cpu_engine(), None, False, 4)
    with pytest.raises(OlyError, match=f"{name}.fit: no policy rows"):
        tr.fit(plcy[:0])
    with pytest.raises(OlyError, match="the state mask reads column 5"):
        tr.fit(plcy[:, :5])
    ptr, plcy, x2 = make_trainer(algo, cpu_engine(), "action", False, 4)
    with pytest.raises(OlyError, match=f"{name}.fit: pair='action' needs the policy's second tensor"):
        ptr.fit(plcy)
    r = make_reward(algo, cpu_engine(), "action")
    args = (VDBLoss(0.1, 1e-5),) if algo == "vail" else ()
    cls = DeviceDiscriminatorTrainer if algo == "vail" else DeviceGAILDiscriminatorTrainer
    with pytest.raises(OlyError, match=f"{name}: the demonstrations lack `actions`"):
        cls(r, {"states": np.zeros((4, OBS), np.float32)}, *args)
    with pytest.raises(OlyError, match=f"{name}: pair='action' takes an ExpertDataset or a dict"):
        cls(r, np.zeros((4, OBS), np.float32), *args)


# ------------------------------------------------------------------------------ the rewards
def _pair_block(pair, full):
    """DiscPair of a reward call: the second tensor at full width, its mask inside the kernel."""
    d2 = widths(pair)[1]
    return dict(x2=True, mask2=pair == "next_state", stride2=full, d2=d2, standardise=int(pair == "next_state"))


@pytest.mark.parametrize("pair", PAIRS)
def test_gail_reward_issues_the_entry_point_of_its_mode(pair):
    eng = cpu_engine()
    r = make_reward("gail", eng, pair)
    plcy, x2, _ = make_inputs(pair)
    kw = {} if pair is None else dict(x2=x2)
    sfx = "" if pair is None else "_pair"
    o = r.forward(plcy, want=("reward", "logits"), **kw)
    assert sorted(o) == ["logits", "reward"] and tuple(o["reward"].shape) == (N_PLCY,)
    r.forward(plcy, **kw)                      # the stream exists: re-packed from the live parameters inside the call
    assert eng.ctx.names() == ["oly_ilmlp_pack", "oly_gail_reward_step" + sfx, "oly_gail_reward_step" + sfx]
    first, second = eng.ctx.calls[1][1], eng.ctx.calls[2][1]
    if pair is None:
        #              B, Dx, D, x, mask, colstats, accumulate, weights, packed, reward, logits, stream
        assert first == [N_PLCY, OBS, DS, True, True, True, 0, False, True, True, True, False]
        assert second == [N_PLCY, OBS, DS, True, True, True, 1, [True] * 6, True, True, False, False]
    else:
        w2 = OBS if pair == "next_state" else ACT
        #              B, Dx, Ds, x, mask, pair, colstats, stats_a, accumulate, weights, packed, reward, logits, stream
        assert first == [N_PLCY, OBS, DS, True, True, _pair_block(pair, w2), True, True, 0, False, True, True, True, False]
        assert second == [N_PLCY, OBS, DS, True, True, _pair_block(pair, w2), True, True, 1, [True] * 6, True, True, False,
                          False]
    eng.ctx.calls.clear()
    o = r.predict(plcy, **kw)
    assert list(o) == ["logits"] and eng.ctx.names() == ["oly_ilmlp_pack", "oly_gail_disc_forward" + sfx]
    a = eng.ctx.calls[1][1]
    if pair is None:
        #            B, Dx, D, x, mask, mean, std, colstats, packed, reward, logits, stream
        assert a == [N_PLCY, OBS, DS, True, True, False, False, True, True, False, True, False]
    else:
        #            B, Dx, Ds, x, mask, pair, stats_a, stats_b, packed, reward, logits, stream
        assert a == [N_PLCY, OBS, DS, True, True, _pair_block(pair, w2), True, True, True, False, True, False]
    with pytest.raises(OlyError, match="unknown output 'mu'"):
        r.forward(plcy, want=("mu",), **kw)
    with pytest.raises(OlyError, match="no output requested"):
        r.predict(plcy, want=(), **kw)


@pytest.mark.parametrize("pair", PAIRS)
def test_vail_reward_issues_the_entry_point_of_its_mode(pair):
    eng = cpu_engine()
    r = make_reward("vail", eng, pair)
    plcy, x2, _ = make_inputs(pair)
    eps = torch.zeros((N_PLCY, 128))
    if pair is None:
        # a masked states-only reward: the statistics, the pack and the forward are three calls
        o = r.forward(plcy, eps, want=("reward", "mu"))
        assert sorted(o) == ["mu", "reward"] and tuple(o["mu"].shape) == (N_PLCY, 128)
        assert eng.ctx.names() == ["oly_col_stats", "oly_disc_pack", "oly_disc_forward"]
        with pytest.raises(OlyError, match="predict serves a paired reward"):
            r.predict(plcy, x2=plcy)
        # whole rows: one call
        whole = DiscriminatorReward(eng, VariationalDiscriminator(in_dim=OBS))
        eng.ctx.calls.clear()
        whole.forward(plcy, eps)
        whole.forward(plcy, eps)
        assert eng.ctx.names() == ["oly_disc_pack", "oly_disc_reward_step", "oly_disc_reward_step"]
        return
    w2 = OBS if pair == "next_state" else ACT
    o = r.forward(plcy, eps, want=("reward", "logits", "mu", "logvar"), x2=x2)
    assert sorted(o) == ["logits", "logvar", "mu", "reward"]
    r.forward(plcy, None, x2=x2)
    assert eng.ctx.names() == ["oly_disc_pack", "oly_disc_reward_step_pair", "oly_disc_reward_step_pair"]
    first, second = eng.ctx.calls[1][1], eng.ctx.calls[2][1]
    #   B, Dx, Ds, x, mask, pair, colstats, stats_a, accumulate, weights, packed, eps, reward, logits, mu, logvar, stream
    assert first == [N_PLCY, OBS, DS, True, True, _pair_block(pair, w2), True, True, 0, False, True, True, True, True, True,
                     True, False]
    assert second == [N_PLCY, OBS, DS, True, True, _pair_block(pair, w2), True, True, 1, [True] * 10, True, False, True,
                      False, False, False, False]
    eng.ctx.calls.clear()
    o = r.predict(plcy, eps=eps, x2=x2)
    assert list(o) == ["logits"] and eng.ctx.names() == ["oly_disc_pack", "oly_disc_forward_pair"]
    #   B, Dx, Ds, x, mask, pair, stats_a, stats_b, packed, eps, reward, logits, mu, logvar, stream
    assert eng.ctx.calls[1][1] == [N_PLCY, OBS, DS, True, True, _pair_block(pair, w2), True, True, True, True, False, True,
                                   False, False, False]
    with pytest.raises(OlyError, match="unknown output 'value'"):
        r.forward(plcy, eps, want=("value",), x2=x2)
    with pytest.raises(OlyError, match="no output requested"):
        r.predict(plcy, eps=eps, want=(), x2=x2)
