"""K15-K22 and K25 on fenced and poisoned buffers (tests/fences.py), at the smallest shapes of their own tables at which
each path can go wrong: the imitation-learning fit, reward, logging, act and reset kernels.

As tests/test_gpu_fences.py does for K10-K14, K23 and K24, every case hands every pointer argument as a Fenced tensor
(inputs copied in, pure outputs poisoned with 0xFF bytes, index and mask buffers fenced int32 / uint8, tables that are
gathered from built with gathered=True), sizes every workspace and packed stream to exactly the number the library
reports, compares the results with the float64 restatement and at the tolerance of the kernel's existing test, and then
asserts that
  * every margin is intact (no write outside a buffer, the last float of a workspace included),
  * every buffer listed as fully written next to the case holds no poisoned element (no store forgotten),
  * no compared output holds a NaN (a read outside an input reads NaN, or index -1, from a margin),
  * in-place buffers keep the bytes the header says they keep.
Every call is a valid call or a documented refusal that launches nothing.  tests/il_fence_ledger.py names the test of
every entry point."""
import contextlib
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import bc_restate as br
import disc_log_restate as dlr
import fences as fn
import il_act_restate as ar
import il_shapes as sh
import iter_log_restate as ilr
import pair_restate as pr
import trpo_restate as tr
from fences import Bufs
from il_shapes import K15_CASES, K16_CASES, K17_CASES, TOL, case_id
from olympic_hip import _abi
from olympic_hip._ffi import OlyError, lib, ptr
from test_disc_fit_cpu import rel
from test_gail_disc_cpu import forward as gail_forward
from test_gail_disc_cpu import gen as gail_gen
from test_gail_disc_cpu import restate_fit as gail_restate_fit
from test_gpu_disc_log import SHAPES as K19_SHAPES
from test_gpu_disc_log import check_scalars
from test_gpu_disc_log import shape_case as k19_case
from test_gpu_disc_pair import PAIRS_ACTION, PAIRS_NEXT, ROWS, sweep_case
from test_gpu_gail_disc import gail_case
from test_gpu_il_act import ACT_SHAPES, act_case
from test_gpu_il_critic import close, dev_params, make_net, ref_forward
from test_gpu_il_reset import make_vec
from test_gpu_il_shapes import critic_shapes, disc_shapes, same_stats
from test_gpu_iter_log import DEV_TOL as K20_TOL
from test_gpu_iter_log import EP_SHAPES, check_episode, episode_blocks
from test_gpu_iter_log import SHAPES as K20_SHAPES
from test_gpu_iter_log import shape_case as k20_case
from test_gpu_sg_act import SHAPES as K25_SHAPES
from test_gpu_sg_act import float64_of, sg_case, switch_rows
from test_trpo_cpu import rel as trel

pytestmark = pytest.mark.gpu
F32, F64, I32, U8 = torch.float32, torch.float64, torch.int32, torch.uint8


@pytest.fixture(scope="module")
def eng():
    from olympic_hip import specs
    from olympic_hip.engine import Engine
    e = Engine(0).il_configure(specs.unitree_h1("walk"))      # 11 actions: the controls of the K21 / K25 cases with A = 11
    yield e
    torch.cuda.synchronize()
    e.ctx.close()
    gc.collect()


def _flat(params):
    return np.concatenate([np.asarray(p, dtype=np.float32).reshape(-1) for p in params])


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _poisoned(t):
    """The number of float32 elements of the tensor (a view into a poisoned buffer) whose bytes are all still 0xFF."""
    return int((t.contiguous().view(I32) == -1).sum())


def _pack(eng, b, tag, net, params):
    """oly_disc_pack ("vail") / oly_ilmlp_pack of fenced copies of `params` into a fenced, poisoned stream of exactly
    oly_disc_packed_floats / oly_ilmlp_packed_floats floats.  Fully written: the stream (its zero padding included)."""
    D, out_dim = int(np.asarray(_np(params[0])).shape[1]), int(np.asarray(_np(params[-1])).shape[0])
    w = [b.inp(f"{tag}.w{i}", _np(p).astype(np.float32)) for i, p in enumerate(params)]
    if net == "vail":
        pk = b.out(f"{tag}.packed", int(lib().oly_disc_packed_floats(D, 256, 128, 128)), F32)
        eng.disc_pack(*w, packed=pk)
    else:
        pk = b.out(f"{tag}.packed", int(lib().oly_ilmlp_packed_floats(D, 512, 256, out_dim)), F32)
        eng.ilmlp_pack(*w, packed=pk)
    b.done(f"pack {tag}", written=(f"{tag}.packed",), finite=(f"{tag}.packed",))
    return pk


@contextlib.contextmanager
def one_float_short(eng, b):
    """Inside the context the argument block of every call reaches the library with a workspace one float short: a
    fenced, poisoned buffer b["ws_short"] of ws_floats - 1 floats and that size in ws_floats.  The typed front end has
    then already passed the full-sized workspace, so the refusal is the library's own."""
    real = eng.ctx.call

    def call(name, *args):
        blk = args[0]._obj
        n = int(blk.ws_floats) - 1
        blk.ws, blk.ws_floats = b.out("ws_short", n, F32).data_ptr(), n
        return real(name, *args)
    eng.ctx.call = call
    try:
        yield
    finally:
        del eng.ctx.call


def assert_refused(eng, b, what, call, outputs, kept=()):
    """`call` with its workspace one float short: OlyError for the workspace, nothing launched."""
    snap = {k: b[k].snapshot() for k in kept}
    with one_float_short(eng, b):
        with pytest.raises(OlyError, match=r": ws [(m]"):
            call()
    torch.cuda.synchronize()
    fn.assert_untouched({k: b[k] for k in tuple(outputs) + ("ws", "ws_short")}, what)
    fn.assert_intact(b, what)
    assert all(b[k].same_as(snap[k]) for k in kept), what


# ------------------------------------------------------------------------------ K15 and K18: the discriminators' fits
FIT_ROWS = {(7, 20, 10), (3, 10, 5), (64, 199, 99), (512, 300, 300), (333, 1022, 0)}
FIT_CASES = tuple(c for c in K15_CASES if (c.batch, c.n_rows, c.n_plcy) in FIT_ROWS)
# (mode, (Ds, D2), (batch, n_rows, n_plcy), seed): actions go in raw (pair->standardise 0), next states are standardised
FIT_PAIRS = (("action", (1, 1), (7, 20, 10), 0), ("action", (33, 31), (64, 199, 99), 3), ("action", (63, 1), (333, 1022, 0), 5),
             ("action", (33, 31), (512, 300, 300), 2), ("next_state", (17, 17), (3, 10, 5), 8))
FIT_KEYS = dict(vail=("loss", "bce", "kl", "beta"), gail=("loss", "bce", "ent"))
FIT_STATE = ("param", "m", "v")                  # in place: copied in, so only the float64 comparison can check them


def test_the_fit_tables_hold_what_the_fenced_cases_need():
    assert len(FIT_CASES) == 5 and {(c.in_dim, c.batch, c.n_rows) for c in FIT_CASES} == {
        (1, 7, 20), (17, 3, 10), (33, 64, 199), (45, 512, 300), (64, 333, 1022)}
    assert any(c.targets for c in FIT_CASES) and any(c.n_plcy == 0 for c in FIT_CASES)
    assert all(p in PAIRS_ACTION for m, p, _, _ in FIT_PAIRS if m == "action")
    assert all(p[0] == p[1] for m, p, _, _ in FIT_PAIRS if m == "next_state") and (32, 32) in PAIRS_NEXT
    assert all(r in ROWS for _, _, r, _ in FIT_PAIRS)


def _fit_ws_floats(algo, batch, ds, d2, standardise):
    stem = "oly_gail_disc_fit" if algo == "gail" else "oly_disc_fit"
    if d2 == 0:
        return int(getattr(lib(), stem + "_ws_floats")(batch, ds))
    return int(getattr(lib(), stem + "_pair_ws_floats")(batch, ds, d2, int(standardise)))


def _fit_buffers(b, algo, params, ds, d2, batch, standardise):
    """The fit's state, fenced.  packed is poisoned: both fits re-pack it from param at the start of a call, so it is a
    pure output.  ws: exactly the reported floats."""
    flat = _flat(params)
    st = dict(param=b.inp("param", flat), m=b.inp("m", np.zeros_like(flat)), v=b.inp("v", np.zeros_like(flat)),
              cs=b.inp("colstats", np.zeros((3, ds))), step=0)
    if algo == "vail":
        st["beta"] = b.inp("beta", np.array([0.1], np.float32))
        st["packed"] = b.out("packed", int(lib().oly_disc_packed_floats(ds + d2, 256, 128, 128)), F32)
        st["views"] = sh.views(st["param"], disc_shapes(ds + d2))
    else:
        st["packed"] = b.out("packed", int(lib().oly_ilmlp_packed_floats(ds + d2, 512, 256, 1)), F32)
        st["views"] = sh.views(st["param"], critic_shapes(ds + d2))
    st["ws"] = b.out("ws", _fit_ws_floats(algo, batch, ds, d2, standardise), F32)
    return st


def _fit_epoch(eng, b, algo, st, e, ep, n_plcy, h, standardise, launch=True):
    """One epoch (x, x2 or None, perm, targets or None, noise or None) on fenced operands: the caller's oly_col_stats
    of the states, then the fit's entry point.  Fully written: packed (poisoned before the first epoch: the opening
    re-pack stores the whole stream) and the per-minibatch outputs loss / bce / kl / beta (VAIL), loss / bce / ent
    (GAIL).  In place: param, m, v, colstats, beta."""
    x, x2, perm, t, noise = ep
    n = int(x.shape[0])
    nb = (n + h["batch"] - 1) // h["batch"]
    xd = b.inp(f"x{e}", x, gathered=True)
    x2d = b.inp(f"x2{e}", x2, gathered=True)
    pd = b.inp(f"perm{e}", np.asarray(perm).astype(np.int32))
    td = b.inp(f"targets{e}", t, gathered=True)
    o = {k: b.out(f"{k}{e}", nb, F32 if k == "beta" else F64) for k in FIT_KEYS[algo]}
    eng.col_stats(xd, st["cs"])
    common = (h["batch"], st["cs"], st["param"], st["m"], st["v"], st["packed"])
    kw = dict(weight_decay=h["wd"], targets=td, loss_out=o["loss"], bce_out=o["bce"])
    if algo == "vail":
        nz = b.inp(f"noise{e}", noise)
        kw.update(info_constraint=h["info_c"], lr_beta=h["lr_beta"], kl_out=o["kl"], beta_out=o["beta"])
        tail = common + (st["beta"], st["ws"], st["step"], h["lr"])
        call = ((lambda: eng.disc_fit_epoch(xd, n_plcy, nz, pd, *tail, **kw)) if x2 is None else
                (lambda: eng.disc_fit_epoch_pair(xd, x2d, standardise, n_plcy, nz, pd, *tail, **kw)))
    else:
        kw.update(entcoeff=h["entcoeff"], ent_out=o["ent"])
        tail = common + (st["ws"], st["step"], h["lr"])
        call = ((lambda: eng.gail_disc_fit_epoch(xd, n_plcy, pd, *tail, **kw)) if x2 is None else
                (lambda: eng.gail_disc_fit_epoch_pair(xd, x2d, standardise, n_plcy, pd, *tail, **kw)))
    names = tuple(f"{k}{e}" for k in FIT_KEYS[algo])
    if not launch:
        return call, names
    call()
    st["step"] += nb
    b.done(f"{algo} fit epoch {e}", written=("packed",) + names, finite=FIT_STATE + ("packed", "colstats") + names)
    return {k: b.host(f"{k}{e}").astype(np.float64) for k in FIT_KEYS[algo]}


def _fit_case(eng, algo, params, epochs, n_plcy, h, ds, d2, standardise, ref, cs_atol=0.0):
    """Two epochs on one set of buffers (the second reuses the workspace and starts from a current stream), then the
    comparisons of test_disc_fit_shapes / test_fit_shapes / test_fit_and_reward_shapes with their tolerance il_shapes.TOL."""
    b = Bufs()
    st = _fit_buffers(b, algo, params, ds, d2, h["batch"], standardise)
    recs = [_fit_epoch(eng, b, algo, st, e, ep, n_plcy, h, standardise) for e, ep in enumerate(epochs)]
    rec = {k: np.concatenate([r[k] for r in recs]) for k in FIT_KEYS[algo]}
    P, cs, rec64, step = ref
    assert st["step"] == step
    for i, (a, w) in enumerate(zip(st["views"], P)):
        r = rel(a.cpu().numpy(), w.cpu().numpy())
        print(f"{algo} tensor {i}: {r:.2e} from float64")
        assert r <= TOL, (i, r)
    for k in rec:
        np.testing.assert_allclose(rec[k], rec64[k], rtol=TOL, atol=TOL, err_msg=k)
    if algo == "vail":
        assert float(st["beta"]) == pytest.approx(rec64["beta"][-1], abs=TOL)
    got, want = b.host("colstats"), cs.cpu().numpy()
    assert np.array_equal(got[0], want[0]), "the count"
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=cs_atol)
    # the stream is the stepped parameters': oly_disc_pack / oly_ilmlp_pack of fenced copies of them, fenced itself
    fresh = _pack(eng, b, "final", algo, [v.cpu().numpy() for v in st["views"]])
    assert torch.equal(st["packed"], fresh), "the packed stream is the stepped parameters'"
    b.done("the fit")
    return b, st


def _plain_epochs(epochs):
    """(x, perm, targets[, noise]) of il_shapes.disc_case / test_gpu_gail_disc.gail_case as _fit_epoch's five."""
    return [(ep[0], None, ep[1], ep[2], ep[3] if len(ep) > 3 else None) for ep in epochs]


@pytest.mark.parametrize("c", FIT_CASES, ids=case_id)
def test_k15_disc_fit_epoch(eng, c):
    """oly_disc_pack and oly_disc_fit_epoch against il_shapes.disc_restate at il_shapes.TOL."""
    params, epochs, h = sh.disc_case(c)
    P, _, cs, rec64, step = sh.disc_restate(c, device="cuda")
    _fit_case(eng, "vail", params, _plain_epochs(epochs), c.n_plcy, h, c.in_dim, 0, False, (P, cs, rec64, step))


@pytest.mark.parametrize("c", FIT_CASES, ids=case_id)
def test_k18_gail_disc_fit_epoch(eng, c):
    """oly_ilmlp_pack (out 1) and oly_gail_disc_fit_epoch against test_gail_disc_cpu.restate_fit at il_shapes.TOL, the
    cases of test_gpu_gail_disc.test_fit_shapes."""
    params, epochs, h = gail_case(c)
    P, _, cs, rec64, step = gail_restate_fit(epochs, c.n_plcy, params, np.zeros((3, c.in_dim)), h["entcoeff"], h["lr"],
                                             h["batch"], wd=h["wd"], device="cuda")
    _fit_case(eng, "gail", params, _plain_epochs(epochs), c.n_plcy, h, c.in_dim, 0, False, (P, cs, rec64, step))


PAIR_IDS = [f"{m}-{p[0]}+{p[1]}-b{r[0]}n{r[1]}" for m, p, r, _ in FIT_PAIRS]


def _pair_fit(eng, algo, mode, pair, rows, seed):
    (ds, d2), (batch, n_rows, n_plcy), ns = pair, rows, mode == "next_state"
    params, epochs, h = sweep_case(algo, mode, ds, d2, batch, n_rows, n_plcy, seed)
    out = pr.restate_fit(algo, epochs, n_plcy, params, np.zeros((3, ds)), ns, device="cuda", **h)
    # atol 1e-9 on the statistics: test_fit_and_reward_shapes' own (tests/test_gpu_disc_pair.py)
    return _fit_case(eng, algo, params, epochs, n_plcy, h, ds, d2, ns, (out[0], out[2], out[3], out[4]), cs_atol=1e-9)


@pytest.mark.parametrize("mode,pair,rows,seed", FIT_PAIRS, ids=PAIR_IDS)
def test_k15_disc_fit_epoch_pair(eng, mode, pair, rows, seed):
    """oly_disc_fit_epoch_pair against pair_restate.restate_fit at il_shapes.TOL; the workspace has exactly
    oly_disc_fit_pair_ws_floats floats."""
    _pair_fit(eng, "vail", mode, pair, rows, seed)


@pytest.mark.parametrize("mode,pair,rows,seed", FIT_PAIRS, ids=PAIR_IDS)
def test_k18_gail_disc_fit_epoch_pair(eng, mode, pair, rows, seed):
    """oly_gail_disc_fit_epoch_pair, as above with oly_gail_disc_fit_pair_ws_floats."""
    _pair_fit(eng, "gail", mode, pair, rows, seed)


@pytest.mark.parametrize("algo", ["vail", "gail"])
@pytest.mark.parametrize("paired", [False, True], ids=["plain", "pair"])
def test_k15_k18_fit_workspace_one_float_short_is_refused_and_nothing_is_launched(eng, algo, paired):
    if paired:
        mode, (ds, d2), (batch, n_rows, n_plcy), seed = FIT_PAIRS[1]
        params, epochs, h = sweep_case(algo, mode, ds, d2, batch, n_rows, n_plcy, seed)
    else:
        c = FIT_CASES[2]
        ds, d2, n_plcy = c.in_dim, 0, c.n_plcy
        params, epochs, h = sh.disc_case(c) if algo == "vail" else gail_case(c)
        epochs = _plain_epochs(epochs)
    b = Bufs()
    st = _fit_buffers(b, algo, params, ds, d2, h["batch"], False)
    call, names = _fit_epoch(eng, b, algo, st, 0, epochs[0], n_plcy, h, False, launch=False)
    kept = ("param", "m", "v") + (("beta",) if algo == "vail" else ())
    assert_refused(eng, b, f"{algo} fit", call, names + ("packed",), kept)


# ------------------------------------------------------------------------------ K16
def _hi_rows():
    """The smallest N at which oly_ilmlp_forward, the GAIL reward and K21 / K25 take 32-row tiles (ragged: 32 k + 1)."""
    return switch_rows()[1]


@pytest.mark.parametrize("act", ["identity", "tanh"])
@pytest.mark.parametrize("out_dim", [1, 11, 32])
def test_k16_ilmlp_pack_and_forward(eng, out_dim, act):
    """oly_ilmlp_pack and oly_ilmlp_forward against test_gpu_il_critic.ref_forward (float64) at its tolerance
    (close: 1e-5 of the output's scale), N 1 / 17 / 33 on 16-row tiles and the first ragged N on 32-row tiles, with
    colstats, with mean / std and without standardisation.  Fully written: the stream, y."""
    in_dim = 45
    lins = make_net(in_dim, out_dim, 100 * in_dim + out_dim)
    b = Bufs()
    packed = _pack(eng, b, "net", "ilmlp", [p.cpu().numpy() for p in dev_params(lins)])
    g = torch.Generator(device="cuda").manual_seed(in_dim + out_dim)
    hi = _hi_rows()
    assert hi <= 17000
    big = (torch.randn((hi, in_dim), device="cuda", generator=g) * 2.0 + 0.5).contiguous()
    cs0 = torch.stack([torch.full((in_dim,), 5000.0, device="cuda", dtype=F64), big[:5000].double().sum(0),
                       (big[:5000].double() ** 2).sum(0)]).contiguous()
    mean0, std0 = big.double().mean(0).contiguous(), big.double().std(0).contiguous()
    cs, mean, std = b.inp("colstats", cs0), b.inp("mean", mean0), b.inp("std", std0)
    for N in (1, 17, 33, hi):
        x = b.inp(f"x{N}", big[:N])
        for mode in ("colstats", "meanstd", "none"):
            if N == hi and mode != "colstats":
                continue
            kw = dict(colstats=cs) if mode == "colstats" else dict(mean=mean, std=std) if mode == "meanstd" else {}
            rkw = dict(colstats=cs0) if mode == "colstats" else dict(mean=mean0, std=std0) if mode == "meanstd" else {}
            name = f"y{N}{mode}"
            y = eng.ilmlp_forward(x, packed, out_dim, act, y=b.out(name, (N, out_dim), F32), **kw)
            b.done(f"ilmlp_forward N={N} {mode}", written=(name,), finite=(name,))
            close(y, ref_forward(big[:N], lins, act, **rkw))


K16_FIT = tuple(c for c in K16_CASES if (c.in_dim, c.batch, c.n) in {(1, 7, 20), (33, 100, 37), (45, 255, 320), (64, 1, 5)})
K16_STATE = ("param", "m", "v", "net.packed", "colstats")      # all in place


def _critic_buffers(eng, b, c, params, cs):
    flat = _flat(params)
    st = dict(param=b.inp("param", flat), m=b.inp("m", np.zeros_like(flat)), v=b.inp("v", np.zeros_like(flat)),
              cs=b.inp("colstats", cs), step=0)
    st["views"] = sh.views(st["param"], critic_shapes(c.in_dim))
    # in / out: this fit has no opening re-pack, the stream must be current on entry and Adam stores the parameters'
    # positions only (the zero padding is the pack's)
    st["packed"] = _pack(eng, b, "net", "ilmlp", params)
    st["ws"] = b.out("ws", int(lib().oly_il_critic_fit_ws_floats(c.batch, c.in_dim)), F32)
    return st


def _critic_epoch(eng, b, c, st, e, xd, vd, perm):
    nb = (c.n + c.batch - 1) // c.batch
    pd, lo = b.inp(f"perm{e}", np.asarray(perm).astype(np.int32)), b.out(f"loss{e}", nb, F64)
    return (lambda: eng.il_critic_fit_epoch(xd, vd, pd, c.batch, st["cs"], st["param"], st["m"], st["v"], st["packed"],
                                            st["ws"], st["step"], c.lr, loss_out=lo)), nb


@pytest.mark.parametrize("c", K16_FIT, ids=case_id)
def test_k16_il_critic_fit_epoch(eng, c):
    """oly_il_critic_fit_epoch against il_shapes.critic_restate at il_shapes.TOL, two epochs on one workspace.  Fully
    written: loss_out.  In place: param, m, v, colstats and packed, which is read and must be current on entry; that
    it stays current, padding included, is the comparison with a fresh oly_ilmlp_pack at the end."""
    assert len(K16_FIT) == 4
    params, x, vt, perms, cs = sh.critic_case(c)
    b = Bufs()
    st = _critic_buffers(eng, b, c, params, cs)
    xd, vd = b.inp("x", x, gathered=True), b.inp("v_target", vt, gathered=True)
    losses = []
    for e, perm in enumerate(perms):
        call, nb = _critic_epoch(eng, b, c, st, e, xd, vd, perm)
        call()
        st["step"] += nb
        b.done(f"critic fit epoch {e}", written=(f"loss{e}",), finite=K16_STATE + (f"loss{e}",))
        losses.append(b.host(f"loss{e}"))
    P, _, cs64, losses64, step = sh.critic_restate(c, device="cuda")
    assert st["step"] == step
    for i, (a, w) in enumerate(zip(st["views"], P)):
        r = rel(a.cpu().numpy(), w.cpu().numpy())
        print(f"K16 tensor {i}: {r:.2e} from float64")
        assert r <= TOL, (i, r)
    np.testing.assert_allclose(np.concatenate(losses), losses64[-2 * nb:], rtol=TOL)
    got, want = b.host("colstats"), cs64.cpu().numpy()
    assert np.array_equal(got[0], want[0]), "the count"
    np.testing.assert_allclose(got, want, rtol=1e-12)
    fresh = _pack(eng, b, "final", "ilmlp", [v.cpu().numpy() for v in st["views"]])
    assert torch.equal(st["packed"], fresh), "the packed stream is the stepped parameters'"
    b.done("the critic's fit")


def test_k16_fit_workspace_one_float_short_is_refused_and_nothing_is_launched(eng):
    c = K16_FIT[1]
    params, x, vt, perms, cs = sh.critic_case(c)
    b = Bufs()
    st = _critic_buffers(eng, b, c, params, cs)
    call, _ = _critic_epoch(eng, b, c, st, 0, b.inp("x", x, gathered=True), b.inp("v_target", vt, gathered=True), perms[0])
    assert_refused(eng, b, "il_critic_fit_epoch", call, ("loss0",), K16_STATE)


# ------------------------------------------------------------------------------ K17
K17_SEL = tuple(c for c in K17_CASES if (c.D, c.A, c.n) in {(1, 1, 65), (17, 1, 1), (45, 11, 63), (64, 32, 257), (64, 32, 16385)})


def _trpo_block(eng, b, c, case, **kw):
    """The oly_trpo_step_args block on fenced operands: obs, act, adv, colstats, theta, the scalar block (poisoned) and a
    poisoned workspace of exactly oly_trpo_ws_floats floats."""
    ws = b.out("ws", int(lib().oly_trpo_ws_floats(c.n, c.D, 512, 256, c.A)), F32)
    a, keep = eng.trpo_args(b.inp("x", case["x"]), b.inp("act", case["act"]), b.inp("adv", case["adv"]),
                            b.inp("colstats", case["S"]), b.inp("theta", case["theta"]), ws=ws,
                            scal_out=b.out("scal", _abi.OLY_TRPO_SCALARS, F64), **kw)
    return a, keep


@pytest.mark.parametrize("c", K17_SEL, ids=case_id)
def test_k17_trpo_grad_and_fvp(eng, c):
    """oly_trpo_grad and oly_trpo_fvp at k_stats 1 and 4 against il_shapes.trpo_grad_fvp_reference at il_shapes.TOL, the
    comparisons of test_trpo_grad_and_fvp_shapes, straight at the C entries so that logp_old, mu_old, log_sigma_old, p, act,
    adv and j_out are fenced too.  Fully written: grad_out, j_out, out.  Kept: theta, colstats; scal_out stays poisoned."""
    assert len(K17_SEL) == 5
    case = sh.trpo_case(c, device="cuda")
    n_par = tr.n_params(c.D, c.A)
    for k in (1, 4):
        J, g, prod, inp = sh.trpo_grad_fvp_reference(c, case, k)
        b = Bufs()
        a, _ = _trpo_block(eng, b, c, case, ent_coeff=sh.K17_STEP["ent_coeff"], cg_damping=0.1)
        snap = {key: b[key].snapshot() for key in ("theta", "colstats")}
        g_dev, J_dev, got = b.out("grad_out", n_par, F32), b.out("j_out", 1, F64), b.out("out", n_par, F32)
        eng.ctx.call("oly_trpo_grad", C.byref(a), k, ptr(b.inp("logp_old", inp["logp_old"])), ptr(g_dev), ptr(J_dev), eng._s())
        b.done(f"trpo_grad k={k}", written=("grad_out", "j_out"), finite=("grad_out", "j_out"))
        eng.ctx.call("oly_trpo_fvp", C.byref(a), k, ptr(b.inp("mu_old", inp["mu_old"])),
                     ptr(b.inp("log_sigma_old", inp["log_sigma_old"])), ptr(b.inp("p", inp["p"])), ptr(got), eng._s())
        b.done(f"trpo_fvp k={k}", written=("grad_out", "j_out", "out"), finite=("grad_out", "j_out", "out"))
        eg, ep = trel(g_dev, g), trel(got, prod)
        print(f"K17 {case_id(c)} k={k}: g {eg:.2e}, product {ep:.2e}, J {abs(float(J_dev) - float(J)):.2e}")
        assert eg <= TOL, (k, eg)
        assert abs(float(J_dev) - float(J)) <= TOL * max(1.0, abs(float(J)))
        assert ep <= TOL, (k, ep)
        assert all(b[key].same_as(snap[key]) for key in snap), "theta and colstats are only read"
        fn.assert_untouched(dict(scal=b["scal"]), "oly_trpo_grad and oly_trpo_fvp leave the step's scalar block alone")


K17_STEP_OUT = ("stepdir_out", "full_step_out", "scal", "packed")


def _trpo_step_buffers(eng, b, c, case):
    n_par = tr.n_params(c.D, c.A)
    return _trpo_block(eng, b, c, case, stepdir_out=b.out("stepdir_out", n_par, F32),
                       full_step_out=b.out("full_step_out", n_par, F32),
                       packed=b.out("packed", int(lib().oly_ilmlp_packed_floats(c.D, 512, 256, c.A)), F32), **sh.K17_STEP)


@pytest.mark.parametrize("c", [c for c in K17_SEL if c.n >= sh.K17_STEP_MIN_ROWS], ids=case_id)
def test_k17_trpo_step(eng, c):
    """oly_trpo_step against trpo_restate.trpo_step with the comparisons of test_trpo_step_shapes (no farther from
    float64 than twice the float32 restatement).  Fully written: stepdir_out, full_step_out, the scalar block, packed (the
    closing re-pack), and inside the workspace the old distribution K20 reads in place (oly_trpo_old_offsets).  In
    place: theta, colstats."""
    case = sh.trpo_case(c, device="cuda")
    kw = sh.K17_STEP
    b = Bufs()
    a, keep = _trpo_step_buffers(eng, b, c, case)
    eng.ctx.call("oly_trpo_step", C.byref(a), eng._s())
    b.done("trpo_step", written=K17_STEP_OUT, finite=K17_STEP_OUT + ("theta", "colstats"))
    r64 = tr.trpo_step(case["theta"], case["S"], case["x"], case["act"], case["adv"], **kw)
    r32 = tr.trpo_step(case["theta"], case["S"], case["x"], case["act"], case["adv"], dtype=F32, **kw)
    v = b.host("scal").tolist()
    assert (int(v[3]), int(v[6]), int(v[1])) == (r64["j"], r64["j_run"], r64["k_run"])
    assert same_stats(b["colstats"].t, r64["S"])
    th0 = case["theta"].double()
    for key, got in (("stepdir", b["stepdir_out"].t), ("theta", b["theta"].t)):
        if key == "stepdir":
            e_dev, e_32 = trel(got, r64[key]), trel(r32[key], r64[key])
        else:
            e_dev, e_32 = trel(got.double() - th0, r64[key] - th0), trel(r32[key].double() - th0, r64[key] - th0)
        print(f"K17 step {key}: device {e_dev:.2e}, float32 restatement {e_32:.2e} from float64")
        assert e_dev <= 2 * e_32 + 1e-6, (key, e_dev, e_32)
    # the old distribution, where K20 reads it: every element stored, mu_old the float64 forward's at S + c
    mu_old, ls_old = eng.trpo_old_distribution(b["ws"].t, c.n, c.D, c.A)
    assert _poisoned(mu_old) == 0 and _poisoned(ls_old) == 0
    assert torch.equal(ls_old, case["theta"][-c.A:])
    assert trel(mu_old, sh.trpo_old_dist(case, c.D, c.A)[1]) <= TOL
    W = [t.contiguous() for t in tr.split(b["theta"].t, c.D, c.A)[:6]]
    fresh = _pack(eng, b, "final", "ilmlp", [w.cpu().numpy() for w in W])
    assert torch.equal(b["packed"].t, fresh), "the packed stream is the stepped parameters'"


@pytest.mark.parametrize("entry", ["oly_trpo_grad", "oly_trpo_fvp", "oly_trpo_step"])
def test_k17_workspace_one_float_short_is_refused_and_nothing_is_launched(eng, entry):
    c = K17_SEL[2]
    case = sh.trpo_case(c, device="cuda")
    n_par = tr.n_params(c.D, c.A)
    b = Bufs()
    a, _ = _trpo_step_buffers(eng, b, c, case)
    outs = K17_STEP_OUT
    if entry == "oly_trpo_step":
        call = lambda: eng.ctx.call(entry, C.byref(a), eng._s())                                      # noqa: E731
    else:
        inp = sh.trpo_grad_fvp_reference(c, case, 1)[3]
        outs += ("out", "j_out")
        out, j = b.out("out", n_par, F32), b.out("j_out", 1, F64)
        if entry == "oly_trpo_grad":
            lp = b.inp("logp_old", inp["logp_old"])
            call = lambda: eng.ctx.call(entry, C.byref(a), 1, ptr(lp), ptr(out), ptr(j), eng._s())    # noqa: E731
        else:
            mu, ls, p = b.inp("mu_old", inp["mu_old"]), b.inp("log_sigma_old", inp["log_sigma_old"]), b.inp("p", inp["p"])
            call = lambda: eng.ctx.call(entry, C.byref(a), 1, ptr(mu), ptr(ls), ptr(p), ptr(out), eng._s())   # noqa: E731
    assert_refused(eng, b, entry, call, outs, ("theta", "colstats"))


# ------------------------------------------------------------------------------ K18: the reward and the forward
def _moments(cs):
    cnt = cs[0] + 1e-2
    mean = cs[1] / cnt
    return mean, torch.sqrt(torch.clamp((cs[2] + 1e-2) / cnt - mean * mean, min=1e-2))


def _sums(x):
    xd = x.double()
    return torch.stack([torch.full((x.shape[1],), float(x.shape[0]), dtype=F64, device=x.device), xd.sum(0), (xd * xd).sum(0)])


def _check_reward(b, tag, d64, what):
    """logits against float64 at test_reward_forward_against_float64's 2e-5 (tests/test_gpu_gail_disc.py); the reward
    within what a logit that far off allows, |dr / dd| = sigmoid(d) <= 1, plus the float32 steps of the formula: the
    bound of test_fit_and_reward_against_the_reference_fixture (tests/test_gpu_disc_pair.py)."""
    d, r = b.host(f"{tag}.logits"), b.host(f"{tag}.reward")
    d64 = d64.cpu().numpy()
    assert rel(d, d64) <= 2e-5, what
    np.testing.assert_allclose(d, d64, rtol=2e-5, atol=2e-5, err_msg=what)
    r64 = -np.log(1.0 - 1.0 / (1.0 + np.exp(-d64)) + 1e-8)
    assert (np.abs(r - r64) <= TOL * (1 + np.abs(d64)) + 2e-6).all(), what


def _k18_rows(B):
    return _hi_rows() if B == "hi" else B


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("B", [1, 31, 33, "hi"])
def test_k18_gail_reward_step_and_forward(eng, B, masked):
    """oly_gail_reward_step (accumulate 0 into poisoned statistics with the stream rebuilt from fenced weights, then
    accumulate 1) and oly_gail_disc_forward on those statistics, against the float64 forward.  B 1 / 31 / 33 run 16-row
    tiles, "hi" the first ragged batch on 32-row tiles.  Fully written: reward, logits, colstats (accumulate 0), packed."""
    B = _k18_rows(B)
    D, Dx = 32, 36 if masked else 32
    rng = np.random.default_rng(B + 3 * masked)
    params = gail_gen.init_params(seed=7 + B % 5, in_dim=D)
    mask = np.sort(rng.choice(Dx, D, replace=False)).astype(np.int32) if masked else None
    x = (rng.normal(0.0, 1.0, (B, Dx)) * rng.uniform(0.3, 3.0, Dx) + rng.normal(0, 1, Dx)).astype(np.float32)
    xm = torch.as_tensor(x if mask is None else x[:, mask]).cuda()
    P64 = [torch.as_tensor(p).cuda().double() for p in params]
    b = Bufs()
    xd, md = b.inp("x", x), b.inp("mask", mask)
    w = [b.inp(f"w{i}", p) for i, p in enumerate(params)]
    packed = b.out("packed", int(lib().oly_ilmlp_packed_floats(D, 512, 256, 1)), F32)
    cs = b.out("colstats", (3, D), F64)                 # accumulate = 0 overwrites it: a pure output of the first call
    S = torch.zeros((3, D), dtype=F64, device="cuda")
    for acc in (0, 1):
        out = dict(reward=b.out(f"{acc}.reward", B, F32), logits=b.out(f"{acc}.logits", B, F32))
        eng.gail_reward_step(xd, packed, cs, acc, mask=md, want=("reward", "logits"), out=out, weights=w if acc == 0 else None)
        names = (f"{acc}.reward", f"{acc}.logits", "colstats", "packed")
        b.done(f"gail_reward_step accumulate={acc}", written=names, finite=names)
        S = S + _sums(xm)
        np.testing.assert_allclose(b.host("colstats"), S.cpu().numpy(), rtol=1e-12)
        assert float(b.host("colstats")[0, 0]) == (acc + 1) * B
        mean, sd = _moments(cs)
        _check_reward(b, str(acc), gail_forward(P64, ((xm.double() - mean) / sd).float().double()), f"accumulate={acc}")
    out = dict(reward=b.out("f.reward", B, F32), logits=b.out("f.logits", B, F32))
    eng.gail_disc_forward(xd, packed, mask=md, colstats=cs, want=("reward", "logits"), out=out)
    b.done("gail_disc_forward", written=("f.reward", "f.logits"), finite=("f.reward", "f.logits"))
    assert torch.equal(out["logits"], b["1.logits"].t) and torch.equal(out["reward"], b["1.reward"].t)
    # mean / std given explicitly, the reward alone: the other output pointer NULL
    mean, sd = _moments(cs)
    r = b.out("alone", B, F32)
    eng.gail_disc_forward(xd, packed, mask=md, mean=b.inp("mean", mean), std=b.inp("std", sd), out=dict(reward=r))
    b.done("gail_disc_forward mean / std", written=("alone",), finite=("alone",))
    assert torch.equal(r, out["reward"])
    assert torch.equal(packed, _pack(eng, b, "fresh", "ilmlp", params))


@pytest.mark.parametrize("mode,pair", [("action", (1, 1)), ("action", (33, 31)), ("action", (63, 1)), ("next_state", (17, 17))],
                         ids=["action-1+1", "action-33+31", "action-63+1", "next_state-17+17"])
@pytest.mark.parametrize("B", [1, 31, 33, "hi"])
def test_k18_gail_reward_step_and_forward_pair(eng, B, mode, pair):
    """oly_gail_reward_step_pair and oly_gail_disc_forward_pair against pair_restate.restate_reward, both sources masked
    in the kernel.  Fully written: reward, logits, colstats (accumulate 0), stats_a (next states), packed."""
    B = _k18_rows(B)
    (ds, d2), ns = pair, mode == "next_state"
    rng = np.random.default_rng(B + ds)
    Dx, W2 = ds + 3, (ds + 3 if ns else d2 + 2)
    mask = np.sort(rng.choice(Dx, ds, replace=False)).astype(np.int32)
    mask2 = mask if ns else np.sort(rng.choice(W2, d2, replace=False)).astype(np.int32)
    scale = rng.uniform(0.3, 3.0, Dx)
    x = (rng.normal(0, 1, (B, Dx)) * scale + rng.normal(0, 1, Dx)).astype(np.float32)
    x2 = ((0.6 * x + 1.5 * scale + rng.normal(0, 0.5, (B, Dx)) * scale) if ns else rng.normal(0.2, 0.8, (B, W2))).astype(np.float32)
    params = pr.gen.gail_init(ds + d2, seed=9 + ds)
    b = Bufs()
    xd, x2d, md = b.inp("x", x), b.inp("x2", x2), b.inp("mask", mask)
    m2d = md if ns else b.inp("mask2", mask2)
    w = [b.inp(f"w{i}", p) for i, p in enumerate(params)]
    packed = b.out("packed", int(lib().oly_ilmlp_packed_floats(ds + d2, 512, 256, 1)), F32)
    cs, sa = b.out("colstats", (3, ds), F64), b.out("stats_a", (3, ds), F64)
    out = dict(reward=b.out("s.reward", B, F32), logits=b.out("s.logits", B, F32))
    eng.gail_reward_step_pair(xd, x2d, packed, cs, sa, 0, ns, mask=md, mask2=m2d, want=("reward", "logits"), out=out, weights=w)
    names = ("s.reward", "s.logits", "colstats", "packed") + (("stats_a",) if ns else ())
    b.done("gail_reward_step_pair", written=names, finite=names)
    d64, _, cs64 = pr.restate_reward("gail", params, np.zeros((3, ds)), x[:, mask], x2[:, mask2], ns, device="cuda")
    _check_reward(b, "s", d64, "reward step")
    np.testing.assert_allclose(b.host("colstats"), cs64.cpu().numpy(), rtol=1e-12, atol=1e-9)
    assert float(b.host("colstats")[0, 0]) == (2 if ns else 1) * B
    if ns:
        assert float(b.host("stats_a")[0, 0]) == B            # S1: the states are in, the next states not yet
    else:
        fn.assert_untouched(dict(stats_a=b["stats_a"]), "actions: stats_a is not touched")
    out = dict(reward=b.out("f.reward", B, F32), logits=b.out("f.logits", B, F32))
    eng.gail_disc_forward_pair(xd, x2d, packed, ns, mask=md, mask2=m2d, stats_a=sa if ns else cs, stats_b=cs if ns else None,
                               want=("reward", "logits"), out=out)
    b.done("gail_disc_forward_pair", written=("f.reward", "f.logits"), finite=("f.reward", "f.logits"))
    _check_reward(b, "f", d64, "forward")


# ------------------------------------------------------------------------------ K19
#          the three smallest entries of test_gpu_disc_log.SHAPES (one row in each half among them), a ragged GAIL case with
#          targets, and one paired case per algorithm
K19_SEL = (("gail", 1, 0, None, 1, 1, False), ("vail", 1, 0, None, 33, 20, False), ("vail", 64, 0, None, 1, 1, True),
           ("gail", 17, 0, None, 33, 20, True), ("gail", 32, 32, "next_state", 257, 100, False),
           ("vail", 20, 7, "action", 257, 31, True))


def _k19_buffers(eng, b, a):
    """Every operand of oly_gail_disc_log / oly_disc_log for test_gpu_disc_log.shape_case's arguments, fenced: x, x2,
    targets, the noise, beta, the stream (packed from fenced weights), colstats (in place), out (poisoned) and a
    poisoned workspace of exactly oly_*_disc_log_ws_floats floats."""
    gail = a["algo"] == "gail"
    n = a["x"].shape[0]
    need = lib().oly_gail_disc_log_ws_floats if gail else lib().oly_disc_log_ws_floats
    packed = _pack(eng, b, "net", a["algo"], a["params"])
    kw = dict(x2=b.inp("x2", a["x2"]), standardise=a["pair"] == "next_state", targets=b.inp("targets", a["targets"]),
              out=b.out("out", 12, F64), entcoeff=a["entcoeff"])
    x, cs, ws = b.inp("x", a["x"]), b.inp("colstats", a["colstats"]), b.out("ws", int(need(n)), F32)
    if gail:
        return lambda: eng.gail_disc_log(x, a["n_plcy"], cs, packed, ws, **kw)
    eps = b.inp("eps", None if a["noise"] is None else np.concatenate(a["noise"]))
    beta = b.inp("beta", np.array([a["beta"]], np.float32))
    return lambda: eng.disc_log(x, a["n_plcy"], cs, packed, beta, ws, info_constraint=a["info_c"], lr_beta=a["lr_beta"],
                                eps=eps, **kw)


@pytest.mark.parametrize("shape", K19_SEL, ids=[f"{s[0]}-{s[1]}+{s[2]}-p{s[4]}d{s[5]}" for s in K19_SEL])
def test_k19_disc_log(eng, shape):
    """oly_gail_disc_log / oly_disc_log against disc_log_restate.restate_log with test_shapes_against_the_restatement's
    comparisons (disc_log_restate.TOL).  Fully written: out (all twelve; GAIL stores 0 in the last three).  In place:
    colstats, left at the last block of the chain; beta is only read."""
    assert all(s in K19_SHAPES for s in K19_SEL) and set(K19_SHAPES[:2]) <= set(K19_SEL)
    a = k19_case(*shape, seed=11 + K19_SHAPES.index(shape))
    b = Bufs()
    call = _k19_buffers(eng, b, a)
    beta0 = b["beta"].snapshot() if "beta" in b else None
    call()
    b.done("disc_log", written=("out",), finite=("out", "colstats"))
    ref = dlr.restate_log(device="cuda", **a)
    got, cs = b.host("out"), b.host("colstats")
    check_scalars(got, ref["scalars"], ref["logits"], a["n_plcy"], label="-".join(str(v) for v in shape[:6]))
    assert np.all(np.abs(cs - ref["colstats"]) <= 1e-12 * np.maximum(1, np.abs(ref["colstats"])))
    k = (5 if shape[0] == "vail" else 4) * (2 if shape[3] == "next_state" else 1)
    assert cs[0, 0] - a["colstats"][0, 0] == k * a["x"].shape[0]
    if shape[0] == "gail":
        assert np.all(got[9:] == 0)
    else:
        assert b["beta"].same_as(beta0)


@pytest.mark.parametrize("shape", [K19_SEL[3], K19_SEL[5]], ids=["gail", "vail-pair"])
def test_k19_workspace_one_float_short_is_refused_and_nothing_is_launched(eng, shape):
    a = k19_case(*shape, seed=11 + K19_SHAPES.index(shape))
    b = Bufs()
    assert_refused(eng, b, "disc_log", _k19_buffers(eng, b, a), ("out",), ("colstats",))


# ------------------------------------------------------------------------------ K20
@pytest.mark.parametrize("r64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", [(1, 1), (1, 65), (33, 257)], ids=["1x1", "1x65", "33x257"])
def test_k20_episode_stats(eng, shape, r64):
    """oly_episode_stats against iter_log_restate.episode_stats with test_episode_stats_against_the_restatement's
    comparisons, gamma 1 and 0.99, with and without the second reward block; the flags are fenced uint8.  Fully
    written: out (all eight)."""
    T, N = shape
    assert shape in EP_SHAPES
    r, r2, last = episode_blocks(T, N, seed=3 + T + N)
    rew = r if r64 else r.astype(np.float32)
    b = Bufs()
    rd, r2d, ld = b.inp("rew", rew), b.inp("rew2", r2), b.inp("last", last.astype(np.uint8))
    for gamma in (1.0, 0.99):
        want2 = ilr.episode_stats(rew, last, gamma, reward2=r2)
        want1 = want2.copy()
        want1[[1, 6]] = 0.0
        for two in (False, True):
            name = f"out{gamma}{two}"
            eng.episode_stats(rd, ld, gamma=gamma, reward2=r2d if two else None, out=b.out(name, 8, F64))
            b.done(f"episode_stats gamma={gamma} two={two}", written=(name,))
            check_episode(b.host(name), want2 if two else want1, two)


def _k20_buffers(eng, b, a):
    """Every operand of oly_iter_log for test_gpu_iter_log.shape_case's arguments, fenced.  The old distribution sits
    where oly_trpo_step leaves it (oly_trpo_old_offsets) in a fenced K17 workspace of exactly oly_trpo_ws_floats floats
    whose every other float is poison: K20 reads it in place."""
    n, D = a["x"].shape
    A = a["mu_old"].shape[1]
    T, N = a["last"].shape
    tws = b.out("trpo_ws", int(lib().oly_trpo_ws_floats(n, D, 512, 256, A)), F32)
    mu_old, ls_old = eng.trpo_old_distribution(tws, n, D, A)
    mu_old.copy_(torch.as_tensor(a["mu_old"]).cuda())
    ls_old.copy_(torch.as_tensor(a["ls_old"]).cuda())
    critic, policy = _pack(eng, b, "critic", "ilmlp", a["critic"]), _pack(eng, b, "policy", "ilmlp", a["policy"])
    args = (b.inp("x", a["x"]), b.inp("v_target", a["v_target"]), mu_old, ls_old, b.inp("log_sigma", a["log_sigma"]), critic,
            policy, b.inp("r_env", a["r_env"]), b.inp("r", a["r"]), b.inp("last", a["last"].astype(np.uint8)),
            b.inp("colstats", a["colstats"]), b.out("ws", int(lib().oly_iter_log_ws_floats(n)), F32))
    out = b.out("out", 8, F64)
    return lambda: eng.iter_log(*args, out=out)


K20_SEL = (K20_SHAPES[0], K20_SHAPES[1])


@pytest.mark.parametrize("shape", K20_SEL, ids=["x".join(str(v) for v in s) for s in K20_SEL])
def test_k20_iter_log(eng, shape):
    """oly_iter_log against iter_log_restate.restate_iter_log with test_shapes_against_the_restatement's comparisons
    (DEV_TOL of tests/test_gpu_iter_log.py).  Fully written: out (all eight).  In place: colstats, left at S + 2c, the
    bits of two accumulating oly_col_stats calls."""
    assert K20_SEL == ((1, 1, 17, 1), (255, 1, 45, 11))
    a = k20_case(*shape, seed=21 + K20_SHAPES.index(shape))
    b = Bufs()
    _k20_buffers(eng, b, a)()
    b.done("iter_log", written=("out",), finite=("colstats",))
    ref = ilr.restate_iter_log(device="cuda", **a)
    got, want, cs = b.host("out"), ref["scalars"], b.host("colstats")
    for i in ilr.EPISODE:
        assert abs(got[i] - want[i]) <= ilr.EP_TOL * abs(want[i])
    assert (np.isnan(got[2]) and np.isnan(want[2])) or got[2] == want[2]
    assert (np.isnan(got[6]) and np.isnan(want[6])) or got[6] == want[6]
    assert got[7] == want[7]
    assert want[5] > 0.05                                                           # the KL is of order one by design
    err = ilr.rel_err(got[3:6], want[3:6])
    assert np.all(err <= K20_TOL), dict(zip(ilr.NAMES[3:], err))
    assert np.all(np.abs(cs - ref["colstats"]) <= 1e-12 * np.maximum(1, np.abs(ref["colstats"])))
    two = torch.as_tensor(a["colstats"]).cuda()
    for _ in range(2):
        two = eng.col_stats(b["x"].t, two)
    assert torch.equal(b["colstats"].t, two)


def test_k20_workspace_one_float_short_is_refused_and_nothing_is_launched(eng):
    a = k20_case(*K20_SEL[1], seed=22)
    b = Bufs()
    assert_refused(eng, b, "iter_log", _k20_buffers(eng, b, a), ("out",), ("colstats",))


# ------------------------------------------------------------------------------ K21
K21_SEL = ((1, 32, 11), (15, 17, 1), (17, 45, 17), (33, 64, 32))


@pytest.mark.parametrize("update", (True, False), ids=("update", "frozen"))
@pytest.mark.parametrize("shape", K21_SEL, ids=["x".join(map(str, s)) for s in K21_SEL])
def test_k21_il_act(eng, shape, update):
    """oly_il_act against il_act_restate.restate_act with test_act_against_the_separate_kernels_and_float64's bounds
    (il_act_restate.DEV_TOL); with A = 11, the configured robot's, the controls at float32 and float64 against
    il_act_restate.restate_ctrl, exactly.  Fully written: action, mu, ctrl (every actuator column: those no action
    drives hold 0).  In place: colstats (kept byte for byte when frozen)."""
    assert all(s in ACT_SHAPES for s in K21_SEL)
    n, D, A = shape
    params, log_sigma, cs0, x, eps = act_case(n, D, A, seed=11 + n + D + A)
    ref = ar.restate_act(params, log_sigma, cs0, x, eps=eps, update_stats=update, device="cuda")
    spec = eng.il_spec
    for ctrl64 in ((False, True) if A == int(spec.n_act) else (None,)):
        b = Bufs()
        packed = _pack(eng, b, "net", "ilmlp", params)
        cs = b.inp("colstats", cs0)
        snap = b["colstats"].snapshot()
        out = dict(action=b.out("action", (n, A), F32), mu=b.out("mu", (n, A), F32))
        names = ("action", "mu")
        if ctrl64 is not None:
            out["ctrl"] = b.out("ctrl", (n, spec.nu), F64 if ctrl64 else F32)
            names += ("ctrl",)
        eng.il_act(b.inp("x", x), packed, b.inp("log_sigma", log_sigma), cs, eps=b.inp("eps", eps), update_stats=update,
                   want_mu=True, want_ctrl=ctrl64 is not None, ctrl_f64=bool(ctrl64), out=out)
        b.done("il_act", written=names, finite=names + ("colstats",))
        mu, act = b.host("mu"), b.host("action")
        assert (np.abs(mu - ref["mu"]) / np.maximum(1.0, np.abs(ref["mu"]))).max() <= ar.DEV_TOL
        assert np.abs(act - ref["action"]).max() <= 2 * ar.DEV_TOL * max(1.0, np.abs(ref["action"]).max())
        want_cs = ref["colstats"]
        assert np.all(np.abs(b.host("colstats") - want_cs) <= 1e-12 * np.maximum(1.0, np.abs(want_cs)))
        assert update or b["colstats"].same_as(snap)
        if ctrl64 is not None:
            c64, _ = ar.restate_ctrl(spec, act)
            got = b.host("ctrl").astype(np.float64)
            assert np.array_equal(got, c64 if ctrl64 else c64.astype(np.float32).astype(np.float64))
    # deterministic: eps NULL, mu not asked for
    b2 = Bufs()
    o = eng.il_act(b2.inp("x", x), _pack(eng, b2, "net", "ilmlp", params), b2.inp("log_sigma", log_sigma),
                   b2.inp("colstats", cs0), update_stats=update, out=dict(action=b2.out("action", (n, A), F32)))
    b2.done("il_act deterministic", written=("action",), finite=("action", "colstats"))
    assert torch.equal(o["action"], b["mu"].t)


# ------------------------------------------------------------------------------ K25
K25_SEL = ((1, 1, 1, True), (45, 19, 7, True), (33, 33, 11, True), (40, 64, 16, False))


@pytest.mark.parametrize("n,D,A,st", K25_SEL, ids=[f"n{n}-in{D}-A{A}" + ("" if st else "-nostd") for n, D, A, st in K25_SEL])
def test_k25_sg_act(eng, n, D, A, st):
    """oly_sg_act against test_gpu_sg_act.float64_of at its TOL (bc_restate.TOL), with the control output (A = 11, at
    float32 and float64, against il_act_restate.restate_ctrl exactly) and without.  Fully written: action, log_prob, mu,
    log_sigma, ctrl.  In place: colstats (the rows added once)."""
    assert all(s in K25_SHAPES for s in K25_SEL)
    k = sg_case(n, D, A, seed=n % 97 + D + A, standardizer=st)
    spec = eng.il_spec
    for ctrl64 in ((None, False, True) if A == int(spec.n_act) else (None,)):
        b = Bufs()
        packed = _pack(eng, b, "net", "ilmlp", k["params"])
        cs = b.inp("colstats", np.zeros((3, D))) if st else None
        names = ("action", "log_prob", "mu", "log_sigma")
        out = dict(action=b.out("action", (n, A), F32), log_prob=b.out("log_prob", n, F32), mu=b.out("mu", (n, A), F32),
                   log_sigma=b.out("log_sigma", (n, A), F32))
        if ctrl64 is not None:
            out["ctrl"] = b.out("ctrl", (n, spec.nu), F64 if ctrl64 else F32)
            names += ("ctrl",)
        o = eng.sg_act(b.inp("x", k["x"]), packed, b.inp("central", k["central"]), b.inp("delta", k["delta"]), colstats=cs,
                       eps=b.inp("eps", k["eps"]), want=names[1:], ctrl_f64=bool(ctrl64), out=out)
        b.done("sg_act", written=names, finite=names + (("colstats",) if st else ()))
        if st:
            assert float(cs[0, 0]) == n
            np.testing.assert_allclose(b.host("colstats"), _sums(torch.as_tensor(k["x"])).numpy(), rtol=1e-12)
        mu64, ls64, raw64, a64, lp64 = float64_of(k, cs, A)
        assert float(ls64.abs().max()) < 1.0 and float(raw64.abs().max()) < 4.0, "the case's conditioning"
        assert float((o["action"].double() - a64).abs().max()) <= br.TOL
        assert float(((o["log_prob"].double() - lp64).abs() / lp64.abs().clamp(min=1.0)).max()) <= br.TOL
        assert float((o["mu"].double() - mu64).abs().max()) <= br.TOL and float((o["log_sigma"].double() - ls64).abs().max()) <= br.TOL
        if ctrl64 is not None:
            c64, _ = ar.restate_ctrl(spec, b.host("action"))
            got = b.host("ctrl").astype(np.float64)
            assert np.array_equal(got, c64 if ctrl64 else c64.astype(np.float32).astype(np.float64))
    # the squashed mean: eps NULL, the optional outputs NULL
    b2 = Bufs()
    det = eng.sg_act(b2.inp("x", k["x"]), _pack(eng, b2, "net", "ilmlp", k["params"]), b2.inp("central", k["central"]),
                     b2.inp("delta", k["delta"]), colstats=b2.inp("colstats", np.zeros((3, D))) if st else None, want=(),
                     out=dict(action=b2.out("action", (n, A), F32)))
    b2.done("sg_act deterministic", written=("action",), finite=("action",))
    ref = torch.tanh(mu64) * torch.as_tensor(k["delta"]).cuda().double() + torch.as_tensor(k["central"]).cuda().double()
    assert float((det["action"].double() - ref).abs().max()) <= br.TOL


# ------------------------------------------------------------------------------ K22
K22_STATE = ("cur_traj", "cur_step", "origin", "sample", "qpos", "qvel", "prev", "episode_steps")
K22_OF = dict(cur_traj="_cur_traj", cur_step="_cur_step", origin="_origin", sample="_sample", prev="_prev",
              episode_steps="episode_steps")


def _k22_call(eng, b, N, obs_f64, in_place=False, traj=True):
    """oly_il_reset_where straight at the C entry on the buffers of b, the two inverse address tables fenced as well."""
    qs, vs = eng.il_reset_tables()
    if "qpos_slot" not in b:
        b.inp("qpos_slot", qs), b.inp("qvel_slot", vs)
    p = dict(n=N, out_flags=_abi.OUT_OBS_F64 if obs_f64 else 0, qpos_slot=b["qpos_slot"].t.data_ptr(),
             qvel_slot=b["qvel_slot"].t.data_ptr())
    names = ("mask", "qpos", "qvel", "obs_in", "prev", "episode_steps")
    names += ("traj_no", "step", "cur_traj", "cur_step", "origin", "sample") if traj else ()
    p.update({k: b[k].t.data_ptr() for k in names})
    p["obs_out"] = b["obs_in" if in_place else "obs_out"].t.data_ptr()
    eng.ctx.call("oly_il_reset_where", C.byref(_abi.ILReset(**p)), eng._s())


def _k22_state(vec):
    d = {k: getattr(vec, a).clone() for k, a in K22_OF.items()}
    d.update(qpos=vec.physics.qpos.clone(), qvel=vec.physics.qvel.clone(), obs=vec._obs.clone())
    return d


@pytest.mark.parametrize("N", (1, 5, 257))
@pytest.mark.parametrize("robot", ("h1", "h1_ff"))
def test_k22_il_reset_where(robot, N):
    """oly_il_reset_where against the host-driven reset(env_mask=) bit for bit, as
    test_reset_where_is_the_host_reset_bit_for_bit, for flags all clear, all set and mixed, observations float32 and
    float64.  Fully written: obs_out when it is not obs_in (the rows whose flag is clear are copied from obs_in).  In
    place: the cursor, the state rows, prev and episode_steps keep the rows whose flag is clear byte for byte; with every
    flag clear and obs_out == obs_in nothing at all is stored."""
    A = make_vec(robot, N)
    try:
        eng = A.eng
        J, L = A.trajectories.number_of_trajectories, A.trajectories.trajectory_length
        n_grf = int(A.spec.n_grf)
        assert n_grf == (6 if robot == "h1_ff" else 0)
        gen = torch.Generator(device="cuda").manual_seed(11 + N)
        A.reset()
        g = np.random.default_rng(7 + N)
        mixed = g.uniform(size=N) < 0.5
        if N > 1:
            mixed[0], mixed[-1] = True, False
        case = 0
        for obs_f64 in (False, True):
            A.obs_f64 = obs_f64
            for mname, m in (("clear", np.zeros(N, bool)), ("set", np.ones(N, bool)), ("mixed", mixed)):
                case += 1
                for _ in range(2):                          # prev, episode_steps and the observation are live values
                    A.step(torch.randn((N, A.spec.n_act), device="cuda", generator=gen))
                if n_grf:
                    # the replayed physics reports no contacts; give the ground-force columns live values by hand
                    A._obs[:, -n_grf:] = torch.arange(1, N * n_grf + 1, device="cuda", dtype=A._obs.dtype).reshape(N, n_grf) / 8
                pre = _k22_state(A)
                seed = 100 * N + case
                rng = np.random.default_rng(seed)           # the order reset() draws them in
                tn, st = rng.integers(0, J, N).astype(np.int32), rng.integers(0, L, N).astype(np.int32)
                b = Bufs()
                for k in K22_STATE:
                    b.inp(k, pre[k])
                b.inp("obs_in", pre["obs"]), b.inp("mask", m.astype(np.uint8)), b.inp("traj_no", tn), b.inp("step", st)
                b.out("obs_out", tuple(pre["obs"].shape), pre["obs"].dtype)
                snap = {k: f.snapshot() for k, f in b.items()}
                tag = f"{robot} N={N} f64={obs_f64} flags {mname}"
                if not m.any():
                    # in place (obs_out == obs_in) and no flag set: nothing at all is stored, the unused buffer included
                    _k22_call(eng, b, N, obs_f64, in_place=True)
                    torch.cuda.synchronize()
                    fn.assert_untouched(dict(obs_out=b["obs_out"]), tag)
                    changed = [k for k in snap if not b[k].same_as(snap[k])]
                    assert not changed, f"{tag}: obs_out == obs_in and no flag set, yet {changed} were stored"
                _k22_call(eng, b, N, obs_f64)
                b.done(tag, written=("obs_out",), finite=("obs_out", "qpos", "qvel", "prev", "origin", "sample"))
                assert b["obs_in"].same_as(snap["obs_in"]), tag
                A._rng = np.random.default_rng(seed)
                md = torch.as_tensor(m).cuda()
                oa = A.reset(env_mask=md)
                host = dict(_k22_state(A), obs=oa)
                for k in K22_STATE + ("obs",):
                    got = b["obs_out" if k == "obs" else k].t
                    assert torch.equal(got[md], host[k][md]), (tag, k)            # reset rows: the host path's bits
                    assert torch.equal(got[~md], pre[k][~md]), (tag, k)           # the others keep theirs
                if n_grf and m.any():
                    assert bool((b["obs_out"].t[md][:, -n_grf:] == 0).all()), tag
                if not m.any():
                    assert all(b[k].same_as(snap[k]) for k in K22_STATE), tag
    finally:
        torch.cuda.synchronize()
        A.eng.ctx.close()
        gc.collect()


@pytest.mark.parametrize("robot", ("h1", "h1_ff"))
def test_k22_il_reset_where_without_a_trajectory(robot):
    """traj_no NULL: the state rows of the flagged environments are zeroed and the observation, prev and the counter
    follow from that, as test_without_a_trajectory_the_state_rows_are_zeroed; the cursor pointers are NULL."""
    from helpers import h1_synthetic_block
    from olympic_hip import specs
    from olympic_hip.envs import ReplayPhysics, VecLocoEnv
    N = 5
    spec = specs.unitree_h1("walk")
    if robot == "h1_ff":
        spec.with_foot_forces("UnitreeH1")
    qpos, qvel, _ = h1_synthetic_block(spec, 2, N, seed=8)
    vec = VecLocoEnv(spec, N, physics=ReplayPhysics(spec, torch.as_tensor(qpos).cuda(), torch.as_tensor(qvel).cuda()),
                     random_start=False)
    try:
        vec.reset()
        vec.step(torch.zeros((N, spec.n_act), device="cuda"))
        pre = dict(qpos=vec.physics.qpos.clone(), qvel=vec.physics.qvel.clone(), prev=vec._prev.clone(),
                   episode_steps=vec.episode_steps.clone(), obs=vec._obs.clone())
        m = np.array([True, False, True, True, False])
        md = torch.as_tensor(m).cuda()
        b = Bufs()
        for k in ("qpos", "qvel", "prev", "episode_steps"):
            b.inp(k, pre[k])
        b.inp("obs_in", pre["obs"]), b.inp("mask", m.astype(np.uint8))
        b.out("obs_out", tuple(pre["obs"].shape), pre["obs"].dtype)
        _k22_call(vec.eng, b, N, pre["obs"].dtype == F64, traj=False)
        b.done("no trajectory", written=("obs_out",), finite=("obs_out", "qpos", "qvel", "prev"))
        for k in ("qpos", "qvel", "prev", "obs", "episode_steps"):
            got = b["obs_out" if k == "obs" else k].t
            assert int(got[md].count_nonzero()) == 0, k                        # the zero state and its observation
            assert torch.equal(got[~md], pre[k][~md]), k
    finally:
        torch.cuda.synchronize()
        vec.eng.ctx.close()
        gc.collect()


# ------------------------------------------------------------------------------ what the engine allocates itself
def test_engine_allocated_outputs_and_workspaces_of_k15_to_k22_and_k25(eng):
    """One small call each through the Engine methods of K15-K22 and K25 that allocate their own outputs or workspaces,
    every allocation fenced and poisoned (fences.fence_engine): no margin written, no returned output with an element
    never stored.  The values are the fenced cases' above; here only NaNs are looked for."""
    d = lambda a, dt=None: None if a is None else torch.as_tensor(np.ascontiguousarray(_np(a))).to(device="cuda", dtype=dt)  # noqa: E731
    with fn.fence_engine(eng) as ef:
        def returned(what, *tensors):
            torch.cuda.synchronize()
            ef.check(what)
            for t in tensors:
                f = ef.of(t)
                assert f.unwritten() == 0, (what, f.shape, f.unwritten())
                assert not t.dtype.is_floating_point or not bool(torch.isnan(t).any()), (what, f.shape)
        # K15 / K18: the streams, the workspaces and loss_out, plain and paired
        for algo in ("vail", "gail"):
            for paired in (False, True):
                if paired:
                    mode, (ds, d2), (batch, n_rows, n_plcy), seed = FIT_PAIRS[0]
                    params, epochs, h = sweep_case(algo, mode, ds, d2, batch, n_rows, n_plcy, seed)
                else:
                    c = FIT_CASES[1]
                    ds, d2, batch, n_plcy = c.in_dim, 0, c.batch, c.n_plcy
                    params, epochs, h = sh.disc_case(c) if algo == "vail" else gail_case(c)
                    epochs = _plain_epochs(epochs)
                x, x2, perm, t, noise = epochs[0]
                flat = d(_flat(params))
                views = sh.views(flat, (disc_shapes if algo == "vail" else critic_shapes)(ds + d2))
                packed = (eng.disc_pack if algo == "vail" else eng.ilmlp_pack)(*views)
                returned(f"{algo} pack", packed)
                m, v, cs = torch.zeros_like(flat), torch.zeros_like(flat), torch.zeros((3, ds), dtype=F64, device="cuda")
                stem = "disc_fit" if algo == "vail" else "gail_disc_fit"
                ws = getattr(eng, stem + "_pair_ws")(batch, ds, d2, False) if paired else getattr(eng, stem + "_ws")(batch, ds)
                assert ef.of(ws).n == _fit_ws_floats(algo, batch, ds, d2, False)
                head = (d(x),) + ((d(x2), False) if paired else ()) + (n_plcy,)
                tail = (d(perm, I32), batch, cs, flat, m, v, packed)
                fit = getattr(eng, stem + "_epoch" + ("_pair" if paired else ""))
                if algo == "vail":
                    loss = fit(*head, d(noise), *tail, torch.full((1,), 0.1, device="cuda"), ws, 0, h["lr"], targets=d(t))
                else:
                    loss = fit(*head, *tail, ws, 0, h["lr"], targets=d(t))
                returned(f"{algo} fit paired={paired}", loss, packed)
        # K16: the stream, y, the workspace and loss_out
        c = K16_FIT[1]
        params, x, vt, perms, cs0 = sh.critic_case(c)
        flat = d(_flat(params))
        packed = eng.ilmlp_pack(*sh.views(flat, critic_shapes(c.in_dim)))
        y = eng.ilmlp_forward(d(x), packed, 1, "tanh", colstats=d(cs0))
        returned("ilmlp_pack, ilmlp_forward", packed, y)
        ws = eng.il_critic_fit_ws(c.batch, c.in_dim)
        assert ef.of(ws).n == int(lib().oly_il_critic_fit_ws_floats(c.batch, c.in_dim))
        loss = eng.il_critic_fit_epoch(d(x), d(vt), d(perms[0], I32), c.batch, d(cs0), flat, torch.zeros_like(flat),
                                       torch.zeros_like(flat), packed, ws, 0, c.lr)
        returned("il_critic_fit_epoch", loss, packed)
        # K17: the workspace of the step, grad_out and out
        c = K17_SEL[2]
        case = sh.trpo_case(c, device="cuda")
        inp = sh.trpo_grad_fvp_reference(c, case, 1)[3]
        g, _ = eng.trpo_grad(case["x"], case["act"], case["adv"], case["S"].clone(), case["theta"], inp["logp_old"])
        out = eng.trpo_fvp(case["x"], case["S"].clone(), case["theta"], inp["mu_old"], inp["log_sigma_old"], inp["p"])
        returned("trpo_grad, trpo_fvp", g, out)
        scal = eng.trpo_step(case["x"], case["act"], case["adv"], case["S"].clone(), case["theta"].clone(), **sh.K17_STEP)
        returned("trpo_step")
        assert not bool(torch.isnan(scal).any())
        # K18: every output of the reward
        rng = np.random.default_rng(5)
        w = [d(p) for p in gail_gen.init_params(seed=7, in_dim=32)]
        x18 = d(rng.normal(0, 1, (33, 32)).astype(np.float32))
        pk = eng.ilmlp_pack(*w)
        cs = torch.zeros((3, 32), dtype=F64, device="cuda")
        o = eng.gail_reward_step(x18, pk, cs, False, want=("reward", "logits"))
        o2 = eng.gail_disc_forward(x18, pk, colstats=cs, want=("reward", "logits"))
        returned("gail_reward_step, gail_disc_forward", pk, *o.values(), *o2.values())
        for ns, x2 in ((False, d(rng.normal(0.2, 0.8, (33, 9)).astype(np.float32))), (True, (0.6 * x18 + 1.0).contiguous())):
            pkp = eng.ilmlp_pack(*[d(p) for p in pr.gen.gail_init(32 + int(x2.shape[1]), seed=3)])
            cs, sa = (torch.zeros((3, 32), dtype=F64, device="cuda") for _ in range(2))
            o = eng.gail_reward_step_pair(x18, x2, pkp, cs, sa, False, ns, want=("reward", "logits"))
            o2 = eng.gail_disc_forward_pair(x18, x2, pkp, ns, stats_a=sa if ns else cs, stats_b=cs if ns else None,
                                            want=("reward", "logits"))
            returned(f"gail_reward_step_pair, gail_disc_forward_pair next states={ns}", pkp, *o.values(), *o2.values())
        # K19: the workspaces and out
        for shape in (K19_SEL[3], K19_SEL[1]):
            a = k19_case(*shape, seed=11 + K19_SHAPES.index(shape))
            n = a["x"].shape[0]
            if a["algo"] == "gail":
                ws = eng.gail_disc_log_ws(n)
                assert ef.of(ws).n == int(lib().oly_gail_disc_log_ws_floats(n))
                out = eng.gail_disc_log(d(a["x"]), a["n_plcy"], d(a["colstats"]), eng.ilmlp_pack(*[d(p) for p in a["params"]]),
                                        ws, entcoeff=a["entcoeff"], targets=d(a["targets"]))
            else:
                ws = eng.disc_log_ws(n)
                assert ef.of(ws).n == int(lib().oly_disc_log_ws_floats(n))
                out = eng.disc_log(d(a["x"]), a["n_plcy"], d(a["colstats"]), eng.disc_pack(*[d(p) for p in a["params"]]),
                                   d(np.array([a["beta"]], np.float32)), ws, info_constraint=a["info_c"], lr_beta=a["lr_beta"],
                                   eps=d(np.concatenate(a["noise"])), entcoeff=a["entcoeff"])
            returned(f"{a['algo']} disc_log", out)
        # K20: out of both entries, the workspace
        r, r2, last = episode_blocks(33, 257, seed=4)
        returned("episode_stats", eng.episode_stats(d(r), d(last), gamma=0.99, reward2=d(r2)))
        a = k20_case(*K20_SEL[1], seed=22)
        n = a["x"].shape[0]
        ws = eng.iter_log_ws(n)
        assert ef.of(ws).n == int(lib().oly_iter_log_ws_floats(n))
        out = eng.iter_log(d(a["x"]), d(a["v_target"]), d(a["mu_old"]), d(a["ls_old"]), d(a["log_sigma"]),
                           eng.ilmlp_pack(*[d(p) for p in a["critic"]]), eng.ilmlp_pack(*[d(p) for p in a["policy"]]),
                           d(a["r_env"]), d(a["r"]), d(a["last"]), d(a["colstats"]), ws)
        returned("iter_log")
        assert ef.of(out).unwritten() == 0
        # K21 and K25: every output, the controls included
        n, D, A = K21_SEL[0]
        params, log_sigma, cs0, x, eps = act_case(n, D, A, seed=3)
        o = eng.il_act(d(x), eng.ilmlp_pack(*[d(p) for p in params]), d(log_sigma), d(cs0), eps=d(eps), want_mu=True,
                       want_ctrl=True)
        returned("il_act", *o.values())
        n, D, A, st = K25_SEL[2]
        k = sg_case(n, D, A, seed=5)
        o = eng.sg_act(d(k["x"]), eng.ilmlp_pack(*[d(p) for p in k["params"]]), d(k["central"]), d(k["delta"]),
                       colstats=torch.zeros((3, D), dtype=F64, device="cuda"), eps=d(k["eps"]),
                       want=("log_prob", "mu", "log_sigma", "ctrl"))
        returned("sg_act", *o.values())
        ef.check("the end")
    assert "_new" not in eng.__dict__
