"""The inverse action model's fit and draw (GaussianInvActionModel, imitation_lib/utils/action_models.py:257-528) on the
rows of two indexed tables, restated in float64: the yardstick of tests/test_gpu_iam.py.  No tests here.

The model is IQ_Learn_Policy's network on the concatenated row (s | s'), fitted by GaussianNLLLoss + Adam to the
un-squashed raw actions of a replay ring.  That is K24's arithmetic on the rows (states[i, :d1] | next_states[i, :d2]),
i = idx[step, r], so the fit's twin is tests/bc_restate.py's restate() on the materialised table; the draw's twin is the
network in float64 with one Standardizer over the whole row.

The second half twins the reference-run fixtures of tests/golden/gen_iam_fit.py: ModelTwin / sequence_twin the action
model through four logging iterations, fo_fit_twin the whole IQfO_SAC.fit / LSIQfO.fit.

CASES is the table of the issue: every (d1, d2), A and batch it names, strides wider than the widths in half the cases, a
ring of 40 rows, three steps, an index with duplicates inside a batch and the entries 0 and n_rows - 1."""
from collections import namedtuple

import numpy as np
import torch

import bc_restate as br
from il_shapes import _columns

TOL = br.TOL
RING = 40
STEPS = 3

IAMCase = namedtuple("IAMCase", "d1 d2 A batch pad1 pad2 standardizer seed")

#          d1  d2   A  batch pad1 pad2
CASES = (
    IAMCase(1, 1, 1, 1, 0, 0, True, 1),          # one column each, one row: every tile all but empty
    IAMCase(5, 12, 8, 15, 3, 1, True, 2),        # the boundary inside the first 16 columns; strides wider
    IAMCase(16, 17, 9, 16, 0, 0, True, 3),       # the boundary on a k-group's edge; two output tiles; one full tile
    IAMCase(32, 32, 16, 17, 4, 9, True, 4),      # the widest row, the <4> instantiation; 16 + 1 rows; strides wider
    IAMCase(3, 61, 9, 33, 0, 0, True, 5),        # the second table across all four k-groups; 16 + 16 + 1 rows
    IAMCase(5, 12, 16, 33, 2, 5, False, 6),      # no Standardizer; strides wider
)


def case_id(c):
    return (f"d{c.d1}+{c.d2}-A{c.A}-b{c.batch}" + ("-wide" if c.pad1 or c.pad2 else "")
            + ("" if c.standardizer else "-nostd"))


def build(c, n_rows=RING, steps=STEPS):
    """dict(params f32, states [n, d1 + pad1] f32 and next_states [n, d2 + pad2] f32 with NaN in the columns beyond the
    widths (a read there shows in every sum), actions [n, A] f32 with elements at and beyond the bounds, central /
    delta f32, min_a / max_a f64, idx [steps, batch] int32, table [n, d1 + d2] f32 the materialised rows, targets
    [n, A] f32 the un-squashed actions (behavioral_cloning.py:63-66 in float32), eps [n, A] f32 noise for the draw)."""
    rng = np.random.default_rng(7000 + c.seed)
    D = c.d1 + c.d2
    scale, shift = _columns(rng, D) if c.standardizer else (np.full(D, 0.5), np.zeros(D))
    table = (rng.standard_normal((n_rows, D)) * scale + shift).astype(np.float32)
    states = np.full((n_rows, c.d1 + c.pad1), np.nan, np.float32)
    next_states = np.full((n_rows, c.d2 + c.pad2), np.nan, np.float32)
    states[:, :c.d1] = table[:, :c.d1]
    next_states[:, :c.d2] = table[:, c.d1:]
    min_a, max_a = -rng.uniform(0.5, 2.0, c.A), rng.uniform(0.5, 3.0, c.A)
    central, delta = (0.5 * (max_a + min_a)).astype(np.float32), (0.5 * (max_a - min_a)).astype(np.float32)
    u = np.tanh(0.8 * rng.standard_normal((n_rows, c.A)))
    actions = (central + delta * u).astype(np.float32)
    # the ring's raw actions are what the policy sent, not what the environment clipped: at and beyond the bounds
    where = rng.uniform(0, 1, actions.shape)
    actions = np.where(where < 0.08, np.float32(min_a)[None, :], actions)
    actions = np.where(where > 0.92, (np.float32(max_a) + np.float32(0.25))[None, :], actions).astype(np.float32)
    actions[0, 0] = np.float32(min_a[0]) - np.float32(0.5)
    actions[n_rows - 1, c.A - 1] = np.float32(max_a[c.A - 1])
    assert (np.abs((actions - central) / delta) >= 1).any(), "the clip at f32(1 - 1e-7) is exercised"
    idx = rng.integers(0, n_rows, (steps, c.batch)).astype(np.int32)       # with replacement
    idx[0, 0], idx[1 % steps, -1] = 0, n_rows - 1
    if c.batch > 1:
        idx[:, 1] = idx[:, 0]                                              # a duplicate inside every batch
        idx[steps - 1, -1] = n_rows - 1
    params = br.linear_params([(D, 512), (512, 256), (256, 2 * c.A)], c.seed)
    eps = np.clip(rng.standard_normal((n_rows, c.A)), -2.0, 2.0).astype(np.float32)
    return dict(params=params, states=states, next_states=next_states, actions=actions, central=central, delta=delta,
                min_a=min_a, max_a=max_a, idx=idx, table=table, targets=br.targets_of(actions, central, delta), eps=eps,
                batch=c.batch)


def fit_twin(c, k, steps=STEPS, dtype=torch.float64):
    """bc_restate.restate on the materialised table: `steps` fits of GaussianInvActionModel.fit."""
    bc = br.BCCase(c.d1 + c.d2, c.A, c.batch, len(k["table"]), steps, c.standardizer, False, c.seed, 1e-3)
    kk = dict(k, states=k["table"], idx=k["idx"][:steps])
    return bc, br.restate(bc, dtype, case=kk)


def draw_twin(c, k, rows, colstats=None, eps=True, clip=None, lo=br.LOG_STD_MIN, hi=br.LOG_STD_MAX):
    """draw_action (action_models.py:330-372) in float64 on table rows `rows`: the Standardizer takes the rows first
    (colstats [3, D] before the call, None: no Standardizer).  Returns dict(action, mu, log_sigma, colstats);
    clip (lo, hi): np.clip against float64 bounds (lsiqfo.py:90)."""
    x = k["table"][np.asarray(rows, np.int64)]
    stand = br.Standardizer(c.d1 + c.d2, colstats) if colstats is not None else None
    z = torch.as_tensor(stand(x) if stand is not None else x).double()
    w = [torch.as_tensor(p).double() for p in k["params"]]
    y = torch.relu(torch.relu(z @ w[0].T + w[1]) @ w[2].T + w[3]) @ w[4].T + w[5]
    mu, ls = y[:, :c.A], torch.clamp(y[:, c.A:], lo, hi)
    raw = mu + ls.exp() * torch.as_tensor(k["eps"][:len(x)]).double() if eps else mu
    action = (torch.tanh(raw) * torch.as_tensor(k["delta"]).double() + torch.as_tensor(k["central"]).double()).numpy()
    if clip is not None:
        action = np.clip(action, clip[0], clip[1])
    return dict(action=action, mu=mu.numpy(), log_sigma=ls.numpy(), colstats=None if stand is None else stand.colstats)


# ---------------------------------------------------------------------------------------------------------------
# The action model through the calls of four iterations of IQfO_SAC.fit, every one logging (iqfo_sac.py:59-120,
# 174-264): the twin of tests/golden/gen_iam_fit.py's reference run.  SEQ_* is the fixtures' setting.
SEQ_IN, SEQ_A, SEQ_B, SEQ_AMB, SEQ_FITS, SEQ_ITERS, SEQ_LR = 6, 5, 9, 7, 2, 4, 1e-3
SEQ_LO, SEQ_HI = -5.0, 2.0                         # GaussianInvActionModel's log_std_min / log_std_max defaults
SEQ_SCALARS = ("loss_fit0", "loss_fit1", "mse_plcy", "mse_exp", "ent_plcy", "ent_exp", "std_exp", "std", "mu_exp", "mu")


class ModelTwin:
    """The action model of the sequence: train(it) is train_action_model on a logging iteration (the fits, then the six
    passes; returns SEQ_SCALARS' row), draw(it) the expert draw of fit.  wrong: None, "draw" (the expert draw does not
    feed the Standardizer) or "logging" (the logging passes do not)."""

    def __init__(self, fx, params, dtype=torch.float64, wrong=None, clip=False):
        A, D = SEQ_A, 2 * SEQ_IN
        self.fx, self.dtype, self.wrong, self.clip = fx, dtype, wrong, clip
        with torch.random.fork_rng(devices=[]):
            self.lins = [torch.nn.Linear(i, o) for i, o in ((D, 512), (512, 256), (256, 2 * A))]
        self.ps = [p for lin in self.lins for p in (lin.weight, lin.bias)]
        with torch.no_grad():
            for p, v in zip(self.ps, params):
                p.data = torch.as_tensor(np.asarray(v)).to(dtype).clone()
        self.opt = torch.optim.Adam(self.ps, lr=SEQ_LR)
        self.loss_fn = torch.nn.GaussianNLLLoss()
        self.stand = br.Standardizer(D)
        self.cen, self.dl = torch.as_tensor(fx["central"]).to(dtype), torch.as_tensor(fx["delta"]).to(dtype)
        self.t = {k: np.asarray(fx[k]) for k in ("ring_s", "ring_ns", "ring_a", "demo_s", "demo_ns", "demo_a")}

    def forward(self, s, ns, feed=True):
        D, stand, lins = 2 * SEQ_IN, self.stand, self.lins
        x = np.concatenate([s, ns], axis=1).astype(np.float32)
        if feed:
            z = stand(x)
        else:       # the wrong readings: standardised with the sums as they are, the rows not taken in
            cnt = stand.colstats[0] + 1e-2
            mean = stand.colstats[1] / cnt
            std = np.sqrt(np.maximum((stand.colstats[2] + 1e-2) / cnt - np.square(mean), 1e-2))
            z = ((x.astype(np.float64) - mean) / std).astype(np.float32)
        y = lins[2](torch.relu(lins[1](torch.relu(lins[0](torch.as_tensor(z).to(self.dtype))))))
        return y[:, :SEQ_A], torch.clamp(y[:, SEQ_A:], SEQ_LO, SEQ_HI)

    def sample(self, s, ns, eps, feed=True):
        with torch.no_grad():
            mu, ls = self.forward(s, ns, feed)
            return (torch.tanh(mu + ls.exp() * torch.as_tensor(eps).to(self.dtype)) * self.dl + self.cen).double().numpy()

    def train(self, it):
        fx, t, row = self.fx, self.t, []
        S, NS, ACT, DS, DNS, DA = (t[k] for k in ("ring_s", "ring_ns", "ring_a", "demo_s", "demo_ns", "demo_a"))
        for f in range(SEQ_FITS):
            i = fx["fit_idx"][it, f]
            target = torch.as_tensor(br.targets_of(ACT[i], fx["central"], fx["delta"])).to(self.dtype)
            mu, ls = self.forward(S[i], NS[i])
            loss = self.loss_fn(input=mu, target=target, var=torch.square(ls.exp()))
            self.opt.zero_grad()
            loss.backward()
            self.opt.step()
            row.append(float(loss.detach().double()))
        half = 0.5 + 0.5 * np.log(2 * np.pi)
        ip, ie, feed = fx["ip"][it], fx["ie"][it], self.wrong != "logging"
        row.append(float(np.mean((self.sample(S[ip], NS[ip], fx["eps_plcy"][it], feed) - ACT[ip]) ** 2)))
        row.append(float(np.mean((self.sample(DS[ie], DNS[ie], fx["eps_exp"][it], feed) - DA[ie]) ** 2)))
        with torch.no_grad():
            row.append(half + float(self.forward(S[ip], NS[ip], feed)[1].double().mean()))
            row.append(half + float(self.forward(DS[ie], DNS[ie], feed)[1].double().mean()))
            last = fx["fit_idx"][it, -1]
            mu, ls = self.forward(S[last], NS[last], feed)
            mu_e, ls_e = self.forward(DS[ie], DNS[ie], feed)
            row += [float(ls_e.exp().double().mean()), float(ls.exp().double().mean()), float(mu_e.double().mean()),
                    float(mu.double().mean())]
        return row

    def draw(self, it):
        i9 = self.fx["ie_draw"][it]
        a = self.sample(self.t["demo_s"][i9], self.t["demo_ns"][i9], self.fx["eps_draw"][it], self.wrong != "draw")
        return np.clip(a, self.fx["min_a"], self.fx["max_a"]) if self.clip else a

    def params(self):
        return [p.detach().double().numpy().copy() for p in self.ps]


def sequence_twin(fx, params, dtype=torch.float64, wrong=None, clip=False):
    """fx: the fixture's inputs (ring_s, ring_ns, ring_a, demo_s, demo_ns, demo_a, central, delta, min_a, max_a, the
    index arrays fit_idx [it, fits, amb], ip / ie [it, amb], ie_draw [it, B] and the noise eps_plcy / eps_exp [it, amb, A],
    eps_draw [it, B, A]); params: the model's six initial tensors.  The model alone (its calls do not depend on the
    agent's updates).  Returns dict(params [it][6], colstats [it, 3, 12], scalars [it, 10], drawn [it, B, A])."""
    m = ModelTwin(fx, params, dtype, wrong, clip)
    snaps, stats, scal, drawn = [], [], [], []
    for it in range(SEQ_ITERS):
        scal.append(m.train(it))
        drawn.append(m.draw(it))
        snaps.append(m.params())
        stats.append(m.stand.colstats.copy())
    return dict(params=snaps, colstats=np.stack(stats), scalars=np.asarray(scal), drawn=np.stack(drawn))


# The agent's hyperparameters in the fixtures (IQ_SAC's / LSIQ's own defaults where they have one)
FO = dict(gamma=0.99, init_alpha=1e-3, reg_mult=0.5, lr=3e-4, tau=0.005, lr_actor=3e-4, ls_min=-20.0, ls_max=2.0,
          Q_min=-1.0, Q_max=1.0)


def fo_fit_twin(fx, algo, p_model, p_policy, p_critic, dtype=torch.float64, wrong=None):
    """Four logging iterations of IQfO_SAC.fit (algo "iqfo") or LSIQfO.fit ("lsiqfo", with its clip) in float64:
    ModelTwin's train_action_model and expert draw, the batch of iqfo_sac.py:107-112 (the policy rows ip_fit of the ring,
    the demonstration rows ie_draw with the drawn actions narrowed to float32), then iq_pi_restate's whole-agent twin's
    iq_update (LSIQ: with lsiq_restate's critic, as tests/test_gpu_lsiq_q.py composes it) on the recorded noise.
    Returns dict(model, policy, critic: state dicts of the twins; am_scalars [it, 10]; actor_scalars: {iteration: row})."""
    import iq_pi_restate as P
    import iq_restate as Q
    m = ModelTwin(fx, p_model, dtype, wrong, clip=algo == "lsiqfo")
    pcfg = P.PiCfg(standardizer=True, lr=FO["lr_actor"], init_alpha=FO["init_alpha"], ls_min=FO["ls_min"], ls_max=FO["ls_max"])
    central, delta = np.asarray(fx["central"]), np.asarray(fx["delta"])
    if algo == "iqfo":
        qcfg = Q.Cfg(algo="iq", mode="value", reg="exp_and_plcy", treat=False, use_target=True, standardizer=True,
                     gamma=FO["gamma"], reg_mult=FO["reg_mult"], R_min=0.0, R_max=1.0, lr=FO["lr"], tau=FO["tau"])
        t = P.Twin(p_policy, p_critic, central, delta, pcfg, qcfg=qcfg, dtype=dtype)
    else:
        import lsiq_restate as L
        lcfg = L.LCfg(type="iq_like", exp_mode="fix", exp_loss="MSE", clip=True, q_min=FO["Q_min"], q_max=FO["Q_max"],
                      mode="value", reg="exp_and_plcy", treat=False, use_target=True, standardizer=True, gamma=FO["gamma"],
                      reg_mult=FO["reg_mult"], lr=FO["lr"], tau=FO["tau"])
        t = P.Twin(p_policy, p_critic, central, delta, pcfg, dtype=dtype)
        t.q = L.LSIQSoftQ(p_critic, lcfg, dtype)

        def iq_update(s, n_policy, eps, tw=t):      # iq_like: IQ's order of the policy passes, LSIQ's critic update
            c = tw.q.cfg = tw.q.cfg._replace(alpha=float(tw.alpha))
            f = lambda x: x.detach().to(torch.float32).numpy()
            with torch.no_grad():
                a_next, lp_next = (f(x) for x in tw.pi.act(s["next_obs"], eps["next"]))
                tw.pi.act(s["obs"][n_policy:], eps["expert"])
                a_pi, lp_pi = (f(x) for x in tw.pi.act(s["obs"], eps["pi"]))
            tw.q.update(s["obs"], s["act"], s["next_obs"], s["absorbing"], a_next, lp_next, a_pi, lp_pi, n_policy)
            tw.update_policy(s["obs"], n_policy, dict(pi=eps["ppi"], log=eps["plog"]), True)
            tw.iter += 1
            tw.pi.iter += 1
        t.iq_update = iq_update
    scal = []
    f32 = np.float32
    for it in range(SEQ_ITERS):
        scal.append(m.train(it))
        demo_act = m.draw(it).astype(f32)
        ip, ie = fx["ip_fit"][it], fx["ie_draw"][it]
        batch = dict(obs=np.concatenate([fx["ring_s"][ip], fx["demo_s"][ie]]).astype(f32),
                     act=np.concatenate([fx["ring_a"][ip], demo_act]).astype(f32),
                     next_obs=np.concatenate([fx["ring_ns"][ip], fx["demo_ns"][ie]]).astype(f32),
                     absorbing=np.concatenate([fx["ring_abs"][ip], fx["demo_abs"][ie]]).astype(f32))
        t.iq_update(batch, SEQ_B, {k: fx["eps_" + k][it] for k in ("next", "expert", "pi", "ppi", "plog")})
    st = t.state()
    return dict(model=dict(params=m.params(), colstats=m.stand.colstats.copy()), policy=st["policy"], critic=st["critic"],
                am_scalars=np.asarray(scal), actor_scalars=t.scalars)
