"""The critic side of the SAC-family imitation agents on the device: IQ-Learn (imitation_lib/imitation/iq_sac.py),
SQIL (imitation_lib/imitation/sqil_sac.py) and LSIQ (imitation_lib/imitation/lsiq.py).

  Regressor(FullyConnectedNetwork((obs | act) -> [512, 256] -> 1)) x 2, _init_target, the critic's optimiser
                                                         -> DeviceSoftQCritic (parameters, target, Adam moments, packed
                                                            streams and the two Standardizers' sums, all on the device)
  mushroom-rl's ReplayMemory (iq_sac.py:286)             -> DeviceReplayMemory, RESTATED from its published definition
                                                            (mushroom-rl is not installed): a ring that add() fills in
                                                            order and get() samples uniformly with replacement
  IQ_SAC.update_Q_function, _lossQ, getV, get_targetV, regularizer_loss, update_Q_parameters, logging_loss,
  _update_all_targets (:421-429, 467-595, 621-647, 674-676)
                                                         -> DeviceIQLearn.update_Q_function: the policy passes are
                                                            oly_sg_act calls (K25) in the reference's order, the rest is
                                                            ONE oly_iq_q_update call (K26)
  IQ_SAC.fit (:373-406), iq_update's critic part (:408-419)  -> DeviceIQLearn.fit_Q
  SQIL._lossQ (sqil_sac.py:64-136)                       -> DeviceSQIL
  LSIQ._lossQ, _lossQ_iq_like, _lossQ_sqil_like (lsiq.py:9-195)  -> DeviceLSIQ: the same ONE oly_iq_q_update call with
                                                            algo "lsiq" and the block of LSIQ's own keywords; the
                                                            policy passes in the order of the loss type; DeviceLSIQSAC
                                                            adds DeviceIQSAC's policy side unchanged
  LSIQ_H / LSIQ_HC's critic side: getV / get_targetV without the entropy, update_H_function, _update_all_targets
  (lsiq_h.py:35-102, 110-126; lsiq_hc.py:23-100)         -> DeviceLSIQH / DeviceLSIQHC: DeviceLSIQ's call with alpha 0, then
                                                            the H update's own policy pass (K25), for LSIQ_HC the two
                                                            target-critic passes (oly_col_stats + K16), and ONE
                                                            oly_iq_q_update call with algo "lsiq_h" on the second critic

  IQ_SAC.update_policy, _actor_loss, _update_alpha (:431-465, 587-595), iq_update (:408-419) and fit (:373-406) whole;
  SQIL.iq_update (sqil_sac.py:16-62)                     -> DeviceIQSAC / DeviceSQILSAC: update_policy is ONE
                                                            oly_iq_pi_update call (K27), its logging passes are K25's
                                                            and K16's calls in the reference's order, _update_alpha is
                                                            one oly_iq_alpha_update call

DeviceIQLearn and DeviceSQIL are the critic side alone and refuse learnable_alpha (the policy never moves there);
DeviceIQSAC and DeviceSQILSAC are the whole agents; DeviceLSIQ and DeviceLSIQSAC are the same pair for LSIQ; DeviceLSIQH
and DeviceLSIQHC are the critic sides of LSIQ_H and LSIQ_HC, DeviceLSIQHSAC and DeviceLSIQHCSAC the whole agents, whose
actor loss takes the sum of the two critics (K27 with its second critic).  Not built, each refused by the constructors: the gradient penalty
(gradient_penalty_lambda > 0), plcy_loss_mode "v0" and gradient clipping of the actor.  v0 runs in olympic_hip.iq_offline
(DeviceLSIQOffline) and through Engine.iq_q_update(..., v0=); these classes keep refusing it.

The cost of a learnable temperature: K25, K26 and K27 take alpha by value, so with learnable_alpha the `alpha` property
reads log_alpha back from its device block, four bytes, once per iteration.  The default path has no read-back.

Stated differences from the reference: the minibatches are drawn from torch's device generator (the replay memory's
indices with replacement, the demonstrations' as the first entries of a fresh permutation): the same distributions,
another sequence than numpy's.  Of logging_loss's scalars the per-action-dimension means, variances, mins and maxes
("All Actions ...") are left out.  SQIL's iq_update logs its loss as "IQ-Loss/LossQ".
"""
import numpy as np
import torch

from . import _abi
from ._ffi import OlyError
from .bc import DeviceSquashedGaussianPolicy
from .gail import DeviceStandardizer, _same

_H1, _H2 = 512, 256
FOLLOW_UP = "the policy side of the SAC family (update_policy, _update_alpha) is the follow-up to the critic update"
DEMO_KEYS = ("states", "actions", "next_states", "absorbing")


class DeviceSoftQCritic:
    """The soft-Q critic and its target.  net: the reference's FullyConnectedNetwork (its `_linears`) or a list of its
    three nn.Linear layers, (in + A) <= 64 -> 512 -> 256 -> 1.  standardizer: a DeviceStandardizer over all in + A columns
    or None; with one the target gets its own (the reference deep-copies critic_params, iq_sac.py:291), starting from
    the same sums.  The target's weights start as a copy of the live ones (_init_target).  The optimiser is
    torch.optim.Adam(lr, betas, eps, weight_decay) (amsgrad off); tau is the soft target update's rate."""

    def __init__(self, engine, net, standardizer=None, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, tau=0.005):
        lins = list(getattr(net, "_linears", net))
        if len(lins) != 3:
            raise OlyError(f"DeviceSoftQCritic: expected three Linear layers, got {len(lins)}")
        self.eng, self.net, self.lins, self.stand = engine, net, lins, standardizer
        self.D = int(lins[0].in_features)
        if (int(lins[0].out_features), int(lins[1].in_features), int(lins[1].out_features), int(lins[2].in_features),
                int(lins[2].out_features)) != (_H1, _H1, _H2, _H2, 1) or not 2 <= self.D <= 64:
            raise OlyError("DeviceSoftQCritic: supported shape is (in + A) <= 64 -> 512 -> 256 -> 1")
        if standardizer is not None and int(standardizer.dim) != self.D:
            raise OlyError(f"DeviceSoftQCritic: the standardizer has {standardizer.dim} columns, the network {self.D} "
                           "(the critic standardises the whole row, actions included)")
        if not 0.0 <= float(tau) <= 1.0:
            raise OlyError(f"DeviceSoftQCritic: tau={tau} outside [0, 1]")
        self.lr, self.betas = float(lr), (float(betas[0]), float(betas[1]))
        self.eps, self.weight_decay, self.tau = float(eps), float(weight_decay), float(tau)
        dev = engine.device
        with torch.no_grad():
            self.param = torch.cat([t.detach().reshape(-1).to(device=dev, dtype=torch.float32)
                                    for lin in lins for t in (lin.weight, lin.bias)]).contiguous()
        self.target_param = self.param.clone()
        self.exp_avg = torch.zeros_like(self.param)
        self.exp_avg_sq = torch.zeros_like(self.param)
        self.step = 0
        self.target_stand = None
        if standardizer is not None:
            self.target_stand = DeviceStandardizer(engine, self.D)
            self.target_stand.colstats.copy_(standardizer.colstats)
            self.target_stand._fresh = standardizer._fresh
        self.packed = engine.ilmlp_pack(*self._views(self.param))
        self.target_packed = engine.ilmlp_pack(*self._views(self.target_param))

    def _views(self, flat):
        shapes = [(_H1, self.D), (_H1,), (_H2, _H1), (_H2,), (1, _H2), (1,)]
        out, o = [], 0
        for s in shapes:
            n = int(np.prod(s))
            out.append(flat[o:o + n].view(s))
            o += n
        return out

    @property
    def n_par(self):
        return int(self.param.numel())

    def repack(self):
        """Re-pack both streams after the parameters were written (load_state_dict does this)."""
        self.eng.ilmlp_pack(*self._views(self.param), packed=self.packed)
        self.eng.ilmlp_pack(*self._views(self.target_param), packed=self.target_packed)

    @staticmethod
    def _colstats(st):
        if st is None:
            return None
        if getattr(st, "_fresh", False):     # the running sums start from zero; an update adds to them in place
            st.colstats.zero_()
        return st.colstats

    def _rows(self, obs, act):
        x = torch.cat([obs.reshape(len(obs), -1), act.reshape(len(act), -1)], dim=1).to(torch.float32).contiguous()
        if int(x.shape[1]) != self.D:
            raise OlyError(f"DeviceSoftQCritic: obs | act has {x.shape[1]} columns, the network {self.D}")
        return x

    @torch.no_grad()
    def predict(self, obs, act):
        """Q(obs | act) [n, 1] with the current statistics, without updating them (K16's forward)."""
        return self.eng.ilmlp_forward(self._rows(obs, act), self.packed, 1, "identity", colstats=self._colstats(self.stand))

    @torch.no_grad()
    def predict_target(self, obs, act, update_stats=False):
        """Q_target(obs | act) [n, 1].  update_stats: the target's Standardizer takes the rows first, as the network's
        forward does in the reference (oly_col_stats, then K16's forward with the statistics that hold them)."""
        x, cs = self._rows(obs, act), self._colstats(self.target_stand)
        if update_stats and cs is not None:
            self.eng.col_stats(x, cs)
            self.target_stand._fresh = False
        return self.eng.ilmlp_forward(x, self.target_packed, 1, "identity", colstats=cs)

    @torch.no_grad()
    def soft_update_target(self):
        """_update_target outside K26's call (a caller that passed update_target=False because something still had to
        read the old target): K26's expression f32(tau) * w + f32(1 - tau) * t, two float32 products and one add, in
        place, and the target's stream packed again; the bits are those of the in-call update."""
        tau, omt = float(np.float32(self.tau)), float(np.float32(1.0 - self.tau))
        self.target_param.copy_(self.param * tau + self.target_param * omt)
        self.eng.ilmlp_pack(*self._views(self.target_param), packed=self.target_packed)

    @torch.no_grad()
    def sync_to_torch(self):
        """Write the live parameters back into the wrapped Linear layers (torch-side evaluation)."""
        v = self._views(self.param)
        for i, lin in enumerate(self.lins):
            lin.weight.copy_(v[2 * i].to(lin.weight.device))
            lin.bias.copy_(v[2 * i + 1].to(lin.bias.device))
        return self.net

    # ---- checkpoint (il_checkpoint)
    def state_dict(self):
        s, t = self.stand, self.target_stand
        return dict(D=self.D, param=self.param.clone(), target_param=self.target_param.clone(),
                    exp_avg=self.exp_avg.clone(), exp_avg_sq=self.exp_avg_sq.clone(), step=int(self.step),
                    standardizer=None if s is None else s.state_dict(),
                    target_standardizer=None if t is None else t.state_dict())

    @torch.no_grad()
    def load_state_dict(self, d):
        """In place (every device buffer keeps its pointer), then repack()."""
        who = "DeviceSoftQCritic"
        _same(who, "D", int(d["D"]), self.D)
        _same(who, "standardizer", d["standardizer"] is not None, self.stand is not None)
        self.param.copy_(d["param"])
        self.target_param.copy_(d["target_param"])
        self.exp_avg.copy_(d["exp_avg"])
        self.exp_avg_sq.copy_(d["exp_avg_sq"])
        self.step = int(d["step"])
        if self.stand is not None:
            self.stand.load_state_dict(d["standardizer"])
            self.target_stand.load_state_dict(d["target_standardizer"])
        self.repack()


class DeviceReplayMemory:
    """mushroom-rl's ReplayMemory RESTATED from its published definition as a ring of device blocks: add() writes the
    samples in order at the running index, which wraps at max_size (the memory is then full); `initialized` is
    size > initial_size; get(n) draws n indices uniformly from [0, size) with replacement.  The indices come from torch's
    generator on the blocks' device and nothing is read back: the counters are host integers."""

    KEYS = ("states", "actions", "rewards", "next_states", "absorbing", "last")

    def __init__(self, engine, initial_size, max_size, in_dim, act_dim):
        if int(max_size) < 1 or int(initial_size) < 0:
            raise OlyError("DeviceReplayMemory: max_size >= 1 and initial_size >= 0 are required")
        self.eng, self.initial_size, self.max_size = engine, int(initial_size), int(max_size)
        self.in_dim, self.act_dim = int(in_dim), int(act_dim)
        z = lambda *s: torch.zeros((self.max_size,) + s, dtype=torch.float32, device=engine.device)
        self.blocks = dict(states=z(self.in_dim), actions=z(self.act_dim), rewards=z(), next_states=z(self.in_dim),
                           absorbing=z(), last=z())
        self._idx, self._full = 0, False

    @property
    def initialized(self):
        return self.size > self.initial_size

    @property
    def size(self):
        return self.max_size if self._full else self._idx

    @torch.no_grad()
    def add(self, dataset):
        """dataset: a dict of blocks of n samples in order: states [n,in], actions [n,A], next_states [n,in], absorbing
        [n]; rewards and last [n] optional (zeros)."""
        dev = self.eng.device
        n = int(torch.as_tensor(dataset["states"]).shape[0])
        if n == 0:
            return
        first = max(0, n - self.max_size)              # older samples of a longer dataset would be overwritten anyway
        pos = (self._idx + torch.arange(first, n, device=dev)) % self.max_size
        for k, blk in self.blocks.items():
            if k not in dataset:
                if k in ("rewards", "last"):
                    blk[pos] = 0.0
                    continue
                raise OlyError(f"DeviceReplayMemory.add: the dataset has no {k!r}")
            t = torch.as_tensor(dataset[k]).to(device=dev, dtype=torch.float32).reshape((n,) + tuple(blk.shape[1:]))
            blk[pos] = t[first:]
        if self._idx + n >= self.max_size:
            self._full = True
        self._idx = (self._idx + n) % self.max_size

    @torch.no_grad()
    def get(self, n_samples, generator=None):
        """(states, actions, rewards, next_states, absorbing, last) of n_samples uniformly drawn samples."""
        if self.size < 1:
            raise OlyError("DeviceReplayMemory.get: the memory is empty")
        idx = torch.randint(self.size, (int(n_samples),), device=self.eng.device, generator=generator)
        return tuple(self.blocks[k][idx] for k in self.KEYS)

    @torch.no_grad()
    def sample_idx(self, n_samples, generator=None):
        """The indices get(n_samples) would draw from the generator's state, [n_samples] int32 rows of the blocks, for
        the callers that hand the ring and an index to a kernel (olympic_hip.iqfo) and gather nothing."""
        if self.size < 1:
            raise OlyError("DeviceReplayMemory.sample_idx: the memory is empty")
        idx = torch.randint(self.size, (int(n_samples),), device=self.eng.device, generator=generator)
        return idx.to(torch.int32)

    def reset(self):
        self._idx, self._full = 0, False

    def state_dict(self):
        return dict(idx=int(self._idx), full=bool(self._full), max_size=self.max_size,
                    blocks={k: v.clone() for k, v in self.blocks.items()})

    @torch.no_grad()
    def load_state_dict(self, d):
        _same("DeviceReplayMemory", "max_size", int(d["max_size"]), self.max_size)
        for k, v in self.blocks.items():
            v.copy_(d["blocks"][k])
        self._idx, self._full = int(d["idx"]), bool(d["full"])


class DeviceIQLearn:
    """IQ_SAC's critic side (iq_sac.py:256-420, 467-595, 621-647, 674-676) with its hot path on the device.

    policy: a DeviceSquashedGaussianPolicy (it is not trained here); critic: a DeviceSoftQCritic over in + A columns;
    demonstrations: a dict with `states` [n, >= in], `actions` [n,A], `next_states`, `absorbing` [n] (state_mask picks the
    states' columns).  sw: an object with add_scalar(name, value, iteration), or None.  _iter starts at 1 as in the
    reference; an update logs when _iter % logging_iter == 0."""

    ALGO = "iq"
    MODES = tuple(k for k in _abi.IQ_PLCY_LOSS_MODES if k != "v0")

    def __init__(self, engine, policy, critic, demonstrations, gamma, batch_size, use_target, init_alpha=1e-3,
                 reg_mult=0.5, plcy_loss_mode="value", regularizer_mode="exp_and_plcy", treat_absorbing_states=False,
                 delay_Q=1, logging_iter=1, state_mask=None, sw=None, n_fits=1, initial_replay_size=0,
                 max_replay_size=100000, learnable_alpha=False, gradient_penalty_lambda=0.0):
        who = type(self).__name__
        if not isinstance(policy, DeviceSquashedGaussianPolicy):
            raise OlyError(f"{who}: policy must be a DeviceSquashedGaussianPolicy")
        if not isinstance(critic, DeviceSoftQCritic):
            raise OlyError(f"{who}: critic must be a DeviceSoftQCritic")
        if learnable_alpha:
            raise OlyError(f"{who}: learnable_alpha=True is not built: {FOLLOW_UP}")
        if float(gradient_penalty_lambda) > 0.0:
            raise OlyError(f"{who}: gradient_penalty_lambda > 0 is not built (a second-order pass through the critic): "
                           f"{FOLLOW_UP}")
        if plcy_loss_mode == "v0":
            raise OlyError(f"{who}: plcy_loss_mode 'v0' is not built (a fourth critic pass on the expert rows): {FOLLOW_UP}")
        if plcy_loss_mode not in self.MODES:
            raise OlyError(f"{who}: plcy_loss_mode {plcy_loss_mode!r} is not one of {list(self.MODES)}")
        if regularizer_mode not in _abi.IQ_REGULARIZER_MODES:
            raise OlyError(f"{who}: regularizer_mode {regularizer_mode!r} is not one of {list(_abi.IQ_REGULARIZER_MODES)}")
        self.in_dim, self.act_dim = int(policy.in_dim), int(policy.act_dim)
        if self.in_dim + self.act_dim > 64:
            raise OlyError(f"{who}: in_dim + act_dim = {self.in_dim + self.act_dim} > 64 columns of the critic's input")
        if int(critic.D) != self.in_dim + self.act_dim:
            raise OlyError(f"{who}: the critic takes {critic.D} columns, the policy's observation and action give "
                           f"{self.in_dim} + {self.act_dim}")
        for k in DEMO_KEYS:
            if k not in demonstrations:
                raise OlyError(f"{who}: demonstrations have no {k!r}")
        if int(batch_size) < 1 or 2 * int(batch_size) > _abi.OLY_BC_MAX_BATCH or int(logging_iter) < 1 or int(delay_Q) < 1:
            raise OlyError(f"{who}: 1 <= batch_size <= {_abi.OLY_BC_MAX_BATCH // 2}, logging_iter >= 1 and delay_Q >= 1 "
                           "are required")
        self.eng, self.policy, self.critic, self.sw = engine, policy, critic, sw
        dev = engine.device
        mask = None if state_mask is None else torch.as_tensor(np.asarray(state_mask, np.int64), device=dev)

        def up(a, width, name, masked=False):
            t = torch.as_tensor(a).to(device=dev, dtype=torch.float32)
            if masked and mask is not None and t.dim() == 2:
                t = t[:, mask]
            if width is None:
                t = t.reshape(-1)
            elif t.dim() != 2 or int(t.shape[1]) != width:
                raise OlyError(f"{who}: demonstrations[{name!r}] has shape {tuple(t.shape)}, expected [n, {width}]")
            return t.contiguous()
        self.demo = dict(states=up(demonstrations["states"], self.in_dim, "states", True),
                         actions=up(demonstrations["actions"], self.act_dim, "actions"),
                         next_states=up(demonstrations["next_states"], self.in_dim, "next_states", True),
                         absorbing=up(demonstrations["absorbing"], None, "absorbing"))
        self.n_demo = int(self.demo["states"].shape[0])
        if self.n_demo < 1 or any(int(v.shape[0]) != self.n_demo for v in self.demo.values()):
            raise OlyError(f"{who}: the demonstrations' blocks have {[int(v.shape[0]) for v in self.demo.values()]} rows")
        self.gamma, self.batch_size, self.use_target = float(gamma), int(batch_size), bool(use_target)
        # torch.tensor(np.log(init_alpha), dtype=float32).exp(): alpha in float32 (iq_sac.py:328, 686-687)
        self.log_alpha = float(np.float32(np.log(init_alpha)))
        self.reg_mult = float(reg_mult)
        self.plcy_loss_mode, self.regularizer_mode = plcy_loss_mode, regularizer_mode
        self.treat_absorbing_states = bool(treat_absorbing_states)
        self.delay_Q, self.logging_iter, self.n_fits = int(delay_Q), int(logging_iter), int(n_fits)
        self.R_min, self.R_max = 0.0, 1.0
        self.replay = DeviceReplayMemory(engine, initial_replay_size, max_replay_size, self.in_dim, self.act_dim)
        self._iter = 1
        self._ws = {}

    @property
    def alpha(self):
        return float(torch.tensor(self.log_alpha, dtype=torch.float32).exp())

    def _has_v(self):
        return True

    def _logs_before_value(self):
        """Whether logging_loss (and its draw_action on the expert rows) runs before the pass on obs: IQ's order; SQIL
        logs after its loss is formed (sqil_sac.py:94-113)."""
        return self.ALGO == "iq"

    def _value_rows(self, obs, n_policy):
        """The rows getV(.) takes in the loss."""
        return obs

    def _algo_block(self):
        """What the algorithm adds to iq_q_update's keywords."""
        return {}

    def _q_alpha(self):
        """The temperature in the critic's values V = Q - alpha log pi."""
        return self.alpha

    def _q_update_target(self):
        """Whether the critic's call also makes its soft target update."""
        return True

    def _workspace(self, B):
        if B not in self._ws:
            self._ws[B] = self.eng.iq_q_ws(B, self.in_dim, self.act_dim)
        return self._ws[B]

    def _policy_pass(self, x, eps, generator, want_log_prob=True):
        p = self.policy
        x = p._rows(x)
        o = p._fused(x, p._noise(int(x.shape[0]), eps, generator), ("log_prob",) if want_log_prob else ())
        return o["action"], o["log_prob"]

    @torch.no_grad()
    def update_Q_function(self, obs, act, next_obs, absorbing, n_policy, eps=None, generator=None):
        """update_Q_function and _update_all_targets on a batch whose rows [0, n_policy) are the policy's and the rest the
        expert's.  The policy passes are issued in the reference's order: next_obs; on a logging iteration draw_action
        on the expert rows (logging_loss, :646: it feeds the policy's Standardizer and draws noise); obs.  eps: None
        (the noise is drawn from `generator` pass by pass) or a dict with `next` [B,A], `pi` [B,A] and, on a logging
        iteration, `expert` [B - n_policy, A].  Returns the [16] f64 device block of _abi.IQ_Q_TAGS; on a logging
        iteration the scalars also go to sw (which reads them back)."""
        batch = obs, act, next_obs, absorbing = self._batch(obs, act, next_obs, absorbing)
        n_policy, eps = int(n_policy), eps or {}
        logging = self._iter % self.logging_iter == 0
        c = self.critic
        a_next, lp_next = self._policy_pass(next_obs, eps.get("next"), generator)
        a_pi = lp_pi = a_exp = None

        def expert_pass():
            return self._policy_pass(obs[n_policy:], eps.get("expert"), generator, want_log_prob=False)[0]
        before = self._logs_before_value()
        if logging and before:
            a_exp = expert_pass()
        if self._has_v():
            a_pi, lp_pi = self._policy_pass(self._value_rows(obs, n_policy), eps.get("pi"), generator)
        if logging and not before:
            a_exp = expert_pass()
        w_norm = torch.linalg.vector_norm(c.param.double()) if logging and self.sw is not None else None
        out = self._net_update(c, batch, a_next, lp_next, a_pi, lp_pi, n_policy, self.use_target, algo=self.ALGO,
                               plcy_loss_mode=self.plcy_loss_mode, regularizer_mode=self.regularizer_mode,
                               treat_absorbing=self.treat_absorbing_states, update_target=self._q_update_target(),
                               alpha=self._q_alpha(), R_min=self.R_min, R_max=self.R_max, tau=c.tau, **self._algo_block())
        if logging and self.sw is not None:
            self._log(out, act, a_exp, n_policy, w_norm)
        return out

    @staticmethod
    def _batch(obs, act, next_obs, absorbing):
        """A batch's four blocks as contiguous float32, absorbing flat."""
        f32 = torch.float32
        return (obs.to(f32).contiguous(), act.to(f32).contiguous(), next_obs.to(f32).contiguous(),
                absorbing.to(f32).reshape(-1).contiguous())

    def _net_update(self, net, batch, a_next, lp_next, a_pi, lp_pi, n_policy, use_target, **kw):
        """One oly_iq_q_update on `net`, a DeviceSoftQCritic: its two Standardizers' sums, parameters, Adam moments, streams,
        target, step count and optimiser are the call's network arguments; kw: the algorithm's.  Afterwards the
        network's bookkeeping: one more step, and the Standardizers that took rows are no longer fresh."""
        out = self.eng.iq_q_update(*batch, a_next, lp_next, a_pi, lp_pi, n_policy, net._colstats(net.stand),
                                   net._colstats(net.target_stand), net.param, net.exp_avg, net.exp_avg_sq, net.packed,
                                   net.target_param, net.target_packed, self._workspace(int(batch[0].shape[0])), net.step,
                                   net.lr, use_target=use_target, gamma=self.gamma, reg_mult=self.reg_mult,
                                   beta1=net.betas[0], beta2=net.betas[1], eps=net.eps, weight_decay=net.weight_decay, **kw)
        net.step += 1
        if net.stand is not None:
            net.stand._fresh = False
            if use_target:
                net.target_stand._fresh = False
        return out

    def _log(self, out, act, a_exp, n_policy, w_norm):
        host, it, sw = out.cpu().numpy(), self._iter, self.sw
        tags = _abi.IQ_Q_TAGS
        if self.ALGO != "sqil":
            for k in (0, 1, 2):
                sw.add_scalar(tags[k], float(host[k]), it)
            sw.add_scalar("IQ-Loss/Alpha", self.alpha, it)
            skip = self._unlogged_slots()
        else:
            sw.add_scalar("IQ-Loss/LossQ", float(host[0]), it)
            sw.add_scalar("Action-Value/R_min", self.R_min, it)
            skip = (3, 13, 14)                      # SQIL logs neither V nor the absorbing states' Q
        for k in range(3, 16):
            if k not in skip:
                sw.add_scalar(tags[k], float(host[k]), it)
        sw.add_scalar("Action-Value/Norm of Q net: ", float(w_norm), it)
        msq = lambda t: float(torch.square(t).mean())
        sw.add_scalar("Actions/mean squared action expert (from data)", msq(act[n_policy:]), it)
        sw.add_scalar("Actions/mean squared action expert (from policy)", msq(a_exp), it)
        sw.add_scalar("Actions/mean squared action policy", msq(act[:n_policy]), it)
        sw.add_scalar("Actions/mean squared action both", msq(act), it)

    def _unlogged_slots(self):
        return ()

    def draw_demo_idx(self, n, generator=None):
        """The first n entries of a fresh permutation of the demonstrations (minibatch_generator's first batch)."""
        n = min(int(n), self.n_demo)
        keys = torch.rand((self.n_demo,), device=self.eng.device, generator=generator)
        return torch.topk(keys, n, largest=False, sorted=True).indices

    @torch.no_grad()
    def _fit(self, dataset, generator, step):
        """IQ_SAC.fit's loop (:373-406): the dataset goes into the replay memory; once that is initialised, n_fits times a
        policy minibatch from it and as many demonstration rows are drawn and step(batch, n_policy) runs, batch() making
        the one batch (obs, act, next_obs, absorbing) of both.  Then _iter and policy.iter advance.  Returns what the
        last step returned that was not None, or None."""
        self.replay.add(dataset)
        out = None
        if self.replay.initialized:
            for _ in range(self.n_fits):
                s, a, _r, ns, ab, _l = self.replay.get(self.batch_size, generator)
                idx = self.draw_demo_idx(int(s.shape[0]), generator)
                d = self.demo
                res = step(lambda: (torch.cat([s, d["states"][idx]]), torch.cat([a, d["actions"][idx]]),
                                    torch.cat([ns, d["next_states"][idx]]), torch.cat([ab, d["absorbing"][idx]])),
                           int(s.shape[0]))
                out = out if res is None else res
        self._iter += 1
        self.policy.iter = getattr(self.policy, "iter", 0) + 1
        return out

    def fit_Q(self, dataset, generator=None):
        """IQ_SAC.fit with iq_update's critic part: update_Q_function on every delay_Q-th iteration's batches.  Returns
        the last update's scalars, or None."""
        def step(batch, n_policy):
            if self._iter % self.delay_Q == 0:
                return self.update_Q_function(*batch(), n_policy, generator=generator)
        return self._fit(dataset, generator, step)

    # ---- checkpoint (il_checkpoint.save / load take this object as the agent)
    KIND = "iq_learn_critic"

    def state_dict(self):
        st = self.policy.stand
        return dict(kind=self.KIND, policy=self.policy.state_dict(), policy_iter=int(getattr(self.policy, "iter", 0)),
                    policy_standardizer=None if st is None else st.state_dict(), critic=self.critic.state_dict(),
                    replay=self.replay.state_dict(), iter=int(self._iter), log_alpha=float(self.log_alpha))

    @torch.no_grad()
    def load_state_dict(self, d):
        """In place (every device buffer keeps its pointer)."""
        who = type(self).__name__
        _same(who, "kind", d.get("kind"), self.KIND)
        st = self.policy.stand
        _same(who, "policy standardizer", d["policy_standardizer"] is not None, st is not None)
        self.policy.load_state_dict(d["policy"])
        self.policy.iter = int(d["policy_iter"])
        if st is not None:
            st.load_state_dict(d["policy_standardizer"])
        self.critic.load_state_dict(d["critic"])
        self.replay.load_state_dict(d["replay"])
        self._iter, self.log_alpha = int(d["iter"]), float(d["log_alpha"])

    def save(self, path, **meta):
        from . import il_checkpoint
        return il_checkpoint.save(path, self, None, **meta)

    def load(self, path):
        from . import il_checkpoint
        return il_checkpoint.load(path, self, None)


class DeviceSQIL(DeviceIQLearn):
    """SQIL (sqil_sac.py): DeviceIQLearn with SQIL's loss, its modes plcy / value / value_plcy and the rewards R_min (policy
    rows) and R_max (expert rows).  plcy, the true SQIL objective, runs no pass on (obs | a_pi)."""

    ALGO = "sqil"
    MODES = tuple(_abi.SQIL_PLCY_LOSS_MODES)
    KIND = "sqil_critic"

    def __init__(self, engine, policy, critic, demonstrations, gamma, batch_size, use_target, R_min=0.0, R_max=1.0,
                 plcy_loss_mode="plcy", **kw):
        super().__init__(engine, policy, critic, demonstrations, gamma, batch_size, use_target,
                         plcy_loss_mode=plcy_loss_mode, **kw)
        self.R_min, self.R_max = float(R_min), float(R_max)

    def _has_v(self):
        return self.plcy_loss_mode != "plcy"


class DeviceLSIQ(DeviceIQLearn):
    """LSIQ (lsiq.py:9-195): DeviceIQLearn with LSIQ's two losses and its clipped target.  The keywords are the
    reference's: Q_max / Q_min bound the target (target_clipping) and Q_max is the constant the expert's Q is fitted to
    with loss_mode_exp "fix" (Q_exp_loss "MSE" or "Huber"; None is refused there, as the reference raises);
    lossQ_type "iq_like" takes IQ's plcy_loss_mode names and value_q_old_policy / off, "sqil_like" takes value, value_plcy
    and q_old_policy and always needs a Q_exp_loss.  sqil_like / value needs as many policy rows as expert rows (the
    reference's r_min vector, lsiq.py:165), which the update checks per batch.  sqil_like logs after its loss is formed
    and runs the pass on obs for value (all rows), value_plcy (the policy's rows alone) or not at all."""

    ALGO = "lsiq"
    KIND = "lsiq_critic"

    def __init__(self, engine, policy, critic, demonstrations, gamma, batch_size, use_target, Q_max=1.0, Q_min=-1.0,
                 loss_mode_exp="fix", Q_exp_loss=None, treat_absorbing_states=False, target_clipping=True,
                 lossQ_type="iq_like", plcy_loss_mode="value", **kw):
        who = type(self).__name__
        if lossQ_type not in _abi.LSIQ_LOSSQ_TYPES:
            raise OlyError(f"{who}: lossQ_type {lossQ_type!r} is not one of {list(_abi.LSIQ_LOSSQ_TYPES)}")
        if loss_mode_exp not in _abi.LSIQ_LOSS_MODES_EXP:
            raise OlyError(f"{who}: loss_mode_exp {loss_mode_exp!r} is not one of {list(_abi.LSIQ_LOSS_MODES_EXP)}")
        if Q_exp_loss not in _abi.LSIQ_Q_EXP_LOSSES:
            raise OlyError(f"{who}: Q_exp_loss {Q_exp_loss!r} is not one of {list(_abi.LSIQ_Q_EXP_LOSSES)}")
        sqil_like = lossQ_type == "sqil_like"
        if Q_exp_loss is None and (sqil_like or loss_mode_exp == "fix"):
            raise OlyError(f"{who}: loss_mode_exp 'fix' and lossQ_type 'sqil_like' need Q_exp_loss 'MSE' or 'Huber'; None is "
                           "not valid there")
        if not float(Q_min) < float(Q_max):
            raise OlyError(f"{who}: Q_min={Q_min} must lie below Q_max={Q_max}")
        self.MODES = tuple(_abi.LSIQ_SQIL_LIKE_MODES) if sqil_like else \
            tuple(k for k in _abi.LSIQ_PLCY_LOSS_MODES if k != "v0")
        super().__init__(engine, policy, critic, demonstrations, gamma, batch_size, use_target,
                         plcy_loss_mode=plcy_loss_mode, treat_absorbing_states=treat_absorbing_states, **kw)
        self.Q_max, self.Q_min = float(Q_max), float(Q_min)
        self.loss_mode_exp, self.Q_exp_loss = loss_mode_exp, Q_exp_loss
        self.target_clipping, self.lossQ_type = bool(target_clipping), lossQ_type

    def _has_v(self):
        return self.lossQ_type == "iq_like" or self.plcy_loss_mode != "q_old_policy"

    def _logs_before_value(self):
        return self.lossQ_type == "iq_like"

    def _value_rows(self, obs, n_policy):
        if self.lossQ_type == "sqil_like" and self.plcy_loss_mode == "value_plcy":
            return obs[:n_policy]                # getV(obs[~is_expert]), lsiq.py:167
        return obs

    def _algo_block(self):
        return dict(lsiq=dict(lossQ_type=self.lossQ_type, loss_mode_exp=self.loss_mode_exp, Q_exp_loss=self.Q_exp_loss,
                              target_clipping=self.target_clipping, Q_min=self.Q_min, Q_max=self.Q_max))

    def _unlogged_slots(self):
        return () if self.lossQ_type == "iq_like" else (3,)       # sqil_like never logs V


class DeviceLSIQH(DeviceLSIQ):
    """LSIQ_H's critic side (lsiq_h.py): LSIQ whose Q target carries no entropy (getV / get_targetV return Q(obs | a_pi):
    DeviceLSIQ's call with alpha 0.0, which is Q - 0 * log_prob = Q bit for bit) and a second critic H that learns the
    entropy by its own TD update, update_H_function, run after the Q critic has stepped.  h_critic (the reference's
    H_params): a second DeviceSoftQCritic over the same in + A columns with its own optimiser and learning rate; its
    `tau` is the agent's.  clip_expert_entropy_to_policy_max, max_H_policy_tau_down and max_H_policy_tau_up are the
    reference's; the running maximum lives in the [2] device block h_max_state (the value, 1.0 once it is set) and is
    never read back.  The H update's scalars (_abi.LSIQ_H_TAGS) are left in h_out and go to sw on a logging iteration."""

    KIND = "lsiq_h_critic"
    H_COST = False

    def __init__(self, engine, policy, critic, demonstrations, gamma, batch_size, use_target, h_critic=None,
                 clip_expert_entropy_to_policy_max=True, max_H_policy_tau_down=1e-4, max_H_policy_tau_up=1e-2, **kw):
        who = type(self).__name__
        if not isinstance(h_critic, DeviceSoftQCritic):
            raise OlyError(f"{who}: h_critic (the reference's H_params) must be a DeviceSoftQCritic")
        if h_critic is critic:
            raise OlyError(f"{who}: h_critic must be a network of its own, not the Q critic")
        for name, t in (("max_H_policy_tau_down", max_H_policy_tau_down), ("max_H_policy_tau_up", max_H_policy_tau_up)):
            if not 0.0 <= float(t) <= 1.0:
                raise OlyError(f"{who}: {name}={t} outside [0, 1]")
        super().__init__(engine, policy, critic, demonstrations, gamma, batch_size, use_target, **kw)
        if int(h_critic.D) != int(critic.D):
            raise OlyError(f"{who}: h_critic takes {h_critic.D} columns, the Q critic {critic.D}")
        self.h_critic = h_critic
        self.clip_expert_entropy_to_policy_max = bool(clip_expert_entropy_to_policy_max)
        self.max_H_policy_tau_down, self.max_H_policy_tau_up = float(max_H_policy_tau_down), float(max_H_policy_tau_up)
        self.h_max_state = torch.zeros(2, dtype=torch.float32, device=engine.device)
        self.h_out = None

    def _q_alpha(self):
        return 0.0

    def _h_loss(self):
        return "MSE"

    def _h_tau(self):
        return self.h_critic.tau

    @torch.no_grad()
    def update_Q_function(self, obs, act, next_obs, absorbing, n_policy, eps=None, generator=None):
        """LSIQ's update_Q_function with the entropy-free values, then update_H_function on the same batch and the target
        updates.  eps: DeviceLSIQ's dict with, in addition, `h_next` [B,A] (the H update's policy pass on next_obs) and,
        for LSIQ_HC, `h_pi` [B,A] (get_targetV's pass on obs).  Returns the Q critic's [16] block; the H update's is
        h_out."""
        out = super().update_Q_function(obs, act, next_obs, absorbing, n_policy, eps=eps, generator=generator)
        self.h_out = self.update_H_function(obs, act, next_obs, absorbing, n_policy, eps=eps, generator=generator)
        return out

    @torch.no_grad()
    def update_H_function(self, obs, act, next_obs, absorbing, n_policy, eps=None, generator=None):
        """update_H_function and the target updates still due, in the reference's order: a NEW
        compute_action_and_log_prob_t(next_obs) (it feeds the policy's Standardizer and draws noise); for LSIQ_HC
        Q_target(obs | act), then get_targetV(obs) = a policy pass on obs and Q_target(obs | a_pi), the target critic's
        Standardizer taking the rows of both; then one oly_iq_q_update with algo "lsiq_h" on h_critic, which also makes
        H's soft target update; for LSIQ_HC last the Q critic's soft target update, deferred to here because the H
        update reads the target from before it."""
        batch = obs, act, next_obs, absorbing = self._batch(obs, act, next_obs, absorbing)
        h, c, eps = self.h_critic, self.critic, eps or {}
        # the H call below shares the Q call's workspace: both run in order on the engine's stream and oly_iq_q_ws does
        # not depend on the algorithm; calls that could overlap would need a workspace each
        a_next, lp_next = self._policy_pass(next_obs, eps.get("h_next"), generator)
        q_t = v_t = None
        if self.H_COST:
            q_t = c.predict_target(obs, act, update_stats=True).reshape(-1)
            a_pi = self._policy_pass(obs, eps.get("h_pi"), generator, want_log_prob=False)[0]
            v_t = c.predict_target(obs, a_pi, update_stats=True).reshape(-1)
        block = dict(self._algo_block()["lsiq"],
                     h=dict(loss=self._h_loss(), cost=self.H_COST, clip_expert=self.clip_expert_entropy_to_policy_max,
                            tau_up=self.max_H_policy_tau_up, tau_down=self.max_H_policy_tau_down,
                            max_state=self.h_max_state if self.clip_expert_entropy_to_policy_max else None, q_t=q_t, v_t=v_t))
        out = self._net_update(h, batch, a_next, lp_next, None, None, int(n_policy), True, algo="lsiq_h", update_target=True,
                               alpha=self.alpha, tau=self._h_tau(), lsiq=block)
        if not self._q_update_target():
            c.soft_update_target()
        if self._iter % self.logging_iter == 0 and self.sw is not None:
            host = out.cpu().numpy()
            for k in range(7):                       # the reference's seven scalars, lsiq_h.py:94-100
                self.sw.add_scalar(_abi.LSIQ_H_TAGS[k], float(host[k]), self._iter)
        return out

    def state_dict(self):
        d = super().state_dict()
        d.update(h_critic=self.h_critic.state_dict(), h_max_state=self.h_max_state.clone())
        return d

    @torch.no_grad()
    def load_state_dict(self, d):
        super().load_state_dict(d)
        self.h_critic.load_state_dict(d["h_critic"])
        self.h_max_state.copy_(d["h_max_state"])


class DeviceLSIQHC(DeviceLSIQH):
    """LSIQ_HC's critic side (lsiq_hc.py): LSIQ_H whose H target adds the squared regularised reward of the target Q
    critic, read BEFORE this iteration's soft update of it (so the Q critic's call runs with update_target=False and
    the update follows the H update), with the MSE or Huber loss (H_loss_mode) and H's own target rate H_tau."""

    KIND = "lsiq_hc_critic"
    H_COST = True

    def __init__(self, engine, policy, critic, demonstrations, gamma, batch_size, use_target, H_tau=None,
                 H_loss_mode="Huber", **kw):
        who = type(self).__name__
        if H_tau is None or not 0.0 <= float(H_tau) <= 1.0:
            raise OlyError(f"{who}: H_tau={H_tau} must be given, in [0, 1]")
        if H_loss_mode not in _abi.LSIQ_H_LOSSES:
            raise OlyError(f"{who}: Unsupported H_loss {H_loss_mode!r} (one of {list(_abi.LSIQ_H_LOSSES)})")
        super().__init__(engine, policy, critic, demonstrations, gamma, batch_size, use_target, **kw)
        if not self.reg_mult > 0.0:
            raise OlyError(f"{who}: reg_mult={self.reg_mult} must be positive (the reward is clipped at 1 / reg_mult)")
        self.H_tau, self.H_loss_mode = float(H_tau), H_loss_mode

    def _q_update_target(self):
        return False

    def _h_loss(self):
        return self.H_loss_mode

    def _h_tau(self):
        return self.H_tau


class _PolicySide:
    """What the whole agents add to their critic-side parents: update_policy, _update_alpha, iq_update, fit.  The
    constructor takes the parent's arguments and actor_optimizer: dict(lr, betas, eps, weight_decay) of torch.optim.Adam
    (a `clipping` entry is refused); warmup_transitions, delay_pi, train_policy_only_on_own_states, learnable_alpha,
    lr_alpha and target_entropy (None: -A) as the reference's; e_thres / e_reduc: the policy's entropy lower bound
    (linear mode), logged only.  The policy's Adam moments and step count and the [3] device block (log_alpha, exp_avg,
    exp_avg_sq) live here."""

    def __init__(self, *args, actor_optimizer=None, warmup_transitions=0, delay_pi=1, train_policy_only_on_own_states=False,
                 learnable_alpha=False, lr_alpha=3e-4, target_entropy=None, init_alpha=1e-3, e_thres=2.0, e_reduc=1e-5,
                 **kw):
        super().__init__(*args, init_alpha=init_alpha, learnable_alpha=False, **kw)
        who = type(self).__name__
        opt = dict(actor_optimizer or {})
        if "clipping" in opt:
            raise OlyError(f"{who}: actor_optimizer['clipping'] is not built (gradient clipping of the actor)")
        unknown = set(opt) - {"lr", "betas", "eps", "weight_decay"}
        if unknown:
            raise OlyError(f"{who}: actor_optimizer has unknown entries {sorted(unknown)}")
        if int(delay_pi) < 1 or int(warmup_transitions) < 0:
            raise OlyError(f"{who}: delay_pi >= 1 and warmup_transitions >= 0 are required")
        betas = opt.get("betas", (0.9, 0.999))
        self.pi_lr, self.pi_betas = float(opt.get("lr", 3e-4)), (float(betas[0]), float(betas[1]))
        self.pi_eps, self.pi_weight_decay = float(opt.get("eps", 1e-8)), float(opt.get("weight_decay", 0.0))
        self.warmup_transitions, self.delay_pi = int(warmup_transitions), int(delay_pi)
        self.train_policy_only_on_own_states = bool(train_policy_only_on_own_states)
        self.learnable_alpha, self.lr_alpha = bool(learnable_alpha), float(lr_alpha)
        self.target_entropy = -float(self.act_dim) if target_entropy is None else float(target_entropy)
        self.e_thres, self.e_reduc = float(e_thres), float(e_reduc)
        dev = self.eng.device
        self.pi_exp_avg = torch.zeros_like(self.policy.param)
        self.pi_exp_avg_sq = torch.zeros_like(self.policy.param)
        self.pi_step = 0
        # log_alpha, exp_avg, exp_avg_sq of Adam([log_alpha], lr_alpha) (iq_sac.py:328-335)
        self.alpha_state = torch.tensor([np.float32(np.log(init_alpha)), 0.0, 0.0], dtype=torch.float32, device=dev)
        self.alpha_step = 0
        self._alpha_read = True          # log_alpha (the host copy) is current
        self._pi_ws, self._pi_h_ws = {}, {}

    @property
    def alpha(self):
        if self.learnable_alpha and not self._alpha_read:      # four bytes, once per iteration that stepped it
            self.log_alpha = float(self.alpha_state[0])
            self._alpha_read = True
        return float(torch.tensor(self.log_alpha, dtype=torch.float32).exp())

    def _pi_workspace(self, B):
        if B not in self._pi_ws:
            self._pi_ws[B] = self.eng.iq_pi_ws(B, self.in_dim, self.act_dim)
        return self._pi_ws[B]

    def _actor_h(self, Bp):
        """The second critic of the actor loss (LSIQ_H / LSIQ_HC: mean(alpha log_prob - (q + H))) as iq_pi_update's `h`,
        with a workspace of its own per batch size; None for the agents with one critic."""
        h = getattr(self, "h_critic", None)
        if h is None:
            return None
        if Bp not in self._pi_h_ws:
            self._pi_h_ws[Bp] = self.eng.iq_pi_ws(Bp, self.in_dim, self.act_dim)
        return dict(packed=h.packed, param=h.param, colstats=h._colstats(h.stand), ws=self._pi_h_ws[Bp])

    def get_e_lb(self):
        """IQ_Learn_Policy.get_e_lb in its linear mode (iq_sac.py:169-171): a host number from policy.iter."""
        return self.e_thres - getattr(self.policy, "iter", 0) * self.e_reduc

    @torch.no_grad()
    def update_policy(self, obs, n_policy, eps=None, generator=None):
        """update_policy (iq_sac.py:431-465) on a batch whose rows [0, n_policy) are the policy's: one oly_iq_pi_update
        on all rows (train_policy_only_on_own_states: on the policy's); on a logging iteration the reference's three
        further passes in its order (compute_action_and_log_prob_t on all rows with the stepped weights, get_mu_log_sigma
        on the policy's rows, then on the expert's: each feeds the policy's Standardizer, the first draws noise); with
        learnable_alpha _update_alpha last, on a logging iteration with the SECOND pass's log-probabilities as the
        reference's rebound name gives it.  eps: None (drawn from `generator` pass by pass) or a dict with `pi` [Bp,A] and,
        on a logging iteration, `log` [B,A].  Returns the [4] f64 device block of _abi.IQ_PI_TAGS."""
        f32 = torch.float32
        obs = obs.to(f32).contiguous()
        B, n_policy = int(obs.shape[0]), int(n_policy)
        eps = eps or {}
        logging = self._iter % self.logging_iter == 0
        c, p = self.critic, self.policy
        x = obs[:n_policy].contiguous() if self.train_policy_only_on_own_states else obs
        Bp = int(x.shape[0])
        noise = p._noise(Bp, eps.get("pi"), generator).contiguous()
        cs, ccs, hk = p._colstats(), c._colstats(c.stand), self._actor_h(Bp)
        o = self.eng.iq_pi_update(x, noise, p.central, p.delta, cs, p.param, self.pi_exp_avg, self.pi_exp_avg_sq, p.packed,
                                  c.packed, c.param, ccs, self._pi_workspace(Bp), self.pi_step, self.pi_lr,
                                  alpha=self.alpha, log_std_min=p.log_std_min, log_std_max=p.log_std_max,
                                  beta1=self.pi_betas[0], beta2=self.pi_betas[1], adam_eps=self.pi_eps,
                                  weight_decay=self.pi_weight_decay, h=hk)
        if hk is not None and hk["colstats"] is not None:
            self.h_critic.stand._fresh = False
        self.pi_step += 1
        if cs is not None:
            p.stand._fresh = False
        if ccs is not None:
            c.stand._fresh = False
        log_prob = o["log_prob"]
        if logging:
            _, log_prob = self._policy_pass(obs, eps.get("log"), generator)
            ls_p = p.get_mu_log_sigma(obs[:n_policy])[1]
            e_lb = self.get_e_lb()
            ls_e = p.get_mu_log_sigma(obs[n_policy:])[1]
            if self.sw is not None:
                host, it, sw = o["out"].cpu().numpy(), self._iter, self.sw
                sw.add_scalar(_abi.IQ_PI_TAGS[1], float(host[1]), it)
                sw.add_scalar(_abi.IQ_PI_TAGS[0], float(host[0]), it)
                sw.add_scalar("Actor/Entropy Expert States", float(torch.mean(-log_prob[n_policy:])), it)
                sw.add_scalar("Actor/Entropy Policy States", float(torch.mean(-log_prob[:n_policy])), it)
                sw.add_scalar("Actor/Entropy from Gaussian Policy States", float(torch.mean(p.entropy_from_logsigma(ls_p))), it)
                sw.add_scalar("Actor/Entropy Lower Bound", float(e_lb), it)
                sw.add_scalar("Actor/Entropy from Gaussian Expert States", float(torch.mean(p.entropy_from_logsigma(ls_e))), it)
        if self.learnable_alpha:
            self.eng.iq_alpha_update(log_prob.contiguous(), self.alpha_state, self.alpha_step, self.lr_alpha,
                                     self.target_entropy)
            self.alpha_step += 1
            self._alpha_read = False
        return o["out"]

    @torch.no_grad()
    def iq_update(self, obs, act, next_obs, absorbing, n_policy, eps=None, generator=None):
        """iq_update (iq_sac.py:408-419; sqil_sac.py:16-62): update_Q_function every delay_Q iterations, update_policy
        once the replay memory holds more than warmup_transitions and every delay_pi iterations.  The target update runs
        inside the critic's call (K26), before the policy update instead of after it: the policy update neither reads
        nor writes the target, so the order does not show.  eps: None or dict(q=update_Q_function's, pi=update_policy's).
        Returns (the critic's scalars or None, the policy's or None)."""
        eps = eps or {}
        out_q = out_pi = None
        if self._iter % self.delay_Q == 0:
            out_q = self.update_Q_function(obs, act, next_obs, absorbing, n_policy, eps=eps.get("q"), generator=generator)
        if self.replay.size > self.warmup_transitions and self._iter % self.delay_pi == 0:
            out_pi = self.update_policy(obs, n_policy, eps=eps.get("pi"), generator=generator)
        return out_q, out_pi

    def fit(self, dataset, generator=None):
        """IQ_SAC.fit (:373-406): DeviceIQLearn._fit's loop around iq_update.  Returns the last iq_update's pair, or None."""
        return self._fit(dataset, generator, lambda batch, n_policy: self.iq_update(*batch(), n_policy, generator=generator))

    def state_dict(self):
        d = super().state_dict()
        d["log_alpha"] = float(self.alpha_state[0]) if self.learnable_alpha else float(self.log_alpha)
        d.update(pi_exp_avg=self.pi_exp_avg.clone(), pi_exp_avg_sq=self.pi_exp_avg_sq.clone(), pi_step=int(self.pi_step),
                 alpha_state=self.alpha_state.clone(), alpha_step=int(self.alpha_step))
        return d

    @torch.no_grad()
    def load_state_dict(self, d):
        """In place (every device buffer keeps its pointer)."""
        super().load_state_dict(d)
        self.pi_exp_avg.copy_(d["pi_exp_avg"])
        self.pi_exp_avg_sq.copy_(d["pi_exp_avg_sq"])
        self.alpha_state.copy_(d["alpha_state"])
        self.pi_step, self.alpha_step = int(d["pi_step"]), int(d["alpha_step"])
        self._alpha_read = True


class DeviceIQSAC(_PolicySide, DeviceIQLearn):
    """IQ_SAC whole (iq_sac.py:256-420, 431-465, 587-595): DeviceIQLearn's critic side with the policy and the
    temperature trained on the device (K27)."""

    KIND = "iq_sac"


class DeviceSQILSAC(_PolicySide, DeviceSQIL):
    """SQIL whole (sqil_sac.py): DeviceSQIL's critic side with DeviceIQSAC's policy side."""

    KIND = "sqil_sac"


class DeviceLSIQSAC(_PolicySide, DeviceLSIQ):
    """LSIQ whole (lsiq.py: an IQ_SAC that overrides _lossQ alone): DeviceLSIQ's critic side with DeviceIQSAC's policy
    side."""

    KIND = "lsiq_sac"


class DeviceLSIQHSAC(_PolicySide, DeviceLSIQH):
    """LSIQ_H whole (lsiq_h.py): DeviceLSIQH's critic side with DeviceIQSAC's policy side, whose actor loss takes the sum
    of the two live critics, mean(alpha log_prob - (Q + H)) (_actor_loss, :104-108): update_policy hands h_critic to
    oly_iq_pi_update, which also feeds H's Standardizer the policy update's rows."""

    KIND = "lsiq_h_sac"


class DeviceLSIQHCSAC(_PolicySide, DeviceLSIQHC):
    """LSIQ_HC whole (lsiq_hc.py): DeviceLSIQHC's critic side with DeviceLSIQHSAC's policy side."""

    KIND = "lsiq_hc_sac"


__all__ = ["DeviceSoftQCritic", "DeviceReplayMemory", "DeviceIQLearn", "DeviceSQIL", "DeviceLSIQ", "DeviceLSIQH",
           "DeviceLSIQHC", "DeviceIQSAC", "DeviceSQILSAC", "DeviceLSIQSAC", "DeviceLSIQHSAC", "DeviceLSIQHCSAC"]
