"""The inverse action model of the reference's learning-from-observations agents (IQfO_SAC, LSIQfO, LSIQfO_H,
LSIQfO_HC: imitation_lib/imitation/iqfo_sac.py, lsiqfo.py, lsiqfo_h.py, lsiqfo_hc.py) on the device.

  GaussianInvActionModel (imitation_lib/utils/action_models.py:322-528): a squashed-Gaussian network on the
  concatenated row (s | s'), IQ_Learn_Policy's shape in -> [512, 256] -> 2A
      fit (:381-401): GaussianNLLLoss + Adam on the un-squashed actions   -> DeviceGaussianInvActionModel.fit: ONE
                                                                             oly_bc_fit_steps call with oly_bc_fit.pair
                                                                             for all fits of an iteration (K24 / K28)
      draw_action / get_mu_log_sigma / entropy (:377-379, :450-503)       -> one oly_sg_act call each with its two-table
                                                                             fields (K25)

The model is fitted every iteration to the agent's own replay transitions and then draws the expert's missing actions.
Its rows come from two tables indexed by a sample drawn with replacement (DeviceReplayMemory.sample_idx: the ring's
states and next_states), its targets from the ring's raw actions, which change every iteration; neither is
materialised: the kernels gather the rows and un-squash the actions themselves.

  IQfO_SAC / LSIQfO / LSIQfO_H / LSIQfO_HC .fit (iqfo_sac.py:59-120) and train_action_model (:133-268)
                                                                          -> the mixin _FromObservations over the
                                                                             agents of olympic_hip.iq: DeviceIQfOSAC,
                                                                             DeviceLSIQfOSAC, DeviceLSIQfOHSAC,
                                                                             DeviceLSIQfOHCSAC

One fit is the reference's in its order: replay.add; if the memory is initialised, train_action_model (fits_per_step
fits on fresh replay samples of the model's batch size, then on a logging iteration its further passes, each feeding
the model's Standardizer as its forward does); one policy minibatch; as many demonstration rows (s, s', absorbing); the
drawn expert actions (LSIQfO alone clips them to the action space, lsiqfo.py:90; lsiqfo_h.py and lsiqfo_hc.py do not);
the optional interpolation; ONE iq_update with n_policy = batch_size (the fO fit has no n_fits loop); _iter and
policy.iter advance.

action_model_fit_params["init_epochs"] is accepted and ignored: the reference's initial-fit branch is unreachable.
_action_model_initialized is True exactly when init_epochs > 0 (iqfo_sac.py:40), so train_action_model(init=True) only
ever runs with init_epochs == 0, where it takes the ordinary branch (:135, :174).  IQfO_ORIG (iqfo_orig.py) never steps
its critic and is not built.

Refused by the constructors: add_noise_to_obs=True and an ext_normalizer_action_model (observation noise through an
external normaliser), every action model but the Gaussian one (KL-Gaussian, GCP, KL-GCP, learnable- and fixed-variance),
interpolate_expert_states together with a state_mask (the reference masks the interpolated block twice there), and
2 * in_dim > 64.

Stated differences from the reference: samples and noise come from torch's device generator; the demonstrations and
the tables are held in float32 (the interpolation is formed in float32); the replay ring holds the policy's in_dim
columns, so the model's rows from it are not masked again.
"""
import numpy as np
import torch

from . import _abi
from ._ffi import OlyError
from .bc import DeviceSquashedGaussianPolicy
from .gail import _same
from .iq import DeviceIQSAC, DeviceLSIQHCSAC, DeviceLSIQHSAC, DeviceLSIQSAC

_HALF_LOG_2PI_E = 0.5 + 0.5 * float(np.log(2 * np.pi))       # Normal.entropy() = 0.5 + 0.5 log 2 pi + log sigma


class DeviceGaussianInvActionModel(DeviceSquashedGaussianPolicy):
    """GaussianInvActionModel with GaussianNLLLoss (eps nll_eps) and torch.optim.Adam(lr, betas, eps, weight_decay).

    It holds its parameters, packed stream and Standardizer as DeviceSquashedGaussianPolicy does (it is one, on rows of
    in = d1 + d2 columns) and its Adam moments and step count as DeviceBehavioralCloning does.  net: the reference's
    FullyConnectedNetwork or its three nn.Linear layers, in <= 64 -> 512 -> 256 -> 2A.  standardizer: ONE
    DeviceStandardizer over the concatenated row or None; every forward feeds it first, as FullyConnectedNetwork.forward
    does (networks.py:144-158): the fits, draw_action, get_mu_log_sigma and entropy.  batch_size: the rows of one fit.

    Every method takes the two tables and an index: s_tbl [n_rows, >= d1] and ns_tbl [n_rows, >= d2] float32 device
    tensors, of which the first d1 / d2 columns are read (default: the tables' widths, which must then add up to in),
    and idx, int32 device rows (None where allowed: row r is table row r).  Nothing is gathered or concatenated on the
    host side and nothing synchronises.  The methods it inherits unchanged (predict, act, compute_action_and_log_prob,
    distribution) keep the policy's contract: one tensor of materialised rows [n, in]."""

    def __init__(self, engine, net, min_a, max_a, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, batch_size=32,
                 standardizer=None, log_std_min=-5, log_std_max=2, nll_eps=1e-6):
        super().__init__(engine, net, min_a, max_a, standardizer=standardizer, log_std_min=log_std_min,
                         log_std_max=log_std_max, fused_act=True)
        if int(batch_size) < 1 or not float(nll_eps) > 0.0:
            raise OlyError("DeviceGaussianInvActionModel: batch_size >= 1 and nll_eps > 0 are required")
        if int(batch_size) > _abi.OLY_BC_MAX_BATCH:
            raise OlyError(f"DeviceGaussianInvActionModel: batch_size {int(batch_size)} > {_abi.OLY_BC_MAX_BATCH}")
        self.lr, self.betas = float(lr), (float(betas[0]), float(betas[1]))
        self.eps, self.weight_decay, self.nll_eps = float(eps), float(weight_decay), float(nll_eps)
        self.batch = int(batch_size)
        self.exp_avg = torch.zeros_like(self.param)
        self.exp_avg_sq = torch.zeros_like(self.param)
        self.step = 0
        self.use_mean = False        # True: draw_action returns the squashed mean, nothing is drawn (:436-437)
        # the action space in float64 on the device: LSIQfO's clip of the drawn expert actions (lsiqfo.py:90)
        self.bounds = tuple(torch.as_tensor(np.asarray(b, np.float64).reshape(-1), device=engine.device) for b in (min_a, max_a))
        self._ws = engine.bc_fit_ws(self.batch, self.in_dim, self.act_dim)

    def _widths(self, s_tbl, ns_tbl, d1, d2):
        d1 = int(s_tbl.shape[1]) if d1 is None else int(d1)
        d2 = int(ns_tbl.shape[1]) if d2 is None else int(d2)
        if d1 + d2 != self.in_dim:
            raise OlyError(f"DeviceGaussianInvActionModel: rows of {d1} + {d2} columns for a network of {self.in_dim}")
        return d1, d2

    @torch.no_grad()
    def fit(self, states_tbl, next_states_tbl, actions_tbl, idx, d1=None, d2=None):
        """idx.shape[0] fits (:381-401, n_epochs 1 each) in ONE oly_bc_fit_steps call: fit s takes the rows idx[s] of the
        two tables and un-squashes actions_tbl's rows idx[s] as its targets.  idx [n_fits, batch_size] int32.  Returns
        the [n_fits, 3] f64 device block: the loss (what the reference's fit returns, per fit), the Gaussian entropy
        and the mean squared error of the mean."""
        if not isinstance(idx, torch.Tensor) or idx.dim() != 2 or int(idx.shape[1]) != self.batch:
            raise OlyError(f"DeviceGaussianInvActionModel.fit: idx must be a [n_fits, {self.batch}] int32 tensor")
        d1, d2 = self._widths(states_tbl, next_states_tbl, d1, d2)
        colstats = self._colstats()
        out = self.eng.bc_fit_steps(states_tbl, None, idx, colstats, self.param, self.exp_avg, self.exp_avg_sq, self.packed,
                                    self._ws, self.step, self.lr, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps,
                                    weight_decay=self.weight_decay, log_std_min=self.log_std_min,
                                    log_std_max=self.log_std_max, nll_eps=self.nll_eps,
                                    pair=dict(x2=next_states_tbl, actions=actions_tbl, central=self.central,
                                              delta=self.delta, d1=d1, d2=d2))
        n_fits = int(idx.shape[0])
        if colstats is not None and n_fits > 0:
            self.stand._fresh = False
        self.step += n_fits
        return out

    def _act(self, s_tbl, ns_tbl, idx, eps, clip, want, d1, d2):
        d1, d2 = self._widths(s_tbl, ns_tbl, d1, d2)
        colstats = self._colstats()
        o = self.eng.sg_act(s_tbl, self.packed, self.central, self.delta, colstats=colstats, eps=eps,
                            update_stats=colstats is not None, log_std_min=self.log_std_min, log_std_max=self.log_std_max,
                            want=want, x2=ns_tbl, idx=idx, clip=clip, d1=d1, d2=d2)
        if colstats is not None:
            self.stand._fresh = False
        return o

    @torch.no_grad()
    def draw_action(self, s_tbl, ns_tbl, idx=None, eps=None, generator=None, clip=None, d1=None, d2=None):
        """draw_action (:377-379) on the rows idx of the two tables: tanh(mu + exp(log_sigma) eps) delta + central, or the
        squashed mean with use_mean.  eps [n, A] f32 or None: drawn from `generator`.  clip: (lo, hi), [A] float64 device
        tensors: LSIQfO's np.clip against the action space (lsiqfo.py:90), in float64 in the kernel."""
        n = int(idx.shape[0]) if idx is not None else int(s_tbl.shape[0])
        noise = None if self.use_mean else self._noise(n, eps, generator).contiguous()
        if clip is not None:
            clip = tuple(torch.as_tensor(c, dtype=torch.float64, device=self.eng.device).contiguous() for c in clip)
        return self._act(s_tbl, ns_tbl, idx, noise, clip, (), d1, d2)["action"]

    @torch.no_grad()
    def get_mu_log_sigma(self, s_tbl, ns_tbl, idx=None, d1=None, d2=None):
        """get_mu_log_sigma (:450-472): (mu, clamped log_sigma), [n, A] each; the Standardizer takes the rows."""
        o = self._act(s_tbl, ns_tbl, idx, None, None, ("mu", "log_sigma"), d1, d2)
        return o["mu"], o["log_sigma"]

    @torch.no_grad()
    def entropy(self, s_tbl, ns_tbl, idx=None, d1=None, d2=None):
        """entropy (:491-503): the mean over all [n, A] elements of 0.5 + 0.5 log 2 pi + log_sigma, a device scalar."""
        return _HALF_LOG_2PI_E + torch.mean(self.get_mu_log_sigma(s_tbl, ns_tbl, idx, d1, d2)[1])

    # ---- checkpoint: in place, every device buffer keeps its pointer
    def state_dict(self):
        st = self.stand
        return dict(kind="gaussian_inv_action_model", policy=super().state_dict(), exp_avg=self.exp_avg.clone(),
                    exp_avg_sq=self.exp_avg_sq.clone(), step=int(self.step), use_mean=bool(self.use_mean),
                    standardizer=None if st is None else st.state_dict())

    @torch.no_grad()
    def load_state_dict(self, d):
        who = "DeviceGaussianInvActionModel"
        _same(who, "kind", d.get("kind"), "gaussian_inv_action_model")
        _same(who, "standardizer", d["standardizer"] is not None, self.stand is not None)
        super().load_state_dict(d["policy"])
        self.exp_avg.copy_(d["exp_avg"])
        self.exp_avg_sq.copy_(d["exp_avg_sq"])
        self.step, self.use_mean = int(d["step"]), bool(d["use_mean"])
        if self.stand is not None:
            self.stand.load_state_dict(d["standardizer"])

    def save(self, path, **meta):
        from . import il_checkpoint
        return il_checkpoint.save(path, self, None, **meta)

    def load(self, path):
        from . import il_checkpoint
        return il_checkpoint.load(path, self, None)


# the reference's other inverse action models (action_models.py), by the names a caller may hand over
_OTHER_MODELS = {"KLGaussianInvActionModel": "KL-Gaussian", "GCPActionModel": "GCP", "KLGCPActionModel": "KL-GCP",
                 "LearnableVarGaussianInvActionModel": "learnable-variance Gaussian",
                 "FixedVarGaussianInvActionModel": "fixed-variance Gaussian"}
AM_LOG_TAGS = ("Action-Model/Loss Policy", "Action-Model/Loss Exp", "Action-Model/Entropy Plcy", "Action-Model/Entropy Exp",
               "Action-Model/Std Exp", "Action-Model/Std", "Action-Model/Mu Exp", "Action-Model/Mu")


class _FromObservations:
    """What the from-observations agents add to the agents of olympic_hip.iq (module docstring).  The constructor takes
    the parent's arguments and action_model: a DeviceGaussianInvActionModel over 2 * in_dim columns with the policy's A;
    action_model_fit_params: dict(fits_per_step=1, init_epochs=0); interpolate_expert_states / interpolation_coef.
    demonstrations need `states`, `next_states`, `absorbing`; `actions` are optional and used for "Loss Exp" alone.
    am_log: the device scalars of the last logging iteration under AM_LOG_TAGS (no read-back without a writer)."""

    CLIP_DRAW = False        # LSIQfO alone clips the drawn expert actions to the action space

    def __init__(self, engine, policy, critic, demonstrations, *args, action_model=None, action_model_fit_params=None,
                 add_noise_to_obs=False, ext_normalizer_action_model=None, interpolate_expert_states=False,
                 interpolation_coef=1.0, state_mask=None, **kw):
        who = type(self).__name__
        if add_noise_to_obs:
            raise OlyError(f"{who}: add_noise_to_obs=True is not built (observation noise needs an external normaliser)")
        if ext_normalizer_action_model is not None:
            raise OlyError(f"{who}: ext_normalizer_action_model is not built (an external normaliser of the model's rows)")
        name = action_model if isinstance(action_model, str) else getattr(action_model, "__name__", type(action_model).__name__)
        if name in _OTHER_MODELS:
            raise OlyError(f"{who}: the {_OTHER_MODELS[name]} action model ({name}) is not built; the Gaussian one "
                           "(DeviceGaussianInvActionModel) is")
        if interpolate_expert_states and state_mask is not None:
            raise OlyError(f"{who}: interpolate_expert_states with a state_mask is refused: the reference masks the "
                           "interpolated block a second time there (iqfo_sac.py:101, 108)")
        in_dim = int(getattr(policy, "in_dim", 0))
        if 2 * in_dim > 64:
            raise OlyError(f"{who}: 2 * in_dim = {2 * in_dim} > 64 columns of the action model's row (s | s')")
        if not isinstance(action_model, DeviceGaussianInvActionModel):
            raise OlyError(f"{who}: action_model must be a DeviceGaussianInvActionModel, got {name}")
        if int(action_model.in_dim) != 2 * in_dim or int(action_model.act_dim) != int(policy.act_dim):
            raise OlyError(f"{who}: the action model takes {action_model.in_dim} columns and gives {action_model.act_dim} "
                           f"actions; the policy's observation and action need {2 * in_dim} and {policy.act_dim}")
        fp = dict(fits_per_step=1, init_epochs=0) if action_model_fit_params is None else dict(action_model_fit_params)
        unknown = set(fp) - {"fits_per_step", "init_epochs"}
        if unknown or int(fp.get("fits_per_step", 1)) < 0:
            raise OlyError(f"{who}: action_model_fit_params takes fits_per_step >= 0 and init_epochs, got {sorted(fp)}")
        demos = dict(demonstrations)
        self.demo_has_actions = "actions" in demos
        if not self.demo_has_actions and "states" in demos:
            demos["actions"] = np.zeros((len(demos["states"]), int(policy.act_dim)), np.float32)      # never read
        super().__init__(engine, policy, critic, demos, *args, state_mask=state_mask, **kw)
        self.action_model = action_model
        self.fits_per_step = int(fp.get("fits_per_step", 1))
        self.interpolate_expert_states, self.interpolation_coef = bool(interpolate_expert_states), float(interpolation_coef)
        self.am_log = None
        self._am_last = None         # the last fit's batch: the rows of "Std" and "Mu" (the reference reads `state`, :256)

    def _demo_idx32(self, n, generator):
        return self.draw_demo_idx(n, generator).to(torch.int32)

    @torch.no_grad()
    def train_action_model(self, generator=None, samples=None):
        """train_action_model's ordinary branch (:174-264): fits_per_step fits in ONE call, then on a logging iteration
        the sampled draws on a fresh policy sample and a demonstration sample, the two entropies, and get_mu_log_sigma
        on the LAST fit's batch and on the demonstration sample.  samples: None, or the draws given instead of taken from
        `generator`, used as they are: dict(fit_idx [fits_per_step, batch] int32, ip / ie [batch] int32 ring and
        demonstration rows of the logging passes, eps_plcy / eps_exp [batch, A] f32).  Returns the fits'
        [fits_per_step, 3] block or None."""
        am, ring = self.action_model, self.replay
        S, NS, ACT = ring.blocks["states"], ring.blocks["next_states"], ring.blocks["actions"]
        given = samples or {}
        out = None
        if self.fits_per_step > 0:
            idx = given["fit_idx"] if "fit_idx" in given else \
                torch.stack([ring.sample_idx(am.batch, generator) for _ in range(self.fits_per_step)])
            out = am.fit(S, NS, ACT, idx)
            self._am_last = idx[-1]
        if self._iter % self.logging_iter != 0:
            return out
        d = self.demo
        ip = given["ip"] if "ip" in given else ring.sample_idx(am.batch, generator)
        ie = given["ie"] if "ie" in given else self._demo_idx32(am.batch, generator)
        log = {}
        pred = am.draw_action(S, NS, idx=ip, generator=generator, eps=given.get("eps_plcy"))
        log[AM_LOG_TAGS[0]] = torch.mean((pred - ACT[ip.long()]) ** 2)
        if self.demo_has_actions:
            pred = am.draw_action(d["states"], d["next_states"], idx=ie, generator=generator, eps=given.get("eps_exp"))
            log[AM_LOG_TAGS[1]] = torch.mean((pred - d["actions"][ie.long()]) ** 2)
        log[AM_LOG_TAGS[2]] = am.entropy(S, NS, idx=ip)
        log[AM_LOG_TAGS[3]] = am.entropy(d["states"], d["next_states"], idx=ie)
        if self._am_last is not None:            # fits_per_step == 0 leaves the reference's `state` unbound: nothing logged
            mu, ls = am.get_mu_log_sigma(S, NS, idx=self._am_last)
            mu_e, ls_e = am.get_mu_log_sigma(d["states"], d["next_states"], idx=ie)
            log[AM_LOG_TAGS[4]], log[AM_LOG_TAGS[5]] = torch.mean(torch.exp(ls_e)), torch.mean(torch.exp(ls))
            log[AM_LOG_TAGS[6]], log[AM_LOG_TAGS[7]] = torch.mean(mu_e), torch.mean(mu)
        self.am_log = log
        if self.sw is not None:
            for k, v in log.items():
                self.sw.add_scalar(k, float(v), self._iter)
        return out

    @torch.no_grad()
    def fit(self, dataset, generator=None, samples=None):
        """IQfO_SAC.fit (iqfo_sac.py:59-120; LSIQfO's with its clip, lsiqfo.py:59-123).  samples: None, or the draws of
        the iteration given instead of taken from `generator`: train_action_model's and idx_policy / idx_demo [batch]
        int32 (the policy minibatch's ring rows, the demonstration rows), eps_draw [batch, A] f32 (the expert draw),
        eps_update (iq_update's eps).  Returns iq_update's pair or None."""
        ring, d, am = self.replay, self.demo, self.action_model
        given = samples or {}
        ring.add(dataset)
        out = None
        if ring.initialized:
            self.train_action_model(generator, samples)
            ip = (given["idx_policy"] if "idx_policy" in given else ring.sample_idx(self.batch_size, generator)).long()
            s, a, ns, ab = (ring.blocks[k][ip] for k in ("states", "actions", "next_states", "absorbing"))
            ie = given["idx_demo"] if "idx_demo" in given else self._demo_idx32(int(s.shape[0]), generator)
            demo_act = am.draw_action(d["states"], d["next_states"], idx=ie, generator=generator, eps=given.get("eps_draw"),
                                      clip=am.bounds if self.CLIP_DRAW else None)
            il = ie.long()
            demo_obs = d["states"][il]
            if self.interpolate_expert_states:
                c = self.interpolation_coef
                demo_obs = c * demo_obs + (1 - c) * s
                demo_act = c * demo_act + (1 - c) * a
            out = self.iq_update(torch.cat([s, demo_obs]), torch.cat([a, demo_act]), torch.cat([ns, d["next_states"][il]]),
                                 torch.cat([ab, d["absorbing"][il]]), int(s.shape[0]), eps=given.get("eps_update"),
                                 generator=generator)
        self._iter += 1
        self.policy.iter = getattr(self.policy, "iter", 0) + 1
        return out

    def state_dict(self):
        d = super().state_dict()
        d["action_model"] = self.action_model.state_dict()
        d["am_last"] = None if self._am_last is None else self._am_last.clone()
        return d

    @torch.no_grad()
    def load_state_dict(self, d):
        super().load_state_dict(d)
        self.action_model.load_state_dict(d["action_model"])
        self._am_last = None if d["am_last"] is None else torch.as_tensor(d["am_last"]).to(self.eng.device, torch.int32)


class DeviceIQfOSAC(_FromObservations, DeviceIQSAC):
    """IQfO_SAC (imitation_lib/imitation/iqfo_sac.py): DeviceIQSAC with the inverse action model."""

    KIND = "iqfo_sac"


class DeviceLSIQfOSAC(_FromObservations, DeviceLSIQSAC):
    """LSIQfO (lsiqfo.py): DeviceLSIQSAC with the inverse action model; the drawn expert actions are clipped to the action
    space in float64 (:90)."""

    KIND = "lsiqfo_sac"
    CLIP_DRAW = True


class DeviceLSIQfOHSAC(_FromObservations, DeviceLSIQHSAC):
    """LSIQfO_H (lsiqfo_h.py): DeviceLSIQHSAC with the inverse action model (no clip of the drawn actions)."""

    KIND = "lsiqfo_h_sac"


class DeviceLSIQfOHCSAC(_FromObservations, DeviceLSIQHCSAC):
    """LSIQfO_HC (lsiqfo_hc.py): DeviceLSIQHCSAC with the inverse action model (no clip of the drawn actions)."""

    KIND = "lsiqfo_hc_sac"


__all__ = ["DeviceGaussianInvActionModel", "DeviceIQfOSAC", "DeviceLSIQfOSAC", "DeviceLSIQfOHSAC", "DeviceLSIQfOHCSAC",
           "AM_LOG_TAGS"]
