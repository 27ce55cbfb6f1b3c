"""Behavioural cloning on the device (imitation_lib/imitation/offline/behavioral_cloning.py) and the squashed-Gaussian
policy it trains (IQ_Learn_Policy, imitation_lib/imitation/iq_sac.py:18-167).

  IQ_Learn_Policy(Regressor(FullyConnectedNetwork(in -> [512, 256] -> 2A)), min_a, max_a, log_std_min, log_std_max)
      get_mu_log_sigma / distribution / compute_action_and_log_prob / entropy_from_logsigma / get_central_delta
                                                         -> DeviceSquashedGaussianPolicy (K16's forward, oly_ilmlp_forward,
                                                            then torch elementwise operations; fused_act=True: one
                                                            oly_sg_act call, K25)
  BehavioralCloning.fit_offline (:46-80) and logging (:82-94)
                                                         -> DeviceBehavioralCloning.fit_offline (K24, oly_bc_fit_steps:
                                                            every step of a call on the device, no host synchronisation)
  the un-squashing of the target actions (:63-66)         -> once at construction (oly_bc_targets): the demonstrations
                                                            are fixed

Stated differences from the reference: a minibatch is the first `batch_size` entries of a fresh device permutation, as
next(minibatch_generator(...)) gives (rows within a step are distinct): the same distribution, another sequence than
numpy's; a given `idx` is used as it is.  "Squashed Gaussian Entropy (Empirical)" needs a sampled second forward per
logged step, which also feeds the Standardizer the minibatch a second time: it is opt-in (empirical_entropy=True, K25);
without it a fit with a Standardizer holds every minibatch once where the reference holds a logged one twice.  Entropy
projection (use_entropy_projec, off by default in the reference) is not built.
"""
import numpy as np
import torch

from . import _abi
from ._ffi import OlyError
from .gail import DeviceStandardizer, _same

_H1, _H2 = 512, 256
LOG_NAMES = _abi.BC_LOG_TAGS


class DeviceSquashedGaussianPolicy:
    """The reference's IQ_Learn_Policy held on the device: flat parameters `param` in torch order W1 | b1 | W2 | b2 |
    W3 [2A,256] | b3 [2A] and K16's packed stream.  Output columns [0, A) are mu, [A, 2A) log_sigma, clamped to
    [log_std_min, log_std_max]; an action is tanh(mu + exp(log_sigma) eps) delta + central with central / delta =
    (max_a + min_a) / 2, (max_a - min_a) / 2.

    net: the reference's FullyConnectedNetwork (its `_linears`) or a list of its three nn.Linear layers, in <= 64 -> 512
    -> 256 -> 2A, A <= 16.  standardizer: a DeviceStandardizer or None; with one, every forward the reference runs through
    FullyConnectedNetwork.forward adds its rows to the statistics first (networks.py:68-81): get_mu_log_sigma and what
    is built on it do, predict does not.  fused_act=True: act and compute_action_and_log_prob are one oly_sg_act call
    (K25) instead of the forward and torch's elementwise operations; the contract, the arguments and the draws from
    `generator` are the same, the values agree to float32 rounding (the tanh is correctly rounded, the log-probability
    is summed in float64)."""

    def __init__(self, engine, net, min_a, max_a, standardizer=None, log_std_min=-20, log_std_max=2, fused_act=False):
        lins = list(getattr(net, "_linears", net))
        if len(lins) != 3:
            raise OlyError(f"DeviceSquashedGaussianPolicy: expected three Linear layers, got {len(lins)}")
        self.eng, self.net, self.lins, self.stand = engine, net, lins, standardizer
        self.in_dim, self.out_dim = int(lins[0].in_features), int(lins[2].out_features)
        if (int(lins[0].out_features), int(lins[1].in_features), int(lins[1].out_features),
                int(lins[2].in_features)) != (_H1, _H1, _H2, _H2) or not 0 < self.in_dim <= 64:
            raise OlyError("DeviceSquashedGaussianPolicy: supported shape is in <= 64 -> 512 -> 256 -> 2A")
        if self.out_dim % 2 != 0 or not 0 < self.out_dim // 2 <= _abi.OLY_BC_MAX_ACT:
            raise OlyError(f"DeviceSquashedGaussianPolicy: the output width {self.out_dim} must be 2A with 1 <= A <= "
                           f"{_abi.OLY_BC_MAX_ACT}")
        self.act_dim = self.out_dim // 2
        min_a = np.asarray(min_a, np.float64).reshape(-1)
        max_a = np.asarray(max_a, np.float64).reshape(-1)
        if min_a.shape != (self.act_dim,) or max_a.shape != (self.act_dim,):
            raise OlyError(f"DeviceSquashedGaussianPolicy: min_a / max_a must have {self.act_dim} entries")
        if standardizer is not None and int(standardizer.dim) != self.in_dim:
            raise OlyError(f"DeviceSquashedGaussianPolicy: the standardizer has {standardizer.dim} columns, the network "
                           f"{self.in_dim}")
        if not float(log_std_min) <= float(log_std_max):
            raise OlyError("DeviceSquashedGaussianPolicy: log_std_min <= log_std_max is required")
        dev = engine.device
        # to_float_tensor(.5 * (max_a -+ min_a)): formed in float64, narrowed to float32 (iq_sac.py:43-44)
        self.delta = torch.as_tensor((0.5 * (max_a - min_a)).astype(np.float32), device=dev)
        self.central = torch.as_tensor((0.5 * (max_a + min_a)).astype(np.float32), device=dev)
        self.log_std_min, self.log_std_max = float(log_std_min), float(log_std_max)
        self.eps_log_prob = 1e-6
        self.fused_act = bool(fused_act)
        with torch.no_grad():
            self.param = torch.cat([t.detach().reshape(-1).to(device=dev, dtype=torch.float32)
                                    for lin in lins for t in (lin.weight, lin.bias)]).contiguous()
        self.packed = engine.ilmlp_pack(*self._views())

    def _views(self):
        shapes = [(_H1, self.in_dim), (_H1,), (_H2, _H1), (_H2,), (self.out_dim, _H2), (self.out_dim,)]
        out, o = [], 0
        for s in shapes:
            n = int(np.prod(s))
            out.append(self.param[o:o + n].view(s))
            o += n
        return out

    @property
    def n_par(self):
        return int(self.param.numel())

    def repack(self):
        """Re-pack the stream after param was written (set_weights and load_state_dict do this)."""
        self.eng.ilmlp_pack(*self._views(), packed=self.packed)

    def _colstats(self):
        st = self.stand
        if st is None:
            return None
        if getattr(st, "_fresh", False):     # the running sums start from zero; a fit adds to them in place
            st.colstats.zero_()
        return st.colstats

    def _rows(self, obs):
        return obs.reshape(-1, self.in_dim).to(torch.float32).contiguous()

    @torch.no_grad()
    def predict(self, obs):
        """The raw network output [n, 2A] with the current statistics, without updating them (K16's forward)."""
        return self.eng.ilmlp_forward(self._rows(obs), self.packed, self.out_dim, "identity", colstats=self._colstats())

    @torch.no_grad()
    def get_mu_log_sigma(self, obs):
        """iq_sac.py:132-151: the statistics take obs's rows (the network's forward), then mu = out[:, :A] and
        log_sigma = clamp(out[:, A:], log_std_min, log_std_max)."""
        x = self._rows(obs)
        if self.stand is not None:
            self.stand.update_mean_std(x)
        y = self.predict(x)
        return y[:, :self.act_dim], torch.clamp(y[:, self.act_dim:], self.log_std_min, self.log_std_max)

    def distribution(self, obs):
        mu, log_sigma = self.get_mu_log_sigma(obs)
        return torch.distributions.Normal(mu, log_sigma.exp())

    def _noise(self, n, eps, generator):
        if eps is None:
            return torch.randn((n, self.act_dim), dtype=torch.float32, device=self.eng.device, generator=generator)
        return eps.reshape(n, self.act_dim).to(torch.float32)

    def _fused(self, obs, eps, want):
        """One oly_sg_act call on obs's rows: the statistics take them first, as get_mu_log_sigma does."""
        colstats = self._colstats()
        o = self.eng.sg_act(self._rows(obs), self.packed, self.central, self.delta, colstats=colstats,
                            eps=None if eps is None else eps.contiguous(), update_stats=colstats is not None,
                            log_std_min=self.log_std_min, log_std_max=self.log_std_max, want=want)
        if colstats is not None:
            self.stand._fresh = False
        return o

    @torch.no_grad()
    def act(self, obs, generator=None, eps=None, deterministic=False, ctrl=False):
        """draw_action for the collection loop (ILCore's contract): the statistics take obs's rows, action =
        tanh(mu + exp(log_sigma) eps) delta + central (iq_sac.py:102-130); deterministic=True: the squashed mean,
        nothing is drawn (use_mean).  eps None: drawn from `generator`.  With ctrl=True the engine's configured model's
        clamped control vector of that action (oly_il_ctrl).  Returns (action [n,A], ctrl [n,nu] or None)."""
        if self.fused_act:
            x = self._rows(obs)
            noise = None if deterministic else self._noise(int(x.shape[0]), eps, generator)
            o = self._fused(x, noise, ("ctrl",) if ctrl else ())
            return o["action"], o["ctrl"]
        mu, log_sigma = self.get_mu_log_sigma(obs)
        a_raw = mu if deterministic else mu + log_sigma.exp() * self._noise(int(mu.shape[0]), eps, generator)
        action = (torch.tanh(a_raw) * self.delta + self.central).contiguous()
        return action, (self.eng.il_ctrl(action) if ctrl else None)

    @torch.no_grad()
    def compute_action_and_log_prob(self, obs, generator=None, eps=None):
        """compute_action_and_log_prob_t (iq_sac.py:102-130): the sampled action and its log-probability [n] with the
        tanh correction log(1 - a^2 + 1e-6), device tensors."""
        if self.fused_act:
            x = self._rows(obs)
            o = self._fused(x, self._noise(int(x.shape[0]), eps, generator), ("log_prob",))
            return o["action"], o["log_prob"]
        mu, log_sigma = self.get_mu_log_sigma(obs)
        dist = torch.distributions.Normal(mu, log_sigma.exp())
        a_raw = mu + log_sigma.exp() * self._noise(int(mu.shape[0]), eps, generator)
        a = torch.tanh(a_raw)
        log_prob = dist.log_prob(a_raw).sum(dim=1)
        log_prob = log_prob - torch.log(1.0 - a.pow(2) + self.eps_log_prob).sum(dim=1)
        return a * self.delta + self.central, log_prob

    def entropy_from_logsigma(self, log_sigma):
        return self.act_dim * (0.5 + 0.5 * float(np.log(2 * np.pi))) + torch.sum(log_sigma, dim=-1)

    def get_central_delta(self):
        return self.central, self.delta

    def get_weights(self):
        """The flat parameters in torch order (a device copy)."""
        return self.param.clone()

    @torch.no_grad()
    def set_weights(self, w):
        w = torch.as_tensor(w, dtype=torch.float32, device=self.param.device).reshape(-1)
        if int(w.numel()) != self.n_par:
            raise OlyError(f"DeviceSquashedGaussianPolicy.set_weights: {w.numel()} values for {self.n_par} parameters")
        self.param.copy_(w)
        self.repack()

    @torch.no_grad()
    def sync_to_torch(self):
        """Write the parameters back into the wrapped Linear layers (torch-side evaluation)."""
        v = self._views()
        for i, lin in enumerate(self.lins):
            lin.weight.copy_(v[2 * i].to(lin.weight.device))
            lin.bias.copy_(v[2 * i + 1].to(lin.bias.device))
        return self.net

    # ---- checkpoint (il_checkpoint); the Standardizer is stored by the trainer that owns the policy
    def state_dict(self):
        return dict(in_dim=self.in_dim, act_dim=self.act_dim, param=self.param.clone(), central=self.central.clone(),
                    delta=self.delta.clone(), log_std_min=self.log_std_min, log_std_max=self.log_std_max)

    @torch.no_grad()
    def load_state_dict(self, d):
        """In place (param and `packed` keep their pointers), then repack()."""
        who = "DeviceSquashedGaussianPolicy"
        _same(who, "in_dim", int(d["in_dim"]), self.in_dim)
        _same(who, "act_dim", int(d["act_dim"]), self.act_dim)
        self.param.copy_(d["param"])
        self.central.copy_(d["central"])
        self.delta.copy_(d["delta"])
        self.log_std_min, self.log_std_max = float(d["log_std_min"]), float(d["log_std_max"])
        self.repack()


class DeviceBehavioralCloning:
    """BehavioralCloning (behavioral_cloning.py:14-99) with its hot loop on the device.

    policy: a DeviceSquashedGaussianPolicy; its `param` and `packed` are stepped in place.  demonstrations: a dict with
    `states` [n,in] and `actions` [n,A] (device tensors or numpy arrays); `next_states` and `absorbing` are accepted and
    ignored, as the reference ignores them.  The optimiser is torch.optim.Adam(lr, betas, eps, weight_decay) (amsgrad
    off) over torch.nn.GaussianNLLLoss(); its step count persists across fit_offline calls.  sw: an object with
    add_scalar(name, value, iteration), or None.

    empirical_entropy=True: the whole of logging() (:82-94).  Every logging_iter iterations the reference calls
    policy.compute_action_and_log_prob on the minibatch: the Standardizer takes the minibatch's rows a second time, the
    forward runs with the weights Adam has just stepped, and -mean(log_prob) of a sample is logged as "Squashed Gaussian
    Entropy (Empirical)".  fit_offline then goes through oly_bc_fit_steps_log (K24 + K25) and returns four columns."""

    def __init__(self, engine, policy, demonstrations, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, batch_size=32,
                 logging_iter=1, sw=None, empirical_entropy=False):
        if not isinstance(policy, DeviceSquashedGaussianPolicy):
            raise OlyError("DeviceBehavioralCloning: policy must be a DeviceSquashedGaussianPolicy")
        for k in ("states", "actions"):
            if k not in demonstrations:
                raise OlyError(f"DeviceBehavioralCloning: demonstrations have no {k!r} (behavioural cloning needs actions)")
        self.eng, self.policy = engine, policy
        dev = engine.device

        def up(a, width, name):
            t = torch.as_tensor(a).to(device=dev, dtype=torch.float32)
            if t.dim() != 2 or int(t.shape[1]) != width or int(t.shape[0]) < 1:
                raise OlyError(f"DeviceBehavioralCloning: demonstrations[{name!r}] has shape {tuple(t.shape)}, expected "
                               f"[n >= 1, {width}]")
            return t.contiguous()
        self.states = up(demonstrations["states"], policy.in_dim, "states")
        actions = up(demonstrations["actions"], policy.act_dim, "actions")
        self.n = int(self.states.shape[0])
        if int(actions.shape[0]) != self.n:
            raise OlyError(f"DeviceBehavioralCloning: {actions.shape[0]} action rows for {self.n} state rows")
        if int(batch_size) < 1 or int(logging_iter) < 1:
            raise OlyError("DeviceBehavioralCloning: batch_size >= 1 and logging_iter >= 1 are required")
        self.batch = min(int(batch_size), self.n)          # minibatch_generator's first batch of a table of n rows
        if self.batch > _abi.OLY_BC_MAX_BATCH:
            raise OlyError(f"DeviceBehavioralCloning: batch_size {self.batch} > {_abi.OLY_BC_MAX_BATCH}")
        self.lr, self.betas = float(lr), (float(betas[0]), float(betas[1]))
        self.eps, self.weight_decay = float(eps), float(weight_decay)
        self.logging_iter, self.sw = int(logging_iter), sw
        self.nll_eps = 1e-6                                # GaussianNLLLoss() as the reference constructs it
        self.targets = engine.bc_targets(actions, policy.central, policy.delta)     # once: the demonstrations are fixed
        self.exp_avg = torch.zeros_like(policy.param)
        self.exp_avg_sq = torch.zeros_like(policy.param)
        self.step = 0
        self.iter = 0
        self.empirical_entropy = bool(empirical_entropy)
        self._ws = (engine.bc_fit_log_ws if self.empirical_entropy else engine.bc_fit_ws)(self.batch, policy.in_dim,
                                                                                         policy.act_dim)

    def fit(self, dataset):
        raise AttributeError("This is a behavior cloning algorithms, which is meant to run offline. It is not supposed"
                             "to use the fit function. Use the fit_offline function instead.")

    def draw_idx(self, n_steps, generator=None):
        """idx [n_steps, batch] int32 on the device: every row the first `batch` entries of a fresh permutation of the
        demonstrations (the smallest `batch` of n uniform keys per step; the steps go through top-k in blocks of at most
        2^24 keys, so a large table does not need n_steps * n floats at once)."""
        n_steps, per = int(n_steps), max(1, (1 << 24) // self.n)
        out = torch.empty((n_steps, self.batch), dtype=torch.int32, device=self.eng.device)
        for s in range(0, n_steps, per):
            keys = torch.rand((min(per, n_steps - s), self.n), device=self.eng.device, generator=generator)
            out[s:s + per] = torch.topk(keys, self.batch, dim=1, largest=False, sorted=True).indices
        return out

    @torch.no_grad()
    def fit_offline(self, n_steps, generator=None, idx=None, eps=None):
        """n_steps iterations of fit_offline in ONE oly_bc_fit_steps call.  idx: [n_steps, batch] int32 device rows, or
        None (drawn from `generator`).  Returns the [n_steps, 3] f64 device block of LOG_NAMES' scalars; with a writer
        they go to sw.add_scalar under the reference's names every logging_iter iterations (which reads them back).

        With empirical_entropy the call is ONE oly_bc_fit_steps_log and the block is [n_steps, 4]: column 3 is "Squashed
        Gaussian Entropy (Empirical)" on the iterations that log (self.iter + s a multiple of logging_iter) and NaN on
        the others.  eps: [n_logged, batch, A] f32 standard normal noise of the logging steps in order, or None: drawn
        from `generator` AFTER idx (first every step's permutation keys, then one randn of that shape)."""
        n_steps = int(n_steps)
        if n_steps < 0:
            raise OlyError(f"DeviceBehavioralCloning.fit_offline: n_steps={n_steps}")
        if idx is None:
            idx = self.draw_idx(n_steps, generator)
        elif not isinstance(idx, torch.Tensor) or tuple(idx.shape) != (n_steps, self.batch):
            raise OlyError(f"DeviceBehavioralCloning.fit_offline: idx must be a [{n_steps}, {self.batch}] int32 tensor")
        p = self.policy
        colstats = p._colstats()
        if self.empirical_entropy:
            return self._fit_logged(n_steps, generator, idx, eps, colstats)
        if eps is not None:
            raise OlyError("DeviceBehavioralCloning.fit_offline: eps is the noise of empirical_entropy=True")
        out = self.eng.bc_fit_steps(self.states, self.targets, idx, colstats, p.param, self.exp_avg, self.exp_avg_sq,
                                    p.packed, self._ws, self.step, self.lr, beta1=self.betas[0], beta2=self.betas[1],
                                    eps=self.eps, weight_decay=self.weight_decay, log_std_min=p.log_std_min,
                                    log_std_max=p.log_std_max, nll_eps=self.nll_eps)
        if colstats is not None and n_steps > 0:
            p.stand._fresh = False
        if self.sw is not None and n_steps > 0:
            host = out.cpu().numpy()
            for s in range(n_steps):
                if (self.iter + s) % self.logging_iter == 0:
                    for k, name in enumerate(LOG_NAMES):
                        self.sw.add_scalar(name, float(host[s, k]), self.iter + s)
        self.step += n_steps
        self.iter += n_steps
        return out

    def _fit_logged(self, n_steps, generator, idx, eps, colstats):
        p = self.policy
        logged = self.eng.bc_logged_steps(n_steps, self.logging_iter, self.iter)
        shape = (len(logged), self.batch, p.act_dim)
        if eps is None:
            eps = torch.randn(shape, dtype=torch.float32, device=self.eng.device, generator=generator)
        elif not isinstance(eps, torch.Tensor) or tuple(eps.shape) != shape:
            raise OlyError(f"DeviceBehavioralCloning.fit_offline: eps must be a {list(shape)} float32 tensor "
                           f"({len(logged)} of the {n_steps} steps log)")
        out = self.eng.bc_fit_steps_log(self.states, self.targets, idx, colstats, p.param, self.exp_avg, self.exp_avg_sq,
                                        p.packed, self._ws, self.step, self.lr, self.logging_iter, self.iter,
                                        eps.to(torch.float32).contiguous(), beta1=self.betas[0], beta2=self.betas[1],
                                        eps=self.eps, weight_decay=self.weight_decay, log_std_min=p.log_std_min,
                                        log_std_max=p.log_std_max, nll_eps=self.nll_eps)
        if colstats is not None and n_steps > 0:
            p.stand._fresh = False
        if self.sw is not None and n_steps > 0:
            host = out.cpu().numpy()
            for s in logged:
                for k, name in enumerate(LOG_NAMES + (_abi.BC_LOG_TAG_EMPIRICAL,)):
                    self.sw.add_scalar(name, float(host[s, k]), self.iter + s)
        self.step += n_steps
        self.iter += n_steps
        return out

    # ---- checkpoint (il_checkpoint.save / load take this object as the agent)
    def state_dict(self):
        st = self.policy.stand
        return dict(kind="behavioral_cloning", policy=self.policy.state_dict(),
                    exp_avg=self.exp_avg.clone(), exp_avg_sq=self.exp_avg_sq.clone(), step=int(self.step),
                    iter=int(self.iter), standardizer=None if st is None else st.state_dict())

    @torch.no_grad()
    def load_state_dict(self, d):
        """In place (every device buffer keeps its pointer)."""
        who = "DeviceBehavioralCloning"
        _same(who, "kind", d.get("kind"), "behavioral_cloning")
        st = self.policy.stand
        _same(who, "standardizer", d["standardizer"] is not None, st is not None)
        self.policy.load_state_dict(d["policy"])
        self.exp_avg.copy_(d["exp_avg"])
        self.exp_avg_sq.copy_(d["exp_avg_sq"])
        self.step, self.iter = int(d["step"]), int(d["iter"])
        if st is not None:
            st.load_state_dict(d["standardizer"])

    def save(self, path, **meta):
        from . import il_checkpoint
        return il_checkpoint.save(path, self, None, **meta)

    def load(self, path):
        from . import il_checkpoint
        return il_checkpoint.load(path, self, None)


__all__ = ["DeviceSquashedGaussianPolicy", "DeviceBehavioralCloning", "DeviceStandardizer", "LOG_NAMES"]
