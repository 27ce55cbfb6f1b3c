"""The imitation-learning agent's fit (GAIL_TRPO.fit, imitation_lib/imitation/gail_TRPO.py:105-165) on the device.

  critic FullyConnectedNetwork(obs -> [512, 256] -> 1)     examples/imitation_learning/utils.py:136-149
      evaluation                                          -> DeviceILCritic.__call__ (K16, oly_ilmlp_forward)
      Regressor.fit (mushroom's minibatch loop + Adam)    -> DeviceILCritic.fit (K16, oly_il_critic_fit_epoch)
  discriminator reward, GAE, advantage normalisation      -> DiscriminatorReward (K12), GAERollout (K6 + K7)
  discriminator training (_fit_discriminator, :167-220)   -> DeviceDiscriminatorTrainer (K15, oly_disc_fit_epoch), for
                                                             GAIL DeviceGAILDiscriminatorTrainer (K18,
                                                             oly_gail_disc_fit_epoch) under GAILAgent, or
                                                             the caller's DiscriminatorTrainer (torch, a different
                                                             reading: one Adam step per epoch on the whole batch)
  TRPO's policy step (:131-149)                           -> the caller's policy_step, e.g. DeviceTRPO (K17,
                                                             oly_trpo_step) on a DeviceGaussianPolicy
  the iteration's diagnostics (_logging_sw, :163, 251-272) -> VAILAgent(iteration_log=True) (K20, oly_iter_log);
                                                             compute_J / compute_episodes_length: episode_stats
  acting in the collection loop (core.learn / evaluate)   -> DeviceGaussianPolicy.act (K21, oly_il_act); the loop
                                                             itself is il_core.ILCore

The critic shares the policy's running Standardizer (trpo_standardizer, utils.py:123); every evaluation and every
fit minibatch adds its rows to it, as Standardizer.forward does (networks.py:68-81).
"""
import numpy as np
import torch

from . import _abi
from ._ffi import OlyError
from .gail import _same

_H1, _H2 = 512, 256

# The scalars of _discriminator_logging in the order of the reference's add_scalar calls (gail_TRPO.py:227-249; VAIL adds
# vail_TRPO.py:30-32): the columns of the `logs` a device trainer's fit(log=True) returns.
DISC_LOG_NAMES = dict(gail=_abi.DISC_LOG_TAGS[:9], vail=_abi.DISC_LOG_TAGS)
# The scalars of _logging_sw in the order of the reference's add_scalar calls (gail_TRPO.py:267-272): the keys of the
# `iter_log` an agent built with iteration_log=True returns.
ITER_LOG_NAMES = _abi.ITER_LOG_TAGS


def episode_stats(eng, reward, last, gamma=1.0, reward2=None):
    """mushroom-rl's compute_J(dataset, gamma) and compute_episodes_length(dataset) (a reading of mushroom-rl >= 1.10;
    the launcher's Eval_R / Eval_J / Eval_L, examples/imitation_learning/experiment.py:57-64, and _logging_sw's episode
    scalars) over [T,N] device blocks, every environment's column one dataset: reward f32 or f64, reward2 an optional
    second f32 block, last bool or uint8.  Returns a device tensor [8] f64 without synchronising: mean return, mean return
    of reward2 (0 without), mean length, number of returns, number of lengths, sum of the returns, of reward2's, of the
    lengths.  An episode still open at the end of a column counts among the returns and not among the lengths; without
    a completed episode the mean length is NaN (the reference raises in int(np.round(nan)))."""
    T, N = int(reward.shape[0]), int(reward.shape[1])
    return eng.episode_stats(reward.reshape(T, N).contiguous(), last.reshape(T, N).contiguous(), gamma=gamma,
                             reward2=None if reward2 is None else reward2.reshape(T, N).to(torch.float32).contiguous())


class DeviceILCritic:
    """A relu MLP in -> 512 -> 256 -> out held as flat parameters (torch order), Adam moments and the packed stream.

    net: a module with `_linears` (the reference's FullyConnectedNetwork) or a list of its three nn.Linear layers.
    standardizer: the DeviceStandardizer shared with the policy (its running statistics are updated in place).
    The fit (out_dim == 1) is torch.optim.Adam(lr, betas, eps, weight_decay=0) over F.mse_loss, as the reference's
    critic_params configure it (utils.py:136-149); the optimiser's step count persists across fit() calls."""

    def __init__(self, engine, net, standardizer, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, last_activation="identity"):
        lins = list(getattr(net, "_linears", net))
        if len(lins) != 3:
            raise OlyError(f"DeviceILCritic: expected three Linear layers, got {len(lins)}")
        self.eng, self.net, self.lins, self.stand = engine, net, lins, standardizer
        self.in_dim, self.out_dim = int(lins[0].in_features), int(lins[2].out_features)
        if (int(lins[0].out_features), int(lins[1].in_features), int(lins[1].out_features),
                int(lins[2].in_features)) != (_H1, _H1, _H2, _H2):
            raise OlyError("DeviceILCritic: supported shape is in -> 512 -> 256 -> out")
        self.lr, self.betas, self.eps, self.act = float(lr), (float(betas[0]), float(betas[1])), float(eps), last_activation
        dev = engine.device
        with torch.no_grad():
            self.param = torch.cat([t.detach().reshape(-1).to(device=dev, dtype=torch.float32)
                                    for lin in lins for t in (lin.weight, lin.bias)]).contiguous()
        self.exp_avg = torch.zeros_like(self.param)
        self.exp_avg_sq = torch.zeros_like(self.param)
        self.step = 0
        self._ws = None
        self.packed = engine.ilmlp_pack(*self._views())

    def _views(self):
        shapes = [(_H1, self.in_dim), (_H1,), (_H2, _H1), (_H2,), (self.out_dim, _H2), (self.out_dim,)]
        out, o = [], 0
        for s in shapes:
            n = 1
            for d in s:
                n *= d
            out.append(self.param[o:o + n].view(s))
            o += n
        return out

    @torch.no_grad()
    def predict(self, x):
        """net(standardise(x)) with the current statistics, without updating them."""
        return self.eng.ilmlp_forward(x, self.packed, self.out_dim, self.act, colstats=self.stand.colstats)

    @torch.no_grad()
    def __call__(self, x):
        """Standardizer.forward then the network: the statistics take x's rows first (networks.py:68-81)."""
        self.stand.update_mean_std(x)
        return self.predict(x)

    @torch.no_grad()
    def fit(self, x, v_target, n_epochs, batch_size=256, generator=None):
        """Regressor.fit: n_epochs epochs, each a fresh device permutation cut into minibatches of batch_size (the
        last one partial), one oly_il_critic_fit_epoch call per epoch.  Returns the per-minibatch losses, [n_epochs,
        n_batches] f64 on the device."""
        if self.out_dim != 1:
            raise OlyError(f"DeviceILCritic.fit: the fit covers out_dim == 1 (this network has {self.out_dim})")
        x = x.reshape(-1, self.in_dim).to(torch.float32).contiguous()
        n = int(x.shape[0])
        v = v_target.reshape(n).to(torch.float32).contiguous()
        if self._ws is None or self._ws[0] != int(batch_size):
            self._ws = (int(batch_size), self.eng.il_critic_fit_ws(batch_size, self.in_dim))
        st = self.stand
        if getattr(st, "_fresh", False):     # the running sums start from zero; the fit adds to them in place
            st.colstats.zero_()
            st._fresh = False
        nb = (n + int(batch_size) - 1) // int(batch_size)
        losses = torch.empty((int(n_epochs), nb), dtype=torch.float64, device=self.eng.device)
        for e in range(int(n_epochs)):
            perm = torch.randperm(n, generator=generator, device=self.eng.device).to(torch.int32)
            self.eng.il_critic_fit_epoch(x, v, perm, batch_size, st.colstats, self.param, self.exp_avg,
                                         self.exp_avg_sq, self.packed, self._ws[1], self.step, self.lr,
                                         beta1=self.betas[0], beta2=self.betas[1], eps=self.eps, loss_out=losses[e])
            self.step += nb
        return losses

    @torch.no_grad()
    def sync_to_torch(self):
        """Write the fitted parameters back into the wrapped Linear layers (checkpoints, torch-side evaluation)."""
        views = self._views()
        for i, lin in enumerate(self.lins):
            lin.weight.copy_(views[2 * i].to(lin.weight.device))
            lin.bias.copy_(views[2 * i + 1].to(lin.bias.device))
        return self.net

    # ---- checkpoint (il_checkpoint); the shared Standardizer is the agent's to store
    def state_dict(self):
        return dict(in_dim=self.in_dim, out_dim=self.out_dim, param=self.param.clone(), exp_avg=self.exp_avg.clone(),
                    exp_avg_sq=self.exp_avg_sq.clone(), step=int(self.step))

    @torch.no_grad()
    def load_state_dict(self, d):
        """In place (param, the moments and `packed` keep their pointers), then the stream is packed again."""
        _same("DeviceILCritic", "in_dim", int(d["in_dim"]), self.in_dim)
        _same("DeviceILCritic", "out_dim", int(d["out_dim"]), self.out_dim)
        for k in ("param", "exp_avg", "exp_avg_sq"):
            getattr(self, k).copy_(d[k])
        self.step = int(d["step"])
        self.eng.ilmlp_pack(*self._views(), packed=self.packed)


class VAILAgent:
    """GAIL_TRPO.fit (gail_TRPO.py:105-165) for VAIL_TRPO with the critic on K16:

        trpo_standardizer.update_mean_std(x)
        r = r_env * env_reward_frac + r_disc * (1 - env_reward_frac)      (discriminator reward, K12)
        v_target, adv = compute_gae(V, x, xn, r, absorbing, last, gamma, lam), adv normalised (K6 + K7; V(x) then
                        V(xn), each updating the statistics)
        policy_step(obs, act, adv, agent)                                  (the caller's TRPO step)
        trpo_standardizer.update_mean_std(x)  critic_fit_params["n_epochs"] times
        V.fit(x, v_target, **critic_fit_params)                            (K16)
        disc_trainer.fit(x) when iter % train_D_n_th_epoch == 0
        iter += 1

    disc_reward: DiscriminatorReward; disc_trainer: DiscriminatorTrainer (or anything with fit(x, generator=));
    critic: DeviceILCritic whose standardizer is the policy's trpo_standardizer.

    sw: None, or a writer (anything with add_scalar(tag, value, step)) as the reference's launcher always passes one
    (examples/imitation_learning/experiment.py:37,48).  With it every trained iteration runs _discriminator_logging
    (gail_TRPO.py:222-249) on the device after each discriminator epoch, which also moves the discriminator's
    Standardizer as the reference's extra forwards do, reads the scalars back once and calls
    sw.add_scalar(tag, value, iter // 3) with the reference's tags in its order (DISC_LOG_NAMES), per epoch; the result
    gains disc_log, a dict tag -> the last epoch's value.

    iteration_log: False, or True to run _logging_sw (:163, 251-272) as well, which the reference does on the same
    iterations: after the discriminator's fit and its diagnostics one oly_iter_log call (K20) forms EpTrueRewMean,
    EpRewMean, EpLenMean, vf_loss, entropy and kl (ITER_LOG_NAMES) and moves the policy / critic Standardizer two
    batches further, as self._V(x) and self.policy.distribution(x) do there; the six doubles are read back once,
    handed to sw.add_scalar(tag, value, iter // 3) after the discriminator's tags, and returned as iter_log (a dict
    tag -> value).  It needs sw, a policy_step with `policy` (a DeviceGaussianPolicy) and old_distribution() (DeviceTRPO),
    and a policy and critic sharing one Standardizer.  EpLenMean is NaN when the rollout completed no episode (the
    reference raises in int(np.round(nan))).  On other iterations nothing runs and the statistics do not move.

    `start_iter` (1) and critic_fit_params' default n_epochs (3) are readings of mushroom-rl's TRPO, whose source is
    not part of this project's reference: they are not verified facts, which is why both are arguments."""

    def __init__(self, engine, disc_reward, disc_trainer, critic, policy_step, gamma=0.99, lam=0.97,
                 env_reward_frac=0.0, train_D_n_th_epoch=3, critic_fit_params=None, start_iter=1, sw=None,
                 iteration_log=False):
        import inspect
        from .rollout import GAERollout
        if sw is not None:
            if not callable(getattr(sw, "add_scalar", None)):
                raise OlyError(f"{type(self).__name__}: sw must have add_scalar(tag, value, step) (a SummaryWriter)")
            if "log" not in inspect.signature(disc_trainer.fit).parameters:
                raise OlyError(f"{type(self).__name__}: sw needs a discriminator trainer whose fit takes log= (the "
                               f"device trainers), not {type(disc_trainer).__name__}")
        self.sw = sw
        self.iteration_log = bool(iteration_log)
        self._iter_ws = None
        if self.iteration_log:
            name = type(self).__name__
            if sw is None:
                raise OlyError(f"{name}: iteration_log=True needs sw (the writer _logging_sw's scalars go to)")
            pol = getattr(policy_step, "policy", None)
            if not isinstance(pol, DeviceGaussianPolicy) or not callable(getattr(policy_step, "old_distribution", None)):
                raise OlyError(f"{name}: iteration_log=True needs a policy_step with `policy` (a DeviceGaussianPolicy) "
                               f"and old_distribution() (DeviceTRPO), not {type(policy_step).__name__}")
            if pol.stand is not critic.stand:
                raise OlyError(f"{name}: iteration_log=True needs the policy and the critic to share one Standardizer "
                               "(trpo_standardizer, examples/imitation_learning/utils.py:123)")
        if not 0.0 <= env_reward_frac <= 1.0:
            raise ValueError("Environment reward must be between [0,1]")
        self.eng, self.disc, self.disc_trainer, self.critic = engine, disc_reward, disc_trainer, critic
        self.policy_step = policy_step
        self.frac = float(env_reward_frac)
        self.train_D_n_th_epoch = int(train_D_n_th_epoch)
        self.critic_fit_params = dict(n_epochs=3, batch_size=256) if critic_fit_params is None else dict(critic_fit_params)
        self.post = GAERollout(engine, gamma=gamma, lam=lam)
        self.iter = int(start_iter)
        if getattr(disc_reward, "pair", None) is not None and not isinstance(disc_trainer, DeviceDiscriminatorFit):
            raise OlyError(f"{type(self).__name__}: the reward was built with pair={disc_reward.pair!r}, which only the "
                           "device trainers fit (DeviceDiscriminatorTrainer, DeviceGAILDiscriminatorTrainer), not "
                           f"{type(disc_trainer).__name__}")

    @property
    def standardizer(self):
        return self.critic.stand

    # ---- checkpoint (il_checkpoint)
    def _header(self):
        """What a stored state must share with the agent it is loaded into (the first six), and what is kept for
        information only."""
        pol = getattr(self.policy_step, "policy", None)
        ds = self.disc._structure()
        return dict(kind="gail" if isinstance(self, GAILAgent) else "vail", in_dim=int(self.critic.in_dim),
                    out_dim=None if pol is None else int(pol.out_dim), disc_in_dim=ds["in_dim"], pair=ds["pair"],
                    state_mask=ds["state_mask"], gamma=float(self.post.gamma), lam=float(self.post.lam),
                    env_reward_frac=self.frac, train_D_n_th_epoch=self.train_D_n_th_epoch,
                    critic_fit_params={k: v for k, v in self.critic_fit_params.items()
                                       if isinstance(v, (int, float, str, bool, type(None)))})

    STRUCTURE = ("kind", "in_dim", "out_dim", "disc_in_dim", "pair", "state_mask")

    def state_dict(self):
        """Everything the agent carries from one fit to the next, as a nested dict of device clones, numbers, strings
        and None: `iter`, the critic, the policy (when the policy step has one), the discriminator with its own
        Standardizer, the discriminator trainer's optimiser, and the Standardizer the policy and the critic share,
        stored once.  The optimisers' hyper-parameters, the writer and the demonstrations are not state."""
        if not callable(getattr(self.disc_trainer, "state_dict", None)):
            raise OlyError(f"{type(self).__name__}.state_dict: {type(self.disc_trainer).__name__} has no state_dict (the "
                           "device trainers have)")
        pol = getattr(self.policy_step, "policy", None)
        d = dict(header=self._header(), iter=int(self.iter), standardizer=self.critic.stand.state_dict(),
                 critic=self.critic.state_dict(), policy=None, policy_standardizer=None,
                 disc=self.disc.state_dict(), disc_trainer=self.disc_trainer.state_dict())
        if pol is not None:
            d["policy"] = pol.state_dict()
            if pol.stand is not self.critic.stand:
                d["policy_standardizer"] = pol.stand.state_dict()
        return d

    def load_state_dict(self, d):
        """Write a stored state into this agent in place.  The structure is checked before anything is written: a
        mismatch raises OlyError naming the field and both values."""
        name = type(self).__name__
        own = self._header()
        for k in self.STRUCTURE:
            _same(name, k, d["header"].get(k), own[k])
        pol = getattr(self.policy_step, "policy", None)
        _same(name, "a stored policy", d["policy"] is not None, pol is not None)
        _same(name, "a separate policy Standardizer", d["policy_standardizer"] is not None,
              pol is not None and pol.stand is not self.critic.stand)
        self.critic.stand.load_state_dict(d["standardizer"])
        self.critic.load_state_dict(d["critic"])
        if pol is not None:
            if d["policy_standardizer"] is not None:
                pol.stand.load_state_dict(d["policy_standardizer"])
            pol.load_state_dict(d["policy"])
        self.disc.load_state_dict(d["disc"])
        self.disc_trainer.load_state_dict(d["disc_trainer"])
        if callable(getattr(self.policy_step, "load_state_dict", None)):
            self.policy_step.load_state_dict({})
        self.iter = int(d["iter"])

    def save(self, path, **meta):
        """il_checkpoint.save(path, self, **meta)."""
        from . import il_checkpoint
        il_checkpoint.save(path, self, **meta)

    def load(self, path):
        """il_checkpoint.load(path, self): this agent, built with its demonstrations like any other, takes the file's
        state; returns the file's meta."""
        from . import il_checkpoint
        return il_checkpoint.load(path, self)

    @staticmethod
    def _blocks(dataset):
        keys = ("state", "action", "reward", "next_state", "absorbing", "last")
        vals = [dataset[k] for k in keys] if isinstance(dataset, dict) else list(dataset)
        if len(vals) != 6:
            raise OlyError("VAILAgent.fit: dataset is (state, action, reward, next_state, absorbing, last)")
        if vals[0].dim() == 2:            # a flat mushroom dataset: the N = 1 case
            vals = [v.unsqueeze(1) for v in vals]
        return vals

    @torch.no_grad()
    def _advantage(self, x, xn, r_env, absorbing, last, eps=None, generator=None, second=None):
        from . import _abi
        from .rollout import RolloutBuffer
        T, N, D = x.shape
        flat = x.reshape(T * N, D)
        if self.frac < 1.0:
            if second is not None:      # a paired reward: (s, s') or (s, a), make_discrim_reward (gail_TRPO.py:320-325)
                r_disc = self.disc(flat, eps, generator=generator, x2=second).reshape(T, N)
            else:
                r_disc = self.disc(flat, eps, generator=generator).reshape(T, N)
            r = r_env * self.frac + r_disc * (1 - self.frac)
        else:
            r = r_env.clone()
        buf = RolloutBuffer(T, N, D, 1, x.device)
        buf.rewards.copy_(r)
        buf.values.copy_(self.critic(flat).reshape(T, N))
        buf.next_values.copy_(self.critic(xn.reshape(T * N, D).contiguous()).reshape(T, N))
        buf.flags.copy_((last.to(torch.uint8) * _abi.FLAG_LAST) | (absorbing.to(torch.uint8) * _abi.FLAG_ABSORBING))
        buf.ptr = T
        v_target, adv = self.post.finish(buf, normalize=True)
        return r, v_target, adv

    def fit(self, dataset, eps=None, generator=None):
        """One GAIL_TRPO.fit on [T,N,...] device blocks.  eps: the discriminator's reparameterisation noise [T*N, z]
        or None (drawn from `generator`).  Returns dict(reward, v_target, adv, critic_loss, disc_loss, disc_trained),
        and disc_log (with iteration_log=True also iter_log) on a trained iteration of an agent with a writer."""
        state, action, reward, next_state, absorbing, last = self._blocks(dataset)
        x = state.to(torch.float32).contiguous()
        xn = next_state.to(torch.float32).contiguous()
        T, N, D = x.shape
        flat = x.reshape(T * N, D)
        st = self.standardizer
        st.update_mean_std(flat)
        obs, act = flat, action.to(torch.float32).reshape(T * N, -1)
        pair = getattr(self.disc, "pair", None)      # what the discriminator looks at besides the states
        second = None if pair is None else (xn.reshape(T * N, D) if pair == "next_state" else act.contiguous())
        r, v_target, adv = self._advantage(x, xn, reward.to(torch.float32).reshape(T, N), absorbing.reshape(T, N),
                                           last.reshape(T, N), eps=eps, generator=generator, second=second)
        self.policy_step(obs, act, adv.reshape(T * N), self)
        fit = dict(self.critic_fit_params)
        for _ in range(int(fit.get("n_epochs", 3))):
            st.update_mean_std(flat)
        critic_loss = self.critic.fit(flat, v_target.reshape(T * N), n_epochs=int(fit.get("n_epochs", 3)),
                                      batch_size=int(fit.get("batch_size", 256)), generator=generator)
        disc_loss, trained, disc_log, iter_log = None, False, None, None
        if self.iter % self.train_D_n_th_epoch == 0:
            kw = dict(generator=generator)
            if second is not None:
                kw["x2"] = second
            if self.sw is not None:
                kw["log"] = True
            disc_loss = self.disc_trainer.fit(flat, **kw)
            if self.sw is not None:
                disc_loss, logs = disc_loss
                vals = logs.cpu().numpy()                           # the one read-back of the diagnostics
                names = getattr(self.disc_trainer, "log_names", DISC_LOG_NAMES["vail"])
                for row in vals:                                    # one _discriminator_logging per epoch, :220
                    for i, name in enumerate(names):
                        self.sw.add_scalar(name, float(row[i]), self.iter // 3)
                disc_log = {name: float(vals[-1][i]) for i, name in enumerate(names)}
            trained = True
            if self.iteration_log:                                  # _logging_sw, :163
                iter_log = self._logging_sw(flat, v_target.reshape(T * N), reward.reshape(T, N), r, last.reshape(T, N))
        self.iter += 1
        out = dict(reward=r, v_target=v_target, adv=adv, critic_loss=critic_loss, disc_loss=disc_loss,
                   disc_trained=trained)
        if disc_log is not None:
            out["disc_log"] = disc_log
        if iter_log is not None:
            out["iter_log"] = iter_log
        return out

    @torch.no_grad()
    def _logging_sw(self, flat, v_target, r_env, r, last):
        """_logging_sw (gail_TRPO.py:251-272) on K20: one call, one read-back, six add_scalar calls."""
        eng, pol = self.eng, self.policy_step.policy
        mu_old, ls_old = self.policy_step.old_distribution()
        n = int(flat.shape[0])
        if int(mu_old.shape[0]) != n:
            raise OlyError(f"{type(self).__name__}: old_distribution() holds {int(mu_old.shape[0])} rows, the batch {n}")
        if self._iter_ws is None or self._iter_ws[0] < n:
            self._iter_ws = (n, eng.iter_log_ws(n))
        r_env = r_env if r_env.dtype == torch.float64 else r_env.to(torch.float32)
        last = last if last.dtype in (torch.bool, torch.uint8) else last != 0
        vals = eng.iter_log(flat, v_target.to(torch.float32).contiguous(), mu_old, ls_old, pol.log_sigma,
                            self.critic.packed, pol.packed, r_env.contiguous(), r.to(torch.float32).contiguous(),
                            last.contiguous(), self.standardizer.colstats, self._iter_ws[1]).cpu().numpy()
        log = {name: float(vals[i]) for i, name in enumerate(ITER_LOG_NAMES)}
        for name in ITER_LOG_NAMES:
            self.sw.add_scalar(name, log[name], self.iter // 3)
        return log


class DeviceDiscriminatorFit:
    """What the two device trainers share, _fit_discriminator's (gail_TRPO.py:167-220) loop around one epoch call: the
    workspace, the demonstrations (for a reward built with a `pair`, their second array and the draw that selects both
    parts together), the flat parameters and Adam's moments, the epochs and the write-back.  A subclass names its
    Engine methods (FIT, LOG), its log_names, and supplies _check_policy, _begin, _epoch_args, _log_args and _end."""

    def __init__(self, reward, demo, lr, betas, eps, weight_decay, batch_size, n_epochs, use_noisy_targets):
        from .gail import ExpertDataset
        self.r, self.eng = reward, reward.eng
        self.in_dim = int(reward._params()[0].shape[1])
        self.batch = int(batch_size)
        self.pair = getattr(reward, "pair", None)
        self.lr, self.betas, self.eps, self.wd = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.n_epochs, self.noisy = int(n_epochs), bool(use_noisy_targets)
        dev = self.eng.device
        self.demo, self.demo2, self.expert = None, None, None
        if self.pair is not None:
            self._ws = getattr(self.eng, self.FIT + "_pair_ws")(self.batch, reward.ds, reward.d2, self.pair == "next_state")
            self._init_pair_demo(demo)
        else:
            self._ws = getattr(self.eng, self.FIT + "_ws")(self.batch, self.in_dim)
            if isinstance(demo, ExpertDataset):
                self.expert = demo
            else:
                self.demo = torch.as_tensor(np.asarray(demo), dtype=torch.float32, device=dev)
        n_par = sum(int(p.numel()) for p in reward._params())
        self.param = torch.empty(n_par, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros_like(self.param)
        self.exp_avg_sq = torch.zeros_like(self.param)
        self.step = 0
        self._log_ws = None

    def _init_pair_demo(self, demo):
        """The demonstrations of a paired fit: an ExpertDataset (next states: its minibatch(idx, want_next=True)) or a
        dict with the reference's keys, `states` and `next_states` or `actions` (gail_TRPO.py:177-194)."""
        from .gail import ExpertDataset
        r, dev = self.r, self.eng.device
        key = "next_states" if self.pair == "next_state" else "actions"
        if isinstance(demo, ExpertDataset):
            if self.pair != "next_state":
                raise OlyError(f"{type(self).__name__}: an ExpertDataset holds no actions; give a dict with "
                               "`states` and `actions`")
            if int(demo.cols.numel()) != r.ds:
                raise OlyError(f"{type(self).__name__}: the ExpertDataset has {int(demo.cols.numel())} masked "
                               f"columns, the states' part takes {r.ds}")
            self.expert = demo
            return
        if not isinstance(demo, dict) or "states" not in demo:
            raise OlyError(f"{type(self).__name__}: pair={self.pair!r} takes an ExpertDataset or a dict with "
                           f"`states` and `{key}`")
        if demo.get(key) is None:
            raise OlyError(f"{type(self).__name__}: the demonstrations lack `{key}` (pair={self.pair!r})")

        def up(a):
            return a.to(device=dev, dtype=torch.float32) if torch.is_tensor(a) else torch.as_tensor(
                np.asarray(a), dtype=torch.float32, device=dev)
        self.demo, self.demo2 = up(demo["states"]), up(demo[key])
        if self.demo.dim() != 2 or self.demo2.dim() != 2 or self.demo.shape[0] != self.demo2.shape[0]:
            raise OlyError(f"{type(self).__name__}: `states` and `{key}` are [rows, columns] with the same rows")
        r._check_pair(self.demo[:1], self.demo2[:1])

    def _demo_rows(self, n, generator):
        """The first min(n, rows) rows of a shuffle of the demonstrations, masked; for a pair (states, second): one
        draw selects both (gail_TRPO.py:178-180, 187-189)."""
        r = self.r
        rows = self.expert.rows if self.expert is not None else int(self.demo.shape[0])
        idx = torch.randperm(rows, generator=generator, device=self.eng.device)[:min(n, rows)]
        if self.expert is not None:
            return self.expert.minibatch(idx, want_next=True) if self.pair is not None else self.expert.minibatch(idx)
        d = self.demo[idx]
        d = d if r.mask is None else d[:, r.mask.long()]
        if self.pair is None:
            return d
        d2 = self.demo2[idx]
        return d, (d2 if r.mask2 is None else d2[:, r.mask2.long()])

    def _pair_policy_rows(self, plcy, x2):
        """The policy's second tensor, checked and masked."""
        r = self.r
        if x2 is None:
            raise OlyError(f"{type(self).__name__}.fit: pair={self.pair!r} needs the policy's second tensor (x2)")
        plcy2 = x2.reshape(-1, x2.shape[-1]).to(torch.float32)
        r._check_pair(plcy, plcy2)
        if r.mask2 is not None:
            plcy2 = plcy2[:, r.mask2.long()]
        return plcy2.contiguous()

    @torch.no_grad()
    def _fit(self, plcy_obs, generator, x2, log, eps=None, log_eps=None):
        """The fit both subclasses document; eps and log_eps reach _epoch_args and _log_args."""
        r, eng, dev = self.r, self.eng, self.eng.device
        plcy = plcy_obs.reshape(-1, plcy_obs.shape[-1]).to(torch.float32)
        n = int(plcy.shape[0])
        if n == 0:
            raise OlyError(f"{type(self).__name__}.fit: no policy rows")
        self._check_policy(plcy)
        plcy2 = self._pair_policy_rows(plcy, x2) if self.pair is not None else None
        if r.mask is not None:
            plcy = plcy[:, r.mask.long()]
        plcy = plcy.contiguous()
        ps = r._params()
        torch.cat([p.detach().reshape(-1).to(torch.float32) for p in ps], out=self.param)
        self._begin()
        if r._packed is None:
            r.packed()
        st = r.stand
        if getattr(st, "_fresh", False):     # the running sums start from zero; the fit adds to them in place
            st.colstats.zero_()
            st._fresh = False
        second = {}
        fit_epoch = getattr(eng, self.FIT + ("_epoch" if self.pair is None else "_epoch_pair"))
        losses = None
        logs = torch.zeros((self.n_epochs, _abi.OLY_DISC_LOG_SCALARS), dtype=torch.float64, device=dev) if log else None
        for e in range(self.n_epochs):
            demo = self._demo_rows(n, generator)
            xb = None
            if self.pair is not None:
                demo, demo2 = demo
                xb = torch.cat([plcy2, demo2]).contiguous()
                second = dict(x2=xb, standardise=self.pair == "next_state")
            x = torch.cat([plcy, demo]).contiguous()
            rows = int(x.shape[0])
            st.colstats = eng.col_stats(x, st.colstats)            # D_standardizer.update_mean_std(concat), :206: states only
            targets = None
            if self.noisy:                                          # :209-211: demo targets drawn first
                demo_t = torch.empty(n, device=dev).uniform_(0.80, 0.99, generator=generator)
                plcy_t = torch.empty(n, device=dev).uniform_(0.01, 0.10, generator=generator)
                targets = torch.cat([plcy_t, demo_t[:rows - n]]).contiguous()
            perm = torch.randperm(rows, generator=generator, device=dev).to(torch.int32)
            own = self._epoch_args(e, rows, generator, eps)
            nb = (rows + self.batch - 1) // self.batch
            if losses is None:
                losses = torch.empty((self.n_epochs, nb), dtype=torch.float64, device=dev)
            fit_epoch(x=x, n_plcy=n, perm=perm, batch=self.batch, colstats=st.colstats, param=self.param,
                      exp_avg=self.exp_avg, exp_avg_sq=self.exp_avg_sq, packed=r._packed, ws=self._ws, step=self.step,
                      lr=self.lr, beta1=self.betas[0], beta2=self.betas[1], adam_eps=self.eps, weight_decay=self.wd,
                      targets=targets, loss_out=losses[e], **second, **own)
            self.step += nb
            if log:                                                 # _discriminator_logging, :220
                own = self._log_args(e, rows, generator, log_eps)
                if self._log_ws is None or self._log_ws[0] < rows:
                    self._log_ws = (rows, getattr(eng, self.LOG + "_ws")(rows))
                getattr(eng, self.LOG)(x=x, n_plcy=n, colstats=st.colstats, packed=r._packed, ws=self._log_ws[1], x2=xb,
                                       standardise=self.pair == "next_state", targets=targets, out=logs[e], **own)
        o = 0
        for p in ps:                                                # in place: captured pointers stay valid
            k = int(p.numel())
            p.data.copy_(self.param[o:o + k].view_as(p))
            o += k
        r.invalidate()
        self._end()
        return (losses, logs) if log else losses

    def _begin(self):
        """Before the first epoch of a fit."""

    def _end(self):
        """After the write-back of a fit."""

    # ---- checkpoint (il_checkpoint): `param` is scratch, refilled at the start of every fit
    def state_dict(self):
        return dict(n_par=int(self.exp_avg.numel()), exp_avg=self.exp_avg.clone(), exp_avg_sq=self.exp_avg_sq.clone(),
                    step=int(self.step))

    @torch.no_grad()
    def load_state_dict(self, d):
        _same(type(self).__name__, "n_par", int(d["n_par"]), int(self.exp_avg.numel()))
        self.exp_avg.copy_(d["exp_avg"])
        self.exp_avg_sq.copy_(d["exp_avg_sq"])
        self.step = int(d["step"])


class DeviceDiscriminatorTrainer(DeviceDiscriminatorFit):
    """_fit_discriminator (gail_TRPO.py:167-220) for VAIL on K15: states only, or the paired input of a reward built
    with pair="next_state" / "action" (then fit takes the policy's second tensor, the demonstrations carry the second
    array, one draw selects both, and the explicit update of :206 still takes the states only).  Per epoch:

        plcy = plcy_obs[:, state_mask] (n rows); demo = the first m = min(n, rows) rows of a shuffle of the
        demonstration states (minibatch_generator, :198-200); concat = [plcy; demo]; targets 0 / 1, or
        U(0.01, 0.10) / U(0.80, 0.99) with use_noisy_targets
        D_standardizer.update_mean_std(concat)                                       (:206, oly_col_stats)
        mushroom's Regressor.fit over concat: a permutation cut into minibatches of batch_size, each
        Standardizer.forward, VariationalNet.forward, VDBLoss (beta's dual update), backward, Adam     (K15)

    Differences from the reference, all stated: the demo draw, the permutation, the noise and the noisy targets come
    from the caller's torch.Generator (the reference uses np.random and torch's global generator), drawn in that
    order per epoch; _discriminator_logging's extra forwards (:222-250), which update the statistics only when a
    SummaryWriter is attached, run with fit(log=True) (K19, oly_disc_log) and not otherwise: log=False is the
    reference's sw=None agent.

    reward: the DiscriminatorReward whose network (VariationalDiscriminator, the K12 shape) and standardizer are
    fitted; demo: an ExpertDataset (mask folded in) or an array of full observations (a paired reward: an ExpertDataset,
    whose minibatch(idx, want_next=True) serves the next states, or a dict with the reference's keys `states` and
    `next_states` / `actions`); loss: a VDBLoss, whose
    _beta is read at the start of every fit and written back once at its end.  Every fit starts from the module's
    current parameters and writes the stepped ones back in place (the pointers DiscriminatorReward.prepared()
    captured stay valid); the reward's packed stream is left current.  The optimiser's moments and step count
    persist across fits."""

    FIT, LOG, log_names = "disc_fit", "disc_log", DISC_LOG_NAMES["vail"]

    def __init__(self, reward, demo, loss, lr=5e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, batch_size=2048,
                 n_epochs=1, use_noisy_targets=False):
        from .gail import VariationalDiscriminator, VDBLoss
        if not isinstance(loss, VDBLoss):
            raise OlyError("DeviceDiscriminatorTrainer: loss must be a VDBLoss (the VAIL discriminator)")
        if loss._use_bernoulli_ent:
            raise OlyError("DeviceDiscriminatorTrainer: use_bernoulli_ent=True is refused: the reference adds an "
                           "unreduced tensor to the loss there (utils/math.py:64-68) and cannot run backward")
        if not isinstance(reward.net, VariationalDiscriminator) or not reward.fused:
            raise OlyError("DeviceDiscriminatorTrainer: supported network is VariationalDiscriminator "
                           "in <= 64 -> 256 -> 128 -> (mu, logvar) 128 -> 1")
        self.loss = loss
        super().__init__(reward, demo, lr, betas, eps, weight_decay, batch_size, n_epochs, use_noisy_targets)
        self._mask_max = None if reward.mask is None else int(reward.mask.max())
        self.beta = torch.empty(1, dtype=torch.float32, device=self.eng.device)

    def _check_policy(self, plcy):
        r, cols = self.r, int(plcy.shape[1])
        if self._mask_max is not None and cols <= self._mask_max:
            raise OlyError(f"DeviceDiscriminatorTrainer.fit: {cols} columns, the state mask reads column {self._mask_max}")
        masked = cols if r.mask is None else int(r.mask.numel())
        if masked != (self.in_dim if self.pair is None else r.ds):
            raise OlyError(f"DeviceDiscriminatorTrainer.fit: {masked} masked columns, the network takes {self.in_dim}")

    def _begin(self):
        self.beta.fill_(float(self.loss._beta))

    def _epoch_args(self, e, rows, generator, eps):
        if eps is None:
            noise = torch.randn((rows, 128), device=self.eng.device, generator=generator)
        else:
            noise = eps[e] if eps.dim() == 3 else eps
        return dict(eps=noise.to(torch.float32).contiguous(), beta=self.beta, info_constraint=self.loss._info_constr,
                    lr_beta=self.loss._lr_beta)

    def _log_args(self, e, rows, generator, log_eps):
        if log_eps is None:
            leps = torch.randn((4 * rows, 128), device=self.eng.device, generator=generator)
        else:
            leps = (log_eps[e] if log_eps.dim() == 3 else log_eps).to(torch.float32).contiguous()
        return dict(eps=leps, beta=self.beta, info_constraint=self.loss._info_constr, lr_beta=self.loss._lr_beta,
                    entcoeff=float(getattr(self.loss, "entcoeff", 1e-3)))

    def _end(self):
        self.loss._beta = float(self.beta)                           # the one host read-back of the call

    def fit(self, plcy_obs, generator=None, eps=None, x2=None, log=False, log_eps=None):
        """n_epochs epochs on the policy rows plcy_obs [n, obs] (full observations) and, for a paired reward, the
        policy's second tensor x2 [n, obs or act] (next states or actions, full width).  eps: the reparameterisation
        noise, [n_epochs, n + m, 128] (or [n + m, 128] for one epoch) in minibatch order, or None (drawn from
        `generator`).  Returns the per-minibatch losses, [n_epochs, n_batches] f64 on the device.

        log=True: _discriminator_logging (gail_TRPO.py:222-249, vail_TRPO.py:23-32) runs on the device right after
        each epoch's minibatch loop, where :220 puts it, so with n_epochs > 1 its seven forwards shift the next epoch's
        statistics; the return value is then (losses, logs), logs [n_epochs, 12] f64 on the device in
        DISC_LOG_NAMES["vail"]'s order.  The noise of forwards 1 .. 6 is log_eps [n_epochs, 4 (n + m), 128] (or
        [4 (n + m), 128]: all rows, demonstration half, policy half, twice), or drawn from `generator` after the epoch's
        other draws.  The halves split at the true boundary n; the reference splits at len // 2, which is the same
        whenever the reference runs at all (with fewer demonstrations than policy rows its target array no longer
        matches its inputs).  The copy of the loss the reference logs through takes beta's dual update between its
        three loss evaluations and is then dropped; that is reproduced, and the trainer's beta is not changed.  With
        log=False nothing differs from a trainer without diagnostics: same return value, statistics and bits."""
        return self._fit(plcy_obs, generator, x2, log, eps, log_eps)

    # ---- checkpoint (il_checkpoint): `beta` is scratch too, refilled from the loss at the start of every fit
    def state_dict(self):
        return dict(super().state_dict(), beta=float(self.loss._beta))

    def load_state_dict(self, d):
        super().load_state_dict(d)
        self.loss._beta = float(d["beta"])


class DeviceGAILDiscriminatorTrainer(DeviceDiscriminatorFit):
    """_fit_discriminator (gail_TRPO.py:167-220) for GAIL on K18: DeviceDiscriminatorTrainer's semantics with GAIL's
    network and loss, states only or the paired input of a reward built with pair="next_state" / "action".  Per epoch:

        plcy = plcy_obs[:, state_mask] (n rows); demo = the first m = min(n, rows) rows of a shuffle of the
        demonstration states (minibatch_generator, :198-200); concat = [plcy; demo]; targets 0 / 1, or
        U(0.01, 0.10) / U(0.80, 0.99) with use_noisy_targets
        D_standardizer.update_mean_std(concat)                                       (:206, oly_col_stats)
        mushroom's Regressor.fit over concat: a permutation cut into minibatches of batch_size, each
        Standardizer.forward, DiscriminatorNetwork.forward, GailDiscriminatorLoss(entcoeff), backward, Adam   (K18)

    The draws come from the caller's torch.Generator in the order demo, noisy targets (demo first), perm, per epoch;
    _discriminator_logging's extra forwards run with fit(log=True) (K19, oly_gail_disc_log; as
    DeviceDiscriminatorTrainer).  Defaults are
    HumanoidMuscle's of confs.yaml (lr_disc 5e-6, d_entr_coef 1e-3) and create_gail_agent's (weight_decay 0, batch 2048).

    reward: the GAILDiscriminatorReward whose network and standardizer are fitted; demo: an ExpertDataset (mask folded
    in) or an array of full observations (a paired reward: an ExpertDataset or a dict, as DeviceDiscriminatorTrainer).  Every fit starts from the module's current parameters and writes the stepped
    ones back in place; the reward's packed stream is left current.  The optimiser's moments and step count persist
    across fits."""

    FIT, LOG, log_names = "gail_disc_fit", "gail_disc_log", DISC_LOG_NAMES["gail"]

    def __init__(self, reward, demo, entcoeff=1e-3, lr=5e-6, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 batch_size=2048, n_epochs=1, use_noisy_targets=False):
        from .gail import GAILDiscriminatorReward
        if not isinstance(reward, GAILDiscriminatorReward):
            raise OlyError("DeviceGAILDiscriminatorTrainer: reward must be a GAILDiscriminatorReward "
                           "(in <= 64 -> 512 -> 256 -> 1, tanh)")
        self.entcoeff = float(entcoeff)
        super().__init__(reward, demo, lr, betas, eps, weight_decay, batch_size, n_epochs, use_noisy_targets)
        if self.pair is None and self.demo is not None and (self.demo.dim() != 2 or int(self.demo.shape[1]) <= (
                reward._mask_max if reward.mask is not None else self.in_dim - 1)):
            raise OlyError("DeviceGAILDiscriminatorTrainer: the demonstrations are [rows, obs] full observations")

    def _check_policy(self, plcy):
        if self.pair is None:
            self.r._check(plcy)

    def _epoch_args(self, e, rows, generator, eps):
        return dict(entcoeff=self.entcoeff)

    _log_args = _epoch_args

    def fit(self, plcy_obs, generator=None, x2=None, log=False):
        """n_epochs epochs on the policy rows plcy_obs [n, obs] (full observations) and, for a paired reward, the
        policy's second tensor x2 [n, obs or act] (next states or actions, full width).  Returns the per-minibatch
        losses, [n_epochs, n_batches] f64 on the device.

        log=True: _discriminator_logging (gail_TRPO.py:222-249) runs on the device right after each epoch's minibatch
        loop, where :220 puts it, so with n_epochs > 1 its six forwards shift the next epoch's statistics; the return
        value is then (losses, logs), logs [n_epochs, 12] f64 on the device, the first nine columns in
        DISC_LOG_NAMES["gail"]'s order and the rest 0.  The halves split at the true boundary n; the reference splits at
        len // 2, which is the same whenever the reference runs at all (with fewer demonstrations than policy rows its
        target array no longer matches its inputs).  With log=False nothing differs from a trainer without
        diagnostics: same return value, statistics and bits."""
        return self._fit(plcy_obs, generator, x2, log)


class GAILAgent(VAILAgent):
    """GAIL_TRPO.fit (gail_TRPO.py:105-165) for GAIL_TRPO: VAILAgent's sequence with GAIL's discriminator, i.e.
    disc_reward a GAILDiscriminatorReward (K18's forward) and disc_trainer a DeviceGAILDiscriminatorTrainer (K18's
    fit).  The discriminator draws no reparameterisation noise, so fit takes no eps."""

    def fit(self, dataset, generator=None):
        """One GAIL_TRPO.fit on [T,N,...] device blocks.  Returns dict(reward, v_target, adv, critic_loss, disc_loss,
        disc_trained), and disc_log on a trained iteration of an agent with a writer."""
        return super().fit(dataset, eps=None, generator=generator)


class DeviceGaussianPolicy:
    """GaussianTorchPolicy(FullyConnectedNetwork(in -> 512 -> 256 -> out, relu, relu, identity), std_0,
    standardizer=trpo_standardizer) (examples/imitation_learning/utils.py:126-134) held on the device: flat
    parameters theta in mushroom's order W1 | b1 | W2 | b2 | W3 | b3 | log_sigma and K16's packed stream of the mean
    network.  mushroom-rl's GaussianTorchPolicy is not part of the reference; this is a reading of mushroom-rl >= 1.10:
    log_sigma is state-independent, initialised to log(std_0), and distribution_t(s) = N(mu(s),
    diag(exp(log_sigma))^2).

    net: the reference's FullyConnectedNetwork (its `_linears`) or a list of its three nn.Linear layers; standardizer:
    the DeviceStandardizer shared with the critic.  Every forward that the reference runs through
    FullyConnectedNetwork.forward adds the rows to the statistics first (networks.py:68-81): draw_action and
    log_prob do; predict does not."""

    def __init__(self, engine, net, standardizer, std_0=1.0, log_sigma=None):
        lins = list(getattr(net, "_linears", net))
        if len(lins) != 3:
            raise OlyError(f"DeviceGaussianPolicy: expected three Linear layers, got {len(lins)}")
        self.eng, self.net, self.lins, self.stand = engine, net, lins, standardizer
        self.in_dim, self.out_dim = int(lins[0].in_features), int(lins[2].out_features)
        if (int(lins[0].out_features), int(lins[1].in_features), int(lins[1].out_features),
                int(lins[2].in_features)) != (_H1, _H1, _H2, _H2) or not 0 < self.in_dim <= 64 or not 0 < self.out_dim <= 32:
            raise OlyError("DeviceGaussianPolicy: supported shape is in <= 64 -> 512 -> 256 -> out <= 32")
        dev = engine.device
        if log_sigma is None:
            log_sigma = torch.full((self.out_dim,), float(np.log(std_0)), dtype=torch.float32)
        log_sigma = torch.as_tensor(log_sigma, dtype=torch.float32).reshape(-1)
        if int(log_sigma.numel()) != self.out_dim:
            raise OlyError(f"DeviceGaussianPolicy: log_sigma has {log_sigma.numel()} values for {self.out_dim} actions")
        with torch.no_grad():
            self.theta = torch.cat([t.detach().reshape(-1).to(device=dev, dtype=torch.float32)
                                    for lin in lins for t in (lin.weight, lin.bias)]
                                   + [log_sigma.to(dev)]).contiguous()
        self.packed = engine.ilmlp_pack(*self._views()[:6])

    def _views(self):
        shapes = [(_H1, self.in_dim), (_H1,), (_H2, _H1), (_H2,), (self.out_dim, _H2), (self.out_dim,), (self.out_dim,)]
        out, o = [], 0
        for s in shapes:
            n = int(np.prod(s))
            out.append(self.theta[o:o + n].view(s))
            o += n
        return out

    @property
    def log_sigma(self):
        return self._views()[6]

    @property
    def n_par(self):
        return int(self.theta.numel())

    def repack(self):
        """Re-pack the mean network after theta was written (set_weights does this)."""
        self.eng.ilmlp_pack(*self._views()[:6], packed=self.packed)

    @torch.no_grad()
    def predict(self, obs):
        """mu(obs) with the current statistics, without updating them (K16's forward)."""
        x = obs.reshape(-1, self.in_dim).to(torch.float32).contiguous()
        return self.eng.ilmlp_forward(x, self.packed, self.out_dim, "identity", colstats=self.stand.colstats)

    @torch.no_grad()
    def draw_action(self, obs, generator=None):
        """distribution_t(obs).sample(): the statistics take obs's rows, then mu(obs) + exp(log_sigma) eps."""
        x = obs.reshape(-1, self.in_dim).to(torch.float32).contiguous()
        self.stand.update_mean_std(x)
        mu = self.predict(x)
        eps = torch.randn(mu.shape, dtype=torch.float32, device=mu.device, generator=generator)
        return mu + torch.exp(self.log_sigma) * eps

    @torch.no_grad()
    def act(self, obs, generator=None, eps=None, deterministic=False, ctrl=False):
        """draw_action for the collection loop in one oly_il_act call (K21): the statistics take obs's rows, mu(obs) on
        the statistics after that, action = mu + exp(log_sigma) eps and, with ctrl=True, the engine's configured
        model's clamped control vector of that action.  eps None: drawn as draw_action draws it (the same generator
        state gives the same noise); deterministic=True: action = mu, nothing is drawn.  Returns (action [n,act],
        ctrl [n,nu] or None)."""
        x = obs.reshape(-1, self.in_dim).to(torch.float32).contiguous()
        st = self.stand
        if getattr(st, "_fresh", False):     # the running sums start from zero; the call adds to them in place
            st.colstats.zero_()
            st._fresh = False
        if deterministic:
            eps = None
        elif eps is None:
            eps = torch.randn((int(x.shape[0]), self.out_dim), dtype=torch.float32, device=x.device, generator=generator)
        log_sigma = self.theta[self.theta.numel() - self.out_dim:]      # the log_sigma property's view, without the others
        o = self.eng.il_act(x, self.packed, log_sigma, st.colstats, eps=eps, update_stats=True, want_ctrl=bool(ctrl))
        return o["action"], o["ctrl"]

    @torch.no_grad()
    def log_prob(self, obs, act):
        """log_prob_t(obs, act) [n,1]: the statistics take obs's rows (the forward), then the diagonal Gaussian's
        log-density as torch's MultivariateNormal forms it."""
        x = obs.reshape(-1, self.in_dim).to(torch.float32).contiguous()
        self.stand.update_mean_std(x)
        mu = self.predict(x)
        sigma = torch.exp(self.log_sigma)
        u = (act.reshape(mu.shape).to(torch.float32) - mu) / sigma
        lp = -0.5 * (self.out_dim * float(np.log(2 * np.pi)) + (u * u).sum(1)) - torch.log(sigma).sum()
        return lp[:, None]

    def entropy(self):
        """entropy_t: out/2 log(2 pi e) + sum(log_sigma) (no forward), a device scalar."""
        return 0.5 * self.out_dim * float(np.log(2 * np.pi * np.e)) + self.log_sigma.sum()

    def get_weights(self):
        """The flat parameters in mushroom's order (a device copy)."""
        return self.theta.clone()

    @torch.no_grad()
    def set_weights(self, w):
        w = torch.as_tensor(w, dtype=torch.float32, device=self.theta.device).reshape(-1)
        if int(w.numel()) != self.n_par:
            raise OlyError(f"DeviceGaussianPolicy.set_weights: {w.numel()} values for {self.n_par} parameters")
        self.theta.copy_(w)
        self.repack()

    @torch.no_grad()
    def sync_to_torch(self):
        """Write theta back into the wrapped Linear layers; returns (net, log_sigma as a host tensor)."""
        v = self._views()
        for i, lin in enumerate(self.lins):
            lin.weight.copy_(v[2 * i].to(lin.weight.device))
            lin.bias.copy_(v[2 * i + 1].to(lin.bias.device))
        return self.net, v[6].detach().cpu().clone()

    # ---- checkpoint (il_checkpoint); the shared Standardizer is the agent's to store
    def state_dict(self):
        return dict(in_dim=self.in_dim, out_dim=self.out_dim, theta=self.theta.clone())

    @torch.no_grad()
    def load_state_dict(self, d):
        """In place (theta and `packed` keep their pointers), then repack()."""
        _same("DeviceGaussianPolicy", "in_dim", int(d["in_dim"]), self.in_dim)
        _same("DeviceGaussianPolicy", "out_dim", int(d["out_dim"]), self.out_dim)
        self.theta.copy_(d["theta"])
        self.repack()


class DeviceTRPO:
    """TRPO's policy step (GAIL_TRPO.fit, gail_TRPO.py:131-149) on K17, one oly_trpo_step call, no host
    synchronisation.  Callable as VAILAgent's policy_step(obs, act, adv, agent).

    mushroom-rl's TRPO is not part of the reference: the step restates a READING of mushroom-rl >= 1.10 (DESIGN.md
    section 13).  cg_damping, cg_residual_tol and n_epochs_line_search default to GAIL's own defaults
    (gail_TRPO.py:30-32); max_kl, ent_coeff and n_epochs_cg come from confs.yaml (UnitreeH1: 5e-3, 1e-3, 25).
    accept_rule: "or" (accept when kl <= 1.5 max_kl or the surrogate did not drop, this reading of mushroom's
    _line_search) or "and" (both, as OpenAI baselines).

    After each call `last` holds the step's scalars, on the device (f64 [8]): prev_loss, CG iterations run, shs,
    accepted j (-1: theta_0 restored), kl and J of the last candidate evaluated, line-search iterations run, r.r."""

    SCALARS = ("prev_loss", "cg_iters", "shs", "accepted_j", "kl", "J", "ls_iters", "residual")

    def __init__(self, policy, max_kl, ent_coeff, n_epochs_cg, cg_damping=1e-1, cg_residual_tol=1e-10,
                 n_epochs_line_search=10, accept_rule="or"):
        if accept_rule not in ("or", "and"):
            raise OlyError(f"DeviceTRPO: accept_rule must be 'or' or 'and' (got {accept_rule!r})")
        self.policy, self.eng = policy, policy.eng
        self.kw = dict(max_kl=float(max_kl), ent_coeff=float(ent_coeff), n_epochs_cg=int(n_epochs_cg),
                       cg_damping=float(cg_damping), cg_residual_tol=float(cg_residual_tol),
                       n_epochs_line_search=int(n_epochs_line_search), accept_rule=accept_rule)
        self._ws = None
        self.last = None

    def old_distribution(self):
        """old_pol_dist of the last call (gail_TRPO.py:132-133) as (mu_old [n,act], log_sigma_old [act]): views into
        the step's workspace, valid until the next call; mu_old at the statistics it was computed with."""
        if self._ws is None or self.last is None:
            raise OlyError("DeviceTRPO.old_distribution: no step has run yet")
        pol = self.policy
        return self.eng.trpo_old_distribution(self._ws[1], self._ws[0], pol.in_dim, pol.out_dim)

    def scalars(self):
        """`last` read back to the host as a dict (one synchronisation)."""
        v = self.last.cpu().tolist()
        return dict(zip(self.SCALARS, v))

    def state_dict(self):
        """Nothing: the step carries no state from one call to the next."""
        return {}

    def load_state_dict(self, d):
        """After a load no step of this run has happened: old_distribution() raises as before the first one."""
        self.last = None

    @torch.no_grad()
    def __call__(self, obs, act, adv, agent=None):
        pol, eng = self.policy, self.eng
        x = obs.reshape(-1, pol.in_dim).to(torch.float32).contiguous()
        n = int(x.shape[0])
        a = act.reshape(n, -1).to(torch.float32).contiguous()
        ad = adv.reshape(n).to(torch.float32).contiguous()
        st = pol.stand
        if getattr(st, "_fresh", False):     # the running sums start from zero; the step adds to them in place
            st.colstats.zero_()
            st._fresh = False
        if self._ws is None or self._ws[0] != n:
            from ._ffi import lib
            nws = int(lib().oly_trpo_ws_floats(n, pol.in_dim, _H1, _H2, pol.out_dim))
            if nws < 0:
                raise OlyError(f"DeviceTRPO: unsupported n={n} / shape")
            self._ws = (n, torch.empty(nws, dtype=torch.float32, device=eng.device))
        self.last = eng.trpo_step(x, a, ad, st.colstats, pol.theta, packed=pol.packed, ws=self._ws[1], **self.kw)
        return self.last
