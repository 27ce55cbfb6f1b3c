"""The imitation-learning agent's fit (GAIL_TRPO.fit, imitation_lib/imitation/gail_TRPO.py:105-165) on the device.

  critic FullyConnectedNetwork(obs -> [512, 256] -> 1)     examples/imitation_learning/utils.py:136-149
      evaluation                                          -> DeviceILCritic.__call__ (K16, oly_ilmlp_forward)
      Regressor.fit (mushroom's minibatch loop + Adam)    -> DeviceILCritic.fit (K16, oly_il_critic_fit_epoch)
  discriminator reward, GAE, advantage normalisation      -> DiscriminatorReward (K12), GAERollout (K6 + K7)
  discriminator training                                  -> the caller's DiscriminatorTrainer (torch)
  TRPO's policy step                                      -> the caller's policy_step

The critic shares the policy's running Standardizer (trpo_standardizer, utils.py:123); every evaluation and every
fit minibatch adds its rows to it, as Standardizer.forward does (networks.py:68-81).
"""
import torch

from ._ffi import OlyError

_H1, _H2 = 512, 256


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

    `start_iter` (1) and critic_fit_params' default n_epochs (3) are readings of mushroom-rl's TRPO, whose source is
    not part of this project's reference: they are not verified facts, which is why both are arguments."""

    def __init__(self, engine, disc_reward, disc_trainer, critic, policy_step, gamma=0.99, lam=0.97,
                 env_reward_frac=0.0, train_D_n_th_epoch=3, critic_fit_params=None, start_iter=1):
        from .rollout import GAERollout
        if not 0.0 <= env_reward_frac <= 1.0:
            raise ValueError("Environment reward must be between [0,1]")
        self.eng, self.disc, self.disc_trainer, self.critic = engine, disc_reward, disc_trainer, critic
        self.policy_step = policy_step
        self.frac = float(env_reward_frac)
        self.train_D_n_th_epoch = int(train_D_n_th_epoch)
        self.critic_fit_params = dict(n_epochs=3, batch_size=256) if critic_fit_params is None else dict(critic_fit_params)
        self.post = GAERollout(engine, gamma=gamma, lam=lam)
        self.iter = int(start_iter)

    @property
    def standardizer(self):
        return self.critic.stand

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
    def _advantage(self, x, xn, r_env, absorbing, last, eps=None, generator=None):
        from . import _abi
        from .rollout import RolloutBuffer
        T, N, D = x.shape
        flat = x.reshape(T * N, D)
        if self.frac < 1.0:
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
        or None (drawn from `generator`).  Returns dict(reward, v_target, adv, critic_loss, disc_loss, disc_trained)."""
        state, action, reward, next_state, absorbing, last = self._blocks(dataset)
        x = state.to(torch.float32).contiguous()
        xn = next_state.to(torch.float32).contiguous()
        T, N, D = x.shape
        flat = x.reshape(T * N, D)
        st = self.standardizer
        st.update_mean_std(flat)
        r, v_target, adv = self._advantage(x, xn, reward.to(torch.float32).reshape(T, N), absorbing.reshape(T, N),
                                           last.reshape(T, N), eps=eps, generator=generator)
        obs, act = flat, action.to(torch.float32).reshape(T * N, -1)
        self.policy_step(obs, act, adv.reshape(T * N), self)
        fit = dict(self.critic_fit_params)
        for _ in range(int(fit.get("n_epochs", 3))):
            st.update_mean_std(flat)
        critic_loss = self.critic.fit(flat, v_target.reshape(T * N), n_epochs=int(fit.get("n_epochs", 3)),
                                      batch_size=int(fit.get("batch_size", 256)), generator=generator)
        disc_loss, trained = None, False
        if self.iter % self.train_D_n_th_epoch == 0:
            disc_loss = self.disc_trainer.fit(flat, generator=generator)
            trained = True
        self.iter += 1
        return dict(reward=r, v_target=v_target, adv=adv, critic_loss=critic_loss, disc_loss=disc_loss,
                    disc_trained=trained)
