"""Offline LS-IQ on the device: LSIQ_Offline (imitation_lib/imitation/offline/lsiq_offline.py:9-210), the SAC-family agent
that trains from a demonstration file alone.

  LSIQ_Offline.fit_offline (:25-48)        -> DeviceLSIQOffline.fit_offline: per step the first batch_size entries of a
                                              fresh permutation of the demonstrations (DeviceIQLearn.draw_demo_idx),
                                              iq_update, _iter and policy.iter advance
  LSIQ_Offline.iq_update (:161-173)        -> DeviceLSIQOffline.iq_update: the Q update on every delay_Q-th iteration, the
                                              policy update on every delay_pi-th (no warm-up condition: there is no replay
                                              memory), the soft target update with the Q update (inside K26's call)
  LSIQ_Offline._lossQ (:50-159), logging_loss (:212-246), IQ_SAC.update_Q_function (iq_sac.py:421-429)
                                           -> DeviceLSIQOffline.update_Q_function: the policy passes are oly_sg_act calls
                                              (K25) in the reference's order, the rest ONE oly_iq_q_update call (K26) with
                                              plcy_loss_mode v0 and all_expert
  LSIQ_Offline.update_policy (:175-210)    -> DeviceLSIQOffline.update_policy: ONE oly_iq_pi_update call (K27) on all rows
                                              and the reference's logging passes

The reference class cannot run as written: it reads _Q_Q_multiplier, _abs_mult and _act_mask, which nothing in IQ_SAC or
LSIQ sets.  This restatement takes the neutral reading _Q_Q_multiplier = 1.0 and _abs_mult = 1.0 (both exact in float32:
every product with them returns its other operand's bits) and refuses other values.  Under it _lossQ is LSIQ's iq_like loss
with plcy_loss_mode v0 on a batch of expert rows alone, the target clip always on (:62 has no target_clipping switch) and
the absorbing-state weighting of the chi2 term always on (:114-120 have no treat_absorbing_states switch), which is K26's
treat_absorbing arithmetic.  _act_mask is only asserted non-empty: the demonstrations must have actions, as they must here.

The policy passes of one logging iteration, each a fresh draw that feeds the policy's Standardizer, in order: next_obs
(getV / get_targetV); draw_action(obs) of logging_loss; getV(obs); getV(obs[is_expert]) for v0; update_policy's training
pass on obs; its logging pass on obs; get_mu_log_sigma(obs[~is_expert]), which has no rows (nothing is launched, the
Standardizer takes zero rows, the two policy-states scalars are NaN as torch's mean of nothing); get_mu_log_sigma(obs).

Still refused: the regularizer modes plcy (no policy rows), value and exp_and_plcy_and_value (further critic passes), the
gradient penalty, train_policy_only_on_own_states (no own states), IQ_Offline and LSIQ_Offline_DM.

Of logging_loss's scalars the per-action-dimension ones ("All Actions ...") are left out, as in olympic_hip.iq."""
import torch

from . import _abi
from ._ffi import OlyError
from .iq import FOLLOW_UP, DeviceLSIQ, _PolicySide

# the scalars of K26's block that logging_loss and update_Q_function log offline (lsiq_offline.py:87, 157, 215-229)
_OFFLINE_SLOTS = (3, 4, 5, 9, 11, 13, 14, 15)


class DeviceLSIQOffline(_PolicySide, DeviceLSIQ):
    """LSIQ_Offline whole.  policy, critic, demonstrations, gamma, batch_size, use_target, Q_max, Q_min, reg_mult,
    actor_optimizer, delay_pi, delay_Q, learnable_alpha, lr_alpha, target_entropy, init_alpha, logging_iter, state_mask and
    sw are DeviceLSIQSAC's; loss_mode_exp defaults to "fix" and regularizer_mode to "off" as the reference's constructor
    has them.  A batch is batch_size demonstration rows (at least 2, the kernel's smallest batch)."""

    KIND = "lsiq_offline"

    def __init__(self, engine, policy, critic, demonstrations, gamma, batch_size, use_target, Q_max=1.0, Q_min=-1.0,
                 loss_mode_exp="fix", Q_exp_loss=None, regularizer_mode="off", plcy_loss_mode="v0", Q_Q_multiplier=1.0,
                 abs_mult=1.0, gradient_penalty_lambda=0.0, train_policy_only_on_own_states=False, **kw):
        who = type(self).__name__
        if plcy_loss_mode != "v0":
            raise OlyError(f"{who}: this is the offline implementation of LS-IQ, which expects plcy_loss_mode='v0'")
        if float(Q_Q_multiplier) != 1.0 or float(abs_mult) != 1.0:
            raise OlyError(f"{who}: Q_Q_multiplier={Q_Q_multiplier} and abs_mult={abs_mult} must be 1.0: the reference sets "
                           "neither, and 1.0 is the reading built here")
        if regularizer_mode in ("value", "exp_and_plcy_and_value"):
            raise OlyError(f"{who}: regularizer_mode {regularizer_mode!r} is not built (further critic passes): {FOLLOW_UP}")
        if regularizer_mode == "plcy":
            raise OlyError(f"{who}: regularizer_mode 'plcy' averages over policy rows, and an offline batch has none")
        if float(gradient_penalty_lambda) > 0.0:
            raise OlyError(f"{who}: gradient_penalty_lambda > 0 is not built (a second-order pass through the critic): "
                           f"{FOLLOW_UP}")
        if train_policy_only_on_own_states:
            raise OlyError(f"{who}: train_policy_only_on_own_states: an offline batch has no states of the policy's own")
        for refused in ("treat_absorbing_states", "target_clipping", "lossQ_type", "warmup_transitions", "n_fits",
                        "initial_replay_size", "max_replay_size"):
            if refused in kw:
                raise OlyError(f"{who}: {refused} is not a keyword of the offline agent (its loss has no such switch and it "
                               "has no replay memory)")
        if int(batch_size) < 2:
            raise OlyError(f"{who}: batch_size={batch_size}: a batch has at least 2 rows")
        # the parent's constructor refuses v0, which its update cannot run; this class's update can
        super().__init__(engine, policy, critic, demonstrations, gamma, batch_size, use_target, Q_max=Q_max, Q_min=Q_min,
                         loss_mode_exp=loss_mode_exp, Q_exp_loss=Q_exp_loss, treat_absorbing_states=True, target_clipping=True,
                         lossQ_type="iq_like", plcy_loss_mode="off", regularizer_mode=regularizer_mode, max_replay_size=1,
                         **kw)
        self.plcy_loss_mode = "v0"
        self.MODES = ("v0",)

    # ---- the critic
    @torch.no_grad()
    def update_Q_function(self, obs, act, next_obs, absorbing, eps=None, generator=None):
        """update_Q_function with _lossQ, and the soft target update, on a batch of expert rows.  eps: None (the noise is
        drawn from `generator` pass by pass) or a dict with `next`, `pi`, `v0` [B,A] and, on a logging iteration, `expert`
        [B,A].  Returns the [16] f64 device block of _abi.IQ_Q_TAGS (the policy subset's slots are NaN); on a logging
        iteration the reference's scalars also go to sw."""
        batch = obs, act, next_obs, absorbing = self._batch(obs, act, next_obs, absorbing)
        eps = eps or {}
        logging = self._iter % self.logging_iter == 0
        c = self.critic
        a_next, lp_next = self._policy_pass(next_obs, eps.get("next"), generator)
        a_exp = None
        if logging:      # logging_loss's draw_action(obs[is_expert])
            a_exp = self._policy_pass(obs, eps.get("expert"), generator, want_log_prob=False)[0]
        a_pi, lp_pi = self._policy_pass(obs, eps.get("pi"), generator)          # getV(obs)
        a_v0, lp_v0 = self._policy_pass(obs, eps.get("v0"), generator)          # getV(obs[is_expert])
        w_norm = torch.linalg.vector_norm(c.param.double()) if logging and self.sw is not None else None
        out = self._net_update(c, batch, a_next, lp_next, a_pi, lp_pi, 0, self.use_target, algo="lsiq", plcy_loss_mode="v0",
                               regularizer_mode=self.regularizer_mode, treat_absorbing=True, update_target=True,
                               alpha=self.alpha, tau=c.tau, v0=(a_v0, lp_v0), all_expert=True, **self._algo_block())
        if logging and self.sw is not None:
            host, it, sw, tags = out.cpu().numpy(), self._iter, self.sw, _abi.IQ_Q_TAGS
            for k in (0, 1, 2):
                sw.add_scalar(tags[k], float(host[k]), it)
            sw.add_scalar("IQ-Loss/Alpha", self.alpha, it)
            for k in _OFFLINE_SLOTS:
                sw.add_scalar(tags[k], float(host[k]), it)
            sw.add_scalar("Action-Value/Norm of Q net: ", float(w_norm), it)
            sw.add_scalar("Actions/mean squared action expert (from data)", float(torch.square(act).mean()), it)
            sw.add_scalar("Actions/mean squared action expert (from policy)", float(torch.square(a_exp).mean()), it)
        return out

    # ---- the policy
    @torch.no_grad()
    def update_policy(self, obs, eps=None, generator=None):
        """LSIQ_Offline.update_policy on a batch of expert rows: one oly_iq_pi_update on all rows; on a logging iteration
        the logging pass on all rows with the stepped weights, then get_mu_log_sigma on the policy's rows, of which there
        are none, then on all rows; with learnable_alpha _update_alpha last, on a logging iteration with the logging
        pass's log-probabilities.  eps: None or a dict with `pi` [B,A] and, on a logging iteration, `log` [B,A].  Returns
        the [4] f64 device block of _abi.IQ_PI_TAGS."""
        obs = obs.to(torch.float32).contiguous()
        B = int(obs.shape[0])
        eps = eps or {}
        logging = self._iter % self.logging_iter == 0
        c, p = self.critic, self.policy
        noise = p._noise(B, eps.get("pi"), generator).contiguous()
        cs, ccs = p._colstats(), c._colstats(c.stand)
        o = self.eng.iq_pi_update(obs, noise, p.central, p.delta, cs, p.param, self.pi_exp_avg, self.pi_exp_avg_sq, p.packed,
                                  c.packed, c.param, ccs, self._pi_workspace(B), self.pi_step, self.pi_lr, alpha=self.alpha,
                                  log_std_min=p.log_std_min, log_std_max=p.log_std_max, beta1=self.pi_betas[0],
                                  beta2=self.pi_betas[1], adam_eps=self.pi_eps, weight_decay=self.pi_weight_decay, h=None)
        self.pi_step += 1
        if cs is not None:
            p.stand._fresh = False
        if ccs is not None:
            c.stand._fresh = False
        log_prob = o["log_prob"]
        if logging:
            _, log_prob = self._policy_pass(obs, eps.get("log"), generator)
            # get_mu_log_sigma(input_states[~is_expert]): zero rows, nothing to launch, the statistics gain nothing
            e_lb = self.get_e_lb()
            ls_e = p.get_mu_log_sigma(obs)[1]
            if self.sw is not None:
                host, it, sw = o["out"].cpu().numpy(), self._iter, self.sw
                sw.add_scalar(_abi.IQ_PI_TAGS[1], float(host[1]), it)
                sw.add_scalar(_abi.IQ_PI_TAGS[0], float(host[0]), it)
                sw.add_scalar("Actor/Entropy Expert States", float(torch.mean(-log_prob)), it)
                sw.add_scalar("Actor/Entropy Policy States", float("nan"), it)
                sw.add_scalar("Actor/Entropy from Gaussian Policy States", float("nan"), it)
                sw.add_scalar("Actor/Entropy Lower Bound", float(e_lb), it)
                sw.add_scalar("Actor/Entropy from Gaussian Expert States", float(torch.mean(p.entropy_from_logsigma(ls_e))), it)
        if self.learnable_alpha:
            self.eng.iq_alpha_update(log_prob.contiguous(), self.alpha_state, self.alpha_step, self.lr_alpha,
                                     self.target_entropy)
            self.alpha_step += 1
            self._alpha_read = False
        return o["out"]

    @torch.no_grad()
    def iq_update(self, obs, act, next_obs, absorbing, eps=None, generator=None):
        """LSIQ_Offline.iq_update: update_Q_function on every delay_Q-th iteration, update_policy on every delay_pi-th.
        The target update runs inside the critic's call (K26), before the policy update instead of after it: the policy
        update neither reads nor writes the target.  eps: None or dict(q=update_Q_function's, pi=update_policy's).
        Returns (the critic's scalars or None, the policy's or None)."""
        eps = eps or {}
        out_q = out_pi = None
        if self._iter % self.delay_Q == 0:
            out_q = self.update_Q_function(obs, act, next_obs, absorbing, eps=eps.get("q"), generator=generator)
        if self._iter % self.delay_pi == 0:
            out_pi = self.update_policy(obs, eps=eps.get("pi"), generator=generator)
        return out_q, out_pi

    def fit(self, dataset, generator=None):
        raise OlyError("DeviceLSIQOffline: this is the offline implementation of LS-IQ; use fit_offline, not fit")

    fit_Q = fit

    @torch.no_grad()
    def fit_offline(self, n_steps, generator=None):
        """n_steps times: the first batch_size entries of a fresh permutation of the demonstrations, iq_update, _iter and
        policy.iter advance.  Returns the last iq_update's pair that was not None each, or (None, None)."""
        d = self.demo
        last_q = last_pi = None
        for _ in range(int(n_steps)):
            idx = self.draw_demo_idx(self.batch_size, generator)
            if int(idx.numel()) < 2:
                raise OlyError("DeviceLSIQOffline.fit_offline: the demonstrations hold fewer than 2 rows")
            out_q, out_pi = self.iq_update(d["states"][idx], d["actions"][idx], d["next_states"][idx], d["absorbing"][idx],
                                           generator=generator)
            last_q = last_q if out_q is None else out_q
            last_pi = last_pi if out_pi is None else out_pi
            self._iter += 1
            self.policy.iter = getattr(self.policy, "iter", 0) + 1
        return last_q, last_pi


__all__ = ["DeviceLSIQOffline"]
