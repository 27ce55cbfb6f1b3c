"""The imitation-learning launcher's loop around GAIL_TRPO.fit / VAIL_TRPO.fit
(examples/imitation_learning/experiment.py:51-65):

    core.learn(n_steps=..., n_steps_per_fit=...)      -> ILCore.learn
    dataset = core.evaluate(n_episodes=...)           -> ILCore.evaluate
    R_mean, J_mean, L -> Eval_R / Eval_J / Eval_L     -> the dict ILCore.evaluate returns

mushroom-rl's Core is not part of the reference tree: this is a READING of mushroom-rl >= 1.10's Core for N environments
stepped together.  Acting is one DeviceGaussianPolicy.act call (K21, oly_il_act) per vec step.
"""
import torch

from ._ffi import OlyError


class ILCore:
    """Core(agent, mdp) for a vec environment.

    The core touches only: env.num_envs, env.reset(env_mask=None) -> obs [N,D], env.reset_where(mask) -> obs [N,D]
    (a new tensor; device path only), env.step(actions, ctrl=None) ->
    (obs, reward, absorbing, info) with info["last"], env.info.horizon / .gamma; policy.act(obs, generator=, ctrl=) ->
    (action, ctrl or None); agent.fit(dataset, generator=); episode_stats(reward
    [T,N], last [T,N], gamma) -> [8] as il_agent.episode_stats (the default, on the environment's engine); for
    state_dict / load_state_dict also env.state_dict() / env.load_state_dict(d) and env.device.

    Differences from the reference's Core, all consequences of stepping N environments together:
      * n_steps / n_steps_per_fit count VEC steps: every environment contributes that many samples to a fit, so N = 1
        means what the reference means;
      * evaluate gives environment e a quota of n_episodes // N + (e < n_episodes % N) complete episodes; the reference
        runs its n_episodes one after the other in one environment;
      * environments past their quota keep stepping until the slowest one is done (their rows do not count), so they
        still add rows to the policy's running statistics, which the reference's single environment would not.
    device_reset selects how the ended episodes are reset.  True: env.reset_where(last) on every step, ONE launch (K22)
    that resets the environments whose flag is set; the host never reads the flags and runs ahead of the device.  False:
    one small device-to-host read per step asks whether any episode ended and env.reset(env_mask=last) is driven from
    the host.  None (default): the device path when the environment has reset_where and its physics declares
    device_state, the host path otherwise (with host physics every step synchronises anyway)."""

    def __init__(self, agent, env, policy, generator=None, episode_stats=None, device_reset=None):
        self.agent, self.env, self.policy, self.generator = agent, env, policy, generator
        able = hasattr(env, "reset_where") and bool(getattr(getattr(env, "physics", None), "device_state", False))
        if device_reset and not able:
            raise OlyError("ILCore: device_reset=True needs an environment with reset_where(mask) whose physics declares "
                           "device_state = True")
        self.device_reset = able if device_reset is None else bool(device_reset)
        if episode_stats is None:
            from .il_agent import episode_stats as _es
            eng = env.eng
            episode_stats = lambda reward, last, gamma: _es(eng, reward, last, gamma=gamma)   # noqa: E731
        self.episode_stats = episode_stats
        self._obs = None
        self.blocks = None      # the last fit's six blocks, `last` as the environment reported it

    # --------------------------------------------------------------------------------------------------- checkpoint
    def _cuda_index(self):
        dev = torch.device(getattr(self.env, "device", "cuda"))
        return torch.cuda.current_device() if dev.index is None else dev.index

    def state_dict(self):
        """What the loop carries besides the agent: the observation the next learn starts from (None: it resets), the
        environment's own state_dict and the state of the random stream the loop draws from.  With generator=None that
        stream is the device's global one (torch.cuda.get_rng_state): a run resumed from such a state continues
        exactly only if nobody else draws from the global generator in between."""
        if not callable(getattr(self.env, "state_dict", None)):
            raise OlyError(f"ILCore.state_dict: {type(self.env).__name__} has no state_dict")
        own = self.generator is not None
        rng = self.generator.get_state() if own else torch.cuda.get_rng_state(self._cuda_index())
        return dict(num_envs=int(self.env.num_envs), obs=None if self._obs is None else self._obs.clone(),
                    env=self.env.state_dict(), generator="own" if own else "global", generator_state=rng.clone())

    def load_state_dict(self, d):
        """The counterpart: the environment and the generator are written in place (the caller's torch.Generator object
        takes the stored state), the observation is a new tensor."""
        if int(d["num_envs"]) != int(self.env.num_envs):
            raise OlyError(f"ILCore.load_state_dict: num_envs is {int(d['num_envs'])} in the stored state, "
                           f"{int(self.env.num_envs)} in this core's environment")
        kind = "own" if self.generator is not None else "global"
        if d["generator"] != kind:
            raise OlyError(f"ILCore.load_state_dict: generator is {d['generator']!r} in the stored state, {kind!r} in this "
                           "core (own: a torch.Generator was passed; global: generator=None)")
        self.env.load_state_dict(d["env"])
        rng = d["generator_state"].cpu()
        if kind == "own":
            self.generator.set_state(rng)
        else:
            torch.cuda.set_rng_state(rng, self._cuda_index())
        obs = d["obs"]
        self._obs = None if obs is None else obs.to(getattr(self.env, "device", obs.device)).clone()
        self.blocks = None

    # ----------------------------------------------------------------------------------------------------- stepping
    def _needs_ctrl(self):
        return bool(getattr(getattr(self.env, "physics", None), "needs_ctrl", False))

    def _step(self, obs, needs_ctrl):
        """One vec step from `obs`: (action, reward, absorbing, last, next_obs before any reset, the current obs)."""
        action, ctrl = self.policy.act(obs, generator=self.generator, ctrl=needs_ctrl)
        nobs, reward, absorbing, info = self.env.step(action, ctrl=ctrl)
        last = info["last"]
        if self.device_reset:           # one launch, nothing read back
            cur = self.env.reset_where(last)
            return action, reward, absorbing, last, nobs, cur
        cur = nobs
        if bool(last.any()):            # the one read-back per step
            cur = self.env.reset(env_mask=last)
        return action, reward, absorbing, last, nobs, cur

    def learn(self, n_steps, n_steps_per_fit):
        """n_steps vec steps, agent.fit every n_steps_per_fit of them on the six [T,N,...] blocks state, action, reward,
        next_state, absorbing, last.  next_state[t] is the observation the step returned, BEFORE any reset; state[t+1]
        is the post-reset observation where last[t] is set.  The final row's `last` is set in the copy handed to fit
        (the GAE tail is the same either way, and the open episodes count as compute_J counts them).  The first call
        resets every environment, later calls continue the running episodes.  Returns the list of fit results."""
        T, total = int(n_steps_per_fit), int(n_steps)
        if T < 1 or total < 0 or total % T != 0:
            raise OlyError(f"ILCore.learn: n_steps={n_steps} is not a multiple of n_steps_per_fit={n_steps_per_fit}")
        N, needs_ctrl = int(self.env.num_envs), self._needs_ctrl()
        if self._obs is None:
            self._obs = self.env.reset()
        results = []
        for _ in range(total // T):
            obs = self._obs
            dev, D = obs.device, int(obs.shape[-1])
            state = torch.empty((T, N, D), dtype=torch.float32, device=dev)
            next_state = torch.empty((T, N, D), dtype=torch.float32, device=dev)
            reward = torch.empty((T, N), dtype=torch.float32, device=dev)
            absorbing = torch.empty((T, N), dtype=torch.bool, device=dev)
            last = torch.empty((T, N), dtype=torch.bool, device=dev)
            action = None
            for t in range(T):
                state[t] = obs
                a, r, ab, la, nobs, obs = self._step(obs, needs_ctrl)
                if action is None:
                    action = torch.empty((T,) + tuple(a.shape), dtype=torch.float32, device=dev)
                action[t], reward[t], absorbing[t], last[t], next_state[t] = a, r, ab, la, nobs
            self._obs = obs
            handed = last.clone()
            handed[-1] = True
            self.blocks = dict(state=state, action=action, reward=reward, next_state=next_state, absorbing=absorbing,
                                last=last)
            results.append(self.agent.fit(dict(self.blocks, last=handed), generator=self.generator))
        return results

    def evaluate(self, n_episodes, gamma=None, poll=32, return_blocks=False):
        """core.evaluate(n_episodes) and the launcher's three scalars: from a full reset, environment e runs
        q_e = n_episodes // N + (e < n_episodes % N) complete episodes with the stochastic policy (the statistics are
        updated, as in the reference, hence its "-stochastic" tags).  Rows of an environment past its quota get reward
        0 and last cleared, so each such column ends in one open zero-return episode; the means are therefore taken
        over the completed count: R_mean = sum of returns (gamma 1) / n_episodes, J_mean likewise with `gamma` (default
        env.info.gamma), L = sum of lengths / n_episodes.  Completion is checked every `poll` steps; at most
        max(q_e) * horizon steps run, since the horizon forces `last`.  Returns dict(R_mean, J_mean, L, n_episodes,
        n_steps), n_steps the counted samples (the reference's len(dataset)); with return_blocks also the [T,N] blocks
        dict(reward, last) as scored and (reward_raw, last_raw) as collected."""
        n_episodes, poll = int(n_episodes), max(1, int(poll))
        N, needs_ctrl = int(self.env.num_envs), self._needs_ctrl()
        if n_episodes < 1:
            raise OlyError(f"ILCore.evaluate: n_episodes={n_episodes}")
        if gamma is None:
            gamma = float(self.env.info.gamma)
        obs = self.env.reset()
        self._obs = None                # the next learn starts from a reset, as after the reference's evaluate
        dev = obs.device
        quota = torch.tensor([n_episodes // N + (e < n_episodes % N) for e in range(N)], dtype=torch.int64, device=dev)
        bound = (n_episodes // N + (n_episodes % N > 0)) * int(self.env.info.horizon)
        done = torch.zeros(N, dtype=torch.int64, device=dev)
        rewards, lasts = [], []
        for t in range(bound):
            _, r, _, la, _, obs = self._step(obs, needs_ctrl)
            rewards.append(r.to(torch.float32).clone())
            lasts.append(la.clone())
            done += la.to(torch.int64)
            if (t + 1) % poll == 0 and bool((done >= quota).all()):
                break
        reward_raw, last_raw = torch.stack(rewards), torch.stack(lasts)
        ended_before = torch.cumsum(last_raw.to(torch.int64), 0) - last_raw.to(torch.int64)
        keep = ended_before < quota[None, :]
        reward = torch.where(keep, reward_raw, torch.zeros_like(reward_raw)).contiguous()
        last = (last_raw & keep).contiguous()
        # rows after every quota was met score nothing; cutting them makes the result independent of `poll`
        live = keep.any(1)
        T = int(live.sum())
        reward, last = reward[:T].contiguous(), last[:T].contiguous()
        r1 = self.episode_stats(reward, last, 1.0).tolist()
        rg = self.episode_stats(reward, last, float(gamma)).tolist()
        if int(r1[4]) != n_episodes:
            raise OlyError(f"ILCore.evaluate: {int(r1[4])} complete episodes counted, {n_episodes} asked for")
        out = dict(R_mean=r1[5] / r1[4], J_mean=rg[5] / rg[4], L=r1[7] / r1[4], n_episodes=n_episodes, n_steps=int(r1[7]))
        if return_blocks:
            return out, dict(reward=reward, last=last, reward_raw=reward_raw, last_raw=last_raw)
        return out
