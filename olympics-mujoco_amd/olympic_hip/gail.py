"""Discriminator reward of GAIL / VAIL with the reference's semantics.

  Standardizer                 imitation_lib/utils/networks.py:48-81   -> DeviceStandardizer
  VariationalNet.forward       networks.py:258-284                     -> VariationalDiscriminator
  GAIL.make_discrim_reward     imitation_lib/imitation/gail_TRPO.py:320-327
  prepare_discrim_inputs       gail_TRPO.py:297-313 (state mask)

The reward path (mask + standardise, 32->256->128->(128,128)->1 for UnitreeH1, examples/
imitation_learning/utils.py:151-161, reparameterisation, reward formula) is ONE launch on the f32
matrix cores (K12, oly_disc_forward) after the statistics update (oly_col_stats); the statistics
live on the device (no CPU bounce as in networks.py:70).  GAIL's own discriminator (DiscriminatorNetwork,
networks.py:194-225: in -> 512 -> 256 -> 1, tanh) is GAILDiscriminator / GAILDiscriminatorReward on K18
(oly_gail_reward_step).  The device fits are il_agent's trainers; DiscriminatorTrainer here is the
torch reading.  The reparameterisation noise is an INPUT so results are
reproducible.
"""
import numpy as np
import torch
import torch.nn as nn


class DeviceStandardizer:
    """Running (count, sum, sumsq) per column on the device; mean/std as the reference
    derives them (_sum=0, _sumsq=1e-2, _count=1e-2, variance floor 1e-2)."""

    def __init__(self, engine, dim):
        self.eng, self.dim = engine, dim
        self.colstats = torch.zeros((3, dim), dtype=torch.float64, device=engine.device)
        self._fresh = True

    def update_mean_std(self, x):
        self.colstats = self.eng.col_stats(x, None if self._fresh else self.colstats)
        self._fresh = False

    @property
    def mean(self):
        return self.colstats[1] / (self.colstats[0] + 1e-2)

    @property
    def std(self):
        cnt = self.colstats[0] + 1e-2
        mean = self.colstats[1] / cnt
        return torch.sqrt(torch.clamp((self.colstats[2] + 1e-2) / cnt - mean * mean, min=1e-2))

    def forward(self, x, mask=None):
        """Updates the statistics with x (as Standardizer.forward does on EVERY call), then
        returns the masked, standardised float32 batch."""
        xm = x if mask is None else x[:, mask.long()].contiguous()
        self.update_mean_std(xm)
        return self.eng.disc_standardize(x, mask, self.mean.contiguous(), self.std.contiguous())

    # ---- checkpoint (il_checkpoint)
    def state_dict(self):
        return dict(dim=int(self.dim), colstats=self.colstats.clone(), fresh=bool(self._fresh))

    @torch.no_grad()
    def load_state_dict(self, d):
        """In place: `colstats` keeps its pointer (a prepared reward step or a launch cache may hold it)."""
        _same("DeviceStandardizer", "dim", int(d["dim"]), int(self.dim))
        self.colstats.copy_(d["colstats"])
        self._fresh = bool(d["fresh"])


def _same(who, field, stored, own):
    """A structural field of a loaded state must be the built object's."""
    if stored != own:
        from ._ffi import OlyError
        raise OlyError(f"{who}.load_state_dict: {field} is {stored!r} in the stored state, {own!r} in this object")


def _mask_list(m):
    return None if m is None else [int(v) for v in m.detach().cpu().reshape(-1).tolist()]


class DiscriminatorState:
    """state_dict / load_state_dict of the two discriminator rewards: the network's parameters and the Standardizer."""

    def _structure(self):
        return dict(kind=type(self).__name__, in_dim=int(self._params()[0].shape[1]), pair=self.pair,
                    state_mask=_mask_list(self.mask), act_mask=_mask_list(getattr(self, "mask2", None)))

    def state_dict(self):
        return dict(self._structure(), params=[p.detach().clone() for p in self._params()],
                    standardizer=self.stand.state_dict())

    @torch.no_grad()
    def load_state_dict(self, d):
        """The parameters are copied into the module's own tensors (the pointers a prepared step captured stay valid),
        the Standardizer in place; then the packed stream is formed again so that the next reward call sees them."""
        who = type(self).__name__
        for k, v in self._structure().items():
            _same(who, k, d[k], v)
        ps = self._params()
        _same(who, "number of parameters", len(d["params"]), len(ps))
        for i, (p, t) in enumerate(zip(ps, d["params"])):
            _same(who, f"shape of parameter {i}", tuple(t.shape), tuple(p.shape))
        for p, t in zip(ps, d["params"]):
            p.data.copy_(t)
        self.stand.load_state_dict(d["standardizer"])
        self.invalidate()
        if self._packed is not None:
            self.packed()


class VariationalDiscriminator(nn.Module):
    """encoder -> (mu, logvar) -> z = mu + exp(logvar/2) eps -> decoder."""

    def __init__(self, in_dim=32, enc_features=(256,), enc_out=128, z_size=128):
        super().__init__()
        dims = [in_dim] + list(enc_features) + [enc_out]
        self.encoder = nn.ModuleList([nn.Linear(dims[i], dims[i + 1]) for i in range(len(dims) - 1)])
        self.mu_out = nn.Linear(enc_out, z_size)
        self.logvar_out = nn.Linear(enc_out, z_size)
        self.decoder = nn.Linear(z_size, 1)

    def load_reference_arrays(self, g):
        """Weights in the layout gen_golden.py saves (state_dict of the reference network)."""
        with torch.no_grad():
            for lin, w, b in ((self.encoder[0], "enc_w0", "enc_b0"), (self.encoder[1], "enc_w1", "enc_b1"),
                              (self.mu_out, "mu_w", "mu_b"), (self.logvar_out, "lv_w", "lv_b"),
                              (self.decoder, "dec_w", "dec_b")):
                lin.weight.copy_(torch.as_tensor(np.asarray(g[w])))
                lin.bias.copy_(torch.as_tensor(np.asarray(g[b])))
        return self

    def encode(self, xs):
        h = xs
        for lin in self.encoder:
            h = torch.relu(lin(h))
        return self.mu_out(h), self.logvar_out(h)


class PairedInput:
    """What DiscriminatorReward and GAILDiscriminatorReward share when built with a `pair`: the widths and masks of
    [ s[:, state_mask] | second ] and the checks of the two tensors."""

    def _init_pair(self, dim, state_mask, act_mask, standardizer):
        """The widths and masks of a paired input: Ds state columns, D2 of the second part, Ds + D2 = the network's."""
        from ._ffi import OlyError
        self.mask, self.mask2, self._mask_max, self._mask2_max = pair_masks(
            type(self).__name__, self.pair, dim, state_mask, act_mask, self.eng.device)
        self.ds = int(self.mask.numel()) if self.mask is not None else (dim // 2 if self.pair == "next_state" else
                                                                        dim - int(self.mask2.numel()))
        self.d2 = dim - self.ds
        self.stand = standardizer or DeviceStandardizer(self.eng, self.ds)
        if not isinstance(self.stand, DeviceStandardizer):
            raise OlyError(f"{type(self).__name__}: pair={self.pair!r} takes a DeviceStandardizer (its running sums are "
                           f"updated inside the reward's call), not {type(self.stand).__name__}")
        if tuple(self.stand.colstats.shape) != (3, self.ds):
            raise OlyError(f"{type(self).__name__}: the standardizer has {self.stand.colstats.shape[1]} columns, the "
                           f"states {self.ds}")
        self._stats_a = torch.zeros((3, self.ds), dtype=torch.float64, device=self.eng.device)   # S1 of a forward
        self._packed = None

    def _check_pair(self, x, x2):
        from ._ffi import OlyError
        self._check_first(x)
        if x2 is None:
            raise OlyError(f"{type(self).__name__}: pair={self.pair!r} needs the second tensor (x2)")
        if x2.dim() != 2 or int(x2.shape[0]) != int(x.shape[0]):
            raise OlyError(f"{type(self).__name__}: x2 is [B, columns] with x's {x.shape[0]} rows")
        if self.mask2 is None and int(x2.shape[1]) != self.d2:
            raise OlyError(f"{type(self).__name__}: x2 has {x2.shape[1]} columns, the second part {self.d2}")
        if self.mask2 is not None and int(x2.shape[1]) <= self._mask2_max:
            raise OlyError(f"{type(self).__name__}: x2 has {x2.shape[1]} columns, its mask reads column {self._mask2_max}")

    def _check_first(self, x):
        from ._ffi import OlyError
        if x.dim() != 2:
            raise OlyError(f"{type(self).__name__}: x is [B, obs]")
        if self.mask is None and int(x.shape[1]) != self.ds:
            raise OlyError(f"{type(self).__name__}: {x.shape[1]} columns, the states' part takes {self.ds}")
        if self.mask is not None and int(x.shape[1]) <= self._mask_max:
            raise OlyError(f"{type(self).__name__}: {x.shape[1]} columns, the state mask reads column {self._mask_max}")


class DiscriminatorReward(PairedInput, DiscriminatorState):
    """make_discrim_reward for a batch of observations on the device.

    pair: what the discriminator looks at besides the states (VariationalNet.forward, networks.py:258-278;
    prepare_discrim_inputs, gail_TRPO.py:297-313), as GAILDiscriminatorReward documents it: None (states only),
    "next_state" ([standardise(s) | standardise(s')], two Standardizer updates per forward) or "action"
    ([standardise(s) | a[:, act_mask]]).  forward / prepared / logits / __call__ then take the second tensor as x2; the
    paired path is the fused network's (K12) only."""

    def __init__(self, engine, net, state_mask=None, standardizer=None, pair=None, act_mask=None):
        self.eng, self.net = engine, net
        self.pair = pair
        if pair is not None:
            from ._ffi import OlyError
            self._packed, self._packed_ver = None, None
            if not self.fused:
                raise OlyError("DiscriminatorReward: a paired input needs the fused network "
                               "in <= 64 -> 256 -> 128 -> (mu, logvar) 128 -> 1")
            self._init_pair(int(net.encoder[0].in_features), state_mask, act_mask, standardizer)
            return
        if act_mask is not None and np.asarray(act_mask).size:
            from ._ffi import OlyError
            raise OlyError("DiscriminatorReward: an act_mask needs pair='action'")
        self.mask = None if state_mask is None else torch.as_tensor(np.asarray(state_mask, dtype=np.int32),
                                                                   device=engine.device)
        dim = net.encoder[0].in_features
        self.stand = standardizer or DeviceStandardizer(engine, dim)
        self._packed, self._packed_ver = None, None
        self._identity_mask = state_mask is not None and np.array_equal(np.asarray(state_mask), np.arange(dim))

    # ---- fused path (K12)
    def _params(self):
        n = self.net
        return [n.encoder[0].weight, n.encoder[0].bias, n.encoder[1].weight, n.encoder[1].bias, n.mu_out.weight,
                n.mu_out.bias, n.logvar_out.weight, n.logvar_out.bias, n.decoder.weight, n.decoder.bias]

    @property
    def fused(self):
        n = self.net
        return (len(n.encoder) == 2 and n.encoder[0].in_features <= 64 and n.encoder[0].out_features == 256
                and n.encoder[1].out_features == 128 and n.mu_out.out_features == 128)

    def packed(self):
        """The MFMA operand stream of the CURRENT weights: re-packed on every call (one ~6 us launch into the same
        buffer), as FusedMLPForward.refresh() does per rollout.  A cache keyed on (data_ptr, _version) would miss writes
        through `.data` (dist.broadcast_parameters, load paths that copy into p.data): `_version` does not move for
        those, and the reward would silently keep the old weights.  `cache_packed = True` opts into that cache for
        callers that own every write to the parameters (benchmarks of a frozen network)."""
        ps = self._params()
        if getattr(self, "cache_packed", False):
            ver = tuple((p.data_ptr(), p._version) for p in ps)
            if ver == self._packed_ver and self._packed is not None:
                return self._packed
            self._packed_ver = ver
        self._packed = self.eng.disc_pack(*[p.detach().to(torch.float32).contiguous() for p in ps], packed=self._packed)
        return self._packed

    def invalidate(self):
        """Forget the cached stream (only meaningful with cache_packed)."""
        self._packed_ver = None

    def _update_statistics(self, x):
        """Standardizer.forward's update_mean_std on the masked batch (networks.py:70,76-81)."""
        whole = self.mask is None or (self._identity_mask and x.shape[1] == self.mask.numel())
        self.stand.update_mean_std(x if whole else x[:, self.mask.long()].contiguous())
        return None if whole else self.mask

    def _pair_args(self, x, x2):
        self._check_pair(x, x2)
        ps = [p.detach() for p in self._params()]
        direct = all(p.dtype == torch.float32 and p.is_contiguous() for p in ps)
        if self._packed is None or not direct or getattr(self, "cache_packed", False):
            packed, ps = self.packed(), None
        else:
            packed = self._packed
        return x.to(torch.float32).contiguous(), x2.to(torch.float32).contiguous(), packed, ps

    @torch.no_grad()
    def forward(self, x, eps, want=("reward",), out=None, x2=None):
        """Statistics update + oly_disc_forward: any of reward / logits / mu / logvar for x [B,Dx] (and the second tensor
        x2 [B, obs or act] of a paired reward: oly_disc_reward_step_pair, the masks applied inside the kernels)."""
        if self.pair is not None:
            x, x2, packed, ps = self._pair_args(x, x2)
            st = self.stand
            o = self.eng.disc_reward_step_pair(x, x2, packed, st.colstats, self._stats_a, not st._fresh,
                                               self.pair == "next_state", mask=self.mask, mask2=self.mask2, eps=eps,
                                               want=want, out=out, weights=ps)
            st._fresh = False
            return o
        whole = self.mask is None or (self._identity_mask and x.shape[1] == self.mask.numel())
        if whole and isinstance(self.stand, DeviceStandardizer):
            # statistics update + forward issued by ONE C call (three launches): from Python the separate calls are
            # host-bound at the reference's batch (B = 4096: 32 us against 21)
            st = self.stand
            ps = [p.detach() for p in self._params()]
            direct = all(p.dtype == torch.float32 and p.is_contiguous() for p in ps)
            if self._packed is None or not direct or getattr(self, "cache_packed", False):
                packed, ps = self.packed(), None                      # separate pack call (or the opt-in cache)
            else:
                packed = self._packed                                # re-packed from the live parameters inside the call
            o = self.eng.disc_reward_step(x, packed, st.colstats, not st._fresh, eps=eps, want=want, out=out, weights=ps)
            st._fresh = False
            return o
        mask = self._update_statistics(x)
        return self.eng.disc_forward(x, self.packed(), mask=mask, colstats=self.stand.colstats, eps=eps, want=want,
                                     out=out)

    def prepared(self, x, eps, want=("reward",), out=None, x2=None):
        """`step()` = forward(x, eps, want, out) on these same tensors with every argument validated once: the loop a
        reward evaluation over a fixed rollout block runs (whole rows, fused network).  The weights are re-packed from
        the live parameters inside every call."""
        if self.pair is not None:
            x, x2, packed, ps = self._pair_args(x, x2)
            st = self.stand
            launch = self.eng.disc_reward_step_pair(x, x2, packed, st.colstats, self._stats_a, None,
                                                    self.pair == "next_state", mask=self.mask, mask2=self.mask2, eps=eps,
                                                    want=want, out=out, weights=ps)

            def pair_step():
                o = launch(not st._fresh)
                st._fresh = False
                return o
            return pair_step
        whole = self.mask is None or (self._identity_mask and x.shape[1] == self.mask.numel())
        ps = [p.detach() for p in self._params()]
        if not (whole and self.fused and isinstance(self.stand, DeviceStandardizer)
                and all(p.dtype == torch.float32 and p.is_contiguous() for p in ps)):
            return lambda: self.forward(x, eps, want=want, out=out)
        st = self.stand
        if self._packed is None:
            self.packed()
        launch = self.eng.disc_reward_step(x, self._packed, st.colstats, None, eps=eps, want=want, out=out,
                                           weights=None if getattr(self, "cache_packed", False) else ps)

        def step():
            o = launch(not st._fresh)
            st._fresh = False
            return o
        return step

    # ---- layer-by-layer path (PyTorch GEMMs + K8 kernels): other network shapes, and the cross-check
    @torch.no_grad()
    def logits_unfused(self, x, eps):
        xs = self.stand.forward(x, self.mask)
        mu, logvar = self.net.encode(xs)
        z = self.eng.disc_reparam(mu.contiguous(), logvar.contiguous(), eps)
        return self.net.decoder(z).reshape(-1).contiguous(), mu, logvar

    @torch.no_grad()
    def logits(self, x, eps, x2=None):
        if not self.fused:
            return self.logits_unfused(x, eps)
        o = self.forward(x, eps, want=("logits", "mu", "logvar"), x2=x2)
        return o["logits"], o["mu"], o["logvar"]

    @torch.no_grad()
    def predict(self, x, eps=None, want=("logits",), out=None, x2=None):
        """The paired forward on the current statistics, without updating them."""
        from ._ffi import OlyError
        if self.pair is None:
            raise OlyError("DiscriminatorReward.predict serves a paired reward; states only: eng.disc_forward")
        self._check_pair(x, x2)
        cs = self.stand.colstats
        return self.eng.disc_forward_pair(x.to(torch.float32).contiguous(), x2.to(torch.float32).contiguous(),
                                          self.packed(), self.pair == "next_state", mask=self.mask, mask2=self.mask2,
                                          stats_a=cs, stats_b=cs, eps=eps, want=want, out=out)

    @torch.no_grad()
    def __call__(self, x, eps=None, generator=None, x2=None):
        if eps is None:
            eps = torch.randn((x.shape[0], self.net.mu_out.out_features), dtype=torch.float32,
                              device=x.device, generator=generator)
        if self.pair is not None:
            return self.forward(x, eps, x2=x2)["reward"]
        if self.fused:
            return self.forward(x, eps)["reward"]
        d, _, _ = self.logits_unfused(x, eps)
        return self.eng.disc_reward(d)


class GAILDiscriminator(nn.Module):
    """GAIL's DiscriminatorNetwork (imitation_lib/utils/networks.py:194-225) as create_gail_agent builds it
    (examples/imitation_learning/utils.py:79-97): in -> n_features -> 1 with tanh / tanh / identity and the default
    initialisation (initializers=None, networks.py:133-139): xavier_uniform_ with the activation's gain (5/3 for tanh,
    1 for identity) on every weight, nn.Linear's own draw for the biases."""

    def __init__(self, in_dim, n_features=(512, 256)):
        super().__init__()
        dims = [int(in_dim)] + [int(f) for f in n_features] + [1]
        self._linears = nn.ModuleList([nn.Linear(dims[i], dims[i + 1]) for i in range(len(dims) - 1)])
        acts = ["tanh"] * len(n_features) + ["linear"]
        for lin, act in zip(self._linears, acts):
            nn.init.xavier_uniform_(lin.weight, gain=nn.init.calculate_gain(act))

    def forward(self, xs):
        """The logits [B, 1] of an already standardised batch."""
        h = xs
        for lin in self._linears[:-1]:
            h = torch.tanh(lin(h))
        return self._linears[-1](h)


class GAILDiscriminatorReward(PairedInput, DiscriminatorState):
    """make_discrim_reward (gail_TRPO.py:320-327) for GAIL's discriminator on the device (K18): the Standardizer's
    update with the masked rows, then in -> 512 -> 256 -> 1 (tanh, tanh, identity) and the reward formula in one launch,
    the state mask (prepare_discrim_inputs, :297-313) applied inside the kernel.

    net: any module exposing three `_linears` of widths in <= 64 -> 512 -> 256 -> 1 (GAILDiscriminator, the reference's
    DiscriminatorNetwork); others are refused with OlyError.  standardizer: the discriminator's own DeviceStandardizer
    (the D_standardizer), created when not given.

    pair: what the discriminator looks at besides the states (DiscriminatorNetwork.preprocess_inputs, networks.py:216-234;
    prepare_discrim_inputs, gail_TRPO.py:297-313).  None: states only.  "next_state" (use_next_states=True): the input
    is [standardise(s[:, state_mask]) | standardise(s'[:, state_mask])], the network takes 2 Ds columns and the
    Standardizer is updated twice per forward, with the states and then with the next states, so the two halves of a row
    are standardised with different statistics and the count rises by 2 B.  "action" (disc_only_states=False): the input
    is [standardise(s[:, state_mask]) | a[:, act_mask]], the actions raw.  The Standardizer has Ds columns in every mode.
    forward / predict / __call__ then take the second tensor as x2.  Next states together with an act_mask (the
    reference's ValueError, gail_TRPO.py:195-196,308-309), an empty second part and Ds + D2 > 64 are refused."""

    def __init__(self, engine, net, state_mask=None, standardizer=None, pair=None, act_mask=None):
        from ._ffi import OlyError
        lins = list(getattr(net, "_linears", ()))
        if len(lins) != 3 or not all(isinstance(l, nn.Linear) for l in lins):
            raise OlyError("GAILDiscriminatorReward: the network must expose three Linear layers as `_linears`")
        dim = int(lins[0].in_features)
        if not 0 < dim <= 64 or (int(lins[0].out_features), int(lins[1].in_features), int(lins[1].out_features),
                                 int(lins[2].in_features), int(lins[2].out_features)) != (512, 512, 256, 256, 1):
            raise OlyError("GAILDiscriminatorReward: supported network is in <= 64 -> 512 -> 256 -> 1")
        self.eng, self.net, self.lins, self.in_dim = engine, net, lins, dim
        self.pair = pair
        if pair is not None:
            self._init_pair(dim, state_mask, act_mask, standardizer)
            return
        if act_mask is not None and np.asarray(act_mask).size:
            raise OlyError("GAILDiscriminatorReward: an act_mask needs pair='action'")
        self.mask = None
        if state_mask is not None:
            m = np.asarray(state_mask, dtype=np.int64).reshape(-1)
            if m.size != dim or (m.size and m.min() < 0):
                raise OlyError(f"GAILDiscriminatorReward: the state mask has {m.size} columns, the network takes {dim}")
            self._mask_max = int(m.max())
            self.mask = torch.as_tensor(m.astype(np.int32), device=engine.device)
        self.stand = standardizer or DeviceStandardizer(engine, dim)
        self._packed = None

    def _params(self):
        return [t for lin in self.lins for t in (lin.weight, lin.bias)]

    def packed(self):
        """The MFMA operand stream of the CURRENT weights, re-packed on every call into the same buffer, for the reason
        DiscriminatorReward.packed documents: a cache keyed on `_version` would miss writes through `.data`."""
        self._packed = self.eng.ilmlp_pack(*[p.detach().to(torch.float32).contiguous() for p in self._params()],
                                           packed=self._packed)
        return self._packed

    def invalidate(self):
        """Nothing is cached: every forward re-packs."""

    def _check(self, x):
        from ._ffi import OlyError
        if x.dim() != 2:
            raise OlyError("GAILDiscriminatorReward: x is [B, obs]")
        if self.mask is None and int(x.shape[1]) != self.in_dim:
            raise OlyError(f"GAILDiscriminatorReward: {x.shape[1]} columns, the network takes {self.in_dim}")
        if self.mask is not None and int(x.shape[1]) <= self._mask_max:
            raise OlyError(f"GAILDiscriminatorReward: {x.shape[1]} columns, the state mask reads column {self._mask_max}")

    @torch.no_grad()
    def forward(self, x, want=("reward",), out=None, x2=None):
        """Statistics update with the masked rows + forward, one C call: any of reward / logits for x [B,obs] (and the
        second tensor x2 [B, obs or act] of a paired reward)."""
        if self.pair is not None:
            self._check_pair(x, x2)
        else:
            self._check(x)
        st = self.stand
        ps = [p.detach() for p in self._params()]
        if self._packed is None or not all(p.dtype == torch.float32 and p.is_contiguous() for p in ps):
            packed, ps = self.packed(), None                        # separate pack call
        else:
            packed = self._packed                                  # re-packed from the live parameters inside the call
        if self.pair is not None:
            o = self.eng.gail_reward_step_pair(x.to(torch.float32).contiguous(), x2.to(torch.float32).contiguous(), packed,
                                               st.colstats, self._stats_a, not st._fresh, self.pair == "next_state",
                                               mask=self.mask, mask2=self.mask2, want=want, out=out, weights=ps)
            st._fresh = False
            return o
        o = self.eng.gail_reward_step(x.to(torch.float32).contiguous(), packed, st.colstats, not st._fresh,
                                      mask=self.mask, want=want, out=out, weights=ps)
        st._fresh = False
        return o

    @torch.no_grad()
    def predict(self, x, want=("logits",), out=None, x2=None):
        """The forward on the current statistics, without updating them."""
        if self.pair is not None:
            self._check_pair(x, x2)
            cs = self.stand.colstats
            return self.eng.gail_disc_forward_pair(x.to(torch.float32).contiguous(), x2.to(torch.float32).contiguous(),
                                                   self.packed(), self.pair == "next_state", mask=self.mask,
                                                   mask2=self.mask2, stats_a=cs, stats_b=cs, want=want, out=out)
        self._check(x)
        return self.eng.gail_disc_forward(x.to(torch.float32).contiguous(), self.packed(), mask=self.mask,
                                          colstats=self.stand.colstats, want=want, out=out)

    @torch.no_grad()
    def __call__(self, x, eps=None, generator=None, x2=None):
        """The reward [B].  eps / generator are accepted and ignored (GAIL's discriminator draws no noise), so the
        agent's sequence can call either discriminator."""
        return self.forward(x, x2=x2)["reward"]


PAIR_MODES = (None, "next_state", "action")


def pair_masks(who, pair, dim, state_mask, act_mask, device):
    """(mask, mask2, max(mask), max(mask2)) of a paired discriminator input of `dim` columns, each mask an int32 device
    tensor or None (identity).  pair "next_state": both parts read state_mask, dim = 2 Ds; an act_mask with columns is
    the reference's refused three-part combination.  pair "action": the second part reads act_mask; one of the two
    masks may be left out (its part then takes the source's columns as they are, dim - the other's width of them)."""
    from ._ffi import OlyError
    if pair not in PAIR_MODES or pair is None:
        raise OlyError(f"{who}: pair is None, 'next_state' or 'action' (got {pair!r})")

    def arr(m, name):
        m = np.asarray(m, dtype=np.int64).reshape(-1)
        if m.size and m.min() < 0:
            raise OlyError(f"{who}: negative column in the {name}")
        return m
    sm = None if state_mask is None else arr(state_mask, "state mask")
    am = None if act_mask is None else arr(act_mask, "act_mask")
    if pair == "next_state":
        if am is not None and am.size:
            raise OlyError(f"{who}: states, actions and next states together are not supported (the reference raises "
                           "ValueError, gail_TRPO.py:195-196,308-309)")
        if dim % 2 or (sm is not None and 2 * sm.size != dim) or dim < 2:
            raise OlyError(f"{who}: with next states the network takes twice the masked state columns, not {dim}")
        am = sm
    else:
        ds = dim - am.size if am is not None else (sm.size if sm is not None else -1)
        if am is None and sm is None:
            raise OlyError(f"{who}: pair='action' needs a state mask or an act_mask to split the {dim} columns")
        if (am is not None and am.size == 0) or ds >= dim:
            raise OlyError(f"{who}: the second part has no column (D2 == 0)")
        if ds <= 0 or (sm is not None and sm.size != ds):
            raise OlyError(f"{who}: the masks select {-1 if sm is None else sm.size} + {-1 if am is None else am.size} "
                           f"columns, the network takes {dim}")
    if dim > 64:
        raise OlyError(f"{who}: the paired input is {dim} columns wide, the kernels take at most 64")

    def dev(m):
        return None if m is None else torch.as_tensor(m.astype(np.int32), device=device)
    return dev(sm), dev(am), (None if sm is None else int(sm.max())), (None if am is None else int(am.max()))


class GAILAdvantage:
    """The reward / advantage half of GAIL.fit (gail_TRPO.py:105-129) on the device:

        r_disc = make_discrim_reward(x, u, xn)
        r      = r * env_reward_frac + r_disc * (1 - env_reward_frac)
        v_target, adv = compute_gae(V, x, xn, r, absorbing, last, gamma, lam)
        adv    = (adv - mean(adv)) / (std(adv) + 1e-8)            (numpy, biased std)

    x / xn are [T,N,obs] rollout blocks (the reference's flat dataset is the N = 1 case)."""

    def __init__(self, engine, disc_reward, critic, gamma=0.99, lam=0.97, env_reward_frac=0.0):
        from .rollout import GAERollout
        assert 0.0 <= env_reward_frac <= 1.0, "Environment reward must be between [0,1]"
        self.eng, self.disc, self.critic = engine, disc_reward, critic
        self.frac = env_reward_frac
        self.post = GAERollout(engine, gamma=gamma, lam=lam)

    @torch.no_grad()
    def __call__(self, x, xn, r_env, absorbing, last, eps=None):
        from . import _abi
        from .rollout import RolloutBuffer
        T, N, D = x.shape
        flat = x.reshape(T * N, D).contiguous()
        if self.frac < 1.0:
            r_disc = self.disc(flat, eps).reshape(T, N)
            r = r_env * self.frac + r_disc * (1 - self.frac)
        else:
            r = r_env
        buf = RolloutBuffer(T, N, D, 1, x.device)
        buf.rewards.copy_(r)
        buf.values.copy_(self.critic(flat).reshape(T, N))
        buf.next_values.copy_(self.critic(xn.reshape(T * N, D)).reshape(T, N))
        buf.flags.copy_((last.to(torch.uint8) * _abi.FLAG_LAST) | (absorbing.to(torch.uint8) * _abi.FLAG_ABSORBING))
        buf.ptr = T
        v_target, adv = self.post.finish(buf, normalize=True)
        return r, v_target, adv


# ------------------------------------------------------------------------------ discriminator fitting
def logit_bernoulli_entropy(logits):
    """(1 - sigmoid(x)) * x - logsigmoid(x)   imitation_lib/utils/math.py:34-39."""
    return (1.0 - torch.sigmoid(logits)) * logits - torch.nn.functional.logsigmoid(logits)


def gail_discriminator_loss(logits, target, entcoeff=1e-3):
    """GailDiscriminatorLoss.forward (imitation_lib/utils/math.py:24-32):
    mean(max(x,0) - x*z + log(1 + exp(-|x|))) - entcoeff * mean(bernoulli entropy)."""
    bce = torch.maximum(logits, torch.zeros_like(logits)) - logits * target + torch.log(1 + torch.exp(-torch.abs(logits)))
    return torch.mean(bce) - entcoeff * torch.mean(logit_bernoulli_entropy(logits))


class VDBLoss:
    """Variational-discriminator-bottleneck loss with the dual variable beta updated on every
    call (imitation_lib/utils/math.py:42-90): bce + beta * (mean KL - I_c) [+ entropy]."""

    def __init__(self, info_constraint, lr_beta, use_bernoulli_ent=False, entcoeff=1e-3):
        self._info_constr, self._lr_beta = info_constraint, lr_beta
        self._use_bernoulli_ent, self.entcoeff = use_bernoulli_ent, entcoeff
        self._beta = 0.1

    @staticmethod
    def kl_divergence(mu, logvar):
        return 0.5 * torch.sum(torch.pow(mu, 2) + torch.exp(logvar) - logvar - 1, dim=1)

    def __call__(self, inputs, target):
        logits, mu, logvar = inputs
        bottleneck = self.kl_divergence(mu, logvar).mean() - self._info_constr
        bce = torch.nn.functional.binary_cross_entropy_with_logits(torch.squeeze(logits), torch.squeeze(target))
        ent = logit_bernoulli_entropy(logits) if self._use_bernoulli_ent else torch.zeros_like(bce)
        loss = bce + self._beta * bottleneck + ent
        with torch.no_grad():                                   # dual ascent, clipped at 0 (:80-82)
            self._beta = max(0, self._beta + self._lr_beta * bottleneck)
        return loss


class ExpertDataset:
    """The demonstrations of GAIL / VAIL resident on the device.

    Trajectory.create_dataset (utils/trajectory.py:129-193) returns states / next_states as slices of
    the flattened trajectory table; here the table is uploaded ONCE (oly_traj_upload, the same copy
    K4's reset / next-sample kernels read) and the dataset is never materialised: a minibatch of the
    discriminator (gail_TRPO.py:176-202, demo_obs = states[indices][:, state_mask].astype(np.float32))
    is one row gather on the device by caller-drawn indices."""

    def __init__(self, engine, trajectory, ignore_keys=("q_pelvis_tx", "q_pelvis_tz"), state_mask=None):
        self.eng = engine
        if engine.traj_shape != tuple(trajectory.table.shape):
            engine.traj_upload(trajectory.table)
        keys = list(trajectory.keys)
        kept = [i for i, k in enumerate(keys) if k not in set(ignore_keys or ())]
        mask = np.arange(len(kept)) if state_mask is None else np.asarray(state_mask, dtype=np.int64)
        self.dataset_cols = torch.as_tensor(np.asarray(kept, dtype=np.int32), device=engine.device)
        self.cols = torch.as_tensor(np.asarray(kept, dtype=np.int32)[mask], device=engine.device)   # mask folded in
        self.rows = engine.expert_rows()

    def arrays(self):
        """states / next_states / absorbing / last exactly as create_dataset returns them (float64)."""
        return self.eng.expert_dataset(self.dataset_cols)

    def shuffled_indices(self, batch, rs=None):
        """The first batch of mushroom's minibatch_generator (np.random.shuffle of arange(rows), first
        `batch` entries): the reference's draw, made on the host, handed over as an input."""
        idx = np.arange(self.rows)
        (rs if rs is not None else np.random).shuffle(idx)
        return torch.as_tensor(idx[:batch].astype(np.int64), device=self.eng.device)

    def minibatch(self, idx, want_next=False):
        return self.eng.expert_gather(idx, self.cols, want_next=want_next)


class DiscriminatorTrainer:
    """The discriminator half of GAIL._fit_discriminator (gail_TRPO.py:167-218), states-only
    input as in the UnitreeH1 configuration: per epoch draw as many demonstration states as
    policy states, update the standardiser with the concatenated batch, targets 0 (policy) / 1
    (demonstrations) or the noisy variants, one optimiser step.  Random numbers (minibatch
    indices, noisy targets, VAIL eps) come from the caller's torch.Generator.

    mushroom's TorchApproximator.fit (absent) drives the optimiser in the reference; one Adam
    step per epoch on the whole concatenated batch is this class's stated reading of it."""

    def __init__(self, reward: "DiscriminatorReward", demo_states, loss, lr=5e-5, weight_decay=1e-3,
                 n_epochs=1, use_noisy_targets=False, variational=True):
        self.r, self.loss, self.n_epochs = reward, loss, n_epochs
        dev = reward.eng.device
        # an ExpertDataset serves minibatches straight from the device-resident trajectory table (its
        # columns already carry the state mask); an array is the dataset's `states` uploaded as is
        self.expert = demo_states if isinstance(demo_states, ExpertDataset) else None
        self.demo = None if self.expert is not None else torch.as_tensor(np.asarray(demo_states), dtype=torch.float32,
                                                                         device=dev)
        self.noisy, self.variational = use_noisy_targets, variational
        self.opt = torch.optim.Adam(reward.net.parameters(), lr=lr, weight_decay=weight_decay)

    def fit(self, plcy_obs, generator=None):
        r, dev = self.r, self.r.eng.device
        n = plcy_obs.shape[0]
        losses = []
        for _ in range(self.n_epochs):
            if self.expert is not None:
                idx = torch.randint(0, self.expert.rows, (n,), device=dev, generator=generator)
                plcy = plcy_obs.to(torch.float32)
                plcy = plcy if r.mask is None else plcy[:, r.mask.long()]
                x = torch.cat([plcy, self.expert.minibatch(idx)]).contiguous()
                xs = r.stand.forward(x, None)                    # updates the running statistics
            else:
                idx = torch.randint(0, self.demo.shape[0], (n,), device=dev, generator=generator)
                x = torch.cat([plcy_obs.to(torch.float32), self.demo[idx]]).contiguous()
                xs = r.stand.forward(x, r.mask)                  # updates the running statistics
            if self.noisy:
                demo_t = torch.empty((n, 1), device=dev).uniform_(0.80, 0.99, generator=generator)
                plcy_t = torch.empty((n, 1), device=dev).uniform_(0.01, 0.10, generator=generator)
            else:
                plcy_t, demo_t = torch.zeros((n, 1), device=dev), torch.ones((n, 1), device=dev)
            target = torch.cat([plcy_t, demo_t])
            mu, logvar = r.net.encode(xs)
            if self.variational:
                eps = torch.randn(mu.shape, device=dev, generator=generator)
                z = mu + torch.exp(logvar / 2) * eps
                loss = self.loss((r.net.decoder(z), mu, logvar), target)
            else:
                loss = self.loss(r.net.decoder(mu), target)
            self.opt.zero_grad()
            loss.backward()
            self.opt.step()
            losses.append(float(loss.detach()))
        return losses
