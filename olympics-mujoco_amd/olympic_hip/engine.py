"""Typed torch front-end over the C ABI: one method per entry point of
include/olympic_hip.h.  Tensors are validated (device, dtype, contiguity, shape) on the
host before any kernel is launched - a wrong shape must never reach the GPU.  PyTorch is
only the allocator/stream provider here; every computation is a HIP kernel of
libolympic_hip.so running on torch's current stream.
"""
import ctypes as C
import types

import numpy as np
import torch

from . import _abi
from ._ffi import Context, OlyError, lib, ptr


def _req(t, name, shape, dtype, device, optional=False):
    if t is None:
        if optional:
            return None
        raise OlyError(f"{name}: required tensor is None")
    if not isinstance(t, torch.Tensor):
        raise OlyError(f"{name}: expected a torch.Tensor, got {type(t).__name__}")
    if t.device != device:
        raise OlyError(f"{name}: tensor on {t.device}, engine on {device}")
    if t.dtype != dtype:
        raise OlyError(f"{name}: dtype {t.dtype}, expected {dtype}")
    if tuple(t.shape) != tuple(shape):
        raise OlyError(f"{name}: shape {tuple(t.shape)}, expected {tuple(shape)}")
    if not t.is_contiguous():
        raise OlyError(f"{name}: tensor must be contiguous")
    return t


# What the host layer knows of the two discriminator networks (VAIL: K12 / K15, GAIL: K18), for the bodies the two
# share below: the pack method the `weights` of a reward step follow and their shapes (the flat parameter vector of a
# fit is their concatenation, n_par values), the packed-size method, the outputs of a forward, whether a forward takes
# noise, and what the fit adds to the common arguments: the entry points' stem, the struct, its own scalars and its own
# tensors as (name, shape key of _disc_fit_epoch, dtype, optional).
_VAIL = types.SimpleNamespace(
    pack="disc_pack", packed_floats="_disc_packed_floats", noise=True,
    weights=lambda D: ((256, D), (256,), (128, 256), (128,), (128, 128), (128,), (128, 128), (128,), (1, 128), (1,)),
    outputs=lambda B: dict(reward=(B,), logits=(B,), mu=(B, 128), logvar=(B, 128)),
    n_par=lambda D: 256 * D + 256 + 128 * 256 + 128 + 2 * (128 * 128 + 128) + 128 + 1,
    fit="disc_fit", struct=_abi.DiscFit, fit_scalars=("info_constraint", "lr_beta"),
    fit_tensors=(("eps", "noise", torch.float32, False), ("beta", "one", torch.float32, False),
                 ("kl_out", "batches", torch.float64, True), ("beta_out", "batches", torch.float32, True)))
_GAIL = types.SimpleNamespace(
    pack="ilmlp_pack", packed_floats="_gail_packed_floats", noise=False,
    weights=lambda D: ((512, D), (512,), (256, 512), (256,), (1, 256), (1,)),
    outputs=lambda B: dict(reward=(B,), logits=(B,)),
    n_par=lambda D: 512 * D + 512 + 256 * 512 + 256 + 256 + 1,
    fit="gail_disc_fit", struct=_abi.GailDiscFit, fit_scalars=("entcoeff",),
    fit_tensors=(("ent_out", "batches", torch.float64, True),))


class Engine:
    """HIP hot-path engine bound to one device."""

    def __init__(self, device=None):
        self.ctx = Context(device)
        self.device = self.ctx.device
        self.il_spec = None
        self.a3_spec = None
        self.traj_shape = None
        self.contact_ok = False

    # -------------------------------------------------------------- helpers
    def _new(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.device)

    def _s(self):
        return self.ctx.stream()

    def _out(self, out, key, shape, dtype):
        """Caller-supplied output buffer `out[key]` (validated) or a fresh one; nothing is allocated
        when the caller passes its own buffers."""
        t = out.get(key) if out else None
        if t is None:
            t = self._new(shape, dtype)
        return _req(t, key, shape, dtype, self.device)

    # -------------------------------------------------------------- K1 / K5
    def il_configure(self, spec):
        self.ctx.call("oly_il_configure", C.byref(spec.to_c()))
        self.il_spec = spec
        return self

    def il_step(self, qpos, qvel, action, prev_in, prev_out=None, grf_mean=None, out=None,
                obs_f64=False, ctrl_f64=False, want_fall_code=True, want_ctrl=True):
        """qpos [T,N,nq] f64, qvel [T,N,nv] f64, action [T,N,n_act] f32 (or None).
        Returns dict(obs, reward, absorbing, fall_code, ctrl, prev)."""
        sp = self.il_spec
        if sp is None:
            raise OlyError("il_step before il_configure")
        if qpos.dim() != 3:
            raise OlyError(f"qpos: expected [T,N,nq], got {tuple(qpos.shape)}")
        T, N = int(qpos.shape[0]), int(qpos.shape[1])
        dv = self.device
        _req(qpos, "qpos", (T, N, sp.nq), torch.float64, dv)
        _req(qvel, "qvel", (T, N, sp.nv), torch.float64, dv)
        want_ctrl = want_ctrl and action is not None
        _req(action, "action", (T, N, sp.n_act), torch.float32, dv, optional=True)
        _req(grf_mean, "grf_mean", (T, N, sp.n_grf), torch.float64, dv, optional=sp.n_grf == 0)
        _req(prev_in, "prev_in", (N,), torch.float64, dv)
        if prev_out is None:
            prev_out = prev_in if T == 1 else self._new((N,), torch.float64)
        _req(prev_out, "prev_out", (N,), torch.float64, dv)
        if T > 1 and prev_out.data_ptr() == prev_in.data_ptr():
            raise OlyError("prev_out must not alias prev_in when T > 1")
        out = out or {}
        od = torch.float64 if obs_f64 else torch.float32
        cd = torch.float64 if ctrl_f64 else torch.float32
        obs = self._out(out, "obs", (T, N, sp.n_obs), od)
        reward = self._out(out, "reward", (T, N), torch.float32)
        absorbing = self._out(out, "absorbing", (T, N), torch.uint8)
        code = self._out(out, "fall_code", (T, N), torch.uint8) if want_fall_code else None
        ctrl = self._out(out, "ctrl", (T, N, sp.nu), cd) if want_ctrl else None
        flags = (_abi.OUT_OBS_F64 if obs_f64 else 0) | (_abi.OUT_CTRL_F64 if ctrl_f64 else 0)
        self.ctx.call("oly_il_step", T, N, ptr(qpos), ptr(qvel), ptr(action), ptr(grf_mean), ptr(prev_in),
                      ptr(prev_out), ptr(obs), ptr(reward), ptr(absorbing), ptr(code), ptr(ctrl), flags,
                      self._s())
        return dict(obs=obs, reward=reward, absorbing=absorbing, fall_code=code, ctrl=ctrl, prev=prev_out)

    def il_step_prepare(self, qpos, qvel, action, prev_in, prev_out=None, **kw):
        """Validate once, then return a zero-argument callable that re-launches oly_il_step on
        the SAME buffers (the per-step regime of a vec env: ~2 us of host time per call instead
        of the full validation path).  Returns (call, outputs)."""
        rec = {}
        orig = self.ctx.call

        def capture(name, *args):
            rec["name"], rec["args"] = name, args
        self.ctx.call = capture
        try:
            outs = self.il_step(qpos, qvel, action, prev_in, prev_out, **kw)
        finally:
            self.ctx.call = orig
        from ._ffi import check, lib
        fn = getattr(lib(), rec["name"])
        h, args = self.ctx.handle, rec["args"][:-1]
        keep = (qpos, qvel, action, prev_in, outs)     # keep the tensors alive with the closure

        def call(stream=None):
            rc = fn(h, *args, stream if stream is not None else self._s())
            if rc:
                check(h, rc, rec["name"])
            return keep[-1]
        return call, outs

    # -------------------------------------------------------------- K4
    def traj_upload(self, table):
        table = np.ascontiguousarray(table, dtype=np.float64)
        if table.ndim != 3:
            raise OlyError(f"trajectory table must be [n_keys,n_traj,len], got {table.shape}")
        K, J, L = table.shape
        self.ctx.call("oly_traj_upload", K, J, L, ptr(table))
        self.traj_shape = (K, J, L)
        return self

    def traj_reset(self, traj_no, step, cur_traj=None, cur_step=None, origin=None, sample=None):
        if self.traj_shape is None:
            raise OlyError("traj_reset before traj_upload")
        K = self.traj_shape[0]
        N = int(traj_no.shape[0])
        dv = self.device
        _req(traj_no, "traj_no", (N,), torch.int32, dv)
        _req(step, "step", (N,), torch.int32, dv)
        cur_traj = _req(cur_traj if cur_traj is not None else self._new((N,), torch.int32), "cur_traj", (N,), torch.int32, dv)
        cur_step = _req(cur_step if cur_step is not None else self._new((N,), torch.int32), "cur_step", (N,), torch.int32, dv)
        origin = _req(origin if origin is not None else self._new((N, 2), torch.float64), "origin", (N, 2), torch.float64, dv)
        sample = _req(sample if sample is not None else self._new((N, K), torch.float64), "sample", (N, K), torch.float64, dv)
        self.ctx.call("oly_traj_reset", N, ptr(traj_no), ptr(step), ptr(cur_traj), ptr(cur_step), ptr(origin),
                      ptr(sample), self._s())
        return cur_traj, cur_step, origin, sample

    def traj_next(self, cur_traj, cur_step, origin, sample, active=None, at_end=None):
        if self.traj_shape is None:
            raise OlyError("traj_next before traj_upload")
        K = self.traj_shape[0]
        N = int(cur_traj.shape[0])
        dv = self.device
        _req(cur_traj, "cur_traj", (N,), torch.int32, dv)
        _req(cur_step, "cur_step", (N,), torch.int32, dv)
        _req(origin, "origin", (N, 2), torch.float64, dv)
        _req(sample, "sample", (N, K), torch.float64, dv)
        _req(active, "active", (N,), torch.uint8, dv, optional=True)
        at_end = _req(at_end if at_end is not None else self._new((N,), torch.uint8), "at_end", (N,), torch.uint8, dv)
        self.ctx.call("oly_traj_next", N, ptr(active), ptr(cur_traj), ptr(cur_step), ptr(origin), ptr(sample),
                      ptr(at_end), self._s())
        return at_end

    def traj_euler(self, n_qpos, dt, curr_qpos, sample):
        if self.traj_shape is None:
            raise OlyError("traj_euler before traj_upload")
        K = self.traj_shape[0]
        N = int(sample.shape[0])
        _req(curr_qpos, "curr_qpos", (N, n_qpos), torch.float64, self.device)
        _req(sample, "sample", (N, K), torch.float64, self.device)
        self.ctx.call("oly_traj_euler", N, int(n_qpos), C.c_double(dt), ptr(curr_qpos), ptr(sample), self._s())
        return sample

    # -------------------------------------------------------------- expert data (K4 table as the dataset)
    def expert_rows(self):
        from ._ffi import lib
        n = int(lib().oly_expert_rows(self.ctx.handle))
        if n < 0:
            raise OlyError("expert data before traj_upload")
        return n

    def expert_gather(self, idx, cols, want_next=False, check=True):
        """Rows `idx` ([B] int64 device tensor, caller-drawn) of create_dataset's states (and next_states)
        restricted to the table keys `cols` ([n_cols] int32 device tensor), as float32."""
        B, n_cols = int(idx.shape[0]), int(cols.shape[0])
        _req(idx, "idx", (B,), torch.int64, self.device)
        _req(cols, "cols", (n_cols,), torch.int32, self.device)
        if check and B:
            lo, hi = int(idx.min()), int(idx.max())
            if lo < 0 or hi >= self.expert_rows():
                raise OlyError(f"expert_gather: row index out of range [{lo}, {hi}] for {self.expert_rows()} rows")
        st = self._new((B, n_cols), torch.float32)
        nx = self._new((B, n_cols), torch.float32) if want_next else None
        self.ctx.call("oly_expert_gather", C.c_int64(B), ptr(idx), n_cols, ptr(cols), ptr(st), ptr(nx), self._s())
        return (st, nx) if want_next else st

    def expert_dataset(self, cols):
        """dict(states, next_states [rows, n_cols] f64, absorbing [rows], last [rows + 1]) on the device."""
        n_cols, rows = int(cols.shape[0]), self.expert_rows()
        _req(cols, "cols", (n_cols,), torch.int32, self.device)
        d = dict(states=self._new((rows, n_cols), torch.float64), next_states=self._new((rows, n_cols), torch.float64),
                 absorbing=self._new((rows,), torch.float64), last=self._new((rows + 1,), torch.float64))
        self.ctx.call("oly_expert_dataset", n_cols, ptr(cols), ptr(d["states"]), ptr(d["next_states"]),
                      ptr(d["absorbing"]), ptr(d["last"]), self._s())
        return d

    # -------------------------------------------------------------- K3
    def contact_configure(self, geom_bodyid, floor_body, rfoot_body, lfoot_body):
        gb = np.ascontiguousarray(geom_bodyid, dtype=np.int32)
        self.ctx.call("oly_contact_configure", len(gb), ptr(gb), int(floor_body), int(rfoot_body), int(lfoot_body))
        self.contact_ok = True
        return self

    def contact_reduce(self, ncon, geom1, geom2, force6, pos_z, want_idx=True):
        if not self.contact_ok:
            raise OlyError("contact_reduce before contact_configure")
        dv = self.device
        if geom1.dim() != 2:
            raise OlyError(f"geom1: expected [N,C], got {tuple(geom1.shape)}")
        N, Cc = int(geom1.shape[0]), int(geom1.shape[1])
        _req(ncon, "ncon", (N,), torch.int32, dv)
        _req(geom1, "geom1", (N, Cc), torch.int32, dv)
        _req(geom2, "geom2", (N, Cc), torch.int32, dv)
        _req(force6, "force6", (N, Cc, 6), torch.float64, dv)
        _req(pos_z, "pos_z", (N, Cc), torch.float64, dv)
        o = dict(n_r=self._new((N,), torch.int32), n_l=self._new((N,), torch.int32),
                 idx_r=self._new((N, Cc), torch.int32) if want_idx else None,
                 idx_l=self._new((N, Cc), torch.int32) if want_idx else None,
                 grf_r=self._new((N,), torch.float64), grf_l=self._new((N,), torch.float64),
                 min_z=self._new((N,), torch.float64), bad=self._new((N,), torch.uint8))
        self.ctx.call("oly_contact_reduce", N, Cc, ptr(ncon), ptr(geom1), ptr(geom2), ptr(force6), ptr(pos_z),
                      ptr(o["n_r"]), ptr(o["n_l"]), ptr(o["idx_r"]), ptr(o["idx_l"]), ptr(o["grf_r"]),
                      ptr(o["grf_l"]), ptr(o["min_z"]), ptr(o["bad"]), self._s())
        return o

    def contact_reduce_csr(self, ncon, coff, records, max_contacts):
        """oly_contact_reduce over compact storage: env n's contacts are records[coff[n] : coff[n] + min(ncon[n], C)];
        records: uint8 device tensor holding oly_contact_record's (64 bytes each)."""
        if not self.contact_ok:
            raise OlyError("contact_reduce_csr before contact_configure")
        dv = self.device
        N = int(ncon.shape[0])
        _req(ncon, "ncon", (N,), torch.int32, dv)
        _req(coff, "coff", (N,), torch.int32, dv)
        _req(records, "records", records.shape, torch.uint8, dv)
        if records.dim() != 1 or records.numel() % C.sizeof(_abi.ContactRecord):
            raise OlyError("records: expected a flat uint8 tensor of whole 64-byte records")
        o = dict(n_r=self._new((N,), torch.int32), n_l=self._new((N,), torch.int32),
                 grf_r=self._new((N,), torch.float64), grf_l=self._new((N,), torch.float64),
                 min_z=self._new((N,), torch.float64), bad=self._new((N,), torch.uint8))
        self.ctx.call("oly_contact_reduce_csr", N, int(max_contacts), ptr(ncon), ptr(coff), ptr(records),
                      records.numel() // C.sizeof(_abi.ContactRecord), ptr(o["n_r"]),
                      ptr(o["n_l"]), ptr(o["grf_r"]), ptr(o["grf_l"]), ptr(o["min_z"]), ptr(o["bad"]), self._s())
        return o

    # -------------------------------------------------------------- K2
    _A3_IN = dict(qpos=("nq", torch.float64), qvel=("nv", torch.float64), act_len=("nu", torch.float64),
                  act_vel=("nu", torch.float64), lf_pos=(3, torch.float64), rf_pos=(3, torch.float64),
                  lf_vel=(3, torch.float64), rf_vel=(3, torch.float64), root_pos=(3, torch.float64),
                  root_quat=(4, torch.float64), head_pos=(3, torch.float64), grf_l=(None, torch.float64),
                  grf_r=(None, torch.float64), min_z=(None, torch.float64), n_r=(None, torch.int32),
                  n_l=(None, torch.int32), bad=(None, torch.uint8))
    _A3_ST = dict(phase=(None, torch.int32), t1=(None, torch.int32), t2=(None, torch.int32),
                  reached_frames=(None, torch.int32), target_reached=(None, torch.uint8),
                  mode=(None, torch.int32), seq_len=(None, torch.int32),
                  sequence=((_abi.OLY_MAX_SEQ, 4), torch.float64), goal=(8, torch.float64))

    def a3_configure(self, spec, clock_lut):
        lut = np.ascontiguousarray(clock_lut, dtype=np.float64)
        self.ctx.call("oly_a3_configure", C.byref(spec.to_c(lut)))
        self.a3_spec = spec
        return self

    def _a3_struct(self, cls, table, tensors, N):
        sp = self.a3_spec
        st = cls()
        for name, (w, dt) in table.items():
            if isinstance(w, str):
                w = getattr(sp, w)
            shape = (N,) if w is None else ((N,) + tuple(w) if isinstance(w, tuple) else (N, w))
            t = _req(tensors.get(name), name, shape, dt, self.device)
            setattr(st, name, t.data_ptr())
        return st

    def a3_state_struct(self, state, N):
        """oly_a3_state filled with the (validated) device tensors of `state`."""
        if self.a3_spec is None:
            raise OlyError("a3 state before a3_configure")
        return self._a3_struct(_abi.A3State, self._A3_ST, state, N)

    def a3_step(self, inputs, state, obs_f64=False, out=None):
        sp = self.a3_spec
        if sp is None:
            raise OlyError("a3_step before a3_configure")
        N = int(state["phase"].shape[0])
        cin = self._a3_struct(_abi.A3Inputs, self._A3_IN, inputs, N)
        cst = self._a3_struct(_abi.A3State, self._A3_ST, state, N)
        out = out or {}
        od = torch.float64 if obs_f64 else torch.float32
        obs = self._out(out, "obs", (N, sp.n_obs), od)
        rew6 = self._out(out, "rew6", (N, 6), torch.float32)
        reward = self._out(out, "reward", (N,), torch.float32)
        done = self._out(out, "done", (N,), torch.uint8)
        self.ctx.call("oly_a3_step", N, C.byref(cin), C.byref(cst), ptr(obs), ptr(rew6), ptr(reward), ptr(done),
                      _abi.OUT_OBS_F64 if obs_f64 else 0, self._s())
        return dict(obs=obs, rew6=rew6, reward=reward, done=done)

    # -------------------------------------------------------------- K10 (one launch per vec step)
    def a3_vec_ctr_len(self, N):
        from ._ffi import lib
        return int(lib().oly_a3_vec_ctr_len(int(N)))

    def a3_vec_prepare(self, blocks, state, ro):
        """Validate every tensor of a device-resident rollout ONCE and return `launch(flags=0, mu=None,
        value=None)`, which enqueues oly_a3_vec_step on the current stream (mu / value may be swapped
        per call for an eager policy forward; everything else is fixed, so the launch is replayable
        from a HIP graph).
          blocks: dict of [K,N,...] readback tensors (oly_a3_blocks fields)
          state:  the VecA3Env task-state dict (oly_a3_state fields; mode / seq_len / sequence are
                  rewritten by device-side resets)
          ro:     dict with T, max_traj_len, deterministic, side_slots, pool_depth (ints) and the
                  tensors mu, value, scale, eps, state, pd_target, buf_states, buf_actions,
                  buf_rewards, buf_values, buf_flags, buf_rew6 (or None), traj_len, side_obs, side_t,
                  side_count, pool (uint8 [N*pool_depth*656]), pool_count, ctr, buf_mu (or None)."""
        sp = self.a3_spec
        if sp is None or not self.contact_ok:
            raise OlyError("a3_vec_prepare before a3_configure / contact_configure")
        dv, f32, f64, i32, u8 = self.device, torch.float32, torch.float64, torch.int32, torch.uint8
        K, N = (int(v) for v in blocks["qpos"].shape[:2])
        Cc = int(blocks["geom1"].shape[2])
        cb = _abi.A3Blocks()
        cb.K, cb.C = K, Cc
        shapes = dict(qpos=(sp.nq,), qvel=(sp.nv,), act_len=(sp.nu,), act_vel=(sp.nu,), lf_pos=(3,), rf_pos=(3,),
                      lf_vel=(3,), rf_vel=(3,), root_pos=(3,), root_quat=(4,), head_pos=(3,), ncon=(), geom1=(Cc,),
                      geom2=(Cc,), force6=(Cc, 6), cpos_z=(Cc,))
        for name, tail in shapes.items():
            dt = i32 if name in ("ncon", "geom1", "geom2") else f64
            setattr(cb, name, _req(blocks.get(name), name, (K, N) + tail, dt, dv).data_ptr())
        cst = self._a3_struct(_abi.A3State, self._A3_ST, state, N)
        T, nobs, nu = int(ro["T"]), sp.n_obs, sp.nu
        slots, depth = int(ro["side_slots"]), int(ro["pool_depth"])
        det = bool(ro["deterministic"])
        cr = _abi.A3Rollout()
        cr.T, cr.max_traj_len, cr.deterministic = T, int(ro["max_traj_len"]), int(det)
        cr.side_slots, cr.pool_depth = slots, depth
        spec = dict(mu=((N, nu), f32), value=((N,), f32), scale=((nu,), f32), eps=((T, N, nu), f32),
                    state=((N, nobs), f32), pd_target=((N, nu), f64), buf_states=((T, N, nobs), f32),
                    buf_actions=((T, N, nu), f32), buf_rewards=((T, N), f64), buf_values=((T, N), f32),
                    buf_flags=((T, N), u8), buf_rew6=((T, N, 6), f32), traj_len=((N,), i32),
                    side_obs=((N * slots, nobs), f32), side_t=((N * slots,), i32), side_count=((N,), i32),
                    pool=((N * depth * C.sizeof(_abi.A3ResetRecord),), u8), pool_count=((N,), i32),
                    ctr=((self.a3_vec_ctr_len(N),), i32), buf_mu=((T, N, nu), f32))
        optional = {"buf_rew6", "buf_mu"} | ({"scale", "eps"} if det else set())
        for name, (shape, dt) in spec.items():
            tns = _req(ro.get(name), name, shape, dt, dv, optional=name in optional)
            setattr(cr, name, None if tns is None else tns.data_ptr())
        keep = (blocks, state, ro)          # the structs hold raw addresses: keep the tensors alive
        from ._ffi import check, lib
        fn, h = lib().oly_a3_vec_step, self.ctx.handle

        def launch(flags=0, mu=None, value=None):
            if mu is not None:
                cr.mu = _req(mu, "mu", (N, nu), f32, dv).data_ptr()
            if value is not None:
                cr.value = _req(value, "value", (N,), f32, dv).data_ptr()
            rc = fn(h, N, C.byref(cb), C.byref(cst), C.byref(cr), int(flags), self._s())
            if rc:
                check(h, rc, "oly_a3_vec_step")
            return keep
        pfn = lib().oly_a3_rollout_persistent

        def persistent(packed_actor, norm_actor, packed_critic, norm_critic, mu_out=None, value_out=None):
            """The remaining steps of the rollout (device counter t .. T - 1) in ONE launch (K13): per step the
            actor + critic forward on the packed weights, then this same vec step; bit-identical buffers."""
            for name, w, od in (("packed_actor", packed_actor, nu), ("packed_critic", packed_critic, 1)):
                _req(w, name, (self._mlp_floats(nobs, od),), f32, dv)
            if mu_out is not None:
                _req(mu_out, "mu_out", (N, nu), f32, dv)
            if value_out is not None:
                _req(value_out, "value_out", (N,), f32, dv)
            rc = pfn(h, N, C.byref(cb), C.byref(cst), C.byref(cr), nobs, ptr(packed_actor), int(bool(norm_actor)),
                     ptr(packed_critic), int(bool(norm_critic)), ptr(mu_out), ptr(value_out), self._s())
            if rc:
                check(h, rc, "oly_a3_rollout_persistent")
            return keep
        launch.persistent = persistent
        launch.structs = (cb, cst, cr)       # the C structs of this launch (tests call the C entry points with them)
        return launch

    # -------------------------------------------------------------- K23 (reset records drawn on the device)
    def a3_reset_draw(self, pool, base, pool_count, pool_depth, seed, step_height_abs, period):
        """oly_a3_reset_draw: base += pool_count, pool_count = 0 (pool_count None: base as it is), then slot j of
        environment n of the ring `pool` (uint8 [N*pool_depth*656]) holds record(seed, n, base[n] + j).  base [N] i64 and
        pool_count [N] i32 are updated in place.  One launch on the current stream, no synchronisation."""
        dv = self.device
        if not isinstance(base, torch.Tensor) or base.dim() != 1:
            raise OlyError("a3_reset_draw: base is a [N] int64 tensor")
        N, depth, seed = int(base.shape[0]), int(pool_depth), int(seed)
        if N < 1 or depth < 1:
            raise OlyError(f"a3_reset_draw: N = {N}, pool_depth = {depth}")
        if not 0 <= seed < 2 ** 64:
            raise OlyError(f"a3_reset_draw: seed {seed} is not an unsigned 64-bit number")
        h = float(step_height_abs)
        if not h >= 0.0 or int(period) < 0:
            raise OlyError(f"a3_reset_draw: step_height_abs = {h}, period = {period}")
        _req(pool, "pool", (N * depth * C.sizeof(_abi.A3ResetRecord),), torch.uint8, dv)
        _req(base, "base", (N,), torch.int64, dv)
        _req(pool_count, "pool_count", (N,), torch.int32, dv, optional=True)
        self.ctx.call("oly_a3_reset_draw", ptr(pool), N, depth, seed, ptr(base), ptr(pool_count), h, int(period), self._s())
        return pool

    def a3_pd_target(self, action):
        sp = self.a3_spec
        N = int(action.shape[0])
        _req(action, "action", (N, sp.nu), torch.float32, self.device)
        target = self._new((N, sp.nu), torch.float64)
        self.ctx.call("oly_a3_pd_target", N, ptr(action), ptr(target), self._s())
        return target

    def a3_pd_torque(self, kp, kd, target, act_len, act_vel):
        sp = self.a3_spec
        N = int(target.shape[0])
        for t, nme in ((target, "target"), (act_len, "act_len"), (act_vel, "act_vel")):
            _req(t, nme, (N, sp.nu), torch.float64, self.device)
        _req(kp, "kp", (sp.nu,), torch.float64, self.device)
        _req(kd, "kd", (sp.nu,), torch.float64, self.device)
        tau = self._new((N, sp.nu), torch.float64)
        self.ctx.call("oly_a3_pd_torque", N, ptr(kp), ptr(kd), ptr(target), ptr(act_len), ptr(act_vel), ptr(tau),
                      self._s())
        return tau

    # -------------------------------------------------------------- K11 (fused MLP forward)
    def mlp_pack(self, w1, b1, w2, b2, w3, b3, in_mean=None, in_std=None, packed=None):
        """torch Linear parameters of a relu MLP in -> 256 -> 256 -> out -> packed operand stream."""
        from ._ffi import lib
        f32, dv = torch.float32, self.device
        H, in_dim = (int(v) for v in w1.shape)
        out_dim = int(w3.shape[0])
        n = int(lib().oly_mlp_packed_floats(in_dim, H, out_dim))
        if n < 0 or tuple(w2.shape) != (H, H) or int(w3.shape[1]) != H:
            raise OlyError(f"mlp_pack: unsupported MLP shape {in_dim} -> {tuple(w2.shape)} -> {out_dim}")
        for t, name, shape in ((w1, "w1", (H, in_dim)), (b1, "b1", (H,)), (w2, "w2", (H, H)), (b2, "b2", (H,)),
                               (w3, "w3", (out_dim, H)), (b3, "b3", (out_dim,))):
            _req(t, name, shape, f32, dv)
        _req(in_mean, "in_mean", (in_dim,), f32, dv, optional=True)
        _req(in_std, "in_std", (in_dim,), f32, dv, optional=True)
        packed = _req(packed if packed is not None else self._new((n,), f32), "packed", (n,), f32, dv)
        self.ctx.call("oly_mlp_pack", in_dim, H, out_dim, ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(w3), ptr(b3),
                      ptr(in_mean), ptr(in_std), ptr(packed), self._s())
        return packed

    def _mlp_floats(self, in_dim, out_dim):
        key = (int(in_dim), int(out_dim))
        cache = self.__dict__.setdefault("_mlp_sizes", {})
        if key not in cache:
            from ._ffi import lib
            cache[key] = int(lib().oly_mlp_packed_floats(key[0], 256, key[1]))
        return cache[key]

    def mlp_forward2(self, x, packed_a, out_a, y_a, packed_b=None, out_b=0, y_b=None, normalize_a=False,
                     normalize_b=False):
        """y_a = net_a(x) and (optionally) y_b = net_b(x) in one launch; x [N,in] f32."""
        N, in_dim = (int(v) for v in x.shape)
        f32, dv = torch.float32, self.device
        _req(x, "x", (N, in_dim), f32, dv)
        # the raw pointers carry no length: a buffer that is not a whole packed stream is refused here
        _req(packed_a, "packed_a", (self._mlp_floats(in_dim, out_a),), f32, dv)
        _req(y_a, "y_a", (N, int(out_a)), f32, dv)
        if packed_b is not None:
            _req(packed_b, "packed_b", (self._mlp_floats(in_dim, out_b),), f32, dv)
            _req(y_b, "y_b", (N, int(out_b)), f32, dv)
        self.ctx.call("oly_mlp_forward2", N, in_dim, ptr(x), ptr(packed_a), int(out_a), int(bool(normalize_a)), ptr(y_a),
                      ptr(packed_b), int(out_b), int(bool(normalize_b)), ptr(y_b), self._s())
        return y_a, y_b

    # -------------------------------------------------------------- K14 (fused PPO update gradients)
    def ppo_update_plan(self, B, in_dim, act_dim, mirror=False):
        """(workspace floats, parts_actor, parts_critic) for minibatches of B rows on this device."""
        from ._ffi import lib
        pa, pc = C.c_int32(0), C.c_int32(0)
        n = int(lib().oly_ppo_update_ws_floats(self.ctx.handle, int(B), int(in_dim), int(act_dim), int(bool(mirror)),
                                               C.byref(pa), C.byref(pc)))
        if n < 0:
            raise OlyError(f"ppo_update: unsupported shape B={B} in={in_dim} act={act_dim}")
        return n, int(pa.value), int(pc.value)

    def ppo_update_grads(self, obs, action, adv, ret, old_mu, packed_actor, packed_critic, sd, log_sd, old_sd, old_log_sd,
                         grad_actor, grad_critic, scal_out, ws, idx=None, mir_obs=None, act_src=None, act_sign=None,
                         normalize_actor=True, normalize_critic=False, clip=0.2, vf_coeff=0.5, mirror_coeff=0.0,
                         parts=(0, 0), gnorm_ws=None, prepare=False):
        """oly_ppo_update_grads: gradients of one PPO minibatch update (rl/algos/ppo.py:232-282,396-410) into the flat
        buffers grad_actor / grad_critic (parameter order), the six scalars of update_policy into scal_out [6] f64.
        gnorm_ws [1024] f64: the finishing launch also leaves the squared-norm block partials ppo_adam_step(norm_ready=True)
        reads.  prepare=True: validate now, launch nothing, return `launch(idx, scal_out)` for minibatches of the same size
        on the same buffers (no per-call checks: at minibatch 64 they cost more host time than the kernels run)."""
        from ._ffi import lib
        f32, dv = torch.float32, self.device
        if obs.dim() != 2 or action.dim() != 2:
            raise OlyError("ppo_update_grads: obs [n, in] and action [n, act] expected")
        n, in_dim = (int(v) for v in obs.shape)
        act_dim = int(action.shape[1])
        _req(obs, "obs", (n, in_dim), f32, dv)
        _req(action, "action", (n, act_dim), f32, dv)
        _req(adv, "adv", (n,), f32, dv)
        _req(ret, "ret", (n,), f32, dv)
        _req(old_mu, "old_mu", (n, act_dim), f32, dv)
        _req(mir_obs, "mir_obs", (n, in_dim), f32, dv, optional=True)
        if idx is not None:
            if idx.dim() != 1:
                raise OlyError("idx: expected [B]")
            _req(idx, "idx", (int(idx.shape[0]),), torch.int32, dv)
        B = int(idx.shape[0]) if idx is not None else n
        for t, name in ((sd, "sd"), (log_sd, "log_sd"), (old_sd, "old_sd"), (old_log_sd, "old_log_sd")):
            _req(t, name, (act_dim,), f32, dv)
        if mir_obs is not None:
            _req(act_src, "act_src", (act_dim,), torch.int32, dv)
            _req(act_sign, "act_sign", (act_dim,), f32, dv)
        _req(packed_actor, "packed_actor", (self._mlp_floats(in_dim, act_dim),), f32, dv)
        _req(packed_critic, "packed_critic", (self._mlp_floats(in_dim, 1),), f32, dv)
        ga = int(lib().oly_ppo_update_grad_floats(in_dim, 256, act_dim))
        gc = int(lib().oly_ppo_update_grad_floats(in_dim, 256, 1))
        if ga < 0 or gc < 0:
            raise OlyError(f"ppo_update_grads: unsupported shape in={in_dim} act={act_dim}")
        _req(grad_actor, "grad_actor", (ga,), f32, dv)
        _req(grad_critic, "grad_critic", (gc,), f32, dv)
        _req(scal_out, "scal_out", (6,), torch.float64, dv)
        if ws.dim() != 1:
            raise OlyError("ws: expected a flat float32 workspace")
        _req(ws, "ws", (int(ws.shape[0]),), f32, dv)
        u = _abi.PPOUpdate()
        u.B, u.in_dim, u.act_dim = B, in_dim, act_dim
        u.parts_actor, u.parts_critic = int(parts[0]), int(parts[1])
        u.normalize_actor, u.normalize_critic = int(bool(normalize_actor)), int(bool(normalize_critic))
        u.obs, u.mir_obs, u.action, u.adv, u.ret, u.old_mu, u.idx = (ptr(t) for t in (obs, mir_obs, action, adv, ret, old_mu, idx))
        u.packed_actor, u.packed_critic = ptr(packed_actor), ptr(packed_critic)
        u.sd, u.log_sd, u.old_sd, u.old_log_sd = ptr(sd), ptr(log_sd), ptr(old_sd), ptr(old_log_sd)
        u.act_src, u.act_sign = ptr(act_src if mir_obs is not None else None), ptr(act_sign if mir_obs is not None else None)
        u.clip, u.vf_coeff, u.mirror_coeff = float(clip), float(vf_coeff), float(mirror_coeff)
        u.grad_actor, u.grad_critic, u.scal_out = ptr(grad_actor), ptr(grad_critic), ptr(scal_out)
        u.ws, u.ws_floats = ptr(ws), int(ws.shape[0])
        _req(gnorm_ws, "gnorm_ws", (1024,), torch.float64, dv, optional=True)
        u.gnorm_ws = ptr(gnorm_ws)
        if prepare:
            from ._ffi import check
            fn, h = lib().oly_ppo_update_grads, self.ctx.handle
            keep = (obs, action, adv, ret, old_mu, mir_obs, packed_actor, packed_critic, sd, log_sd, old_sd, old_log_sd, act_src,
                    act_sign, grad_actor, grad_critic, ws, gnorm_ws)
            ref = C.byref(u)

            def launch(idx_, scal_):
                if idx_.dtype != torch.int32 or idx_.shape[0] != B or not idx_.is_contiguous():
                    raise OlyError("prepared ppo_update_grads: idx must be a contiguous int32 [B] of the prepared size")
                u.idx, u.scal_out = idx_.data_ptr(), scal_.data_ptr()
                rc = fn(h, ref, self._s())
                if rc:
                    check(h, rc, "oly_ppo_update_grads")
                return keep
            launch.struct, launch.B, launch.keep = u, B, keep
            return launch
        self.ctx.call("oly_ppo_update_grads", C.byref(u), self._s())
        return grad_actor, grad_critic, scal_out

    def ppo_adam_step(self, in_dim, step, lr, eps, max_grad_norm, nets, ws, beta1=0.9, beta2=0.999, norm_ready=False,
                      prepare=False):
        """oly_ppo_adam_step: clip_grad_norm_ + Adam.step + weight re-pack for (actor, critic).  nets: two dicts with
        flat f32 tensors param / grad / exp_avg / exp_avg_sq, out_dim, and optionally packed / in_mean / in_std.
        norm_ready: `ws` already holds the squared-norm partials of these gradients (gnorm_ws of ppo_update_grads).
        prepare=True: validate now, launch nothing, return `launch(step, norm_ready)`."""
        from ._ffi import lib
        f32, dv = torch.float32, self.device
        a = _abi.PPOAdam()
        a.in_dim, a.step = int(in_dim), int(step)
        a.lr, a.beta1, a.beta2, a.eps, a.max_grad_norm = float(lr), float(beta1), float(beta2), float(eps), float(max_grad_norm)
        if len(nets) != 2:
            raise OlyError("ppo_adam_step: nets = (actor, critic)")
        for i, nt in enumerate(nets):
            out_dim = int(nt["out_dim"])
            gf = int(lib().oly_ppo_update_grad_floats(int(in_dim), 256, out_dim))
            if gf < 0:
                raise OlyError(f"ppo_adam_step: unsupported shape in={in_dim} out={out_dim}")
            for k in ("param", "grad", "exp_avg", "exp_avg_sq"):
                _req(nt[k], k, (gf,), f32, dv)
            packed = nt.get("packed")
            if packed is not None:
                _req(packed, "packed", (self._mlp_floats(in_dim, out_dim),), f32, dv)
            _req(nt.get("in_mean"), "in_mean", (int(in_dim),), f32, dv, optional=True)
            _req(nt.get("in_std"), "in_std", (int(in_dim),), f32, dv, optional=True)
            s = a.net[i]
            s.param, s.grad, s.exp_avg, s.exp_avg_sq = ptr(nt["param"]), ptr(nt["grad"]), ptr(nt["exp_avg"]), ptr(nt["exp_avg_sq"])
            s.packed, s.in_mean, s.in_std, s.out_dim = ptr(packed), ptr(nt.get("in_mean")), ptr(nt.get("in_std")), out_dim
        _req(ws, "ws", (1024,), torch.float64, dv)
        a.ws = ptr(ws)
        a.norm_ready = int(bool(norm_ready))
        if prepare:
            from ._ffi import check
            fn, h, ref, keep = lib().oly_ppo_adam_step, self.ctx.handle, C.byref(a), (nets, ws)

            def launch(step_, ready_):
                a.step, a.norm_ready = int(step_), 1 if ready_ else 0
                rc = fn(h, ref, self._s())
                if rc:
                    check(h, rc, "oly_ppo_adam_step")
                return keep
            launch.struct, launch.keep = a, keep
            return launch
        self.ctx.call("oly_ppo_adam_step", C.byref(a), self._s())

    def ppo_update_epoch(self, grads_launch, adam_launch, first_step, perm, n_batches, scal_out):
        """oly_ppo_update_epoch: the minibatch loop of one epoch in one call, from the two prepared launches
        (ppo_update_grads / ppo_adam_step with prepare=True): minibatch b takes rows perm[b B : (b + 1) B], leaves its six
        scalars in scal_out[b] and is optimiser step first_step + b."""
        u, a, B = grads_launch.struct, adam_launch.struct, grads_launch.B
        n_batches = int(n_batches)
        if perm.dim() != 1 or int(perm.shape[0]) < n_batches * B:
            raise OlyError(f"ppo_update_epoch: perm holds {tuple(perm.shape)} indices, {n_batches} minibatches of {B} need {n_batches * B}")
        _req(perm, "perm", (int(perm.shape[0]),), torch.int32, self.device)
        _req(scal_out, "scal_out", (n_batches, 6), torch.float64, self.device)
        a.step = int(first_step)
        self.ctx.call("oly_ppo_update_epoch", C.byref(u), C.byref(a), ptr(perm), n_batches, ptr(scal_out), self._s())

    # -------------------------------------------------------------- K16 (imitation MLP forward, critic fit)
    def ilmlp_pack(self, w1, b1, w2, b2, w3, b3, packed=None):
        """torch Linear parameters of the relu MLP in -> 512 -> 256 -> out -> packed operand stream."""
        from ._ffi import lib
        f32, dv = torch.float32, self.device
        if w1.dim() != 2 or w2.dim() != 2 or w3.dim() != 2:
            raise OlyError("ilmlp_pack: weights must be 2-D")
        h1, in_dim = (int(v) for v in w1.shape)
        h2, out_dim = int(w2.shape[0]), int(w3.shape[0])
        n = int(lib().oly_ilmlp_packed_floats(in_dim, h1, h2, out_dim))
        if n < 0 or int(w2.shape[1]) != h1 or int(w3.shape[1]) != h2:
            raise OlyError(f"ilmlp_pack: unsupported MLP shape {in_dim} -> {h1} -> {tuple(w2.shape)} -> {tuple(w3.shape)}")
        for t, name, shape in ((w1, "w1", (h1, in_dim)), (b1, "b1", (h1,)), (w2, "w2", (h2, h1)), (b2, "b2", (h2,)),
                               (w3, "w3", (out_dim, h2)), (b3, "b3", (out_dim,))):
            _req(t, name, shape, f32, dv)
        packed = _req(packed if packed is not None else self._new((n,), f32), "packed", (n,), f32, dv)
        self.ctx.call("oly_ilmlp_pack", in_dim, h1, h2, out_dim, ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(w3), ptr(b3),
                      ptr(packed), self._s())
        return packed

    def ilmlp_forward(self, x, packed, out_dim, act="identity", colstats=None, mean=None, std=None, y=None):
        """y [N,out] = net(standardise(x)); x [N,in] f32; standardisation from colstats [3,in] f64, or mean / std [in]
        f64, or none.  act: "identity" or "tanh" (the last activation)."""
        from ._ffi import lib
        f32, f64, dv = torch.float32, torch.float64, self.device
        if not isinstance(x, torch.Tensor) or x.dim() != 2:
            raise OlyError("x: expected a [N,in] tensor")
        N, in_dim = (int(v) for v in x.shape)
        out_dim = int(out_dim)
        n = int(lib().oly_ilmlp_packed_floats(in_dim, 512, 256, out_dim))
        if n < 0:
            raise OlyError(f"ilmlp_forward: unsupported shape in={in_dim} out={out_dim}")
        if act not in ("identity", "tanh"):
            raise OlyError(f"ilmlp_forward: last activation {act!r} is not identity or tanh")
        if (mean is None) != (std is None) or (mean is not None and colstats is not None):
            raise OlyError("ilmlp_forward: give colstats, or mean and std, or neither")
        _req(x, "x", (N, in_dim), f32, dv)
        _req(packed, "packed", (n,), f32, dv)
        _req(colstats, "colstats", (3, in_dim), f64, dv, optional=True)
        _req(mean, "mean", (in_dim,), f64, dv, optional=True)
        _req(std, "std", (in_dim,), f64, dv, optional=True)
        y = _req(y if y is not None else self._new((N, out_dim), f32), "y", (N, out_dim), f32, dv)
        self.ctx.call("oly_ilmlp_forward", N, in_dim, out_dim, _abi.ACT_TANH if act == "tanh" else _abi.ACT_IDENTITY,
                      ptr(x), ptr(mean), ptr(std), ptr(colstats), ptr(packed), ptr(y), self._s())
        return y

    def il_critic_fit_ws(self, batch, in_dim):
        """A workspace for il_critic_fit_epoch with minibatches of `batch` rows."""
        from ._ffi import lib
        n = int(lib().oly_il_critic_fit_ws_floats(int(batch), int(in_dim)))
        if n < 0:
            raise OlyError(f"il_critic_fit: unsupported batch={batch} in={in_dim} (0 < batch <= 256, in <= 64)")
        return self._new((n,), torch.float32)

    def il_critic_fit_epoch(self, x, v_target, perm, batch, colstats, param, exp_avg, exp_avg_sq, packed, ws, step,
                            lr, beta1=0.9, beta2=0.999, eps=1e-8, loss_out=None):
        """oly_il_critic_fit_epoch: one epoch of the critic's minibatch loop in one call.  x [n,in] f32 raw rows,
        v_target [n] (or [n,1]) f32, perm [n] int32, param / exp_avg / exp_avg_sq flat in torch order, packed the
        ilmlp_pack stream of param; step = Adam steps taken before.  Returns loss_out [n_batches] f64."""
        from ._ffi import lib
        f32, dv = torch.float32, self.device
        if not isinstance(x, torch.Tensor) or x.dim() != 2:
            raise OlyError("x: expected a [n,in] tensor")
        n, in_dim = (int(v) for v in x.shape)
        batch = int(batch)
        nws = int(lib().oly_il_critic_fit_ws_floats(batch, in_dim))
        if nws < 0:
            raise OlyError(f"il_critic_fit_epoch: unsupported batch={batch} in={in_dim} (0 < batch <= 256, in <= 64)")
        nb = (n + batch - 1) // batch
        n_par = 512 * in_dim + 512 + 256 * 512 + 256 + 256 + 1
        _req(x, "x", (n, in_dim), f32, dv)
        _req(v_target, "v_target", tuple(v_target.shape) if v_target.dim() == 2 and int(v_target.shape[-1]) == 1
             else (n,), f32, dv)
        if v_target.numel() != n:
            raise OlyError(f"v_target: {v_target.numel()} values for {n} rows")
        _req(perm, "perm", (n,), torch.int32, dv)
        _req(colstats, "colstats", (3, in_dim), torch.float64, dv)
        for t, name in ((param, "param"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
            _req(t, name, (n_par,), f32, dv)
        _req(packed, "packed", (int(lib().oly_ilmlp_packed_floats(in_dim, 512, 256, 1)),), f32, dv)
        _req(ws, "ws", (nws,), f32, dv)
        loss_out = _req(loss_out if loss_out is not None else self._new((nb,), torch.float64), "loss_out", (nb,),
                        torch.float64, dv)
        f = _abi.ILCriticFit(in_dim=in_dim, step=int(step), lr=float(lr), beta1=float(beta1), beta2=float(beta2),
                             eps=float(eps), x=x.data_ptr(), v_target=v_target.data_ptr(), colstats=colstats.data_ptr(),
                             param=param.data_ptr(), exp_avg=exp_avg.data_ptr(), exp_avg_sq=exp_avg_sq.data_ptr(),
                             packed=packed.data_ptr(), ws=ws.data_ptr(), ws_floats=nws, loss_out=loss_out.data_ptr())
        self.ctx.call("oly_il_critic_fit_epoch", C.byref(f), ptr(perm), n, batch, self._s())
        return loss_out

    # -------------------------------------------------------------- what the two discriminators' methods share
    # `net` is _VAIL or _GAIL, `name` the public method, which is also its entry point without the oly_ prefix, and
    # `second` None for states only or (x2, mask2, standardise) for a paired input: (s, s') with use_next_states, (s, a)
    # with actions (networks.py:216-234, 258-278).  Every path calls its own entry point.
    def _disc_head(self, name, x, mask, second):
        """x [B,Dx] f32, its mask [Ds] int32 or None (Ds = Dx) and the oly_disc_pair block of `second` -> (B, Dx, Ds,
        block or None, D2 or 0)."""
        if not isinstance(x, torch.Tensor) or x.dim() != 2:
            raise OlyError("x: expected a [B,Dx] tensor")
        B, Dx = (int(v) for v in x.shape)
        _req(x, "x", (B, Dx), torch.float32, self.device)
        Ds = Dx if mask is None else int(mask.shape[0])
        _req(mask, "mask", (Ds,), torch.int32, self.device, optional=True)
        pair, d2 = (None, 0) if second is None else self._disc_pair(name, second[0], second[1], second[2], B, Ds)
        return B, Dx, Ds, pair, d2

    def _disc_pair(self, name, x2, mask2, standardise, rows, Ds):
        """The oly_disc_pair block of x2 [rows, W2] f32 (mask2 [d2] int32 or None) -> (block, d2).  Refused: an empty
        second part, Ds + d2 > 64, next states of another width than the states."""
        f32, dv = torch.float32, self.device
        if not isinstance(x2, torch.Tensor) or x2.dim() != 2:
            raise OlyError(f"{name}: x2: expected a [rows,W2] tensor")
        W2 = int(x2.shape[1])
        _req(x2, "x2", (rows, W2), f32, dv)
        d2 = W2 if mask2 is None else int(mask2.shape[0])
        _req(mask2, "mask2", (d2,), torch.int32, dv, optional=True)
        if d2 <= 0:
            raise OlyError(f"{name}: the second part has no column (D2 == 0)")
        if Ds + d2 > 64:
            raise OlyError(f"{name}: the paired input is {Ds} + {d2} columns wide, the kernels take at most 64")
        if standardise and d2 != Ds:
            raise OlyError(f"{name}: next states have {d2} masked columns, the states {Ds}")
        return _abi.DiscPair(x2=x2.data_ptr(), mask2=ptr(mask2), stride2=W2, d2=d2, standardise=int(bool(standardise))), d2

    def _disc_weights(self, name, net, weights, D):
        """The pointer array of `weights` (the tensors of net.pack in its order, re-packed inside the call) or None."""
        if weights is None:
            return None
        shapes = net.weights(D)
        if len(weights) != len(shapes):
            raise OlyError(f"{name}: weights = the {len(shapes)} tensors of {net.pack}")
        for i, (t, sh) in enumerate(zip(weights, shapes)):
            _req(t, f"weights[{i}]", sh, torch.float32, self.device)
        return (C.c_void_p * len(shapes))(*[t.data_ptr() for t in weights])

    def _disc_outputs(self, name, shapes, want, out):
        """The outputs `want` among `shapes` (the caller's out[k], validated, or fresh) -> (dict, the pointer or None of
        every output in shapes' order)."""
        f32, dv = torch.float32, self.device
        out = dict(out or {})
        if not want:
            raise OlyError(f"{name}: no output requested")
        for k in want:
            if k not in shapes:
                raise OlyError(f"{name}: unknown output {k!r}")
            out[k] = _req(out.get(k) if out.get(k) is not None else self._new(shapes[k], f32), k, shapes[k], f32, dv)
        return out, tuple(ptr(out[k]) if k in want else None for k in shapes)

    def _disc_forward_on(self, net, name, x, packed, mask, stats, second, eps, want, out):
        """A forward on given statistics: stats = (mean, std, colstats) for states only, (stats_a, stats_b) for a pair."""
        f32, f64, dv = torch.float32, torch.float64, self.device
        B, Dx, Ds, pair, d2 = self._disc_head(name, x, mask, second)
        if pair is None:
            mean, std, colstats = stats
            if (mean is None) != (std is None) or (mean is not None and colstats is not None):
                raise OlyError(f"{name}: give mean and std together, or colstats, or neither")
            _req(colstats, "colstats", (3, Ds), f64, dv, optional=True)
            _req(mean, "mean", (Ds,), f64, dv, optional=True)
            _req(std, "std", (Ds,), f64, dv, optional=True)
            stats = (ptr(mean), ptr(std), ptr(colstats))
        else:
            stats_a, stats_b = stats
            _req(stats_a, "stats_a", (3, Ds), f64, dv, optional=True)
            _req(stats_b, "stats_b", (3, Ds), f64, dv, optional=True)
            if second[2] and (stats_a is None) != (stats_b is None):
                raise OlyError(f"{name}: give stats_a and stats_b together")
            stats = (C.byref(pair), ptr(stats_a), ptr(stats_b))
        _req(packed, "packed", (getattr(self, net.packed_floats)(Ds + d2),), f32, dv)   # the raw pointer carries no length
        noise = ()
        if net.noise:
            noise = (ptr(_req(eps, "eps", (B, 128), f32, dv, optional=True)),)
        out, outs = self._disc_outputs(name, net.outputs(B), want, out)
        self.ctx.call("oly_" + name, C.c_int64(B), Dx, Ds, ptr(x), ptr(mask), *stats, ptr(packed), *noise, *outs, self._s())
        return out

    def _disc_reward_step_args(self, net, name, x, packed, colstats, stats_a, mask, second, eps, want, out, weights):
        """A reward step's arguments, validated -> (out, the arguments before `accumulate`, those after it)."""
        f32, f64, dv = torch.float32, torch.float64, self.device
        B, Dx, Ds, pair, d2 = self._disc_head(name, x, mask, second)
        _req(colstats, "colstats", (3, Ds), f64, dv)
        head = (C.c_int64(B), Dx, Ds, ptr(x), ptr(mask))
        if pair is None:
            head += (ptr(colstats),)
        else:
            _req(stats_a, "stats_a", (3, Ds), f64, dv, optional=not second[2])
            head += (C.byref(pair), ptr(colstats), ptr(stats_a))
        _req(packed, "packed", (getattr(self, net.packed_floats)(Ds + d2),), f32, dv)
        noise = ()
        if net.noise:
            noise = (ptr(_req(eps, "eps", (B, 128), f32, dv, optional=True)),)
        wp = self._disc_weights(name, net, weights, Ds + d2)
        out, outs = self._disc_outputs(name, net.outputs(B), want, out)
        return out, head, (wp, ptr(packed), *noise, *outs)

    def _disc_fit_ws_floats(self, net, name, batch, ds, d2=None, standardise=False):
        """The floats of a fit workspace for minibatches of `batch` rows of ds (d2 None) or ds + d2 columns."""
        if d2 is None:
            n = int(getattr(lib(), f"oly_{net.fit}_ws_floats")(int(batch), int(ds)))
            if n < 0:
                raise OlyError(f"{name}: unsupported batch={batch} in={ds} (0 < batch <= 4096, in <= 64)")
            return n
        n = int(getattr(lib(), f"oly_{net.fit}_pair_ws_floats")(int(batch), int(ds), int(d2), int(bool(standardise))))
        if n < 0:
            raise OlyError(f"{name}: unsupported batch={batch}, {ds} + {d2} columns (0 < batch <= 4096, 0 < D2, "
                           "Ds + D2 <= 64, next states as wide as the states)")
        return n

    def _disc_fit_epoch(self, net, name, x, second, n_plcy, perm, batch, colstats, param, exp_avg, exp_avg_sq, packed, ws,
                        step, lr, beta1, beta2, adam_eps, weight_decay, targets, loss_out, bce_out, **own):
        """One epoch of either discriminator's minibatch loop; `own` holds net.fit_scalars and net.fit_tensors."""
        f32, f64, dv = torch.float32, torch.float64, self.device
        n, _, Ds, pair, d2 = self._disc_head(name, x, None, second)
        batch, in_dim = int(batch), Ds + d2
        nws = self._disc_fit_ws_floats(net, name, batch, Ds, *(() if pair is None else (d2, second[2])))
        if not 0 <= int(n_plcy) <= n:
            raise OlyError(f"{name}: n_plcy={n_plcy} outside [0, {n}]")
        nb = (n + batch - 1) // batch
        n_par = net.n_par(in_dim)
        _req(perm, "perm", (n,), torch.int32, dv)
        _req(targets, "targets", (n,), f32, dv, optional=True)
        _req(colstats, "colstats", (3, Ds), f64, dv)
        for t, key in ((param, "param"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
            _req(t, key, (n_par,), f32, dv)
        _req(packed, "packed", (getattr(self, net.packed_floats)(in_dim),), f32, dv)
        _req(ws, "ws", (nws,), f32, dv)
        loss_out = _req(loss_out if loss_out is not None else self._new((nb,), f64), "loss_out", (nb,), f64, dv)
        _req(bce_out, "bce_out", (nb,), f64, dv, optional=True)
        shapes = dict(noise=(n, 128), one=(1,), batches=(nb,))
        for key, shape, dtype, optional in net.fit_tensors:
            _req(own[key], key, shapes[shape], dtype, dv, optional=optional)
        f = net.struct(in_dim=in_dim, n_plcy=int(n_plcy), step=int(step), lr=float(lr), beta1=float(beta1),
                       beta2=float(beta2), adam_eps=float(adam_eps), weight_decay=float(weight_decay), x=x.data_ptr(),
                       targets=ptr(targets), colstats=colstats.data_ptr(), param=param.data_ptr(),
                       exp_avg=exp_avg.data_ptr(), exp_avg_sq=exp_avg_sq.data_ptr(), packed=packed.data_ptr(),
                       ws=ws.data_ptr(), ws_floats=nws, loss_out=loss_out.data_ptr(), bce_out=ptr(bce_out),
                       **{key: float(own[key]) for key in net.fit_scalars},
                       **{key: ptr(own[key]) for key, _, _, _ in net.fit_tensors})
        self.ctx.call("oly_" + name, C.byref(f), *(() if pair is None else (C.byref(pair),)), ptr(perm), n, batch, self._s())
        return loss_out

    # -------------------------------------------------------------- K15 (VAIL discriminator fit), K12 / K15 on a pair
    def _disc_packed_floats(self, D):
        cache = self.__dict__.setdefault("_disc_sizes", {})
        if D not in cache:
            cache[D] = int(lib().oly_disc_packed_floats(D, 256, 128, 128))
        return cache[D]

    def disc_fit_ws(self, batch, in_dim):
        """A workspace for disc_fit_epoch with minibatches of `batch` rows."""
        return self._new((self._disc_fit_ws_floats(_VAIL, "disc_fit", batch, in_dim),), torch.float32)

    def disc_fit_pair_ws(self, batch, ds, d2, standardise):
        """A workspace for disc_fit_epoch_pair with minibatches of `batch` rows."""
        return self._new((self._disc_fit_ws_floats(_VAIL, "disc_fit_pair", batch, ds, d2, standardise),), torch.float32)

    def disc_fit_epoch(self, x, n_plcy, eps, perm, batch, colstats, param, exp_avg, exp_avg_sq, packed, beta, ws, step,
                       lr, beta1=0.9, beta2=0.999, adam_eps=1e-8, weight_decay=0.0, info_constraint=0.1, lr_beta=1e-5,
                       targets=None, loss_out=None, bce_out=None, kl_out=None, beta_out=None):
        """oly_disc_fit_epoch: one epoch of the discriminator's minibatch loop in one call.  x [n,in] f32 the masked
        concatenated rows (policy rows first, n_plcy of them), eps [n,128] f32 noise in minibatch order, perm [n] int32,
        param / exp_avg / exp_avg_sq flat in oly_disc_pack's order, packed the disc_pack stream (re-packed from param,
        then kept current), beta [1] f32 VDBLoss's beta (read and written), targets [n] f32 or None (0 / 1); step =
        Adam steps taken before.  Returns loss_out [n_batches] f64 (bce_out, kl_out f64 and beta_out f32 likewise
        when given)."""
        return self._disc_fit_epoch(_VAIL, "disc_fit_epoch", x, None, n_plcy, perm, batch, colstats, param, exp_avg,
                                    exp_avg_sq, packed, ws, step, lr, beta1, beta2, adam_eps, weight_decay, targets,
                                    loss_out, bce_out, eps=eps, beta=beta, info_constraint=info_constraint,
                                    lr_beta=lr_beta, kl_out=kl_out, beta_out=beta_out)

    def disc_fit_epoch_pair(self, x, x2, standardise, n_plcy, eps, perm, batch, colstats, param, exp_avg, exp_avg_sq, packed,
                            beta, ws, step, lr, beta1=0.9, beta2=0.999, adam_eps=1e-8, weight_decay=0.0,
                            info_constraint=0.1, lr_beta=1e-5, targets=None, loss_out=None, bce_out=None, kl_out=None,
                            beta_out=None):
        """oly_disc_fit_epoch_pair: disc_fit_epoch on the paired rows x [n,Ds] | x2 [n,D2] (both masked and concatenated,
        policy rows first); colstats [3,Ds]; param / moments for in = Ds + D2."""
        return self._disc_fit_epoch(_VAIL, "disc_fit_epoch_pair", x, (x2, None, standardise), n_plcy, perm, batch, colstats,
                                    param, exp_avg, exp_avg_sq, packed, ws, step, lr, beta1, beta2, adam_eps, weight_decay,
                                    targets, loss_out, bce_out, eps=eps, beta=beta, info_constraint=info_constraint,
                                    lr_beta=lr_beta, kl_out=kl_out, beta_out=beta_out)

    def disc_forward_pair(self, x, x2, packed, standardise, mask=None, mask2=None, stats_a=None, stats_b=None, eps=None,
                          want=("reward",), out=None):
        """oly_disc_forward_pair: disc_forward on [ standardise(x[:, mask]) | second ], second = standardise(x2[:, mask2])
        with stats_b (standardise: next states) or x2[:, mask2] raw (actions).  stats_a / stats_b [3,Ds] f64 running sums,
        or both None (nothing is standardised)."""
        return self._disc_forward_on(_VAIL, "disc_forward_pair", x, packed, mask, (stats_a, stats_b),
                                     (x2, mask2, standardise), eps, want, out)

    def disc_reward_step_pair(self, x, x2, packed, colstats, stats_a, accumulate, standardise, mask=None, mask2=None,
                              eps=None, want=("reward",), out=None, weights=None):
        """oly_disc_reward_step_pair: the Standardizer's update with x's masked rows (colstats [3,Ds]; that result kept in
        stats_a [3,Ds]), for next states its second update with x2's masked rows, then the paired forward on both, one C
        call without a host synchronisation.  accumulate=None: validate now and return `launch(accumulate)`."""
        out, head, tail = self._disc_reward_step_args(_VAIL, "disc_reward_step_pair", x, packed, colstats, stats_a, mask,
                                                      (x2, mask2, standardise), eps, want, out, weights)
        if accumulate is None:
            from ._ffi import check
            fn, h = lib().oly_disc_reward_step_pair, self.ctx.handle
            keep = (x, x2, mask, mask2, colstats, stats_a, packed, eps, weights, out)

            def launch(acc):
                rc = fn(h, *head, 1 if acc else 0, *tail, self._s())
                if rc:
                    check(h, rc, "oly_disc_reward_step_pair")
                return keep[-1]
            return launch
        self.ctx.call("oly_disc_reward_step_pair", *head, int(bool(accumulate)), *tail, self._s())
        return out

    # -------------------------------------------------------------- K24 (behavioural cloning: targets, fit)
    def bc_targets(self, actions, central, delta, out=None):
        """oly_bc_targets: atanh(clip((actions - central) / delta, -+0.99999988)) for the whole table in one launch
        (behavioral_cloning.py:63-66).  actions [n,A] f32, central / delta [A] f32; returns targets [n,A] f32."""
        f32, dv = torch.float32, self.device
        if not isinstance(actions, torch.Tensor) or actions.dim() != 2:
            raise OlyError("bc_targets: actions is a [n,A] tensor")
        n, A = (int(v) for v in actions.shape)
        if not 0 < A <= _abi.OLY_BC_MAX_ACT:
            raise OlyError(f"bc_targets: unsupported act_dim={A} (0 < act_dim <= {_abi.OLY_BC_MAX_ACT})")
        _req(actions, "actions", (n, A), f32, dv)
        _req(central, "central", (A,), f32, dv)
        _req(delta, "delta", (A,), f32, dv)
        out = _req(out if out is not None else self._new((n, A), f32), "targets", (n, A), f32, dv)
        self.ctx.call("oly_bc_targets", C.c_int64(n), A, ptr(actions), ptr(central), ptr(delta), ptr(out), self._s())
        return out

    def bc_fit_ws(self, batch, in_dim, act_dim):
        """A workspace for bc_fit_steps with minibatches of `batch` rows."""
        from ._ffi import lib
        n = int(lib().oly_bc_fit_ws(int(batch), int(in_dim), int(act_dim)))
        if n < 0:
            raise OlyError(f"bc_fit: unsupported batch={batch} in={in_dim} act={act_dim} (0 < batch <= "
                           f"{_abi.OLY_BC_MAX_BATCH}, in <= 64, act <= {_abi.OLY_BC_MAX_ACT})")
        return self._new((n,), torch.float32)

    def _bc_rows(self, name, states, targets, pair):
        """The row and target widths of a K24 fit and its oly_bc_pair: (in_dim, A, BCPair or None).  pair: None, or
        dict(x2 [n,stride2] f32, actions [n,A] f32, central [A] f32, delta [A] f32, d1=stride1, d2=stride2): the rows are
        (states[i, :d1] | x2[i, :d2]) and the targets are formed from the raw actions in the kernel (targets None)."""
        f32, dv = torch.float32, self.device
        if not isinstance(states, torch.Tensor) or states.dim() != 2:
            raise OlyError(f"{name}: states is a [n,in] tensor")
        n, s1 = (int(t) for t in states.shape)
        _req(states, "states", (n, s1), f32, dv)
        if pair is None:
            if not isinstance(targets, torch.Tensor) or targets.dim() != 2:
                raise OlyError(f"{name}: targets is a [n,A] tensor")
            _req(targets, "targets", (n, int(targets.shape[1])), f32, dv)
            return s1, int(targets.shape[1]), None
        if targets is not None:
            raise OlyError(f"{name}: with pair the targets are formed from pair['actions'] (targets must be None)")
        unknown = set(pair) - {"x2", "actions", "central", "delta", "d1", "d2"}
        if unknown:
            raise OlyError(f"{name}: unknown pair entries {sorted(unknown)}")
        x2, actions = pair.get("x2"), pair.get("actions")
        if not isinstance(x2, torch.Tensor) or x2.dim() != 2 or not isinstance(actions, torch.Tensor) or actions.dim() != 2:
            raise OlyError(f"{name}: pair needs x2 [n,stride2] and actions [n,A] tensors")
        s2, A = int(x2.shape[1]), int(actions.shape[1])
        d1, d2 = int(pair.get("d1") or s1), int(pair.get("d2") or s2)
        if not (1 <= d1 <= s1 and 1 <= d2 <= s2):
            raise OlyError(f"{name}: pair widths d1={d1} (1 .. {s1}), d2={d2} (1 .. {s2})")
        _req(x2, "pair.x2", (n, s2), f32, dv)
        _req(actions, "pair.actions", (n, A), f32, dv)
        _req(pair.get("central"), "pair.central", (A,), f32, dv)
        _req(pair.get("delta"), "pair.delta", (A,), f32, dv)
        bp = _abi.BCPair(d1=d1, d2=d2, stride1=s1, stride2=s2, x2=x2.data_ptr(), actions=actions.data_ptr(),
                         central=pair["central"].data_ptr(), delta=pair["delta"].data_ptr())
        return d1 + d2, A, bp

    def bc_fit_steps(self, states, targets, idx, colstats, param, m, v, packed, ws, step, lr, beta1=0.9, beta2=0.999,
                     eps=1e-8, weight_decay=0.0, log_std_min=-20.0, log_std_max=2.0, nll_eps=1e-6, out=None, pair=None):
        """oly_bc_fit_steps: idx.shape[0] iterations of BehavioralCloning.fit_offline in one call.  states [n,in] f32 raw
        rows, targets [n,A] f32 (bc_targets), idx [n_steps,batch] int32 the rows of every step, colstats [3,in] f64 the
        Standardizer's running sums or None (no Standardizer), param / m / v flat in torch order (W1 | b1 | W2 | b2 |
        W3 [2A,256] | b3), packed the ilmlp_pack stream (re-packed from param, then kept current); step = Adam steps
        taken before.  pair (see _bc_rows; targets None): the rows of two tables indexed by idx, in = d1 + d2, and the
        targets from the raw actions, the fit of the inverse action model on a replay ring.
        Returns out [n_steps,3] f64: the loss, the Gaussian entropy, the mean squared error."""
        from ._ffi import lib
        f32, f64, dv = torch.float32, torch.float64, self.device
        in_dim, A, bp = self._bc_rows("bc_fit_steps", states, targets, pair)
        if not isinstance(idx, torch.Tensor) or idx.dim() != 2:
            raise OlyError("bc_fit_steps: idx is a [n_steps,batch] tensor")
        n = int(states.shape[0])
        n_steps, batch = (int(t) for t in idx.shape)
        nws = int(lib().oly_bc_fit_ws(batch, in_dim, A))
        if nws < 0 or n < 1:
            raise OlyError(f"bc_fit_steps: unsupported batch={batch} in={in_dim} act={A} n={n} (0 < batch <= "
                           f"{_abi.OLY_BC_MAX_BATCH}, in <= 64, act <= {_abi.OLY_BC_MAX_ACT}, n >= 1)")
        if not float(log_std_min) <= float(log_std_max) or not float(nll_eps) > 0.0:
            raise OlyError("bc_fit_steps: log_std_min <= log_std_max and nll_eps > 0 are required")
        n_par = 512 * in_dim + 512 + 256 * 512 + 256 + 2 * A * 256 + 2 * A
        _req(idx, "idx", (n_steps, batch), torch.int32, dv)
        _req(colstats, "colstats", (3, in_dim), f64, dv, optional=True)
        for t, name in ((param, "param"), (m, "m"), (v, "v")):
            _req(t, name, (n_par,), f32, dv)
        npk = int(lib().oly_ilmlp_packed_floats(in_dim, 512, 256, 2 * A))
        _req(packed, "packed", (npk,), f32, dv)
        _req(ws, "ws", (nws,), f32, dv)
        out = _req(out if out is not None else self._new((n_steps, 3), f64), "out", (n_steps, 3), f64, dv)
        if n_steps == 0:
            return out
        f = _abi.BCFit(in_dim=in_dim, act_dim=A, batch=batch, n_rows=n, step=int(step), lr=float(lr), beta1=float(beta1),
                       beta2=float(beta2), eps=float(eps), weight_decay=float(weight_decay),
                       log_std_min=float(log_std_min), log_std_max=float(log_std_max), nll_eps=float(nll_eps),
                       states=states.data_ptr(), targets=ptr(targets), idx=idx.data_ptr(), colstats=ptr(colstats),
                       param=param.data_ptr(), m=m.data_ptr(), v=v.data_ptr(), packed=packed.data_ptr(),
                       ws=ws.data_ptr(), ws_floats=nws, out=out.data_ptr(), pair=C.pointer(bp) if bp else None)
        self.ctx.call("oly_bc_fit_steps", C.byref(f), n_steps, self._s())
        return out

    def bc_fit_log_ws(self, batch, in_dim, act_dim):
        """A workspace for bc_fit_steps_log with minibatches of `batch` rows."""
        from ._ffi import lib
        n = int(lib().oly_bc_fit_log_ws(int(batch), int(in_dim), int(act_dim)))
        if n < 0:
            raise OlyError(f"bc_fit: unsupported batch={batch} in={in_dim} act={act_dim} (0 < batch <= "
                           f"{_abi.OLY_BC_MAX_BATCH}, in <= 64, act <= {_abi.OLY_BC_MAX_ACT})")
        return self._new((n,), torch.float32)

    @staticmethod
    def bc_logged_steps(n_steps, logging_iter, iter0):
        """The steps s < n_steps of a call that log: (iter0 + s) % logging_iter == 0."""
        return [s for s in range(int(n_steps)) if (int(iter0) + s) % int(logging_iter) == 0]

    def bc_fit_steps_log(self, states, targets, idx, colstats, param, m, v, packed, ws, step, lr, logging_iter, iter0, noise,
                         beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, log_std_min=-20.0, log_std_max=2.0,
                         nll_eps=1e-6, out=None, pair=None):
        """oly_bc_fit_steps_log: bc_fit_steps with the sampled second forward of BehavioralCloning.logging() on every
        step s with (iter0 + s) % logging_iter == 0.  noise [n_logged, batch, A] f32: the standard normal draws of the
        logging steps in order; ws from bc_fit_log_ws.  Returns out [n_steps,4] f64: bc_fit_steps' three scalars and
        -mean(log_prob); column 3 of a step that does not log is not written (NaN in a buffer made here).  pair: as
        bc_fit_steps'."""
        from ._ffi import lib
        f32, f64, dv = torch.float32, torch.float64, self.device
        in_dim, A, bp = self._bc_rows("bc_fit_steps_log", states, targets, pair)
        if not isinstance(idx, torch.Tensor) or idx.dim() != 2:
            raise OlyError("bc_fit_steps_log: idx is a [n_steps,batch] tensor")
        n = int(states.shape[0])
        n_steps, batch = (int(t) for t in idx.shape)
        nws = int(lib().oly_bc_fit_log_ws(batch, in_dim, A))
        if nws < 0 or n < 1:
            raise OlyError(f"bc_fit_steps_log: unsupported batch={batch} in={in_dim} act={A} n={n} (0 < batch <= "
                           f"{_abi.OLY_BC_MAX_BATCH}, in <= 64, act <= {_abi.OLY_BC_MAX_ACT}, n >= 1)")
        if not float(log_std_min) <= float(log_std_max) or not float(nll_eps) > 0.0:
            raise OlyError("bc_fit_steps_log: log_std_min <= log_std_max and nll_eps > 0 are required")
        if int(logging_iter) < 1 or int(iter0) < 0:
            raise OlyError(f"bc_fit_steps_log: logging_iter={logging_iter} (>= 1), iter0={iter0} (>= 0)")
        n_logged = len(self.bc_logged_steps(n_steps, logging_iter, iter0))
        n_par = 512 * in_dim + 512 + 256 * 512 + 256 + 2 * A * 256 + 2 * A
        _req(idx, "idx", (n_steps, batch), torch.int32, dv)
        _req(colstats, "colstats", (3, in_dim), f64, dv, optional=True)
        for t, name in ((param, "param"), (m, "m"), (v, "v")):
            _req(t, name, (n_par,), f32, dv)
        npk = int(lib().oly_ilmlp_packed_floats(in_dim, 512, 256, 2 * A))
        _req(packed, "packed", (npk,), f32, dv)
        _req(ws, "ws", (nws,), f32, dv)
        _req(noise, "noise", (n_logged, batch, A), f32, dv, optional=n_logged == 0)
        if out is None:
            out = torch.full((n_steps, 4), float("nan"), dtype=f64, device=dv)
        _req(out, "out", (n_steps, 4), f64, dv)
        if n_steps == 0:
            return out
        fit = _abi.BCFit(in_dim=in_dim, act_dim=A, batch=batch, n_rows=n, step=int(step), lr=float(lr), beta1=float(beta1),
                         beta2=float(beta2), eps=float(eps), weight_decay=float(weight_decay),
                         log_std_min=float(log_std_min), log_std_max=float(log_std_max), nll_eps=float(nll_eps),
                         states=states.data_ptr(), targets=ptr(targets), idx=idx.data_ptr(), colstats=ptr(colstats),
                         param=param.data_ptr(), m=m.data_ptr(), v=v.data_ptr(), packed=packed.data_ptr(),
                         ws=ws.data_ptr(), ws_floats=nws, out=out.data_ptr(), pair=C.pointer(bp) if bp else None)
        f = _abi.BCFitLog(fit=fit, logging_iter=int(logging_iter), iter0=int(iter0), eps=ptr(noise))
        self.ctx.call("oly_bc_fit_steps_log", C.byref(f), n_steps, self._s())
        return out

    # -------------------------------------------------------------- K25 (the squashed-Gaussian act and log-probability)
    def sg_act(self, x, packed, central, delta, colstats=None, eps=None, update_stats=True, log_std_min=-20.0,
               log_std_max=2.0, want=("log_prob",), ctrl_f64=False, out=None, x2=None, idx=None, clip=None, d1=None,
               d2=None):
        """oly_sg_act: compute_action_and_log_prob (iq_sac.py:102-151) on x [n,in] f32 in one call.  colstats [3,in] f64
        takes the rows first (update_stats) and standardises them, None: no Standardizer.  packed: ilmlp_pack's stream of
        the network in -> 512 -> 256 -> 2A; central / delta [A] f32; eps [n,A] f32 (None: the squashed mean).  want: which
        of "log_prob" [n], "mu" [n,A], "log_sigma" [n,A] (clamped), "ctrl" [n,nu] (il_ctrl of the action, from the
        configured model) to return beside "action" [n,A].  Returns a dict (absent outputs None); `out` may supply the
        buffers.  No synchronisation.
        x2 [rows,stride2] f32 / idx [n] int32 / clip (lo [A], hi [A]) f64 / d1 / d2: the inverse action model's draw.  Row r
        is (x[i, :d1] | x2[i, :d2]), i = idx[r] (None: r), d1 / d2 default to the tables' widths, in = d1 + d2 and
        colstats [3,in]; the action is clipped in float64, np.clip(action, lo, hi), before it is stored."""
        from ._ffi import lib
        f32, f64, dv = torch.float32, torch.float64, self.device
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or not isinstance(central, torch.Tensor) or central.dim() != 1:
            raise OlyError("sg_act: x [n,in] and central [A] must be tensors")
        n, D = (int(v) for v in x.shape)
        A = int(central.shape[0])
        paired = x2 is not None or idx is not None or clip is not None or d1 is not None or d2 is not None
        rows, s1, s2, w2 = n, D, 0, 0
        if paired:
            if x2 is not None and (not isinstance(x2, torch.Tensor) or x2.dim() != 2 or x2.shape[0] != rows):
                raise OlyError(f"sg_act: x2 is a [{rows},stride2] tensor")
            if x2 is None and d2:
                raise OlyError("sg_act: d2 without x2")
            s2 = int(x2.shape[1]) if x2 is not None else 0
            w1, w2 = int(d1 or s1), int(d2 or s2)
            if not 1 <= w1 <= s1 or not (x2 is None or 1 <= w2 <= s2):
                raise OlyError(f"sg_act: widths d1={w1} (1 .. {s1}), d2={w2} (1 .. {s2})")
            D = w1 + w2
            if idx is not None:
                if not isinstance(idx, torch.Tensor) or idx.dim() != 1:
                    raise OlyError("sg_act: idx is a [n] int32 tensor")
                n = int(idx.shape[0])
                _req(idx, "idx", (n,), torch.int32, dv)
            if clip is not None:
                _req(clip[0], "clip lo", (A,), f64, dv)
                _req(clip[1], "clip hi", (A,), f64, dv)
        if n < 1:
            raise OlyError(f"sg_act: n={n} rows (n >= 1)")
        if not 0 < D <= 64 or not 0 < A <= _abi.OLY_BC_MAX_ACT:
            raise OlyError(f"sg_act: unsupported shape in={D} act={A} (in <= 64, act <= {_abi.OLY_BC_MAX_ACT})")
        if not float(log_std_min) <= float(log_std_max):
            raise OlyError("sg_act: log_std_min <= log_std_max is required")
        unknown = set(want) - {"log_prob", "mu", "log_sigma", "ctrl"}
        if unknown:
            raise OlyError(f"sg_act: unknown outputs {sorted(unknown)}")
        if colstats is None and update_stats:
            update_stats = False
        npk = int(lib().oly_ilmlp_packed_floats(D, 512, 256, 2 * A))
        _req(x, "x", (rows, s1), f32, dv)
        _req(x2, "x2", (rows, s2), f32, dv, optional=True)
        _req(packed, "packed", (npk,), f32, dv)
        _req(central, "central", (A,), f32, dv)
        _req(delta, "delta", (A,), f32, dv)
        _req(colstats, "colstats", (3, D), f64, dv, optional=True)
        _req(eps, "eps", (n, A), f32, dv, optional=True)
        nu = 0
        if "ctrl" in want:
            sp = self.il_spec
            if sp is None:
                raise OlyError("sg_act: ctrl before il_configure")
            if int(sp.n_act) != A:
                raise OlyError(f"sg_act: ctrl for {A} actions, the configured model has n_act={sp.n_act}")
            nu = int(sp.nu)
        out = out or {}
        cd = f64 if ctrl_f64 else f32
        o = dict(action=self._out(out, "action", (n, A), f32),
                 log_prob=self._out(out, "log_prob", (n,), f32) if "log_prob" in want else None,
                 mu=self._out(out, "mu", (n, A), f32) if "mu" in want else None,
                 log_sigma=self._out(out, "log_sigma", (n, A), f32) if "log_sigma" in want else None,
                 ctrl=self._out(out, "ctrl", (n, nu), cd) if "ctrl" in want else None)
        f = _abi.SGAct(n=n, in_dim=D, act_dim=A, update_stats=int(bool(update_stats)), x=x.data_ptr(),
                       colstats=ptr(colstats), packed=packed.data_ptr(), log_std_min=float(log_std_min),
                       log_std_max=float(log_std_max), central=central.data_ptr(), delta=delta.data_ptr(), eps=ptr(eps),
                       action=o["action"].data_ptr(), log_prob=ptr(o["log_prob"]), mu=ptr(o["mu"]),
                       log_sigma=ptr(o["log_sigma"]), ctrl=ptr(o["ctrl"]),
                       out_flags=_abi.OUT_CTRL_F64 if ("ctrl" in want and ctrl_f64) else 0, pad=0)
        if paired:
            f.x2, f.d2, f.stride1, f.stride2 = ptr(x2), w2, s1, s2
            f.idx, f.n_rows = ptr(idx), rows
            f.clip_lo, f.clip_hi = (ptr(clip[0]), ptr(clip[1])) if clip is not None else (None, None)
        self.ctx.call("oly_sg_act", C.byref(f), self._s())
        return o

    # -------------------------------------------------------------- K26 (the soft-Q critic update of IQ-Learn / SQIL)
    def iq_q_ws(self, batch, in_dim, act_dim):
        """A workspace for iq_q_update with batches of `batch` rows."""
        from ._ffi import lib
        n = int(lib().oly_iq_q_ws(int(batch), int(in_dim), int(act_dim)))
        if n < 0:
            raise OlyError(f"iq_q_update: unsupported batch={batch} in={in_dim} act={act_dim} (2 <= batch <= "
                           f"{_abi.OLY_BC_MAX_BATCH}, act <= {_abi.OLY_BC_MAX_ACT}, in + act <= 64)")
        return self._new((n,), torch.float32)

    def iq_q_update(self, obs, act, next_obs, absorbing, a_next, logp_next, a_pi, logp_pi, n_policy, colstats,
                    target_colstats, param, m, v, packed, target_param, target_packed, ws, step, lr, algo="iq",
                    plcy_loss_mode="value", regularizer_mode="exp_and_plcy", treat_absorbing=False, use_target=True,
                    update_target=True, gamma=0.99, alpha=1e-3, reg_mult=0.5, R_min=0.0, R_max=1.0, tau=0.005, beta1=0.9,
                    beta2=0.999, eps=1e-8, weight_decay=0.0, gradient_penalty_lambda=0.0, out=None, lsiq=None, v0=None,
                    all_expert=False):
        """oly_iq_q_update: one update_Q_function and _update_all_targets of IQ_SAC (algo "iq"), SQIL ("sqil") or LSIQ
        ("lsiq").  obs /
        next_obs [B,in] f32, act / a_next / a_pi [B,A] f32, absorbing / logp_next / logp_pi [B] f32; rows [0, n_policy)
        are the policy's, the rest the expert's.  colstats / target_colstats [3,in+A] f64 or None; param / m / v /
        target_param flat in torch order (W1 [512,in+A] | b1 | W2 | b2 | W3 [1,256] | b3); packed / target_packed their
        ilmlp_pack streams, kept current by the call; step = Adam steps taken before.  a_pi / logp_pi may be None for
        SQIL's plcy mode.  lsiq (algo "lsiq" only, required there): dict(lossQ_type "iq_like" | "sqil_like", loss_mode_exp
        "fix" | "bootstrap", Q_exp_loss None | "MSE" | "Huber", target_clipping, Q_min, Q_max), LSIQ's keywords;
        plcy_loss_mode is then one of _abi.LSIQ_PLCY_LOSS_MODES (iq_like) or _abi.LSIQ_SQIL_LIKE_MODES (sqil_like).  With
        sqil_like / value_plcy a_pi is [n_policy, A] and logp_pi [n_policy]; with sqil_like / q_old_policy both may be
        None.
        algo "lsiq_h" is the H update of LSIQ_H / LSIQ_HC (update_H_function): param .. target_packed, colstats,
        target_colstats, lr and tau are H's network, a_next / logp_next the update's own policy pass on next_obs, a_pi /
        logp_pi are not read (None), use_target must hold and plcy_loss_mode / regularizer_mode keep their defaults.
        The lsiq block then also takes h=dict(loss "MSE" | "Huber", cost (False: LSIQ_H's target, True: LSIQ_HC's),
        clip_expert, tau_up, tau_down, max_state [2] f32 (the running maximum and its flag, on the device; needed with
        clip_expert), q_t / v_t [B] f32 (Q_target(obs | act), Q_target(obs | a_pi); needed with cost)); out holds
        _abi.LSIQ_H_TAGS in its first nine slots.
        v0=(a_v0 [B - n_policy, A], logp_v0 [B - n_policy]) f32, the policy's OWN draw on the expert rows' obs, goes with
        plcy_loss_mode "v0" (algo "iq", or "lsiq" with iq_like) and is required there: the fourth pass
        Q_v0 = critic(obs[expert] | a_v0) carries Loss2 = mean(f32(1 - gamma) (Q_v0 - alpha logp_v0)), the pass on
        (obs | a_pi) feeds the Standardizer and the logged V alone.  all_expert=True (same algorithms) permits
        n_policy == 0, the offline agents' batches; the modes that average over policy rows are refused with it and the
        policy subset's scalars come out NaN.
        Returns out [16] f64 (_abi.IQ_Q_TAGS).  No synchronisation."""
        from ._ffi import lib
        f32, f64, dv = torch.float32, torch.float64, self.device
        if not isinstance(obs, torch.Tensor) or obs.dim() != 2 or not isinstance(act, torch.Tensor) or act.dim() != 2:
            raise OlyError("iq_q_update: obs [B,in] and act [B,A] must be tensors")
        B, in_dim = (int(t) for t in obs.shape)
        A = int(act.shape[1])
        nws = int(lib().oly_iq_q_ws(B, in_dim, A))
        if nws < 0:
            raise OlyError(f"iq_q_update: unsupported batch={B} in={in_dim} act={A} (2 <= batch <= "
                           f"{_abi.OLY_BC_MAX_BATCH}, act <= {_abi.OLY_BC_MAX_ACT}, in + act <= 64)")
        if not (0 if all_expert else 1) <= int(n_policy) < B:
            raise OlyError(f"iq_q_update: n_policy={n_policy} outside [1, {B}) (0 takes all_expert=True)")
        if algo not in _abi.IQ_ALGO:
            raise OlyError(f"iq_q_update: unknown algorithm {algo!r}")
        modes = _abi.IQ_PLCY_LOSS_MODES if algo == "iq" else _abi.SQIL_PLCY_LOSS_MODES
        block, sqil_like, hb = None, False, algo == "lsiq_h"
        if algo in ("lsiq", "lsiq_h"):
            if lsiq is None:
                raise OlyError(f"iq_q_update: algo {algo!r} needs the lsiq block")
            ls = dict(lossQ_type="iq_like", loss_mode_exp="fix", Q_exp_loss=None, target_clipping=True, Q_min=-1.0, Q_max=1.0)
            if hb:
                ls["h"] = None
            unknown = set(lsiq) - set(ls)
            if unknown:
                raise OlyError(f"iq_q_update: the lsiq block has unknown entries {sorted(unknown)}")
            ls.update(lsiq)
            for key, table in (("lossQ_type", _abi.LSIQ_LOSSQ_TYPES), ("loss_mode_exp", _abi.LSIQ_LOSS_MODES_EXP),
                               ("Q_exp_loss", _abi.LSIQ_Q_EXP_LOSSES)):
                if ls[key] not in table:
                    raise OlyError(f"iq_q_update: {key} {ls[key]!r} is not one of {list(table)}")
            sqil_like = ls["lossQ_type"] == "sqil_like" and not hb
            if not hb and ls["Q_exp_loss"] is None and (ls["lossQ_type"] == "sqil_like" or ls["loss_mode_exp"] == "fix"):
                raise OlyError("iq_q_update: loss_mode_exp 'fix' and lossQ_type 'sqil_like' need Q_exp_loss 'MSE' or 'Huber'")
            if not float(ls["Q_min"]) < float(ls["Q_max"]):
                raise OlyError(f"iq_q_update: Q_min={ls['Q_min']} must lie below Q_max={ls['Q_max']}")
            modes = _abi.LSIQ_SQIL_LIKE_MODES if sqil_like else _abi.LSIQ_PLCY_LOSS_MODES
            if sqil_like and plcy_loss_mode == "value" and 2 * int(n_policy) != B:
                raise OlyError(f"iq_q_update: sqil_like with plcy_loss_mode 'value' needs 2 n_policy == batch (got "
                               f"{n_policy} of {B})")
            block = _abi.LSIQ(lossQ_type=_abi.LSIQ_LOSSQ_TYPES[ls["lossQ_type"]],
                              loss_mode_exp=_abi.LSIQ_LOSS_MODES_EXP[ls["loss_mode_exp"]],
                              Q_exp_loss=_abi.LSIQ_Q_EXP_LOSSES[ls["Q_exp_loss"]],
                              target_clipping=int(bool(ls["target_clipping"])), Q_min=float(ls["Q_min"]),
                              Q_max=float(ls["Q_max"]))
            if hb:
                hd = dict(loss="MSE", cost=False, clip_expert=True, tau_up=1e-2, tau_down=1e-4, max_state=None, q_t=None,
                          v_t=None)
                given = ls["h"]
                if not isinstance(given, dict) or set(given) - set(hd):
                    raise OlyError(f"iq_q_update: algo 'lsiq_h' needs lsiq['h'], a dict with entries among {sorted(hd)}")
                hd.update(given)
                if hd["loss"] not in _abi.LSIQ_H_LOSSES:
                    raise OlyError(f"iq_q_update: h loss {hd['loss']!r} is not one of {list(_abi.LSIQ_H_LOSSES)}")
                for key in ("tau_up", "tau_down"):
                    if not 0.0 <= float(hd[key]) <= 1.0:
                        raise OlyError(f"iq_q_update: h {key}={hd[key]} outside [0, 1]")
                if not use_target:
                    raise OlyError("iq_q_update: the H update needs use_target")
                if plcy_loss_mode != "value" or regularizer_mode != "exp_and_plcy":
                    raise OlyError("iq_q_update: the H update takes no plcy_loss_mode or regularizer_mode")
                if bool(hd["cost"]) and not float(reg_mult) > 0.0:
                    raise OlyError("iq_q_update: the H update's cost needs reg_mult > 0")
                _req(hd["max_state"], "h max_state", (2,), f32, dv, optional=not hd["clip_expert"])
                _req(hd["q_t"], "h q_t", (B,), f32, dv, optional=not hd["cost"])
                _req(hd["v_t"], "h v_t", (B,), f32, dv, optional=not hd["cost"])
                block.h_loss, block.h_cost = _abi.LSIQ_H_LOSSES[hd["loss"]], int(bool(hd["cost"]))
                block.h_clip_expert = int(bool(hd["clip_expert"]))
                block.h_tau_up, block.h_tau_down = float(hd["tau_up"]), float(hd["tau_down"])
                block.h_max_state, block.h_q_t, block.h_v_t = ptr(hd["max_state"]), ptr(hd["q_t"]), ptr(hd["v_t"])
        elif lsiq is not None:
            raise OlyError(f"iq_q_update: the lsiq block goes with algo 'lsiq', not {algo!r}")
        v0_family = algo == "iq" or (algo == "lsiq" and not sqil_like)
        if (v0 is not None or all_expert) and not v0_family:
            raise OlyError("iq_q_update: v0 and all_expert go with algo 'iq' and with 'lsiq' / iq_like alone")
        if plcy_loss_mode not in modes or (v0_family and plcy_loss_mode == "v0" and v0 is None):
            raise OlyError(f"iq_q_update: plcy_loss_mode {plcy_loss_mode!r} is not one of "
                           f"{[k for k in modes if k != 'v0']} (v0 is not built without v0=(a_v0, logp_v0))")
        is_v0 = v0_family and plcy_loss_mode == "v0"
        if is_v0 and (not isinstance(v0, (tuple, list)) or len(v0) != 2):
            raise OlyError("iq_q_update: v0 must be the pair (a_v0, logp_v0)")
        if all_expert and (regularizer_mode == "plcy" or plcy_loss_mode in ("value_policy", "q_old_policy",
                                                                            "value_q_old_policy")):
            raise OlyError(f"iq_q_update: all_expert leaves no policy rows for plcy_loss_mode {plcy_loss_mode!r} / "
                           f"regularizer_mode {regularizer_mode!r}")
        if regularizer_mode not in _abi.IQ_REGULARIZER_MODES:
            raise OlyError(f"iq_q_update: unknown regularizer_mode {regularizer_mode!r}")
        if float(gradient_penalty_lambda) > 0.0:
            raise OlyError("iq_q_update: the gradient penalty is not built")
        if not 0.0 <= float(tau) <= 1.0:
            raise OlyError(f"iq_q_update: tau={tau} outside [0, 1]")
        D = in_dim + A
        need_pi = not (hb or (algo == "sqil" and plcy_loss_mode == "plcy") or (sqil_like and plcy_loss_mode == "q_old_policy"))
        n_pi = int(n_policy) if sqil_like and plcy_loss_mode == "value_plcy" else B      # the rows of the third pass
        need_target = bool(use_target) or bool(update_target)
        n_par = 512 * D + 512 + 256 * 512 + 256 + 256 + 1
        npk = int(lib().oly_ilmlp_packed_floats(D, 512, 256, 1))
        _req(obs, "obs", (B, in_dim), f32, dv)
        _req(act, "act", (B, A), f32, dv)
        _req(next_obs, "next_obs", (B, in_dim), f32, dv)
        _req(absorbing, "absorbing", (B,), f32, dv)
        _req(a_next, "a_next", (B, A), f32, dv)
        _req(logp_next, "logp_next", (B,), f32, dv)
        _req(a_pi, "a_pi", (n_pi, A), f32, dv, optional=not need_pi)
        _req(logp_pi, "logp_pi", (n_pi,), f32, dv, optional=not need_pi)
        a_v0, logp_v0 = v0 if is_v0 else (None, None)
        if is_v0:
            _req(a_v0, "a_v0", (B - int(n_policy), A), f32, dv)
            _req(logp_v0, "logp_v0", (B - int(n_policy),), f32, dv)
        _req(colstats, "colstats", (3, D), f64, dv, optional=True)
        _req(target_colstats, "target_colstats", (3, D), f64, dv, optional=True)
        for t, name in ((param, "param"), (m, "m"), (v, "v")):
            _req(t, name, (n_par,), f32, dv)
        _req(packed, "packed", (npk,), f32, dv)
        _req(target_param, "target_param", (n_par,), f32, dv, optional=not need_target)
        _req(target_packed, "target_packed", (npk,), f32, dv, optional=not need_target)
        _req(ws, "ws", (nws,), f32, dv)
        out = _req(out if out is not None else self._new((16,), f64), "out", (16,), f64, dv)
        f = _abi.IQQ(in_dim=in_dim, act_dim=A, batch=B, n_policy=int(n_policy), algo=_abi.IQ_ALGO[algo],
                     plcy_loss_mode=modes[plcy_loss_mode], regularizer_mode=_abi.IQ_REGULARIZER_MODES[regularizer_mode],
                     treat_absorbing=int(bool(treat_absorbing)), use_target=int(bool(use_target)),
                     update_target=int(bool(update_target)), step=int(step), pad=0, gamma=float(gamma), alpha=float(alpha),
                     reg_mult=float(reg_mult), R_min=float(R_min), R_max=float(R_max),
                     gradient_penalty_lambda=float(gradient_penalty_lambda), lr=float(lr), beta1=float(beta1),
                     beta2=float(beta2), eps=float(eps), weight_decay=float(weight_decay), pad2=0.0, tau=float(tau),
                     obs=obs.data_ptr(), act=act.data_ptr(), next_obs=next_obs.data_ptr(), absorbing=absorbing.data_ptr(),
                     a_next=a_next.data_ptr(), logp_next=logp_next.data_ptr(), a_pi=ptr(a_pi), logp_pi=ptr(logp_pi),
                     colstats=ptr(colstats), target_colstats=ptr(target_colstats), param=param.data_ptr(),
                     m=m.data_ptr(), v=v.data_ptr(), packed=packed.data_ptr(), target_param=ptr(target_param),
                     target_packed=ptr(target_packed), packed_floats=npk, target_packed_floats=npk if need_target else 0,
                     ws=ws.data_ptr(), ws_floats=nws, out=out.data_ptr(),
                     lsiq=C.pointer(block) if block is not None else None)
        if is_v0 or all_expert:        # the block hangs behind an oly_iq_q whose pad says so (oly_iq_q_ext)
            f.pad = _abi.OLY_IQ_Q_EXT
            vblock = _abi.IQV0(a_v0=ptr(a_v0), logp_v0=ptr(logp_v0), all_expert=int(bool(all_expert)), pad=0)
            ext = _abi.IQQExt(q=f, v0=C.pointer(vblock))
            self.ctx.call("oly_iq_q_update", C.cast(C.pointer(ext), C.POINTER(_abi.IQQ)), self._s())
            return out
        self.ctx.call("oly_iq_q_update", C.byref(f), self._s())
        return out

    # -------------------------------------------------------------- K27 (the policy and temperature update of IQ-Learn / SQIL)
    def iq_pi_ws(self, batch, in_dim, act_dim):
        """A workspace for iq_pi_update with batches of `batch` rows."""
        from ._ffi import lib
        n = int(lib().oly_iq_pi_ws(int(batch), int(in_dim), int(act_dim)))
        if n < 0:
            raise OlyError(f"iq_pi_update: unsupported batch={batch} in={in_dim} act={act_dim} (1 <= batch <= "
                           f"{_abi.OLY_BC_MAX_BATCH}, act <= {_abi.OLY_BC_MAX_ACT}, in + act <= 64)")
        return self._new((n,), torch.float32)

    def iq_pi_update(self, x, eps, central, delta, colstats, param, m, v, packed, critic_packed, critic_param,
                     critic_colstats, ws, step, lr, alpha=1e-3, log_std_min=-20.0, log_std_max=2.0, beta1=0.9, beta2=0.999,
                     adam_eps=1e-8, weight_decay=0.0, out=None, h=None):
        """oly_iq_pi_update: one update_policy of IQ_SAC / SQIL (iq_sac.py:431-439, 587-590) without its logging passes.
        x [Bp,in] f32 the policy_training_states, eps [Bp,A] f32 the noise, central / delta [A] f32; colstats [3,in] f64
        the policy's Standardizer or None (it takes the rows first); param / m / v the policy's flat parameters and Adam
        moments in torch order (W1 [512,in] | b1 | W2 | b2 | W3 [2A,256] | b3), packed their ilmlp_pack stream, kept
        current by the call; critic_packed / critic_param the live critic's (read only), critic_colstats [3,in+A] f64 or
        None (it takes the rows (x | a_new)); step = Adam steps taken before.  h (LSIQ_H / LSIQ_HC's _actor_loss over two
        critics, lsiq_h.py:104-108): None, or dict(packed, param, colstats (or None), ws) of the second live critic H, ws a
        workspace of its own of iq_pi_ws() floats; the loss is then mean(alpha log_prob - (q + H)), out[3] mean(q + H), and
        H(x | a_new) lies in h["ws"] at oly_iq_pi_ws_values().  Returns dict(action [Bp,A] f32, log_prob
        [Bp] f32, out [4] f64 (_abi.IQ_PI_TAGS)); `out` may supply the buffers.  No synchronisation."""
        from ._ffi import lib
        f32, f64, dv = torch.float32, torch.float64, self.device
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or not isinstance(central, torch.Tensor) or central.dim() != 1:
            raise OlyError("iq_pi_update: x [Bp,in] and central [A] must be tensors")
        B, in_dim = (int(t) for t in x.shape)
        A = int(central.shape[0])
        nws = int(lib().oly_iq_pi_ws(B, in_dim, A))
        if nws < 0:
            raise OlyError(f"iq_pi_update: unsupported batch={B} in={in_dim} act={A} (1 <= batch <= "
                           f"{_abi.OLY_BC_MAX_BATCH}, act <= {_abi.OLY_BC_MAX_ACT}, in + act <= 64)")
        if not float(log_std_min) <= float(log_std_max):
            raise OlyError("iq_pi_update: log_std_min <= log_std_max is required")
        D = in_dim + A
        n_par = 512 * in_dim + 512 + 256 * 512 + 256 + 2 * A * 256 + 2 * A
        n_cpar = 512 * D + 512 + 256 * 512 + 256 + 256 + 1
        npk = int(lib().oly_ilmlp_packed_floats(in_dim, 512, 256, 2 * A))
        ncpk = int(lib().oly_ilmlp_packed_floats(D, 512, 256, 1))
        _req(x, "x", (B, in_dim), f32, dv)
        _req(eps, "eps", (B, A), f32, dv)
        _req(central, "central", (A,), f32, dv)
        _req(delta, "delta", (A,), f32, dv)
        _req(colstats, "colstats", (3, in_dim), f64, dv, optional=True)
        _req(critic_colstats, "critic_colstats", (3, D), f64, dv, optional=True)
        for t, name in ((param, "param"), (m, "m"), (v, "v")):
            _req(t, name, (n_par,), f32, dv)
        _req(packed, "packed", (npk,), f32, dv)
        _req(critic_packed, "critic_packed", (ncpk,), f32, dv)
        _req(critic_param, "critic_param", (n_cpar,), f32, dv)
        _req(ws, "ws", (nws,), f32, dv)
        hk = {}
        if h is not None:
            if not isinstance(h, dict) or set(h) != {"packed", "param", "colstats", "ws"}:
                raise OlyError("iq_pi_update: h must be dict(packed, param, colstats, ws)")
            _req(h["packed"], "h packed", (ncpk,), f32, dv)
            _req(h["param"], "h param", (n_cpar,), f32, dv)
            _req(h["colstats"], "h colstats", (3, D), f64, dv, optional=True)
            _req(h["ws"], "h ws", (nws,), f32, dv)
            if h["ws"].data_ptr() == ws.data_ptr() or h["packed"].data_ptr() == critic_packed.data_ptr():
                raise OlyError("iq_pi_update: H needs a stream and a workspace of its own")
            hk = dict(h_packed=h["packed"].data_ptr(), h_packed_floats=ncpk, h_param=h["param"].data_ptr(),
                      h_colstats=ptr(h["colstats"]), h_ws=h["ws"].data_ptr(), h_ws_floats=nws)
        out = out or {}
        o = dict(action=self._out(out, "action", (B, A), f32), log_prob=self._out(out, "log_prob", (B,), f32),
                 out=self._out(out, "out", (4,), f64))
        f = _abi.IQPi(in_dim=in_dim, act_dim=A, batch=B, step=int(step), alpha=float(alpha),
                      log_std_min=float(log_std_min), log_std_max=float(log_std_max), lr=float(lr), beta1=float(beta1),
                      beta2=float(beta2), adam_eps=float(adam_eps), weight_decay=float(weight_decay), x=x.data_ptr(),
                      eps=eps.data_ptr(), central=central.data_ptr(), delta=delta.data_ptr(), colstats=ptr(colstats),
                      param=param.data_ptr(), m=m.data_ptr(), v=v.data_ptr(), packed=packed.data_ptr(), packed_floats=npk,
                      critic_packed=critic_packed.data_ptr(), critic_packed_floats=ncpk,
                      critic_param=critic_param.data_ptr(), critic_colstats=ptr(critic_colstats), ws=ws.data_ptr(),
                      ws_floats=nws, action=o["action"].data_ptr(), log_prob=o["log_prob"].data_ptr(),
                      out=o["out"].data_ptr(), **hk)
        self.ctx.call("oly_iq_pi_update", C.byref(f), self._s())
        return o

    def iq_alpha_update(self, log_prob, state, step, lr, target_entropy, beta1=0.9, beta2=0.999, eps=1e-8):
        """oly_iq_alpha_update: one _update_alpha (iq_sac.py:592-595) in one launch.  log_prob [n] f32; state [3] f32 the
        device block (log_alpha, exp_avg, exp_avg_sq), stepped in place by Adam with step + 1.  Returns state.  No
        synchronisation."""
        f32, dv = torch.float32, self.device
        if not isinstance(log_prob, torch.Tensor) or log_prob.dim() != 1 or int(log_prob.shape[0]) < 1:
            raise OlyError("iq_alpha_update: log_prob [n] with n >= 1 must be a tensor")
        n = int(log_prob.shape[0])
        _req(log_prob, "log_prob", (n,), f32, dv)
        _req(state, "state", (3,), f32, dv)
        if int(step) < 0:
            raise OlyError(f"iq_alpha_update: step={step} < 0")
        f = _abi.IQAlpha(n=n, step=int(step), target_entropy=float(target_entropy), lr=float(lr), beta1=float(beta1),
                         beta2=float(beta2), eps=float(eps), pad=0.0, log_prob=log_prob.data_ptr(), state=state.data_ptr())
        self.ctx.call("oly_iq_alpha_update", C.byref(f), self._s())
        return state

    # -------------------------------------------------------------- K18 (GAIL's discriminator: reward, fit)
    def _gail_packed_floats(self, D):
        cache = self.__dict__.setdefault("_gail_sizes", {})
        if D not in cache:
            cache[D] = int(lib().oly_ilmlp_packed_floats(D, 512, 256, 1))
        if cache[D] < 0:
            raise OlyError(f"gail discriminator: unsupported input width {D} (0 < in <= 64)")
        return cache[D]

    def gail_disc_forward(self, x, packed, mask=None, mean=None, std=None, colstats=None, want=("reward",), out=None):
        """GAIL's make_discrim_reward for x [B,Dx] f32 in one launch (in -> 512 -> 256 -> 1, tanh, tanh, identity).
        mask [D] int32: the state columns, gathered inside the kernel (the block is never copied to its masked
        width).  want: any of reward / logits.  Standardisation from mean / std [D] f64, or from the running colstats
        [3,D] of col_stats, or none.  packed: the ilmlp_pack stream of the network (out_dim 1)."""
        return self._disc_forward_on(_GAIL, "gail_disc_forward", x, packed, mask, (mean, std, colstats), None, None, want,
                                     out)

    def gail_disc_forward_pair(self, x, x2, packed, standardise, mask=None, mask2=None, stats_a=None, stats_b=None,
                               want=("reward",), out=None):
        """oly_gail_disc_forward_pair: gail_disc_forward on [ standardise(x[:, mask]) | second ], second =
        standardise(x2[:, mask2]) with stats_b (standardise: next states) or x2[:, mask2] raw (actions).  stats_a /
        stats_b [3,Ds] f64 running sums, or both None (nothing is standardised)."""
        return self._disc_forward_on(_GAIL, "gail_disc_forward_pair", x, packed, mask, (stats_a, stats_b),
                                     (x2, mask2, standardise), None, want, out)

    def _gail_reward_step(self, name, x, packed, colstats, stats_a, accumulate, mask, second, want, out, weights):
        out, head, tail = self._disc_reward_step_args(_GAIL, name, x, packed, colstats, stats_a, mask, second, None, want,
                                                      out, weights)
        self.ctx.call("oly_" + name, *head, int(bool(accumulate)), *tail, self._s())
        return out

    def gail_reward_step(self, x, packed, colstats, accumulate, mask=None, want=("reward",), out=None, weights=None):
        """oly_gail_reward_step: (re-pack of `weights`, the six parameter tensors in ilmlp_pack's order, when given,) the
        Standardizer's running update with x's masked rows (into colstats [3,D] f64, accumulate: added to the running
        sums) and the forward on the updated statistics, one C call.  x [B,Dx] f32; mask [D] int32 or None."""
        return self._gail_reward_step("gail_reward_step", x, packed, colstats, None, accumulate, mask, None, want, out,
                                      weights)

    def gail_reward_step_pair(self, x, x2, packed, colstats, stats_a, accumulate, standardise, mask=None, mask2=None,
                              want=("reward",), out=None, weights=None):
        """oly_gail_reward_step_pair: the Standardizer's update with x's masked rows (colstats [3,Ds]; that result kept in
        stats_a [3,Ds]), for next states its second update with x2's masked rows, then the paired forward on both, one C
        call without a host synchronisation."""
        return self._gail_reward_step("gail_reward_step_pair", x, packed, colstats, stats_a, accumulate, mask,
                                      (x2, mask2, standardise), want, out, weights)

    def gail_disc_fit_ws(self, batch, in_dim):
        """A workspace for gail_disc_fit_epoch with minibatches of `batch` rows."""
        return self._new((self._disc_fit_ws_floats(_GAIL, "gail_disc_fit", batch, in_dim),), torch.float32)

    def gail_disc_fit_pair_ws(self, batch, ds, d2, standardise):
        """A workspace for gail_disc_fit_epoch_pair with minibatches of `batch` rows."""
        return self._new((self._disc_fit_ws_floats(_GAIL, "gail_disc_fit_pair", batch, ds, d2, standardise),),
                         torch.float32)

    def gail_disc_fit_epoch(self, x, n_plcy, perm, batch, colstats, param, exp_avg, exp_avg_sq, packed, ws, step, lr,
                            beta1=0.9, beta2=0.999, adam_eps=1e-8, weight_decay=0.0, entcoeff=1e-3, targets=None,
                            loss_out=None, bce_out=None, ent_out=None):
        """oly_gail_disc_fit_epoch: one epoch of GAIL's discriminator minibatch loop in one call.  x [n,in] f32 the masked
        concatenated rows (policy rows first, n_plcy of them), perm [n] int32, param / exp_avg / exp_avg_sq flat in torch
        order (W1 | b1 | W2 | b2 | W3 | b3), packed the ilmlp_pack stream (re-packed from param, then kept current),
        targets [n] f32 or None (0 / 1); step = Adam steps taken before.  Returns loss_out [n_batches] f64 (bce_out,
        ent_out likewise when given)."""
        return self._disc_fit_epoch(_GAIL, "gail_disc_fit_epoch", x, None, n_plcy, perm, batch, colstats, param, exp_avg,
                                    exp_avg_sq, packed, ws, step, lr, beta1, beta2, adam_eps, weight_decay, targets,
                                    loss_out, bce_out, entcoeff=entcoeff, ent_out=ent_out)

    def gail_disc_fit_epoch_pair(self, x, x2, standardise, n_plcy, perm, batch, colstats, param, exp_avg, exp_avg_sq,
                                 packed, ws, step, lr, beta1=0.9, beta2=0.999, adam_eps=1e-8, weight_decay=0.0,
                                 entcoeff=1e-3, targets=None, loss_out=None, bce_out=None, ent_out=None):
        """oly_gail_disc_fit_epoch_pair: gail_disc_fit_epoch on the paired rows x [n,Ds] | x2 [n,D2] (both masked and
        concatenated, policy rows first); colstats [3,Ds]; param / moments for in = Ds + D2."""
        return self._disc_fit_epoch(_GAIL, "gail_disc_fit_epoch_pair", x, (x2, None, standardise), n_plcy, perm, batch,
                                    colstats, param, exp_avg, exp_avg_sq, packed, ws, step, lr, beta1, beta2, adam_eps,
                                    weight_decay, targets, loss_out, bce_out, entcoeff=entcoeff, ent_out=ent_out)

    # -------------------------------------------------------------- K19 (the discriminator's diagnostics)
    def gail_disc_log_ws(self, n_rows):
        """A workspace for gail_disc_log on up to n_rows rows."""
        from ._ffi import lib
        n = int(lib().oly_gail_disc_log_ws_floats(int(n_rows)))
        if n < 0:
            raise OlyError(f"gail_disc_log: unsupported n_rows={n_rows} (at least one policy and one demonstration row)")
        return self._new((n,), torch.float32)

    def disc_log_ws(self, n_rows):
        """A workspace for disc_log on up to n_rows rows."""
        from ._ffi import lib
        n = int(lib().oly_disc_log_ws_floats(int(n_rows)))
        if n < 0:
            raise OlyError(f"disc_log: unsupported n_rows={n_rows} (at least one policy and one demonstration row)")
        return self._new((n,), torch.float32)

    def _disc_log_common(self, name, x, n_plcy, colstats, ws, need, x2, standardise, targets, out):
        f32, f64, dv = torch.float32, torch.float64, self.device
        if not isinstance(x, torch.Tensor) or x.dim() != 2:
            raise OlyError("x: expected a [n,Ds] tensor")
        n, Ds = (int(v) for v in x.shape)
        _req(x, "x", (n, Ds), f32, dv)
        pair, d2 = None, 0
        if x2 is not None:
            pair, d2 = self._disc_pair(name, x2, None, standardise, n, Ds)
        if not 0 < int(n_plcy) < n:
            raise OlyError(f"{name}: n_plcy={n_plcy} outside (0, {n}): both halves need a row")
        _req(targets, "targets", (n,), f32, dv, optional=True)
        _req(colstats, "colstats", (3, Ds), f64, dv)
        nws = int(need(n))
        if not isinstance(ws, torch.Tensor) or ws.dim() != 1 or int(ws.shape[0]) < nws:
            raise OlyError(f"{name}: the workspace holds {0 if not isinstance(ws, torch.Tensor) else int(ws.numel())} "
                           f"floats, {n} rows need {nws}")
        _req(ws, "ws", (int(ws.shape[0]),), f32, dv)
        out = _req(out if out is not None else self._new((_abi.OLY_DISC_LOG_SCALARS,), f64), "out",
                   (_abi.OLY_DISC_LOG_SCALARS,), f64, dv)
        return n, Ds, d2, pair, out

    def gail_disc_log(self, x, n_plcy, colstats, packed, ws, entcoeff=1e-3, x2=None, standardise=False, targets=None,
                      out=None):
        """oly_gail_disc_log: _discriminator_logging's six forwards for GAIL on x [n,Ds] f32 (the masked concatenated
        rows, n_plcy policy rows first) and, for a paired discriminator, x2 [n,D2] (standardise: next states).  colstats
        [3,Ds] f64 is read and left where the reference's Standardizer ends; packed is the ilmlp_pack stream of the
        current parameters.  Returns out [12] f64 on the device in _abi.DISC_LOG_TAGS' order (GAIL fills nine)."""
        from ._ffi import lib
        n, Ds, d2, pair, out = self._disc_log_common("gail_disc_log", x, n_plcy, colstats, ws,
                                                     lib().oly_gail_disc_log_ws_floats, x2, standardise, targets, out)
        _req(packed, "packed", (self._gail_packed_floats(Ds + d2),), torch.float32, self.device)
        f = _abi.GailDiscLog(in_dim=Ds + d2, n_rows=n, n_plcy=int(n_plcy), entcoeff=float(entcoeff), x=x.data_ptr(),
                             targets=ptr(targets), colstats=colstats.data_ptr(), packed=packed.data_ptr(),
                             ws=ws.data_ptr(), ws_floats=int(ws.shape[0]), out=out.data_ptr())
        self.ctx.call("oly_gail_disc_log", C.byref(f), C.byref(pair) if pair is not None else None, self._s())
        return out

    def disc_log(self, x, n_plcy, colstats, packed, beta, ws, info_constraint=0.1, lr_beta=1e-5, entcoeff=1e-3, eps=None,
                 x2=None, standardise=False, targets=None, out=None):
        """oly_disc_log: _discriminator_logging's seven forwards for VAIL.  As gail_disc_log, with beta [1] f32 the
        VDBLoss's beta (read only) and eps [2 n + 2 n_plcy + 2 n_demo = 4 n, 128] f32 the noise of forwards 1 .. 6 in
        forward order (all rows, demonstration half, policy half, twice), or None (z = mu)."""
        from ._ffi import lib
        n, Ds, d2, pair, out = self._disc_log_common("disc_log", x, n_plcy, colstats, ws, lib().oly_disc_log_ws_floats,
                                                     x2, standardise, targets, out)
        _req(packed, "packed", (self._disc_packed_floats(Ds + d2),), torch.float32, self.device)
        _req(beta, "beta", (1,), torch.float32, self.device)
        _req(eps, "eps", (4 * n, 128), torch.float32, self.device, optional=True)
        f = _abi.DiscLog(in_dim=Ds + d2, n_rows=n, n_plcy=int(n_plcy), entcoeff=float(entcoeff),
                         info_constraint=float(info_constraint), lr_beta=float(lr_beta), x=x.data_ptr(),
                         targets=ptr(targets), eps=ptr(eps), beta=beta.data_ptr(), colstats=colstats.data_ptr(),
                         packed=packed.data_ptr(), ws=ws.data_ptr(), ws_floats=int(ws.shape[0]), out=out.data_ptr())
        self.ctx.call("oly_disc_log", C.byref(f), C.byref(pair) if pair is not None else None, self._s())
        return out

    # -------------------------------------------------------------- K20 (the agent's iteration diagnostics)
    def _episode_blocks(self, name, reward, last, reward2):
        f32, dv = torch.float32, self.device
        if not isinstance(reward, torch.Tensor) or reward.dim() != 2:
            raise OlyError(f"{name}: reward is a [T,N] tensor")
        T, N = (int(v) for v in reward.shape)
        if T < 1 or N < 1 or T * N >= 2 ** 31:
            raise OlyError(f"{name}: supported: T >= 1, N >= 1, T N < 2^31 (got [{T}, {N}])")
        r64 = reward.dtype == torch.float64
        _req(reward, "reward", (T, N), torch.float64 if r64 else f32, dv)
        _req(reward2, "reward2", (T, N), f32, dv, optional=True)
        if not isinstance(last, torch.Tensor) or last.dtype not in (torch.bool, torch.uint8):
            raise OlyError(f"{name}: last is a bool or uint8 tensor")
        _req(last, "last", (T, N), last.dtype, dv)
        return T, N, r64

    def episode_stats(self, reward, last, gamma=1.0, reward2=None, out=None):
        """oly_episode_stats: compute_J / compute_episodes_length per environment over reward [T,N] (f32 or f64), an
        optional second block reward2 [T,N] f32 and last [T,N] (bool or uint8).  Returns out [8] f64 on the device: mean
        return, mean return of reward2, mean length (NaN without a completed episode), number of returns, number of
        lengths, and the three sums.  No synchronisation."""
        T, N, r64 = self._episode_blocks("episode_stats", reward, last, reward2)
        if not 0.0 <= float(gamma) <= 1.0:
            raise OlyError(f"episode_stats: gamma {gamma} outside [0, 1]")
        out = _req(out if out is not None else self._new((_abi.OLY_EPISODE_STATS,), torch.float64), "out",
                   (_abi.OLY_EPISODE_STATS,), torch.float64, self.device)
        self.ctx.call("oly_episode_stats", T, N, int(r64), C.c_double(float(gamma)), ptr(reward), ptr(reward2), ptr(last),
                      ptr(out), self._s())
        return out

    def iter_log_ws(self, n):
        """A workspace for iter_log on up to n rows."""
        from ._ffi import lib
        k = int(lib().oly_iter_log_ws_floats(int(n)))
        if k < 0:
            raise OlyError(f"iter_log: unsupported n={n}")
        return self._new((k,), torch.float32)

    def iter_log(self, x, v_target, mu_old, log_sigma_old, log_sigma, critic_packed, policy_packed, reward_env, reward, last,
                 colstats, ws, out=None):
        """oly_iter_log: _logging_sw (gail_TRPO.py:251-272) on x [n,in] f32 (row t N + e), v_target [n] f32, the old
        distribution mu_old [n,act] / log_sigma_old [act], the stepped policy's log_sigma [act], the packed critic and
        policy mean networks, reward_env [T,N] (f32 or f64), reward [T,N] f32 (the reward trained on) and last [T,N].
        colstats [3,in] f64 is read as S and left at S + 2c.  Returns out [8] f64 on the device: _abi.ITER_LOG_TAGS'
        six scalars, the mean episode length before rounding, the completed episodes."""
        from ._ffi import lib
        f32, f64, dv = torch.float32, torch.float64, self.device
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or not isinstance(mu_old, torch.Tensor) or mu_old.dim() != 2:
            raise OlyError("iter_log: x [n,in] and mu_old [n,act] must be 2-D tensors")
        n, D = (int(v) for v in x.shape)
        A = int(mu_old.shape[1])
        T, N, r64 = self._episode_blocks("iter_log", reward_env, last, reward)
        if reward is None:
            raise OlyError("iter_log: reward (the reward the agent trained on) is required")
        if T * N != n:
            raise OlyError(f"iter_log: x has {n} rows, the blocks are [{T}, {N}]")
        np_c = int(lib().oly_ilmlp_packed_floats(D, 512, 256, 1))
        np_p = int(lib().oly_ilmlp_packed_floats(D, 512, 256, A))
        if np_c < 0 or np_p < 0:
            raise OlyError(f"iter_log: unsupported shape in={D} act={A} (in <= 64, act <= 32)")
        _req(x, "x", (n, D), f32, dv)
        _req(v_target, "v_target", (n,), f32, dv)
        _req(mu_old, "mu_old", (n, A), f32, dv)
        _req(log_sigma_old, "log_sigma_old", (A,), f32, dv)
        _req(log_sigma, "log_sigma", (A,), f32, dv)
        _req(critic_packed, "critic_packed", (np_c,), f32, dv)
        _req(policy_packed, "policy_packed", (np_p,), f32, dv)
        _req(colstats, "colstats", (3, D), f64, dv)
        need = int(lib().oly_iter_log_ws_floats(n))
        if not isinstance(ws, torch.Tensor) or ws.dim() != 1 or int(ws.shape[0]) < need:
            raise OlyError(f"iter_log: the workspace holds {0 if not isinstance(ws, torch.Tensor) else int(ws.numel())} "
                           f"floats, {n} rows need {need}")
        _req(ws, "ws", (int(ws.shape[0]),), f32, dv)
        out = _req(out if out is not None else self._new((_abi.OLY_ITER_LOG_SCALARS,), f64), "out",
                   (_abi.OLY_ITER_LOG_SCALARS,), f64, dv)
        f = _abi.IterLog(n=n, in_dim=D, act_dim=A, T=T, N=N, rew_f64=int(r64), x=x.data_ptr(), v_target=v_target.data_ptr(),
                         mu_old=mu_old.data_ptr(), log_sigma_old=log_sigma_old.data_ptr(), log_sigma=log_sigma.data_ptr(),
                         critic_packed=critic_packed.data_ptr(), policy_packed=policy_packed.data_ptr(),
                         rew_env=reward_env.data_ptr(), rew=reward.data_ptr(), last=last.data_ptr(),
                         colstats=colstats.data_ptr(), ws=ws.data_ptr(), ws_floats=int(ws.shape[0]), out=out.data_ptr())
        self.ctx.call("oly_iter_log", C.byref(f), self._s())
        return out

    # -------------------------------------------------------------- K21 (one acting step) / K5
    def il_ctrl(self, action, ctrl_f64=False, out=None):
        """oly_il_ctrl: action [N,n_act] f32 -> ctrl [N,nu] (f32, or f64), un-normalised, clamped, actuator order."""
        sp = self.il_spec
        if sp is None:
            raise OlyError("il_ctrl before il_configure")
        if not isinstance(action, torch.Tensor) or action.dim() != 2:
            raise OlyError("il_ctrl: action is a [N,n_act] tensor")
        N = int(action.shape[0])
        _req(action, "action", (N, sp.n_act), torch.float32, self.device)
        cd = torch.float64 if ctrl_f64 else torch.float32
        out = _req(out if out is not None else self._new((N, sp.nu), cd), "ctrl", (N, sp.nu), cd, self.device)
        self.ctx.call("oly_il_ctrl", N, ptr(action), ptr(out), _abi.OUT_CTRL_F64 if ctrl_f64 else 0, self._s())
        return out

    def il_act(self, x, packed, log_sigma, colstats, eps=None, update_stats=True, want_mu=False, want_ctrl=False,
               ctrl_f64=False, out=None):
        """oly_il_act: one acting step on x [n,in] f32.  colstats [3,in] f64 takes the rows first (update_stats), the mean
        network (packed, ilmlp_pack's stream) runs on the statistics after that, action = mu + exp(log_sigma) eps (eps
        [n,act] f32, None: action = mu) and, with want_ctrl, ctrl [n,nu] = il_ctrl(action) from the configured model.
        Returns dict(action, mu or None, ctrl or None); `out` may supply the buffers.  No synchronisation."""
        from ._ffi import lib
        f32, f64, dv = torch.float32, torch.float64, self.device
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or not isinstance(log_sigma, torch.Tensor) or log_sigma.dim() != 1:
            raise OlyError("il_act: x [n,in] and log_sigma [act] must be tensors")
        n, D = (int(v) for v in x.shape)
        A = int(log_sigma.shape[0])
        if n < 1:
            raise OlyError(f"il_act: n={n} rows (n >= 1)")
        npk = int(lib().oly_ilmlp_packed_floats(D, 512, 256, A))
        if npk < 0:
            raise OlyError(f"il_act: unsupported shape in={D} act={A} (in <= 64, act <= 32)")
        _req(x, "x", (n, D), f32, dv)
        _req(packed, "packed", (npk,), f32, dv)
        _req(log_sigma, "log_sigma", (A,), f32, dv)
        _req(colstats, "colstats", (3, D), f64, dv)
        _req(eps, "eps", (n, A), f32, dv, optional=True)
        nu = 0
        if want_ctrl:
            sp = self.il_spec
            if sp is None:
                raise OlyError("il_act: want_ctrl before il_configure")
            if int(sp.n_act) != A:
                raise OlyError(f"il_act: want_ctrl for {A} actions, the configured model has n_act={sp.n_act}")
            nu = int(sp.nu)
        out = out or {}
        cd = f64 if ctrl_f64 else f32
        action = self._out(out, "action", (n, A), f32)
        mu = self._out(out, "mu", (n, A), f32) if want_mu else None
        ctrl = self._out(out, "ctrl", (n, nu), cd) if want_ctrl else None
        f = _abi.ILAct(n=n, in_dim=D, act_dim=A, update_stats=int(bool(update_stats)), x=x.data_ptr(),
                       colstats=colstats.data_ptr(), packed=packed.data_ptr(), log_sigma=log_sigma.data_ptr(),
                       eps=ptr(eps), action=action.data_ptr(), mu=ptr(mu), ctrl=ptr(ctrl),
                       out_flags=_abi.OUT_CTRL_F64 if (want_ctrl and ctrl_f64) else 0, pad=0)
        self.ctx.call("oly_il_act", C.byref(f), self._s())
        return dict(action=action, mu=mu, ctrl=ctrl)

    # -------------------------------------------------------------- K22 (reset the ended episodes on the device)
    def il_reset_tables(self):
        """The inverse address tables of the configured spec as device int32 tensors, cached per spec: (qpos_slot [nq],
        qvel_slot [nv]) with slot[address] = the spec slot whose qpos_adr / qvel_adr is that address, or -1."""
        sp = self.il_spec
        if sp is None:
            raise OlyError("il_reset_where before il_configure")
        cached = getattr(self, "_il_reset_tabs", None)
        if cached is None or cached[0] is not sp:
            tabs = []
            for adr, size in ((sp.qpos_adr, sp.nq), (sp.qvel_adr, sp.nv)):
                inv = np.full(int(size), -1, np.int32)
                inv[np.asarray(adr, np.int64)] = np.arange(len(adr), dtype=np.int32)
                tabs.append(torch.as_tensor(inv).to(self.device))
            cached = self._il_reset_tabs = (sp, tabs[0], tabs[1])
        return cached[1], cached[2]

    def il_reset_where(self, mask, qpos, qvel, obs_in, obs_out, prev, episode_steps, traj_no=None, step=None, cur_traj=None,
                       cur_step=None, origin=None, sample=None):
        """oly_il_reset_where: reset the environments with mask[n] set (mask [N] bool or uint8, None: all) in one launch.
        qpos [N,nq] / qvel [N,nv] f64, prev [N] f64, episode_steps [N] i32 and, with traj_no / step [N] i32, cur_traj /
        cur_step [N] i32, origin [N,2] f64, sample [N,n_keys] f64 are updated in place; obs_out [N,n_obs] (f32 or f64, the
        type of obs_in) takes the created observation of the reset rows and obs_in's rows elsewhere (obs_out may be
        obs_in).  traj_no None: the state rows are zeroed.  Returns obs_out.  No synchronisation."""
        if not isinstance(qpos, torch.Tensor) or qpos.dim() != 2:
            raise OlyError("il_reset_where: qpos is a [N,nq] tensor")
        N = int(qpos.shape[0])
        with_traj = traj_no is not None
        launch = self.il_reset_where_prepare(N, prev, episode_steps, *((cur_traj, cur_step, origin, sample) if with_traj
                                                                       else ()), with_traj=with_traj)
        self._il_reset_check(N, mask, qpos, qvel, obs_in, obs_out, traj_no, step)
        return launch(mask, qpos, qvel, obs_in, obs_out, traj_no, step)

    def _il_reset_check(self, N, mask, qpos, qvel, obs_in, obs_out, traj_no, step):
        """The per-call tensors of il_reset_where."""
        sp, dv = self.il_spec, self.device
        if mask is not None and isinstance(mask, torch.Tensor) and mask.dtype not in (torch.bool, torch.uint8):
            raise OlyError(f"mask: dtype {mask.dtype}, expected torch.bool or torch.uint8")
        _req(mask, "mask", (N,), mask.dtype if isinstance(mask, torch.Tensor) else torch.bool, dv, optional=True)
        _req(qpos, "qpos", (N, sp.nq), torch.float64, dv)
        _req(qvel, "qvel", (N, sp.nv), torch.float64, dv)
        if not isinstance(obs_in, torch.Tensor) or obs_in.dtype not in (torch.float32, torch.float64):
            raise OlyError("obs_in: expected a float32 or float64 tensor")
        _req(obs_in, "obs_in", (N, sp.n_obs), obs_in.dtype, dv)
        _req(obs_out, "obs_out", (N, sp.n_obs), obs_in.dtype, dv)
        if traj_no is not None:
            _req(traj_no, "traj_no", (N,), torch.int32, dv)
            _req(step, "step", (N,), torch.int32, dv)

    def il_reset_where_prepare(self, N, prev, episode_steps, cur_traj=None, cur_step=None, origin=None, sample=None,
                               with_traj=False):
        """Validate once the buffers a vec environment keeps for its lifetime and return
        launch(mask, qpos, qvel, obs_in, obs_out, traj_no, step) -> obs_out, which re-points the argument block and
        launches oly_il_reset_where.  The launch validates NOTHING about its seven tensors (the per-step regime: that is
        the caller's contract, Engine._il_reset_check is the check); it refuses to run after the engine was configured
        with another spec or another trajectory table."""
        from ._ffi import check, lib
        sp = self.il_spec
        if sp is None:
            raise OlyError("il_reset_where before il_configure")
        N, dv = int(N), self.device
        i32, f64 = torch.int32, torch.float64
        _req(prev, "prev", (N,), f64, dv, optional=sp.reward_type == _abi.REWARD_NONE)
        _req(episode_steps, "episode_steps", (N,), i32, dv)
        shape = self.traj_shape
        if with_traj:
            if shape is None:
                raise OlyError("il_reset_where: traj_no given before traj_upload")
            K = shape[0]
            if K < sp.n_pos + sp.n_vel:
                raise OlyError(f"il_reset_where: the uploaded table has {K} keys, the model needs {sp.n_pos + sp.n_vel}")
            _req(cur_traj, "cur_traj", (N,), i32, dv)
            _req(cur_step, "cur_step", (N,), i32, dv)
            _req(origin, "origin", (N, 2), f64, dv)
            _req(sample, "sample", (N, K), f64, dv)
        qs, vs = self.il_reset_tables()
        f = _abi.ILReset(n=N, out_flags=0, prev=ptr(prev), episode_steps=ptr(episode_steps), qpos_slot=ptr(qs),
                         qvel_slot=ptr(vs))
        if with_traj:
            f.cur_traj, f.cur_step, f.origin, f.sample = (t.data_ptr() for t in (cur_traj, cur_step, origin, sample))
        fn, h, ref = lib().oly_il_reset_where, self.ctx.handle, C.byref(f)
        keep = (prev, episode_steps, cur_traj, cur_step, origin, sample, qs, vs, f)     # alive with the closure
        f64_flag = _abi.OUT_OBS_F64

        def launch(mask, qpos, qvel, obs_in, obs_out, traj_no=None, step=None):
            if self.il_spec is not sp or self.traj_shape != shape:
                raise OlyError("il_reset_where: the engine was configured again after this launch was prepared")
            if (traj_no is not None) != with_traj:
                raise OlyError("il_reset_where: prepared " + ("with" if with_traj else "without") + " trajectory indices")
            f.mask = None if mask is None else mask.data_ptr()
            f.qpos, f.qvel, f.obs_in, f.obs_out = qpos.data_ptr(), qvel.data_ptr(), obs_in.data_ptr(), obs_out.data_ptr()
            f.out_flags = f64_flag if obs_in.dtype == f64 else 0
            if with_traj:
                f.traj_no, f.step = traj_no.data_ptr(), step.data_ptr()
            rc = fn(h, ref, self._s())
            if rc:
                check(h, rc, "oly_il_reset_where")
            return obs_out
        launch.keep = keep
        return launch

    def trpo_old_distribution(self, ws, n, in_dim, out_dim, hidden=(512, 256)):
        """Views (no copy) of the old distribution the last trpo_step on `ws` left in it: (mu_old [n,out] f32,
        log_sigma_old [out] f32), gail_TRPO.py:132-133."""
        from ._ffi import lib
        a, b = C.c_int64(), C.c_int64()
        rc = lib().oly_trpo_old_offsets(int(n), int(in_dim), int(hidden[0]), int(hidden[1]), int(out_dim), C.byref(a),
                                        C.byref(b))
        if rc != _abi.OLY_OK:
            raise OlyError(f"trpo_old_distribution: unsupported n={n} / policy {in_dim} -> {hidden} -> {out_dim}")
        need = int(lib().oly_trpo_ws_floats(int(n), int(in_dim), int(hidden[0]), int(hidden[1]), int(out_dim)))
        _req(ws, "ws", (need,), torch.float32, self.device)
        return ws[a.value:a.value + n * out_dim].view(n, out_dim), ws[b.value:b.value + out_dim]

    # -------------------------------------------------------------- K6
    # -------------------------------------------------------------- K17 (TRPO's policy step)
    def trpo_args(self, obs, act, adv, colstats, theta, max_kl=0.01, ent_coeff=0.0, n_epochs_cg=10, cg_damping=1e-1,
                  cg_residual_tol=1e-10, n_epochs_line_search=10, accept_rule="or", ws=None, packed=None,
                  stepdir_out=None, full_step_out=None, scal_out=None, last_act="identity", hidden=(512, 256)):
        """The oly_trpo_step_args block for obs [n,in] f32, act [n,out] f32, adv [n] (or [n,1]) f32, colstats [3,in]
        f64 (the live Standardizer) and theta [n_par] f32 (W1|b1|W2|b2|W3|b3|log_sigma).  Every shape is checked
        here, before anything can launch.  Returns (args, keep): keep holds the tensors the block points into."""
        from ._ffi import lib
        f32, dv = torch.float32, self.device
        if not isinstance(obs, torch.Tensor) or obs.dim() != 2 or not isinstance(act, torch.Tensor) or act.dim() != 2:
            raise OlyError("trpo: obs [n,in] and act [n,out] must be 2-D tensors")
        n, in_dim = (int(v) for v in obs.shape)
        out_dim = int(act.shape[1])
        if last_act != "identity":
            raise OlyError(f"trpo: the last activation must be identity (got {last_act!r}); a tanh mean is not supported")
        h1, h2 = (int(v) for v in hidden)
        n_par = int(lib().oly_trpo_param_count(in_dim, h1, h2, out_dim))
        if n_par < 0:
            raise OlyError(f"trpo: unsupported policy {in_dim} -> {h1} -> {h2} -> {out_dim} (in <= 64 -> 512 -> 256 -> out <= 32)")
        if n <= 0:
            raise OlyError("trpo: no rows")
        if accept_rule not in ("or", "and"):
            raise OlyError(f"trpo: accept_rule must be 'or' or 'and' (got {accept_rule!r})")
        if int(n_epochs_cg) < 1 or int(n_epochs_line_search) < 0:
            raise OlyError("trpo: n_epochs_cg >= 1 and n_epochs_line_search >= 0")
        nws = int(lib().oly_trpo_ws_floats(n, in_dim, h1, h2, out_dim))
        _req(obs, "obs", (n, in_dim), f32, dv)
        _req(act, "act", (n, out_dim), f32, dv)
        _req(adv, "adv", tuple(adv.shape) if adv.dim() == 2 and int(adv.shape[-1]) == 1 else (n,), f32, dv)
        if adv.numel() != n:
            raise OlyError(f"adv: {adv.numel()} values for {n} rows")
        _req(colstats, "colstats", (3, in_dim), torch.float64, dv)
        _req(theta, "theta", (n_par,), f32, dv)
        ws = _req(ws if ws is not None else self._new((nws,), f32), "ws", (nws,), f32, dv)
        _req(packed, "packed", (int(lib().oly_ilmlp_packed_floats(in_dim, h1, h2, out_dim)),), f32, dv, optional=True)
        _req(stepdir_out, "stepdir_out", (n_par,), f32, dv, optional=True)
        _req(full_step_out, "full_step_out", (n_par,), f32, dv, optional=True)
        scal_out = _req(scal_out if scal_out is not None else torch.zeros(_abi.OLY_TRPO_SCALARS, dtype=torch.float64,
                                                                          device=dv),
                        "scal_out", (_abi.OLY_TRPO_SCALARS,), torch.float64, dv)
        a = _abi.TRPOStep(n=n, in_dim=in_dim, hidden1=h1, hidden2=h2, out_dim=out_dim, last_act=_abi.ACT_IDENTITY,
                          n_epochs_cg=int(n_epochs_cg), n_epochs_line_search=int(n_epochs_line_search),
                          accept_rule=_abi.OLY_TRPO_ACCEPT_AND if accept_rule == "and" else _abi.OLY_TRPO_ACCEPT_OR,
                          max_kl=float(max_kl), ent_coeff=float(ent_coeff), cg_damping=float(cg_damping),
                          cg_residual_tol=float(cg_residual_tol), obs=obs.data_ptr(), act=act.data_ptr(),
                          adv=adv.data_ptr(), colstats=colstats.data_ptr(), theta=theta.data_ptr(),
                          packed=None if packed is None else packed.data_ptr(), ws=ws.data_ptr(), ws_floats=nws,
                          stepdir_out=None if stepdir_out is None else stepdir_out.data_ptr(),
                          full_step_out=None if full_step_out is None else full_step_out.data_ptr(),
                          scal_out=scal_out.data_ptr())
        return a, dict(ws=ws, scal=scal_out, n_par=n_par, n=n, out_dim=out_dim)

    def trpo_grad(self, obs, act, adv, colstats, theta, logp_old, k_stats=1, ent_coeff=0.0, grad_out=None, ws=None):
        """oly_trpo_grad: (grad [n_par] f32, J [1] f64) of TRPO's surrogate at colstats + k_stats c."""
        a, keep = self.trpo_args(obs, act, adv, colstats, theta, ent_coeff=ent_coeff, ws=ws)
        _req(logp_old, "logp_old", (keep["n"],), torch.float32, self.device)
        g = _req(grad_out if grad_out is not None else self._new((keep["n_par"],), torch.float32), "grad_out",
                 (keep["n_par"],), torch.float32, self.device)
        j = torch.zeros(1, dtype=torch.float64, device=self.device)
        self.ctx.call("oly_trpo_grad", C.byref(a), int(k_stats), ptr(logp_old), ptr(g), ptr(j), self._s())
        return g, j

    def trpo_fvp(self, obs, colstats, theta, mu_old, log_sigma_old, p, k_stats=1, cg_damping=1e-1, out=None, ws=None):
        """oly_trpo_fvp: Fvp(p) + cg_damping p [n_par] f32 at colstats + k_stats c against N(mu_old, exp(log_sigma_old)^2)."""
        n, out_dim = (int(v) for v in mu_old.shape)
        act = torch.zeros((n, out_dim), dtype=torch.float32, device=self.device)   # not read by the product
        adv = torch.zeros(n, dtype=torch.float32, device=self.device)
        a, keep = self.trpo_args(obs, act, adv, colstats, theta, cg_damping=cg_damping, ws=ws)
        _req(mu_old, "mu_old", (n, out_dim), torch.float32, self.device)
        _req(log_sigma_old, "log_sigma_old", (out_dim,), torch.float32, self.device)
        _req(p, "p", (keep["n_par"],), torch.float32, self.device)
        out = _req(out if out is not None else self._new((keep["n_par"],), torch.float32), "out", (keep["n_par"],),
                   torch.float32, self.device)
        self.ctx.call("oly_trpo_fvp", C.byref(a), int(k_stats), ptr(mu_old), ptr(log_sigma_old), ptr(p), ptr(out),
                      self._s())
        return out

    def trpo_step(self, obs, act, adv, colstats, theta, **kw):
        """oly_trpo_step: one TRPO policy step in one call (theta and colstats updated in place).  Returns the scalars
        [8] f64 on the device: prev_loss, CG iterations run, shs, accepted j (-1: restored), kl, J, line-search
        iterations run, last r.r."""
        a, keep = self.trpo_args(obs, act, adv, colstats, theta, **kw)
        self.ctx.call("oly_trpo_step", C.byref(a), self._s())
        return keep["scal"]

    def return_scan(self, mode, gamma, lam, rew, val, next_val, flags, ret=None, adv=None, stats3=None):
        """rew [T,N] float32, or float64 (RETURN mode: the un-narrowed reward of env.step).  With
        `stats3` ([3] f64 device tensor) the same pass also leaves (T*N, sum adv, sum adv^2) there."""
        if rew.dim() != 2:
            raise OlyError(f"rew: expected [T,N], got {tuple(rew.shape)}")
        T, N = int(rew.shape[0]), int(rew.shape[1])
        dv = self.device
        r64 = rew.dtype == torch.float64
        if r64 and int(mode) != _abi.SCAN_RETURN:
            raise OlyError("float64 rewards are defined for SCAN_RETURN only")
        _req(rew, "rew", (T, N), torch.float64 if r64 else torch.float32, dv)
        _req(val, "val", (T, N), torch.float32, dv)
        _req(next_val, "next_val", (T, N), torch.float32, dv)
        _req(flags, "flags", (T, N), torch.uint8, dv)
        _req(stats3, "stats3", (3,), torch.float64, dv, optional=True)
        ret = _req(ret if ret is not None else self._new((T, N), torch.float32), "ret", (T, N), torch.float32, dv)
        adv = _req(adv if adv is not None else self._new((T, N), torch.float32), "adv", (T, N), torch.float32, dv)
        self.ctx.call("oly_return_scan_stats", int(mode) | (_abi.SCAN_REW_F64 if r64 else 0), T, N, C.c_double(gamma),
                      C.c_double(lam), ptr(rew), ptr(val), ptr(next_val), ptr(flags), ptr(ret), ptr(adv), ptr(stats3),
                      self._s())
        return ret, adv

    def rollout_cuts(self, done, traj_len, flags, n_cut, max_traj_len, last_step):
        """PPO.sample's per-step episode-cut bookkeeping (traj_len / flags updated in place; n_cut [1] i32)."""
        N = int(done.shape[0])
        _req(done, "done", (N,), torch.uint8, self.device)
        _req(traj_len, "traj_len", (N,), torch.int32, self.device)
        _req(flags, "flags", (N,), torch.uint8, self.device)
        _req(n_cut, "n_cut", (1,), torch.int32, self.device)
        self.ctx.call("oly_rollout_cuts", N, int(max_traj_len), int(bool(last_step)), ptr(done), ptr(traj_len), ptr(flags),
                      ptr(n_cut), self._s())
        return flags

    # -------------------------------------------------------------- K7
    def adv_stats(self, x, stats3=None):
        _req(x, "x", x.shape, torch.float32, self.device)
        stats3 = _req(stats3 if stats3 is not None else self._new((3,), torch.float64), "stats3", (3,), torch.float64, self.device)
        self.ctx.call("oly_adv_stats", C.c_int64(x.numel()), ptr(x), ptr(stats3), self._s())
        return stats3

    def adv_normalize(self, x, stats3, ddof, eps):
        """stats3: [3] (one triple) or [parts,3] (one triple per rank, as all-gathered)."""
        _req(x, "x", x.shape, torch.float32, self.device)
        parts = 1 if stats3.dim() == 1 else int(stats3.shape[0])
        if not 1 <= parts <= _abi.OLY_MAX_STAT_PARTS:
            raise OlyError(f"stats3: {parts} parts, at most {_abi.OLY_MAX_STAT_PARTS}")
        _req(stats3, "stats3", (3,) if stats3.dim() == 1 else (parts, 3), torch.float64, self.device)
        self.ctx.call("oly_adv_normalize_parts", C.c_int64(x.numel()), ptr(x), ptr(stats3), parts, int(ddof),
                      C.c_double(eps), self._s())
        return x

    def col_stats(self, x, colstats=None):
        if x.dim() != 2:
            raise OlyError(f"x: expected [B,D], got {tuple(x.shape)}")
        B, D = int(x.shape[0]), int(x.shape[1])
        _req(x, "x", (B, D), torch.float32, self.device)
        acc = colstats is not None
        colstats = _req(colstats if acc else self._new((3, D), torch.float64), "colstats", (3, D), torch.float64, self.device)
        self.ctx.call("oly_col_stats", B, D, ptr(x), ptr(colstats), int(acc), self._s())
        return colstats

    # -------------------------------------------------------------- K3 (IL ground forces)
    def grf_configure(self, geom_group, pairs):
        """geom_group [ngeom] (collision-group index per geom, -1 none); pairs [(group_a, group_b), ...]."""
        gg = np.ascontiguousarray(geom_group, dtype=np.int32)
        pa = np.ascontiguousarray([a for a, _ in pairs], dtype=np.int32)
        pb = np.ascontiguousarray([b for _, b in pairs], dtype=np.int32)
        self.ctx.call("oly_grf_configure", len(gg), ptr(gg), len(pairs), ptr(pa), ptr(pb))
        self.n_grf_pairs = len(pairs)
        return self

    def il_ground_forces(self, ncon, geom1, geom2, force6, want_steps=False, check=False):
        """[W,N,...] substep contact slots -> dict(mean [N,3P], steps [W,N,3P] or None, overflow [N] u8).
        `ncon` is the raw data.ncon.  An environment whose count exceeded the staged slots in a substep where a
        sensor pair found no contact among them cannot be reproduced (the reference scans every contact,
        UnitreeH1.py:113-123): the kernel flags it in `overflow` and the caller owns those bytes (VecLocoEnv keeps a
        sticky copy and reads it in its next host round trip: reset() / raise_if_contact_overflow()).  check=True reads
        them back HERE: a blocking device-to-host round trip per call, which also breaks graph capture of the caller."""
        if not getattr(self, "n_grf_pairs", 0):
            raise OlyError("il_ground_forces before grf_configure")
        W, N, Cc = (int(v) for v in geom1.shape)
        _req(ncon, "ncon", (W, N), torch.int32, self.device)
        _req(geom1, "geom1", (W, N, Cc), torch.int32, self.device)
        _req(geom2, "geom2", (W, N, Cc), torch.int32, self.device)
        _req(force6, "force6", (W, N, Cc, 6), torch.float64, self.device)
        k = 3 * self.n_grf_pairs
        mean = self._new((N, k), torch.float64)
        steps = self._new((W, N, k), torch.float64) if want_steps else None
        over = self._new((N,), torch.uint8)
        self.ctx.call("oly_il_ground_forces", W, N, Cc, ptr(ncon), ptr(geom1), ptr(geom2), ptr(force6), ptr(steps),
                      ptr(mean), ptr(over), self._s())
        if check and N and bool(over.any().item()):
            bad = torch.nonzero(over).flatten()[:8].tolist()
            raise OlyError(f"il_ground_forces: more contacts than the {Cc} staged slots and a sensor pair without a "
                           f"contact among them (or a negative count) in environments {bad}: stage more slots")
        return dict(mean=mean, steps=steps, overflow=over)

    def il_grf_window(self, grf_step, mean=None):
        """[W,N,K] per-substep ground-force rows -> [N,K] window mean (sum in substep order / W)."""
        W, N, K = (int(v) for v in grf_step.shape)
        _req(grf_step, "grf_step", (W, N, K), torch.float64, self.device)
        mean = _req(mean if mean is not None else self._new((N, K), torch.float64), "mean", (N, K), torch.float64,
                    self.device)
        self.ctx.call("oly_il_grf_window", W, N, K, ptr(grf_step), ptr(mean), self._s())
        return mean

    # -------------------------------------------------------------- K8
    def disc_standardize(self, x, mask, mean, std, out=None):
        B, Dx = int(x.shape[0]), int(x.shape[1])
        _req(x, "x", (B, Dx), torch.float32, self.device)
        D = Dx if mask is None else int(mask.shape[0])
        _req(mask, "mask", (D,), torch.int32, self.device, optional=True)
        _req(mean, "mean", (D,), torch.float64, self.device)
        _req(std, "std", (D,), torch.float64, self.device)
        out = _req(out if out is not None else self._new((B, D), torch.float32), "out", (B, D), torch.float32, self.device)
        self.ctx.call("oly_disc_standardize", B, Dx, D, ptr(x), ptr(mask), ptr(mean), ptr(std), ptr(out), self._s())
        return out

    def obs_filter(self, x, mean, var, eps=1e-8, clip=10.0, out=None):
        """Normalize._obfilt on a [B,D] float32 batch (out may be x itself)."""
        B, D = int(x.shape[0]), int(x.shape[1])
        _req(x, "x", (B, D), torch.float32, self.device)
        _req(mean, "mean", (D,), torch.float64, self.device)
        _req(var, "var", (D,), torch.float64, self.device)
        out = _req(out if out is not None else self._new((B, D), torch.float32), "out", (B, D), torch.float32, self.device)
        self.ctx.call("oly_obs_filter", B, D, ptr(x), ptr(mean), ptr(var), float(eps), float(clip or 0.0), ptr(out),
                      self._s())
        return out

    def disc_reparam(self, mu, logvar, eps, z=None):
        for t, nme in ((mu, "mu"), (logvar, "logvar"), (eps, "eps")):
            _req(t, nme, mu.shape, torch.float32, self.device)
        z = _req(z if z is not None else self._new(tuple(mu.shape), torch.float32), "z", mu.shape, torch.float32, self.device)
        self.ctx.call("oly_disc_reparam", C.c_int64(mu.numel()), ptr(mu), ptr(logvar), ptr(eps), ptr(z), self._s())
        return z

    def disc_reward(self, logits, reward=None):
        _req(logits, "logits", logits.shape, torch.float32, self.device)
        reward = _req(reward if reward is not None else self._new((logits.numel(),), torch.float32), "reward",
                      (logits.numel(),), torch.float32, self.device)
        self.ctx.call("oly_disc_reward", C.c_int64(logits.numel()), ptr(logits), ptr(reward), self._s())
        return reward

    # -------------------------------------------------------------- K12 (fused discriminator forward)
    def disc_pack(self, enc_w0, enc_b0, enc_w1, enc_b1, mu_w, mu_b, lv_w, lv_b, dec_w, dec_b, packed=None):
        """torch parameters of the variational discriminator in -> 256 -> 128 -> (mu, logvar) 128 -> 1
        -> packed operand stream of oly_disc_forward."""
        from ._ffi import lib
        f32, dv = torch.float32, self.device
        H, in_dim = (int(v) for v in enc_w0.shape)
        E, Z = int(enc_w1.shape[0]), int(mu_w.shape[0])
        n = int(lib().oly_disc_packed_floats(in_dim, H, E, Z))
        if n < 0:
            raise OlyError(f"disc_pack: unsupported discriminator shape {in_dim} -> {H} -> {E} -> {Z} -> 1")
        for t, name, shape in ((enc_w0, "enc_w0", (H, in_dim)), (enc_b0, "enc_b0", (H,)), (enc_w1, "enc_w1", (E, H)),
                               (enc_b1, "enc_b1", (E,)), (mu_w, "mu_w", (Z, E)), (mu_b, "mu_b", (Z,)),
                               (lv_w, "lv_w", (Z, E)), (lv_b, "lv_b", (Z,)), (dec_w, "dec_w", (1, Z)),
                               (dec_b, "dec_b", (1,))):
            _req(t, name, shape, f32, dv)
        packed = _req(packed if packed is not None else self._new((n,), f32), "packed", (n,), f32, dv)
        self.ctx.call("oly_disc_pack", in_dim, H, E, Z, ptr(enc_w0), ptr(enc_b0), ptr(enc_w1), ptr(enc_b1), ptr(mu_w),
                      ptr(mu_b), ptr(lv_w), ptr(lv_b), ptr(dec_w), ptr(dec_b), ptr(packed), self._s())
        return packed

    def disc_forward(self, x, packed, mask=None, mean=None, std=None, colstats=None, eps=None, want=("reward",),
                     out=None):
        """make_discrim_reward for x [B,Dx] f32 in one launch.  want: any of reward / logits / mu / logvar.
        Standardisation from mean / std [D] f64, or from the running colstats [3,D] of col_stats, or none."""
        from ._ffi import lib
        f32, dv = torch.float32, self.device
        B, Dx = (int(v) for v in x.shape)
        D = Dx if mask is None else int(mask.shape[0])
        _req(x, "x", (B, Dx), f32, dv)
        _req(mask, "mask", (D,), torch.int32, dv, optional=True)
        if (mean is None) != (std is None) or (mean is not None and colstats is not None):
            raise OlyError("disc_forward: give mean and std together, or colstats, or neither")
        _req(colstats, "colstats", (3, D), torch.float64, dv, optional=True)
        _req(mean, "mean", (D,), torch.float64, dv, optional=True)
        _req(std, "std", (D,), torch.float64, dv, optional=True)
        cache = self.__dict__.setdefault("_disc_sizes", {})
        if D not in cache:
            cache[D] = int(lib().oly_disc_packed_floats(D, 256, 128, 128))
        _req(packed, "packed", (cache[D],), f32, dv)        # the raw pointer carries no length
        _req(eps, "eps", (B, 128), f32, dv, optional=True)
        shapes = dict(reward=(B,), logits=(B,), mu=(B, 128), logvar=(B, 128))
        out = dict(out or {})
        for k in want:
            if k not in shapes:
                raise OlyError(f"disc_forward: unknown output {k!r}")
            out[k] = _req(out.get(k) if out.get(k) is not None else self._new(shapes[k], f32), k, shapes[k], f32, dv)
        if not want:
            raise OlyError("disc_forward: no output requested")
        g = lambda k: ptr(out[k]) if k in want else None
        self.ctx.call("oly_disc_forward", C.c_int64(B), Dx, D, ptr(x), ptr(mask), ptr(mean), ptr(std), ptr(colstats),
                      ptr(packed), ptr(eps), g("reward"), g("logits"), g("mu"), g("logvar"), self._s())
        return out

    def disc_reward_step(self, x, packed, colstats, accumulate, eps=None, want=("reward",), out=None, weights=None):
        """oly_disc_reward_step: (re-pack of `weights`, the ten parameter tensors in oly_disc_pack's order, when given,)
        the Standardizer's running update with x (into colstats [3,D] f64, accumulate: added to the running sums) and
        the fused forward on the updated statistics, one C call.  x [B,D] f32, whole rows.  accumulate=None: validate
        now and return `launch(accumulate)` for repeated calls on the same tensors."""
        from ._ffi import lib
        f32, dv = torch.float32, self.device
        B, D = (int(v) for v in x.shape)
        _req(x, "x", (B, D), f32, dv)
        _req(colstats, "colstats", (3, D), torch.float64, dv)
        cache = self.__dict__.setdefault("_disc_sizes", {})
        if D not in cache:
            cache[D] = int(lib().oly_disc_packed_floats(D, 256, 128, 128))
        _req(packed, "packed", (cache[D],), f32, dv)
        _req(eps, "eps", (B, 128), f32, dv, optional=True)
        wp = None
        if weights is not None:
            shapes_w = ((256, D), (256,), (128, 256), (128,), (128, 128), (128,), (128, 128), (128,), (1, 128), (1,))
            if len(weights) != 10:
                raise OlyError("disc_reward_step: weights = the ten tensors of disc_pack")
            for i, (t, sh) in enumerate(zip(weights, shapes_w)):
                _req(t, f"weights[{i}]", sh, f32, dv)
            wp = (C.c_void_p * 10)(*[t.data_ptr() for t in weights])
        shapes = dict(reward=(B,), logits=(B,), mu=(B, 128), logvar=(B, 128))
        out = dict(out or {})
        if not want:
            raise OlyError("disc_reward_step: no output requested")
        for k in want:
            if k not in shapes:
                raise OlyError(f"disc_reward_step: unknown output {k!r}")
            out[k] = _req(out.get(k) if out.get(k) is not None else self._new(shapes[k], f32), k, shapes[k], f32, dv)
        g = lambda k: ptr(out[k]) if k in want else None
        if accumulate is None:
            # validated once: `launch(accumulate)` re-issues the same call on the current stream with no per-call checks
            # (at B = 4096 the kernels take ~20 us; the checks above cost the host more than that)
            from ._ffi import check
            fn, h = lib().oly_disc_reward_step, self.ctx.handle
            args = (C.c_int64(B), D, ptr(x), ptr(colstats))
            tail = (wp, ptr(packed), ptr(eps), g("reward"), g("logits"), g("mu"), g("logvar"))
            keep = (x, colstats, packed, eps, weights, out)

            def launch(acc):
                rc = fn(h, *args, 1 if acc else 0, *tail, self._s())
                if rc:
                    check(h, rc, "oly_disc_reward_step")
                return keep[-1]
            return launch
        self.ctx.call("oly_disc_reward_step", C.c_int64(B), D, ptr(x), ptr(colstats), int(bool(accumulate)), wp, ptr(packed),
                      ptr(eps), g("reward"), g("logits"), g("mu"), g("logvar"), self._s())
        return out

    # -------------------------------------------------------------- K9
    def signed_perm(self, x, src, sign, out=None):
        B, D = int(x.shape[0]), int(x.shape[1])
        _req(x, "x", (B, D), torch.float32, self.device)
        _req(src, "src", (D,), torch.int32, self.device)
        _req(sign, "sign", (D,), torch.float32, self.device)
        out = _req(out if out is not None else self._new((B, D), torch.float32), "out", (B, D), torch.float32, self.device)
        self.ctx.call("oly_signed_perm", B, D, ptr(x), ptr(src), ptr(sign), ptr(out), self._s())
        return out

    def mirror_loss(self, det, mir, src, sign, want_grad=True):
        """-> (loss [1] f64, grad_det, grad_mir)."""
        B, A = int(det.shape[0]), int(det.shape[1])
        _req(det, "det", (B, A), torch.float32, self.device)
        _req(mir, "mir", (B, A), torch.float32, self.device)
        _req(src, "src", (A,), torch.int32, self.device)
        _req(sign, "sign", (A,), torch.float32, self.device)
        loss = self._new((1,), torch.float64)
        gd = self._new((B, A), torch.float32) if want_grad else None
        gm = self._new((B, A), torch.float32) if want_grad else None
        self.ctx.call("oly_mirror_loss", B, A, ptr(det), ptr(mir), ptr(src), ptr(sign), ptr(loss), ptr(gd), ptr(gm),
                      self._s())
        return loss, gd, gm

    def _std_arg(self, std, B, A, name):
        if std.numel() == 1:
            mode, shape = _abi.STD_SCALAR, (1,)
        elif std.numel() == A:
            mode, shape = _abi.STD_PER_DIM, (A,)
        else:
            mode, shape = _abi.STD_FULL, (B, A)
        return _req(std.reshape(shape), name, shape, torch.float32, self.device), mode

    def ppo_loss(self, mu, std, old_mu, old_std, action, adv, ret, value, clip, vf_coeff=0.5, want_grad=True,
                 want_grad_std=False):
        """-> dict(scal [5] f64: actor, entropy_penalty, critic, approx_kl, clip_fraction;
        grad_mu [B,A], grad_std [B,A] or None, grad_value [B])."""
        B, A = int(mu.shape[0]), int(mu.shape[1])
        for t, nme in ((mu, "mu"), (old_mu, "old_mu"), (action, "action")):
            _req(t, nme, (B, A), torch.float32, self.device)
        std, sm = self._std_arg(std, B, A, "std")
        old_std, om = self._std_arg(old_std, B, A, "old_std")
        adv, ret, value = (_req(t.reshape(B), nme, (B,), torch.float32, self.device)
                           for t, nme in ((adv, "adv"), (ret, "ret"), (value, "value")))
        scal = self._new((5,), torch.float64)
        gmu = self._new((B, A), torch.float32) if want_grad else None
        gsd = self._new((B, A), torch.float32) if want_grad_std else None
        gv = self._new((B,), torch.float32) if want_grad else None
        self.ctx.call("oly_ppo_loss", B, A, ptr(mu), ptr(std), sm, ptr(old_mu), ptr(old_std), om, ptr(action),
                      ptr(adv), ptr(ret), ptr(value), float(clip), float(vf_coeff), ptr(scal), ptr(gmu), ptr(gsd),
                      ptr(gv), self._s())
        return dict(scal=scal, grad_mu=gmu, grad_std=gsd, grad_value=gv)
