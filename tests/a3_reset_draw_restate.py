"""K23 restated in numpy (a helper, not collected): Philox4x32-10 and record(seed, n, k), written from the specification in
include/olympic_hip.h's K23 block, not from the kernel.

    philox4x32_10(ctr [..., 4], key [..., 2]) -> [..., 4] uint32
    draws(seed, n, k, period, h) -> dict of the five draws per (n, k) pair (arrays of one shape)
    records(seed, n, k, period, h) -> vecstep.REC array, one record per (n, k) pair
    ring(seed, base [N], depth, period, h) -> REC array [N, depth]: slot j of environment n = record(seed, n, base[n] + j)
"""
import numpy as np

from olympic_hip import _abi
from olympic_hip.vecstep import REC

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
P_STANDING = 858993459            # floor(0.2 * 2^32)
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    c = [np.asarray(ctr, dtype=np.uint64)[..., i] & MASK for i in range(4)]
    k = [np.asarray(key, dtype=np.uint64)[..., i] & MASK for i in range(2)]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]          # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return np.stack(c, axis=-1).astype(np.uint32)


def step_height(iter_count):
    """h(iteration): formed on the host in float64 and passed to the kernel."""
    return float(np.clip((iter_count - 3000) / 8000, 0, 1) * 0.1)


def draws(seed, n, k, period, h):
    n, k = np.broadcast_arrays(np.asarray(n, dtype=np.uint64), np.asarray(k, dtype=np.uint64))
    seed = int(seed)
    ctr = np.stack([k & MASK, k >> np.uint64(32), n & MASK, np.zeros_like(n)], axis=-1)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64), n.shape + (2,))
    r = philox4x32_10(ctr, key).astype(np.uint64)
    r0, r1, r2, r3 = (r[..., i] for i in range(4))
    bit = lambda b: ((r1 >> np.uint64(b)) & np.uint64(1)).astype(bool)
    u = ((r2 >> np.uint64(5)).astype(np.float64) * 2.0 ** 26 + (r3 >> np.uint64(6)).astype(np.float64)) * 2.0 ** -53
    return dict(mode=np.where(r0 < P_STANDING, _abi.MODE_STANDING, _abi.MODE_FORWARD),
                phase=np.where(bit(31), period // 2, 0), step_height=np.where(bit(30), h, -h),
                c=2 + bit(29).astype(np.int64), u=u, first=0.095 + (0.105 - 0.095) * u)


def records(seed, n, k, period, h):
    d = draws(seed, n, k, period, h)
    shape = d["mode"].shape
    rec = np.zeros(shape, REC)
    half = d["phase"] == 0.5 * period
    fwd = d["mode"] == _abi.MODE_FORWARD
    seq = np.zeros(shape + (_abi.OLY_MAX_SEQ, 4))
    seq[..., 0, 1] = np.where(half, -d["first"], d["first"])
    x, y, z = np.zeros(shape), np.where(half, -0.15, 0.15), np.zeros(shape)
    for i in range(1, 20):
        x = x + 0.3
        y = -y
        z = np.where(i > d["c"], z + d["step_height"], z)
        seq[..., i, 0], seq[..., i, 1], seq[..., i, 2] = x, y, z
    seq[~fwd, 1:] = 0.0
    rec["mode"], rec["phase"], rec["seq_len"], rec["pad"], rec["seq"] = d["mode"], d["phase"], np.where(fwd, 20, 1), 0, seq
    return rec


def ring(seed, base, depth, period, h):
    base = np.asarray(base, dtype=np.uint64)
    n = np.arange(len(base), dtype=np.uint64)[:, None]
    return records(seed, n, base[:, None] + np.arange(depth, dtype=np.uint64)[None, :], period, h)
