"""K23 without a GPU: the numpy restatement of record(seed, n, k) (tests/a3_reset_draw_restate.py) against the host function
the device path replaces, the generator against its published vectors, the distribution of the draws, and the C ABI of
oly_a3_reset_draw.

The restatement is tied to vecstep.draw_reset_records, which tests/test_gpu_vecstep.py ties to the reference's
WalkingTask.reset; tests/test_gpu_a3_reset_draw.py ties the kernel to the restatement byte for byte.

Distribution bounds: 65 536 records, every frequency within 5 binomial standard deviations of its probability
(sqrt(0.2 * 0.8 / 65536) = 0.00156 -> 0.0078; sqrt(0.25 / 65536) = 0.00195 -> 0.0098), the mean of `first` within
5 * 0.01 / sqrt(12 * 65536) = 5.6e-5 of 0.1, sample correlations below 5 / sqrt(65536)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import a3_reset_draw_restate as R
from olympic_hip import _abi, specs
from olympic_hip._ffi import OlyError
from olympic_hip.vecstep import A3DeviceRollout, draw_reset_records, step_height_abs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EEDFACE12345678


class StubStream:
    """A numpy stream whose choice / uniform / randint return given draws, in draw_reset_records' call order."""

    def __init__(self, d, period, h):
        self.answers = [("choice", np.where(d["phase"] != 0, period / 2, 0.0)), ("choice", d["mode"]),
                        ("choice", d["step_height"]), ("uniform", d["first"]), ("randint", d["c"])]
        self.period, self.h = period, h

    def _next(self, name, size):
        want, out = self.answers.pop(0)
        assert want == name and out.shape == (size,)
        return out.copy()

    def choice(self, options, size, p=None):
        out = self._next("choice", size)
        assert set(np.unique(out).tolist()) <= set(np.asarray(options, dtype=np.float64).tolist())
        return out

    def uniform(self, low, high, size):
        assert (low, high) == (0.095, 0.105)
        return self._next("uniform", size)

    def randint(self, low, high, size):
        assert (low, high) == (2, 4)
        return self._next("randint", size)


@pytest.mark.parametrize("iter_count,h", [(0, 0.0), (3000, 0.0), (7000, 0.05), (20000, 0.1)])
def test_restatement_equals_the_host_function(iter_count, h):
    spec = specs.A3Spec(mass=41.5)
    assert R.step_height(iter_count) == step_height_abs(iter_count) == h
    n = np.repeat(np.arange(37), 11)
    k = np.tile(np.array([0, 1, 2, 3, 5, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 7, 2 ** 40, 2 ** 63 + 1], dtype=np.uint64), 37)
    d = R.draws(SEED, n, k, spec.period, h)
    assert len(np.unique(d["mode"])) == 2 and len(np.unique(d["phase"])) == 2 and len(np.unique(d["c"])) == 2
    stub = StubStream(d, spec.period, h)
    host = draw_reset_records(stub, len(n), spec, iter_count)
    assert not stub.answers
    rec = R.records(SEED, n, k, spec.period, h)
    assert host.tobytes() == rec.tobytes()
    # and what the bytes mean
    fwd = rec["mode"] == _abi.MODE_FORWARD
    assert np.array_equal(rec["seq_len"], np.where(fwd, 20, 1)) and not rec["pad"].any()
    assert not rec["seq"][~fwd, 1:].any() and np.array_equal(np.abs(rec["seq"][:, 0, 1]), d["first"])
    assert np.all(rec["seq"][fwd, 19, 0] > 5.69) and np.all(np.abs(rec["seq"][fwd, 19, 2]) <= 17 * h + 1e-12)
    if h:
        assert np.array_equal(rec["seq"][fwd, 4, 2], d["step_height"][fwd] * (4 - d["c"][fwd]))


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32, 10 rounds."""
    ones = 0xFFFFFFFF
    cases = [([0, 0, 0, 0], [0, 0], [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]),
             ([ones] * 4, [ones] * 2, [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]),
             ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0],
              [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1])]
    for ctr, key, want in cases:
        assert R.philox4x32_10(ctr, key).tolist() == want
    got = R.philox4x32_10([c for c, _, _ in cases], [k for _, k, _ in cases])          # vectorised over leading axes
    assert got.tolist() == [w for _, _, w in cases]


def _corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def test_distribution_of_the_draws():
    N, K, period = 4096, 16, 88
    d = R.draws(SEED, np.arange(N)[:, None], np.arange(K)[None, :], period, 0.05)
    assert d["mode"].shape == (N, K)
    freq = {"standing": (d["mode"] == _abi.MODE_STANDING).mean(), "half phase": (d["phase"] == period // 2).mean(),
            "positive height": (d["step_height"] > 0).mean(), "c = 3": (d["c"] == 3).mean()}
    first, u = d["first"], d["u"]
    stats = dict(freq, first_mean=first.mean(), corr_ordinals=_corr(u[:, :-1].ravel(), u[:, 1:].ravel()),
                 corr_environments=_corr(u[:-1].ravel(), u[1:].ravel()))
    print(stats)
    assert abs(freq["standing"] - 0.2) <= 0.0078
    for name in ("half phase", "positive height", "c = 3"):
        assert abs(freq[name] - 0.5) <= 0.0098, name
    assert set(np.unique(d["mode"])) == {_abi.MODE_STANDING, _abi.MODE_FORWARD} and set(np.unique(d["c"])) == {2, 3}
    assert first.min() >= 0.095 and first.max() < 0.105 and u.min() >= 0.0 and u.max() < 1.0
    assert abs(stats["first_mean"] - 0.1) <= 5.6e-5
    assert abs(stats["corr_ordinals"]) < 5 / np.sqrt(65536) and abs(stats["corr_environments"]) < 5 / np.sqrt(65536)
    # another seed, another sequence
    other = R.draws(SEED + 1, np.arange(N)[:, None], np.arange(K)[None, :], period, 0.05)
    assert abs(_corr(u.ravel(), other["u"].ravel())) < 5 / np.sqrt(65536)


def test_ring_is_indexed_by_base():
    base = np.array([0, 5, 2 ** 32 - 1, 2 ** 32 + 7], dtype=np.uint64)
    ring = R.ring(SEED, base, 3, 88, 0.1)
    assert ring.shape == (4, 3)
    for n in range(4):
        for j in range(3):
            assert ring[n, j].tobytes() == R.records(SEED, n, int(base[n]) + j, 88, 0.1).tobytes()
    moved = R.ring(SEED, base + np.uint64(2), 3, 88, 0.1)
    assert moved[:, 0].tobytes() == ring[:, 2].tobytes()


def test_an_unknown_draw_mode_is_refused():
    with pytest.raises(OlyError, match="draw is 'host' or 'device', not 'x'"):
        A3DeviceRollout(None, None, draw="x")


def test_header_abi_and_library_agree():
    raw = open(os.path.join(ROOT, "include", "olympic_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    proto = re.search(r"\bint\s+oly_a3_reset_draw\s*\(([^)]*)\)\s*;", txt)
    assert proto
    args = [re.sub(r"\s+", " ", a).strip() for a in proto.group(1).split(",")]
    assert args == ["oly_ctx* ctx", "oly_a3_reset_record* pool", "int N", "int pool_depth", "uint64_t seed", "int64_t* base",
                    "int32_t* pool_count", "double step_height_abs", "int period", "oly_stream stream"]
    C, vp = ctypes, ctypes.c_void_p
    assert _abi.SIGNATURES["oly_a3_reset_draw"] == (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_uint64, vp, vp, C.c_double,
                                                              C.c_int, vp])
    assert int(re.search(r"#define OLY_ABI_VERSION (\d+)", txt).group(1)) == _abi.ABI_VERSION == 8
    block = raw[raw.index("K23 :"):raw.index("int oly_a3_reset_draw")]
    for cite in ("walking_task.py:137-182,353-392", "0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "858993459"):
        assert cite in block, cite
    from olympic_hip import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        pytest.fail(f"{_ffi.LIB_PATH} missing: run python __graft_entry__.py build")
    L = _ffi.lib()
    assert int(L.oly_abi_version()) == 8
    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.LIB_PATH], text=True)
    assert re.search(r" T oly_a3_reset_draw\b", out)
    # the argument refusals need a context, hence a device (tests/test_gpu_a3_reset_draw.py); without one nothing is launched
    assert L.oly_a3_reset_draw(None, None, 4, 4, 1, None, None, 0.0, 88, None) == _abi.OLY_EINVAL
