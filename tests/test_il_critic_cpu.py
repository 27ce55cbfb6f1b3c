"""K16 without a GPU: the reference-pinned critic-fit fixture, a float64 restatement of the epoch, and the C ABI
entries of oly_ilmlp_* / oly_il_critic_fit_epoch."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from olympic_hip import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "il_critic", "il_critic_fit.npz")
NAMES = ("w1", "b1", "w2", "b2", "w3", "b3")


def w2_init():
    """Layer 2's initial weight as tests/golden/gen_il_critic.py draws it (not stored in the fixture)."""
    g = np.random.default_rng(7).standard_normal((256, 512))
    return (g / np.sqrt(np.sum(np.square(g)))).astype(np.float32)


def initial_params(g):
    return [w2_init() if n == "w2" else g[f"init_{n}"] for n in NAMES]


def initial_colstats(g):
    """The fixture's Standardizer before the fit as raw (count, sum, sumsq) rows (its _count / _sumsq start at 1e-2)."""
    cnt = np.full(g["st0_sum"].shape, float(g["st0_count"][0]) - 1e-2)
    return np.stack([cnt, g["st0_sum"].astype(np.float64), g["st0_sumsq"].astype(np.float64) - 1e-2])


def restate_fit(x, vt, perms, params, colstats, lr, batch, step0=0, moments=None, dtype=torch.float64, device="cpu",
                betas=(0.9, 0.999), eps=1e-8):
    """The critic's epochs in torch: per minibatch the Standardizer update (networks.py:76-81, sums in fp64), the
    standardisation f32((f64(x) - mean) / std) (networks.py:68-74), the forward in->512->256->1 (relu, relu,
    identity), F.mse_loss (mean over the minibatch), backward, and torch's default Adam step.
    Returns (params, moments, colstats, losses, step)."""
    x = torch.as_tensor(x, device=device)
    vt = torch.as_tensor(vt, device=device).reshape(-1, 1).to(dtype)
    P = [torch.as_tensor(p, device=device).to(dtype).clone() for p in params]
    M = [torch.zeros_like(p) for p in P] if moments is None else [m.clone() for m in moments[0]]
    V = [torch.zeros_like(p) for p in P] if moments is None else [v.clone() for v in moments[1]]
    cs = torch.as_tensor(colstats, device=device).to(torch.float64).clone()
    losses, step, n = [], step0, x.shape[0]
    for perm in perms:
        perm = torch.as_tensor(np.asarray(perm, dtype=np.int64), device=device)
        for b in range((n + batch - 1) // batch):
            idx = perm[b * batch:min(n, (b + 1) * batch)]
            xb = x[idx].to(torch.float64)
            cs[0] += xb.shape[0]
            cs[1] += xb.sum(0)
            cs[2] += (xb * xb).sum(0)
            cnt = cs[0] + 1e-2
            mean = cs[1] / cnt
            sd = torch.sqrt(torch.clamp((cs[2] + 1e-2) / cnt - mean * mean, min=1e-2))
            xs = ((xb - mean) / sd).to(torch.float32).to(dtype)
            for p in P:
                p.requires_grad_(True)
            h1 = torch.relu(xs @ P[0].T + P[1])
            h2 = torch.relu(h1 @ P[2].T + P[3])
            y = h2 @ P[4].T + P[5]
            loss = torch.nn.functional.mse_loss(y, vt[idx])
            grads = torch.autograd.grad(loss, P)
            losses.append(float(loss.detach()))
            step += 1
            bc1, bc2 = 1 - betas[0] ** step, 1 - betas[1] ** step
            with torch.no_grad():
                for i in range(6):
                    p, gr = P[i].detach(), grads[i]
                    M[i] = M[i] + (gr - M[i]) * (1 - betas[0])
                    V[i] = V[i] * betas[1] + (1 - betas[1]) * gr * gr
                    P[i] = p - (lr / bc1) * (M[i] / (torch.sqrt(V[i]) / bc2 ** 0.5 + eps))
    return [p.detach() for p in P], (M, V), cs, np.array(losses), step


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _reference_dir():
    sys.path.insert(0, GOLDEN)
    import _ref_stubs
    return _ref_stubs.REF


@pytest.mark.skipif(not os.path.isdir(_reference_dir()), reason="the reference tree is only in the build container")
def test_fixture_regenerates_byte_for_byte(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "gen_il_critic.py"), "--out", str(tmp_path)],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONHASHSEED="random"))
    assert r.returncode == 0, r.stderr[-2000:]
    a, b = np.load(FIXTURE), np.load(str(tmp_path / "il_critic_fit.npz"))
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert a[k].tobytes() == b[k].tobytes(), f"{k} does not regenerate"


def test_fixture_shape():
    g = np.load(FIXTURE)
    assert g["x"].shape == (1000, 32) and g["x"].shape[0] % 256 != 0
    assert g["perms"].shape == (2, 1000) and all(sorted(p) == list(range(1000)) for p in g["perms"])
    assert g["losses"].shape == (2 * 4,)
    assert os.path.getsize(FIXTURE) < 1 << 20


def test_float64_restatement_reproduces_the_reference_fit():
    g = np.load(FIXTURE)
    P, _, cs, losses, step = restate_fit(g["x"], g["v_target"], g["perms"], initial_params(g), initial_colstats(g),
                                         float(g["lr"]), int(g["batch"]))
    assert step == 8
    for n, p in zip(NAMES, P):
        assert rel(p.numpy(), g[f"final_{n}"]) <= 1e-6, n
        # and the fit moved every tensor far beyond that tolerance
        init = w2_init() if n == "w2" else g[f"init_{n}"]
        assert rel(init, g[f"final_{n}"]) > 1e-4, n
    np.testing.assert_allclose(losses, g["losses"], rtol=2e-6)
    # the Standardizer's own sums (float32 in numpy) against the fp64 running sums
    np.testing.assert_allclose(cs[0].numpy() + 1e-2, np.full(32, g["st_count"][0]), rtol=0, atol=1e-9)
    np.testing.assert_allclose(cs[1].numpy(), g["st_sum"], rtol=1e-6, atol=1e-3)
    np.testing.assert_allclose(cs[2].numpy() + 1e-2, g["st_sumsq"], rtol=1e-6)


def test_forward_restatement_reproduces_v0():
    """V(x) before the fit: the reference forward after its own statistics update of the same rows."""
    g = np.load(FIXTURE)
    w1, b1, w2, b2, w3, b3 = (torch.as_tensor(p).double() for p in initial_params(g))
    x = torch.as_tensor(g["x"]).double()
    cs = initial_colstats(g)
    cnt = cs[0] + 1e-2
    mean = cs[1] / cnt
    sd = np.sqrt(np.maximum((cs[2] + 1e-2) / cnt - mean * mean, 1e-2))
    xs = ((x - torch.as_tensor(mean)) / torch.as_tensor(sd)).float().double()
    y = torch.relu(torch.relu(xs @ w1.T + b1) @ w2.T + b2) @ w3.T + b3
    np.testing.assert_allclose(y.numpy(), g["v0"], rtol=1e-4, atol=1e-6)


# ------------------------------------------------------------------------------ C ABI
def _header():
    return open(os.path.join(ROOT, "include", "olympic_hip.h")).read()


def test_header_declares_the_k16_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in ("oly_ilmlp_packed_floats", "oly_ilmlp_pack", "oly_ilmlp_forward", "oly_il_critic_fit_ws_floats",
                 "oly_il_critic_fit_epoch"):
        assert re.search(rf"\b{name}\s*\(", txt), name
        assert name in _abi.SIGNATURES, name
    assert int(re.search(r"#define OLY_ABI_VERSION (\d+)", txt).group(1)) == _abi.ABI_VERSION == 8
    assert int(re.search(r"#define OLY_ACT_TANH (\d+)", txt).group(1)) == _abi.ACT_TANH
    assert int(re.search(r"#define OLY_ACT_IDENTITY (\d+)", txt).group(1)) == _abi.ACT_IDENTITY


def test_fit_struct_layout_matches_the_header(tmp_path):
    cls = _abi.ILCriticFit
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/olympic_hip.h"', "int main(){",
             'printf("size %zu\\n", sizeof(oly_il_critic_fit));']
    lines += [f'printf("{f} %zu\\n", offsetof(oly_il_critic_fit, {f}));' for f, _ in cls._fields_]
    lines.append("return 0;}")
    src, exe = tmp_path / "t.c", tmp_path / "t"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["size"]) == ctypes.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(out[f]) == getattr(cls, f).offset, f


def test_library_sizes_and_refusals():
    from olympic_hip import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        pytest.fail(f"{_ffi.LIB_PATH} missing: run python __graft_entry__.py build")
    L = _ffi.lib()
    n = int(L.oly_ilmlp_packed_floats(32, 512, 256, 1))
    assert n > 512 * 64 + 512 * 256 and n % 4 == 0
    assert n == int(L.oly_ilmlp_packed_floats(64, 512, 256, 32))
    for shape in ((65, 512, 256, 1), (0, 512, 256, 1), (32, 256, 256, 1), (32, 512, 512, 1), (32, 512, 256, 33),
                  (32, 512, 256, 0)):
        assert int(L.oly_ilmlp_packed_floats(*shape)) == -1, shape
    assert int(L.oly_il_critic_fit_ws_floats(256, 32)) > 0
    for bad in ((257, 32), (0, 32), (256, 65), (256, 0)):
        assert int(L.oly_il_critic_fit_ws_floats(*bad)) == -1, bad
