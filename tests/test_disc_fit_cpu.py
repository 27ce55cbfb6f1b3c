"""K15 without a GPU: the reference-pinned discriminator-fit fixture, a float64 restatement of _fit_discriminator's
epochs for VAIL, and the C ABI entries of oly_disc_fit_*."""
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
FIXTURE = os.path.join(GOLDEN, "vail_disc_fit", "vail_disc_fit.npz")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import gen_vail_disc_fit as gen  # noqa: E402  (init_params / noise: the parts of the fixture rebuilt from seeds)


def case_inputs(g, case):
    """Per epoch the concatenated masked rows [policy; demonstrations], the permutation, the targets (None: 0 / 1)
    and the noise, as the fixture's run drew them."""
    mask = g["state_mask"]
    plcy = g["plcy_obs"][:, mask]
    eps = gen.noise(case)
    out = []
    for e in range(g[f"{case}_perms"].shape[0]):
        demo = g["demo_states"][g[f"{case}_demo_idx"][e]][:, mask].astype(np.float32)
        t = g[f"{case}_targets"][e] if f"{case}_targets" in g.files else None
        out.append((np.concatenate([plcy, demo]), g[f"{case}_perms"][e], t, eps[e]))
    return out


def hyper(g, case):
    info_c, lr_beta, _, wd = (float(v) for v in g[f"{case}_hyper"])
    return dict(info_c=info_c, lr_beta=lr_beta, wd=wd, lr=float(g["lr"]), batch=int(g["batch"]))


def restate_fit(epochs, n_plcy, params, colstats, info_c, lr_beta, lr, batch, wd=0.0, beta=0.1, step0=0, moments=None,
                dtype=torch.float64, device="cpu", betas=(0.9, 0.999), eps=1e-8):
    """_fit_discriminator's epochs in torch.  epochs: [(x [n,in] f32 masked concatenated rows, perm, targets or None,
    noise [n,128])].  Per epoch the explicit update_mean_std(x) (gail_TRPO.py:206), then per minibatch the
    Standardizer update and f32((f64(x) - mean) / std) (networks.py:68-81), the forward (relu, relu; z = mu +
    exp(logvar / 2) eps), VDBLoss (BCEWithLogits mean + beta (mean KL - I_c)), beta <- max(0, beta + lr_beta
    bottleneck) and torch's Adam step with L2 weight decay.
    Returns (params, moments, colstats, dict(loss, bce, kl, beta), step)."""
    P = [torch.as_tensor(np.asarray(p), device=device).to(dtype).clone() for p in params]
    M = [torch.zeros_like(p) for p in P] if moments is None else [m.clone() for m in moments[0]]
    V = [torch.zeros_like(p) for p in P] if moments is None else [v.clone() for v in moments[1]]
    cs = torch.as_tensor(np.asarray(colstats), device=device).to(torch.float64).clone()
    rec = {k: [] for k in ("loss", "bce", "kl", "beta")}
    step = step0
    def dev(a):
        return (a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))).to(device)
    for x, perm, targets, noise in epochs:
        x = dev(x)
        n = x.shape[0]
        t_all = (dev(targets) if targets is not None else
                 (torch.arange(n, device=device) >= n_plcy).to(torch.float32)).to(dtype)
        noise = dev(noise).to(dtype)
        perm = torch.as_tensor(np.asarray(perm, dtype=np.int64), device=device)
        xd = x.to(torch.float64)
        cs[0] += n
        cs[1] += xd.sum(0)
        cs[2] += (xd * xd).sum(0)
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
            mu, lv = h2 @ P[4].T + P[5], h2 @ P[6].T + P[7]
            z = mu + torch.exp(lv / 2) * noise[b * batch:b * batch + idx.shape[0]]
            d = (z @ P[8].T + P[9]).reshape(-1)
            bce = torch.nn.functional.binary_cross_entropy_with_logits(d, t_all[idx])
            kl = (0.5 * torch.sum(mu * mu + torch.exp(lv) - lv - 1, dim=1)).mean()
            bottleneck = kl - info_c
            loss = bce + beta * bottleneck
            grads = torch.autograd.grad(loss, P)
            rec["loss"].append(float(loss.detach()))
            rec["bce"].append(float(bce.detach()))
            rec["kl"].append(float(kl.detach()))
            beta = max(0.0, beta + lr_beta * float(bottleneck.detach()))
            rec["beta"].append(beta)
            step += 1
            bc1, bc2 = 1 - betas[0] ** step, 1 - betas[1] ** step
            with torch.no_grad():
                for i in range(len(P)):
                    p, gr = P[i].detach(), grads[i]
                    if wd:
                        gr = gr + wd * p
                    M[i] = M[i] + (gr - M[i]) * (1 - betas[0])
                    V[i] = V[i] * betas[1] + (1 - betas[1]) * gr * gr
                    P[i] = p - (lr / bc1) * (M[i] / (torch.sqrt(V[i]) / bc2 ** 0.5 + eps))
    return [p.detach() for p in P], (M, V), cs, {k: np.array(v) for k, v in rec.items()}, step


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def check_statistics(cs, g, case):
    """The fp64 running (count, sum, sumsq) against the reference Standardizer's own sums (float32 in numpy)."""
    cs = np.asarray(cs)
    np.testing.assert_allclose(cs[0] + 1e-2, np.full(cs.shape[1], g[f"{case}_st_count"][0]), rtol=0, atol=1e-9)
    np.testing.assert_allclose(cs[1], g[f"{case}_st_sum"], rtol=1e-5, atol=1e-2)
    np.testing.assert_allclose(cs[2] + 1e-2, g[f"{case}_st_sumsq"], rtol=1e-5)


def _reference_dir():
    import _ref_stubs
    return _ref_stubs.REF


@pytest.mark.skipif(not os.path.isdir(_reference_dir()), reason="the reference tree is only in the build container")
def test_fixture_regenerates_byte_for_byte(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "gen_vail_disc_fit.py"), "--out", str(tmp_path)],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONHASHSEED="random"))
    assert r.returncode == 0, r.stderr[-2000:]
    a, b = np.load(FIXTURE), np.load(str(tmp_path / "vail_disc_fit.npz"))
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert a[k].tobytes() == b[k].tobytes(), f"{k} does not regenerate"


def test_fixture_shape():
    g = np.load(FIXTURE)
    assert g["plcy_obs"].shape == (640, 34) and g["demo_states"].shape == (1000, 34) and g["state_mask"].shape == (32,)
    for case in "ab":
        assert g[f"{case}_perms"].shape == (2, 1280) and all(sorted(p) == list(range(1280)) for p in g[f"{case}_perms"])
        assert g[f"{case}_demo_idx"].shape == (2, 640) and all(len(set(d)) == 640 for d in g[f"{case}_demo_idx"])
        for k in ("loss", "bce", "kl", "beta"):
            assert g[f"{case}_{k}"].shape == (6,), k      # 3 minibatches (512, 512, 256) per epoch
    assert g["b_targets"].shape == (2, 1280) and "a_targets" not in g.files
    assert g["a_beta"][-1] > g["a_beta"][0] > 0.1 and 0.0 in g["b_beta"] and g["b_beta"][0] > 0
    assert os.path.getsize(FIXTURE) < 1 << 20


@pytest.mark.parametrize("case", ["a", "b"])
def test_float64_restatement_reproduces_the_reference_fit(case):
    g = np.load(FIXTURE)
    h = hyper(g, case)
    P, _, cs, rec, step = restate_fit(case_inputs(g, case), 640, gen.init_params(), np.zeros((3, 32)), h["info_c"],
                                      h["lr_beta"], h["lr"], h["batch"], wd=h["wd"])
    assert step == 6
    for i, name in enumerate(gen.NAMES):
        assert rel(P[i].numpy(), g[f"{case}_final_{name}"]) <= 1e-6, name
        # and the fit moved every tensor far beyond that tolerance
        assert rel(gen.init_params()[i], g[f"{case}_final_{name}"]) > 1e-4, name
    for k in ("loss", "bce", "kl", "beta"):
        np.testing.assert_allclose(rec[k], g[f"{case}_{k}"], rtol=2e-6, atol=2e-6, err_msg=k)
    check_statistics(cs.numpy(), g, case)


# ------------------------------------------------------------------------------ C ABI
def _header():
    return open(os.path.join(ROOT, "include", "olympic_hip.h")).read()


def test_header_declares_the_k15_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in ("oly_disc_fit_ws_floats", "oly_disc_fit_epoch"):
        assert re.search(rf"\b{name}\s*\(", txt), name
        assert name in _abi.SIGNATURES, name
    assert int(re.search(r"#define OLY_ABI_VERSION (\d+)", txt).group(1)) == _abi.ABI_VERSION == 8


def test_fit_struct_layout_matches_the_header(tmp_path):
    cls = _abi.DiscFit
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/olympic_hip.h"', "int main(){",
             'printf("size %zu\\n", sizeof(oly_disc_fit));']
    lines += [f'printf("{f} %zu\\n", offsetof(oly_disc_fit, {f}));' for f, _ in cls._fields_]
    lines.append("return 0;}")
    src, exe = tmp_path / "t.c", tmp_path / "t"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["size"]) == ctypes.sizeof(cls)
    assert len(out) == len(cls._fields_) + 1
    for f, _ in cls._fields_:
        assert int(out[f]) == getattr(cls, f).offset, f


def test_workspace_sizes_and_refusals():
    from olympic_hip import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        pytest.fail(f"{_ffi.LIB_PATH} missing: run python __graft_entry__.py build")
    L = _ffi.lib()
    small, big = int(L.oly_disc_fit_ws_floats(1, 32)), int(L.oly_disc_fit_ws_floats(4096, 64))
    assert 0 < small < big and big == int(L.oly_disc_fit_ws_floats(4096, 1))
    assert int(L.oly_disc_fit_ws_floats(2048, 32)) > 2048 * 1200      # about 5 KB of activations and deltas per row
    for bad in ((4097, 32), (0, 32), (-1, 32), (2048, 65), (2048, 0)):
        assert int(L.oly_disc_fit_ws_floats(*bad)) == -1, bad
