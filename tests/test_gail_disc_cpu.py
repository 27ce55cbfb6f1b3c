"""K18 without a GPU: the reference-pinned fixtures of GAIL's discriminator fit, a float64 restatement of
_fit_discriminator's epochs for GAIL, and the C ABI entries of oly_gail_*."""
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
FIXTURE_DIR = os.path.join(GOLDEN, "gail_disc_fit")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import gen_gail_disc_fit as gen  # noqa: E402  (inputs / init_params: the parts of the fixture rebuilt from seeds)

TOL = 2e-5            # the device tolerance per tensor (tests/il_shapes.py)
K18_ENTRIES = ("oly_gail_disc_forward", "oly_gail_reward_step", "oly_gail_disc_fit_ws_floats", "oly_gail_disc_fit_epoch")


def fixture(case):
    return os.path.join(FIXTURE_DIR, f"gail_disc_fit_{case}.npz")


def case_inputs(g):
    """Per epoch the concatenated masked rows [policy; demonstrations], the permutation and the targets (None: 0 / 1),
    as the fixture's run drew them."""
    mask = g["state_mask"]
    plcy_obs, demo_states = gen.inputs()
    plcy = plcy_obs[:, mask]
    out = []
    for e in range(g["perms"].shape[0]):
        demo = demo_states[g["demo_idx"][e]][:, mask].astype(np.float32)
        t = g["targets"][e] if "targets" in g.files else None
        out.append((np.concatenate([plcy, demo]), g["perms"][e], t))
    return out


def hyper(g):
    entcoeff, _, wd = (float(v) for v in g["hyper"])
    return dict(entcoeff=entcoeff, wd=wd, lr=float(g["lr"]), batch=int(g["batch"]))


def gail_loss(d, t, entcoeff):
    """GailDiscriminatorLoss.forward (imitation_lib/utils/math.py:22-36) -> (loss, bce, ent)."""
    bce = torch.mean(torch.clamp(d, min=0) - d * t + torch.log1p(torch.exp(-torch.abs(d))))
    ent = torch.mean((1.0 - torch.sigmoid(d)) * d - torch.nn.functional.logsigmoid(d))
    return bce - entcoeff * ent, bce, ent


def forward(P, xs):
    h1 = torch.tanh(xs @ P[0].T + P[1])
    h2 = torch.tanh(h1 @ P[2].T + P[3])
    return (h2 @ P[4].T + P[5]).reshape(-1)


def restate_fit(epochs, n_plcy, params, colstats, entcoeff, lr, batch, wd=0.0, step0=0, moments=None,
                dtype=torch.float64, device="cpu", betas=(0.9, 0.999), eps=1e-8):
    """_fit_discriminator's epochs for GAIL in torch.  epochs: [(x [n,in] f32 masked concatenated rows, perm, targets or
    None)].  Per epoch the explicit update_mean_std(x) (gail_TRPO.py:206), then per minibatch the Standardizer update
    and f32((f64(x) - mean) / std) (networks.py:68-81), the forward (tanh, tanh, identity), GailDiscriminatorLoss and
    torch's Adam step with L2 weight decay.  Returns (params, moments, colstats, dict(loss, bce, ent), step)."""
    P = [torch.as_tensor(np.asarray(p), device=device).to(dtype).clone() for p in params]
    M = [torch.zeros_like(p) for p in P] if moments is None else [m.clone() for m in moments[0]]
    V = [torch.zeros_like(p) for p in P] if moments is None else [v.clone() for v in moments[1]]
    cs = torch.as_tensor(np.asarray(colstats), device=device).to(torch.float64).clone()
    rec = {k: [] for k in ("loss", "bce", "ent")}
    step = step0

    def dev(a):
        return (a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))).to(device)
    for x, perm, targets in epochs:
        x = dev(x)
        n = x.shape[0]
        t_all = (dev(targets) if targets is not None else
                 (torch.arange(n, device=device) >= n_plcy).to(torch.float32)).to(dtype)
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
            loss, bce, ent = gail_loss(forward(P, xs), t_all[idx], entcoeff)
            grads = torch.autograd.grad(loss, P)
            for k, v in (("loss", loss), ("bce", bce), ("ent", ent)):
                rec[k].append(float(v.detach()))
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


def check_statistics(cs, g):
    """The fp64 running (count, sum, sumsq) against the reference Standardizer's own sums (float32 in numpy), with
    test_disc_fit_cpu.check_statistics' bounds."""
    cs = np.asarray(cs)
    np.testing.assert_allclose(cs[0] + 1e-2, np.full(cs.shape[1], g["st_count"][0]), rtol=0, atol=1e-9)
    np.testing.assert_allclose(cs[1], g["st_sum"], rtol=1e-5, atol=1e-2)
    np.testing.assert_allclose(cs[2] + 1e-2, g["st_sumsq"], rtol=1e-5)


def _reference_dir():
    import _ref_stubs
    return _ref_stubs.REF


@pytest.mark.skipif(not os.path.isdir(_reference_dir()), reason="the reference tree is only in the build container")
def test_fixture_regenerates_byte_for_byte(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "gen_gail_disc_fit.py"), "--out", str(tmp_path)],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONHASHSEED="random"))
    assert r.returncode == 0, r.stderr[-2000:]
    for case in "ab":
        a, b = np.load(fixture(case)), np.load(str(tmp_path / f"gail_disc_fit_{case}.npz"))
        assert sorted(a.files) == sorted(b.files)
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
            assert a[k].tobytes() == b[k].tobytes(), f"{case}: {k} does not regenerate"


def test_fixture_shape():
    plcy_obs, demo_states = gen.inputs()
    assert plcy_obs.shape == (640, 34) and demo_states.shape == (1000, 34)
    for case in "ab":
        g = np.load(fixture(case))
        assert g["state_mask"].shape == (32,) and 3 not in g["state_mask"] and 17 not in g["state_mask"]
        assert g["perms"].shape == (2, 1280) and all(sorted(p) == list(range(1280)) for p in g["perms"])
        assert g["demo_idx"].shape == (2, 640) and all(len(set(d)) == 640 for d in g["demo_idx"])
        for k in ("loss", "bce", "ent"):
            assert g[k].shape == (6,), k      # 3 minibatches (512, 512, 256) per epoch
        for name, shape in zip(gen.NAMES, gen.SHAPES):
            assert g[f"final_{name}"].shape == shape and g[f"final_{name}"].dtype == np.float32
        assert float(g["lr"]) == 5e-5 and int(g["batch"]) == 512
        assert os.path.getsize(fixture(case)) < 1 << 20
    assert "targets" not in np.load(fixture("a")).files and np.load(fixture("b"))["targets"].shape == (2, 1280)
    assert tuple(np.load(fixture("a"))["hyper"]) == (1e-3, 0.0, 0.0)
    assert tuple(np.load(fixture("b"))["hyper"]) == (0.05, 1.0, 1e-3)


@pytest.mark.parametrize("case", ["a", "b"])
def test_the_fit_moves_every_tensor_far_beyond_the_tolerance(case):
    g = np.load(fixture(case))
    for p0, name in zip(gen.init_params(), gen.NAMES):
        move = rel(p0, g[f"final_{name}"])
        print(f"{case} {name}: moved {move:.3e}")
        assert move > 50 * TOL, (name, move)


@pytest.mark.parametrize("case", ["a", "b"])
def test_float64_restatement_reproduces_the_reference_fit(case):
    g = np.load(fixture(case))
    h = hyper(g)
    P, _, cs, rec, step = restate_fit(case_inputs(g), 640, gen.init_params(), np.zeros((3, 32)), h["entcoeff"], h["lr"],
                                      h["batch"], wd=h["wd"])
    assert step == 6
    for i, name in enumerate(gen.NAMES):
        r = rel(P[i].numpy(), g[f"final_{name}"])
        print(f"{case} {name}: rel {r:.3e}")
        assert r <= 1e-6, name
    for k in ("loss", "bce", "ent"):
        np.testing.assert_allclose(rec[k], g[k], rtol=2e-6, atol=2e-6, err_msg=k)
    check_statistics(cs.numpy(), g)


def test_default_initialisation_is_the_reference_rule():
    """GAILDiscriminator draws xavier_uniform_ with tanh's gain (output layer: gain 1), as networks.py:133-139 does."""
    from olympic_hip.gail import GAILDiscriminator
    torch.manual_seed(0)
    net = GAILDiscriminator(32)
    assert [tuple(l.weight.shape) for l in net._linears] == [(512, 32), (256, 512), (1, 256)]
    for lin, gain in zip(net._linears, (5.0 / 3.0, 5.0 / 3.0, 1.0)):
        a = gain * np.sqrt(6.0 / (lin.in_features + lin.out_features))
        w = lin.weight.detach().numpy()
        assert np.abs(w).max() <= a and np.abs(w).max() > 0.9 * a
    xs = torch.randn(5, 32)
    h = torch.tanh(torch.tanh(xs @ net._linears[0].weight.T + net._linears[0].bias) @ net._linears[1].weight.T
                   + net._linears[1].bias)
    assert torch.allclose(net(xs), h @ net._linears[2].weight.T + net._linears[2].bias)


# ------------------------------------------------------------------------------ C ABI
def _header():
    return open(os.path.join(ROOT, "include", "olympic_hip.h")).read()


def test_header_declares_the_k18_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in K18_ENTRIES:
        assert re.search(rf"\b{name}\s*\(", txt), name
        assert name in _abi.SIGNATURES, name
    assert int(re.search(r"#define OLY_ABI_VERSION (\d+)", txt).group(1)) == _abi.ABI_VERSION


def test_fit_struct_layout_matches_the_header(tmp_path):
    cls = _abi.GailDiscFit
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/olympic_hip.h"', "int main(){",
             'printf("size %zu\\n", sizeof(oly_gail_disc_fit));']
    lines += [f'printf("{f} %zu\\n", offsetof(oly_gail_disc_fit, {f}));' for f, _ in cls._fields_]
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
    small, big = int(L.oly_gail_disc_fit_ws_floats(1, 32)), int(L.oly_gail_disc_fit_ws_floats(4096, 64))
    assert 0 < small < big and big == int(L.oly_gail_disc_fit_ws_floats(4096, 1))
    # per row: 64 + 512 + 256 activations, 512 + 256 + 1 deltas; plus the transposed W2
    assert int(L.oly_gail_disc_fit_ws_floats(2048, 32)) >= 2048 * 1601 + 256 * 512
    assert small >= 16 * 1601 + 256 * 512
    for bad in ((4097, 32), (0, 32), (-1, 32), (2048, 65), (2048, 0)):
        assert int(L.oly_gail_disc_fit_ws_floats(*bad)) == -1, bad
    # a NULL context is refused before anything is read
    assert L.oly_gail_disc_fit_epoch(None, None, None, 0, 1, None) == _abi.OLY_EINVAL
    assert L.oly_gail_disc_forward(None, 0, 1, 1, None, None, None, None, None, None, None, None, None) == _abi.OLY_EINVAL
    assert L.oly_gail_reward_step(None, 0, 1, 1, None, None, None, 0, None, None, None, None, None) == _abi.OLY_EINVAL
