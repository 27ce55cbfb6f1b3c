"""The shape tables of tests/il_shapes.py and their float64 yardsticks, without a GPU: the restatements against an
independent float64 run through torch.optim.Adam and autograd at shapes other than 32 columns, and for every case of
the tables that float32 arithmetic can meet the GPU tests' tolerance with a factor of ten to spare, that the fit moves
every tensor ten times farther than that tolerance, and that the TRPO step's branches do not hang on rounding."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import il_shapes as sh
import trpo_restate as tr
from il_shapes import K15_CASES, K16_CASES, K17_CASES, TOL, case_id
from test_disc_fit_cpu import rel

K17_STEP_CASES = [c for c in K17_CASES if c.n >= sh.K17_STEP_MIN_ROWS]


# the shapes themselves, seed and learning rate left free: a case that turns out to sit on a threshold is given another
# seed or learning rate, never dropped
SHAPES = dict(
    K15_CASES={(1, 7, 20, 10, False, 0.0), (17, 3, 10, 5, False, 0.0), (17, 256, 257, 128, False, 0.0),
               (33, 4096, 4097, 2048, False, 0.0), (33, 64, 199, 99, True, 0.0), (45, 100, 250, 125, False, 0.0),
               (45, 512, 300, 300, False, 0.0), (64, 255, 513, 200, True, 1e-3), (64, 333, 1022, 0, False, 0.0)},
    K16_CASES={(1, 7, 20), (17, 256, 257), (33, 100, 250), (33, 100, 37), (45, 255, 511), (45, 255, 320), (64, 256, 385),
               (64, 1, 5)},
    K17_CASES={(1, 1, 65), (1, 32, 63), (17, 1, 1), (17, 12, 257), (32, 11, 1), (45, 11, 63), (45, 12, 16684),
               (64, 32, 257), (64, 32, 16385), (64, 12, 65)})
WIDTH = dict(K15_CASES=6, K16_CASES=3, K17_CASES=3)


def check_tables():
    sh.required_shapes_present()
    for table, shapes in SHAPES.items():
        missing = shapes - {tuple(c[:WIDTH[table]]) for c in getattr(sh, table)}
        assert not missing, (table, missing)


def test_tables_hold_the_required_shapes():
    check_tables()
    assert len(K17_STEP_CASES) >= 7


@pytest.mark.parametrize("table", sorted(SHAPES))
def test_a_table_without_one_of_its_cases_is_noticed(monkeypatch, table):
    full = getattr(sh, table)
    for i in range(len(full)):
        monkeypatch.setattr(sh, table, full[:i] + full[i + 1:])
        with pytest.raises(AssertionError):
            check_tables()
    monkeypatch.setattr(sh, table, full)
    check_tables()


# ------------------------------------------------------------------------------ the yardstick against torch's own Adam
class _Running:
    """The Standardizer's sums (networks.py:76-81) in numpy float64."""

    def __init__(self, cs):
        self.cnt, self.s, self.ss = float(cs[0][0]), np.array(cs[1], dtype=np.float64), np.array(cs[2], dtype=np.float64)

    def add(self, x):
        self.cnt += x.shape[0]
        self.s = self.s + x.sum(0)
        self.ss = self.ss + (x * x).sum(0)

    def standardise(self, x):
        cnt = self.cnt + 1e-2
        mean = self.s / cnt
        sd = np.sqrt(np.maximum((self.ss + 1e-2) / cnt - mean * mean, 1e-2))
        return torch.from_numpy(((x - mean) / sd).astype(np.float32).astype(np.float64))


def adam_disc_fit(c):
    """The discriminator's epochs with nn.Parameters, autograd's backward and torch.optim.Adam, float64."""
    params, epochs, h = sh.disc_case(c)
    P = [torch.nn.Parameter(torch.from_numpy(p).double()) for p in params]
    opt = torch.optim.Adam(P, lr=h["lr"], weight_decay=h["wd"])
    st = _Running(np.zeros((3, c.in_dim)))
    beta, rec = 0.1, {k: [] for k in ("loss", "bce", "kl", "beta")}
    for x, perm, t, noise in epochs:
        xd = x.astype(np.float64)
        st.add(xd)
        t_all = torch.from_numpy(t if t is not None else (np.arange(c.n_rows) >= c.n_plcy).astype(np.float32)).double()
        for lo in range(0, c.n_rows, c.batch):
            idx = perm[lo:lo + c.batch]
            st.add(xd[idx])
            xs = st.standardise(xd[idx])
            h2 = F.relu(F.linear(F.relu(F.linear(xs, P[0], P[1])), P[2], P[3]))
            mu, lv = F.linear(h2, P[4], P[5]), F.linear(h2, P[6], P[7])
            z = mu + torch.exp(0.5 * lv) * torch.from_numpy(noise[lo:lo + len(idx)]).double()
            bce = F.binary_cross_entropy_with_logits(F.linear(z, P[8], P[9]).squeeze(1), t_all[torch.from_numpy(idx)])
            kl = (0.5 * (mu.pow(2) + lv.exp() - lv - 1).sum(1)).mean()
            loss = bce + beta * (kl - h["info_c"])
            opt.zero_grad()
            loss.backward()
            opt.step()
            beta = max(0.0, beta + h["lr_beta"] * (float(kl.detach()) - h["info_c"]))
            for k, v in (("loss", loss), ("bce", bce), ("kl", kl), ("beta", beta)):
                rec[k].append(float(v.detach()) if torch.is_tensor(v) else float(v))
    return [p.detach() for p in P], {k: np.array(v) for k, v in rec.items()}, np.stack([np.full(c.in_dim, st.cnt), st.s, st.ss])


def adam_critic_fit(c):
    params, x, vt, perms, cs = sh.critic_case(c)
    P = [torch.nn.Parameter(torch.from_numpy(p).double()) for p in params]
    opt = torch.optim.Adam(P, lr=c.lr)
    st, xd, losses = _Running(cs), x.astype(np.float64), []
    target = torch.from_numpy(vt).double().reshape(-1, 1)
    for perm in perms:
        for lo in range(0, c.n, c.batch):
            idx = perm[lo:lo + c.batch]
            st.add(xd[idx])
            xs = st.standardise(xd[idx])
            y = F.linear(F.relu(F.linear(F.relu(F.linear(xs, P[0], P[1])), P[2], P[3])), P[4], P[5])
            loss = F.mse_loss(y, target[torch.from_numpy(idx)])
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
    return [p.detach() for p in P], np.array(losses), np.stack([np.full(c.in_dim, st.cnt), st.s, st.ss])


# both sides are float64 and differ only in the order of operations (measured: at most 3e-17)
SAME = 1e-12


@pytest.mark.parametrize("c", [K15_CASES[0], K15_CASES[5], K15_CASES[7]], ids=case_id)
def test_disc_restatement_against_torch_adam(c):
    assert c.in_dim != 32
    P, _, cs, rec, step = sh.disc_restate(c)
    Q, rec_q, cs_q = adam_disc_fit(c)
    assert step == len(rec_q["loss"]) == sh.K15_EPOCHS * math.ceil(c.n_rows / c.batch)
    for i, (a, b) in enumerate(zip(P, Q)):
        assert rel(a.numpy(), b.numpy()) <= SAME, i
    for k in rec:
        np.testing.assert_allclose(rec[k], rec_q[k], rtol=SAME, atol=SAME, err_msg=k)
    np.testing.assert_allclose(cs.numpy(), cs_q, rtol=SAME)


@pytest.mark.parametrize("c", [K16_CASES[0], K16_CASES[4], K16_CASES[6]], ids=case_id)
def test_critic_restatement_against_torch_adam(c):
    assert c.in_dim != 32
    P, _, cs, losses, step = sh.critic_restate(c)
    Q, losses_q, cs_q = adam_critic_fit(c)
    assert step == len(losses_q) == sh.K16_EPOCHS * math.ceil(c.n / c.batch)
    for i, (a, b) in enumerate(zip(P, Q)):
        assert rel(a.numpy(), b.numpy()) <= SAME, i
    np.testing.assert_allclose(losses, losses_q, rtol=SAME)
    np.testing.assert_allclose(cs.numpy(), cs_q, rtol=SAME)


# ------------------------------------------------------------------------------ every case of the tables
@pytest.mark.parametrize("c", K15_CASES, ids=case_id)
def test_disc_case_is_attainable_and_moves(c):
    params = sh.disc_case(c)[0]
    P, (M, V), _, rec, step = sh.disc_restate(c)
    P32, _, _, rec32, _ = sh.disc_restate(c, dtype=torch.float32)
    for i, (p0, a, b) in enumerate(zip(params, P, P32)):
        r32, moved = rel(b.numpy(), a.numpy()), rel(p0, a.numpy())
        print(f"{case_id(c)} tensor {i}: float32 {r32:.2e} from float64, moved {moved:.2e}")
        assert r32 <= TOL / 10, i
        assert moved >= 10 * TOL, i
    for k in rec:
        np.testing.assert_allclose(rec32[k], rec[k], rtol=TOL / 10, atol=TOL / 10, err_msg=k)
    assert np.isfinite(rec["loss"]).all()
    # the second epoch starts from moments, a beta and a step count that the first one left
    first = step // 2
    assert first >= 1 and abs(rec["beta"][first - 1] - 0.1) >= 10 * TOL
    assert all(float(m.abs().max()) > 0 for m in M) and all(float(v.abs().max()) > 0 for v in V)


@pytest.mark.parametrize("c", K16_CASES, ids=case_id)
def test_critic_case_is_attainable_and_moves(c):
    params = sh.critic_case(c)[0]
    P, _, _, losses, _ = sh.critic_restate(c)
    P32, _, _, losses32, _ = sh.critic_restate(c, dtype=torch.float32)
    for i, (p0, a, b) in enumerate(zip(params, P, P32)):
        r32, moved = rel(b.numpy(), a.numpy()), rel(p0, a.numpy())
        print(f"{case_id(c)} tensor {i}: float32 {r32:.2e} from float64, moved {moved:.2e}")
        assert r32 <= TOL / 10, i
        assert moved >= 10 * TOL, i
    np.testing.assert_allclose(losses32, losses, rtol=TOL / 10)
    assert np.isfinite(losses).all() and (losses > 0).all()


@pytest.mark.parametrize("c", K17_CASES, ids=case_id)
def test_trpo_grad_and_fvp_case_is_attainable(c):
    case = sh.trpo_case(c)
    assert float(case["adv"].abs().max()) > 0
    for k in (1, 4):
        J, g, prod, _ = sh.trpo_grad_fvp_reference(c, case, k)
        J32, g32, prod32, _ = sh.trpo_grad_fvp_reference(c, case, k, dtype=torch.float32)
        eg, ep = rel(g32.numpy(), g.numpy()), rel(prod32.numpy(), prod.numpy())
        print(f"{case_id(c)} k={k}: float32 g {eg:.2e}, product {ep:.2e}, J {abs(float(J32) - float(J)):.2e}")
        assert eg <= TOL / 10 and ep <= TOL / 10
        assert abs(float(J32) - float(J)) <= TOL / 10 * max(1.0, abs(float(J)))
        # every tensor of the gradient and of the product is there to be got wrong
        for name, v in (("g", g), ("product", prod)):
            for i, t in enumerate(tr.split(v, c.D, c.A)):
                assert float(t.abs().max()) > 0, (name, i)


@pytest.mark.parametrize("c", K17_STEP_CASES, ids=case_id)
def test_trpo_step_case_is_decided_away_from_its_thresholds(c):
    case = sh.trpo_case(c)
    kw = sh.K17_STEP
    r64 = tr.trpo_step(case["theta"], case["S"], case["x"], case["act"], case["adv"], **kw)
    r32 = tr.trpo_step(case["theta"], case["S"], case["x"], case["act"], case["adv"], dtype=torch.float32, **kw)
    for k in ("j", "j_run", "k_run"):
        assert r64[k] == r32[k], k
    assert r64["j"] >= 0, "the step is accepted, so theta moves"
    gain = r64["J"] - r64["prev_loss"]
    print(f"{case_id(c)}: j {r64['j']} k_run {r64['k_run']} kl {r64['kl']:.4e} (1.5 max_kl {1.5 * kw['max_kl']:.4e}) "
          f"gain {gain:.4e} (J {r64['J']:.4e}); float32 stepdir {rel(r32['stepdir'].numpy(), r64['stepdir'].numpy()):.2e}")
    # neither acceptance test of the accepted candidate sits within 2 % of its threshold
    assert abs(r64["kl"] - 1.5 * kw["max_kl"]) >= 0.02 * 1.5 * kw["max_kl"]
    assert abs(gain) >= 0.02 * max(abs(r64["J"]), abs(r64["prev_loss"]))
    d = (r64["theta"] - case["theta"].double())
    assert rel(r64["theta"].numpy(), case["theta"].double().numpy()) >= 10 * TOL
    for i, t in enumerate(tr.split(d, c.D, c.A)):
        assert float(t.abs().max()) > 0, i


def test_workspace_sizes_for_every_case():
    from olympic_hip import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        pytest.fail(f"{_ffi.LIB_PATH} missing: run python __graft_entry__.py build")
    L = _ffi.lib()
    for c in K15_CASES:
        assert int(L.oly_disc_fit_ws_floats(c.batch, c.in_dim)) > 0, c
    for c in K16_CASES:
        assert int(L.oly_il_critic_fit_ws_floats(c.batch, c.in_dim)) > 0, c
    for c in K17_CASES:
        assert int(L.oly_trpo_ws_floats(c.n, c.D, 512, 256, c.A)) > 0, c
        assert int(L.oly_trpo_param_count(c.D, 512, 256, c.A)) == tr.n_params(c.D, c.A), c
