"""A2C without a GPU: the float64 references of tests/helpers/a2c_ref.py against torch
autograd and torch.optim.RMSprop, planted errors against the comparisons the GPU tests
use, the C ABI additions, and the host side of A2C_ACKTR and its checkpoints."""
import os
import re

import numpy as np
import pytest
import torch

from a2c_ppo_acktr import checkpoint as CK
from a2c_ppo_acktr import model as M
from a2c_ppo_acktr.algo import A2C_ACKTR, PPO
from a2c_ppo_acktr.synthetic import Discrete
from conftest import ROOT
from helpers import a2c_ref as R
from helpers import mlp_rec_ref

HEADER = os.path.join(ROOT, "include", "ppo_hip.h")
NEW = ("ppo_heads_train_a2c", "ppo_heads_gauss_train_a2c", "ppo_heads_bern_train_a2c", "ppo_clip_rmsprop_guarded")


# ------------------------------------------------------------------ references
@pytest.mark.parametrize("A", [1, 16])
@pytest.mark.parametrize("kind", R.KINDS)
def test_closed_forms_equal_float64_autograd(kind, A):
    """head_grads' g_value, g_logits, g_logstd and the three losses equal float64
    autograd of the restated loss (torch_loss) to 1e-10."""
    g = np.random.default_rng(100 * A + R.KINDS.index(kind))
    B = 23
    value, z, ret = g.normal(size=B), g.normal(size=(B, A)) * 2, g.normal(size=B)
    logstd = g.normal(size=A) * 0.3 if kind == "gauss" else None
    actions = (g.integers(0, A, B) if kind == "cat" else z + g.normal(size=(B, A)) if kind == "gauss"
               else g.integers(0, 2, (B, A)).astype(np.float64))
    r = R.head_grads(kind, value, z, actions, ret, 0.5, 0.01, logstd)
    t = lambda x: torch.from_numpy(np.asarray(x))  # noqa: E731
    tv, tz = t(value).requires_grad_(), t(z).requires_grad_()
    tl = t(logstd).requires_grad_() if kind == "gauss" else None
    total, vl, al, ent = R.torch_loss(kind, tv, tz, t(actions), t(ret), 0.5, 0.01, tl)
    total.backward()
    assert np.abs(tv.grad.numpy() - r["g_value"]).max() <= 1e-10
    assert np.abs(tz.grad.numpy() - r["g_logits"]).max() <= 1e-10
    if kind == "gauss":
        assert np.abs(tl.grad.numpy() - r["g_logstd"]).max() <= 1e-10
    else:
        assert r["g_logstd"] is None
    np.testing.assert_allclose([vl.item(), al.item(), ent.item()], [r["value_loss"], r["action_loss"], r["entropy"]],
                               rtol=0, atol=1e-10)


def test_rmsprop_step_equals_torch_float64():
    """three steps of rmsprop_step against torch.optim.RMSprop on float64 tensors, 1e-12"""
    g = np.random.default_rng(5)
    n, lr, alpha, eps = 1003, 7e-4, 0.99, 1e-5
    p = torch.from_numpy(g.normal(size=n)).requires_grad_()
    opt = torch.optim.RMSprop([p], lr, eps=eps, alpha=alpha, foreach=False)
    mine, sq = p.detach().numpy().copy(), np.zeros(n)
    for k in range(3):
        grad = g.normal(size=n) * 10.0 ** g.uniform(-6, 2, n)
        p.grad = torch.from_numpy(grad.copy())
        opt.step()
        mine, sq = R.rmsprop_step(mine, sq, grad, lr, alpha, eps)
        assert np.abs(mine - p.detach().numpy()).max() <= 1e-12
        assert np.abs(sq - opt.state[p]["square_avg"].numpy()).max() <= 1e-12 * max(1.0, sq.max())


def test_policy_forward_mlp_gru_equals_the_module():
    """a2c_ref.policy_forward("mlp_gru") is mlp_rec_ref.MLPRecRef's model: same value and
    head output to 1e-12 (T = 3, n = 4, masks with resets)"""
    torch.manual_seed(2)
    from a2c_ppo_acktr.synthetic import MultiBinary
    pol = M.Policy((6,), MultiBinary(5), base=M.MLPBase, base_kwargs={"recurrent": True, "hidden_size": 32},
                   vector_obs_len=2)
    T, n = 3, 4
    g = torch.Generator().manual_seed(1)
    obs, vec = torch.randn(T * n, 6, generator=g), torch.rand(T * n, 2, generator=g)
    h0 = torch.randn(n, 32, generator=g)
    masks = (torch.rand(T, n, generator=g) > 0.3).float()
    params = list(pol.parameters())
    v, z = R.policy_forward("mlp_gru", [p.detach().double() for p in params], obs, vec, h0, masks)
    v2, z2, _ = mlp_rec_ref.forward(params, "bern", torch.cat([obs, vec], 1).numpy(), h0.numpy(), masks.numpy())
    assert np.abs(v.numpy() - v2).max() <= 1e-12 and np.abs(z.numpy() - z2).max() <= 1e-12


# -------------------------------------------------------------- planted errors
CASES = [("cat", 64, 3, 37, "idx", False, 1), ("gauss", 128, 6, 37, "idx", True, 2), ("bern", 64, 8, 129, 5, False, 1)]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_float64_autograd_meets_the_gpu_comparison(case):
    """torch float64 autograd of the restated loss on a GPU test case passes check_grads /
    check_losses against the case's closed-form reference (and torch's CPU fp32 does too:
    the bound is reachable in fp32)."""
    c = R.build_case(*case)
    for dtype in (torch.float64, torch.float32):
        got = R.torch_head_grads(c, dtype)
        R.check_grads(got, c["ref"], show=lambda *a: None)
        R.check_losses(got["losses"], c["ref"]["losses"])


@pytest.mark.parametrize("planted", ["half", "attached", "normalized"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_planted_loss_errors_are_rejected(case, planted):
    """a 0.5 on the value loss, an advantage that is not detached, normalised advantages:
    each computed in float64 (no rounding to hide behind) fails check_grads, and the first
    and the last fail check_losses too"""
    c = R.build_case(*case)
    got = R.torch_head_grads(c, torch.float64, planted)
    with pytest.raises(AssertionError):
        R.check_grads(got, c["ref"], show=lambda *a: None)
    if planted != "attached":   # detaching changes gradients, not the loss values
        with pytest.raises(AssertionError):
            R.check_losses(got["losses"], c["ref"]["losses"])


def test_planted_swapped_alpha_is_rejected():
    """w (g g) with alpha and 1 - alpha exchanged fails check_rmsprop on square_avg and on
    the parameters; the right step passes"""
    g = np.random.default_rng(11)
    n, lr, alpha, eps = 255, 7e-4, 0.99, 1e-5
    p, sq = g.normal(size=n), g.uniform(0, 1, n)
    grad = g.normal(size=n) * 10.0 ** g.uniform(-6, 2, n)
    norm = np.sqrt((grad ** 2).sum())
    good = R.rmsprop_step(p, sq, grad, lr, alpha, eps)
    bad = R.rmsprop_step(p, sq, grad, lr, alpha, eps, planted="swapped")
    R.check_rmsprop((norm, grad, good[0].astype(np.float32), good[1].astype(np.float32)), (norm, grad) + good,
                    show=lambda *a: None)
    with pytest.raises(AssertionError):
        R.check_rmsprop((norm, grad, good[0], bad[1]), (norm, grad) + good, show=lambda *a: None)
    with pytest.raises(AssertionError):
        R.check_rmsprop((norm, grad, bad[0], good[1]), (norm, grad) + good, show=lambda *a: None)


# ------------------------------------------------------------------------- ABI
def test_new_entry_points_declared_bound_and_exported():
    from a2c_ppo_acktr import _hip
    src = open(HEADER).read()
    lib = _hip.lib()
    for name in NEW:
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", src)
        assert decl, name
        assert decl.group(1).count(",") + 1 == len(_hip.SIGNATURES[name]), name
        assert hasattr(lib, name), name
    assert lib.ppo_abi_version() == 3
    # the A2C entry points have no old_logp / adv / vpred / clip / clipped-value arguments
    for name, sib in zip(NEW[:3], ("ppo_heads_train", "ppo_heads_gauss_train", "ppo_heads_bern_train")):
        assert len(_hip.SIGNATURES[name]) == len(_hip.SIGNATURES[sib]) - 5
        args = re.search(name + r"\s*\(([^)]*)\)", src).group(1)
        assert not re.search(r"\b(old_logp|adv|vpred|clip)\b", args), args


# ------------------------------------------------------------------ host side
def _policy(seed=3):
    torch.manual_seed(seed)
    return M.Policy((4, 84, 84), Discrete(6), base=M.CNNBase, base_kwargs={"recurrent": False, "hidden_size": 64})


def _a2c(pol, lr=7e-4):
    return A2C_ACKTR(pol, 0.5, 0.01, lr=lr, eps=1e-5, alpha=0.99, max_grad_norm=0.5)


def test_a2c_constructs_without_a_gpu():
    agent = _a2c(_policy())
    g = agent.optimizer.param_groups[0]
    assert g["lr"] == 7e-4 and g["alpha"] == 0.99 and g["eps"] == 1e-5
    assert agent.optimizer.max_grad_norm == 0.5 and agent.optimizer.step_count == 0
    assert agent.optimizer.last_grad_norm is None and agent.optimizer.guard is None
    from a2c_ppo_acktr import utils
    utils.update_linear_schedule(agent.optimizer, 5, 10, 7e-4)
    assert agent.optimizer.param_groups[0]["lr"] == pytest.approx(3.5e-4)
    sd = agent.optimizer.state_dict()
    assert sd["step"] == 0 and sd["square_avg"] is None and "params" not in sd["param_groups"][0]
    agent.optimizer.zero_grad()


def test_acktr_is_not_implemented():
    with pytest.raises(NotImplementedError):
        A2C_ACKTR(_policy(), 0.5, 0.01, acktr=True)


def _fill(agent, n, step=7):
    g = torch.Generator().manual_seed(0)
    sd = agent.optimizer.state_dict()
    sd["step"] = step
    for k in agent.optimizer.STATE:
        sd[k] = torch.rand(n, generator=g)
    sd["param_groups"][0]["lr"] = 1.25e-4
    agent.optimizer.load_state_dict(sd)


def test_checkpoint_roundtrips_rmsprop_state(tmp_path):
    pol = _policy()
    agent = _a2c(pol)
    n = sum(p.numel() for p in pol.parameters())
    _fill(agent, n)
    path = str(tmp_path / "a2c.pt")
    CK.save_checkpoint(path, pol, None, agent=agent)
    raw = torch.load(path, weights_only=True)
    assert raw["format"] == CK.FORMAT and raw["optimizer"]["kind"] == "rmsprop"
    assert "exp_avg" not in raw["optimizer"]
    agent2 = _a2c(_policy(seed=99), lr=1.0)
    pol2, _ = CK.load_checkpoint(path, agent=agent2)
    assert pol2 is agent2.actor_critic
    for a, b in zip(pol.parameters(), pol2.parameters()):
        assert torch.equal(a, b)
    o1, o2 = agent.optimizer.state_dict(), agent2.optimizer.state_dict()
    assert o2["step"] == 7 and torch.equal(o1["square_avg"], o2["square_avg"])
    assert agent2.optimizer.param_groups[0]["lr"] == 1.25e-4 and agent2.optimizer.param_groups[0]["alpha"] == 0.99


def _ppo(pol):
    return PPO(pol, 0.1, 2, 2, 0.5, 0.01, lr=3e-4, eps=1e-5, max_grad_norm=0.5)


def test_cross_loading_optimizer_kinds_raises(tmp_path):
    pol = _policy()
    n = sum(p.numel() for p in pol.parameters())
    a2c, ppo = _a2c(pol), _ppo(pol)
    _fill(a2c, n)
    _fill(ppo, n)
    pa, pp = str(tmp_path / "a2c.pt"), str(tmp_path / "ppo.pt")
    CK.save_checkpoint(pa, pol, None, agent=a2c)
    CK.save_checkpoint(pp, pol, None, agent=ppo)
    assert torch.load(pp, weights_only=True)["optimizer"]["kind"] == "adam"
    with pytest.raises(ValueError, match="rmsprop.*adam"):
        CK.load_checkpoint(pa, agent=_ppo(_policy(seed=4)))
    with pytest.raises(ValueError, match="adam.*rmsprop"):
        CK.load_checkpoint(pp, agent=_a2c(_policy(seed=4)))


def test_checkpoint_without_a_kind_loads_into_ppo(tmp_path):
    """the optimizer block as written before RMSprop existed (step, exp_avg, exp_avg_sq,
    param_groups; no "kind") loads into a PPO agent unchanged and is refused by an A2C one"""
    pol = _policy()
    n = sum(p.numel() for p in pol.parameters())
    ppo = _ppo(pol)
    _fill(ppo, n)
    path = str(tmp_path / "old.pt")
    CK.save_checkpoint(path, pol, None, agent=ppo)
    raw = torch.load(path, weights_only=True)
    del raw["optimizer"]["kind"]
    assert sorted(raw["optimizer"]) == ["exp_avg", "exp_avg_sq", "param_groups", "step"]
    torch.save(raw, path)
    ppo2 = _ppo(_policy(seed=5))
    CK.load_checkpoint(path, agent=ppo2)
    o1, o2 = ppo.optimizer.state_dict(), ppo2.optimizer.state_dict()
    assert o2["step"] == 7 and torch.equal(o1["exp_avg"], o2["exp_avg"]) and torch.equal(o1["exp_avg_sq"],
                                                                                        o2["exp_avg_sq"])
    assert ppo2.optimizer.param_groups[0]["betas"] == (0.9, 0.999)
    with pytest.raises(ValueError):
        CK.load_checkpoint(path, agent=_a2c(_policy(seed=6)))
