"""MultiBinary action spaces (Bernoulli) — host-side checks: the ABI carries the
Bernoulli heads entry points, the MultiBinary duck type, the package's FixedBernoulli
against the reference's record (bern.npz), and the float64 loss-head helper against
autograd."""
import os
import pickle
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
from helpers import bern_ref as R

HEADER = os.path.join(ROOT, "include", "ppo_hip.h")
# the two new entry points and the Categorical reduce that sums their partials (the
# partial layouts are identical, so there is no ppo_heads_bern_reduce)
SYMBOLS = ("ppo_heads_bern_act", "ppo_heads_bern_train", "ppo_heads_reduce")


def test_bern_symbols_declared_and_exported():
    from a2c_ppo_acktr import _hip
    src = open(HEADER).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _hip.LIB_PATH], capture_output=True, text=True, check=True)
    exported = {ln.split()[-1] for ln in out.stdout.splitlines() if ln.strip()}
    for name in SYMBOLS:
        decl = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)", src, re.M)
        assert decl, name + " is not declared in include/ppo_hip.h"
        assert decl.group(1).count(",") + 1 == len(_hip.SIGNATURES[name]), name
        assert name in exported, name + " is not exported by libppo_hip.so"
    assert "ppo_heads_bern_reduce" not in exported
    assert _hip.call("ppo_abi_version") == 3   # symbols were only added


def test_multibinary_space_pickles_and_names_parameters():
    from a2c_ppo_acktr import model as M
    from a2c_ppo_acktr.distributions import Bernoulli
    from a2c_ppo_acktr.storage import RolloutStorage
    from a2c_ppo_acktr.synthetic import MultiBinary
    mb = pickle.loads(pickle.dumps(MultiBinary(3)))
    assert mb.__class__.__name__ == "MultiBinary" and mb.shape == (3,) and mb.n == 3
    d = golden("bern.npz")
    pol = M.Policy((4,), mb, base=M.MLPBase, base_kwargs={"recurrent": False, "hidden_size": 64})
    assert isinstance(pol.dist, Bernoulli)
    want = ["base." + n for n in d["base_names"]] + ["dist." + n for n in d["head_names"]]
    assert [n for n, _ in pol.named_parameters()] == want
    assert want[-2:] == ["dist.linear.weight", "dist.linear.bias"]   # the engine's WA, BA
    assert want == [n for n, _ in R.mlp_bern_param_shapes(4, 64, 3)]
    assert sum(p.numel() for p in pol.parameters()) == d["base_params"].size + d["head_params"].size
    st = RolloutStorage(5, 2, (4,), [0], mb, 1)
    assert st.actions.shape == (5, 2, 3) and st.actions.dtype == torch.float32


def test_multibinary_config_round_trips():
    """checkpoint._space / _Space rebuild a MultiBinary policy's action space by class
    name and shape (the GPU file saves and loads a whole checkpoint)."""
    from a2c_ppo_acktr import checkpoint as C
    from a2c_ppo_acktr import model as M
    from a2c_ppo_acktr.distributions import Bernoulli
    from a2c_ppo_acktr.synthetic import MultiBinary
    sp = C._Space(C._space(MultiBinary(5)))
    assert sp.__class__.__name__ == "MultiBinary" and sp.shape == (5,)
    pol = M.Policy((4,), sp, base=M.MLPBase, base_kwargs={"recurrent": False, "hidden_size": 64})
    assert isinstance(pol.dist, Bernoulli) and pol.dist.linear.weight.shape == (5, 64)


def test_host_mode_noise_is_the_uniform_draw():
    """Policy._noise in host sampling mode draws torch.empty(n, A).uniform_() for a
    Bernoulli head and leaves the default generator where that draw does."""
    from a2c_ppo_acktr import model as M
    from a2c_ppo_acktr.synthetic import MultiBinary
    pol = M.Policy((4,), MultiBinary(3), base=M.MLPBase, base_kwargs={"recurrent": False, "hidden_size": 64})
    keep = torch.get_rng_state()
    M.set_sampling_mode("host")
    try:
        torch.manual_seed(3)
        u = pol._noise(7)
        after = torch.get_rng_state()
        torch.manual_seed(3)
        want = torch.empty(7, 3).uniform_()
        assert torch.equal(u, want) and torch.equal(torch.get_rng_state(), after)
        assert float(u.min()) >= 0.0 and float(u.max()) < 1.0
    finally:
        M.set_sampling_mode("device")
        torch.set_rng_state(keep)
    assert pol._noise(7) is None


def test_fixed_bernoulli_reproduces_reference_record():
    """The package's Bernoulli / FixedBernoulli on the recorded actor features and head
    parameters: logits, probs, log_probs, entropy, mode and — from the recorded
    generator state — the sample, bit for bit; and sample == (u < probs) on the
    recorded uniform_() draw (what the HIP kernel computes)."""
    from a2c_ppo_acktr.distributions import Bernoulli
    d = golden("bern.npz")
    torch.set_num_threads(1)
    head = Bernoulli(64, 3)
    with torch.no_grad():
        flat, off = torch.from_numpy(d["head_params"]), 0
        for p in head.parameters():
            p.copy_(flat[off:off + p.numel()].view_as(p))
            off += p.numel()
        dist = head(torch.from_numpy(d["actor_features"]))
        assert torch.equal(dist.logits, torch.from_numpy(d["logits"]))
        assert torch.equal(dist.probs, torch.from_numpy(d["probs"]))
        act = torch.from_numpy(d["action"])
        assert set(np.unique(d["action"])) <= {0.0, 1.0}
        assert torch.equal(dist.log_probs(act), torch.from_numpy(d["log_probs"]))
        assert torch.equal(dist.entropy(), torch.from_numpy(d["entropy"]))
        assert torch.equal(dist.mode(), torch.from_numpy(d["mode"]))
        keep = torch.get_rng_state()
        try:
            torch.set_rng_state(torch.from_numpy(d["rng_state"]))
            assert torch.equal(dist.sample(), act)
            after = torch.get_rng_state()
            torch.set_rng_state(torch.from_numpy(d["rng_state"]))
            u = torch.empty(8, 3).uniform_()
            assert torch.equal(torch.get_rng_state(), after)
        finally:
            torch.set_rng_state(keep)
        assert torch.equal(u, torch.from_numpy(d["uniform_noise"]))
        assert torch.equal((u < dist.probs).float(), act)
    # the float64 helper agrees with the record to fp32 precision
    lp, ent = R.bern_logp_entropy(d["logits"], d["action"])
    np.testing.assert_allclose(lp, d["log_probs"][:, 0], atol=1e-5)
    np.testing.assert_allclose(ent, d["entropy"], atol=1e-6)


def test_float64_helper_is_finite_when_saturated():
    z = np.array([[-100.0, 100.0, 0.0, 40.0, -40.0]])
    for a in (np.zeros_like(z), np.ones_like(z)):
        lp, ent = R.bern_logp_entropy(z, a)
        assert np.isfinite(lp).all() and np.isfinite(ent).all()
    lp, ent = R.bern_logp_entropy(z, np.array([[0.0, 1.0, 1.0, 1.0, 0.0]]))
    np.testing.assert_allclose(lp, -np.log(2.0), atol=1e-12)
    np.testing.assert_allclose(ent, np.log(2.0), atol=1e-12)


def _case(A, B, seed, use_clipped):
    g = np.random.default_rng(seed)
    value, logits = g.normal(size=B), g.normal(size=(B, A)) * 2.0
    actions = (g.uniform(size=(B, A)) < 1.0 / (1.0 + np.exp(-logits))).astype(np.float64)
    lp, _ = R.bern_logp_entropy(logits, actions)
    old_logp = lp + g.normal(size=B) * 0.15      # ratios on both sides of the clip range
    old_logp[:3] = lp[:3]                        # ratio exactly 1 (the first epoch's case)
    adv = g.normal(size=B)
    vpred = value + g.normal(size=B) * 0.2       # |v - v_old| on both sides of clip
    ret = g.normal(size=B)
    return value, logits, actions, old_logp, adv, vpred, ret


@pytest.mark.parametrize("A", [1, 3])
@pytest.mark.parametrize("use_clipped", [True, False])
def test_float64_helper_equals_autograd(A, use_clipped):
    """bern_ref.bern_loss_head_grads == torch float64 autograd of the reference's loss
    (algo/ppo.py:61-81 with FixedBernoulli) to 1e-10, on a batch holding rows with a
    clipped ratio, rows inside the range, and rows with a clipped value."""
    from a2c_ppo_acktr.distributions import FixedBernoulli
    B, clip, vc, ec = 64, 0.1, 0.5, 0.01
    value, logits, actions, old_logp, adv, vpred, ret = _case(A, B, 7 + A, use_clipped)
    r = R.bern_loss_head_grads(value, logits, actions, old_logp, adv, vpred, ret, clip, vc, ec, use_clipped)
    out = (r["ratio"] < 1 - clip) | (r["ratio"] > 1 + clip)
    assert out.sum() >= 5 and (~out).sum() >= 5
    if use_clipped:
        assert r["clipped_value"].sum() >= 5 and (~r["clipped_value"]).sum() >= 5
    t = lambda x: torch.tensor(x, dtype=torch.float64)  # noqa: E731
    v, z = t(value).requires_grad_(), t(logits).requires_grad_()
    dist = FixedBernoulli(logits=z)
    logp = dist.log_probs(t(actions))
    entropy = dist.entropy().mean()
    ratio = torch.exp(logp - t(old_logp)[:, None])
    a_ = t(adv)[:, None]
    action_loss = -torch.min(ratio * a_, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * a_).mean()
    values, vp, Rt = v[:, None], t(vpred)[:, None], t(ret)[:, None]
    if use_clipped:
        vpc = vp + (values - vp).clamp(-clip, clip)
        value_loss = 0.5 * torch.max((values - Rt).pow(2), (vpc - Rt).pow(2)).mean()
    else:
        value_loss = 0.5 * (Rt - values).pow(2).mean()
    (value_loss * vc + action_loss - entropy * ec).backward()
    for got, ref in ((r["value_loss"], value_loss), (r["action_loss"], action_loss), (r["entropy"], entropy),
                     (r["logp"], logp[:, 0]), (r["g_value"], v.grad), (r["g_logits"], z.grad)):
        np.testing.assert_allclose(got, ref.detach().numpy(), rtol=0, atol=1e-10)
