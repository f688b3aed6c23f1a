"""Box action spaces (DiagGaussian) — host-side checks: the ABI carries the Gaussian
heads entry points, the Box duck type, the package's FixedNormal against the
reference's record (gauss.npz), and the float64 loss-head helper against autograd."""
import os
import pickle
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
from helpers import gauss_ref as G

HEADER = os.path.join(ROOT, "include", "ppo_hip.h")
NEW = ("ppo_heads_gauss_act", "ppo_heads_gauss_train", "ppo_heads_gauss_reduce")


def test_gauss_symbols_declared_and_exported():
    from a2c_ppo_acktr import _hip
    src = open(HEADER).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _hip.LIB_PATH], capture_output=True, text=True, check=True)
    exported = {ln.split()[-1] for ln in out.stdout.splitlines() if ln.strip()}
    for name in NEW:
        decl = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)", src, re.M)
        assert decl, name + " is not declared in include/ppo_hip.h"
        assert decl.group(1).count(",") + 1 == len(_hip.SIGNATURES[name]), name
        assert name in exported, name + " is not exported by libppo_hip.so"
    assert _hip.call("ppo_abi_version") == 3   # symbols were only added


def test_box_space_pickles_and_names_parameters():
    from a2c_ppo_acktr import model as M
    from a2c_ppo_acktr.distributions import DiagGaussian
    from a2c_ppo_acktr.storage import RolloutStorage
    from a2c_ppo_acktr.synthetic import Box
    box = pickle.loads(pickle.dumps(Box(-2.0, 2.0, (3,))))
    assert box.__class__.__name__ == "Box" and box.shape == (3,) and (box.low, box.high) == (-2.0, 2.0)
    d = golden("gauss.npz")
    pol = M.Policy((4,), box, base=M.MLPBase, base_kwargs={"recurrent": False, "hidden_size": 64})
    assert isinstance(pol.dist, DiagGaussian)
    want = ["base." + n for n in d["base_names"]] + ["dist." + n for n in d["head_names"]]
    assert [n for n, _ in pol.named_parameters()] == want
    assert want[-3:] == ["dist.fc_mean.weight", "dist.fc_mean.bias", "dist.logstd._bias"]   # the engine's WA, BA, LS
    assert sum(p.numel() for p in pol.parameters()) == d["base_params"].size + d["head_params"].size
    st = RolloutStorage(5, 2, (4,), [0], box, 1)
    assert st.actions.shape == (5, 2, 3) and st.actions.dtype == torch.float32


def test_fixed_normal_reproduces_reference_record():
    """The package's DiagGaussian / FixedNormal on the recorded actor features and
    head parameters: mean, std, log_probs, entropy, mode and — from the recorded
    generator state — the sample, bit for bit; and sample == noise * std + mean as
    a rounded multiply then add (what the HIP kernel computes)."""
    from a2c_ppo_acktr.distributions import DiagGaussian
    d = golden("gauss.npz")
    torch.set_num_threads(1)
    head = DiagGaussian(64, 3)
    with torch.no_grad():
        flat, off = torch.from_numpy(d["head_params"]), 0
        for p in head.parameters():
            p.copy_(flat[off:off + p.numel()].view_as(p))
            off += p.numel()
        dist = head(torch.from_numpy(d["actor_features"]))
        assert torch.equal(dist.mean, torch.from_numpy(d["mean"]))
        assert torch.equal(dist.stddev, torch.from_numpy(d["std"]))
        act = torch.from_numpy(d["action"])
        assert torch.equal(dist.log_probs(act), torch.from_numpy(d["log_probs"]))
        assert torch.equal(dist.entropy(), torch.from_numpy(d["entropy"]))
        assert torch.equal(dist.mode(), torch.from_numpy(d["mode"]))
        keep = torch.get_rng_state()
        try:
            torch.set_rng_state(torch.from_numpy(d["rng_state"]))
            assert torch.equal(dist.sample(), act)
            torch.set_rng_state(torch.from_numpy(d["rng_state"]))
            eps = torch.empty(8, 3).normal_()
        finally:
            torch.set_rng_state(keep)
        assert torch.equal(eps, torch.from_numpy(d["normal_noise"]))
        assert torch.equal(eps * dist.stddev + dist.mean, act)
    # the float64 helper agrees with the record to fp32 precision
    lp, ent = G.gauss_logp_entropy(d["mean"], np.log(d["std"][0].astype(np.float64)), d["action"])
    np.testing.assert_allclose(lp, d["log_probs"][:, 0], atol=1e-5)
    np.testing.assert_allclose(ent, d["entropy"], atol=1e-6)


def _case(A, B, seed, use_clipped):
    g = np.random.default_rng(seed)
    value, mean = g.normal(size=B), g.normal(size=(B, A))
    logstd = g.uniform(-1.0, 0.5, size=A)
    actions = mean + np.exp(logstd) * g.normal(size=(B, A))
    lp, _ = G.gauss_logp_entropy(mean, logstd, actions)
    old_logp = lp + g.normal(size=B) * 0.15      # ratios on both sides of the clip range
    old_logp[:3] = lp[:3]                        # ratio exactly 1 (the first epoch's case)
    adv = g.normal(size=B)
    vpred = value + g.normal(size=B) * 0.2       # |v - v_old| on both sides of clip
    ret = g.normal(size=B)
    return value, mean, logstd, actions, old_logp, adv, vpred, ret


@pytest.mark.parametrize("A", [1, 3])
@pytest.mark.parametrize("use_clipped", [True, False])
def test_float64_helper_equals_autograd(A, use_clipped):
    """gauss_ref.gauss_loss_head_grads == torch float64 autograd of the reference's
    loss (algo/ppo.py:61-81 with FixedNormal) to 1e-10, on a batch holding rows with
    a clipped ratio, rows inside the range, and rows with a clipped value."""
    from a2c_ppo_acktr.distributions import FixedNormal
    B, clip, vc, ec = 64, 0.1, 0.5, 0.01
    value, mean, logstd, actions, old_logp, adv, vpred, ret = _case(A, B, 7 + A, use_clipped)
    r = G.gauss_loss_head_grads(value, mean, logstd, actions, old_logp, adv, vpred, ret, clip, vc, ec, use_clipped)
    out = (r["ratio"] < 1 - clip) | (r["ratio"] > 1 + clip)
    assert out.sum() >= 5 and (~out).sum() >= 5
    if use_clipped:
        assert r["clipped_value"].sum() >= 5 and (~r["clipped_value"]).sum() >= 5
    t = lambda x: torch.tensor(x, dtype=torch.float64)  # noqa: E731
    v, mu, s = t(value).requires_grad_(), t(mean).requires_grad_(), t(logstd).requires_grad_()
    dist = FixedNormal(mu, s.exp().expand_as(mu))
    logp = dist.log_probs(t(actions))
    entropy = dist.entropy().mean()
    ratio = torch.exp(logp - t(old_logp)[:, None])
    a_ = t(adv)[:, None]
    action_loss = -torch.min(ratio * a_, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * a_).mean()
    values, vp, R = v[:, None], t(vpred)[:, None], t(ret)[:, None]
    if use_clipped:
        vpc = vp + (values - vp).clamp(-clip, clip)
        value_loss = 0.5 * torch.max((values - R).pow(2), (vpc - R).pow(2)).mean()
    else:
        value_loss = 0.5 * (R - values).pow(2).mean()
    (value_loss * vc + action_loss - entropy * ec).backward()
    for got, ref in ((r["value_loss"], value_loss), (r["action_loss"], action_loss), (r["entropy"], entropy),
                     (r["logp"], logp[:, 0]), (r["g_value"], v.grad), (r["g_mean"], mu.grad),
                     (r["g_logstd"], s.grad)):
        np.testing.assert_allclose(got, ref.detach().numpy(), rtol=0, atol=1e-10)
