"""The float64 yardstick of the recurrent MLPBase tests (helpers/mlp_rec_ref.py: torch's
nn.GRU / nn.Linear with autograd) against a second, independent float64 implementation
— the oracle's numpy GRU (gru_sequence_cache / gru_backward) composed with its numpy
MLP towers (mlp_forward / mlp_backward) — and the parameter order the engine indexes."""
import numpy as np
import torch

from helpers import mlp_rec_ref as R
from oracle import ppo_oracle as O


def _policy(I0, V, H, A, seed=0):
    from a2c_ppo_acktr import model as M
    from a2c_ppo_acktr.synthetic import Discrete
    torch.manual_seed(seed)
    return M.Policy((I0,), Discrete(A), base=M.MLPBase, base_kwargs={"recurrent": True, "hidden_size": H},
                    vector_obs_len=V)


def test_recurrent_mlp_parameter_order():
    """gru.{weight_ih, weight_hh, bias_ih, bias_hh}, actor.0, actor.2, critic.0, critic.2,
    critic_linear, then the distribution's parameters (RecurrentMLPEngine's indices);
    the towers' first layers are H x H (model.py:207-208 num_inputs = hidden_size)."""
    I0, V, H, A = 5, 2, 32, 6
    pol = _policy(I0, V, H, A)
    want = [("base.gru.weight_ih_l0", (3 * H, I0 + V)), ("base.gru.weight_hh_l0", (3 * H, H)),
            ("base.gru.bias_ih_l0", (3 * H,)), ("base.gru.bias_hh_l0", (3 * H,)),
            ("base.actor.0.weight", (H, H)), ("base.actor.0.bias", (H,)),
            ("base.actor.2.weight", (H, H)), ("base.actor.2.bias", (H,)),
            ("base.critic.0.weight", (H, H)), ("base.critic.0.bias", (H,)),
            ("base.critic.2.weight", (H, H)), ("base.critic.2.bias", (H,)),
            ("base.critic_linear.weight", (1, H)), ("base.critic_linear.bias", (1,)),
            ("dist.linear.weight", (A, H)), ("dist.linear.bias", (A,))]
    assert [(n, tuple(p.shape)) for n, p in pol.named_parameters()] == want
    assert pol.is_recurrent and pol.recurrent_hidden_state_size == H


def test_reference_agrees_with_oracle_composition():
    """T = 4, n = 3, I = 7, H = 32: forward outputs and the gradients of a random linear
    functional of (value, logits) from the autograd model and from the oracle's analytic
    GRU BPTT + tower backward agree to 1e-10 relative per tensor."""
    T, n, I, H, A = 4, 3, 7, 32, 6
    pol = _policy(5, 2, H, A, seed=11)
    g = torch.Generator().manual_seed(12)
    with torch.no_grad():
        pol.base.gru.bias_ih_l0.uniform_(-0.3, 0.3, generator=g)
        pol.base.gru.bias_hh_l0.uniform_(-0.3, 0.3, generator=g)
        for name, p in pol.named_parameters():
            if name.endswith("bias") and "gru" not in name:
                p.uniform_(-0.2, 0.2, generator=g)
    params = list(pol.parameters())
    x = torch.randn(T * n, I, generator=g).double().numpy()
    h0 = (0.5 * torch.randn(n, H, generator=g)).double().numpy()
    masks = (torch.rand(T, n, generator=g) > 0.3).double().numpy()
    assert (masks[1:] == 0).any() and (masks == 1).any()
    cv = torch.randn(T * n, generator=g).double().numpy()
    cl = torch.randn(T * n, A, generator=g).double().numpy()
    grads, value, logits, hs = R.functional_grads(params, "cat", x, h0, masks, cv, cl)

    names = [nm for nm, _ in pol.named_parameters()]
    p = {nm: q.detach().double().numpy() for nm, q in pol.named_parameters()}
    out, gcache = O.gru_sequence_cache(p, x, h0, masks)
    value2, logits2, cache = O.mlp_forward(p, out)
    g2 = O.mlp_backward(p, cache, cv, cl)
    # dL/d(GRU output): each tower's first-layer gradient through its weight (mlp_backward
    # keeps it internal), from the same cache
    douts = {"critic": cv[:, None] * p["base.critic_linear.weight"], "actor": cl @ p["dist.linear.weight"]}
    dout = np.zeros_like(out)
    for tower in ("actor", "critic"):
        h1, h2 = cache[tower]
        dz1 = ((douts[tower] * (1 - h2 * h2)) @ p[f"base.{tower}.2.weight"]) * (1 - h1 * h1)
        dout += dz1 @ p[f"base.{tower}.0.weight"]
    gg, _ = O.gru_backward(p, x, masks, gcache, dout)
    g2.update(gg)

    def rel(a, b):
        return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)

    assert rel(hs, out) <= 1e-10 and rel(value, value2) <= 1e-10 and rel(logits, logits2) <= 1e-10
    for nm, ga in zip(names, grads):
        assert np.abs(g2[nm]).max() > 0, nm
        assert rel(ga, g2[nm].reshape(ga.shape)) <= 1e-10, (nm, rel(ga, g2[nm].reshape(ga.shape)))
