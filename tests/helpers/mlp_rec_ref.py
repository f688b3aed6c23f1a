"""float64 restatement of the recurrent MLPBase policy (model.py:111-166, 224-234) on
the CPU, built from torch's own nn.GRU / nn.Linear with autograd:

    x   = cat(obs, vector_obs)                          [T*n, I], rows t*n + j
    h_t = GRU(x_t, h_{t-1} * mask_t)                    (what _forward_gru computes, per step)
    a   = tanh(W_a2 tanh(W_a1 h + b_a1) + b_a2),  c likewise with the critic's weights
    value = critic_linear(c),  head = dist's linear layer on a

and the project's PPO loss in float64: the head's analytic gradients come from
oracle.loss_head_grads (Discrete) or the gauss_ref / bern_ref helpers, and autograd
carries them through the towers and the GRU.  Parameters are taken positionally from
the fp32 policy's policy.parameters() (gru.*, actor.*, critic.*, critic_linear, dist)."""
import numpy as np
import torch
import torch.nn as nn

from helpers import bern_ref, gauss_ref
from oracle import ppo_oracle as O


class MLPRecRef(nn.Module):
    def __init__(self, params, kind="cat"):
        """params: the fp32 policy's parameters in policy.parameters() order (any device)"""
        super().__init__()
        params = [p.detach().cpu().double() for p in params]
        H, I = params[1].shape[1], params[0].shape[1]
        A = params[14].shape[0]
        self.kind, self.H, self.I, self.A = kind, H, I, A
        self.gru = nn.GRU(I, H)
        tower = lambda: nn.Sequential(nn.Linear(H, H), nn.Tanh(), nn.Linear(H, H), nn.Tanh())  # noqa: E731
        self.actor, self.critic = tower(), tower()
        self.critic_linear = nn.Linear(H, 1)
        self.head = nn.Linear(H, A)
        if kind == "gauss":
            self.logstd = nn.Parameter(torch.zeros(A, 1))
        self.double()
        own = self.ordered()
        assert len(own) == len(params) == (17 if kind == "gauss" else 16), (len(own), len(params))
        with torch.no_grad():
            for q, p in zip(own, params):
                assert q.shape == p.shape, (q.shape, p.shape)
                q.copy_(p)

    def ordered(self):
        """parameters in policy.parameters() order (a module's own parameters — logstd —
        would otherwise come first)"""
        mods = (self.gru, self.actor, self.critic, self.critic_linear, self.head)
        return [p for m in mods for p in m.parameters()] + ([self.logstd] if self.kind == "gauss" else [])

    def forward(self, x, h0, masks):
        """x [T*n, I], h0 [n, H], masks [T, n] -> value [T*n], head [T*n, A], h_t [T*n, H]"""
        T, n = masks.shape
        xs = x.reshape(T, n, self.I)
        h = h0
        outs = []
        for t in range(T):
            _, hn = self.gru(xs[t:t + 1], (h * masks[t].reshape(n, 1))[None])
            h = hn[0]
            outs.append(h)
        hs = torch.cat(outs, 0)
        value = self.critic_linear(self.critic(hs))[:, 0]
        return value, self.head(self.actor(hs)), hs


def _t(a):
    return torch.as_tensor(np.asarray(a, np.float64))


def forward(params, kind, x, h0, masks):
    """numpy (value, head output, hidden states) of the float64 model, no gradients"""
    ref = MLPRecRef(params, kind)
    with torch.no_grad():
        value, out, hs = ref(_t(x), _t(h0), _t(masks))
    return value.numpy(), out.numpy(), hs.numpy()


def logp_entropy(params, kind, out, actions):
    """per-row log-prob and entropy of `actions` under the head output `out`"""
    if kind == "gauss":
        return gauss_ref.gauss_logp_entropy(out, params[16].detach().cpu().double().numpy()[:, 0], actions)
    if kind == "bern":
        return bern_ref.bern_logp_entropy(out, actions)
    c = O.categorical(out)
    a = np.asarray(actions).reshape(-1).astype(np.int64)
    return np.take_along_axis(c["norm_logits"], a[:, None], -1)[:, 0], c["entropy"]


def functional_grads(params, kind, x, h0, masks, c_value, c_out):
    """gradients of Σ c_value·value + Σ c_out·head output w.r.t. every parameter (numpy list,
    policy.parameters() order) and the forward outputs"""
    ref = MLPRecRef(params, kind)
    value, out, hs = ref(_t(x), _t(h0), _t(masks))
    torch.autograd.backward([value, out], [_t(c_value), _t(c_out)])
    grads = [(p.grad if p.grad is not None else torch.zeros_like(p)).numpy() for p in ref.ordered()]
    return grads, value.detach().numpy(), out.detach().numpy(), hs.detach().numpy()


def minibatch(params, kind, x, h0, masks, actions, old_logp, adv, vpred, returns, clip, value_coef, entropy_coef):
    """One recurrent minibatch: the three losses and dL/d(parameter) for every parameter.
    Rows of every per-sample argument are t*n + j, as x."""
    ref = MLPRecRef(params, kind)
    value, out, _ = ref(_t(x), _t(h0), _t(masks))
    v, o = value.detach().numpy(), out.detach().numpy()
    if kind == "gauss":
        r = gauss_ref.gauss_loss_head_grads(v, o, ref.logstd.detach().numpy()[:, 0], actions, old_logp, adv, vpred,
                                            returns, clip, value_coef, entropy_coef)
        g_out = r["g_mean"]
    elif kind == "bern":
        r = bern_ref.bern_loss_head_grads(v, o, actions, old_logp, adv, vpred, returns, clip, value_coef,
                                          entropy_coef)
        g_out = r["g_logits"]
    else:
        r = O.loss_head_grads(v, o, actions, old_logp, adv, vpred, returns, clip, value_coef, entropy_coef)
        g_out = r["g_logits"]
    torch.autograd.backward([value, out], [_t(r["g_value"]), _t(g_out)])
    if kind == "gauss":
        ref.logstd.grad = _t(r["g_logstd"]).reshape(-1, 1)   # the head helper's own (no autograd path)
    grads = [p.grad.numpy() for p in ref.ordered()]
    return dict(grads=grads, losses=np.array([r["value_loss"], r["action_loss"], r["entropy"]]), value=v, out=o,
                logp=r["logp"])
