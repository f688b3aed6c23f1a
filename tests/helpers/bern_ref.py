"""float64 reference of the Bernoulli loss head (distributions.py:45-56, 93-104,
algo/ppo.py:61-81): value / logits -> losses and their analytic gradients, with
torch autograd's tie conventions (gauss_ref.gauss_loss_head_grads is the DiagGaussian
counterpart; the ratio / clip / value-loss part is the same).

    p_o      = sigmoid(z_o)
    log_prob = Σ_o [ a_o z_o - softplus(z_o) ]
    entropy  = Σ_o [ softplus(-z_o) + (1 - p_o) z_o ]
    dL/dz_o  = g_logp (a_o - p_o) + (entropy_coef / B) z_o p_o (1 - p_o)
"""
import numpy as np


def _softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def _sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def bern_logp_entropy(logits, actions):
    z = np.asarray(logits, np.float64)
    a = np.asarray(actions, np.float64).reshape(z.shape)
    logp = (a * z - _softplus(z)).sum(-1)
    ent = (_softplus(-z) + _sigmoid(-z) * z).sum(-1)
    return logp, ent


def bern_loss_head_grads(value, logits, actions, old_logp, adv, vpred_old, returns, clip, value_coef, entropy_coef,
                         use_clipped_value_loss=True):
    B = np.asarray(value).shape[0]
    z = np.asarray(logits, np.float64)
    a = np.asarray(actions, np.float64).reshape(z.shape)
    logp, ent_row = bern_logp_entropy(z, a)
    A = np.asarray(adv, np.float64).reshape(B)
    ratio = np.exp(logp - np.asarray(old_logp, np.float64).reshape(B))
    surr1 = ratio * A
    surr2 = np.clip(ratio, 1.0 - clip, 1.0 + clip) * A
    action_loss = -np.minimum(surr1, surr2).mean()
    w1 = np.where(surr1 < surr2, 1.0, np.where(surr1 == surr2, 0.5, 0.0))
    inr = ((ratio >= 1.0 - clip) & (ratio <= 1.0 + clip)).astype(np.float64)
    g_logp = -(1.0 / B) * (w1 * A + (1.0 - w1) * A * inr) * ratio
    v = np.asarray(value, np.float64).reshape(B)
    vo = np.asarray(vpred_old, np.float64).reshape(B)
    R = np.asarray(returns, np.float64).reshape(B)
    if use_clipped_value_loss:
        dv = v - vo
        vpc = vo + np.clip(dv, -clip, clip)
        l1, l2 = (v - R) ** 2, (vpc - R) ** 2
        value_loss = 0.5 * np.maximum(l1, l2).mean()
        u1 = np.where(l1 > l2, 1.0, np.where(l1 == l2, 0.5, 0.0))
        vin = ((dv >= -clip) & (dv <= clip)).astype(np.float64)
        g_v = value_coef * (0.5 / B) * (u1 * 2 * (v - R) + (1.0 - u1) * 2 * (vpc - R) * vin)
    else:
        value_loss = 0.5 * ((R - v) ** 2).mean()
        g_v = value_coef * (1.0 / B) * (v - R)
    p = _sigmoid(z)
    g_logits = g_logp[:, None] * (a - p) + (entropy_coef / B) * z * p * _sigmoid(-z)
    return dict(value_loss=value_loss, action_loss=action_loss, entropy=ent_row.mean(), g_value=g_v,
                g_logits=g_logits, logp=logp, ratio=ratio, clipped_value=(np.abs(v - vo) > clip)
                if use_clipped_value_loss else np.zeros(B, bool))


def mlp_bern_param_shapes(num_inputs, hidden, num_actions):
    """named_parameters() order of Policy((I,), MultiBinary(A), MLPBase)"""
    I, H = num_inputs, hidden
    return [("base.actor.0.weight", (H, I)), ("base.actor.0.bias", (H,)),
            ("base.actor.2.weight", (H, H)), ("base.actor.2.bias", (H,)),
            ("base.critic.0.weight", (H, I)), ("base.critic.0.bias", (H,)),
            ("base.critic.2.weight", (H, H)), ("base.critic.2.bias", (H,)),
            ("base.critic_linear.weight", (1, H)), ("base.critic_linear.bias", (1,)),
            ("dist.linear.weight", (num_actions, H)), ("dist.linear.bias", (num_actions,))]
