"""float64 reference of the DiagGaussian loss head (distributions.py:30-42, 71-86,
algo/ppo.py:61-81): value / mean / logstd -> losses and their analytic gradients,
with torch autograd's tie conventions (oracle/ppo_oracle.loss_head_grads is the
Categorical counterpart; the ratio / clip / value-loss part is the same).

    log_prob = Σ_o [ -(a_o - μ_o)² / (2 σ_o²) - log σ_o - log √(2π) ],  σ_o = exp(s_o)
    entropy  = Σ_o [ 0.5 + 0.5 log 2π + s_o ]
    dL/dμ_o  = g_logp (a_o - μ_o) / σ_o²
    dL/ds_o  = Σ_rows g_logp ((a_o - μ_o)² / σ_o² - 1) - entropy_coef
"""
import math

import numpy as np


def gauss_logp_entropy(mean, logstd, actions):
    mean = np.asarray(mean, np.float64)
    s = np.asarray(logstd, np.float64).reshape(1, -1)
    a = np.asarray(actions, np.float64).reshape(mean.shape)
    sig = np.exp(s)
    logp = (-(a - mean) ** 2 / (2 * sig * sig) - s - math.log(math.sqrt(2 * math.pi))).sum(-1)
    ent = (0.5 + 0.5 * math.log(2 * math.pi) + s).sum() * np.ones(mean.shape[0])
    return logp, ent


def gauss_loss_head_grads(value, mean, logstd, actions, old_logp, adv, vpred_old, returns, clip, value_coef,
                          entropy_coef, use_clipped_value_loss=True):
    B = np.asarray(value).shape[0]
    mean = np.asarray(mean, np.float64)
    s = np.asarray(logstd, np.float64).reshape(1, -1)
    a = np.asarray(actions, np.float64).reshape(mean.shape)
    logp, ent_row = gauss_logp_entropy(mean, s, a)
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
    ivar = np.exp(-2.0 * s)
    d = a - mean
    g_mean = g_logp[:, None] * d * ivar
    g_logstd = (g_logp[:, None] * (d * d * ivar - 1.0)).sum(0) - entropy_coef
    return dict(value_loss=value_loss, action_loss=action_loss, entropy=ent_row.mean(), g_value=g_v, g_mean=g_mean,
                g_logstd=g_logstd, logp=logp, ratio=ratio, clipped_value=(np.abs(v - vo) > clip)
                if use_clipped_value_loss else np.zeros(B, bool))


def mlp_gauss_param_shapes(num_inputs, hidden, num_actions):
    """named_parameters() order of Policy((I,), Box(A), MLPBase)"""
    I, H = num_inputs, hidden
    return [("base.actor.0.weight", (H, I)), ("base.actor.0.bias", (H,)),
            ("base.actor.2.weight", (H, H)), ("base.actor.2.bias", (H,)),
            ("base.critic.0.weight", (H, I)), ("base.critic.0.bias", (H,)),
            ("base.critic.2.weight", (H, H)), ("base.critic.2.bias", (H,)),
            ("base.critic_linear.weight", (1, H)), ("base.critic_linear.bias", (1,)),
            ("dist.fc_mean.weight", (num_actions, H)), ("dist.fc_mean.bias", (num_actions,)),
            ("dist.logstd._bias", (num_actions, 1))]
