"""float64 references of the A2C update (reference algo/a2c_acktr.py:33-80): the row
loss of the three distributions in closed form, a torch restatement of the loss for
autograd, RMSprop, the inputs of tests/test_a2c_heads_gpu.py and the comparisons the
A2C GPU tests use.

    adv         = R - v                       (detached in the action loss)
    value_loss  = mean(adv^2)                 (no 0.5)
    action_loss = -mean(adv log_prob)
    total       = value_coef value_loss + action_loss - entropy_coef mean(entropy)
    dL/dv       = value_coef (2 / B) (v - R),   dL/dlog_prob = -(1 / B) adv

The reference's own update() cannot be run to record vectors: its evaluate_actions
call has four arguments and the function five.  torch_loss restates its lines 45-51
and 71-72 with the package's FixedCategorical / FixedNormal / FixedBernoulli, and
test_a2c_cpu.py checks the closed forms against float64 autograd of that.

The A2C loss has no clamp, min or max: no branch can flip between float64 and fp32,
so (unlike cat_ref.build_case) the case builder needs no margin search, takes its
first seed, and no row is ever left out of a comparison.
"""
import functools

import numpy as np
import torch

from helpers import bern_ref as Bn
from helpers import cat_ref as C
from helpers import gauss_ref as G
from oracle import ppo_oracle as O

VC, EC = C.VC, C.EC
KINDS = ("cat", "gauss", "bern")


# ---------------------------------------------------------------- closed forms
def head_grads(kind, value, z, actions, returns, vc, ec, logstd=None):
    """float64: g_value [B], g_logits [B, A] (gauss: dL/dmean), g_logstd [A] (gauss) or
    None, value_loss, action_loss, entropy, logp [B]."""
    v = np.asarray(value, np.float64).reshape(-1)
    B = v.shape[0]
    z = np.asarray(z, np.float64)
    R = np.asarray(returns, np.float64).reshape(B)
    adv = R - v
    g_logp = -(1.0 / B) * adv
    g_v = vc * (2.0 / B) * (v - R)
    g_ls = None
    if kind == "cat":
        cat = O.categorical(z)
        a = np.asarray(actions).reshape(B).astype(np.int64)
        nl, p = cat["norm_logits"], cat["probs"]
        logp, ent = np.take_along_axis(nl, a[:, None], -1)[:, 0], cat["entropy"]
        onehot = np.zeros_like(p)
        onehot[np.arange(B), a] = 1.0
        g_z = g_logp[:, None] * (onehot - p) + (ec / B) * p * (nl + ent[:, None])
    elif kind == "gauss":
        s = np.asarray(logstd, np.float64).reshape(1, -1)
        a = np.asarray(actions, np.float64).reshape(z.shape)
        logp, ent = G.gauss_logp_entropy(z, s, a)
        ivar, d = np.exp(-2.0 * s), a - z
        g_z = g_logp[:, None] * d * ivar
        g_ls = (g_logp[:, None] * (d * d * ivar - 1.0)).sum(0) - ec
    else:
        a = np.asarray(actions, np.float64).reshape(z.shape)
        logp, ent = Bn.bern_logp_entropy(z, a)
        p = Bn._sigmoid(z)
        g_z = g_logp[:, None] * (a - p) + (ec / B) * z * p * Bn._sigmoid(-z)
    return dict(g_value=g_v, g_logits=g_z, g_logstd=g_ls, value_loss=(adv ** 2).mean(),
                action_loss=-(adv * logp).mean(), entropy=ent.mean(), logp=logp)


# ------------------------------------------------------------------ torch text
def torch_dist(kind, z, logstd=None):
    from a2c_ppo_acktr import distributions as D
    if kind == "cat":
        return D.FixedCategorical(logits=z)
    if kind == "gauss":
        return D.FixedNormal(z, logstd.view(1, -1).expand_as(z).exp())
    return D.FixedBernoulli(logits=z)


def torch_loss(kind, value, z, actions, returns, vc, ec, logstd=None, planted=None):
    """algo/a2c_acktr.py:45-51, 71-72 on torch tensors of any float dtype (value [B],
    z [B, A], returns [B]; actions int64 [B] or float [B, A]) -> (total, value_loss,
    action_loss, entropy).  planted: one of the errors the comparisons must reject —
    "half" (a 0.5 on the value loss), "attached" (the advantage not detached),
    "normalized" (advantages normalised as PPO does)."""
    dist = torch_dist(kind, z, logstd)
    logp = dist.log_probs(actions.view(-1, 1) if kind == "cat" else actions.view(z.shape))
    entropy = dist.entropy().mean()
    values = value.view(-1, 1)
    advantages = returns.view(-1, 1) - values
    value_loss = advantages.pow(2).mean()
    if planted == "half":
        value_loss = 0.5 * value_loss
    a_ = advantages if planted == "attached" else advantages.detach()
    if planted == "normalized":
        a_ = (a_ - a_.mean()) / (a_.std() + 1e-5)
    action_loss = -(a_ * logp).mean()
    return value_loss * vc + action_loss - entropy * ec, value_loss, action_loss, entropy


# --------------------------------------------------------------------- RMSprop
def rmsprop_step(p, sq, g, lr, alpha, eps, planted=None):
    """torch.optim.RMSprop (no momentum, not centered, no weight decay) in float64 ->
    (p, square_avg).  planted "swapped": alpha and 1 - alpha exchanged."""
    p, sq, g = (np.asarray(x, np.float64) for x in (p, sq, g))
    a, w = (1.0 - alpha, alpha) if planted == "swapped" else (alpha, 1.0 - alpha)
    sq = sq * a + w * g * g
    return p - lr * g / (np.sqrt(sq) + eps), sq


def clip_coef(total_norm, max_norm):
    """clip_grad_norm_'s coefficient; max_norm None or <= 0: no clipping"""
    if max_norm is None or max_norm <= 0:
        return 1.0
    return min(1.0, max_norm / (total_norm + 1e-6))


def check_rmsprop(got, ref, show=print):
    """(norm, clipped gradient, parameters, square_avg) of one clip + RMSprop step: total
    norm rtol 1e-6, clipped gradient rtol 1e-5 / atol 1e-9, parameters atol 1e-6 (the three
    bounds of test_clip_adam_golden), square_avg rtol 2e-6 (torch's own fp32 is 3.1e-7 from
    float64 after four steps)."""
    f = lambda x: np.asarray(x, np.float64)  # noqa: E731
    show("norm", float(got[0]), float(ref[0]))
    np.testing.assert_allclose(f(got[0]), f(ref[0]), rtol=1e-6)
    np.testing.assert_allclose(f(got[1]), f(ref[1]), rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(f(got[2]), f(ref[2]), rtol=0, atol=1e-6)
    np.testing.assert_allclose(f(got[3]), f(ref[3]), rtol=2e-6, atol=0)


# ----------------------------------------------------------------------- cases
GRAD_NAMES = C.GRAD_NAMES + ("g_logstd",)


@functools.lru_cache(maxsize=None)
def build_case(kind, H, A, B, rows, sep_v, feat_act):
    """fp32 inputs of one heads case with cat_ref.build_case's distributions (features
    uniform in [-1, 1]; wc scaled by 2 / sqrt(H), wa by 4 / sqrt(H); biases 0.1 N(0, 1);
    ret N(0, 1); rows "idx": B storage rows gathered from B + 16, else the row0 offset)
    and the float64 reference of what train kernel + reduce return.  Actions: uniform in
    [0, A) (cat), mean + sigma N(0, 1) with logstd = -0.5 + 0.2 N(0, 1) (gauss), uniform
    in {0, 1} (bern).  The storage planes hold only actions and ret.  Computed once per
    case, never modified."""
    seed = 1000 * H + 10 * A + B + 7 * KINDS.index(kind)
    g = np.random.default_rng(seed)
    f32 = lambda x: np.ascontiguousarray(x, np.float32)  # noqa: E731
    d = lambda x: x.astype(np.float64)  # noqa: E731
    c = C._forward(g, B, H, A, sep_v, 4.0)
    value, z = c["value"], c["z"]
    Rn = B + 16 if rows == "idx" else rows + B
    sr = (g.permutation(Rn)[:B] if rows == "idx" else rows + np.arange(B)).astype(np.int64)
    logstd = None
    if kind == "cat":
        act = np.zeros(Rn, np.int64)
        act[sr] = g.integers(0, A, B)
    elif kind == "gauss":
        logstd = f32(-0.5 + 0.2 * g.normal(size=A))
        act = np.zeros((Rn, A), np.float32)
        act[sr] = f32(z + np.exp(d(logstd)) * g.normal(size=(B, A)))
    else:
        act = np.zeros((Rn, A), np.float32)
        act[sr] = g.integers(0, 2, (B, A)).astype(np.float32)
    ret = f32(g.normal(size=Rn))
    c.update(kind=kind, sr=sr, actions=act, ret=ret, logstd=logstd, R=Rn, seed=seed, H=H, A=A, B=B, rows=rows,
             sep_v=sep_v, feat_act=feat_act)
    r = head_grads(kind, value, z, act[sr], ret[sr], VC, EC, logstd)
    ag = C._act_grad(feat_act)
    fv = c["feat_v"] if sep_v else c["feat"]
    dv = r["g_value"][:, None] * d(c["wc"])[None, :]
    dz = r["g_logits"] @ d(c["wa"])
    c["ref"] = {"dfeat": ag(dz if sep_v else dz + dv, d(c["feat"])),
                "dfeat_v": ag(dv, d(fv)) if sep_v else None,
                "g_wc": r["g_value"] @ d(fv), "g_bc": np.array([r["g_value"].sum()]),
                "g_wa": r["g_logits"].T @ d(c["feat"]), "g_ba": r["g_logits"].sum(0),
                "g_logstd": r["g_logstd"],
                "losses": np.array([r["value_loss"], r["action_loss"], r["entropy"]])}
    return c


def torch_head_grads(c, dtype=torch.float32, planted=None):
    """What the A2C train kernel + reduce compute for case c, by torch CPU autograd in
    `dtype` from the case's fp32 inputs and torch_loss: in fp32 the yardstick of the
    comparison, in float64 (with `planted`) a wrong implementation."""
    kind = c["kind"]
    t = lambda k: torch.from_numpy(c[k]).to(dtype)  # noqa: E731
    sr = torch.from_numpy(c["sr"])
    feat, wc, bc, wa, ba = (t(k).requires_grad_() for k in ("feat", "wc", "bc", "wa", "ba"))
    fv = t("feat_v").requires_grad_() if c["sep_v"] else feat
    ls = t("logstd").requires_grad_() if kind == "gauss" else None
    value = fv @ wc + bc[0]
    z = feat @ wa.T + ba
    actions = torch.from_numpy(c["actions"])[sr]
    actions = actions if kind == "cat" else actions.to(dtype)
    total, vl, al, ent = torch_loss(kind, value, z, actions, t("ret")[sr], VC, EC, ls, planted)
    total.backward()
    ag = C._act_grad(c["feat_act"])
    n = lambda x: x.detach().double().numpy()  # noqa: E731
    return {"dfeat": ag(n(feat.grad), n(feat)), "dfeat_v": ag(n(fv.grad), n(fv)) if c["sep_v"] else None,
            "g_wc": n(wc.grad), "g_bc": n(bc.grad), "g_wa": n(wa.grad), "g_ba": n(ba.grad),
            "g_logstd": n(ls.grad) if ls is not None else None,
            "losses": np.array([vl.item(), al.item(), ent.item()])}


# ---------------------------------------------------------------- whole update
def policy_forward(arch, P, obs, vec, h0, masks, relu=None):
    """float64 forward of a Policy over all T*N rows in storage order (row t*N + n), from
    its parameters P in policy.parameters() order (leaf tensors) -> (value [R], head [R, A]).
    arch: "cnn" (oracle.torch_ref.cnn_forward), "cnn_gru" (its trunk, cat vector obs,
    torch's gru_cell per step on h * mask as model.py:111-166 does, heads on h), "mlp"
    (tanh towers on cat(obs, vec)), "mlp_gru" (gru_cell, then the towers;
    mlp_rec_ref.MLPRecRef is the same model as a module, compared in test_a2c_cpu.py).
    obs: u8 images are decoded as u8 / 255.  masks [T, N]; h0 [N, H].  relu: the trunk's
    four ReLU decisions to apply instead of (pre-activation > 0), torch_ref.trunk's `masks`
    (helpers/relu_decisions.py: the engine's own, each checked to differ from float64's only
    within a rounding of 0)."""
    from oracle import torch_ref as TR
    F = torch.nn.functional
    x = obs.double() / 255.0 if obs.dtype == torch.uint8 else obs.double()
    if arch in ("cnn_gru", "mlp_gru"):
        gru, P = P[:4], P[4:]
    if arch in ("cnn", "cnn_gru"):
        trunkp, P = P[:8], P[8:]
        x = TR.trunk(trunkp, x, masks=relu)
    if vec is not None and vec.shape[-1] > 0:
        x = torch.cat([x, vec.double()], 1)
    if arch in ("cnn_gru", "mlp_gru"):
        T, N = masks.shape
        xs, h, outs = x.reshape(T, N, -1), h0.double(), []
        for t in range(T):
            h = torch.gru_cell(xs[t], h * masks[t].double().reshape(N, 1), *gru)
            outs.append(h)
        x = torch.cat(outs, 0)
    if arch in ("mlp", "mlp_gru"):
        tower = lambda q: torch.tanh(F.linear(torch.tanh(F.linear(x, q[0], q[1])), q[2], q[3]))  # noqa: E731
        fa, fc, P = tower(P[0:4]), tower(P[4:8]), P[8:]
    else:
        fa = fc = x
    return F.linear(fc, P[0], P[1])[:, 0], F.linear(fa, P[2], P[3])


def update_reference(arch, kind, params, obs, vec, h0, masks, actions, returns, vc, ec, max_norm, relu=None):
    """One A2C update in float64 by autograd of torch_loss over policy_forward: the
    gradients after clip_grad_norm_(max_norm) in policy.parameters() order (numpy), the
    three losses, the total norm and the clip coefficient.  params: the fp32 policy's
    parameters before the update; the planes are the storage's [:-1] rows flattened."""
    P = [p.detach().cpu().double().clone().requires_grad_() for p in params]
    value, z = policy_forward(arch, P, obs.cpu(), None if vec is None else vec.cpu(), h0.cpu(), masks.cpu(), relu)
    ls = P[-1] if kind == "gauss" else None
    a = actions.cpu()
    total, vl, al, ent = torch_loss(kind, value, z, a if kind == "cat" else a.double(), returns.cpu().double(), vc, ec,
                                    ls)
    grads = torch.autograd.grad(total, P)
    norm = float(torch.sqrt(sum((g * g).sum() for g in grads)))
    coef = clip_coef(norm, max_norm)
    return dict(grads=[g.numpy() * coef for g in grads], losses=np.array([vl.item(), al.item(), ent.item()]),
                norm=norm, coef=coef)


# ------------------------------------------------------------------ comparison
def check_grads(got, ref, show=print):
    """cat_ref.check_grads (1e-5 of the tensor's largest entry, floor 1e-8, per tensor)
    on the six tensors it knows, and the same rule on g_logstd where the reference has one."""
    seen = C.check_grads(got, ref, show)
    if ref.get("g_logstd") is not None:
        g = got["g_logstd"]
        g = g.detach().cpu().numpy() if isinstance(g, torch.Tensor) else np.asarray(g)
        r = ref["g_logstd"]
        err, bound = float(np.abs(g.astype(np.float64).reshape(r.shape) - r).max()), C.grad_bound(r)
        show(f"g_logstd: max err {err:.3e} bound {bound:.3e}")
        assert err <= bound, ("g_logstd", err, bound)
        seen["g_logstd"] = (err, bound)
    return seen


check_losses = C.check_losses


def check_update_losses(got, ref):
    """the three floats update() returns: test_full_iteration_replays_reference's bounds"""
    np.testing.assert_allclose(np.asarray(got, np.float64), np.asarray(ref, np.float64), rtol=1e-4, atol=1e-6)


def check_param_grads(got, ref, show=print):
    """{name: gradient}: the check_grads rule per parameter tensor"""
    for name, r in ref.items():
        r = np.asarray(r, np.float64)
        g = np.asarray(got[name], np.float64).reshape(r.shape)
        err, bound = float(np.abs(g - r).max()), C.grad_bound(r)
        show(f"{name}: max err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (name, err, bound)
