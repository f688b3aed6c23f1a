"""Float64 references for the GAIL discriminator (algo/gail.py, csrc/gail.hip).

closed_form(): the minibatch loss and its six gradient tensors, written out by hand — the
formulas the train kernel implements.  torch_loss(): the reference's loss (gail.py:30-56,
79-88) restated in torch for autograd; the CPU tests hold closed_form to it in float64.
adam_step(): torch.optim.Adam's default step in float64.  RunningMeanStd / returns_ref():
baselines' running moments and gail.py:104-111's recursion in float64, with the reward
being the logit d (the package's stated departure).

Bounds.  Gradients: cat_ref.grad_bound per tensor (1e-5 of its largest entry, floor
1e-8); fp32 torch autograd on the CPU is at most 2.5e-6 of the largest entry on the train
cases (b3 at (5, 100, 7), a cancelling sum; the other tensors at most 4.0e-7).  Loss sums: a2c_ref.check_update_losses (rtol 1e-4, atol 1e-6).  Rewards: 4x what
fp32 torch on the CPU differs from float64 on the same inputs (measure_reward_fp32(), the
T = 5, N = 7 and N = 1 cases of the GPU test, two consecutive rollouts, trunk 7-100-100-1;
the device's tanh and summation order differ from torch's by a few ulp).  Measured:
    logit d                 6.25e-8 absolute                     -> 2.5e-7
    returns                 1.86e-7 absolute                     -> 7.44e-7
    scaled reward           1.34e-6 absolute (values up to 2)    -> 5.36e-6
    mean                    1.23e-7 of max(|mean|, 1e-3)         -> 4.92e-7
    var                     2.33e-7 of max(|var|, 1e-3)          -> 9.32e-7
    count                   exact                                -> 0
"""
import functools

import numpy as np
import torch
import torch.nn as nn

from helpers import cat_ref as C

LAMBDA = 10.0
NAMES = ("W1", "b1", "W2", "b2", "w3", "b3")
PLANTS = ("const_s", "sum", "alpha_swapped", "no_pen")
REWARD_BOUNDS = {"d": 2.5e-7, "returns": 7.44e-7, "scaled": 5.36e-6, "mean": 4.92e-7, "var": 9.32e-7, "count": 0.0}


# ------------------------------------------------------------------ parameters
def num_params(D, Hd):
    return Hd * D + Hd * Hd + 3 * Hd + 1


def unpack(flat, D, Hd):
    """flat [P] in trunk.parameters() order -> {W1 [Hd, D], b1, W2 [Hd, Hd], b2, w3 [Hd], b3 [1]}"""
    flat = np.asarray(flat)
    out, off = {}, 0
    for name, shape in zip(NAMES, ((Hd, D), (Hd,), (Hd, Hd), (Hd,), (Hd,), (1,))):
        k = int(np.prod(shape))
        out[name] = flat[off:off + k].reshape(shape)
        off += k
    assert off == flat.size
    return out


def pack(p):
    return np.concatenate([np.asarray(p[n], np.float64).reshape(-1) for n in NAMES])


def make_trunk(D, Hd, seed, dtype=torch.float32):
    """the reference's construction under torch.manual_seed(seed); the caller's generator is kept"""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        trunk = nn.Sequential(nn.Linear(D, Hd), nn.Tanh(), nn.Linear(Hd, Hd), nn.Tanh(), nn.Linear(Hd, 1))
    return trunk.to(dtype)


def trunk_flat(trunk):
    return torch.cat([p.detach().reshape(-1) for p in trunk.parameters()]).cpu().numpy()


def set_trunk(trunk, flat):
    off = 0
    with torch.no_grad():
        for p in trunk.parameters():
            k = p.numel()
            p.copy_(torch.as_tensor(np.array(flat[off:off + k]).reshape(p.shape), dtype=p.dtype))
            off += k


# ----------------------------------------------------------------- closed form
def _softplus(z):
    return np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))


def _sigmoid(z):
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0, e) / (1.0 + e)


def forward(p, x):
    h1 = np.tanh(x @ p["W1"].T + p["b1"])
    h2 = np.tanh(h1 @ p["W2"].T + p["b2"])
    return h1, h2, h2 @ p["w3"] + p["b3"][0]


def closed_form(flat, D, Hd, x_e, x_p, alpha, lam=LAMBDA, plant=None):
    """-> {"sums": [sum BCE(d_e, 1), sum BCE(d_p, 0), sum (|g| - 1)^2], "loss": L, "grads":
    {name: float64 array}, "gnorm": |dd/dx(x_m)| per row}.  plant: one of PLANTS, a wrong
    variant the checks must reject."""
    p = {k: np.asarray(v, np.float64) for k, v in unpack(flat, D, Hd).items()}
    x_e, x_p = np.asarray(x_e, np.float64), np.asarray(x_p, np.float64)
    a = np.asarray(alpha, np.float64).reshape(-1, 1)
    B = x_e.shape[0]
    W1, W2, w3 = p["W1"], p["W2"], p["w3"]
    G = {k: np.zeros_like(v) for k, v in p.items()}

    def plain(x, h1, h2, c, hb1, hb2):
        s1, s2 = 1 - h1 * h1, 1 - h2 * h2
        p2 = (c[:, None] * w3 + hb2) * s2
        p1 = (p2 @ W2 + hb1) * s1
        G["W1"] += p1.T @ x
        G["b1"] += p1.sum(0)
        G["W2"] += p2.T @ h1
        G["b2"] += p2.sum(0)
        G["w3"] += c @ h2
        G["b3"] += c.sum()

    h1, h2, d_e = forward(p, x_e)
    plain(x_e, h1, h2, -_sigmoid(-d_e) / B, 0.0, 0.0)
    h1, h2, d_p = forward(p, x_p)
    plain(x_p, h1, h2, _sigmoid(d_p) / B, 0.0, 0.0)

    x_m = (1 - a) * x_e + a * x_p if plant == "alpha_swapped" else a * x_e + (1 - a) * x_p
    h1, h2, _ = forward(p, x_m)
    s1, s2 = 1 - h1 * h1, 1 - h2 * h2
    u2 = s2 * w3
    v1 = u2 @ W2
    u1 = s1 * v1
    g = u1 @ W1
    n = np.sqrt((g * g).sum(1))
    scale = {"sum": lam * 2.0, "no_pen": 0.0}.get(plant, lam * 2.0 / B)
    gbar = (scale * (n - 1) / n)[:, None] * g
    G["W1"] += u1.T @ gbar
    ub1 = gbar @ W1.T
    vb1 = s1 * ub1
    G["W2"] += u2.T @ vb1
    ub2 = vb1 @ W2.T
    G["w3"] += (s2 * ub2).sum(0)
    hb1, hb2 = -2 * h1 * v1 * ub1, -2 * h2 * w3 * ub2
    if plant == "const_s":
        hb1, hb2 = 0.0 * hb1, 0.0 * hb2
    plain(x_m, h1, h2, np.zeros(B), hb1, hb2)

    sums = np.array([_softplus(-d_e).sum(), _softplus(d_p).sum(), ((n - 1) ** 2).sum()])
    pen = {"sum": lam * sums[2], "no_pen": 0.0}.get(plant, lam * sums[2] / B)
    return {"sums": sums, "loss": (sums[0] + sums[1]) / B + pen, "grads": G, "gnorm": n}


def torch_loss(trunk, x_e, x_p, alpha, lam=LAMBDA):
    """gail.py:69-88 with compute_grad_pen's alpha passed in: BCE-with-logits of the expert
    rows against 1 and the policy rows against 0, plus lam mean (|dd/dx(x_m)|_2 - 1)^2.
    Any dtype; differentiable in the trunk's parameters (create_graph)."""
    F = torch.nn.functional
    d_p, d_e = trunk(x_p), trunk(x_e)
    gail_loss = (F.binary_cross_entropy_with_logits(d_e, torch.ones_like(d_e)) +
                 F.binary_cross_entropy_with_logits(d_p, torch.zeros_like(d_p)))
    a = alpha.reshape(-1, 1).expand_as(x_e)
    mix = (a * x_e + (1 - a) * x_p).detach().requires_grad_(True)
    disc = trunk(mix)
    grad, = torch.autograd.grad(disc, mix, torch.ones_like(disc), create_graph=True, retain_graph=True)
    return gail_loss + lam * (grad.norm(2, dim=1) - 1).pow(2).mean()


def autograd_grads(flat, D, Hd, x_e, x_p, alpha, dtype=torch.float64, lam=LAMBDA):
    """(loss, {name: gradient}) of torch_loss by torch autograd in `dtype`"""
    trunk = make_trunk(D, Hd, 0, dtype)
    set_trunk(trunk, flat)
    t = lambda v: torch.as_tensor(np.array(v), dtype=dtype)   # noqa: E731
    loss = torch_loss(trunk, t(x_e), t(x_p), t(alpha), lam)
    grads = torch.autograd.grad(loss, list(trunk.parameters()))
    return float(loss.detach()), {n: g.numpy().astype(np.float64).reshape(s.shape) for n, g, s in
                         zip(NAMES, grads, unpack(np.zeros(num_params(D, Hd)), D, Hd).values())}


def check_grads(got, ref, show=print):
    """{name: gradient} against the float64 reference: cat_ref.grad_bound per tensor"""
    worst = {}
    for name in NAMES:
        r = np.asarray(ref[name], np.float64)
        g = np.asarray(got[name], np.float64).reshape(r.shape)
        err, bound = float(np.abs(g - r).max()), C.grad_bound(r)
        show(f"{name}: max err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (name, err, bound)   # NaN compares false
        worst[name] = (err, bound)
    return worst


# ------------------------------------------------------------------------ Adam
def adam_step(p, g, m, v, step, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam defaults, float64, step counted from 1 -> (p, m, v)"""
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    den = np.sqrt(v) / np.sqrt(1 - b2 ** step) + eps
    return p - (lr / (1 - b1 ** step)) * m / den, m, v


# --------------------------------------------------------------------- rewards
class RunningMeanStd(object):
    """baselines.common.running_mean_std.RunningMeanStd(shape=()) in float64"""

    def __init__(self):
        self.mean, self.var, self.count = 0.0, 1.0, 1e-4

    def update(self, x):
        x = np.asarray(x, np.float64).reshape(-1)
        bmean, bvar, bcount = float(x.mean()), float(x.var()), float(x.size)
        delta = bmean - self.mean
        tot = self.count + bcount
        new_mean = self.mean + delta * bcount / tot
        m2 = self.var * self.count + bvar * bcount + delta * delta * self.count * bcount / tot
        self.mean, self.var, self.count = new_mean, m2 / tot, tot


def returns_ref(d, masks, gamma, returns=None, rms=None, update_rms=True):
    """gail.py:104-111 over T steps in float64 with reward = d: d, masks [T, N] ->
    (scaled [T, N], returns [N], rms).  returns None: the first call (returns = d[0])."""
    d, masks = np.asarray(d, np.float64), np.asarray(masks, np.float64)
    rms = RunningMeanStd() if rms is None else rms
    out = np.empty_like(d)
    for t in range(d.shape[0]):
        if returns is None:
            returns = d[t].copy()
        if update_rms:
            returns = returns * masks[t] * float(np.float32(gamma)) + d[t]
            rms.update(returns)
        out[t] = d[t] / np.sqrt(rms.var + 1e-8)
    return out, returns, rms


def returns_fp32(trunk, x, masks, gamma, returns, rms):
    """the same in fp32 torch as gail.py writes it (reward = d, numpy float32 batch
    moments): the yardstick measure_reward_fp32 holds against float64"""
    T = x.shape[0]
    ds, out = [], []
    with torch.no_grad():
        for t in range(T):
            d = trunk(torch.as_tensor(np.array(x[t])))
            if returns is None:
                returns = d.clone()
            returns = returns * torch.as_tensor(np.array(masks[t])).view(-1, 1) * gamma + d
            rms.update(returns.numpy())
            ds.append(d.numpy().reshape(-1))
            out.append((d / np.sqrt(rms.var + 1e-8)).numpy().reshape(-1))
    return np.stack(ds), np.stack(out), returns, rms


class _RMS32(RunningMeanStd):
    def update(self, x):
        x = np.asarray(x)
        bmean, bvar, bcount = np.mean(x, axis=0), np.var(x, axis=0), x.shape[0]
        bmean, bvar = float(np.asarray(bmean).reshape(-1)[0]), float(np.asarray(bvar).reshape(-1)[0])
        delta = bmean - self.mean
        tot = self.count + bcount
        new_mean = self.mean + delta * bcount / tot
        m2 = self.var * self.count + bvar * bcount + delta * delta * self.count * bcount / tot
        self.mean, self.var, self.count = new_mean, m2 / tot, tot


@functools.lru_cache(maxsize=None)
def reward_case(N, T=5, obs_dim=5, A=2, Hd=100, rollouts=2):
    """inputs of the reward tests: trunk (obs_dim + A)-Hd-Hd-1 from its seed, `rollouts`
    consecutive rollouts x [T, N, D] ~ N(0, 1), masks [T, N] with zeros in two lanes (one
    when N == 1), and the float64 reference of each rollout: (d, scaled, returns after,
    (mean, var, count) after).  gamma = 0.99."""
    D = obs_dim + A
    g = np.random.default_rng(1000 + N)
    trunk = make_trunk(D, Hd, 77 + N)
    flat = trunk_flat(trunk)
    p = {k: np.asarray(v, np.float64) for k, v in unpack(flat, D, Hd).items()}
    xs, ms, refs = [], [], []
    returns, rms = None, RunningMeanStd()
    for k in range(rollouts):
        x = g.normal(size=(T, N, D)).astype(np.float32)
        m = np.ones((T, N), np.float32)
        m[1 + k, 0] = 0.0
        m[3, N - 1] = 0.0
        d = np.stack([forward(p, x[t].astype(np.float64))[2] for t in range(T)])
        scaled, returns, rms = returns_ref(d, m, 0.99, returns, rms)
        xs.append(x), ms.append(m)
        refs.append((d, scaled, returns.copy(), (rms.mean, rms.var, rms.count)))
    return {"D": D, "Hd": Hd, "obs_dim": obs_dim, "A": A, "T": T, "N": N, "gamma": 0.99, "flat": flat, "x": xs,
            "masks": ms, "ref": refs}


def measure_reward_fp32(show=print):
    """what fp32 torch on the CPU differs from returns_ref by, over reward_case(7) and
    reward_case(1): the figures in this module's docstring"""
    worst = {k: 0.0 for k in REWARD_BOUNDS}
    rel = lambda a, b: abs(a - b) / max(abs(b), 1e-3)   # noqa: E731
    for N in (7, 1):
        c = reward_case(N)
        trunk = make_trunk(c["D"], c["Hd"], 77 + N)
        returns, rms = None, _RMS32()
        for x, m, (d, scaled, ret, (mean, var, count)) in zip(c["x"], c["masks"], c["ref"]):
            d32, s32, returns, rms = returns_fp32(trunk, x, m, c["gamma"], returns, rms)
            worst["d"] = max(worst["d"], float(np.abs(d32 - d).max()))
            worst["scaled"] = max(worst["scaled"], float(np.abs(s32 - scaled).max()))
            worst["returns"] = max(worst["returns"], float(np.abs(returns.numpy().reshape(-1) - ret).max()))
            worst["mean"] = max(worst["mean"], rel(rms.mean, mean))
            worst["var"] = max(worst["var"], rel(rms.var, var))
            worst["count"] = max(worst["count"], abs(rms.count - count))
    show(worst)
    return worst


def check_rewards(got, ref, show=print):
    """(d, scaled, returns, (mean, var, count)) of one rollout against reward_case's"""
    d, scaled, ret, (mean, var, count) = ref
    f = lambda v: np.asarray(v, np.float64).reshape(-1)   # noqa: E731
    errs = {"d": np.abs(f(got[0]) - f(d)).max(), "scaled": np.abs(f(got[1]) - f(scaled)).max(),
            "returns": np.abs(f(got[2]) - f(ret)).max(),
            "mean": abs(got[3][0] - mean) / max(abs(mean), 1e-3), "var": abs(got[3][1] - var) / max(abs(var), 1e-3),
            "count": abs(got[3][2] - count)}
    for k, e in errs.items():
        show(f"{k}: err {float(e):.3e} bound {REWARD_BOUNDS[k]:.3e}")
    for k, e in errs.items():
        assert float(e) <= REWARD_BOUNDS[k], (k, float(e), REWARD_BOUNDS[k])


# ----------------------------------------------------------------------- cases
TRAIN_CASES = ((3, 4, 1, "row0"), (5, 100, 7, "row0"), (14, 100, 33, "idx"), (23, 100, 128, "row0"))


@functools.lru_cache(maxsize=None)
def build_case(D, Hd, B, rows):
    """One train case: default nn.Linear init from a seed derived from the shape, x_e ~
    N(0, 1), x_p ~ N(0.3, 1), alpha ~ U[0, 1), all fp32.  The policy rows live in storage
    planes of B + 16 rows split into obs [., D - V - A], vector_obs [., V] and actions
    [., A] (A = 1 below D = 5, else 2; V = 3 when rows == "idx", else 0): gathered by a
    permutation's first B entries when rows == "idx", else rows 5 .. 5 + B.  Holds the
    float64 closed_form reference.  The first seed is used; min |g_b| >= 0.01 is asserted
    (the norm is singular at 0), no row is left out of any comparison.  Never modified."""
    seed = 100000 * D + 1000 * Hd + B
    g = np.random.default_rng(seed)
    flat = trunk_flat(make_trunk(D, Hd, seed))
    A = 1 if D < 5 else 2
    V = 3 if rows == "idx" else 0
    od = D - V - A
    R = B + 16
    plane = (0.3 + g.normal(size=(R, D))).astype(np.float32)
    x_e = g.normal(size=(B, D)).astype(np.float32)
    alpha = g.random(size=B).astype(np.float32)
    idx = g.permutation(R)[:B].astype(np.int64) if rows == "idx" else None
    row0 = 0 if rows == "idx" else 5
    x_p = plane[idx] if idx is not None else plane[row0:row0 + B]
    ref = closed_form(flat, D, Hd, x_e, x_p, alpha)
    assert ref["gnorm"].min() >= 0.01, ref["gnorm"].min()
    case = {"D": D, "Hd": Hd, "B": B, "R": R, "od": od, "V": V, "A": A, "flat": flat, "x_e": x_e, "x_p": x_p,
            "alpha": alpha, "idx": idx, "row0": row0, "obs": np.ascontiguousarray(plane[:, :od]),
            "vec": np.ascontiguousarray(plane[:, od:od + V]), "act": np.ascontiguousarray(plane[:, od + V:]),
            "ref": ref}
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return case


# ---------------------------------------------------------------------- update
def reference_update(flat, D, Hd, expert_loader, obs, vec, act, mini_batch_size, obsfilt=None, lr=1e-3):
    """gail.py:58-96's loop in float64, with state = (obs | vector_obs) and action = the
    stored action: zip(expert_loader, policy minibatches cut from one torch.randperm(T N)),
    one torch.rand(B, 1) per pair, the loss by autograd of torch_loss, Adam by adam_step.
    obs / vec / act: [T N, .] float arrays (the first T steps of the planes).  Draws on the
    default CPU generator exactly as the reference's loop does.  -> (flat after, mean loss,
    [per-pair (x_e, x_p, alpha)])."""
    planes = np.concatenate([np.asarray(a, np.float64) for a in (obs, vec, act) if a.shape[1]], axis=1)
    batch_size = planes.shape[0]

    def policy_batches():
        perm = torch.randperm(batch_size).numpy()
        for start in range(0, batch_size - mini_batch_size + 1, mini_batch_size):
            yield planes[perm[start:start + mini_batch_size]]

    p = np.asarray(flat, np.float64).copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    loss, n, pairs = 0.0, 0, []
    for (e_state, e_action), x_p in zip(expert_loader, policy_batches()):
        e_state = e_state.numpy()
        if obsfilt is not None:
            e_state = obsfilt(e_state, update=False)
        x_e = np.concatenate([np.asarray(e_state, np.float32), e_action.numpy()], axis=1).astype(np.float64)
        alpha = torch.rand(x_e.shape[0], 1).numpy().reshape(-1)
        L, grads = autograd_grads(p, D, Hd, x_e, x_p, alpha)
        loss += L
        n += 1
        p, m, v = adam_step(p, pack(grads), m, v, n, lr=lr)
        pairs.append((x_e, x_p, alpha))
    return p, loss / n, pairs
