"""float64 reference of the Categorical loss head (distributions.py:17-27, 54-68,
algo/ppo.py:61-81), the inputs of tests/test_heads_gpu.py and the comparison it uses.

The reference wraps oracle/ppo_oracle.categorical and loss_head_grads (pinned to the
reference by test_oracle_golden.py; test_heads_cpu.py checks them against torch
float64 autograd once more, at A = 1 and A = 16 and for both value losses).

A branch of the loss that flips between float64 and fp32 (the ratio clamp, the value
clamp, max(l1, l2), an argmax) moves a gradient by a whole row's term, so the case
builder measures, in float64, how far every row of a case is from each branch point
and steps its seed until all of them are at least MARGIN away.  The condition is on
the inputs alone and no row is ever left out of a comparison.
"""
import functools
import math

import numpy as np
import torch

from oracle import ppo_oracle as O

CLIP, VC, EC = 0.1, 0.5, 0.01
MARGIN = 2e-5
MAX_SEEDS = 16

# H, A, B, rows ("idx": gathered storage rows, or the row0 offset), separate critic
# features, activation of the features (0 none, 1 ReLU, 2 tanh), use_clipped_value_loss
CASES = [
    (64, 1, 1, 0, False, 0, True),          # single row; A = 1: p = 1, entropy 0, logit gradient 0
    (64, 3, 37, "idx", False, 1, True),     # partial second wave, two empty waves, A < AMAX
    (64, 8, 129, 5, False, 1, False),       # FAST HC = 1; crosses the 128-rows-per-block boundary; unclipped
    (100, 8, 129, 5, False, 2, True),       # H not a multiple of 64 (HC = 2, lane bound), tanh
    (128, 6, 37, "idx", True, 2, True),     # separate critic features and dfeat_v (MLPBase)
    (256, 8, 130, "idx", False, 0, True),   # FAST HC = 4, no activation (the GRU policy's shape)
    (320, 11, 200, "idx", False, 1, True),  # hc_of(320) = 8 with H < 512; AMAX = 16 generic
    (512, 8, 130, "idx", False, 1, True),   # LDS-weight kernel, two blocks
    (512, 8, 300, "idx", False, 1, False),  # LDS-weight kernel, unclipped value loss
    (512, 9, 300, "idx", False, 1, True),   # the A = 8 -> 9 switch to AMAX = 16
    (512, 16, 300, 11, False, 0, True),     # FAST AMAX = 16, HC = 8: the largest instantiation; row0 offset
    (256, 16, 128, "idx", True, 2, False),  # AMAX = 16 with separate critic features; one block; unclipped
]
LDS_CASES = [c for c in CASES if c[:2] == (512, 8)]


def case_id(case):
    return "-".join(str(int(x) if isinstance(x, bool) else x) for x in case)


# ------------------------------------------------------------------ reference
def cat_logp_entropy(logits, actions):
    """log-prob of the given actions and entropy per row of FixedCategorical(logits)"""
    cat = O.categorical(logits)
    a = np.asarray(actions).reshape(-1).astype(np.int64)
    return np.take_along_axis(cat["norm_logits"], a[:, None], -1)[:, 0], cat["entropy"]


def cat_loss_head_grads(value, logits, actions, old_logp, adv, vpred, ret, clip, vc, ec, use_clipped):
    """g_value [B], g_logits [B, A], value_loss, action_loss, entropy (and logp) of
    value_loss * vc + action_loss - entropy * ec, with autograd's tie conventions"""
    return O.loss_head_grads(np.asarray(value, np.float64), np.asarray(logits, np.float64), actions, old_logp, adv,
                             vpred, ret, clip, vc, ec, use_clipped_value_loss=bool(use_clipped))


def torch_loss(value, logits, actions, old_logp, adv, vpred, ret, clip, vc, ec, use_clipped):
    """The reference's loss (algo/ppo.py:61-81 with FixedCategorical) on torch tensors
    of any float dtype: (total, value_loss, action_loss, entropy, log-probs [B])."""
    from a2c_ppo_acktr.distributions import FixedCategorical
    dist = FixedCategorical(logits=logits)
    logp = dist.log_probs(actions.view(-1, 1))
    entropy = dist.entropy().mean()
    ratio = torch.exp(logp - old_logp.view(-1, 1))
    a_ = adv.view(-1, 1)
    action_loss = -torch.min(ratio * a_, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * a_).mean()
    values, vp, R = value.view(-1, 1), vpred.view(-1, 1), ret.view(-1, 1)
    if use_clipped:
        vpc = vp + (values - vp).clamp(-clip, clip)
        value_loss = 0.5 * torch.max((values - R).pow(2), (vpc - R).pow(2)).mean()
    else:
        value_loss = 0.5 * (R - values).pow(2).mean()
    return value_loss * vc + action_loss - entropy * ec, value_loss, action_loss, entropy, logp[:, 0]


def _act_grad(feat_act):
    return (lambda dd, y: dd) if feat_act == 0 else (lambda dd, y: dd * (y > 0)) if feat_act == 1 else \
        (lambda dd, y: dd * (1 - y * y))


GRAD_NAMES = ("dfeat", "dfeat_v", "g_wc", "g_bc", "g_wa", "g_ba")


def torch_head_grads(c, dtype=torch.float32, ec=EC, use_clipped=None):
    """What the train kernel + reduce compute for case c, by torch CPU autograd in
    `dtype` from the case's fp32 inputs: the fp32 yardstick of the comparison (and,
    with another ec or the other value loss, a planted error).  dfeat is autograd's
    gradient of the features times the activation's derivative, as in the kernel."""
    use_clipped = c["use_clipped"] if use_clipped is None else use_clipped
    t = lambda k: torch.from_numpy(c[k]).to(dtype)  # noqa: E731
    sr = torch.from_numpy(c["sr"])
    feat, wc, bc, wa, ba = (t(k).requires_grad_() for k in ("feat", "wc", "bc", "wa", "ba"))
    fv = t("feat_v").requires_grad_() if c["sep_v"] else feat
    value = fv @ wc + bc[0]
    logits = feat @ wa.T + ba
    p = lambda k: t(k)[sr]  # noqa: E731
    total, vl, al, ent, _ = torch_loss(value, logits, torch.from_numpy(c["actions"])[sr], p("old_logp"), p("adv"),
                                       p("vpred"), p("ret"), CLIP, VC, ec, use_clipped)
    total.backward()
    ag = _act_grad(c["feat_act"])
    n = lambda x: x.detach().double().numpy()  # noqa: E731
    return {"dfeat": ag(n(feat.grad), n(feat)), "dfeat_v": ag(n(fv.grad), n(fv)) if c["sep_v"] else None,
            "g_wc": n(wc.grad), "g_bc": n(bc.grad), "g_wa": n(wa.grad), "g_ba": n(ba.grad),
            "losses": np.array([vl.item(), al.item(), ent.item()])}


# ----------------------------------------------------------------- comparison
def grad_bound(ref):
    """test_mlp_minibatch_grads_vs_oracle's rule: 1e-5 of the tensor's largest entry"""
    return 1e-5 * max(float(np.abs(ref).max()), 1e-3)


def check_grads(got, ref, show=print):
    """Every gradient tensor of ref (dfeat, dfeat_v, g_wc, g_bc, g_wa, g_ba) against
    got: max |err| <= 1e-5 * max(max|ref|, 1e-3) per tensor; a NaN in got fails.
    Returns {name: (err, bound)}."""
    seen = {}
    for name in GRAD_NAMES:
        r = ref[name]
        if r is None:
            continue
        g = got[name]
        g = g.detach().cpu().numpy() if isinstance(g, torch.Tensor) else np.asarray(g)
        assert g.shape == r.shape, (name, g.shape, r.shape)
        err = float(np.abs(g.astype(np.float64) - r).max())
        bound = grad_bound(r)
        show(f"{name}: max err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (name, err, bound)   # NaN compares false
        seen[name] = (err, bound)
    return seen


def check_losses(got, ref):
    np.testing.assert_allclose(np.asarray(got, np.float64)[:3], ref, rtol=2e-5, atol=1e-6)


# ---------------------------------------------------------------------- cases
def _top2(x):
    s = np.sort(x, -1)
    return s[:, -1], s[:, -2]


def _forward(g, B, H, A, sep_v, zscale):
    """features, head parameters, Exp(1) noise (fp32) and the float64 forward"""
    f32 = lambda x: np.ascontiguousarray(x, np.float32)  # noqa: E731
    d = lambda x: x.astype(np.float64)  # noqa: E731
    c = {"feat": f32(g.uniform(-1, 1, (B, H)))}
    c["feat_v"] = f32(g.uniform(-1, 1, (B, H))) if sep_v else None
    c["wc"] = f32(g.uniform(-1, 1, H) * 2 / math.sqrt(H))
    c["bc"] = f32(g.normal(size=1) * 0.1)
    c["wa"] = f32(g.uniform(-1, 1, (A, H)) * zscale / math.sqrt(H))
    c["ba"] = f32(g.normal(size=A) * 0.1)
    c["noise"] = f32(g.exponential(size=(B, A)))
    fv = c["feat_v"] if sep_v else c["feat"]
    value = d(fv) @ d(c["wc"]) + d(c["bc"])[0]
    z = d(c["feat"]) @ d(c["wa"]).T + d(c["ba"])
    cat = O.categorical(z)
    m = {}
    if A >= 2:
        s1, s2 = _top2(cat["probs"] / d(c["noise"]))
        m["sample"] = float(((s1 - s2) / s1).min())
        p1, p2 = _top2(cat["probs"])
        m["mode"] = float((p1 - p2).min())
    c.update(value=value, z=z, cat=cat, zmax=float(np.abs(z).max()), margins=m)
    return c


def _fp32_yardstick(c, actions, logp):
    """torch's own CPU fp32 FixedCategorical.log_probs on these inputs against float64"""
    from a2c_ppo_acktr.distributions import FixedCategorical
    t = torch.from_numpy
    dist = FixedCategorical(logits=t(c["feat"]) @ t(c["wa"]).T + t(c["ba"]))
    lp32 = dist.log_probs(t(np.asarray(actions, np.int64)).view(-1, 1))[:, 0].numpy()
    return float(np.abs(lp32 - logp).max())


def _draw(seed, H, A, B, rows, sep_v, feat_act, use_clipped, zscale):
    g = np.random.default_rng(seed)
    f32 = lambda x: np.ascontiguousarray(x, np.float32)  # noqa: E731
    d = lambda x: x.astype(np.float64)  # noqa: E731
    c = _forward(g, B, H, A, sep_v, zscale)
    value, z = c["value"], c["z"]
    Rn = B + 16 if rows == "idx" else rows + B          # storage rows
    sr = g.permutation(Rn)[:B] if rows == "idx" else rows + np.arange(B)
    c["sr"] = sr.astype(np.int64)
    act = np.zeros(Rn, np.int64)
    act[sr] = g.integers(0, A, B)
    lp, ent = cat_logp_entropy(z, act[sr])
    planes = {k: f32(g.normal(size=Rn)) for k in ("adv", "ret")}
    planes["old_logp"] = np.zeros(Rn, np.float32)
    planes["old_logp"][sr] = f32(lp + g.normal(size=B) * 0.15)
    planes["vpred"] = np.zeros(Rn, np.float32)
    planes["vpred"][sr] = f32(value + g.normal(size=B) * 0.2)
    c.update(planes, actions=act, R=Rn, seed=seed, H=H, A=A, B=B, rows=rows, sep_v=sep_v, feat_act=feat_act,
             use_clipped=use_clipped)
    # distance of every row from each branch point, float64
    m = c["margins"]
    ratio = np.exp(lp - d(planes["old_logp"][sr]))
    m["ratio"] = float(np.minimum(np.abs(ratio - (1 - CLIP)), np.abs(ratio - (1 + CLIP))).min())
    if use_clipped:
        vo, R = d(planes["vpred"][sr]), d(planes["ret"][sr])
        dv = value - vo
        m["vclip"] = float(np.abs(np.abs(dv) - CLIP).min())
        l1, l2 = (value - R) ** 2, (vo + np.clip(dv, -CLIP, CLIP) - R) ** 2
        out = np.abs(dv) > CLIP
        m["vmax"] = float((np.abs(l1 - l2) / np.maximum(1.0, l1))[out].min()) if out.any() else math.inf
    c["logp"], c["ent"] = lp, ent
    return c


@functools.lru_cache(maxsize=None)
def build_case(H, A, B, rows, sep_v, feat_act, use_clipped, zscale=4.0):
    """fp32 inputs of one case (features uniform in [-1, 1]; wc scaled by 2 / sqrt(H),
    wa by zscale / sqrt(H): |z| <~ zscale; biases 0.1 N(0, 1); actions uniform in
    [0, A); old_logp = float64 log-prob + 0.15 N; vpred = value + 0.2 N; adv and ret
    N(0, 1); Exp(1) noise [B, A]) and the float64 reference of everything the kernels
    return, computed from those same fp32 values.  The seed starts at 1000 H + 10 A +
    B and steps until every margin is >= MARGIN (at most MAX_SEEDS seeds).  The
    sample / mode margins are required at the default zscale only: the saturated
    inputs are not used for sampling.  Computed once per case, never modified."""
    base = 1000 * H + 10 * A + B + (int(zscale) if zscale != 4.0 else 0)
    tried = []
    for seed in range(base, base + MAX_SEEDS):
        c = _draw(seed, H, A, B, rows, sep_v, feat_act, use_clipped, zscale)
        need = {k: v for k, v in c["margins"].items() if zscale == 4.0 or k not in ("sample", "mode")}
        if all(v >= MARGIN for v in need.values()):
            break
        tried.append((seed, need))
    else:
        raise RuntimeError(f"no seed in {base}..{base + MAX_SEEDS - 1} meets the margins: {tried}")
    c["seeds_tried"] = len(tried) + 1
    d = lambda x: x.astype(np.float64)  # noqa: E731
    sr, cat, value = c["sr"], c["cat"], c["value"]
    r = cat_loss_head_grads(value, c["z"], c["actions"][sr], c["old_logp"][sr], c["adv"][sr], c["vpred"][sr],
                            c["ret"][sr], CLIP, VC, EC, use_clipped)
    ag = _act_grad(feat_act)
    fv = c["feat_v"] if sep_v else c["feat"]
    dv = r["g_value"][:, None] * d(c["wc"])[None, :]
    dz = r["g_logits"] @ d(c["wa"])
    c["ref"] = {"value": value, "logp": c["logp"], "entropy": c["ent"],
                "sample": (cat["probs"] / d(c["noise"])).argmax(-1), "mode": cat["probs"].argmax(-1),
                "dfeat": ag(dz if sep_v else dz + dv, d(c["feat"])),
                "dfeat_v": ag(dv, d(fv)) if sep_v else None,
                "g_wc": r["g_value"] @ d(fv), "g_bc": np.array([r["g_value"].sum()]),
                "g_wa": r["g_logits"].T @ d(c["feat"]), "g_ba": r["g_logits"].sum(0),
                "losses": np.array([r["value_loss"], r["action_loss"], r["entropy"]])}
    c["torch_fp32_err"] = _fp32_yardstick(c, c["actions"][sr], c["logp"])
    return c


@functools.lru_cache(maxsize=None)
def build_act_case(N, H, A):
    """Forward-only inputs for the act kernel at N rows (same distributions as
    build_case, the same seed rule on the sample / mode margins) with random given
    actions and their float64 log-probs."""
    base = 1000 * H + 10 * A + N
    for seed in range(base, base + MAX_SEEDS):
        g = np.random.default_rng(seed)
        c = _forward(g, N, H, A, False, 4.0)
        if all(v >= MARGIN for v in c["margins"].values()):
            break
    else:
        raise RuntimeError(f"no seed in {base}..{base + MAX_SEEDS - 1} meets the sample / mode margins")
    c["seed"] = seed
    given = g.integers(0, A, N).astype(np.int64)
    lp, ent = cat_logp_entropy(c["z"], given)
    cat = c["cat"]
    c["given"] = given
    c["ref"] = {"value": c["value"], "logp": lp, "entropy": ent,
                "sample": (cat["probs"] / c["noise"].astype(np.float64)).argmax(-1), "mode": cat["probs"].argmax(-1)}
    c["torch_fp32_err"] = _fp32_yardstick(c, given, lp)
    return c
