"""Box action spaces on the HIP engine: the DiagGaussian heads kernels through the
C ABI against float64 (tests/helpers/gauss_ref.py), sampling, and the public API
(Policy / PPO / RolloutStorage / GraphedActor / checkpoints) against the
reference's records gauss.npz and gauss_update.npz."""
import functools
import math

import numpy as np
import pytest
import torch

from conftest import golden
from helpers import gauss_ref as G
from oracle import ppo_oracle as O

pytestmark = pytest.mark.gpu

CLIP, VC, EC = 0.1, 0.5, 0.01


def _hip():
    from a2c_ppo_acktr import _hip
    return _hip


def _s():
    return torch.cuda.current_stream().cuda_stream


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def _load_flat(pol, flat):
    with torch.no_grad():
        flat, off = torch.from_numpy(np.ascontiguousarray(flat, np.float32)), 0
        for p in pol.parameters():
            p.copy_(flat[off:off + p.numel()].view_as(p))
            off += p.numel()
        assert off == flat.numel()


# ------------------------------------------------------------ kernels, direct
# H, A, B, rows ("idx": gathered storage rows, or the row0 offset), separate critic
# features, activation of the features (0 none, 1 ReLU, 2 tanh)
KERNEL_CASES = [
    (64, 1, 1, 0, False, 0),         # single row
    (64, 3, 37, "idx", False, 1),    # partial wave of rows
    (100, 8, 129, 5, False, 2),      # generic non-FAST path; crosses the 128-rows-per-block boundary
    (512, 9, 300, "idx", False, 1),  # AMAX = 16 at the A = 8 -> 9 switch, HC = 8, gathered rows
    (512, 9, 300, 11, False, 0),     # the same with a row0 offset
    (128, 16, 37, "idx", True, 2),   # separate feat_v / dfeat_v (MLPBase)
    (512, 8, 130, "idx", False, 1),  # the LDS-weight kernel (H = 512, A = 8), two blocks
]


@functools.lru_cache(maxsize=None)
def _kernel_case(H, A, B, rows, sep_v, feat_act, use_clipped=True):
    """fp32 inputs (random features in [-1, 1], weights scaled so |mu| <~ 2, logstd in
    [-1, 0.5], actions within 3 sigma of the mean) and the float64 reference computed
    from those same fp32 values; computed once per case, never modified."""
    g = np.random.default_rng(1000 * H + 10 * A + B)
    f32 = lambda x: np.ascontiguousarray(x, np.float32)  # noqa: E731
    c = {"feat": f32(g.uniform(-1, 1, (B, H)))}
    c["feat_v"] = f32(g.uniform(-1, 1, (B, H))) if sep_v else None
    c["wc"] = f32(g.uniform(-1, 1, H) * 2 / math.sqrt(H))
    c["bc"] = f32(g.normal(size=1) * 0.1)
    c["wa"] = f32(g.uniform(-1, 1, (A, H)) * 2 / math.sqrt(H))
    c["ba"] = f32(g.normal(size=A) * 0.1)
    c["logstd"] = f32(g.uniform(-1.0, 0.5, A))
    R = B + 16 if rows == "idx" else rows + B          # storage rows
    sr = g.permutation(R)[:B] if rows == "idx" else rows + np.arange(B)
    c["sr"] = sr.astype(np.int64)
    d = lambda x: x.astype(np.float64)  # noqa: E731
    fv = c["feat_v"] if sep_v else c["feat"]
    value = d(fv) @ d(c["wc"]) + d(c["bc"])[0]
    mean = d(c["feat"]) @ d(c["wa"]).T + d(c["ba"])
    sig = np.exp(d(c["logstd"]))
    act = np.zeros((R, A), np.float32)
    act[sr] = f32(mean + sig * np.clip(g.normal(size=(B, A)), -3, 3))
    lp, ent = G.gauss_logp_entropy(mean, c["logstd"], act[sr])
    planes = {k: f32(g.normal(size=R)) for k in ("adv", "ret")}
    planes["old_logp"] = np.zeros(R, np.float32)
    planes["old_logp"][sr] = f32(lp + g.normal(size=B) * 0.15)
    planes["vpred"] = np.zeros(R, np.float32)
    planes["vpred"][sr] = f32(value + g.normal(size=B) * 0.2)
    c.update(planes, actions=act, R=R)
    r = G.gauss_loss_head_grads(value, mean, c["logstd"], act[sr], planes["old_logp"][sr], planes["adv"][sr],
                                planes["vpred"][sr], planes["ret"][sr], CLIP, VC, EC, use_clipped)
    ag = (lambda dd, y: dd) if feat_act == 0 else (lambda dd, y: dd * (y > 0)) if feat_act == 1 else \
        (lambda dd, y: dd * (1 - y * y))
    dv = r["g_value"][:, None] * d(c["wc"])[None, :]
    dm = r["g_mean"] @ d(c["wa"])
    ref = {"value": value, "logp": lp, "entropy": ent,
           "dfeat": ag(dm if sep_v else dm + dv, d(c["feat"])),
           "dfeat_v": ag(dv, d(fv)) if sep_v else None,
           "g_wc": r["g_value"] @ d(fv), "g_bc": np.array([r["g_value"].sum()]),
           "g_wa": r["g_mean"].T @ d(c["feat"]), "g_ba": r["g_mean"].sum(0), "g_logstd": r["g_logstd"],
           "losses": np.array([r["value_loss"], r["action_loss"], r["entropy"]])}
    # the fp32 yardstick: torch's own fp32 Normal.log_prob on these inputs (CPU) vs float64
    from a2c_ppo_acktr.distributions import FixedNormal
    t = torch.from_numpy
    m32 = t(c["feat"]) @ t(c["wa"]).T + t(c["ba"])
    lp32 = FixedNormal(m32, t(c["logstd"]).exp().expand_as(m32)).log_probs(t(act[sr]))[:, 0].numpy()
    c["torch_fp32_err"] = float(np.abs(lp32 - lp).max())
    c["ref"] = ref
    return c


def _run_train(gpu, c, H, A, B, rows, sep_v, feat_act, use_clipped=True):
    Hh = _hip()
    t = {k: _dev(c[k]) for k in ("feat", "wc", "bc", "wa", "ba", "logstd", "actions", "old_logp", "adv", "vpred",
                                 "ret")}
    fv = _dev(c["feat_v"]) if sep_v else None
    idx = _dev(c["sr"]) if rows == "idx" else None
    nblk = Hh.call("ppo_heads_train_blocks", B)
    out = {"dfeat": torch.full((B, H), float("nan"), device=gpu),
           "dfeat_v": torch.full((B, H), float("nan"), device=gpu) if sep_v else None,
           "part_w": torch.full((nblk * (1 + A) * H,), float("nan"), device=gpu),
           "part_b": torch.full((nblk * (1 + 2 * A),), float("nan"), device=gpu),
           "part_l": torch.full((nblk * 4,), float("nan"), device=gpu)}
    p = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    Hh.call("ppo_heads_gauss_train", p(t["feat"]), p(fv), B, H, p(t["wc"]), p(t["bc"]), p(t["wa"]), p(t["ba"]),
            p(t["logstd"]), A, p(idx), 0 if rows == "idx" else rows, p(t["actions"]), p(t["old_logp"]), p(t["adv"]),
            p(t["vpred"]), p(t["ret"]), CLIP, VC, EC, 1.0 / B, int(use_clipped), feat_act, p(out["dfeat"]),
            p(out["dfeat_v"]), p(out["part_w"]), p(out["part_b"]), p(out["part_l"]), _s())
    torch.cuda.synchronize()
    return t, out, nblk


@pytest.mark.parametrize("H,A,B,rows,sep_v,feat_act", KERNEL_CASES)
def test_gauss_act_kernel_vs_float64(gpu, H, A, B, rows, sep_v, feat_act):
    """ppo_heads_gauss_act evaluating the given actions: value, log-prob and entropy
    vs float64 from the same fp32 inputs.  Tolerance: twice the worst error of torch's
    own fp32 Normal.log_prob (CPU) against float64 on these inputs, floor 1e-5
    (test_mlp_golden_evaluate's bound).  Measured torch fp32 error per case, in
    KERNEL_CASES order: 6.6e-8, 9.0e-7, 3.1e-6, 4.8e-6, 5.2e-6, 2.9e-6, 3.8e-6 — so
    the bound is the floor, 1e-5, except 1.03e-5 for (512, 9, 300, row0 11); it is
    recomputed from the inputs at run time, not taken from these figures."""
    Hh = _hip()
    c = _kernel_case(H, A, B, rows, sep_v, feat_act)
    tol = max(2 * c["torch_fp32_err"], 1e-5)
    sr = c["sr"]
    t = {k: _dev(c[k]) for k in ("feat", "wc", "bc", "wa", "ba", "logstd")}
    fv = _dev(c["feat_v"]) if sep_v else None
    given = _dev(c["actions"][sr])
    val, lp, ent = (torch.full((B,), float("nan"), device=gpu) for _ in range(3))
    Hh.call("ppo_heads_gauss_act", t["feat"].data_ptr(), None if fv is None else fv.data_ptr(), B, H,
            t["wc"].data_ptr(), t["bc"].data_ptr(), t["wa"].data_ptr(), t["ba"].data_ptr(), t["logstd"].data_ptr(), A,
            None, 0, 0, 0, given.data_ptr(), val.data_ptr(), None, lp.data_ptr(), ent.data_ptr(), _s())
    ref = c["ref"]
    for name, got in (("value", val), ("logp", lp), ("entropy", ent)):
        err = np.abs(got.cpu().numpy() - ref[name]).max()
        print(f"{name}: max err {err:.3e} (tol {tol:.1e}, torch fp32 {c['torch_fp32_err']:.1e})")
        assert err <= tol, (name, err, tol)


@pytest.mark.parametrize("H,A,B,rows,sep_v,feat_act", KERNEL_CASES)
def test_gauss_train_kernel_vs_float64(gpu, H, A, B, rows, sep_v, feat_act):
    """ppo_heads_gauss_train + ppo_heads_gauss_reduce: dfeat, dfeat_v and the head /
    logstd gradients vs the float64 helper, max |err| <= 1e-5 * max(max|ref|, 1e-3)
    per tensor (test_mlp_minibatch_grads_vs_oracle's rule); losses rtol 2e-5, atol
    1e-6; a second identical launch gives bit-identical partials."""
    _train_vs_float64(gpu, H, A, B, rows, sep_v, feat_act, True)


def _train_vs_float64(gpu, H, A, B, rows, sep_v, feat_act, use_clipped):
    Hh = _hip()
    c = _kernel_case(H, A, B, rows, sep_v, feat_act, use_clipped)
    t, out, nblk = _run_train(gpu, c, H, A, B, rows, sep_v, feat_act, use_clipped)
    _, out2, _ = _run_train(gpu, c, H, A, B, rows, sep_v, feat_act, use_clipped)
    for k in ("part_w", "part_b", "part_l", "dfeat"):
        assert torch.equal(out[k], out2[k]), k
    assert not torch.isnan(out["part_w"]).any() and not torch.isnan(out["part_b"]).any()
    assert float(out["part_l"].view(nblk, 4)[:, 3].sum()) == 0.0
    g = {"g_wc": torch.empty(H, device=gpu), "g_bc": torch.empty(1, device=gpu),
         "g_wa": torch.empty(A, H, device=gpu), "g_ba": torch.empty(A, device=gpu),
         "g_logstd": torch.empty(A, device=gpu)}
    acc = torch.zeros(4, dtype=torch.float64, device=gpu)
    Hh.call("ppo_heads_gauss_reduce", out["part_w"].data_ptr(), out["part_b"].data_ptr(), out["part_l"].data_ptr(),
            nblk, H, A, g["g_wc"].data_ptr(), g["g_bc"].data_ptr(), g["g_wa"].data_ptr(), g["g_ba"].data_ptr(),
            g["g_logstd"].data_ptr(), acc.data_ptr(), 1.0 / B, 1.0, _s())
    g["dfeat"] = out["dfeat"]
    if sep_v:
        g["dfeat_v"] = out["dfeat_v"]
    ref = c["ref"]
    for name, got in g.items():
        r = ref[name]
        err = np.abs(got.cpu().numpy().astype(np.float64) - r).max()
        bound = 1e-5 * max(np.abs(r).max(), 1e-3)
        print(f"{name}: max err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (name, err, bound)
    np.testing.assert_allclose(acc.cpu().numpy()[:3], ref["losses"], rtol=2e-5, atol=1e-6)
    return c


@pytest.mark.parametrize("H,A,B,rows,sep_v,feat_act", [KERNEL_CASES[2], KERNEL_CASES[6]])
def test_gauss_train_kernel_unclipped_value_loss(gpu, H, A, B, rows, sep_v, feat_act):
    """test_gauss_train_kernel_vs_float64 with use_clipped_value_loss = 0 (value loss
    0.5 mean((R - v)^2)) on the generic (100, 8, 129) and the LDS-weight (512, 8, 130)
    case: the same bounds against the float64 helper's unclipped branch, whose
    critic gradients differ from the clipped branch's on these inputs."""
    c = _train_vs_float64(gpu, H, A, B, rows, sep_v, feat_act, False)
    clipped = _kernel_case(H, A, B, rows, sep_v, feat_act)["ref"]
    gap = np.abs(clipped["g_wc"] - c["ref"]["g_wc"]).max()
    assert gap > 100 * 1e-5 * np.abs(c["ref"]["g_wc"]).max(), gap
    assert abs(clipped["losses"][0] - c["ref"]["losses"][0]) > 1e-3 * c["ref"]["losses"][0]


# ------------------------------------------------------------------- sampling
def _mlp_box(gpu, I=4, V=0, H=64, A=3, seed=0, logstd=None):
    from a2c_ppo_acktr import model as M
    from a2c_ppo_acktr.synthetic import Box
    torch.manual_seed(seed)
    pol = M.Policy((I,), Box(-1.0, 1.0, (A,)), base=M.MLPBase, base_kwargs={"recurrent": False, "hidden_size": H},
                   vector_obs_len=V)
    if logstd is not None:
        with torch.no_grad():
            pol.dist.logstd._bias.copy_(torch.as_tensor(logstd, dtype=torch.float32).view(A, 1))
    return pol.to(gpu)


def test_host_noise_sample_is_mul_then_add(gpu):
    """act(noise=eps) == eps * exp(logstd) + mean as torch's fp32 multiply, then add,
    on the device (torch.equal: no FMA contraction in the kernel), and
    evaluate_actions of the sampled actions returns act's log-prob bit for bit."""
    A, N = 5, 333
    pol = _mlp_box(gpu, A=A, seed=2, logstd=np.linspace(-1.0, 0.5, A))
    with torch.no_grad():
        pol.dist.fc_mean.weight.mul_(30.0)
    eng = pol.hip_engine()
    g = torch.Generator().manual_seed(9)
    x = torch.randn(N, 4, generator=g).to(gpu)
    eps = torch.empty(N, A).normal_(generator=g)
    _, mean, _, _ = eng.act(x, deterministic=True)
    v, a, lp, _ = eng.act(x, noise=eps)
    assert a.dtype == torch.float32 and a.shape == (N, A) and mean.abs().max() > 0.5
    sigma = pol.dist.logstd._bias.detach().view(1, A).exp()
    assert torch.equal(a, eps.to(gpu) * sigma + mean)
    v2, lp2, ent, _ = pol.evaluate_actions(x, None, None, None, a)
    assert torch.equal(lp2, lp) and torch.equal(v2, v)
    want = (0.5 + 0.5 * math.log(2 * math.pi)) * A + float(pol.dist.logstd._bias.detach().sum())
    assert abs(float(ent) - want) <= 1e-5


def test_device_normal_noise_statistics(gpu):
    """Counter-RNG sampling, N = 65,536 rows x A = 4: the n = 262,144 draws recovered
    as (a - mu) / sigma are finite, |mean| <= 5 / sqrt(n), |var - 1| <= 5 sqrt(2 / n),
    max |eps| < 7; another counter gives other draws, the same (seed, counter) the
    same draws bit for bit."""
    Hh = _hip()
    N, H, A = 65536, 64, 4
    feat = torch.zeros(N, H, device=gpu)
    wc, bc, wa = torch.zeros(H, device=gpu), torch.zeros(1, device=gpu), torch.zeros(A, H, device=gpu)
    mu = torch.tensor([0.5, -1.0, 0.0, 2.0], device=gpu)
    logstd = torch.tensor([-0.5, 0.0, 0.3, 0.1], device=gpu)

    def draw(seed, counter):
        a = torch.full((N, A), float("nan"), device=gpu)
        Hh.call("ppo_heads_gauss_act", feat.data_ptr(), None, N, H, wc.data_ptr(), bc.data_ptr(), wa.data_ptr(),
                mu.data_ptr(), logstd.data_ptr(), A, None, seed, counter, 0, None, None, a.data_ptr(), None, None,
                _s())
        return a

    a1, a2, a3 = draw(1234, 1), draw(1234, 2), draw(1234, 1)
    assert torch.equal(a1, a3) and not torch.equal(a1, a2)
    eps = ((a1 - mu) / logstd.exp()).double().cpu().numpy().reshape(-1)
    n = eps.size
    assert np.isfinite(eps).all()
    print("mean", eps.mean(), "var", eps.var(), "max", np.abs(eps).max())
    assert abs(eps.mean()) <= 5 / math.sqrt(n)
    assert abs(eps.var() - 1.0) <= 5 * math.sqrt(2.0 / n)
    assert np.abs(eps).max() < 7
    # dimensions and successive calls are not copies of each other
    e = eps.reshape(N, A)
    assert abs(np.corrcoef(e[:, 0], e[:, 1])[0, 1]) <= 5 / math.sqrt(N)
    e2 = ((a2 - mu) / logstd.exp()).double().cpu().numpy()
    assert abs(np.corrcoef(e[:, 0], e2[:, 0])[0, 1]) <= 5 / math.sqrt(N)


# ----------------------------------------------------------------- public API
def test_gauss_golden_through_policy(gpu):
    """gauss.npz (the reference's MLPBase(4, 64) submodules + DiagGaussian(64, 3)):
    evaluate_actions, get_value and act(deterministic=True) within 1e-5."""
    d = golden("gauss.npz")
    pol = _mlp_box(gpu, A=3)
    _load_flat(pol, np.concatenate([d["base_params"], d["head_params"]]))
    x = _dev(d["x"])
    v, lp, ent, _ = pol.evaluate_actions(x, None, None, None, _dev(d["action"]))
    np.testing.assert_allclose(v.cpu().numpy(), d["value"], atol=1e-5)
    np.testing.assert_allclose(lp.cpu().numpy(), d["log_probs"], atol=1e-5)
    np.testing.assert_allclose(float(ent), d["entropy"].mean(), atol=1e-5)
    np.testing.assert_allclose(pol.get_value(x, None, None, None).cpu().numpy(), d["value"], atol=1e-5)
    v, a, lp, _ = pol.act(x, None, None, None, deterministic=True)
    np.testing.assert_allclose(a.cpu().numpy(), d["mode"], atol=1e-5)
    np.testing.assert_allclose(v.cpu().numpy(), d["value"], atol=1e-5)
    # host-noise sample from the recorded draw
    _, a, lp, _ = pol.hip_engine().act(x, noise=torch.from_numpy(d["normal_noise"]))
    np.testing.assert_allclose(a.cpu().numpy(), d["action"], atol=1e-5)
    np.testing.assert_allclose(lp.cpu().numpy(), d["log_probs"], atol=2e-5)   # (a - mu) carries both errors


def test_mlp_box_minibatch_grads_vs_float64(gpu):
    """One MLPEngine minibatch (I = 5, V = 3, H = 128, A = 6, B = 37, lr 0): every
    parameter gradient, logstd included, vs float64 — the oracle's MLP forward /
    backward fed with the Gaussian helper's head gradients; max |err| <= 1e-5 *
    max(max|ref|, 1e-3) per tensor, losses rtol 2e-5 / atol 1e-6."""
    from a2c_ppo_acktr.algo.ppo import FlatAdam
    from a2c_ppo_acktr.storage import RolloutStorage
    from a2c_ppo_acktr.synthetic import Box
    I, V, H, A, B = 5, 3, 128, 6, 37
    pol = _mlp_box(gpu, I, V, H, A, seed=B, logstd=np.linspace(-1.0, 0.5, A)).cpu()
    with torch.no_grad():
        pol.base.critic_linear.weight.mul_(3.0)
    init = torch.cat([p.detach().reshape(-1) for p in pol.parameters()]).numpy().astype(np.float64)
    pol.to(gpu)
    eng = pol.hip_engine()
    T, N = 4, (B + 1) // 2
    st = RolloutStorage(T, N, (I,), [V], Box(-1.0, 1.0, (A,)), 1, device=gpu)
    g = torch.Generator().manual_seed(B + 1)
    st.obs.copy_(torch.randn(st.obs.shape, generator=g).to(gpu))
    st.vector_obs.copy_(torch.rand(st.vector_obs.shape, generator=g).to(gpu))
    # actions within 3 sigma of the policy's mean, as a rollout stores them (the
    # kernel tests' input rule): the log-prob's magnitude sets the fp32 resolution of
    # the ratio, and actions tens of sigma away would make the test one of that
    with torch.no_grad():
        _, mu, _, _ = pol.act(st.obs[:-1].reshape(T * N, I), st.vector_obs[:-1].reshape(T * N, V), None, None,
                              deterministic=True)
    sigma = pol.dist.logstd._bias.detach().view(1, A).exp()
    st.actions.copy_((mu + sigma * torch.randn(T * N, A, generator=g).clamp(-3, 3).to(gpu)).view(T, N, A))
    st.value_preds.copy_(torch.randn(st.value_preds.shape, generator=g).to(gpu) * 0.1)
    st.returns.copy_(torch.randn(st.returns.shape, generator=g).to(gpu))
    adv = torch.randn(T, N, generator=g).to(gpu)
    idx = torch.randperm(T * N, generator=g)[:B].to(gpu)
    shapes = G.mlp_gauss_param_shapes(I + V, H, A)
    p = O.unflatten(init, shapes)
    po = dict(p, **{"dist.linear.weight": p["dist.fc_mean.weight"], "dist.linear.bias": p["dist.fc_mean.bias"]})
    ii = idx.cpu().numpy()
    x = np.concatenate([st.obs[:-1].reshape(T * N, I).cpu().numpy()[ii],
                        st.vector_obs[:-1].reshape(T * N, V).cpu().numpy()[ii]], 1)
    value, mean, cache = O.mlp_forward(po, x.astype(np.float64))
    acts = st.actions.reshape(T * N, A).cpu().numpy()[ii]
    lp, _ = G.gauss_logp_entropy(mean, p["dist.logstd._bias"][:, 0], acts)
    olp = torch.zeros(T * N)
    olp[idx.cpu()] = torch.from_numpy(lp).float() + torch.randn(B, generator=g) * 0.15
    st.action_log_probs.copy_(olp.view(T, N, 1).to(gpu))
    hp = {"clip": CLIP, "value_coef": VC, "entropy_coef": EC, "use_clipped_value_loss": True}
    loss = torch.zeros(4, dtype=torch.float64, device=gpu)
    eng.train_minibatch(st, adv, idx, hp, loss, FlatAdam(pol.parameters(), lr=0.0, eps=1e-5, max_grad_norm=None))
    torch.cuda.synchronize()
    f = lambda t: t.reshape(-1).cpu().numpy()[ii]  # noqa: E731
    r = G.gauss_loss_head_grads(value, mean, p["dist.logstd._bias"][:, 0], acts, f(st.action_log_probs), f(adv),
                                f(st.value_preds[:-1]), f(st.returns[:-1]), CLIP, VC, EC)
    out = (r["ratio"] < 1 - CLIP) | (r["ratio"] > 1 + CLIP)
    assert out.any() and (~out).any()
    grads = O.mlp_backward(po, cache, r["g_value"], r["g_mean"])
    grads["dist.fc_mean.weight"], grads["dist.fc_mean.bias"] = grads["dist.linear.weight"], grads["dist.linear.bias"]
    grads["dist.logstd._bias"] = r["g_logstd"][:, None]
    got = O.unflatten(eng.grad.cpu().numpy(), shapes)
    for name, _ in shapes:
        ref = grads[name]
        err = np.abs(got[name] - ref).max()
        assert err <= 1e-5 * max(np.abs(ref).max(), 1e-3), (name, err, np.abs(ref).max())
    np.testing.assert_allclose(loss.cpu().numpy()[:3], [r["value_loss"], r["action_loss"], r["entropy"]],
                               rtol=2e-5, atol=1e-6)


def test_gauss_iteration_replays_reference(gpu):
    """The reference's iteration recorded in gauss_update.npz (CNNBase hidden 64 +
    DiagGaussian(64, 3), 4 envs x 4 steps, E = 2, Mb = 2, lr 1e-3) replayed in
    host-noise mode: stored values / log-probs / actions per step within 1e-5,
    returns within 1e-5, losses rtol 1e-4 / atol 1e-6, final parameters atol 2e-5 —
    the Categorical replay's bounds.  They stand because the reference's own fp32
    record is far closer than half of each to float64 on the recorded rollout
    (measured on the CPU by tools/gen_golden_gauss.py: values 3.4e-7, log-probs
    9.9e-7, returns 2.3e-7, losses 7.1e-7 relative, final parameters 3.7e-7)."""
    from a2c_ppo_acktr import model as M
    from a2c_ppo_acktr.algo import PPO
    from a2c_ppo_acktr.storage import RolloutStorage
    from a2c_ppo_acktr.synthetic import Box
    d = golden("gauss_update.npz")
    hidden, N, T, E, Mb, A = (int(x) for x in d["meta"])
    clip, vcoef, ecoef = (float(x) for x in d["coefs"])
    torch.set_num_threads(1)
    torch.manual_seed(1)
    box = Box(-1.0, 1.0, (A,))
    pol = M.Policy((4, 84, 84), box, base=M.CNNBase, base_kwargs={"recurrent": False, "hidden_size": hidden})
    assert [n for n, _ in pol.named_parameters()] == list(d["names"])
    _load_flat(pol, d["init_params"])
    pol.to(gpu)
    agent = PPO(pol, clip, E, Mb, vcoef, ecoef, lr=float(d["lr"][0]), eps=1e-5, max_grad_norm=0.5)
    st = RolloutStorage(T, N, (4, 84, 84), [0], box, 1, obs_dtype=torch.uint8, device=gpu)
    st.obs.copy_(_dev(d["obs_u8"]))
    keep = torch.get_rng_state()
    M.set_sampling_mode("host")
    try:
        noise = []
        for step in range(T):
            rs = torch.get_rng_state()
            v, a, lp, h = pol.act(st.obs[step], st.vector_obs[step], st.recurrent_hidden_states[step],
                                  st.masks[step])
            after = torch.get_rng_state()
            torch.set_rng_state(rs)
            noise.append(torch.empty(N, A).normal_().numpy())   # host mode consumed exactly this draw
            assert torch.equal(torch.get_rng_state(), after)
            st.insert(st.obs[step + 1], st.vector_obs[step + 1], h, a, lp, v, _dev(d["rewards"][step]),
                      _dev(d["masks"][step]), torch.ones(N, 1, device=gpu))
        nv = pol.get_value(st.obs[-1], st.vector_obs[-1], st.recurrent_hidden_states[-1], st.masks[-1])
        st.compute_returns(nv, True, 0.99, 0.95, False)
        losses = agent.update(st)
    finally:
        M.set_sampling_mode("device")
        torch.set_rng_state(keep)
    assert np.array_equal(np.stack(noise), d["normal_noise"])
    np.testing.assert_allclose(st.actions.cpu().numpy(), d["actions"], atol=1e-5)
    np.testing.assert_allclose(st.action_log_probs.cpu().numpy(), d["action_log_probs"], atol=1e-5)
    np.testing.assert_allclose(st.value_preds[:T].cpu().numpy(), d["values"], atol=1e-5)
    np.testing.assert_allclose(st.returns.cpu().numpy(), d["returns"], atol=1e-5)
    np.testing.assert_allclose(losses, d["losses"], rtol=1e-4, atol=1e-6)
    final = torch.cat([p.detach().reshape(-1) for p in pol.parameters()]).cpu().numpy()
    print("final params: max |err|", np.abs(final - d["final_params"]).max())
    np.testing.assert_allclose(final, d["final_params"], rtol=0, atol=2e-5)


def _cnn_box(gpu, recurrent, A, H, V=0, seed=3, logstd=None):
    from a2c_ppo_acktr import model as M
    from a2c_ppo_acktr.synthetic import Box
    torch.manual_seed(seed)
    pol = M.Policy((4, 84, 84), Box(-1.0, 1.0, (A,)), base=M.CNNBase,
                   base_kwargs={"recurrent": recurrent, "hidden_size": H}, vector_obs_len=V)
    if logstd is not None:
        with torch.no_grad():
            pol.dist.logstd._bias.copy_(torch.as_tensor(logstd, dtype=torch.float32).view(A, 1))
    return pol.to(gpu)


def _fill(pol, st, env, V=0):
    T, N = st.num_steps, st.rewards.shape[1]
    for step in range(T):
        v, a, lp, h = pol.act(st.obs[step], st.vector_obs[step], st.recurrent_hidden_states[step], st.masks[step])
        r, m, bm = env.step_into(st.obs[step + 1], a)
        st.insert(st.obs[step + 1], torch.rand(N, V, device=a.device) if V else st.vector_obs[step + 1], h, a, lp, v,
                  r, m, bm)
    nv = pol.get_value(st.obs[-1], st.vector_obs[-1], st.recurrent_hidden_states[-1], st.masks[-1])
    st.compute_returns(nv, True, 0.99, 0.95, False)


def test_recurrent_box_first_step_losses(gpu):
    """CNNBase recurrent (H = 32, V = 14, N = 4, T = 5) + Box(2), E = 1, Mb = 1: before
    the only optimizer step every ratio is 1, so the returned losses follow from the
    storage alone — value loss 0.5 mean((R - V)^2), action loss -mean(normalised
    advantage) (within 1e-6 of 0), entropy Σ(0.5 + 0.5 log 2π + logstd) within 1e-5;
    logstd moves and the BPTT path's error word stays 0."""
    from a2c_ppo_acktr.algo import PPO
    from a2c_ppo_acktr.storage import RolloutStorage
    from a2c_ppo_acktr.synthetic import Box, SyntheticVecEnv
    H, V, N, T, A = 32, 14, 4, 5, 2
    ls = [-0.4, 0.2]
    pol = _cnn_box(gpu, True, A, H, V, logstd=ls)
    agent = PPO(pol, 0.1, 1, 1, 0.5, 0.01, lr=1e-3, eps=1e-5, max_grad_norm=0.5)
    st = RolloutStorage(T, N, (4, 84, 84), [V], Box(-1.0, 1.0, (A,)), H, obs_dtype=torch.uint8, device=gpu)
    env = SyntheticVecEnv(N, seed=5, p_done=0.2, device=gpu)
    env.reset_into(st.obs[0])
    _fill(pol, st, env, V)
    assert st.actions.dtype == torch.float32 and st.actions.shape == (T, N, A)
    before = pol.dist.logstd._bias.detach().clone()
    R, Vp = st.returns[:-1].double().cpu().numpy(), st.value_preds[:-1].double().cpu().numpy()
    adv = R - Vp
    adv_n = (adv - adv.mean()) / (adv.std(ddof=1) + 1e-5)
    vl, al, ent = agent.update(st)
    eng = pol.hip_engine()
    assert int(eng.status[0].item()) == 0 and int(eng.status[1].item()) == 0
    np.testing.assert_allclose(vl, 0.5 * (adv ** 2).mean(), rtol=1e-4, atol=1e-6)
    assert abs(al - (-adv_n.mean())) <= 1e-6 and abs(al) <= 1e-6
    assert abs(ent - sum(0.5 + 0.5 * math.log(2 * math.pi) + s for s in ls)) <= 1e-5
    moved = (pol.dist.logstd._bias.detach() - before).abs()
    assert moved.min().item() > 1e-5, moved


def test_graphed_actor_on_box_policy(gpu):
    """GraphedActor captures Policy.act(deterministic=True) of a Box policy unchanged:
    float [N, A] actions, bit-equal to the eager call."""
    from a2c_ppo_acktr.evaluation import GraphedActor
    N, A = 6, 3
    pol = _cnn_box(gpu, False, A, 64, logstd=[-0.3, 0.0, 0.2])
    with torch.no_grad():
        pol.dist.fc_mean.weight.mul_(50.0)
    ga = GraphedActor(pol, num_envs=N, obs_dtype=torch.uint8)
    g = torch.Generator().manual_seed(4)
    for _ in range(2):
        obs = torch.randint(0, 256, (N, 4, 84, 84), dtype=torch.uint8, generator=g).to(gpu)
        hx, m = torch.zeros(N, 1, device=gpu), torch.ones(N, 1, device=gpu)
        v, a, lp, _ = ga.act(obs, torch.zeros(N, 0, device=gpu), hx, m)
        ev, ea, elp, _ = pol.act(obs, None, hx, m, deterministic=True)
        assert a.dtype == torch.float32 and a.shape == (N, A) and a.abs().max() > 1e-3
        assert torch.equal(a, ea) and torch.equal(v, ev) and torch.equal(lp, elp)


def test_nan_action_raises_before_any_step(gpu):
    """A stored action with a NaN component: PPO.update raises ValueError; the
    parameters, Adam moments and step counter stay bit-unchanged; after the caller
    repairs the rollout the update succeeds (mirrors the out-of-range-action test)."""
    from a2c_ppo_acktr.algo import PPO
    from a2c_ppo_acktr.storage import RolloutStorage
    from a2c_ppo_acktr.synthetic import Box, SyntheticVecEnv
    N, T, A = 16, 8, 3
    pol = _cnn_box(gpu, False, A, 64)
    agent = PPO(pol, 0.1, 2, 2, 0.5, 0.001, lr=1e-3, eps=1e-5, max_grad_norm=0.5)
    st = RolloutStorage(T, N, (4, 84, 84), [0], Box(-1.0, 1.0, (A,)), 1, obs_dtype=torch.uint8, device=gpu)
    env = SyntheticVecEnv(N, seed=3, p_done=0.05, device=gpu)
    env.reset_into(st.obs[0])
    _fill(pol, st, env)
    agent.update(st)
    st.after_update()
    _fill(pol, st, env)
    opt, eng = agent.optimizer, pol.hip_engine()
    before = (eng.flat.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.step_count)
    good = st.actions[3].clone()
    st.actions[3, :, 1] = float("nan")      # one component of every lane of one step
    with pytest.raises(ValueError, match=r"\b16 non-finite stored action"):
        agent.update(st)
    torch.cuda.synchronize()
    after = (eng.flat, opt.exp_avg, opt.exp_avg_sq, opt.step_count)
    for x, y in zip(before[:3], after[:3]):
        assert torch.equal(x, y)
    assert before[3] == after[3]
    st.actions[3] = good
    losses = agent.update(st)
    assert all(np.isfinite(losses)) and opt.step_count == before[3] + 4


def test_box_checkpoint_resume_is_bit_identical(gpu, tmp_path):
    """test_checkpoint.test_resume_is_bit_identical for a Box policy: the rebuilt
    policy (config round trip included) continues bit-identically."""
    from a2c_ppo_acktr import checkpoint as C
    from a2c_ppo_acktr.algo import PPO
    from a2c_ppo_acktr.distributions import DiagGaussian
    from a2c_ppo_acktr.storage import RolloutStorage
    from a2c_ppo_acktr.synthetic import Box, SyntheticVecEnv
    N, T, A = 8, 16, 3
    pol = _cnn_box(gpu, False, A, 64, logstd=[-0.3, 0.0, 0.2])
    agent = PPO(pol, 0.1, 2, 2, 0.5, 0.01, lr=1e-3, eps=1e-5, max_grad_norm=0.5)
    st = RolloutStorage(T, N, (4, 84, 84), [0], Box(-1.0, 1.0, (A,)), 1, obs_dtype=torch.uint8, device=gpu)
    env = SyntheticVecEnv(N, seed=5, p_done=0.2, device=gpu)
    env.reset_into(st.obs[0])
    _fill(pol, st, env)
    agent.update(st)
    st.after_update()
    path = str(tmp_path / "ck.pt")
    C.save_checkpoint(path, pol, None, agent=agent)
    _fill(pol, st, env)
    rng = torch.get_rng_state()
    l1 = agent.update(st)
    p1 = torch.cat([p.detach().reshape(-1) for p in pol.parameters()]).cpu()
    pol2, _ = C.load_checkpoint(path, device=gpu)
    assert isinstance(pol2.dist, DiagGaussian) and pol2.dist.fc_mean.weight.shape[0] == A
    agent2 = PPO(pol2, 0.1, 2, 2, 0.5, 0.01, lr=1e-3, eps=1e-5, max_grad_norm=0.5)
    C.load_checkpoint(path, device=gpu, agent=agent2)
    torch.set_rng_state(rng)
    l2 = agent2.update(st)
    p2 = torch.cat([p.detach().reshape(-1) for p in pol2.parameters()]).cpu()
    assert l1 == l2
    assert torch.equal(p1, p2)


def test_ppo_learns_to_track_its_observation(gpu):
    """Learning end to end (MLPBase hidden 64, Box(2)): one-step episodes built from
    torch ops on the device — obs x ~ U(-1, 1)^2, reward -|a - x|^2, every mask 0;
    16 envs x 128 steps, 4 epochs x 4 minibatches.  After 40 iterations mean|mu(x) -
    x|^2 over a fixed probe batch is below half its initial value."""
    from a2c_ppo_acktr.algo import PPO
    from a2c_ppo_acktr.storage import RolloutStorage
    from a2c_ppo_acktr.synthetic import Box
    N, T, iters = 16, 128, 40
    pol = _mlp_box(gpu, I=2, H=64, A=2, seed=0)
    agent = PPO(pol, 0.2, 4, 4, 0.5, 0.0, lr=2.5e-3, eps=1e-5, max_grad_norm=0.5)
    st = RolloutStorage(T, N, (2,), [0], Box(-1.0, 1.0, (2,)), 1, device=gpu)
    g = torch.Generator(device=gpu).manual_seed(11)
    probe = torch.rand(512, 2, device=gpu, generator=g) * 2 - 1

    def probe_err():
        _, mu, _, _ = pol.act(probe, None, None, None, deterministic=True)
        return float(((mu - probe) ** 2).sum(1).mean())

    e0 = probe_err()
    zeros, ones = torch.zeros(N, 1, device=gpu), torch.ones(N, 1, device=gpu)
    st.obs[0].copy_(torch.rand(N, 2, device=gpu, generator=g) * 2 - 1)
    for it in range(iters):
        for step in range(T):
            v, a, lp, h = pol.act(st.obs[step], st.vector_obs[step], st.recurrent_hidden_states[step],
                                  st.masks[step])
            r = -((a - st.obs[step]) ** 2).sum(1, keepdim=True)
            nxt = torch.rand(N, 2, device=gpu, generator=g) * 2 - 1
            st.insert(nxt, st.vector_obs[step + 1], h, a, lp, v, r, zeros, ones)
        nv = pol.get_value(st.obs[-1], st.vector_obs[-1], st.recurrent_hidden_states[-1], st.masks[-1])
        st.compute_returns(nv, True, 0.99, 0.95, True)
        losses = agent.update(st)
        st.after_update()
        assert all(np.isfinite(losses))
    e1 = probe_err()
    print(f"probe mean|mu(x) - x|^2: {e0:.4f} -> {e1:.4f} (ratio {e1 / e0:.3f})")
    assert e1 < 0.5 * e0, (e0, e1)
