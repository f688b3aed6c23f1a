"""MultiBinary action spaces on the HIP engine: the Bernoulli heads kernels through
the C ABI against float64 (tests/helpers/bern_ref.py), sampling, and the public API
(Policy / PPO / RolloutStorage / GraphedActor / checkpoints) against the
reference's records bern.npz and bern_update.npz."""
import functools
import math

import numpy as np
import pytest
import torch

from conftest import golden
from helpers import bern_ref as R
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
SATURATED = (512, 8, 130, "idx", False, 1)   # run with logit weights scaled for |z| up to ~40


@functools.lru_cache(maxsize=None)
def _kernel_case(H, A, B, rows, sep_v, feat_act, zscale=4.0, use_clipped=True):
    """fp32 inputs (random features in [-1, 1], logit weights scaled so the logits'
    standard deviation is zscale / 3: |z| <~ 4 at the default, actions drawn from
    those logits) and the float64 reference computed from those same fp32 values;
    computed once per case, never modified."""
    g = np.random.default_rng(1000 * H + 10 * A + B + int(zscale))
    f32 = lambda x: np.ascontiguousarray(x, np.float32)  # noqa: E731
    c = {"feat": f32(g.uniform(-1, 1, (B, H)))}
    c["feat_v"] = f32(g.uniform(-1, 1, (B, H))) if sep_v else None
    c["wc"] = f32(g.uniform(-1, 1, H) * 2 / math.sqrt(H))
    c["bc"] = f32(g.normal(size=1) * 0.1)
    c["wa"] = f32(g.uniform(-1, 1, (A, H)) * zscale / math.sqrt(H))
    c["ba"] = f32(g.normal(size=A) * 0.1)
    Rn = B + 16 if rows == "idx" else rows + B          # storage rows
    sr = g.permutation(Rn)[:B] if rows == "idx" else rows + np.arange(B)
    c["sr"] = sr.astype(np.int64)
    d = lambda x: x.astype(np.float64)  # noqa: E731
    fv = c["feat_v"] if sep_v else c["feat"]
    value = d(fv) @ d(c["wc"]) + d(c["bc"])[0]
    z = d(c["feat"]) @ d(c["wa"]).T + d(c["ba"])
    c["zmax"] = float(np.abs(z).max())
    act = np.zeros((Rn, A), np.float32)
    act[sr] = f32(g.uniform(size=(B, A)) < 1.0 / (1.0 + np.exp(-z)))
    lp, ent = R.bern_logp_entropy(z, act[sr])
    planes = {k: f32(g.normal(size=Rn)) for k in ("adv", "ret")}
    planes["old_logp"] = np.zeros(Rn, np.float32)
    planes["old_logp"][sr] = f32(lp + g.normal(size=B) * 0.15)
    planes["vpred"] = np.zeros(Rn, np.float32)
    planes["vpred"][sr] = f32(value + g.normal(size=B) * 0.2)
    c.update(planes, actions=act, R=Rn)
    r = R.bern_loss_head_grads(value, z, act[sr], planes["old_logp"][sr], planes["adv"][sr], planes["vpred"][sr],
                               planes["ret"][sr], CLIP, VC, EC, use_clipped)
    ag = (lambda dd, y: dd) if feat_act == 0 else (lambda dd, y: dd * (y > 0)) if feat_act == 1 else \
        (lambda dd, y: dd * (1 - y * y))
    dv = r["g_value"][:, None] * d(c["wc"])[None, :]
    dz = r["g_logits"] @ d(c["wa"])
    ref = {"value": value, "logp": lp, "entropy": ent,
           "dfeat": ag(dz if sep_v else dz + dv, d(c["feat"])),
           "dfeat_v": ag(dv, d(fv)) if sep_v else None,
           "g_wc": r["g_value"] @ d(fv), "g_bc": np.array([r["g_value"].sum()]),
           "g_wa": r["g_logits"].T @ d(c["feat"]), "g_ba": r["g_logits"].sum(0),
           "losses": np.array([r["value_loss"], r["action_loss"], r["entropy"]])}
    # the fp32 yardstick: torch's own fp32 FixedBernoulli on these inputs (CPU) vs float64
    from a2c_ppo_acktr.distributions import FixedBernoulli
    t = torch.from_numpy
    dist = FixedBernoulli(logits=t(c["feat"]) @ t(c["wa"]).T + t(c["ba"]))
    lp32 = dist.log_probs(t(act[sr]))[:, 0].numpy()
    c["torch_fp32_err"] = float(max(np.abs(lp32 - lp).max(), np.abs(dist.entropy().numpy() - ent).max()))
    c["ref"] = ref
    return c


def _run_train(gpu, c, H, A, B, rows, sep_v, feat_act, use_clipped=True):
    Hh = _hip()
    t = {k: _dev(c[k]) for k in ("feat", "wc", "bc", "wa", "ba", "actions", "old_logp", "adv", "vpred", "ret")}
    fv = _dev(c["feat_v"]) if sep_v else None
    idx = _dev(c["sr"]) if rows == "idx" else None
    nblk = Hh.call("ppo_heads_train_blocks", B)
    out = {"dfeat": torch.full((B, H), float("nan"), device=gpu),
           "dfeat_v": torch.full((B, H), float("nan"), device=gpu) if sep_v else None,
           "part_w": torch.full((nblk * (1 + A) * H,), float("nan"), device=gpu),
           "part_b": torch.full((nblk * (1 + A),), float("nan"), device=gpu),
           "part_l": torch.full((nblk * 4,), float("nan"), device=gpu)}
    p = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    Hh.call("ppo_heads_bern_train", p(t["feat"]), p(fv), B, H, p(t["wc"]), p(t["bc"]), p(t["wa"]), p(t["ba"]), A,
            p(idx), 0 if rows == "idx" else rows, p(t["actions"]), p(t["old_logp"]), p(t["adv"]), p(t["vpred"]),
            p(t["ret"]), CLIP, VC, EC, 1.0 / B, int(use_clipped), feat_act, p(out["dfeat"]),
            p(out["dfeat_v"]), p(out["part_w"]),
            p(out["part_b"]), p(out["part_l"]), _s())
    torch.cuda.synchronize()
    return t, out, nblk


def _reduce(gpu, out, nblk, H, A, B):
    Hh = _hip()
    g = {"g_wc": torch.empty(H, device=gpu), "g_bc": torch.empty(1, device=gpu),
         "g_wa": torch.empty(A, H, device=gpu), "g_ba": torch.empty(A, device=gpu)}
    acc = torch.zeros(4, dtype=torch.float64, device=gpu)
    Hh.call("ppo_heads_reduce", out["part_w"].data_ptr(), out["part_b"].data_ptr(), out["part_l"].data_ptr(), nblk, H,
            A, g["g_wc"].data_ptr(), g["g_bc"].data_ptr(), g["g_wa"].data_ptr(), g["g_ba"].data_ptr(), acc.data_ptr(),
            1.0 / B, 1.0, 1, _s())
    return g, acc


def _run_act(gpu, c, H, A, B, sep_v):
    Hh = _hip()
    t = {k: _dev(c[k]) for k in ("feat", "wc", "bc", "wa", "ba")}
    fv = _dev(c["feat_v"]) if sep_v else None
    given = _dev(c["actions"][c["sr"]])
    val, lp, ent = (torch.full((B,), float("nan"), device=gpu) for _ in range(3))
    Hh.call("ppo_heads_bern_act", t["feat"].data_ptr(), None if fv is None else fv.data_ptr(), B, H,
            t["wc"].data_ptr(), t["bc"].data_ptr(), t["wa"].data_ptr(), t["ba"].data_ptr(), A, None, 0, 0, 0,
            given.data_ptr(), val.data_ptr(), None, lp.data_ptr(), ent.data_ptr(), _s())
    return val, lp, ent


@pytest.mark.parametrize("H,A,B,rows,sep_v,feat_act", KERNEL_CASES)
def test_bern_act_kernel_vs_float64(gpu, H, A, B, rows, sep_v, feat_act):
    """ppo_heads_bern_act evaluating the given actions: value, log-prob and entropy vs
    float64 from the same fp32 inputs.  Tolerance: twice the worst error of torch's
    own fp32 FixedBernoulli log_probs / entropy (CPU) against float64 on these
    inputs, floor 1e-5 (test_gauss_act_kernel_vs_float64's rule), recomputed from
    the inputs at run time."""
    c = _kernel_case(H, A, B, rows, sep_v, feat_act)
    assert c["zmax"] < 8.0
    tol = max(2 * c["torch_fp32_err"], 1e-5)
    val, lp, ent = _run_act(gpu, c, H, A, B, sep_v)
    ref = c["ref"]
    for name, got in (("value", val), ("logp", lp), ("entropy", ent)):
        err = np.abs(got.cpu().numpy() - ref[name]).max()
        print(f"{name}: max err {err:.3e} (tol {tol:.1e}, torch fp32 {c['torch_fp32_err']:.1e})")
        assert err <= tol, (name, err, tol)


@pytest.mark.parametrize("H,A,B,rows,sep_v,feat_act", KERNEL_CASES)
def test_bern_train_kernel_vs_float64(gpu, H, A, B, rows, sep_v, feat_act):
    """ppo_heads_bern_train + ppo_heads_reduce: dfeat, dfeat_v and the head gradients
    vs the float64 helper, max |err| <= 1e-5 * max(max|ref|, 1e-3) per tensor
    (test_mlp_minibatch_grads_vs_oracle's rule); losses rtol 2e-5, atol 1e-6; no bad
    action counted; a second identical launch gives bit-identical partials."""
    _train_vs_float64(gpu, H, A, B, rows, sep_v, feat_act, True)


def _train_vs_float64(gpu, H, A, B, rows, sep_v, feat_act, use_clipped):
    c = _kernel_case(H, A, B, rows, sep_v, feat_act, use_clipped=use_clipped)
    t, out, nblk = _run_train(gpu, c, H, A, B, rows, sep_v, feat_act, use_clipped)
    _, out2, _ = _run_train(gpu, c, H, A, B, rows, sep_v, feat_act, use_clipped)
    for k in ("part_w", "part_b", "part_l", "dfeat"):
        assert torch.equal(out[k], out2[k]), k
    assert not torch.isnan(out["part_w"]).any() and not torch.isnan(out["part_b"]).any()
    assert float(out["part_l"].view(nblk, 4)[:, 3].sum()) == 0.0
    g, acc = _reduce(gpu, out, nblk, H, A, B)
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
def test_bern_train_kernel_unclipped_value_loss(gpu, H, A, B, rows, sep_v, feat_act):
    """test_bern_train_kernel_vs_float64 with use_clipped_value_loss = 0 (value loss
    0.5 mean((R - v)^2)) on the generic (100, 8, 129) and the LDS-weight (512, 8, 130)
    case: the same bounds against the float64 helper's unclipped branch, whose
    critic gradients differ from the clipped branch's on these inputs."""
    c = _train_vs_float64(gpu, H, A, B, rows, sep_v, feat_act, False)
    clipped = _kernel_case(H, A, B, rows, sep_v, feat_act)["ref"]
    gap = np.abs(clipped["g_wc"] - c["ref"]["g_wc"]).max()
    assert gap > 100 * 1e-5 * np.abs(c["ref"]["g_wc"]).max(), gap
    assert abs(clipped["losses"][0] - c["ref"]["losses"][0]) > 1e-3 * c["ref"]["losses"][0]


@pytest.mark.parametrize("lds", [1, 0])
def test_bern_kernels_stay_finite_when_saturated(gpu, lds):
    """Logits up to |z| ~ 40 (sigmoid rounds to exactly 0 or 1 in fp32, and stored
    actions on the improbable side occur): every output of act, train (LDS-weight and
    register kernel) and reduce is finite and no action is counted as bad."""
    Hh = _hip()
    H, A, B, rows, sep_v, feat_act = SATURATED
    c = _kernel_case(H, A, B, rows, sep_v, feat_act, zscale=36.0)
    assert 30.0 < c["zmax"] < 100.0
    acts = c["actions"].copy()
    acts[c["sr"][:8]] = 1.0 - acts[c["sr"][:8]]      # a few rows on the improbable side
    c = dict(c, actions=acts)
    for x in _run_act(gpu, c, H, A, B, sep_v):
        assert torch.isfinite(x).all()
    keep = Hh.call("ppo_tune_get", b"heads_lds")
    Hh.call("ppo_tune_set", b"heads_lds", lds)
    try:
        _, out, nblk = _run_train(gpu, c, H, A, B, rows, sep_v, feat_act)
    finally:
        Hh.call("ppo_tune_set", b"heads_lds", keep)
    g, acc = _reduce(gpu, out, nblk, H, A, B)
    for name, x in list(out.items()) + list(g.items()) + [("acc", acc)]:
        if x is not None:
            assert torch.isfinite(x).all(), name
    assert float(acc[3]) == 0.0


def test_lds_and_register_train_kernels_agree(gpu):
    """The LDS-weight kernel's case through the register kernel (heads_lds off): the
    same float64 bounds hold, so both variants are covered at H = 512, A = 8."""
    Hh = _hip()
    H, A, B, rows, sep_v, feat_act = KERNEL_CASES[-1]
    c = _kernel_case(H, A, B, rows, sep_v, feat_act)
    keep = Hh.call("ppo_tune_get", b"heads_lds")
    Hh.call("ppo_tune_set", b"heads_lds", 0)
    try:
        _, out, nblk = _run_train(gpu, c, H, A, B, rows, sep_v, feat_act)
    finally:
        Hh.call("ppo_tune_set", b"heads_lds", keep)
    g, acc = _reduce(gpu, out, nblk, H, A, B)
    g["dfeat"] = out["dfeat"]
    for name, got in g.items():
        r = c["ref"][name]
        err = np.abs(got.cpu().numpy().astype(np.float64) - r).max()
        assert err <= 1e-5 * max(np.abs(r).max(), 1e-3), (name, err)
    np.testing.assert_allclose(acc.cpu().numpy()[:3], c["ref"]["losses"], rtol=2e-5, atol=1e-6)


# ------------------------------------------------------------------- sampling
def _mlp_mb(gpu, I=4, V=0, H=64, A=3, seed=0):
    from a2c_ppo_acktr import model as M
    from a2c_ppo_acktr.synthetic import MultiBinary
    torch.manual_seed(seed)
    pol = M.Policy((I,), MultiBinary(A), base=M.MLPBase, base_kwargs={"recurrent": False, "hidden_size": H},
                   vector_obs_len=V)
    return pol.to(gpu)


def _mlp_logits64(pol, x):
    """float64 logits of an MLPBase policy from its fp32 parameters, on the device"""
    a = pol.base.actor
    h = torch.tanh(x.double() @ a[0].weight.double().T + a[0].bias.double())
    h = torch.tanh(h @ a[2].weight.double().T + a[2].bias.double())
    return h @ pol.dist.linear.weight.double().T + pol.dist.linear.bias.double()


def _host_noise_inputs(A, N):
    """x and uniforms for the host-noise test, drawn on the CPU: the first seed whose
    draw leaves at least 99 % of the rows at |u - p| >= 1e-5 from the CPU float64 p"""
    pol = _mlp_mb(torch.device("cpu"), A=A, seed=2)
    with torch.no_grad():
        pol.dist.linear.weight.mul_(3.0)
        for seed in range(9, 20):
            g = torch.Generator().manual_seed(seed)
            x = torch.randn(N, 4, generator=g)
            u = torch.empty(N, A).uniform_(generator=g)
            p = torch.sigmoid(_mlp_logits64(pol, x))
            if ((u.double() - p).abs().min(1).values >= 1e-5).float().mean() >= 0.99:
                return pol, x, u
    raise AssertionError("no seed leaves 99 % of the rows clear of p")


def test_host_noise_sample_is_u_less_than_p(gpu):
    """act(noise=u) == (u < p), which is torch.bernoulli(p) on the uniform_() draw u,
    with p = sigmoid(z) recomputed in torch on the device from the policy's
    parameters, for every row whose draws are all at least 1e-5 from p (at least 99 %
    of the rows); evaluate_actions of the sampled actions returns act's log-prob and
    value bit for bit."""
    A, N = 5, 333
    pol, x, u = _host_noise_inputs(A, N)
    pol.to(gpu)
    eng = pol.hip_engine()
    x = x.to(gpu)
    with torch.no_grad():
        p = torch.sigmoid(_mlp_logits64(pol, x))
    v, a, lp, _ = eng.act(x, noise=u)
    assert a.dtype == torch.float32 and a.shape == (N, A)
    assert bool(((a == 0) | (a == 1)).all()) and 0.2 < float(a.mean()) < 0.8
    clear = (u.to(gpu).double() - p).abs().min(1).values >= 1e-5
    assert float(clear.float().mean()) >= 0.99
    assert torch.equal(a[clear], (u.to(gpu).double() < p).float()[clear])
    v2, lp2, ent, _ = pol.evaluate_actions(x, None, None, None, a)
    assert torch.equal(lp2, lp) and torch.equal(v2, v)
    z = _mlp_logits64(pol, x).detach().cpu().numpy()
    want_lp, want_ent = R.bern_logp_entropy(z, a.cpu().numpy())
    np.testing.assert_allclose(lp.cpu().numpy()[:, 0], want_lp, atol=1e-5)
    assert abs(float(ent) - want_ent.mean()) <= 1e-5


def test_mode_is_probs_greater_than_half(gpu):
    """act(deterministic=True) == torch.gt(probs, 0.5): rows with |z| >= 1e-3 equal
    z > 0, and a head with all-zero weights and bias (p exactly 0.5) gives 0."""
    A, N = 6, 257
    pol = _mlp_mb(gpu, A=A, seed=4)
    x = torch.randn(N, 4, generator=torch.Generator().manual_seed(1)).to(gpu)
    _, a, _, _ = pol.act(x, None, None, None, deterministic=True)
    with torch.no_grad():
        z = _mlp_logits64(pol, x)
    sure = z.abs() >= 1e-3
    assert float(sure.float().mean()) > 0.9
    assert torch.equal(a[sure], (z > 0).float()[sure])
    assert 0.1 < float(a.mean()) < 0.9
    with torch.no_grad():
        pol.dist.linear.weight.zero_()
        pol.dist.linear.bias.zero_()
    _, a, lp, _ = pol.act(x, None, None, None, deterministic=True)
    assert float(a.abs().max()) == 0.0
    np.testing.assert_allclose(lp.cpu().numpy(), -A * math.log(2.0), atol=1e-6)


def test_device_uniform_noise_statistics(gpu):
    """Counter-RNG sampling, N = 65,536 rows x A = 4 with p = (0.1, 0.5, 0.9, 0.5):
    per-dimension frequency within 5 sqrt(p (1 - p) / N) of p; the correlation between
    two dimensions and between two counters is at most 5 / sqrt(N); another counter
    gives other bits, the same (seed, counter) the same bits."""
    Hh = _hip()
    N, H, A = 65536, 64, 4
    feat = torch.zeros(N, H, device=gpu)
    wc, bc, wa = torch.zeros(H, device=gpu), torch.zeros(1, device=gpu), torch.zeros(A, H, device=gpu)
    p = np.array([0.1, 0.5, 0.9, 0.5])
    ba = torch.tensor(np.log(p / (1 - p)), dtype=torch.float32, device=gpu)

    def draw(seed, counter):
        a = torch.full((N, A), float("nan"), device=gpu)
        Hh.call("ppo_heads_bern_act", feat.data_ptr(), None, N, H, wc.data_ptr(), bc.data_ptr(), wa.data_ptr(),
                ba.data_ptr(), A, None, seed, counter, 0, None, None, a.data_ptr(), None, None, _s())
        return a

    a1, a2, a3 = draw(1234, 1), draw(1234, 2), draw(1234, 1)
    assert torch.equal(a1, a3) and not torch.equal(a1, a2)
    e, e2 = a1.double().cpu().numpy(), a2.double().cpu().numpy()
    assert set(np.unique(e)) == {0.0, 1.0}
    freq = e.mean(0)
    print("frequency", freq)
    assert (np.abs(freq - p) <= 5 * np.sqrt(p * (1 - p) / N)).all(), freq
    assert abs(np.corrcoef(e[:, 1], e[:, 3])[0, 1]) <= 5 / math.sqrt(N)
    assert abs(np.corrcoef(e[:, 0], e[:, 2])[0, 1]) <= 5 / math.sqrt(N)
    assert abs(np.corrcoef(e[:, 1], e2[:, 1])[0, 1]) <= 5 / math.sqrt(N)


# ----------------------------------------------------------------- public API
def test_bern_golden_through_policy(gpu):
    """bern.npz (the reference's MLPBase(4, 64) submodules + Bernoulli(64, 3)):
    evaluate_actions and get_value within 1e-5, act(deterministic=True) and the
    host-noise sample from the recorded uniform draw bit-equal to the record."""
    d = golden("bern.npz")
    pol = _mlp_mb(gpu, A=3)
    _load_flat(pol, np.concatenate([d["base_params"], d["head_params"]]))
    x = _dev(d["x"])
    v, lp, ent, _ = pol.evaluate_actions(x, None, None, None, _dev(d["action"]))
    np.testing.assert_allclose(v.cpu().numpy(), d["value"], atol=1e-5)
    np.testing.assert_allclose(lp.cpu().numpy(), d["log_probs"], atol=1e-5)
    np.testing.assert_allclose(float(ent), d["entropy"].mean(), atol=1e-5)
    np.testing.assert_allclose(pol.get_value(x, None, None, None).cpu().numpy(), d["value"], atol=1e-5)
    assert np.abs(d["logits"]).min() > 1e-3 and np.abs(d["uniform_noise"] - d["probs"]).min() > 1e-4
    v, a, lp, _ = pol.act(x, None, None, None, deterministic=True)
    assert np.array_equal(a.cpu().numpy(), d["mode"])
    np.testing.assert_allclose(v.cpu().numpy(), d["value"], atol=1e-5)
    _, a, lp, _ = pol.hip_engine().act(x, noise=torch.from_numpy(d["uniform_noise"]))
    assert np.array_equal(a.cpu().numpy(), d["action"])
    np.testing.assert_allclose(lp.cpu().numpy(), d["log_probs"], atol=1e-5)


def test_mlp_multibinary_minibatch_grads_vs_float64(gpu):
    """One MLPEngine minibatch (I = 5, V = 3, H = 128, A = 6, B = 37, lr 0): every
    parameter gradient vs float64 — the oracle's MLP forward / backward fed with the
    Bernoulli helper's head gradients; max |err| <= 1e-5 * max(max|ref|, 1e-3) per
    tensor, losses rtol 2e-5 / atol 1e-6."""
    from a2c_ppo_acktr.algo.ppo import FlatAdam
    from a2c_ppo_acktr.storage import RolloutStorage
    from a2c_ppo_acktr.synthetic import MultiBinary
    I, V, H, A, B = 5, 3, 128, 6, 37
    pol = _mlp_mb(gpu, I, V, H, A, seed=B).cpu()
    with torch.no_grad():
        pol.base.critic_linear.weight.mul_(3.0)
        pol.dist.linear.weight.mul_(2.0)
    init = torch.cat([p.detach().reshape(-1) for p in pol.parameters()]).numpy().astype(np.float64)
    pol.to(gpu)
    eng = pol.hip_engine()
    T, N = 4, (B + 1) // 2
    st = RolloutStorage(T, N, (I,), [V], MultiBinary(A), 1, device=gpu)
    g = torch.Generator().manual_seed(B + 1)
    st.obs.copy_(torch.randn(st.obs.shape, generator=g).to(gpu))
    st.vector_obs.copy_(torch.rand(st.vector_obs.shape, generator=g).to(gpu))
    st.actions.copy_((torch.rand(T, N, A, generator=g) < 0.5).float().to(gpu))
    st.value_preds.copy_(torch.randn(st.value_preds.shape, generator=g).to(gpu) * 0.1)
    st.returns.copy_(torch.randn(st.returns.shape, generator=g).to(gpu))
    adv = torch.randn(T, N, generator=g).to(gpu)
    idx = torch.randperm(T * N, generator=g)[:B].to(gpu)
    shapes = R.mlp_bern_param_shapes(I + V, H, A)
    p = O.unflatten(init, shapes)
    ii = idx.cpu().numpy()
    x = np.concatenate([st.obs[:-1].reshape(T * N, I).cpu().numpy()[ii],
                        st.vector_obs[:-1].reshape(T * N, V).cpu().numpy()[ii]], 1)
    value, z, cache = O.mlp_forward(p, x.astype(np.float64))
    acts = st.actions.reshape(T * N, A).cpu().numpy()[ii]
    lp, _ = R.bern_logp_entropy(z, acts)
    olp = torch.zeros(T * N)
    olp[idx.cpu()] = torch.from_numpy(lp).float() + torch.randn(B, generator=g) * 0.15
    st.action_log_probs.copy_(olp.view(T, N, 1).to(gpu))
    hp = {"clip": CLIP, "value_coef": VC, "entropy_coef": EC, "use_clipped_value_loss": True}
    loss = torch.zeros(4, dtype=torch.float64, device=gpu)
    eng.train_minibatch(st, adv, idx, hp, loss, FlatAdam(pol.parameters(), lr=0.0, eps=1e-5, max_grad_norm=None))
    torch.cuda.synchronize()
    f = lambda t: t.reshape(-1).cpu().numpy()[ii]  # noqa: E731
    r = R.bern_loss_head_grads(value, z, acts, f(st.action_log_probs), f(adv), f(st.value_preds[:-1]),
                               f(st.returns[:-1]), CLIP, VC, EC)
    out = (r["ratio"] < 1 - CLIP) | (r["ratio"] > 1 + CLIP)
    assert out.any() and (~out).any()
    grads = O.mlp_backward(p, cache, r["g_value"], r["g_logits"])
    got = O.unflatten(eng.grad.cpu().numpy(), shapes)
    for name, _ in shapes:
        ref = grads[name]
        err = np.abs(got[name] - ref).max()
        assert err <= 1e-5 * max(np.abs(ref).max(), 1e-3), (name, err, np.abs(ref).max())
    assert float(loss[3]) == 0.0
    np.testing.assert_allclose(loss.cpu().numpy()[:3], [r["value_loss"], r["action_loss"], r["entropy"]],
                               rtol=2e-5, atol=1e-6)


def test_bern_iteration_replays_reference(gpu):
    """The reference's iteration recorded in bern_update.npz (CNNBase hidden 64 +
    Bernoulli(64, 3), 4 envs x 4 steps, E = 2, Mb = 2, lr 1e-3) replayed in host-noise
    mode: stored actions bit-exact, values / log-probs per step within 1e-5, returns
    within 1e-5, losses rtol 1e-4 / atol 1e-6, final parameters atol 2e-5 — the
    Categorical replay's bounds.  They stand because the reference's own fp32 record
    is far closer than half of each to float64 on the recorded rollout (measured on
    the CPU by tools/gen_golden_bern.py and kept in the fixture: values 3.4e-7,
    log-probs 2.4e-7, returns 2.3e-7, losses 2.6e-7 relative, final parameters
    2.5e-7), and no recorded draw is closer than 3.2e-2 to its p."""
    from a2c_ppo_acktr import model as M
    from a2c_ppo_acktr.algo import PPO
    from a2c_ppo_acktr.storage import RolloutStorage
    from a2c_ppo_acktr.synthetic import MultiBinary
    d = golden("bern_update.npz")
    hidden, N, T, E, Mb, A = (int(x) for x in d["meta"])
    clip, vcoef, ecoef = (float(x) for x in d["coefs"])
    dist = dict(zip(d["fp64_distance_names"], d["fp64_distance"]))
    assert max(dist["values"], dist["log_probs"], dist["returns"]) < 0.5e-5
    assert dist["losses_rel"] < 0.5e-4 and dist["final_params"] < 1e-5 and float(d["min_margin"][0]) >= 1e-4
    torch.set_num_threads(1)
    torch.manual_seed(1)
    mb = MultiBinary(A)
    pol = M.Policy((4, 84, 84), mb, base=M.CNNBase, base_kwargs={"recurrent": False, "hidden_size": hidden})
    assert [n for n, _ in pol.named_parameters()] == list(d["names"])
    _load_flat(pol, d["init_params"])
    pol.to(gpu)
    agent = PPO(pol, clip, E, Mb, vcoef, ecoef, lr=float(d["lr"][0]), eps=1e-5, max_grad_norm=0.5)
    st = RolloutStorage(T, N, (4, 84, 84), [0], mb, 1, obs_dtype=torch.uint8, device=gpu)
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
            noise.append(torch.empty(N, A).uniform_().numpy())   # host mode consumed exactly this draw
            assert torch.equal(torch.get_rng_state(), after)
            st.insert(st.obs[step + 1], st.vector_obs[step + 1], h, a, lp, v, _dev(d["rewards"][step]),
                      _dev(d["masks"][step]), torch.ones(N, 1, device=gpu))
        nv = pol.get_value(st.obs[-1], st.vector_obs[-1], st.recurrent_hidden_states[-1], st.masks[-1])
        st.compute_returns(nv, True, 0.99, 0.95, False)
        losses = agent.update(st)
    finally:
        M.set_sampling_mode("device")
        torch.set_rng_state(keep)
    assert np.array_equal(np.stack(noise), d["uniform_noise"])
    assert np.array_equal(st.actions.cpu().numpy(), d["actions"])
    np.testing.assert_allclose(st.action_log_probs.cpu().numpy(), d["action_log_probs"], atol=1e-5)
    np.testing.assert_allclose(st.value_preds[:T].cpu().numpy(), d["values"], atol=1e-5)
    np.testing.assert_allclose(st.returns.cpu().numpy(), d["returns"], atol=1e-5)
    np.testing.assert_allclose(losses, d["losses"], rtol=1e-4, atol=1e-6)
    final = torch.cat([p.detach().reshape(-1) for p in pol.parameters()]).cpu().numpy()
    print("final params: max |err|", np.abs(final - d["final_params"]).max())
    np.testing.assert_allclose(final, d["final_params"], rtol=0, atol=2e-5)


def _cnn_mb(gpu, recurrent, A, H, V=0, seed=3):
    from a2c_ppo_acktr import model as M
    from a2c_ppo_acktr.synthetic import MultiBinary
    torch.manual_seed(seed)
    pol = M.Policy((4, 84, 84), MultiBinary(A), base=M.CNNBase,
                   base_kwargs={"recurrent": recurrent, "hidden_size": H}, vector_obs_len=V)
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


def test_recurrent_multibinary_first_step_losses(gpu):
    """CNNBase recurrent (H = 64, N = 4, T = 5) + MultiBinary(3), E = 1, Mb = 1.  The
    GRU's output is the head's feature vector, so the hidden states the rollout stored
    are the engine's own features: the float64 helper on them (logits and values from
    the fp32 head parameters, the stored actions, log-probs, value predictions,
    returns and normalised advantages) gives the losses of the only optimizer step.
    Value loss rtol 1e-4, action loss and entropy within 1e-5 (the evaluate bound on
    a log-prob, with mean |normalised advantage| <= 1); sequence evaluate_actions
    returns the stored log-probs within 1e-5; the head parameters move and the BPTT
    path's error word stays 0."""
    from a2c_ppo_acktr.algo import PPO
    from a2c_ppo_acktr.storage import RolloutStorage
    from a2c_ppo_acktr.synthetic import MultiBinary, SyntheticVecEnv
    H, N, T, A = 64, 4, 5, 3
    pol = _cnn_mb(gpu, True, A, H)
    with torch.no_grad():
        pol.dist.linear.weight.mul_(3.0)
    agent = PPO(pol, 0.1, 1, 1, 0.5, 0.01, lr=1e-3, eps=1e-5, max_grad_norm=0.5)
    st = RolloutStorage(T, N, (4, 84, 84), [0], MultiBinary(A), H, obs_dtype=torch.uint8, device=gpu)
    env = SyntheticVecEnv(N, seed=5, p_done=0.2, device=gpu)
    env.reset_into(st.obs[0])
    _fill(pol, st, env)
    assert st.actions.dtype == torch.float32 and st.actions.shape == (T, N, A)
    assert bool(((st.actions == 0) | (st.actions == 1)).all())
    d64 = lambda t: t.detach().double().cpu().numpy()  # noqa: E731
    feat = d64(st.recurrent_hidden_states[1:]).reshape(T * N, H)
    z = feat @ d64(pol.dist.linear.weight).T + d64(pol.dist.linear.bias)
    value = feat @ d64(pol.base.critic_linear.weight)[0] + d64(pol.base.critic_linear.bias)[0]
    assert np.abs(z).max() > 0.05
    Rt, Vp = d64(st.returns[:-1]), d64(st.value_preds[:-1])
    adv = Rt - Vp
    adv_n = (adv - adv.mean()) / (adv.std(ddof=1) + 1e-5)
    r = R.bern_loss_head_grads(value, z, d64(st.actions).reshape(T * N, A), d64(st.action_log_probs).reshape(-1),
                               adv_n.reshape(-1), Vp.reshape(-1), Rt.reshape(-1), 0.1, 0.5, 0.01)
    np.testing.assert_allclose(r["logp"], d64(st.action_log_probs).reshape(-1), atol=1e-5)
    v2, lp2, ent2, _ = pol.evaluate_actions(st.obs[:-1].reshape(T * N, 4, 84, 84), st.vector_obs[:-1].reshape(T * N, 0),
                                            st.recurrent_hidden_states[0], st.masks[:-1].reshape(T * N, 1),
                                            st.actions.reshape(T * N, A))
    np.testing.assert_allclose(d64(lp2), d64(st.action_log_probs).reshape(T * N, 1), atol=1e-5)
    assert abs(float(ent2) - r["entropy"]) <= 1e-5
    before = [p.detach().clone() for p in pol.dist.parameters()]
    vl, al, ent = agent.update(st)
    eng = pol.hip_engine()
    assert int(eng.status[0].item()) == 0 and int(eng.status[1].item()) == 0
    print("losses", vl, al, ent, "helper", r["value_loss"], r["action_loss"], r["entropy"])
    assert all(np.isfinite([vl, al, ent]))
    np.testing.assert_allclose(vl, r["value_loss"], rtol=1e-4, atol=1e-6)
    assert abs(al - r["action_loss"]) <= 1e-5
    assert abs(ent - r["entropy"]) <= 1e-5
    for b, p in zip(before, pol.dist.parameters()):
        assert float((p.detach() - b).abs().max()) > 1e-5


def test_graphed_actor_on_multibinary_policy(gpu):
    """GraphedActor captures Policy.act(deterministic=True) of a MultiBinary policy
    unchanged: float [N, A] actions, bit-equal to the eager call."""
    from a2c_ppo_acktr.evaluation import GraphedActor
    N, A = 6, 3
    pol = _cnn_mb(gpu, False, A, 64)
    with torch.no_grad():
        pol.dist.linear.weight.mul_(50.0)
    ga = GraphedActor(pol, num_envs=N, obs_dtype=torch.uint8)
    g = torch.Generator().manual_seed(4)
    seen = []
    for _ in range(2):
        obs = torch.randint(0, 256, (N, 4, 84, 84), dtype=torch.uint8, generator=g).to(gpu)
        hx, m = torch.zeros(N, 1, device=gpu), torch.ones(N, 1, device=gpu)
        v, a, lp, _ = ga.act(obs, torch.zeros(N, 0, device=gpu), hx, m)
        ev, ea, elp, _ = pol.act(obs, None, hx, m, deterministic=True)
        assert a.dtype == torch.float32 and a.shape == (N, A) and bool(((a == 0) | (a == 1)).all())
        assert torch.equal(a, ea) and torch.equal(v, ev) and torch.equal(lp, elp)
        seen.append(a.clone())
    both = torch.cat(seen)
    assert 0.0 < float(both.mean()) < 1.0     # the mode is not a constant


@pytest.mark.parametrize("bad", [0.5, float("nan")])
def test_bad_action_raises_before_any_step(gpu, bad):
    """A stored action with a component that is not 0 or 1 (0.5, NaN): PPO.update
    raises ValueError naming the row count; the parameters, Adam moments and step
    counter stay bit-unchanged; after the caller repairs the rollout the update
    succeeds (mirrors the Box NaN-action test)."""
    from a2c_ppo_acktr.algo import PPO
    from a2c_ppo_acktr.storage import RolloutStorage
    from a2c_ppo_acktr.synthetic import MultiBinary, SyntheticVecEnv
    N, T, A = 16, 8, 3
    pol = _cnn_mb(gpu, False, A, 64)
    agent = PPO(pol, 0.1, 2, 2, 0.5, 0.001, lr=1e-3, eps=1e-5, max_grad_norm=0.5)
    st = RolloutStorage(T, N, (4, 84, 84), [0], MultiBinary(A), 1, obs_dtype=torch.uint8, device=gpu)
    env = SyntheticVecEnv(N, seed=3, p_done=0.05, device=gpu)
    env.reset_into(st.obs[0])
    _fill(pol, st, env)
    agent.update(st)
    st.after_update()
    _fill(pol, st, env)
    opt, eng = agent.optimizer, pol.hip_engine()
    before = (eng.flat.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.step_count)
    good = st.actions[3].clone()
    st.actions[3, :, 1] = bad      # one component of every lane of one step
    with pytest.raises(ValueError, match=r"\b16 stored action\(s\) with a component that is not 0 or 1"):
        agent.update(st)
    torch.cuda.synchronize()
    after = (eng.flat, opt.exp_avg, opt.exp_avg_sq, opt.step_count)
    for x, y in zip(before[:3], after[:3]):
        assert torch.equal(x, y)
    assert before[3] == after[3]
    st.actions[3] = good
    losses = agent.update(st)
    assert all(np.isfinite(losses)) and opt.step_count == before[3] + 4


def test_multibinary_checkpoint_resume_is_bit_identical(gpu, tmp_path):
    """test_checkpoint.test_resume_is_bit_identical for a MultiBinary policy: the
    rebuilt policy (config round trip included) continues bit-identically."""
    from a2c_ppo_acktr import checkpoint as C
    from a2c_ppo_acktr.algo import PPO
    from a2c_ppo_acktr.distributions import Bernoulli
    from a2c_ppo_acktr.storage import RolloutStorage
    from a2c_ppo_acktr.synthetic import MultiBinary, SyntheticVecEnv
    N, T, A = 8, 16, 3
    pol = _cnn_mb(gpu, False, A, 64)
    agent = PPO(pol, 0.1, 2, 2, 0.5, 0.01, lr=1e-3, eps=1e-5, max_grad_norm=0.5)
    st = RolloutStorage(T, N, (4, 84, 84), [0], MultiBinary(A), 1, obs_dtype=torch.uint8, device=gpu)
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
    assert isinstance(pol2.dist, Bernoulli) and pol2.dist.linear.weight.shape[0] == A
    agent2 = PPO(pol2, 0.1, 2, 2, 0.5, 0.01, lr=1e-3, eps=1e-5, max_grad_norm=0.5)
    C.load_checkpoint(path, device=gpu, agent=agent2)
    torch.set_rng_state(rng)
    l2 = agent2.update(st)
    p2 = torch.cat([p.detach().reshape(-1) for p in pol2.parameters()]).cpu()
    assert l1 == l2
    assert torch.equal(p1, p2)


def test_ppo_learns_the_sign_of_its_observation(gpu):
    """Learning end to end (MLPBase hidden 64, MultiBinary(3)): one-step episodes built
    from torch ops on the device — obs x ~ U(-1, 1)^3, reward = the number of
    components with a_o == (x_o > 0), every mask 0; 16 envs x 128 steps, 4 epochs x 4
    minibatches.  After 40 iterations the mode's error rate over a fixed 512-row
    probe is below half its initial value."""
    from a2c_ppo_acktr.algo import PPO
    from a2c_ppo_acktr.storage import RolloutStorage
    from a2c_ppo_acktr.synthetic import MultiBinary
    N, T, iters, A = 16, 128, 40, 3
    pol = _mlp_mb(gpu, I=A, H=64, A=A, seed=0)
    agent = PPO(pol, 0.2, 4, 4, 0.5, 0.0, lr=2.5e-3, eps=1e-5, max_grad_norm=0.5)
    st = RolloutStorage(T, N, (A,), [0], MultiBinary(A), 1, device=gpu)
    g = torch.Generator(device=gpu).manual_seed(11)
    probe = torch.rand(512, A, device=gpu, generator=g) * 2 - 1

    def probe_err():
        _, a, _, _ = pol.act(probe, None, None, None, deterministic=True)
        return float((a != (probe > 0).float()).float().mean())

    e0 = probe_err()
    zeros, ones = torch.zeros(N, 1, device=gpu), torch.ones(N, 1, device=gpu)
    st.obs[0].copy_(torch.rand(N, A, device=gpu, generator=g) * 2 - 1)
    for it in range(iters):
        for step in range(T):
            v, a, lp, h = pol.act(st.obs[step], st.vector_obs[step], st.recurrent_hidden_states[step],
                                  st.masks[step])
            r = (a == (st.obs[step] > 0).float()).float().sum(1, keepdim=True)
            nxt = torch.rand(N, A, device=gpu, generator=g) * 2 - 1
            st.insert(nxt, st.vector_obs[step + 1], h, a, lp, v, r, zeros, ones)
        nv = pol.get_value(st.obs[-1], st.vector_obs[-1], st.recurrent_hidden_states[-1], st.masks[-1])
        st.compute_returns(nv, True, 0.99, 0.95, True)
        losses = agent.update(st)
        st.after_update()
        assert all(np.isfinite(losses))
    e1 = probe_err()
    print(f"probe error rate of the mode: {e0:.4f} -> {e1:.4f} (ratio {e1 / max(e0, 1e-9):.3f})")
    assert e0 > 0.2 and e1 < 0.5 * e0, (e0, e1)
