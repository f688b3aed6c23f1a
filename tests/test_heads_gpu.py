"""The Categorical heads kernels (heads.hip) through the C ABI against float64
(tests/helpers/cat_ref.py) across their dispatch matrix: every HC x AMAX x FAST
instantiation of the act and train kernels, the LDS-weight kernel, its register
counterpart and its alignment fallback, gathered rows and row0 offsets, separate
critic features, the three feature activations, both value losses, several rows per
wave in the act kernel, saturated logits, stored actions outside the int32 range,
and ppo_mean_f32.  Output buffers are prefilled with NaN."""
import numpy as np
import pytest
import torch

from helpers import cat_ref as C
from oracle import ppo_oracle as O

pytestmark = pytest.mark.gpu

CLIP, VC, EC = C.CLIP, C.VC, C.EC
IDS = [C.case_id(c) for c in C.CASES]
NAN = float("nan")


def _hip():
    from a2c_ppo_acktr import _hip
    return _hip


def _s():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(x):
    return None if x is None else x.data_ptr()


def _off4(t):
    """a copy of t that starts 4 bytes into a larger buffer (not 16-byte aligned)"""
    buf = torch.full((t.numel() + 4,), NAN, device=t.device, dtype=t.dtype)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


class _Knob:
    """ppo_tune_set(name, value) for the block, the old value restored after it"""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.keep = _hip().call("ppo_tune_get", self.name)
        if self.value is not None:
            _hip().call("ppo_tune_set", self.name, self.value)

    def __exit__(self, *exc):
        _hip().call("ppo_tune_set", self.name, self.keep)


def _run_act(gpu, c, N, H, A, given=None, noise=None, deterministic=0):
    """ppo_heads_act -> value, action, log-prob, entropy (NaN / -1 prefilled)"""
    t = {k: _dev(c[k]) for k in ("feat", "wc", "bc", "wa", "ba")}
    fv = _dev(c["feat_v"]) if c.get("feat_v") is not None else None
    gv = None if given is None else _dev(np.asarray(given, np.int64))
    nz = None if noise is None else _dev(noise)
    val, lp, ent = (torch.full((N,), NAN, device=gpu) for _ in range(3))
    act = torch.full((N,), -1, dtype=torch.int64, device=gpu)
    _hip().call("ppo_heads_act", _p(t["feat"]), _p(fv), N, H, _p(t["wc"]), _p(t["bc"]), _p(t["wa"]), _p(t["ba"]), A,
                _p(nz), 0, 0, deterministic, _p(gv), _p(val), _p(act), _p(lp), _p(ent), _s())
    torch.cuda.synchronize()
    return val, act, lp, ent


def _run_train(gpu, c, lds=None, feat_off=False, dfeat_off=False, actions=None):
    """ppo_heads_train + ppo_heads_reduce of case c -> (raw outputs, gradients, loss_acc)"""
    Hh = _hip()
    H, A, B, rows, sep_v = c["H"], c["A"], c["B"], c["rows"], c["sep_v"]
    t = {k: _dev(c[k]) for k in ("feat", "wc", "bc", "wa", "ba", "old_logp", "adv", "vpred", "ret")}
    t["actions"] = _dev(c["actions"] if actions is None else actions)
    if feat_off:
        t["feat"] = _off4(t["feat"])
    fv = _dev(c["feat_v"]) if sep_v else None
    idx = _dev(c["sr"]) if rows == "idx" else None
    nblk = Hh.call("ppo_heads_train_blocks", B)
    out = {"dfeat": torch.full((B, H), NAN, device=gpu),
           "dfeat_v": torch.full((B, H), NAN, device=gpu) if sep_v else None,
           "part_w": torch.full((nblk * (1 + A) * H,), NAN, device=gpu),
           "part_b": torch.full((nblk * (1 + A),), NAN, device=gpu),
           "part_l": torch.full((nblk * 4,), NAN, device=gpu)}
    if dfeat_off:
        out["dfeat"] = _off4(out["dfeat"])
    with _Knob(b"heads_lds", lds):
        Hh.call("ppo_heads_train", _p(t["feat"]), _p(fv), B, H, _p(t["wc"]), _p(t["bc"]), _p(t["wa"]), _p(t["ba"]), A,
                _p(idx), 0 if rows == "idx" else rows, _p(t["actions"]), _p(t["old_logp"]), _p(t["adv"]),
                _p(t["vpred"]), _p(t["ret"]), CLIP, VC, EC, 1.0 / B, int(c["use_clipped"]), c["feat_act"],
                _p(out["dfeat"]), _p(out["dfeat_v"]), _p(out["part_w"]), _p(out["part_b"]), _p(out["part_l"]), _s())
    torch.cuda.synchronize()
    g = {"g_wc": torch.full((H,), NAN, device=gpu), "g_bc": torch.full((1,), NAN, device=gpu),
         "g_wa": torch.full((A, H), NAN, device=gpu), "g_ba": torch.full((A,), NAN, device=gpu)}
    acc = torch.zeros(4, dtype=torch.float64, device=gpu)
    Hh.call("ppo_heads_reduce", _p(out["part_w"]), _p(out["part_b"]), _p(out["part_l"]), nblk, H, A, _p(g["g_wc"]),
            _p(g["g_bc"]), _p(g["g_wa"]), _p(g["g_ba"]), _p(acc), 1.0 / B, 1.0, int(c["use_clipped"]), _s())
    torch.cuda.synchronize()
    g["dfeat"], g["dfeat_v"] = out["dfeat"], out["dfeat_v"]
    return out, g, acc.cpu().numpy()


def _check_act(c, val, lp, ent):
    tol = max(2 * c["torch_fp32_err"], 1e-5)
    ref = c["ref"]
    for name, got in (("value", val), ("logp", lp), ("entropy", ent)):
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref[name]).max())
        print(f"{name}: max err {err:.3e} (tol {tol:.2e}, torch fp32 {c['torch_fp32_err']:.1e})")
        assert err <= tol, (name, err, tol)


# ------------------------------------------------------------------------ act
@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_cat_act_kernel_vs_float64(gpu, case):
    """ppo_heads_act evaluating the given actions: value, log-prob and entropy vs
    float64 from the same fp32 inputs.  Tolerance: twice the worst error of torch's
    own fp32 FixedCategorical.log_probs (CPU) against float64 on these inputs, floor
    1e-5 (test_gauss_act_kernel_vs_float64's rule), recomputed at run time; the
    yardstick is below 2.1e-6 on every case, so the bound is the floor."""
    H, A, B = case[:3]
    c = C.build_case(*case)
    val, act, lp, ent = _run_act(gpu, c, B, H, A, given=c["actions"][c["sr"]])
    assert np.array_equal(act.cpu().numpy(), c["actions"][c["sr"]])
    _check_act(c, val, lp, ent)


def _tie_case():
    g = np.random.default_rng(9)
    H, A, N = 64, 9, 37
    f32 = lambda x: np.ascontiguousarray(x, np.float32)  # noqa: E731
    wa = f32(g.uniform(-1, 1, (A, H)) * 0.5)
    wa[7] = wa[3]
    ba = f32(g.normal(size=A) * 0.1)
    ba[3] = ba[7] = 8.0        # |other logits| <= 0.5 * 64 / 8 + 0.4: rows 3 and 7 lead by > 3
    return {"feat": f32(g.uniform(-1, 1, (N, H))), "wc": f32(g.uniform(-1, 1, H)), "bc": f32([0.1]), "wa": wa,
            "ba": ba}, N, H, A


@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_cat_sample_and_mode_exact(gpu, case):
    """Host noise: action == float64 argmax(p / E) on every row; deterministic:
    action == float64 argmax p on every row (the builder keeps the two largest
    scores of each row >= 2e-5 apart; at A = 1 both are 0), and the returned log-prob
    is that action's."""
    H, A, B = case[:3]
    c = C.build_case(*case)
    ref = c["ref"]
    for name, kw in (("sample", {"noise": c["noise"]}), ("mode", {"deterministic": 1})):
        val, act, lp, ent = _run_act(gpu, c, B, H, A, **kw)
        a = act.cpu().numpy()
        assert np.array_equal(a, ref[name]), (name, np.flatnonzero(a != ref[name]))
        want = np.take_along_axis(c["cat"]["norm_logits"], ref[name][:, None], -1)[:, 0]
        assert np.abs(lp.cpu().numpy() - want).max() <= max(2 * c["torch_fp32_err"], 1e-5)
    assert (ref["sample"] != ref["mode"]).any() or B == 1


def test_cat_mode_tie_takes_the_first_maximum(gpu):
    """A = 9 with weight rows 3 and 7 identical and the largest bias on both: their
    probabilities are equal bit for bit and the mode is 3 on every row
    (torch.argmax's first-maximum rule)."""
    c, N, H, A = _tie_case()
    z = c["feat"].astype(np.float64) @ c["wa"].astype(np.float64).T + c["ba"]
    assert (z[:, 3] == z[:, 7]).all() and (np.delete(z, (3, 7), 1).max(1) < z[:, 3] - 3).all()
    _, act, lp, _ = _run_act(gpu, c, N, H, A, deterministic=1)
    assert (act.cpu().numpy() == 3).all(), act
    assert torch.isfinite(lp).all()


@pytest.mark.parametrize("N,A", [(9001, 8), (9001, 5), (33001, 8), (33001, 5)])
def test_cat_act_many_rows_per_wave(gpu, N, A):
    """rows_per_wave = 3 with a ragged last block (N = 9,001) and the cap of 8
    (N = 33,001), FAST (A = 8) and generic (A = 5) at H = 64: value, log-prob and
    entropy of given actions within the act test's bound, host-noise actions and the
    mode equal to float64's on every row."""
    H = 64
    c = C.build_act_case(N, H, A)
    print("seed", c["seed"], "margins", c["margins"])
    val, act, lp, ent = _run_act(gpu, c, N, H, A, given=c["given"])
    _check_act(c, val, lp, ent)
    for name, kw in (("sample", {"noise": c["noise"]}), ("mode", {"deterministic": 1})):
        val, act, lp, ent = _run_act(gpu, c, N, H, A, **kw)
        a = act.cpu().numpy()
        assert np.array_equal(a, c["ref"][name]), (name, np.flatnonzero(a != c["ref"][name])[:8])
        assert np.abs(val.cpu().numpy() - c["ref"]["value"]).max() <= 1e-5


# ---------------------------------------------------------------------- train
@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_cat_train_kernel_vs_float64(gpu, case):
    """ppo_heads_train + ppo_heads_reduce: dfeat, dfeat_v and the head gradients vs
    the float64 helper, max |err| <= 1e-5 * max(max|ref|, 1e-3) per tensor; losses
    rtol 2e-5, atol 1e-6; no bad action counted; no NaN left in any partial; a second
    identical launch gives bit-identical partials and dfeat."""
    c = C.build_case(*case)
    out, g, acc = _run_train(gpu, c)
    out2, _, _ = _run_train(gpu, c)
    for k in ("part_w", "part_b", "part_l", "dfeat"):
        assert not torch.isnan(out[k]).any(), k
        assert torch.equal(out[k], out2[k]), k
    assert float(out["part_l"].view(-1, 4)[:, 3].sum()) == 0.0 and acc[3] == 0.0
    C.check_grads(g, c["ref"])
    print("losses", acc[:3], "ref", c["ref"]["losses"])
    C.check_losses(acc, c["ref"]["losses"])


def _errs(g, ref):
    return {k: float(np.abs(g[k].cpu().numpy().astype(np.float64) - ref[k]).max())
            for k in ("dfeat", "g_wc", "g_bc", "g_wa", "g_ba")}


@pytest.mark.parametrize("case", C.LDS_CASES, ids=[C.case_id(c) for c in C.LDS_CASES])
def test_cat_lds_register_and_unaligned_agree(gpu, case):
    """The (512, 8) cases through the LDS-weight kernel, through the register kernel
    (heads_lds = 0), and through launch_train's alignment fallback (feat, then dfeat,
    4 bytes into a larger buffer): each meets the float64 bounds, and the paths agree
    with each other within twice the larger of their float64 errors."""
    c = C.build_case(*case)
    ref = c["ref"]
    runs = {"lds": {}, "register": {"lds": 0}, "feat+4": {"feat_off": True}, "dfeat+4": {"dfeat_off": True}}
    got, err = {}, {}
    for name, kw in runs.items():
        out, g, acc = _run_train(gpu, c, **kw)
        print(name)
        C.check_grads(g, ref)
        C.check_losses(acc, ref["losses"])
        assert acc[3] == 0.0
        got[name], err[name] = g, _errs(g, ref)
    names = list(runs)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            for k in err[a]:
                d = float((got[a][k].double() - got[b][k].double()).abs().max())
                assert d <= 2 * max(err[a][k], err[b][k]), (a, b, k, d, err[a][k], err[b][k])
    # the fallback is the register kernel: same arithmetic, so the same bits
    for k in err["register"]:
        assert torch.equal(got["register"][k], got["feat+4"][k]) and torch.equal(got["register"][k], got["dfeat+4"][k])


SATURATED = [((512, 8, 130, "idx", False, 1, True), 1), ((512, 8, 130, "idx", False, 1, True), 0),
             ((64, 16, 130, "idx", False, 1, True), None)]
ZSAT = 54.0


@pytest.mark.parametrize("case,lds", SATURATED, ids=["512-8-lds", "512-8-register", "64-16"])
def test_cat_saturated_logits_stay_finite(gpu, case, lds):
    """wa scaled by 54 / sqrt(H): logits reach about +-65 and exp(nl - max) underflows
    to exactly 0 in fp32 for some actions (nl < -104).  Every output of act, train and
    reduce is finite; log-prob and entropy within max(2 * torch fp32 error, 1e-5) *
    max(1, max|ref|); gradients and losses by the usual rule.  Measured: log-prob
    error 1.5e-5 (bound 3.1e-3), entropy 3.2e-6 (2.8e-5); the worst gradient tensor
    is dfeat at 0.60 of its bound (5.6e-7 of 9.3e-7, H = 512), where torch's own CPU
    fp32 autograd is at 1.03 of it, so this bound has little room at these logits."""
    H, A, B = case[:3]
    c = C.build_case(*case, zscale=ZSAT)
    nl = c["cat"]["norm_logits"]
    assert 50.0 < c["zmax"] < 80.0 and (nl < -104).any(), (c["zmax"], nl.min())
    val, act, lp, ent = _run_act(gpu, c, B, H, A, given=c["actions"][c["sr"]])
    for x in (val, lp, ent):
        assert torch.isfinite(x).all()
    tol = max(2 * c["torch_fp32_err"], 1e-5)
    for name, got in (("logp", lp), ("entropy", ent)):
        r = c["ref"][name]
        err = float(np.abs(got.cpu().numpy() - r).max())
        bound = tol * max(1.0, float(np.abs(r).max()))
        print(f"{name}: max err {err:.3e} bound {bound:.3e} (torch fp32 {c['torch_fp32_err']:.1e})")
        assert err <= bound, (name, err, bound)
    out, g, acc = _run_train(gpu, c, lds=lds)
    for name, x in list(out.items()) + list(g.items()):
        if x is not None:
            assert torch.isfinite(x).all(), name
    assert np.isfinite(acc).all() and acc[3] == 0.0
    C.check_grads(g, c["ref"])
    C.check_losses(acc, c["ref"]["losses"])


BAD_CASES = [(512, 8, 130, "idx", False, 1, True), (64, 3, 37, "idx", False, 1, True)]


@pytest.mark.parametrize("case", BAD_CASES, ids=["lds", "generic"])
def test_cat_int64_action_outside_int32_counts_as_bad(gpu, case):
    """Stored actions -1, A, 16, 2^32 + 2 and -2^32 + 1 (the last two are 2 and 1 in
    their low 32 bits) at known rows: the train kernel counts exactly 5 bad actions
    (part_loss slot 3) and ppo_heads_act returns a NaN log-prob on those rows and a
    finite one on every other row, as the reference's gather raises there."""
    H, A, B = case[:3]
    c = C.build_case(*case)
    bad = [-1, A, 16, 2 ** 32 + 2, -2 ** 32 + 1]
    at = [0, 7, 19, 30, B - 1]
    acts = c["actions"].copy()
    acts[c["sr"][at]] = bad
    out, g, acc = _run_train(gpu, c, actions=acts)
    assert float(out["part_l"].view(-1, 4)[:, 3].sum()) == 5.0 and acc[3] == 5.0
    val, act, lp, ent = _run_act(gpu, c, B, H, A, given=acts[c["sr"]])
    nan = torch.isnan(lp).cpu().numpy()
    assert np.array_equal(np.flatnonzero(nan), np.array(at)), np.flatnonzero(nan)
    assert torch.isfinite(val).all() and torch.isfinite(ent).all()


# ----------------------------------------------------------------------- mean
@pytest.mark.parametrize("n", [1, 255, 257, 100003])
def test_mean_f32_vs_float64(gpu, n):
    """ppo_mean_f32 (the entropy mean of evaluate_actions) sums in double, so only the
    final rounding to fp32 remains: |got - ref| <= 2^-23 |ref|."""
    x = np.random.default_rng(n).uniform(0.5, 1.5, n).astype(np.float32)
    out = torch.full((1,), NAN, device=gpu)
    xd = _dev(x)
    _hip().call("ppo_mean_f32", xd.data_ptr(), n, out.data_ptr(), _s())
    ref = x.astype(np.float64).mean()
    got = float(out.cpu()[0])
    print(f"n {n}: got {got!r} ref {ref!r} rel err {abs(got - ref) / ref:.2e}")
    assert abs(got - ref) <= 2.0 ** -23 * abs(ref)


# ------------------------------------------------------------------- sampling
def test_device_sampling_distribution_amax16(gpu):
    """test_device_sampling_distribution at A = 11 (the AMAX = 16 act kernel), H = 64:
    empirical action frequencies of the counter RNG match probs within 0.005."""
    Hh = _hip()
    N, Hp, A = 200000, 64, 11
    f = torch.zeros(N, Hp, device=gpu)
    f[:, 0] = 1.0
    wa = torch.zeros(A, Hp, device=gpu)
    wa[:, 0] = torch.linspace(-1, 1.5, A, device=gpu)
    ba = torch.zeros(A, device=gpu)
    wc, bc = torch.zeros(Hp, device=gpu), torch.zeros(1, device=gpu)
    act = torch.full((N,), -1, dtype=torch.int64, device=gpu)
    Hh.call("ppo_heads_act", f.data_ptr(), None, N, Hp, wc.data_ptr(), bc.data_ptr(), wa.data_ptr(), ba.data_ptr(), A,
            None, 1234, 1, 0, None, None, act.data_ptr(), None, None, _s())
    a = act.cpu().numpy()
    assert a.min() >= 0 and a.max() < A
    freq = np.bincount(a, minlength=A) / N
    p = torch.softmax(torch.linspace(-1, 1.5, A), 0).numpy()
    print("max |freq - p|", np.abs(freq - p).max())
    assert np.abs(freq - p).max() < 0.005


# --------------------------------------------------------------------- engine
def test_mlp_minibatch_unclipped_value_loss_vs_oracle(gpu):
    """test_mlp_minibatch_grads_vs_oracle's (5, 3, 128, 6, 37) minibatch of an MLPBase
    Discrete(6) policy with use_clipped_value_loss False, against
    O.loss_head_grads(..., use_clipped_value_loss=False): max |err| <= 1e-5 *
    max(max|grad|, 1e-3) per tensor, losses rtol 2e-5 / atol 1e-6; the value loss
    differs from the clipped one on these inputs."""
    from a2c_ppo_acktr import model as M
    from a2c_ppo_acktr.algo.ppo import FlatAdam
    from a2c_ppo_acktr.storage import RolloutStorage
    from a2c_ppo_acktr.synthetic import Discrete
    I, V, H, A, B = 5, 3, 128, 6, 37
    torch.manual_seed(B)
    pol = M.Policy((I,), Discrete(A), base=M.MLPBase, base_kwargs={"recurrent": False, "hidden_size": H},
                   vector_obs_len=V)
    with torch.no_grad():
        pol.dist.linear.weight.mul_(20.0)
        pol.base.critic_linear.weight.mul_(3.0)
    init = torch.cat([p.detach().reshape(-1) for p in pol.parameters()]).numpy().astype(np.float64)
    pol.to(gpu)
    eng = pol.hip_engine()
    T, N = 4, (B + 1) // 2
    st = RolloutStorage(T, N, (I,), [V], Discrete(A), 1, device=gpu)
    g = torch.Generator().manual_seed(B + 1)
    st.obs.copy_(torch.randn(st.obs.shape, generator=g).to(gpu))
    st.vector_obs.copy_(torch.rand(st.vector_obs.shape, generator=g).to(gpu))
    st.actions.copy_(torch.randint(0, A, st.actions.shape, generator=g).to(gpu))
    st.action_log_probs.copy_((torch.log(torch.rand(st.action_log_probs.shape, generator=g)) * 0.3 - 1.0).to(gpu))
    st.value_preds.copy_(torch.randn(st.value_preds.shape, generator=g).to(gpu) * 0.1)
    st.returns.copy_(torch.randn(st.returns.shape, generator=g).to(gpu))
    adv = torch.randn(T, N, generator=g).to(gpu)
    idx = torch.randperm(T * N, generator=g)[:B].to(gpu)
    hp = {"clip": 0.1, "value_coef": 0.5, "entropy_coef": 0.01, "use_clipped_value_loss": False}
    loss = torch.zeros(4, dtype=torch.float64, device=gpu)
    eng.train_minibatch(st, adv, idx, hp, loss, FlatAdam(pol.parameters(), lr=0.0, eps=1e-5, max_grad_norm=None))
    torch.cuda.synchronize()
    shapes = O.mlp_param_shapes(I + V, H, A)
    p = O.unflatten(init, shapes)
    ii = idx.cpu().numpy()
    x = np.concatenate([st.obs[:-1].reshape(T * N, I).cpu().numpy()[ii],
                        st.vector_obs[:-1].reshape(T * N, V).cpu().numpy()[ii]], 1)
    value, logits, cache = O.mlp_forward(p, x.astype(np.float64))
    f = lambda t: t.reshape(-1).cpu().numpy()[ii]  # noqa: E731
    args = (value, logits, f(st.actions), f(st.action_log_probs), f(adv), f(st.value_preds[:-1]), f(st.returns[:-1]),
            0.1, 0.5, 0.01)
    lg = O.loss_head_grads(*args, use_clipped_value_loss=False)
    clipped = O.loss_head_grads(*args, use_clipped_value_loss=True)
    assert abs(clipped["value_loss"] - lg["value_loss"]) > 1e-3 * lg["value_loss"]
    grads = O.mlp_backward(p, cache, lg["g_value"], lg["g_logits"])
    got = O.unflatten(eng.grad.cpu().numpy(), shapes)
    for name, _ in shapes:
        ref = grads[name]
        err = np.abs(got[name] - ref).max()
        assert err <= 1e-5 * max(np.abs(ref).max(), 1e-3), (name, err, np.abs(ref).max())
    np.testing.assert_allclose(loss.cpu().numpy()[:3], [lg["value_loss"], lg["action_loss"], lg["entropy"]],
                               rtol=2e-5, atol=1e-6)
