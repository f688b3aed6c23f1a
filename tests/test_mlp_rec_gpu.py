"""Recurrent MLPBase on the HIP engine (model.py:111-166, 224-234: a GRU on cat(obs,
vector_obs) in front of the actor / critic towers): the two-operand data gradient
ppo_linear_dgrad_pair through the C ABI, and RecurrentMLPEngine through Policy / PPO,
against float64 (helpers/mlp_rec_ref.py, pinned by test_mlp_rec_cpu.py).

Bars are those of the tests this path's pieces already have: 1e-5 * max|ref| for a
dense kernel (test_rec_dense.py), 2e-5 absolute for forward values / log-probs /
entropy / hidden states (test_gru_golden_evaluate_and_step), 2e-5 * max(max|ref|, 1e-3)
per BPTT gradient tensor and rtol 2e-5 / atol 1e-6 for the losses
(test_recurrent_minibatch_grads_vs_oracle), 2e-2 relative Frobenius per tensor in half
mode (test_half.py).  Kernel outputs start as NaN with 64 NaN guard rows behind them."""
import functools

import numpy as np
import pytest
import torch

from helpers import mlp_rec_ref as R
from oracle import ppo_oracle as O

pytestmark = pytest.mark.gpu

GUARD = 64
CLIP, VC, EC = 0.1, 0.5, 0.01
HP = {"clip": CLIP, "value_coef": VC, "entropy_coef": EC, "use_clipped_value_loss": True}


def _hip():
    from a2c_ppo_acktr import _hip
    return _hip


def _s():
    return torch.cuda.current_stream().cuda_stream


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _close(name, got, ref, rel=1e-5, scale=None):
    got, ref = got.cpu().double(), ref.double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), (name, "non-finite", int((~torch.isfinite(got)).sum()))
    err, mx = (got - ref).abs().max().item(), (ref.abs().max().item() if scale is None else scale)
    print(f"{name}: max|err| {err:.3e}  max|ref| {mx:.3f}  bound {rel * mx:.3e}", flush=True)
    assert err <= rel * mx, (name, err, rel * mx)


# ------------------------------------------------------------ ppo_linear_dgrad_pair
@pytest.mark.parametrize("M,K0,K1,N", [(129, 64, 64, 64), (300, 128, 32, 128), (99, 32, 32, 32)])
def test_linear_dgrad_pair_vs_float64(gpu, M, K0, K1, N):
    """dx [M][N] = dy0 [M][K0] · W0 [K0][N] + dy1 [M][K1] · W1 [K1][N], the weights given
    transposed ([N][K] rows): one full 128-row tile plus one row at the H = 64 towers'
    shape; unequal operands over several row tiles (the k tile that holds K0 = 128 ..
    159 ends inside pair 1); the smallest legal layer (K0 = 32 = one k tile per pair).
    A second launch gives the same bits, and with dy1 = 0 the result is the one-operand
    ppo_linear_dgrad_ex's within the same bar."""
    Hh = _hip()
    g = torch.Generator().manual_seed(M + K0 + 3 * K1 + N)
    dy0, dy1 = torch.randn(M, K0, generator=g), torch.randn(M, K1, generator=g)
    W0 = torch.randn(K0, N, generator=g) / (K0 + K1) ** 0.5
    W1 = torch.randn(K1, N, generator=g) / (K0 + K1) ** 0.5
    ref = dy0.double() @ W0.double() + dy1.double() @ W1.double()
    d0, d1, t0, t1 = dy0.cuda(), dy1.cuda(), W0.t().contiguous().cuda(), W1.t().contiguous().cuda()
    runs = []
    for _ in range(2):
        dx = _nan(M + GUARD, N)
        Hh.call("ppo_linear_dgrad_pair", d0.data_ptr(), t0.data_ptr(), K0, d1.data_ptr(), t1.data_ptr(), K1, M, N,
                dx.data_ptr(), _s())
        torch.cuda.synchronize()
        runs.append(dx)
    _close("linear_dgrad_pair", runs[0][:M], ref)
    assert torch.isnan(runs[0][M:]).all()   # nothing stored past row M
    assert torch.equal(runs[0][:M], runs[1][:M])
    z1 = torch.zeros_like(d1)
    dxz, dxe = _nan(M + GUARD, N), _nan(M + GUARD, N)
    Hh.call("ppo_linear_dgrad_pair", d0.data_ptr(), t0.data_ptr(), K0, z1.data_ptr(), t1.data_ptr(), K1, M, N,
            dxz.data_ptr(), _s())
    Hh.call("ppo_linear_dgrad_ex", d0.data_ptr(), M, K0, t0.data_ptr(), N, None, 0, 1, dxe.data_ptr(), _s())
    torch.cuda.synchronize()
    ref0 = dy0.double() @ W0.double()
    _close("linear_dgrad_pair dy1=0", dxz[:M], ref0)
    _close("pair(dy1=0) vs dgrad_ex", dxz[:M], dxe[:M].cpu(), scale=ref0.abs().max().item())
    assert torch.isnan(dxz[M:]).all()


@pytest.mark.parametrize("key,value", [("x9", 0), ("products", 9), ("products", 1)])
def test_linear_dgrad_pair_honours_the_knobs(gpu, key, value):
    """The run-time knobs of the dense kernels reach the pair dgrad: x9 = 0 (the fp32-MFMA
    tile core) and products = 9 are fp32 arithmetic and meet the 1e-5 bar; products = 1
    (Policy.half(): bf16-rounded operands, 2^-9 relative each) differs from float64 by more
    than that bar and by at most test_half.py's 2e-2 relative Frobenius error."""
    Hh = _hip()
    M, K0, K1, N = 300, 128, 32, 128
    g = torch.Generator().manual_seed(9)
    dy0, dy1 = torch.randn(M, K0, generator=g), torch.randn(M, K1, generator=g)
    W0, W1 = torch.randn(K0, N, generator=g) / 160 ** 0.5, torch.randn(K1, N, generator=g) / 160 ** 0.5
    ref = dy0.double() @ W0.double() + dy1.double() @ W1.double()
    d0, d1, t0, t1 = dy0.cuda(), dy1.cuda(), W0.t().contiguous().cuda(), W1.t().contiguous().cuda()
    dx = _nan(M + GUARD, N)
    prev = Hh.call("ppo_tune_get", key.encode())
    Hh.call("ppo_tune_set", key.encode(), value)
    try:
        Hh.call("ppo_linear_dgrad_pair", d0.data_ptr(), t0.data_ptr(), K0, d1.data_ptr(), t1.data_ptr(), K1, M, N,
                dx.data_ptr(), _s())
        torch.cuda.synchronize()
    finally:
        Hh.call("ppo_tune_set", key.encode(), prev)
    assert torch.isnan(dx[M:]).all()
    got = dx[:M].cpu().double()
    if (key, value) == ("products", 1):
        err = (got - ref).abs().max().item()
        fro = ((got - ref).norm() / ref.norm()).item()
        print(f"products=1: max|err| {err:.3e}  relative Frobenius error {fro:.3e}", flush=True)
        assert torch.isfinite(got).all() and err > 1e-5 * ref.abs().max().item() and fro <= 2e-2
    else:
        _close(f"linear_dgrad_pair {key}={value}", got, ref)


@pytest.mark.parametrize("K0,K1", [(6, 64), (64, 6), (0, 64), (64, 0), (-4, 64)])
def test_linear_dgrad_pair_rejects_bad_k(gpu, K0, K1):
    """K0, K1 must be positive multiples of 4: PPO_EARG (1001), and nothing is launched"""
    Hh = _hip()
    M, N = 40, 64
    d, t = torch.zeros(M, 64, device=gpu), torch.zeros(N, 64, device=gpu)
    dx = _nan(M, N)
    with pytest.raises(Hh.HipError, match=r"\(1001\)"):
        Hh.call("ppo_linear_dgrad_pair", d.data_ptr(), t.data_ptr(), K0, d.data_ptr(), t.data_ptr(), K1, M, N,
                dx.data_ptr(), _s())
    torch.cuda.synchronize()
    assert torch.isnan(dx).all()


# ------------------------------------------------------------------ policies, inputs
def _space(kind, A):
    from a2c_ppo_acktr.synthetic import Box, Discrete, MultiBinary
    return {"cat": lambda: Discrete(A), "gauss": lambda: Box(-1.0, 1.0, (A,)), "bern": lambda: MultiBinary(A)}[kind]()


def _policy(I0, V, H, A, kind="cat", seed=0):
    """A recurrent MLPBase policy on the CPU with the head weights scaled as
    test_mlp_minibatch_grads_vs_oracle scales them (dist x 20, critic_linear x 3) and
    non-zero GRU biases (the constructor zeroes them)."""
    from a2c_ppo_acktr import model as M
    torch.manual_seed(seed)
    pol = M.Policy((I0,), _space(kind, A), base=M.MLPBase, base_kwargs={"recurrent": True, "hidden_size": H},
                   vector_obs_len=V)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        (pol.dist.fc_mean if kind == "gauss" else pol.dist.linear).weight.mul_(20.0)
        pol.base.critic_linear.weight.mul_(3.0)
        pol.base.gru.bias_ih_l0.uniform_(-0.3, 0.3, generator=g)
        pol.base.gru.bias_hh_l0.uniform_(-0.3, 0.3, generator=g)
        if kind == "gauss":
            pol.dist.logstd._bias.copy_(torch.linspace(-1.0, 0.5, A).view(A, 1))
    return pol


def _params(pol):
    return [p.detach().cpu().clone() for p in pol.parameters()]


def _names(pol):
    return [n for n, _ in pol.named_parameters()]


def _rows_x(c, rows):
    T, N = c["T"], c["N"]
    x = torch.cat([c["obs"][:T].reshape(T * N, c["I0"]), c["vec"][:T].reshape(T * N, c["V"])], 1)
    return x[rows].double().numpy()


@functools.lru_cache(maxsize=None)
def _train_case(T, N, n, I0, V, H, A, kind):
    """Storage planes (fp32, CPU), an out-of-order choice of n env lanes, and the float64
    minibatch reference, computed once per configuration.  Stored actions are the kind a
    rollout stores (Box: within 3 sigma of the float64 mean) and the stored log-probs sit
    0.15 sigma around the float64 log-probs, so ratios fall on both sides of the clip."""
    seed = 100 * T + N + H + A + {"cat": 0, "gauss": 1000, "bern": 2000}[kind]
    pol = _policy(I0, V, H, A, kind, seed)
    params = _params(pol)
    g = torch.Generator().manual_seed(seed + 7)
    c = {"T": T, "N": N, "n": n, "I0": I0, "V": V, "H": H, "A": A, "kind": kind, "seed": seed, "params": params,
         "names": _names(pol)}
    c["obs"] = torch.randn(T + 1, N, I0, generator=g)
    c["vec"] = torch.rand(T + 1, N, V, generator=g)
    c["hxs0"] = 0.5 * torch.randn(N, H, generator=g)
    c["masks"] = (torch.rand(T + 1, N, 1, generator=g) > 0.2).float()
    c["value_preds"] = 0.1 * torch.randn(T + 1, N, 1, generator=g)
    c["returns"] = torch.randn(T + 1, N, 1, generator=g)
    c["adv"] = torch.randn(T, N, generator=g)
    envs = torch.randperm(N, generator=g)[:n]
    assert not torch.equal(envs, envs.sort().values)
    c["envs"] = envs
    rows = (torch.arange(T)[:, None] * N + envs[None, :]).reshape(-1)
    c["rows"] = rows
    x, h0, m = _rows_x(c, rows), c["hxs0"][envs].double().numpy(), c["masks"][:T, :, 0][:, envs].double().numpy()
    assert (m[1:] == 0).any()
    _, out, _ = R.forward(params, kind, x, h0, m)
    if kind == "cat":
        acts = torch.randint(0, A, (T, N, 1), generator=g)
    elif kind == "bern":
        acts = (torch.rand(T, N, A, generator=g) < 0.5).float()
    else:
        acts = torch.zeros(T * N, A)
        sigma = params[16].view(1, A).exp()
        acts[rows] = torch.from_numpy(out).float() + sigma * torch.randn(T * n, A, generator=g).clamp(-3, 3)
        acts = acts.view(T, N, A)
    c["actions"] = acts
    a_rows = acts.reshape(T * N, -1)[rows].numpy()
    lp, _ = R.logp_entropy(params, kind, out, a_rows)
    olp = torch.zeros(T * N)
    olp[rows] = torch.from_numpy(lp).float() + 0.15 * torch.randn(T * n, generator=g)
    c["old_logp"] = olp.view(T, N, 1)
    f = lambda t: t.reshape(-1)[rows].double().numpy()  # noqa: E731
    ref = R.minibatch(params, kind, x, h0, m, a_rows, f(c["old_logp"]), f(c["adv"]), f(c["value_preds"][:T]),
                      f(c["returns"][:T]), CLIP, VC, EC)
    ratio = np.exp(ref["logp"] - f(c["old_logp"]))
    outside = (ratio < 1 - CLIP) | (ratio > 1 + CLIP)
    assert outside.any() and (~outside).any()
    c["ref"] = ref
    return c


def _storage(gpu, c):
    from a2c_ppo_acktr.storage import RolloutStorage
    st = RolloutStorage(c["T"], c["N"], (c["I0"],), [c["V"]], _space(c["kind"], c["A"]), c["H"], device=gpu)
    st.obs.copy_(c["obs"])
    if c["V"]:
        st.vector_obs.copy_(c["vec"])
    st.recurrent_hidden_states[0].copy_(c["hxs0"])
    st.masks.copy_(c["masks"])
    st.actions.copy_(c["actions"])
    st.action_log_probs.copy_(c["old_logp"])
    st.value_preds.copy_(c["value_preds"])
    st.returns.copy_(c["returns"])
    return st


def _run_minibatch(gpu, c, pol, st):
    """one train_minibatch_rec at lr = 0 -> (per-parameter gradients, losses)"""
    from a2c_ppo_acktr.algo.ppo import FlatAdam
    eng = pol.hip_engine()
    loss = torch.zeros(4, dtype=torch.float64, device=gpu)   # 3 losses + bad-action count
    opt = FlatAdam(pol.parameters(), lr=0.0, eps=1e-5, max_grad_norm=None)
    eng.train_minibatch_rec(st, c["adv"].to(gpu), c["envs"].to(gpu), HP, loss, opt)
    torch.cuda.synchronize()
    assert eng.status.tolist() == [0, 0, 0, 0]
    assert loss[3].item() == 0
    grads = torch.split(eng.grad.detach().cpu().double(), [p.numel() for p in pol.parameters()])
    return [g.numpy() for g in grads], loss[:3].cpu().numpy()


def _check_fp32(c, grads, losses):
    for name, got, ref in zip(c["names"], grads, c["ref"]["grads"]):
        ref = ref.reshape(-1)
        err, mx = np.abs(got - ref).max(), np.abs(ref).max()
        print(f"{name}: max|err| {err:.3e}  max|grad| {mx:.3e}  bound {2e-5 * max(mx, 1e-3):.3e}", flush=True)
        assert err <= 2e-5 * max(mx, 1e-3), (name, err, mx)
    print("losses", losses, "ref", c["ref"]["losses"], flush=True)
    np.testing.assert_allclose(losses, c["ref"]["losses"], rtol=2e-5, atol=1e-6)


# ------------------------------------------------------------ forward through Policy
@functools.lru_cache(maxsize=None)
def _forward_case(I0, V, H, A):
    T, N = 5, 35
    pol = _policy(I0, V, H, A, "cat", seed=I0 + H)
    params = _params(pol)
    g = torch.Generator().manual_seed(I0 + V + H + A)
    obs = torch.randn(T * N, I0, generator=g)
    vec = torch.rand(T * N, V, generator=g)
    h0 = 0.5 * torch.randn(N, H, generator=g)
    masks = (torch.rand(T * N, 1, generator=g) > 0.2).float()
    acts = torch.randint(0, A, (T * N, 1), generator=g)
    # a reset in the second 32-row group after the first step, and resets overall ~20 %
    assert (masks.view(T, N)[1:, 32:] == 0).any() and 0.1 < (masks == 0).float().mean() < 0.3
    x = torch.cat([obs, vec], 1).double().numpy()
    value, logits, hs = R.forward(params, "cat", x, h0.double().numpy(), masks.view(T, N).double().numpy())
    top2 = np.sort(logits, 1)[:, -2:]
    decided = (top2[:, 1] - top2[:, 0]) > 1e-4
    assert decided.mean() >= 0.9 and decided[:N].mean() >= 0.9, (decided.mean(), decided[:N].mean())
    cat = O.categorical(logits)
    return dict(T=T, N=N, seed=I0 + H, obs=obs, vec=vec, h0=h0, masks=masks, acts=acts, value=value, logits=logits,
                hs=hs, decided=decided, nl=cat["norm_logits"], ent=cat["entropy"])


@pytest.mark.parametrize("I0,V,H,A", [(4, 0, 64, 2), (5, 2, 32, 6)])
def test_forward_through_policy_vs_float64(gpu, I0, V, H, A):
    """act(deterministic), get_value, evaluate_actions single-step (R == N) and the T = 5,
    N = 35 sequence branch: H = 64 with I = 4 (the persistent GRU kernels) and H = 32 with
    I = 7 -> Ip = 8 (live input padding, vector observations).  Value, log-prob, mean
    entropy and the returned hidden state within 2e-5; the deterministic action is
    float64's argmax wherever its top-two logit gap exceeds 1e-4 (>= 90 % of the rows)."""
    c = _forward_case(I0, V, H, A)
    T, N = c["T"], c["N"]
    pol = _policy(I0, V, H, A, "cat", seed=c["seed"]).to(gpu)
    assert type(pol.hip_engine()).__name__ == "RecurrentMLPEngine"
    d = lambda t: t.to(gpu)  # noqa: E731
    obs, masks, acts, h0 = d(c["obs"]), d(c["masks"]), d(c["acts"]), d(c["h0"])
    vec = d(c["vec"]) if V else None
    a_np = c["acts"].numpy()[:, 0]
    lp_ref = np.take_along_axis(c["nl"], a_np[:, None], 1)[:, 0]

    def near(name, got, ref):
        got = got.detach().cpu().numpy().reshape(np.shape(ref))
        err = np.abs(got - ref).max()
        print(f"{name}: max|err| {err:.3e} (bound 2e-5)", flush=True)
        assert np.isfinite(got).all() and err <= 2e-5, (name, err)

    # sequence branch
    value, logp, ent, hT = pol.evaluate_actions(obs, vec, h0, masks, acts)
    assert value.shape == (T * N, 1) and logp.shape == (T * N, 1) and hT.shape == (N, H)
    near("seq value", value, c["value"][:, None])
    near("seq logp", logp, lp_ref[:, None])
    near("seq entropy", ent, c["ent"].mean())
    near("seq hidden", hT, c["hs"][(T - 1) * N:])
    # single step: the first N rows
    v1, lp1, e1, h1 = pol.evaluate_actions(obs[:N], None if vec is None else vec[:N], h0, masks[:N], acts[:N])
    near("step value", v1, c["value"][:N, None])
    near("step logp", lp1, lp_ref[:N, None])
    near("step entropy", e1, c["ent"][:N].mean())
    near("step hidden", h1, c["hs"][:N])
    near("get_value", pol.get_value(obs[:N], None if vec is None else vec[:N], h0, masks[:N]), c["value"][:N, None])
    va, a, lpa, ha = pol.act(obs[:N], None if vec is None else vec[:N], h0, masks[:N], deterministic=True)
    near("act value", va, c["value"][:N, None])
    near("act hidden", ha, c["hs"][:N])
    ok = c["decided"][:N]
    best = c["logits"][:N].argmax(1)
    assert a.dtype == torch.int64 and np.array_equal(a.cpu().numpy()[ok, 0], best[ok])
    near("act logp", lpa[torch.from_numpy(ok).to(gpu)], c["nl"][:N].max(1)[ok][:, None])
    assert pol.hip_engine().status.tolist() == [0, 0, 0, 0]


# ------------------------------------------------------ one minibatch vs float64
_SHAPES = [(6, 40, 33, 4, 0, 64, 2), (3, 5, 3, 5, 2, 32, 6)]


@pytest.mark.parametrize("T,N,n,I0,V,H,A,kind", [_SHAPES[0] + ("cat",), _SHAPES[1] + ("cat",),
                                                 _SHAPES[0][:6] + (3, "gauss"), _SHAPES[0][:6] + (3, "bern")],
                         ids=["h64-cat", "h32-vec-cat", "h64-box", "h64-multibinary"])
def test_train_minibatch_rec_grads_vs_float64(gpu, T, N, n, I0, V, H, A, kind):
    """One recurrent_generator minibatch (input gather + concat + padding, gi, the GRU
    over T with masks, both towers, heads / loss, tower backward, the pair dgrad, BPTT,
    every weight gradient) at lr = 0 vs float64 autograd.  h64: 33 of 40 lanes out of
    order over T = 6 — two 32-row GRU groups with a one-row tail, 198 rows across a
    128-row tile; h32-vec: I = 7 -> Ip = 8 with vector observations.  The first shape
    again with a Box and a MultiBinary head (A = 3)."""
    c = _train_case(T, N, n, I0, V, H, A, kind)
    pol = _policy(I0, V, H, A, kind, c["seed"]).to(gpu)
    grads, losses = _run_minibatch(gpu, c, pol, _storage(gpu, c))
    _check_fp32(c, grads, losses)


def test_half_mode_minibatch_and_back(gpu):
    """Policy.half(): the first shape's gradients within test_half.py's bar (relative
    Frobenius error <= 2e-2 per tensor against float64); Policy.float() restores the fp32
    bar."""
    c = _train_case(*_SHAPES[0], "cat")
    pol = _policy(*_SHAPES[0][3:], "cat", c["seed"]).to(gpu)
    st = _storage(gpu, c)
    assert pol.half() is pol and pol.half_precision
    grads, losses = _run_minibatch(gpu, c, pol, st)
    for name, got, ref in zip(c["names"], grads, c["ref"]["grads"]):
        fro = np.linalg.norm(got - ref.reshape(-1)) / max(np.linalg.norm(ref), 1e-12)
        print(f"{name:28s} half-mode relative Frobenius error {fro:.2e}", flush=True)
        assert fro <= 2e-2, (name, fro)
    np.testing.assert_allclose(losses, c["ref"]["losses"], rtol=2e-2, atol=1e-4)
    pol.float()
    assert not pol.half_precision
    grads, losses = _run_minibatch(gpu, c, pol, st)
    _check_fp32(c, grads, losses)


# -------------------------------------------------------------------- PPO.update
@functools.lru_cache(maxsize=None)
def _update_case():
    """T = 8, N = 8, H = 64 Discrete(2) rollout planes and, for the permutations that
    torch.manual_seed(77) gives PPO.update, the float64 mean losses of its 2 x 2
    minibatches at fixed parameters (lr = 0)."""
    T, N, I0, V, H, A, E, Mb = 8, 8, 4, 0, 64, 2, 2, 2
    seed = 41
    pol = _policy(I0, V, H, A, "cat", seed)
    params = _params(pol)
    g = torch.Generator().manual_seed(seed + 7)
    c = {"T": T, "N": N, "n": N, "I0": I0, "V": V, "H": H, "A": A, "kind": "cat", "seed": seed, "E": E, "Mb": Mb}
    c["obs"] = torch.randn(T + 1, N, I0, generator=g)
    c["vec"] = torch.zeros(T + 1, N, 0)
    c["hxs0"] = 0.5 * torch.randn(N, H, generator=g)
    c["masks"] = (torch.rand(T + 1, N, 1, generator=g) > 0.2).float()
    c["value_preds"] = 0.1 * torch.randn(T + 1, N, 1, generator=g)
    c["returns"] = torch.randn(T + 1, N, 1, generator=g)
    c["actions"] = torch.randint(0, A, (T, N, 1), generator=g)
    allrows = torch.arange(T * N)
    x, m = _rows_x(c, allrows), c["masks"][:T, :, 0].double().numpy()
    _, out, _ = R.forward(params, "cat", x, c["hxs0"].double().numpy(), m)
    lp, _ = R.logp_entropy(params, "cat", out, c["actions"].reshape(-1).numpy())
    c["old_logp"] = (torch.from_numpy(lp).float() + 0.15 * torch.randn(T * N, generator=g)).view(T, N, 1)
    adv = O.normalize_advantages(c["returns"][:, :, 0].numpy(), c["value_preds"][:, :, 0].numpy())   # [T, N] fp32
    state = torch.get_rng_state()
    torch.manual_seed(77)
    perms = [torch.randperm(N) for _ in range(E)]
    c["rng_after"] = torch.get_rng_state()
    torch.set_rng_state(state)
    losses = []
    for perm in perms:
        for envs in O.rec_minibatches(perm.numpy(), Mb):
            rows = (np.arange(T)[:, None] * N + envs[None, :]).reshape(-1)
            f = lambda t: np.asarray(t, np.float64).reshape(-1)[rows]  # noqa: E731
            r = R.minibatch(params, "cat", x[rows], c["hxs0"].double().numpy()[envs], m[:, envs],
                            c["actions"].reshape(-1).numpy()[rows], f(c["old_logp"]), f(adv),
                            f(c["value_preds"][:T]), f(c["returns"][:T]), CLIP, VC, EC)
            losses.append(r["losses"])
    c["losses"] = np.mean(losses, 0)
    return c


def test_ppo_update_losses_and_rng(gpu):
    """PPO.update of a recurrent MLP policy at lr = 0 (2 epochs x 2 minibatches of 4 whole
    env sequences): the returned mean losses equal float64's over the same
    torch.randperm(N) env sets, and the default CPU generator ends where exactly
    ppo_epoch calls of torch.randperm(N) leave it.  With lr = 2.5e-4: four optimizer
    steps, finite parameters, and the GRU, both towers and the heads all move."""
    from a2c_ppo_acktr.algo import PPO
    c = _update_case()
    st = _storage(gpu, c)
    pol = _policy(c["I0"], c["V"], c["H"], c["A"], "cat", c["seed"]).to(gpu)
    before = _params(pol)
    agent = PPO(pol, CLIP, c["E"], c["Mb"], VC, EC, lr=0.0, eps=1e-5, max_grad_norm=0.5)
    torch.manual_seed(77)
    losses = agent.update(st)
    print("update losses", losses, "ref", c["losses"], flush=True)
    assert torch.equal(torch.get_rng_state(), c["rng_after"])
    np.testing.assert_allclose(losses, c["losses"], rtol=2e-5, atol=1e-6)
    assert all(torch.equal(a, b) for a, b in zip(before, _params(pol)))   # lr = 0
    assert agent.optimizer.step_count == 4

    pol = _policy(c["I0"], c["V"], c["H"], c["A"], "cat", c["seed"]).to(gpu)
    agent = PPO(pol, CLIP, c["E"], c["Mb"], VC, EC, lr=2.5e-4, eps=1e-5, max_grad_norm=0.5)
    torch.manual_seed(77)
    losses = agent.update(st)
    assert all(np.isfinite(losses)) and agent.optimizer.step_count == 4
    after = _params(pol)
    assert all(torch.isfinite(p).all() for p in after)
    moved = {n: not torch.equal(a, b) for n, a, b in zip(_names(pol), before, after)}
    for group in ("base.gru.", "base.actor.", "base.critic.", "base.critic_linear.", "dist."):
        assert any(v for n, v in moved.items() if n.startswith(group)), (group, moved)
    assert pol.hip_engine().status.tolist() == [0, 0, 0, 0]


# -------------------------------------------------------------------- checkpoint
def test_checkpoint_resume_is_bit_identical(gpu, tmp_path):
    """One update, checkpoint, a second rollout; then act(deterministic) and a second
    update from the live pair and from the pair restored from the file (same host RNG
    state for the env permutations): identical bits (test_checkpoint.py's pattern)."""
    from a2c_ppo_acktr import checkpoint as C
    from a2c_ppo_acktr.algo import PPO
    from a2c_ppo_acktr.storage import RolloutStorage
    from a2c_ppo_acktr.synthetic import Discrete
    N, T, I0, H, A = 8, 8, 4, 64, 2
    pol = _policy(I0, 0, H, A, "cat", seed=5).to(gpu)
    agent = PPO(pol, 0.1, 2, 2, 0.5, 0.01, lr=1e-3, eps=1e-5, max_grad_norm=0.5)
    st = RolloutStorage(T, N, (I0,), [0], Discrete(A), H, device=gpu)
    g = torch.Generator().manual_seed(6)
    frames = torch.randn(2, T + 1, N, I0, generator=g).to(gpu)
    rewards = torch.rand(2, T, N, 1, generator=g).to(gpu)
    masks = (torch.rand(2, T, N, 1, generator=g) > 0.2).float().to(gpu)
    ones = torch.ones(N, 1, device=gpu)

    def rollout(k):
        st.obs[0].copy_(frames[k, 0])
        for step in range(T):
            v, a, lp, h = pol.act(st.obs[step], st.vector_obs[step], st.recurrent_hidden_states[step], st.masks[step])
            st.insert(frames[k, step + 1], st.vector_obs[step + 1], h, a, lp, v, rewards[k, step], masks[k, step],
                      ones)
        nv = pol.get_value(st.obs[-1], st.vector_obs[-1], st.recurrent_hidden_states[-1], st.masks[-1])
        st.compute_returns(nv, True, 0.99, 0.95, False)

    rollout(0)
    agent.update(st)
    st.after_update()
    path = str(tmp_path / "ck.pt")
    C.save_checkpoint(path, pol, None, agent=agent)
    rollout(1)
    probe = (st.obs[3], None, st.recurrent_hidden_states[3], st.masks[3])
    rng = torch.get_rng_state()
    out1 = pol.act(*probe, deterministic=True)
    l1 = agent.update(st)
    p1 = torch.cat([p.detach().reshape(-1) for p in pol.parameters()]).cpu()
    pol2 = _policy(I0, 0, H, A, "cat", seed=77).to(gpu)   # (re-seeds the global generator)
    agent2 = PPO(pol2, 0.1, 2, 2, 0.5, 0.01, lr=1e-3, eps=1e-5, max_grad_norm=0.5)
    C.load_checkpoint(path, device=gpu, actor_critic=pol2, agent=agent2)
    assert type(pol2.hip_engine()).__name__ == "RecurrentMLPEngine"
    torch.set_rng_state(rng)   # same env permutations as the live run
    out2 = pol2.act(*probe, deterministic=True)
    l2 = agent2.update(st)
    p2 = torch.cat([p.detach().reshape(-1) for p in pol2.parameters()]).cpu()
    assert all(torch.equal(a, b) for a, b in zip(out1, out2))
    assert l1 == l2 and all(np.isfinite(l1))
    assert torch.equal(p1, p2)
    # a policy rebuilt from the file's recorded constructor is a recurrent MLPBase again
    pol3, _ = C.load_checkpoint(path)
    assert pol3.is_recurrent and type(pol3.base).__name__ == "MLPBase"


# ------------------------------------------------------------------------ errors
def test_unsupported_hidden_size_raises(gpu):
    """the GRU kernels' limit: hidden_size a multiple of 32 up to 512"""
    with pytest.raises(NotImplementedError, match="multiple of 32"):
        _policy(4, 0, 48, 2).to(gpu).hip_engine()


def test_wrong_hidden_width_storage_raises_before_any_launch(gpu):
    from a2c_ppo_acktr.algo.ppo import FlatAdam
    from a2c_ppo_acktr.storage import RolloutStorage
    from a2c_ppo_acktr.synthetic import Discrete
    T, N, I0, H, A = 3, 4, 4, 64, 2
    pol = _policy(I0, 0, H, A).to(gpu)
    eng = pol.hip_engine()
    st = RolloutStorage(T, N, (I0,), [0], Discrete(A), 32, device=gpu)   # hidden states of width 32
    loss = torch.zeros(4, dtype=torch.float64, device=gpu)
    opt = FlatAdam(pol.parameters(), lr=1e-3, eps=1e-5, max_grad_norm=None)
    with pytest.raises(RuntimeError, match="hidden states of width 32"):
        eng.train_minibatch_rec(st, torch.zeros(T, N, device=gpu), torch.arange(2, device=gpu), HP, loss, opt)
    torch.cuda.synchronize()
    assert not eng.ws["train"].bufs and opt.step_count == 0   # no workspace was touched, no step taken
    assert not eng.grad.any() and not loss.any()


def test_cnn_wrong_hidden_width_storage_raises_before_any_launch(gpu):
    """RecurrentEngine shares the prologue of train_minibatch_rec, so the same check guards its
    ppo_gather_rows (4 H bytes per row of the stored hidden states): nothing is launched."""
    from a2c_ppo_acktr import model as M
    from a2c_ppo_acktr.algo.ppo import FlatAdam
    from a2c_ppo_acktr.storage import RolloutStorage
    from a2c_ppo_acktr.synthetic import Discrete
    T, N, C, H, A = 3, 4, 4, 64, 2
    torch.manual_seed(0)
    pol = M.Policy((C, 84, 84), Discrete(A), base=M.CNNBase, base_kwargs={"recurrent": True, "hidden_size": H}).to(gpu)
    eng = pol.hip_engine()
    assert type(eng).__name__ == "RecurrentEngine"
    st = RolloutStorage(T, N, (C, 84, 84), [0], Discrete(A), 32, obs_dtype=torch.uint8, device=gpu)
    loss = torch.zeros(4, dtype=torch.float64, device=gpu)
    opt = FlatAdam(pol.parameters(), lr=1e-3, eps=1e-5, max_grad_norm=None)
    with pytest.raises(RuntimeError, match="hidden states of width 32"):
        eng.train_minibatch_rec(st, torch.zeros(T, N, device=gpu), torch.arange(2, device=gpu), HP, loss, opt)
    torch.cuda.synchronize()
    assert not eng.ws["train"].bufs and opt.step_count == 0   # no workspace was touched, no step taken
    assert not eng.grad.any() and not loss.any()
