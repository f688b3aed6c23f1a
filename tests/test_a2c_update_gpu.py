"""A2C_ACKTR.update end to end on the four engines against a float64 restatement
(tests/helpers/a2c_ref.update_reference: autograd of algo/a2c_acktr.py:45-51, 71-72 over
the restated policy, clip_grad_norm_, RMSprop), two consecutive updates on small synthetic
rollouts filled through RolloutStorage.insert and compute_returns; the optimizer's
bookkeeping, the device guards, half-precision mode, checkpoint resume, and a CartPole
learning smoke."""
import numpy as np
import pytest
import torch

from helpers import a2c_ref as R

pytestmark = pytest.mark.gpu

VC, EC, LR, EPS, ALPHA, MAXN = 0.5, 0.01, 7e-4, 1e-5, 0.99, 0.5

# name -> (arch, kind, obs shape, base, base kwargs, vector obs, action space, T, N)
CASES = {
    "cnn": ("cnn", "cat", (4, 84, 84), "CNNBase", {"recurrent": False, "hidden_size": 64}, 0, ("Discrete", 8), 5, 8),
    "cnn_gru": ("cnn_gru", "cat", (4, 84, 84), "CNNBase", {"recurrent": True, "hidden_size": 64}, 3, ("Discrete", 8),
                5, 4),
    "mlp": ("mlp", "gauss", (6,), "MLPBase", {"recurrent": False, "hidden_size": 64}, 0, ("Box", 3), 5, 8),
    "mlp_gru": ("mlp_gru", "bern", (6,), "MLPBase", {"recurrent": True, "hidden_size": 64}, 2, ("MultiBinary", 5),
                4, 4),
}


def _space(spec):
    from a2c_ppo_acktr import synthetic as S
    name, n = spec
    return S.Box(shape=(n,)) if name == "Box" else getattr(S, name)(n)


def _build(gpu, name, seed=0, lr=LR):
    from a2c_ppo_acktr import model as M
    from a2c_ppo_acktr.algo import A2C_ACKTR
    from a2c_ppo_acktr.storage import RolloutStorage
    arch, kind, oshape, base, kw, V, space, T, N = CASES[name]
    torch.manual_seed(10 + seed)
    sp = _space(space)
    pol = M.Policy(oshape, sp, base=getattr(M, base), base_kwargs=dict(kw), vector_obs_len=V)
    pol.to(gpu)
    agent = A2C_ACKTR(pol, VC, EC, lr=lr, eps=EPS, alpha=ALPHA, max_grad_norm=MAXN)
    image = len(oshape) == 3
    st = RolloutStorage(T, N, oshape, [V], sp, kw["hidden_size"] if kw["recurrent"] else 1,
                        obs_dtype=torch.uint8 if image else torch.float32, device=gpu)
    return pol, agent, st


def _rollout(gpu, name, pol, st, seed):
    """T steps of pol.act on random observations, random rewards and episode ends, then
    compute_returns: every plane goes through insert"""
    arch, kind, oshape, base, kw, V, space, T, N = CASES[name]
    g = torch.Generator().manual_seed(seed)
    image = len(oshape) == 3

    def obs():
        if image:
            return torch.randint(0, 256, (N,) + oshape, dtype=torch.uint8, generator=g).to(gpu)
        return torch.randn((N,) + oshape, generator=g).to(gpu)

    st.obs[0].copy_(obs())
    st.vector_obs[0].copy_(torch.rand(N, V, generator=g).to(gpu))
    for step in range(T):
        v, a, lp, h = pol.act(st.obs[step], st.vector_obs[step], st.recurrent_hidden_states[step], st.masks[step])
        r = torch.randn(N, 1, generator=g).to(gpu)
        m = (torch.rand(N, 1, generator=g) > 0.25).float().to(gpu)
        st.insert(obs(), torch.rand(N, V, generator=g).to(gpu), h, a, lp, v, r, m, torch.ones(N, 1, device=gpu))
    nv = pol.get_value(st.obs[-1], st.vector_obs[-1], st.recurrent_hidden_states[-1], st.masks[-1])
    st.compute_returns(nv, False, 0.99, 0.95, False)


def _planes(name, st):
    arch, kind, oshape, base, kw, V, space, T, N = CASES[name]
    R_ = T * N
    return dict(obs=st.obs[:-1].reshape((R_,) + oshape), vec=st.vector_obs[:-1].reshape(R_, V),
                h0=st.recurrent_hidden_states[0], masks=st.masks[:-1].reshape(T, N),
                actions=st.actions.reshape(R_, -1)[:, 0] if kind == "cat" else st.actions.reshape(R_, -1),
                returns=st.returns[:-1].reshape(R_))


def _relu_decisions(pol, arch, params, obs):
    """CNNBase: the ReLU decisions of the update's own training forward for the reference
    to take (a unit within a rounding of 0 would otherwise move a gradient by a whole
    term), each differing one checked to sit within 1e-5 of its layer's largest
    pre-activation of 0 in float64 (helpers/relu_decisions.py)"""
    if arch not in ("cnn", "cnn_gru"):
        return None
    from helpers.relu_decisions import check_relu_decisions, engine_relu_masks
    eng, B = pol.hip_engine(), obs.shape[0]
    h = None if arch == "cnn" else eng.ws["train"].bufs["xpad"][:B * eng.Ip].view(B, eng.Ip)[:, :eng.H]
    relu = [m.cpu() for m in engine_relu_masks(eng, B, eng.H, h)]
    trunk = [p.cpu().double() for p in (params[4:12] if arch == "cnn_gru" else params[:8])]
    print("ReLU decisions differing from float64's:", check_relu_decisions(trunk, obs.cpu(), None, relu))
    return relu


def _flat(pol):
    return torch.cat([p.detach().reshape(-1) for p in pol.parameters()]).clone()


@pytest.mark.parametrize("name", list(CASES))
def test_a2c_update_vs_float64(gpu, name):
    """two consecutive updates; after each: p.grad (the clipped gradient) vs float64 autograd
    times the float64 clip coefficient, 1e-5 of each parameter tensor's largest entry; the
    returned losses rtol 1e-4 / atol 1e-6; the parameters vs an fp32 RMSprop step computed on
    the CPU from the GPU's own clipped gradient and previous state, atol 1e-6 (optimiser
    parity kept apart from gradient parity: near g = 0 the step's sensitivity to g is
    lr / eps = 70); square_avg by the same step rtol 2e-6; step_count advances by one."""
    arch, kind = CASES[name][:2]
    pol, agent, st = _build(gpu, name)
    sq_prev = None
    for k in range(2):
        _rollout(gpu, name, pol, st, 100 + k)
        params = [p.detach().clone() for p in pol.parameters()]
        before = _flat(pol).cpu().numpy()
        planes = _planes(name, st)
        losses = agent.update(st)
        torch.cuda.synchronize()
        ref = R.update_reference(arch, kind, params, **planes, vc=VC, ec=EC, max_norm=MAXN,
                                 relu=_relu_decisions(pol, arch, params, planes["obs"]))
        st.after_update()
        assert agent.optimizer.step_count == k + 1
        print("update", k, "norm", ref["norm"], "coef", ref["coef"], "losses", losses, ref["losses"])
        names = [n for n, _ in pol.named_parameters()]
        got = {n: p.grad.detach().cpu().numpy() for n, p in pol.named_parameters()}
        R.check_param_grads(got, dict(zip(names, ref["grads"])))
        R.check_update_losses(losses, ref["losses"])
        g = torch.cat([p.grad.detach().reshape(-1) for p in pol.parameters()]).cpu().numpy()
        sq0 = np.zeros_like(g) if sq_prev is None else sq_prev
        f = np.float32
        s = (sq0 * f(ALPHA)).astype(f)
        s = (s + ((f(1.0 - ALPHA) * g).astype(f) * g).astype(f)).astype(f)
        want = (before + (f(-LR) * (g / (np.sqrt(s).astype(f) + f(EPS))).astype(f)).astype(f)).astype(f)
        np.testing.assert_allclose(_flat(pol).cpu().numpy(), want, rtol=0, atol=1e-6)
        sq_prev = agent.optimizer.square_avg.cpu().numpy()
        np.testing.assert_allclose(sq_prev, s, rtol=2e-6, atol=0)


def test_a2c_zero_lr_moves_only_square_avg(gpu):
    """param_groups[0]['lr'] = 0 (what update_linear_schedule writes at the end of a run):
    parameters bit-unchanged, square_avg still moves"""
    pol, agent, st = _build(gpu, "mlp")
    _rollout(gpu, "mlp", pol, st, 1)
    agent.optimizer.param_groups[0]["lr"] = 0.0
    before = _flat(pol)
    losses = agent.update(st)
    assert all(np.isfinite(losses)) and torch.equal(_flat(pol), before)
    assert agent.optimizer.step_count == 1 and float(agent.optimizer.square_avg.abs().max()) > 0


@pytest.mark.parametrize("name,exc", [("cnn", IndexError), ("mlp", ValueError), ("mlp_gru", ValueError)])
def test_a2c_bad_stored_action_raises_and_skips_the_step(gpu, name, exc):
    """an out-of-range (Discrete), non-finite (Box) or non-binary (MultiBinary) stored action
    in the second update: the error the reference would raise, with parameters, square_avg
    and the step count those of the first update, bit for bit"""
    kind = CASES[name][1]
    pol, agent, st = _build(gpu, name)
    _rollout(gpu, name, pol, st, 1)
    agent.update(st)
    st.after_update()
    _rollout(gpu, name, pol, st, 2)
    st.actions[1, 2, 0] = {"cat": 8, "gauss": float("nan"), "bern": 0.5}[kind]
    before, sq = _flat(pol), agent.optimizer.square_avg.clone()
    with pytest.raises(exc, match="A2C_ACKTR.update"):
        agent.update(st)
    assert torch.equal(_flat(pol), before) and torch.equal(agent.optimizer.square_avg, sq)
    assert agent.optimizer.step_count == 1 and agent.optimizer.guard is None
    st.actions[1, 2, 0] = 1
    assert all(np.isfinite(agent.update(st))) and agent.optimizer.step_count == 2


def test_a2c_half_precision_losses_are_finite(gpu):
    pol, agent, st = _build(gpu, "cnn")
    pol.half()
    _rollout(gpu, "cnn", pol, st, 1)
    losses = agent.update(st)
    assert all(np.isfinite(losses)) and torch.isfinite(_flat(pol)).all()


@pytest.mark.parametrize("name", ["cnn", "mlp_gru"])
def test_a2c_checkpoint_resume_is_bit_identical(gpu, name, tmp_path):
    """save after update 1, load into a fresh agent, run update 2 on the same rollout:
    parameters, square_avg and losses equal the uninterrupted run's bit for bit"""
    from a2c_ppo_acktr import checkpoint as CK
    pol, agent, st = _build(gpu, name)
    _rollout(gpu, name, pol, st, 1)
    agent.update(st)
    st.after_update()
    path = str(tmp_path / "a2c.pt")
    CK.save_checkpoint(path, pol, None, agent=agent)
    _rollout(gpu, name, pol, st, 2)
    pol2, agent2, _ = _build(gpu, name, seed=5, lr=1.0)
    CK.load_checkpoint(path, device=gpu, agent=agent2)
    assert agent2.optimizer.step_count == 1 and agent2.optimizer.param_groups[0]["lr"] == LR
    l1 = agent.update(st)
    l2 = agent2.update(st)
    assert l1 == l2
    assert torch.equal(_flat(pol), _flat(pol2))
    assert torch.equal(agent.optimizer.square_avg, agent2.optimizer.square_avg)


def test_a2c_learns_cartpole(gpu):
    """MLPBase on the device CartPole with the reference's A2C defaults (T = 5, lr 7e-4, eps
    1e-5, alpha 0.99, gamma 0.99, no GAE, value_loss_coef 0.5, entropy_coef 0.01,
    max_grad_norm 0.5), 32 envs, 400 updates.  The float64 restatement on the CPU
    (tools/a2c_cartpole_ref.py --envs 32 --updates 400, seeds 0 / 1 / 2) takes the mean
    length of the episodes finishing in the first tenth of the run from 25.9 / 26.5 / 23.6
    to 282.7 / 299.1 / 301.5 in the last tenth (x 10.9 / 11.3 / 12.8); this run has other
    random streams, so it must reach twice the early length, with finite losses."""
    from a2c_ppo_acktr import model as M
    from a2c_ppo_acktr.algo import A2C_ACKTR
    from a2c_ppo_acktr.storage import RolloutStorage
    from a2c_ppo_acktr.synthetic import CartPoleVecEnv
    torch.manual_seed(0)
    N, T, updates = 32, 5, 400
    env = CartPoleVecEnv(N, seed=3, device=gpu)
    pol = M.Policy(env.obs_shape, env.action_space, base=M.MLPBase, base_kwargs={"recurrent": False})
    pol.to(gpu)
    agent = A2C_ACKTR(pol, 0.5, 0.01, lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5)
    st = RolloutStorage(T, N, env.obs_shape, [0], env.action_space, 1, device=gpu)
    env.reset_into(st.obs[0])
    tot = torch.zeros(updates, 2, device=gpu)   # per update: Σ length and number of the episodes that finished
    for it in range(updates):
        for step in range(T):
            v, a, lp, h = pol.act(st.obs[step], st.vector_obs[step], st.recurrent_hidden_states[step], st.masks[step])
            r, m, bm = env.step_into(st.obs[step + 1], a)
            tot[it, 0] += env.ep_len.sum()
            tot[it, 1] += (env.ep_len > 0).sum()
            st.insert(st.obs[step + 1], st.vector_obs[step + 1], h, a, lp, v, r, m, bm)
        nv = pol.get_value(st.obs[-1], st.vector_obs[-1], st.recurrent_hidden_states[-1], st.masks[-1])
        st.compute_returns(nv, False, 0.99, 0.95, False)
        losses = agent.update(st)
        st.after_update()
        assert all(np.isfinite(losses)), (it, losses)
    t = tot.cpu().numpy().reshape(10, updates // 10, 2).sum(1)
    curve = t[:, 0] / np.maximum(t[:, 1], 1)
    print("cartpole mean episode length per tenth of the run:", " ".join("%.1f" % x for x in curve))
    assert curve[-1] >= 2 * curve[0], curve
