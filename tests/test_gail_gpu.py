"""GAIL on the MI355X: the train kernel and its reduce against float64 closed forms,
Discriminator.update against the float64 reference loop (parameters, loss, the CPU
generator's state), the reward kernels against float64 with the per-step and the
whole-rollout forms bit-equal, one PPO + GAIL iteration end to end, checkpoint resume and
the refusals."""
import numpy as np
import pytest
import torch
import torch.utils.data

from a2c_ppo_acktr import checkpoint as CK
from a2c_ppo_acktr import model as M
from a2c_ppo_acktr import synthetic as S
from a2c_ppo_acktr._hip import call
from a2c_ppo_acktr.algo import PPO, gail
from a2c_ppo_acktr.storage import RolloutStorage
from helpers import a2c_ref
from helpers import gail_ref as R

pytestmark = pytest.mark.gpu
POISON = -12345.0
TAIL = 8


def _t(a, gpu):
    return torch.as_tensor(np.array(a)).to(gpu)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _run_train(c, gpu, alpha=None):
    """ppo_gail_train + ppo_gail_reduce on a build_case (alpha: in place of the case's):
    every output has TAIL poisoned elements past its end -> ({name: gradient}, loss_acc
    [4], the raw output tensors)"""
    D, Hd, B = c["D"], c["Hd"], c["B"]
    P = R.num_params(D, Hd)
    nblk = call("ppo_gail_train_blocks", B)
    params, obs, act = _t(c["flat"], gpu), _t(c["obs"], gpu), _t(c["act"], gpu)
    vec = _t(c["vec"], gpu) if c["V"] else None
    expert, alpha = _t(c["x_e"], gpu), _t(c["alpha"] if alpha is None else alpha, gpu)
    idx = _t(c["idx"], gpu) if c["idx"] is not None else None
    pg = torch.full((nblk * P + TAIL,), POISON, device=gpu)
    pl = torch.full((nblk * 3 + TAIL,), POISON, device=gpu)
    grad = torch.full((P + TAIL,), POISON, device=gpu)
    acc = torch.full((4 + TAIL,), POISON, dtype=torch.float64, device=gpu)
    acc[0] = 0.0
    s = torch.cuda.current_stream().cuda_stream
    call("ppo_gail_train", params.data_ptr(), D, Hd, B, obs.data_ptr(), c["od"], _ptr(vec), c["V"], act.data_ptr(),
         c["A"], c["R"], _ptr(idx), c["row0"], expert.data_ptr(), alpha.data_ptr(), R.LAMBDA, pg.data_ptr(),
         pl.data_ptr(), s)
    call("ppo_gail_reduce", pg.data_ptr(), pl.data_ptr(), nblk, P, B, R.LAMBDA, grad.data_ptr(), acc.data_ptr(), s)
    torch.cuda.synchronize()
    for name, t, n in (("part_grad", pg, nblk * P), ("part_loss", pl, nblk * 3), ("grad", grad, P), ("loss_acc", acc, 4)):
        assert bool((t[n:] == POISON).all()), name + ": stored past its end"
        assert bool(torch.isfinite(t[:n]).all()), name
    return R.unpack(grad[:P].cpu().numpy(), D, Hd), acc[:4].cpu().numpy(), (pg, pl, grad, acc)


@pytest.mark.parametrize("case", R.TRAIN_CASES, ids=lambda c: "D{}-Hd{}-B{}-{}".format(*c))
def test_train_kernel_against_float64(gpu, case):
    """the six gradient tensors under cat_ref.grad_bound, the three loss sums and L under
    check_update_losses' bounds; a second run gives the same bits; nothing is stored past
    the end of any output"""
    c = R.build_case(*case)
    grads, acc, raw = _run_train(c, gpu)
    ref = c["ref"]
    print("sums", acc[1:], ref["sums"], "L", acc[0], ref["loss"])
    R.check_grads(grads, ref["grads"])
    a2c_ref.check_update_losses(acc[1:], ref["sums"])
    a2c_ref.check_update_losses([acc[0]], [ref["loss"]])
    _, _, again = _run_train(c, gpu)
    for a, b in zip(raw, again):
        assert torch.equal(a, b)


def test_compute_grad_pen_agrees_with_the_kernel(gpu):
    """the torch method on the device (autograd, create_graph) against the kernel's
    penalty sum for the same alpha (the draw of one seed)"""
    c = R.build_case(14, 100, 33, "idx")
    B, D = c["B"], c["D"]
    torch.manual_seed(8)
    alpha = torch.rand(B, 1)              # compute_grad_pen's draw under this seed
    _, acc, _ = _run_train(c, gpu, alpha.numpy().reshape(-1))
    discr = gail.Discriminator(D, c["Hd"], gpu)
    with torch.no_grad():
        discr.flat.copy_(_t(c["flat"], gpu))
    x_e, x_p = _t(c["x_e"], gpu), _t(c["x_p"], gpu)
    torch.manual_seed(8)
    pen = discr.compute_grad_pen(x_e[:, :D - 2], x_e[:, D - 2:], x_p[:, :D - 2], x_p[:, D - 2:])
    a2c_ref.check_update_losses([R.LAMBDA * acc[3] / B], [pen.item()])


# ---------------------------------------------------------------------- update
def _storage(gpu, T, N, od, A, V=0, seed=0):
    g = torch.Generator().manual_seed(seed)
    st = RolloutStorage(T, N, (od,), [V], S.Box(shape=(A,)), 1, device=gpu)
    st.obs.copy_((0.3 + torch.randn(T + 1, N, od, generator=g)).to(gpu))
    if V:
        st.vector_obs.copy_(torch.rand(T + 1, N, V, generator=g).to(gpu))
    st.actions.copy_(torch.randn(T, N, A, generator=g).to(gpu))
    st.masks[1:].copy_((torch.rand(T, N, 1, generator=g) > 0.25).float().to(gpu))
    return st


def _loader(n, od, A, batch, seed=1):
    g = torch.Generator().manual_seed(seed)
    ds = torch.utils.data.TensorDataset(torch.randn(n, od, generator=g), torch.randn(n, A, generator=g))
    return torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True, drop_last=True)


def _obsfilt(x, update=True):
    assert update is False
    return (x - 0.1) * 0.5


@pytest.mark.parametrize("V", [0, 3])
def test_update_against_float64_reference_loop(gpu, V):
    """T N = 12 x 8, D = 5 (+ V) + 2, batch 32, an expert loader of 3 shuffled batches:
    three Adam steps.  Parameters within atol 1e-6 of the float64 loop, the returned loss
    under check_update_losses, and the default CPU generator in the state the
    reference-text loop leaves it in."""
    T, N, od, A, Hd, batch = 12, 8, 5, 2, 100, 32
    D = od + V + A
    st = _storage(gpu, T, N, od, A, V)
    loader = _loader(96, od + V, A, batch)
    torch.manual_seed(5)
    discr = gail.Discriminator(D, Hd, gpu)
    flat0 = discr.flat.cpu().numpy().copy()
    torch.manual_seed(11)
    start = torch.get_rng_state()
    loss = discr.update(loader, st, _obsfilt)
    after = torch.get_rng_state()
    torch.set_rng_state(start)
    flat = lambda t, k: t[:T].reshape(T * N, k).cpu().numpy()   # noqa: E731
    p_ref, loss_ref, pairs = R.reference_update(flat0, D, Hd, loader, flat(st.obs, od), flat(st.vector_obs, V),
                                                flat(st.actions, A), batch, _obsfilt)
    assert len(pairs) == 3 and discr.optimizer.step_count == 3
    assert torch.equal(torch.get_rng_state(), after)
    err = np.abs(discr.flat.cpu().numpy().astype(np.float64) - p_ref).max()
    print("params: max err", err, "moved", np.abs(p_ref - flat0).max(), "loss", loss, loss_ref)
    assert np.abs(p_ref - flat0).max() > 1e-3
    assert err <= 1e-6
    a2c_ref.check_update_losses([loss], [loss_ref])
    # the parameters are still views of the flat buffer and the torch path sees the step
    x = torch.randn(4, D).to(gpu)
    ref_d = R.forward({k: v.astype(np.float64) for k, v in R.unpack(discr.flat.cpu().numpy(), D, Hd).items()},
                      x.cpu().numpy().astype(np.float64))[2]
    np.testing.assert_allclose(discr.trunk(x).detach().cpu().numpy().reshape(-1), ref_d, atol=1e-5)


def test_update_edge_cases(gpu):
    st = _storage(gpu, 4, 8, 5, 2)
    discr = gail.Discriminator(7, 100, gpu)
    with pytest.raises(ZeroDivisionError):
        discr.update(_loader(8, 5, 2, 16), st)      # drop_last: no expert batch at all
    ds = torch.utils.data.TensorDataset(torch.randn(20, 5), torch.randn(20, 2))
    with pytest.raises(ValueError, match="expert batch"):
        discr.update(torch.utils.data.DataLoader(ds, batch_size=16), st)   # 16, then 4 rows
    # more expert batches than policy minibatches: the zip ends with the policy side
    before = discr.optimizer.step_count
    discr.update(torch.utils.data.DataLoader(ds, batch_size=5), st)        # 4 expert batches, 32 // 5 = 6
    assert discr.optimizer.step_count == before + 4
    before = discr.optimizer.step_count
    discr.update(_loader(96, 5, 2, 16), st)                                # 6 expert batches, 32 // 16 = 2
    assert discr.optimizer.step_count == before + 2


# --------------------------------------------------------------------- rewards
def _reward_discr(c, gpu):
    discr = gail.Discriminator(c["D"], c["Hd"], gpu)
    with torch.no_grad():
        discr.flat.copy_(_t(c["flat"], gpu))
    return discr


def _fill(st, c, k, gpu):
    T, od = c["T"], c["obs_dim"]
    x = _t(c["x"][k], gpu)
    st.obs[:T].copy_(x[..., :od])
    st.actions.copy_(x[..., od:])
    st.masks[:T, :, 0].copy_(_t(c["masks"][k], gpu))


@pytest.mark.parametrize("N", [7, 1])
def test_rewards_against_float64_and_step_equals_rollout(gpu, N):
    """two consecutive rollouts of T = 5: the logit, the scaled reward, the carried
    returns and {mean, var, count} against float64 under gail_ref.REWARD_BOUNDS;
    predict_reward step by step and predict_rewards over the rollout give the same bits;
    update_rms=False leaves the state bit-unchanged."""
    c = R.reward_case(N)
    T, od, D, Hd = c["T"], c["obs_dim"], c["D"], c["Hd"]
    whole, steps = _reward_discr(c, gpu), _reward_discr(c, gpu)
    st = RolloutStorage(T, N, (od,), [0], S.Box(shape=(c["A"],)), 1, device=gpu)
    s = torch.cuda.current_stream().cuda_stream
    for k in range(2):
        _fill(st, c, k, gpu)
        d = torch.full((T * N + TAIL,), POISON, device=gpu)
        call("ppo_gail_reward", whole.flat.data_ptr(), D, Hd, st.obs.data_ptr(), od, None, 0, st.actions.data_ptr(),
             c["A"], 0, T * N, d.data_ptr(), s)
        assert bool((d[T * N:] == POISON).all())
        out = whole.predict_rewards(st, c["gamma"])
        assert out is st.rewards
        per_step = torch.stack([steps.predict_reward(st.obs[t], st.actions[t], c["gamma"], st.masks[t])
                                for t in range(T)])
        assert torch.equal(per_step, st.rewards)
        assert torch.equal(whole.returns, steps.returns) and torch.equal(whole._rms, steps._rms)
        assert whole.returns.shape == (N, 1)
        rms = whole.ret_rms
        R.check_rewards((d[:T * N].cpu().numpy(), st.rewards.cpu().numpy(), whole.returns.cpu().numpy(),
                         (rms.mean, rms.var, rms.count)), c["ref"][k])
    ret, words = whole.returns.clone(), whole._rms.clone()
    whole.predict_rewards(st, c["gamma"], update_rms=False)
    frozen = steps.predict_reward(st.obs[2], st.actions[2], c["gamma"], st.masks[2], update_rms=False)
    assert torch.equal(frozen, st.rewards[2])
    for dsc in (whole, steps):
        assert torch.equal(dsc.returns, ret) and torch.equal(dsc._rms, words)
    scale = np.float32(np.sqrt(words[1].item() + 1e-8))
    assert np.array_equal(st.rewards.cpu().numpy().reshape(-1), d[:T * N].cpu().numpy() / scale)


def test_reward_kernel_tiles_and_offsets(gpu):
    """more rows than one 64-row tile and than one pass of the grid's blocks (1024 tiles), a
    row offset, a vector_obs plane: each row's logit equals the one-row launch's, bit for bit"""
    od, V, A, Hd = 3, 2, 1, 8
    D, rows, row0 = od + V + A, 64 * 1024 + 64 + 5, 3
    g = torch.Generator().manual_seed(2)
    obs, vec, act = (torch.randn(rows + row0, k, generator=g).to(gpu) for k in (od, V, A))
    params = _t(R.trunk_flat(R.make_trunk(D, Hd, 9)), gpu)
    out = torch.full((rows + TAIL,), POISON, device=gpu)
    s = torch.cuda.current_stream().cuda_stream
    args = (params.data_ptr(), D, Hd, obs.data_ptr(), od, vec.data_ptr(), V, act.data_ptr(), A)
    call("ppo_gail_reward", *args, row0, rows, out.data_ptr(), s)
    assert bool((out[rows:] == POISON).all())
    x = torch.cat([obs, vec, act], 1)[row0:].cpu().numpy().astype(np.float64)
    p = {k: v.astype(np.float64) for k, v in R.unpack(params.cpu().numpy(), D, Hd).items()}
    assert np.abs(out[:rows].cpu().numpy() - R.forward(p, x)[2]).max() <= 1e-6
    one = torch.empty(1, device=gpu)
    for r in (0, 63, 64, 65535, 65536, rows - 1):
        call("ppo_gail_reward", *args, row0 + r, 1, one.data_ptr(), s)
        assert torch.equal(one, out[r:r + 1]), r


# ------------------------------------------------------------------ end to end
def _iteration(gpu, pol, agent, st, discr, loader):
    T = st.num_steps
    for step in range(T):
        v, a, lp, h = pol.act(st.obs[step], st.vector_obs[step], st.recurrent_hidden_states[step], st.masks[step])
        obs = torch.tanh(st.obs[step] + 0.1 * a.sum(1, keepdim=True))
        st.insert(obs, st.vector_obs[step + 1], h, a, lp, v, torch.zeros_like(v), torch.ones_like(v),
                  torch.ones_like(v))
    nv = pol.get_value(st.obs[-1], st.vector_obs[-1], st.recurrent_hidden_states[-1], st.masks[-1])
    d_losses = [discr.update(loader, st) for _ in range(2)]
    discr.predict_rewards(st, 0.99)
    st.compute_returns(nv, True, 0.99, 0.95, False)
    losses = agent.update(st)
    st.after_update()
    return d_losses, losses


def _e2e(gpu, seed=0):
    torch.manual_seed(seed)
    N, T, od, A = 4, 8, 5, 2
    space = S.Box(shape=(A,))
    pol = M.Policy((od,), space, base=M.MLPBase, base_kwargs={"recurrent": False})
    pol.to(gpu)
    agent = PPO(pol, 0.2, 2, 2, 0.5, 0.0, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
    st = RolloutStorage(T, N, (od,), [0], space, 1, device=gpu)
    st.obs[0].copy_(torch.randn(N, od).to(gpu))
    discr = gail.Discriminator(od + A, 100, gpu)
    return pol, agent, st, discr, _loader(64, od, A, 16)


def test_ppo_with_gail_rewards_end_to_end(gpu):
    pol, agent, st, discr, loader = _e2e(gpu)
    before = torch.cat([p.detach().reshape(-1) for p in pol.parameters()]).clone()
    d_losses, losses = _iteration(gpu, pol, agent, st, discr, loader)
    assert all(np.isfinite(d_losses)) and all(np.isfinite(losses)), (d_losses, losses)
    rew = st.rewards
    assert bool(torch.isfinite(rew).all()) and float(rew.abs().max()) > 0 and float(rew.std()) > 0
    after = torch.cat([p.detach().reshape(-1) for p in pol.parameters()])
    assert bool(torch.isfinite(after).all()) and float((after - before).abs().max()) > 0
    assert discr.optimizer.step_count == 4 and discr.ret_rms.count == pytest.approx(32 + 1e-4)


def test_checkpoint_resume_is_bit_identical(gpu, tmp_path):
    """save after one iteration, rebuild everything, load: the next discriminator update
    and predict_rewards give the bits of the uninterrupted run"""
    pol, agent, st, discr, loader = _e2e(gpu)
    _iteration(gpu, pol, agent, st, discr, loader)
    path = str(tmp_path / "gail.pt")
    CK.save_checkpoint(path, pol, None, agent=agent, discr=discr)
    rng = torch.get_rng_state()
    loss = discr.update(loader, st)
    discr.predict_rewards(st, 0.99)
    want = (discr.flat.clone(), st.rewards.clone(), discr.returns.clone(), discr._rms.clone())
    pol2, agent2, st2, discr2, _ = _e2e(gpu, seed=123)
    CK.load_checkpoint(path, gpu, agent=agent2, discr=discr2)
    assert list(discr2.state_dict()) == ["trunk.%d.%s" % (i, k) for i in (0, 2, 4) for k in ("weight", "bias")]
    for name in ("obs", "actions", "masks"):
        getattr(st2, name).copy_(getattr(st, name))
    torch.set_rng_state(rng)
    loss2 = discr2.update(loader, st2)
    discr2.predict_rewards(st2, 0.99)
    assert loss2 == loss
    for a, b in zip(want, (discr2.flat, st2.rewards, discr2.returns, discr2._rms)):
        assert torch.equal(a, b)
    with pytest.raises(KeyError):
        CK.save_checkpoint(path, pol, None, agent=agent)
        CK.load_checkpoint(path, gpu, agent=agent2, discr=discr2)


# -------------------------------------------------------------------- refusals
def test_refusals(gpu):
    discr = gail.Discriminator(7, 100, gpu)
    loader = _loader(32, 5, 2, 16)
    good = _storage(gpu, 4, 8, 5, 2)
    with pytest.raises(TypeError, match="input_dim"):
        discr.update(loader, _storage(gpu, 4, 8, 6, 2))
    with pytest.raises(TypeError, match="input_dim"):
        discr.predict_rewards(_storage(gpu, 4, 8, 5, 2, V=1), 0.99)
    image = RolloutStorage(2, 2, (4, 84, 84), [0], S.Box(shape=(2,)), 1, obs_dtype=torch.uint8, device=gpu)
    with pytest.raises(NotImplementedError, match="1-D observations"):
        discr.update(loader, image)
    disc = RolloutStorage(4, 8, (6,), [0], S.Discrete(3), 1, device=gpu)
    with pytest.raises(NotImplementedError, match="Discrete"):
        discr.predict_rewards(disc, 0.99)
    half = _storage(gpu, 4, 8, 5, 2)
    half.obs = half.obs.half()
    with pytest.raises(NotImplementedError, match="half"):
        discr.update(loader, half)
    dbl = _storage(gpu, 4, 8, 5, 2)
    dbl.actions = dbl.actions.double()
    with pytest.raises(TypeError, match="float32"):
        discr.update(loader, dbl)
    host = RolloutStorage(4, 8, (5,), [0], S.Box(shape=(2,)), 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        discr.update(loader, host)
    with pytest.raises(TypeError):
        discr.predict_reward(good.obs[0], good.actions[0].double(), 0.99, good.masks[0])
    with pytest.raises(TypeError):
        discr.predict_reward(good.obs[0, :, :4], good.actions[0], 0.99, good.masks[0])
    discr.predict_reward(good.obs[0], good.actions[0], 0.99, good.masks[0])
    with pytest.raises(RuntimeError, match="lanes"):
        discr.predict_reward(good.obs[0, :4], good.actions[0, :4], 0.99, good.masks[0, :4])


def test_distributed_run_is_refused(gpu, monkeypatch):
    discr = gail.Discriminator(7, 100, gpu)
    st = _storage(gpu, 4, 8, 5, 2)
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    with pytest.raises(NotImplementedError, match="torch.distributed"):
        discr.update(_loader(32, 5, 2, 16), st)
    with pytest.raises(NotImplementedError, match="torch.distributed"):
        discr.predict_rewards(st, 0.99)
    with pytest.raises(NotImplementedError, match="torch.distributed"):
        discr.predict_reward(st.obs[0], st.actions[0], 0.99, st.masks[0])
