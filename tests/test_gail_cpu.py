"""GAIL without a GPU: the float64 references (closed forms against autograd, the planted
errors, Adam and the running moments), the C ABI of csrc/gail.hip and its argument
checks, ExpertDataset, and the host side of algo.gail.Discriminator."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from a2c_ppo_acktr.algo import gail
from a2c_ppo_acktr.arguments import get_args
from conftest import ROOT
from helpers import gail_ref as R

HEADER = os.path.join(ROOT, "include", "ppo_hip.h")
NEW = ("ppo_gail_train_blocks", "ppo_gail_lds_bytes", "ppo_gail_train", "ppo_gail_reduce", "ppo_gail_reward", "ppo_gail_returns")
PPO_EARG = 1001
SHAPES = ((5, 100, 7), (23, 100, 128), (14, 100, 33), (393, 100, 128))


# ------------------------------------------------------------------ references
@pytest.mark.parametrize("D,Hd,B", SHAPES)
def test_closed_forms_equal_float64_autograd(D, Hd, B):
    """closed_form's loss and six gradient tensors against float64 autograd (create_graph)
    of the restated loss: every tensor within 1e-12 of its largest entry."""
    g = np.random.default_rng(D + B)
    flat = R.trunk_flat(R.make_trunk(D, Hd, D * B))
    x_e, x_p = g.normal(size=(B, D)).astype(np.float32), (0.3 + g.normal(size=(B, D))).astype(np.float32)
    alpha = g.random(size=B).astype(np.float32)
    ref = R.closed_form(flat, D, Hd, x_e, x_p, alpha)
    loss, grads = R.autograd_grads(flat, D, Hd, x_e, x_p, alpha)
    assert abs(loss - ref["loss"]) <= 1e-12 * abs(loss)
    for name in R.NAMES:
        err = np.abs(grads[name] - ref["grads"][name]).max()
        assert err <= 1e-12 * np.abs(grads[name]).max(), (name, err)


@pytest.mark.parametrize("plant", R.PLANTS)
def test_planted_errors_are_rejected(plant):
    """the comparison the GPU tests use (check_grads; check_update_losses for the loss,
    which "const_s" alone leaves unchanged) rejects each planted error of the float64
    reference, on a train case with B > 1"""
    from helpers import a2c_ref
    c = R.build_case(5, 100, 7, "row0")
    bad = R.closed_form(c["flat"], c["D"], c["Hd"], c["x_e"], c["x_p"], c["alpha"], plant=plant)
    with pytest.raises(AssertionError):
        R.check_grads(bad["grads"], c["ref"]["grads"], show=lambda *a: None)
    if plant == "const_s":
        a2c_ref.check_update_losses([bad["loss"]], [c["ref"]["loss"]])
    else:
        with pytest.raises(AssertionError):
            a2c_ref.check_update_losses([bad["loss"]], [c["ref"]["loss"]])
    R.check_grads(c["ref"]["grads"], c["ref"]["grads"], show=lambda *a: None)


def test_adam_restatement_equals_torch_float64():
    g = np.random.default_rng(5)
    p0 = g.normal(size=50)
    t = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([t])
    p, m, v = p0.copy(), np.zeros(50), np.zeros(50)
    for step in range(1, 5):
        grad = g.normal(size=50) * 10.0 ** g.integers(-6, 2, size=50)
        t.grad = torch.tensor(grad)
        opt.step()
        p, m, v = R.adam_step(p, grad, m, v, step)
        np.testing.assert_allclose(p, t.detach().numpy(), rtol=0, atol=1e-13)


def test_running_mean_std_equals_moments_of_the_concatenation():
    """RunningMeanStd (the parallel-variance merge) against numpy float64 moments of all
    batches at once; the 1e-4 pseudo-count of the prior (mean 0, var 1) is accounted for"""
    g = np.random.default_rng(9)
    rms, seen = R.RunningMeanStd(), []
    for n in (7, 1, 128, 33):
        x = g.normal(loc=0.7, scale=2.0, size=n).astype(np.float32)
        rms.update(x)
        seen.append(x.astype(np.float64))
    x = np.concatenate(seen)
    c0, n = 1e-4, x.size
    mean = x.sum() / (n + c0)
    var = (c0 * (1.0 + mean ** 2) + ((x - mean) ** 2).sum()) / (n + c0)
    assert rms.count == pytest.approx(n + c0, rel=1e-15)
    assert rms.mean == pytest.approx(mean, rel=1e-12)
    assert rms.var == pytest.approx(var, rel=1e-12)
    # returns_ref: the first call's returns start as d[0], then one recursion step
    d, m = g.normal(size=(2, 3)), np.array([[1, 0, 1], [1, 1, 0]], np.float64)
    out, ret, rm = R.returns_ref(d, m, 0.5)
    g32 = float(np.float32(0.5))
    r0 = d[0] * m[0] * g32 + d[0]
    np.testing.assert_array_equal(ret, r0 * m[1] * g32 + d[1])
    assert rm.count == 6 + 1e-4
    _, ret2, rm2 = R.returns_ref(d, m, 0.5, update_rms=False)
    np.testing.assert_array_equal(ret2, d[0])
    assert (rm2.mean, rm2.var, rm2.count) == (0.0, 1.0, 1e-4)


# ------------------------------------------------------------------------- ABI
def test_entry_points_declared_bound_and_exported():
    from a2c_ppo_acktr import _hip
    src = open(HEADER).read()
    lib = _hip.lib()
    declared = set(re.findall(r"\b(?:int|long long)\s+(ppo_gail_\w+)\s*\(", src))
    assert declared == set(NEW) == {n for n in _hip.SIGNATURES if n.startswith("ppo_gail_")}
    for name in NEW:
        decl = re.search(r"\b(?:int|long long)\s+" + name + r"\s*\(([^)]*)\)", src)
        assert decl.group(1).count(",") + 1 == len(_hip.SIGNATURES[name]), name
        assert hasattr(lib, name), name
    assert lib.ppo_abi_version() == 3
    assert "ppo_gail_train_blocks" in _hip._VALUE_FUNCS
    assert [_hip.call("ppo_gail_train_blocks", b) for b in (1, 2, 5, 128)] == [1, 1, 3, 64]
    # the LDS footprint: the reference's default fits, Hd = 100 up to D = 145
    lds = lambda D, Hd: _hip.call("ppo_gail_lds_bytes", D, Hd)   # noqa: E731
    par = 100 * 23 + 100 * 101 + 301                       # W1 and W2 rows at odd strides
    assert lds(23, 100) == 4 * max(par + 8 * 23 + 38 * 101 + 12, par + 64 * 23 + 64 * 101 + 256) == 83572
    assert lds(145, 100) <= 160 * 1024 < lds(146, 100) and lds(1, 100) == lds(23, 132) == -1


def test_argument_checks_return_earg_before_any_hip_call():
    """bad sizes and NULL pointers: PPO_EARG, on a machine with no GPU (no HIP call is made)"""
    from a2c_ppo_acktr import _hip
    lib = _hip.lib()
    buf = (ctypes.c_float * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def train(D=3, Hd=4, B=1, od=2, V=0, A=1, rows=4, params=p, expert=p, obs=p, vec=None, out=p):
        return lib.ppo_gail_train(params, D, Hd, B, obs, od, vec, V, p, A, rows, None, 0, expert, p, 10.0, out, p, None)

    for bad in (dict(Hd=6), dict(Hd=0), dict(Hd=132), dict(D=1, od=0), dict(B=0), dict(params=None),
                dict(expert=None), dict(out=None), dict(obs=None), dict(V=1, od=1), dict(od=3), dict(rows=0),
                dict(D=393, Hd=100, od=391, A=2), dict(D=248, Hd=100, od=246, A=2)):
        assert train(**bad) == PPO_EARG, bad
        assert lib.ppo_last_error()

    def reward(D=3, Hd=4, R_=1, od=2, A=1, params=p, out=p):
        return lib.ppo_gail_reward(params, D, Hd, p, od, None, 0, p, A, 0, R_, out, None)

    for bad in (dict(Hd=5), dict(Hd=256), dict(D=1, od=0), dict(R_=0), dict(params=None), dict(out=None), dict(od=1),
                dict(D=146, Hd=100, od=145)):
        assert reward(**bad) == PPO_EARG, bad
    assert lib.ppo_gail_reduce(p, p, 0, 10, 1, 10.0, p, p, None) == PPO_EARG
    assert lib.ppo_gail_reduce(p, p, 1, 10, 1, 10.0, None, p, None) == PPO_EARG
    assert lib.ppo_gail_returns(p, p, p, p, 0, 1, 0.99, 1, None) == PPO_EARG
    assert lib.ppo_gail_returns(p, p, p, None, 1, 1, 0.99, 1, None) == PPO_EARG
    assert lib.ppo_gail_returns(None, p, p, p, 1, 1, 0.99, 1, None) == PPO_EARG


# --------------------------------------------------------------- ExpertDataset
def test_expert_dataset(tmp_path):
    """6 trajectories x 40 steps with uneven lengths, 3 kept, every 4th step: len, every
    item and the generator state afterwards (one randperm(6), one randint(0, 4, (3,)))"""
    g = torch.Generator().manual_seed(3)
    n, L, S, A = 6, 40, 5, 2
    data = {"states": torch.randn(n, L, S, generator=g), "actions": torch.randn(n, L, A, generator=g),
            "rewards": torch.randn(n, L, generator=g), "lengths": torch.tensor([40, 33, 17, 40, 8, 25])}
    path = str(tmp_path / "experts.pt")
    torch.save(data, path)
    torch.manual_seed(21)
    start = torch.get_rng_state()
    ds = gail.ExpertDataset(path, num_trajectories=3, subsample_frequency=4)
    after = torch.get_rng_state()
    torch.set_rng_state(start)
    perm, off = torch.randperm(n), torch.randint(0, 4, size=(3,))
    assert torch.equal(torch.get_rng_state(), after)
    lengths = [int(data["lengths"][perm[i]]) // 4 for i in range(3)]
    assert len(ds) == sum(lengths)
    i = 0
    for t in range(3):
        for j in range(lengths[t]):
            s, a = ds[i]
            assert torch.equal(s, data["states"][perm[t], int(off[t]) + 4 * j]), (t, j)
            assert torch.equal(a, data["actions"][perm[t], int(off[t]) + 4 * j]), (t, j)
            i += 1
    with pytest.raises(IndexError):
        ds[len(ds)]
    batches = list(torch.utils.data.DataLoader(ds, batch_size=4, shuffle=True, drop_last=True))
    assert len(batches) == len(ds) // 4 and batches[0][0].shape == (4, S) and batches[0][1].shape == (4, A)


# ------------------------------------------------------------------ host side
def test_discriminator_init_matches_plain_sequential():
    torch.manual_seed(4)
    ref = nn.Sequential(nn.Linear(7, 100), nn.Tanh(), nn.Linear(100, 100), nn.Tanh(), nn.Linear(100, 1))
    torch.manual_seed(4)
    d = gail.Discriminator(7, 100, torch.device("cpu"))
    assert list(d.state_dict()) == ["trunk." + k for k in ref.state_dict()]
    for a, b in zip(d.trunk.parameters(), ref.parameters()):
        assert torch.equal(a, b)
    # the parameters are views of one flat buffer, in trunk.parameters() order
    assert d.numel == R.num_params(7, 100) and d.flat.numel() == d.numel
    assert torch.equal(d.flat, torch.cat([p.detach().reshape(-1) for p in ref.parameters()]))
    with torch.no_grad():
        d.flat.zero_()
    assert all(float(p.detach().abs().max()) == 0.0 for p in d.trunk.parameters())
    x = torch.randn(3, 7)
    assert d.trunk(x).shape == (3, 1)
    assert d.optimizer.param_groups[0]["lr"] == 1e-3 and d.optimizer.param_groups[0]["eps"] == 1e-8
    assert d.returns is None
    assert (d.ret_rms.mean, d.ret_rms.var, d.ret_rms.count) == (0.0, 1.0, 1e-4)
    assert isinstance(d.compute_grad_pen(x[:, :5], x[:, 5:], x[:, :5] + 1, x[:, 5:]).item(), float)


def test_cpu_device_has_no_compute_path():
    d = gail.Discriminator(7, 100, torch.device("cpu"))
    x = torch.zeros(4, 5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        d.update([], None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        d.predict_reward(x, torch.zeros(4, 2), 0.99, torch.ones(4, 1))
    with pytest.raises(RuntimeError, match="no CPU path"):
        d.predict_rewards(None, 0.99)


@pytest.mark.parametrize("hidden", [0, 6, 132, 256])
def test_hidden_dim_outside_the_kernel_limits_is_refused(hidden):
    with pytest.raises(NotImplementedError, match="hidden_dim"):
        gail.Discriminator(7, hidden, torch.device("cpu"))


def test_input_dim_beyond_the_lds_is_refused():
    gail.Discriminator(145, 100, torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="LDS"):
        gail.Discriminator(393, 100, torch.device("cpu"))     # Humanoid


def test_checkpoint_state_round_trip_on_the_host():
    torch.manual_seed(1)
    a = gail.Discriminator(7, 8, torch.device("cpu"))
    a.returns = torch.randn(4, 1)
    a._rms.copy_(torch.tensor([0.5, 2.0, 9.0001], dtype=torch.float64))
    a.optimizer.step_count = 3
    a.optimizer.exp_avg, a.optimizer.exp_avg_sq = torch.randn(a.numel), torch.rand(a.numel)
    st = a.checkpoint_state()
    b = gail.Discriminator(7, 8, torch.device("cpu"))
    b.load_checkpoint_state(st)
    assert torch.equal(a.flat, b.flat) and torch.equal(a.returns, b.returns)
    assert (b.ret_rms.mean, b.ret_rms.var, b.ret_rms.count) == (0.5, 2.0, 9.0001)
    assert b.optimizer.step_count == 3 and torch.equal(a.optimizer.exp_avg_sq, b.optimizer.exp_avg_sq)
    assert b.flat.data_ptr() == next(b.trunk.parameters()).data_ptr()
    with pytest.raises(ValueError):
        gail.Discriminator(7, 12, torch.device("cpu")).load_checkpoint_state(st)


def test_gail_arguments_have_the_reference_defaults():
    a = get_args([])
    assert (a.gail, a.gail_experts_dir, a.gail_batch_size, a.gail_epoch) == (False, "./gail_experts", 128, 5)
    assert get_args(["--gail", "--gail-batch-size", "64"]).gail_batch_size == 64
