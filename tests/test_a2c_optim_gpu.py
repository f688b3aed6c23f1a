"""ppo_grad_sumsq + ppo_clip_rmsprop_guarded (optim.hip) against torch.optim.RMSprop
(foreach=False) + clip_grad_norm_ on CPU fp32 fed the same gradients: three consecutive
steps at n = 1, 255, 1025 (the tail handling) and 1,048,579 (more than the 1,024 partial
blocks' first pass), gradient magnitudes from 1e-6 to 1e2, with clipping, without
(max_norm <= 0) and with scale = 0.5; and the device guards."""
import numpy as np
import pytest
import torch

from helpers import a2c_ref as R

pytestmark = pytest.mark.gpu

LR, ALPHA, EPS = 7e-4, 0.99, 1e-5
SIZES = [1, 255, 1025, 1048579]
VARIANTS = {"clip": (0.5, 1.0), "noclip": (-1.0, 1.0), "scale": (0.5, 0.5)}   # (max_norm, scale)


def _hip():
    from a2c_ppo_acktr import _hip
    return _hip


def _s():
    return torch.cuda.current_stream().cuda_stream


def _inputs(n, steps=3):
    """parameters N(0, 1); gradients N(0, 1) * 10^e with e rising linearly with the position
    from -6 to 2 (a flat buffer whose later layers have the larger gradients).  The order
    matters to the reference, not to the kernel: torch's CPU fp32 vector_norm accumulates in
    fp32, and at n = 1,048,579 with the same magnitudes shuffled it is itself 2.6e-5 from the
    float64 norm (the small squares are lost once its accumulators are large), which no
    kernel could match to 1e-6; with the magnitudes ascending it is 1.1e-7 from float64."""
    g = np.random.default_rng(n)
    p0 = g.normal(size=n).astype(np.float32)
    grads = [(g.normal(size=n) * 10.0 ** np.linspace(-6, 2, n)).astype(np.float32) for _ in range(steps)]
    return p0, grads


def _step(Hh, p, g, sq, parts, nrm, scale, max_norm, gi=None, gd=None, sk=None):
    n = p.numel()
    Hh.call("ppo_grad_sumsq", g.data_ptr(), n, scale, parts.data_ptr(), _s())
    Hh.call("ppo_clip_rmsprop_guarded", p.data_ptr(), g.data_ptr(), sq.data_ptr(), n, parts.data_ptr(), scale,
            max_norm, LR, ALPHA, EPS, nrm.data_ptr(), gi, gd, sk, _s())
    torch.cuda.synchronize()


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("n", SIZES)
def test_clip_rmsprop_vs_torch_cpu(gpu, n, variant):
    """per step: total norm rtol 1e-6, clipped gradient rtol 1e-5 / atol 1e-9, parameters
    atol 1e-6, square_avg rtol 2e-6 (a2c_ref.check_rmsprop) against torch's CPU fp32"""
    Hh = _hip()
    max_norm, scale = VARIANTS[variant]
    p0, grads = _inputs(n)
    ref_p = torch.from_numpy(p0.copy()).requires_grad_()
    opt = torch.optim.RMSprop([ref_p], LR, eps=EPS, alpha=ALPHA, foreach=False)
    p = torch.from_numpy(p0.copy()).to(gpu)
    sq = torch.zeros(n, device=gpu)
    parts = torch.zeros(Hh.call("ppo_grad_partials_count", n), dtype=torch.float64, device=gpu)
    nrm = torch.full((1,), float("nan"), dtype=torch.float64, device=gpu)
    for k, gk in enumerate(grads):
        ref_p.grad = torch.from_numpy(gk.copy()) * scale          # the averaged gradient (exact in fp32 at 0.5)
        if max_norm > 0:
            total = torch.nn.utils.clip_grad_norm_([ref_p], max_norm, foreach=False)
        else:
            total = ref_p.grad.norm()
        opt.step()
        g = torch.from_numpy(gk.copy()).to(gpu)
        _step(Hh, p, g, sq, parts, nrm, scale, max_norm)
        print("step", k)
        R.check_rmsprop((nrm.item(), g.cpu().numpy(), p.cpu().numpy(), sq.cpu().numpy()),
                        (total.item(), ref_p.grad.numpy(), ref_p.detach().numpy(), opt.state[ref_p]["square_avg"].numpy()))
    if variant == "clip" and n > 1:
        assert total.item() > 0.5   # the clip was active


@pytest.mark.parametrize("which", ["guard_i", "guard_d"])
def test_clip_rmsprop_guards_skip_the_step(gpu, which):
    """*guard_i = 1 or *guard_d = 1.0: parameters, gradient and square_avg stay bit-unchanged
    and *skipped goes 0 -> 1; with both guards clear the same call steps and leaves it at 1"""
    Hh = _hip()
    n = 1025
    p0, grads = _inputs(n, 1)
    p, g = torch.from_numpy(p0.copy()).to(gpu), torch.from_numpy(grads[0].copy()).to(gpu)
    sq = torch.rand(n, device=gpu)
    keep = [x.clone() for x in (p, g, sq)]
    parts = torch.zeros(Hh.call("ppo_grad_partials_count", n), dtype=torch.float64, device=gpu)
    nrm = torch.zeros(1, dtype=torch.float64, device=gpu)
    gi = torch.tensor([1 if which == "guard_i" else 0], dtype=torch.int32, device=gpu)
    gd = torch.tensor([1.0 if which == "guard_d" else 0.0], dtype=torch.float64, device=gpu)
    sk = torch.zeros(1, dtype=torch.int32, device=gpu)
    _step(Hh, p, g, sq, parts, nrm, 1.0, 0.5, gi.data_ptr(), gd.data_ptr(), sk.data_ptr())
    assert int(sk.item()) == 1
    for a, b in zip((p, g, sq), keep):
        assert torch.equal(a, b)
    gi.zero_()
    gd.zero_()
    _step(Hh, p, g, sq, parts, nrm, 1.0, 0.5, gi.data_ptr(), gd.data_ptr(), sk.data_ptr())
    assert int(sk.item()) == 1
    assert not torch.equal(p, keep[0]) and not torch.equal(sq, keep[2]) and not torch.equal(g, keep[1])
