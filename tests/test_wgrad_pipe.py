"""ppo_linear_wgrad's pipelined k loop (knob wgrad_pipe = 1, igemm_x9.h: split-and-store
inside the MFMA stream, loads issued mid-step, last two k-steps peeled) against the plain
loop (knob 0): slab and slab_bias must agree bit for bit, torch.equal, under products 1, 6
and 9.

Shapes (N, K): the fc layer (512, 1568: a ragged 13th column tile), one row tile with a
ragged second column tile (128, 136), the GRU's dW_hh (768, 256: no remainder).  Rows and
splits (R, Z): one k-step (the peeled last step alone), two with the second ragged, three,
one k-step per split, a long odd loop, and a split that receives no rows (it writes
zeros).  One integer-valued case, reduced by ppo_wgrad_reduce, is compared with float64
with no tolerance.

The operands are followed by NaN rows (a read past row R would show), the slabs start as
NaN with NaN guard rows behind them."""
import pytest
import torch

from test_conv_gpu import _Knobs

pytestmark = pytest.mark.gpu

GUARD = 64
SHAPES = [(512, 1568), (128, 136), (768, 256)]
ROWS = [(32, 1), (40, 1), (96, 1), (96, 3), (2080, 3), (32, 2)]


def _hip():
    from a2c_ppo_acktr import _hip
    return _hip


def _s():
    return torch.cuda.current_stream().cuda_stream


def _padded(t, gpu):
    """t [R][C] on the device with 8 NaN rows behind it"""
    buf = torch.full((t.shape[0] + 8, t.shape[1]), float("nan"), device=gpu)
    buf[:t.shape[0]] = t
    return buf


def _wgrad(gpu, dy, x, R, N, K, Z, pipe, products):
    slab = torch.full((Z * N * K + GUARD,), float("nan"), device=gpu)
    slab_b = torch.full((Z * N + GUARD,), float("nan"), device=gpu)
    with _Knobs(products=products, wgrad_pipe=pipe):
        _hip().call("ppo_linear_wgrad", dy.data_ptr(), x.data_ptr(), R, N, K, Z, slab.data_ptr(), slab_b.data_ptr(),
                    _s())
    torch.cuda.synchronize()
    return slab, slab_b


@pytest.mark.parametrize("R,Z", ROWS, ids=[f"R{r}Z{z}" for r, z in ROWS])
@pytest.mark.parametrize("N,K", SHAPES, ids=[f"N{n}K{k}" for n, k in SHAPES])
def test_pipe_equals_plain(gpu, N, K, R, Z):
    g = torch.Generator(device=gpu).manual_seed(7001 + N + K + R + Z)
    dy = _padded(torch.randn(R, N, device=gpu, generator=g), gpu)
    x = _padded(torch.randn(R, K, device=gpu, generator=g), gpu)
    for products in (1, 6, 9):
        what = f"linear_wgrad N={N} K={K} R={R} Z={Z} products={products}"
        (s0, b0), (s1, b1) = (_wgrad(gpu, dy, x, R, N, K, Z, pipe, products) for pipe in (0, 1))
        for name, t, n in (("slab", s0, Z * N * K), ("slab", s1, Z * N * K), ("slab_bias", b0, Z * N),
                           ("slab_bias", b1, Z * N)):
            assert not torch.isnan(t[:n]).any(), f"{what}: {name} elements left unwritten"
            assert torch.isnan(t[n:]).all(), f"{what}: {name} written past its end"
        assert s0[:Z * N * K].abs().max() > 0, what + ": a zero result compares nothing"
        chunk = -(-((R + 31) // 32) // Z) * 32   # rows per split; a split that starts past row R has none
        full = -(-R // chunk)
        assert (s1[full * N * K:Z * N * K] == 0).all() and (b1[full * N:Z * N] == 0).all(), what + ": empty split"
        for name, a, b, n in (("slab", s0, s1, Z * N * K), ("slab_bias", b0, b1, Z * N)):
            if not torch.equal(a[:n], b[:n]):
                bad = (a[:n] != b[:n]).nonzero()
                raise AssertionError(f"{what}: {len(bad)} {name} elements differ between the pipelined and the "
                                     f"plain loop, first at {bad[0].tolist()}")


def test_pipe_vs_float64(gpu):
    """small integers: every product and every partial sum is exact in fp32 (and the operands
    in bf16, so also under products = 1); |dW| <= 2080 * 64 < 2^24"""
    N, K, R, Z = 512, 1568, 2080, 3
    g = torch.Generator().manual_seed(7002)
    dy = torch.randint(-8, 9, (R, N), generator=g).float()
    x = torch.randint(-8, 9, (R, K), generator=g).float()
    ref_w = dy.double().t() @ x.double()
    ref_b = dy.double().sum(0)
    dyd, xd = _padded(dy, gpu), _padded(x, gpu)
    for products in (1, 6, 9):
        what = f"linear_wgrad integers products={products} pipelined loop"
        slab, slab_b = _wgrad(gpu, dyd, xd, R, N, K, Z, 1, products)
        gw = torch.full((N * K + GUARD,), float("nan"), device=gpu)
        gb = torch.full((N + GUARD,), float("nan"), device=gpu)
        _hip().call("ppo_wgrad_reduce", slab.data_ptr(), slab_b.data_ptr(), Z, N, K, 0, 0, 0, gw.data_ptr(),
                    gb.data_ptr(), 1.0, 0, _s())
        torch.cuda.synchronize()
        assert torch.isnan(gw[N * K:]).all() and torch.isnan(gb[N:]).all(), what
        assert torch.equal(gw[:N * K].view(N, K).cpu().double(), ref_w), what + ": dW differs from float64"
        assert torch.equal(gb[:N].cpu().double(), ref_b), what + ": db differs from float64"
