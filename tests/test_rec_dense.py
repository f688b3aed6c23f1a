"""The dense kernels around the GRU at the recurrent policy's shapes, through the C
ABI against float64 (torch on the CPU from the same fp32 inputs): the input
projection / MLP layers (ppo_linear_fwd_ex), the dgrad through the fc ReLU or a tanh
(ppo_linear_dgrad_ex), the GRU weight gradients (ppo_linear_wgrad + ppo_wgrad_reduce
kinds 0 and 3), and the exact helpers ppo_gru_pack, ppo_concat_cols, ppo_rec_indices.

Shapes leave one 128-row tile (M = 129 = one full tile + one row; M = 300), take
c5's padded input width (I = 270 -> Ip = 272) and the 3H x Ip / 3H x H weight shapes of
H = 64 and H = 256.  Bar: max|err| <= 1e-5 * max|ref|, the rule of test_dense.py and
test_small_batch.py for fp32 sums of <= 1,568 terms.  Outputs start as NaN with 64
NaN guard rows behind them; strided outputs keep NaN in their padding columns."""
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64


def _hip():
    from a2c_ppo_acktr import _hip
    return _hip


def _s():
    return torch.cuda.current_stream().cuda_stream


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _close(name, got, ref, rel=1e-5):
    got, ref = got.cpu().double(), ref.double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), (name, "non-finite", int((~torch.isfinite(got)).sum()))
    err, mx = (got - ref).abs().max().item(), ref.abs().max().item()
    print(f"{name}: max|err| {err:.3e}  max|ref| {mx:.3f}  bound {rel * mx:.3e}", flush=True)
    assert err <= rel * mx, (name, err, rel * mx)


# ------------------------------------------------------------ ppo_linear_fwd_ex
@pytest.mark.parametrize("M,K,lda,N,ldo,act,gather", [(129, 272, 272, 768, 768, 0, 0), (129, 272, 272, 768, 772, 0, 140),
                                                      (300, 80, 84, 192, 196, 2, 0)])
def test_linear_fwd_ex_vs_float64(gpu, M, K, lda, N, ldo, act, gather):
    """out[m*ldo + n] = act(x[idx(m)*lda .. + K) · w[n] + b[n]): the GRU input projection
    at Ip = 272 over one full 128-row tile plus one row (plain, and with an A-row gather
    of 129 out of 140 rows into a wider output), and an MLP tanh layer with strided
    input and output.  The input's padding columns (lda > K) hold NaN: never read."""
    Hh = _hip()
    g = torch.Generator().manual_seed(M + K + N + ldo)
    rows = gather or M
    x = torch.randn(rows, lda, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = 0.1 * torch.randn(N, generator=g)
    idx = torch.randperm(rows, generator=g)[:M] if gather else None
    xin = x.clone()
    xin[:, K:] = float("nan")
    out = _nan(M + GUARD, ldo)
    xd, wd, bd = xin.cuda(), w.cuda(), b.cuda()
    idxd = idx.cuda() if gather else None
    Hh.call("ppo_linear_fwd_ex", xd.data_ptr(), None if idxd is None else idxd.data_ptr(), M, K, lda, wd.data_ptr(),
            bd.data_ptr(), N, out.data_ptr(), ldo, act, _s())
    torch.cuda.synchronize()
    xs = x[idx] if gather else x
    ref = xs[:, :K].double() @ w.double().t() + b.double()
    if act == 2:
        ref = torch.tanh(ref)
    _close("linear_fwd_ex", out[:M, :N], ref)
    assert torch.isnan(out[:M, N:]).all()   # the padding columns are untouched
    assert torch.isnan(out[M:]).all()       # nothing stored past row M


# ---------------------------------------------------------- ppo_linear_dgrad_ex
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("M,K,N,ldact", [(129, 768, 256, 272), (99, 192, 64, 80)])
def test_linear_dgrad_ex_vs_float64(gpu, M, K, N, ldact, mode):
    """dx [M][N] = g(act) * (dy [M][K] · W [K][N]), W given transposed ([N][K] rows, as
    ppo_gru_pack's wihT); act rows have stride ldact (the padded GRU input x, whose
    first N columns are the fc output): mode 1 g = [act > 0], mode 2 g = 1 - act²."""
    Hh = _hip()
    g = torch.Generator().manual_seed(M + K + N + mode)
    dy = torch.randn(M, K, generator=g)
    W = torch.randn(K, N, generator=g) / K ** 0.5
    a = torch.randn(M, N, generator=g)
    if mode == 2:
        a = torch.tanh(a)
    act = torch.full((M, ldact), float("nan"))
    act[:, :N] = a
    dx = _nan(M + GUARD, N)
    dyd, wtd, actd = dy.cuda(), W.t().contiguous().cuda(), act.cuda()
    Hh.call("ppo_linear_dgrad_ex", dyd.data_ptr(), M, K, wtd.data_ptr(), N, actd.data_ptr(), ldact, mode,
            dx.data_ptr(), _s())
    torch.cuda.synchronize()
    ref = dy.double() @ W.double()
    ref = ref * ((a > 0).double() if mode == 1 else 1 - a.double() ** 2)
    _close("linear_dgrad_ex", dx[:M], ref)
    if mode == 1:
        assert (dx[:M].cpu()[a <= 0] == 0).all()
    assert torch.isnan(dx[M:]).all()


# ------------------------------------------- ppo_linear_wgrad + ppo_wgrad_reduce
@pytest.mark.parametrize("Z", ["splits", 1, 7])
@pytest.mark.parametrize("R,N,K,kind,a", [(99, 192, 64, 0, 0), (160, 768, 256, 0, 0), (160, 768, 272, 3, 270)])
def test_linear_wgrad_reduce_vs_float64(gpu, R, N, K, kind, a, Z):
    """dW[n][k] = Σ_r dy[r][n] x[r][k], db[n] = Σ_r dy[r][n]: the split-K slabs of
    ppo_linear_wgrad reduced by ppo_wgrad_reduce — kind 0 (dW_hh, [N][K]) and kind 3
    (dW_ih: the K - a padding columns of x cut, result [N][a]).  Z as the engine's
    _dense_wgrad takes it from ppo_wgrad_splits, 1, and 7 (more slabs than 32-row
    chunks at R = 99 / 160: the empty slabs must come out as zeros).  The padding
    columns of x hold 1000, so a leak of one into the result cannot pass.  A second
    identical launch gives the same bits."""
    Hh = _hip()
    g = torch.Generator().manual_seed(R + N + K)
    dy = torch.randn(R, N, generator=g)
    x = torch.randn(R, K, generator=g)
    width = a if kind == 3 else K
    x[:, width:] = 1000.0
    if Z == "splits":
        Z = Hh.call("ppo_wgrad_splits", R, ((N + 127) // 128) * ((K + 127) // 128), 2048, 16)
    assert Z >= 1
    dyd, xd = dy.cuda(), x.cuda()
    runs = []
    for _ in range(2):
        slab, slab_b = _nan(Z * N * K), _nan(Z * N)
        gw, gb = _nan(N * width + GUARD), _nan(N + GUARD)
        Hh.call("ppo_linear_wgrad", dyd.data_ptr(), xd.data_ptr(), R, N, K, Z, slab.data_ptr(), slab_b.data_ptr(), _s())
        Hh.call("ppo_wgrad_reduce", slab.data_ptr(), slab_b.data_ptr(), Z, N, K, kind, a, 0, gw.data_ptr(),
                gb.data_ptr(), 1.0, 0, _s())
        torch.cuda.synchronize()
        runs.append((gw, gb))
    gw, gb = runs[0]
    _close(f"wgrad Z={Z} dW", gw[:N * width].view(N, width), dy.double().t() @ x[:, :width].double())
    _close(f"wgrad Z={Z} db", gb[:N], dy.double().sum(0))
    assert torch.isnan(gw[N * width:]).all() and torch.isnan(gb[N:]).all()
    assert torch.equal(gw[:N * width], runs[1][0][:N * width]) and torch.equal(gb[:N], runs[1][1][:N])


# ------------------------------------------------------------------ ppo_gru_pack
@pytest.mark.parametrize("H,I,Ip", [(64, 78, 80), (256, 270, 272)])
def test_gru_pack_exact(gpu, H, I, Ip):
    """W_ih [3H][I] -> zero-padded [3H][Ip], W_ih[:, :H]ᵀ [H][3H], W_hhᵀ [H][3H] (the
    layouts ppo_hip.h names), bit for bit; the pad columns are exactly 0."""
    Hh = _hip()
    g = torch.Generator().manual_seed(H + I)
    wih = torch.randn(3 * H, I, generator=g)
    whh = torch.randn(3 * H, H, generator=g)
    wih_pad, wihT, whhT = _nan(3 * H * Ip + GUARD), _nan(3 * H * H + GUARD), _nan(3 * H * H + GUARD)
    wd, hd = wih.cuda(), whh.cuda()
    Hh.call("ppo_gru_pack", wd.data_ptr(), hd.data_ptr(), H, I, Ip, wih_pad.data_ptr(), wihT.data_ptr(),
            whhT.data_ptr(), _s())
    torch.cuda.synchronize()
    ref_pad = torch.zeros(3 * H, Ip)
    ref_pad[:, :I] = wih
    got_pad = wih_pad[:3 * H * Ip].view(3 * H, Ip).cpu()
    assert torch.equal(got_pad, ref_pad)
    assert (got_pad[:, I:] == 0).all() and not torch.signbit(got_pad[:, I:]).any()
    assert torch.equal(wihT[:3 * H * H].view(H, 3 * H).cpu(), wih[:, :H].t().contiguous())
    assert torch.equal(whhT[:3 * H * H].view(H, 3 * H).cpu(), whh.t().contiguous())
    for t, nel in ((wih_pad, 3 * H * Ip), (wihT, 3 * H * H), (whhT, 3 * H * H)):
        assert torch.isnan(t[nel:]).all()


# --------------------------------------------------------------- ppo_concat_cols
@pytest.mark.parametrize("rows,src_rows,ncols,ld,col0,zero_to,use_idx", [(37, 37, 14, 84, 64, 20, False),
                                                                         (37, 50, 14, 84, 64, 20, True),
                                                                         (300, 300, 14, 272, 256, 16, True),
                                                                         (33, 33, 0, 68, 64, 4, False)])
def test_concat_cols_exact(gpu, rows, src_rows, ncols, ld, col0, zero_to, use_idx):
    """dst[r][col0 + c] = src[idx(r)][c] for c < ncols, 0 for ncols <= c < zero_to
    (zero_to > ncols: the GRU input's zero padding); every other element of dst is
    untouched.  ncols = 0: only the zero pad is written (no vector observations)."""
    Hh = _hip()
    g = torch.Generator().manual_seed(rows + ld)
    src = torch.randn(src_rows, max(ncols, 1), generator=g)
    idx = torch.randperm(src_rows, generator=g)[:rows] if use_idx else None
    dst = _nan(rows + GUARD, ld)
    sd = src.cuda()
    idxd = idx.cuda() if use_idx else None
    Hh.call("ppo_concat_cols", sd.data_ptr(), None if idxd is None else idxd.data_ptr(), rows, ncols, dst.data_ptr(),
            ld, col0, zero_to, _s())
    torch.cuda.synchronize()
    got = dst.cpu()
    picked = src[idx] if use_idx else src
    assert torch.equal(got[:rows, col0:col0 + ncols], picked[:rows, :ncols])
    pad = got[:rows, col0 + ncols:col0 + zero_to]
    assert (pad == 0).all() and not torch.signbit(pad).any()
    assert torch.isnan(got[:rows, :col0]).all() and torch.isnan(got[:rows, col0 + zero_to:]).all()
    assert torch.isnan(got[rows:]).all()


# --------------------------------------------------------------- ppo_rec_indices
@pytest.mark.parametrize("T,N,n", [(3, 40, 33), (5, 6, 3), (300, 7, 5)])
def test_rec_indices_exact(gpu, T, N, n):
    """idx[t*n + j] = t*N + envs[j] for an unordered choice of envs (the
    recurrent_generator's sample order, storage.py:195-220)."""
    Hh = _hip()
    envs = torch.randperm(N, generator=torch.Generator().manual_seed(T + N))[:n]
    assert not torch.equal(envs, envs.sort().values)
    idx = torch.full((T * n + GUARD,), -7, dtype=torch.int64, device=gpu)
    ed = envs.cuda()
    Hh.call("ppo_rec_indices", ed.data_ptr(), n, T, N, idx.data_ptr(), _s())
    torch.cuda.synchronize()
    ref = (torch.arange(T)[:, None] * N + envs[None, :]).reshape(-1)
    assert torch.equal(idx[:T * n].cpu(), ref)
    assert (idx[T * n:] == -7).all()
