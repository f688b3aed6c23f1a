"""The GRU sequence kernels past one 32-row group, through the C ABI against a plain
float64 restatement (tests/helpers/gru_ref.py; torch on the CPU from the same fp32
inputs): ppo_gru_seq_fwd_ws and ppo_gru_seq_bwd_ws as the persistent launches
(ppo_gru_persist_set(3)) and as the step launches (0), and ppo_gru_cell_bwd.

Shapes (T, n, H, use_idx), the smallest that leave one row group:
  (4, 33, 64, no)    two groups, the second holds one row; fp32-MFMA W_hh
  (3, 64, 128, yes)  two exactly full groups
  (5, 40, 256, yes)  c5's H, 8-row tail, 2 x 16 unit blocks
  (2, 70, 512, no)   three groups x 32 unit blocks, the shortest BPTT
  (6, 97, 256, yes)  four groups, one-row tail, middle steps with carry in and out
Inputs: h0 ~ 0.5 N(0,1), W_hh ~ N(0,1)/sqrt(H), b_hh ~ 0.1 N(0,1), gi, dout ~ N(0,1),
masks 0 with p = 0.25, direct [T][n] or through idx into a [T*(n+7)] plane with
idx[t*n + j] = t*(n+7) + envs[j], envs unordered (as the engine passes them).

Bound per tensor, recomputed at run time (gru_ref.seq_tol):
  max|err| <= max(2e-5 * max(max|ref|, 1), 2 x the fp32 CPU yardstick's own error)
The first term is test_gru_step_kernels_vs_float64's single-step bound; the
yardstick is the same recurrence in fp32 torch on the CPU.  Every output buffer
starts as NaN with 64 NaN guard rows behind its last row (behind row n for dhz /
carry): outputs must be finite, guards still NaN — a partial last group storing past
row n in the last step would show only there.

tests/test_gru_ref_cpu.py shows on the CPU that this comparison rejects a mask
dropped or misplaced in the forward's h_in or in the backward's carry, a wrong row
offset, and a store past the last row, each confined to the rows of groups >= 1."""
import pytest
import torch

from helpers import gru_ref as GR

pytestmark = pytest.mark.gpu

FWD_KEYS = ("h", "r", "z", "n", "ghn", "hin")


def _hip():
    from a2c_ppo_acktr import _hip
    return _hip


def _s():
    return torch.cuda.current_stream().cuda_stream


def _nan(rows, cols, gpu):
    return torch.full((rows + GR.GUARD, cols), float("nan"), device=gpu)


def _words(Hh, n, gpu):
    """caller-owned counters (with 8 sentinel ints behind them) and error word"""
    nc = Hh.call("ppo_gru_seq_counters", n)
    assert nc == 2 * ((n + 31) // 32)
    cnt = torch.zeros(nc + 8, dtype=torch.int32, device=gpu)
    cnt[nc:] = -7
    return cnt, nc, torch.zeros(1, dtype=torch.int32, device=gpu)


def _ptr(t):
    return None if t is None else t.data_ptr()


@pytest.mark.parametrize("persist", [3, 0])
@pytest.mark.parametrize("T,n,H,use_idx", GR.SEQ_SHAPES)
def test_gru_seq_fwd_vs_float64(gpu, T, n, H, use_idx, persist):
    """ppo_gru_seq_fwd_ws with caller-owned counters and error word: hout and the five
    saves over all T steps vs float64, error word 0, guard rows untouched.

    Measured max|err| on the MI355X (persistent = step launches, bit-identical), per
    shape the largest over the six tensors, beside the fp32 CPU yardstick's:
      (4, 33, 64)   kernel 2.5e-7   yardstick 4.7e-7      (3, 64, 128)  kernel 2.1e-7   yardstick 7.4e-7
      (5, 40, 256)  kernel 3.7e-7   yardstick 5.8e-7      (2, 70, 512)  kernel 5.1e-7   yardstick 8.3e-7
      (6, 97, 256)  kernel 3.4e-7   yardstick 7.7e-7
    with max|ref| 0.98 - 2.2: the 2e-5 floor decides every bound (2.0e-5 - 4.3e-5)."""
    Hh = _hip()
    d = GR.seq_inputs(T, n, H, use_idx)
    GR.check_mask_conditions(d["m"])
    dev = {k: d[k].cuda() for k in ("h0", "masks", "whh", "bhh", "gi")}
    idx = d["idx"].cuda() if use_idx else None
    out = {k: _nan(T * n, H, gpu) for k in FWD_KEYS}
    cnt, nc, err = _words(Hh, n, gpu)
    prev = Hh.call("ppo_gru_persist_get")
    Hh.call("ppo_gru_persist_set", persist)
    try:
        Hh.call("ppo_gru_seq_fwd_ws", dev["h0"].data_ptr(), dev["masks"].data_ptr(), _ptr(idx), dev["whh"].data_ptr(),
                dev["bhh"].data_ptr(), dev["gi"].data_ptr(), T, n, H, out["h"].data_ptr(), out["r"].data_ptr(),
                out["z"].data_ptr(), out["n"].data_ptr(), out["ghn"].data_ptr(), out["hin"].data_ptr(),
                cnt.data_ptr(), err.data_ptr(), _s())
        torch.cuda.synchronize()
    finally:
        Hh.call("ppo_gru_persist_set", prev)
    assert err.item() == 0
    assert (cnt[nc:] == -7).all()
    tag = f"fwd T={T} n={n} H={H} persist={persist}"
    for k in FWD_KEYS:
        got = out[k].cpu()
        GR.check_guard(k, got, T * n)
        GR.check_close(k, got[:T * n], d["fwd64"][k], d["fwd32"][k], n=n, tag=tag)


@pytest.mark.parametrize("persist", [3, 0])
@pytest.mark.parametrize("T,n,H,use_idx", GR.SEQ_SHAPES)
def test_gru_seq_bwd_vs_float64(gpu, T, n, H, use_idx, persist):
    """ppo_gru_seq_bwd_ws on the saves of a real forward (the float64 forward's gates
    rounded to fp32, so no forward error is mixed in): dgi and dgh over all steps and
    the final dhz (step 0's dh'·z) / carry (step 1's) vs the float64 BPTT from those
    same fp32 values; error word 0; with persist 3, where ceil(n/32)·H/16 blocks fit the
    CUs, every group's report is 1 — with the clear error word: ran and finished.

    Measured max|err| on the MI355X (persistent = step launches, bit-identical), per
    shape the largest over dgi, dgh, dhz, carry, beside the fp32 CPU yardstick's:
      (4, 33, 64)   kernel 4.0e-7   yardstick 5.0e-7      (3, 64, 128)  kernel 4.0e-7   yardstick 6.0e-7
      (5, 40, 256)  kernel 5.2e-7   yardstick 8.8e-7      (2, 70, 512)  kernel 4.7e-7   yardstick 4.6e-7
      (6, 97, 256)  kernel 6.6e-7   yardstick 7.7e-7
    with max|ref| 2.4 - 4.3: the 2e-5 floor decides every bound (4.8e-5 - 8.6e-5)."""
    Hh = _hip()
    d = GR.seq_inputs(T, n, H, use_idx)
    GR.check_mask_conditions(d["m"])
    G = (n + 31) // 32
    dout, masks = d["dout"].cuda(), d["masks"].cuda()
    sv = {k: v.cuda() for k, v in d["saves"].items()}
    whhT = d["whh"].cuda().t().contiguous()
    idx = d["idx"].cuda() if use_idx else None
    out = {"dgi": _nan(T * n, 3 * H, gpu), "dgh": _nan(T * n, 3 * H, gpu), "dhz": _nan(n, H, gpu),
           "carry": _nan(n, H, gpu)}
    cnt, nc, err = _words(Hh, n, gpu)
    prev = Hh.call("ppo_gru_persist_get")
    Hh.call("ppo_gru_persist_set", persist)
    try:
        Hh.call("ppo_gru_seq_bwd_ws", dout.data_ptr(), sv["r"].data_ptr(), sv["z"].data_ptr(), sv["n"].data_ptr(),
                sv["ghn"].data_ptr(), sv["hin"].data_ptr(), masks.data_ptr(), _ptr(idx), whhT.data_ptr(), T, n, H,
                out["dgi"].data_ptr(), out["dgh"].data_ptr(), out["dhz"].data_ptr(), out["carry"].data_ptr(),
                cnt.data_ptr(), err.data_ptr(), _s())
        torch.cuda.synchronize()
    finally:
        Hh.call("ppo_gru_persist_set", prev)
    assert err.item() == 0
    assert (cnt[nc:] == -7).all()
    if persist == 3 and G * (H // 16) <= torch.cuda.get_device_properties(0).multi_processor_count:
        assert cnt[G:nc].tolist() == [1] * G, cnt[:nc].tolist()
    tag = f"bwd T={T} n={n} H={H} persist={persist}"
    for k, rows in (("dgi", T * n), ("dgh", T * n), ("dhz", n), ("carry", n)):
        got = out[k].cpu()
        GR.check_guard(k, got, rows)
        GR.check_close(k, got[:rows], d["bwd64"][k], d["bwd32"][k], n=n if rows > n else None, tag=tag)


@pytest.mark.parametrize("has_carry", [0, 1])
@pytest.mark.parametrize("M,H", [(1, 64), (33, 64), (300, 256)])
def test_gru_cell_bwd_vs_float64(gpu, M, H, has_carry):
    """ppo_gru_cell_bwd (one step's gate gradients, elementwise): dgi, dgh, dhz vs
    float64 within 1e-5 * max(max|ref|, 1); without a carry the carry buffer (NaN here)
    is not read; 64 NaN guard rows behind every output stay NaN.

    Measured max|err| on the MI355X: 5.2e-8 - 4.6e-7 at max|ref| 1.4 - 5.5."""
    Hh = _hip()
    g = torch.Generator().manual_seed(M * H + has_carry)
    dout = torch.randn(M, H, generator=g)
    carry = torch.randn(M, H, generator=g) if has_carry else torch.full((M, H), float("nan"))
    r, z = torch.rand(M, H, generator=g), torch.rand(M, H, generator=g)
    nn = torch.rand(M, H, generator=g) * 2 - 1
    ghn, hin = torch.randn(M, H, generator=g), torch.randn(M, H, generator=g)
    dh = dout.double() + (carry.double() if has_carry else 0.0)
    r6, z6, n6, g6, h6 = (t.double() for t in (r, z, nn, ghn, hin))
    dan = dh * (1 - z6) * (1 - n6 * n6)
    dar = dan * g6 * r6 * (1 - r6)
    daz = dh * (h6 - n6) * z6 * (1 - z6)
    ref = {"dgi": torch.cat([dar, daz, dan], 1), "dgh": torch.cat([dar, daz, dan * r6], 1), "dhz": dh * z6}
    out = {"dgi": _nan(M, 3 * H, gpu), "dgh": _nan(M, 3 * H, gpu), "dhz": _nan(M, H, gpu)}
    ins = [t.cuda() for t in (dout, carry, r, z, nn, ghn, hin)]
    Hh.call("ppo_gru_cell_bwd", *[t.data_ptr() for t in ins], out["dgi"].data_ptr(), out["dgh"].data_ptr(),
            out["dhz"].data_ptr(), M, H, has_carry, _s())
    torch.cuda.synchronize()
    for k, v in ref.items():
        got = out[k].cpu()
        GR.check_guard(k, got, M)
        assert torch.isfinite(got[:M]).all(), k
        e = (got[:M].double() - v).abs().max().item()
        print(f"cell_bwd M={M} H={H} carry={has_carry} {k}: max|err| {e:.3e}  max|ref| {v.abs().max().item():.3f}",
              flush=True)
        assert e <= 1e-5 * max(v.abs().max().item(), 1.0), (k, e)
