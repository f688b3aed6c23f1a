"""CPU checks of tests/helpers/gru_ref.py: the float64 GRU sequence / BPTT on given
gi equals the oracle's gru_sequence_cache / gru_backward (pinned to the reference by
test_oracle_golden.py), the inputs of tests/test_gru_sequence.py meet its input
conditions, and its comparison logic rejects the mistakes it is there to catch —
shown by handing it the fp32 yardstick run on deliberately wrong masks or rows in
the kernel's place."""
import numpy as np
import pytest
import torch

from helpers import gru_ref as GR
from oracle import ppo_oracle as O


def test_gru_ref_equals_oracle():
    """helper (gi given) vs oracle (x, W_ih given), float64, masks with zeros: outputs,
    every saved gate, dx = dgi·W_ih and the four GRU parameter gradients to 1e-12."""
    rng = np.random.default_rng(3)
    T, n, H, I = 4, 5, 8, 11
    p = {"base.gru.weight_ih_l0": rng.standard_normal((3 * H, I)) / I ** 0.5,
         "base.gru.weight_hh_l0": rng.standard_normal((3 * H, H)) / H ** 0.5,
         "base.gru.bias_ih_l0": 0.1 * rng.standard_normal(3 * H), "base.gru.bias_hh_l0": 0.1 * rng.standard_normal(3 * H)}
    x = rng.standard_normal((T * n, I))
    h0 = 0.5 * rng.standard_normal((n, H))
    masks = (rng.random((T, n)) >= 0.3).astype(np.float64)
    assert (masks[1:] == 0).any() and (masks[1:] == 1).any()
    dout = rng.standard_normal((T * n, H))
    out, cache = O.gru_sequence_cache(p, x, h0, masks)
    grads, dx = O.gru_backward(p, x, masks, cache, dout)
    gi = x @ p["base.gru.weight_ih_l0"].T + p["base.gru.bias_ih_l0"]
    m = GR.mask_plane(masks, T, n)
    f = GR.gru_seq_forward(h0, p["base.gru.weight_hh_l0"], p["base.gru.bias_hh_l0"], gi, m)
    np.testing.assert_allclose(f["h"].numpy(), out, rtol=0, atol=1e-12)
    for k, i in (("hin", 0), ("r", 1), ("z", 2), ("n", 3), ("ghn", 4)):
        np.testing.assert_allclose(f[k].numpy(), np.concatenate([c[i] for c in cache], 0), rtol=0, atol=1e-12)
    b = GR.gru_seq_backward(dout, {k: f[k] for k in ("r", "z", "n", "ghn", "hin")}, p["base.gru.weight_hh_l0"], m)
    dgi, dgh = b["dgi"].numpy(), b["dgh"].numpy()
    np.testing.assert_allclose(dgi @ p["base.gru.weight_ih_l0"], dx, rtol=0, atol=1e-12)
    np.testing.assert_allclose(dgi.T @ x, grads["base.gru.weight_ih_l0"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(dgi.sum(0), grads["base.gru.bias_ih_l0"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(dgh.T @ f["hin"].numpy(), grads["base.gru.weight_hh_l0"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(dgh.sum(0), grads["base.gru.bias_hh_l0"], rtol=0, atol=1e-12)
    # the final dhz / carry as the step loop leaves them: step 0's dh'·z, step 1's carry
    r, z, nn, ghn, hin = (f[k].numpy().reshape(T, n, H) for k in ("r", "z", "n", "ghn", "hin"))
    dh0 = dgi[:n, 2 * H:] / ((1 - z[0]) * (1 - nn[0] ** 2))
    np.testing.assert_allclose(b["dhz"].numpy(), dh0 * z[0], rtol=0, atol=1e-9)
    np.testing.assert_allclose(b["carry"].numpy(), dh0 - dout[:n], rtol=0, atol=1e-9)
    one = GR.gru_seq_backward(dout[:n], {k: f[k][:n] for k in ("r", "z", "n", "ghn", "hin")},
                              p["base.gru.weight_hh_l0"], m[:1])
    assert one["carry"] is None


def test_mask_plane_through_index():
    T, n, N = 3, 4, 6
    plane = torch.arange(T * N, dtype=torch.float32)
    envs = torch.tensor([5, 0, 3, 2])
    idx = (torch.arange(T)[:, None] * N + envs[None, :]).reshape(-1)
    m = GR.mask_plane(plane, T, n, idx)
    assert m.tolist() == [[5, 0, 3, 2], [11, 6, 9, 8], [17, 12, 15, 14]]
    assert torch.equal(GR.mask_plane(plane[:T * n], T, n), plane[:T * n].reshape(T, n))


@pytest.mark.parametrize("T,n,H,use_idx", GR.SEQ_SHAPES)
def test_sequence_inputs_meet_their_conditions(T, n, H, use_idx):
    d = GR.seq_inputs(T, n, H, use_idx)
    print("zero-mask entries past the first group at t >= 1:", GR.check_mask_conditions(d["m"]))
    for k in ("h", "r", "z", "n", "ghn", "hin"):   # the yardstick itself sits far below the floor
        tol, yard = GR.seq_tol(d["fwd64"][k], d["fwd32"][k])
        assert yard < 2e-6 and tol == GR.FLOOR * max(d["fwd64"][k].abs().max().item(), 1.0), (k, yard, tol)
    for k in ("dgi", "dgh", "dhz", "carry"):
        tol, yard = GR.seq_tol(d["bwd64"][k], d["bwd32"][k])
        assert yard < 2e-6 and tol == GR.FLOOR * max(d["bwd64"][k].abs().max().item(), 1.0), (k, yard, tol)


def _wrong_masks(m, how):
    """masks wrong only past the first 32-row group: dropped (1 everywhere) or
    misplaced (row j takes row j - 1's)"""
    w = m.clone()
    w[:, 32:] = 1.0 if how == "dropped" else torch.roll(m, 1, 1)[:, 32:]
    return w


def _fwd_all(d, f):
    for k in ("h", "r", "z", "n", "ghn", "hin"):
        GR.check_close(k, f[k], d["fwd64"][k], d["fwd32"][k], n=d["n"])


def _bwd_all(d, b):
    for k in ("dgi", "dgh"):
        GR.check_close(k, b[k], d["bwd64"][k], d["bwd32"][k], n=d["n"])
    for k in ("dhz", "carry"):
        GR.check_close(k, b[k], d["bwd64"][k], d["bwd32"][k])


@pytest.mark.parametrize("T,n,H,use_idx", GR.SEQ_SHAPES)
def test_comparison_accepts_the_yardstick(T, n, H, use_idx):
    d = GR.seq_inputs(T, n, H, use_idx)
    _fwd_all(d, d["fwd32"])
    _bwd_all(d, d["bwd32"])


@pytest.mark.parametrize("how", ["dropped", "misplaced"])
@pytest.mark.parametrize("T,n,H,use_idx", GR.SEQ_SHAPES)
def test_comparison_rejects_wrong_forward_mask(T, n, H, use_idx, how):
    """h_in = h·mask with the mask dropped or taken from the neighbouring row, in the
    rows of groups >= 1 only"""
    d = GR.seq_inputs(T, n, H, use_idx)
    f = GR.gru_seq_forward(d["h0"], d["whh"], d["bhh"], d["gi"], _wrong_masks(d["m"], how), dtype=torch.float32)
    with pytest.raises(AssertionError):
        _fwd_all(d, f)


@pytest.mark.parametrize("how", ["dropped", "misplaced"])
@pytest.mark.parametrize("T,n,H,use_idx", GR.SEQ_SHAPES)
def test_comparison_rejects_wrong_backward_mask(T, n, H, use_idx, how):
    """(dgh·W_hh + dh'·z)·mask with the mask dropped or taken from the neighbouring
    row, in the rows of groups >= 1 only (the saves are the true forward's)"""
    d = GR.seq_inputs(T, n, H, use_idx)
    b = GR.gru_seq_backward(d["dout"], d["saves"], d["whh"], _wrong_masks(d["m"], how), dtype=torch.float32)
    with pytest.raises(AssertionError):
        _bwd_all(d, b)


@pytest.mark.parametrize("T,n,H,use_idx", GR.SEQ_SHAPES)
def test_comparison_rejects_wrong_row_offset(T, n, H, use_idx):
    """groups >= 1 computed from (and stored to) rows one off within each step"""
    d = GR.seq_inputs(T, n, H, use_idx)

    def shifted(t, cols):
        s = t.reshape(T, n, cols).clone()
        s[:, 32:] = torch.roll(s[:, 32:], 1, 1) if n - 32 > 1 else s[:, 31:32]
        return s.reshape(T * n, cols)
    with pytest.raises(AssertionError):
        _fwd_all(d, {k: shifted(v, H) for k, v in d["fwd32"].items()})
    with pytest.raises(AssertionError):
        _bwd_all(d, dict(d["bwd32"], dgi=shifted(d["bwd32"]["dgi"], 3 * H), dgh=shifted(d["bwd32"]["dgh"], 3 * H)))


def test_guard_rows_reject_a_store_past_the_last_row():
    buf = torch.full((40 + GR.GUARD, 8), float("nan"))
    buf[:40] = 0.0
    GR.check_guard("ok", buf, 40)
    buf[40, 3] = 0.0   # the 8-row tail group of n = 40 storing a ninth row
    with pytest.raises(AssertionError):
        GR.check_guard("hit", buf, 40)
    short = torch.full((40 + GR.GUARD, 8), float("nan"))   # an output row never written
    short[:39] = 0.0
    with pytest.raises(AssertionError):
        GR.check_close("unwritten", short[:40], torch.zeros(40, 8), torch.zeros(40, 8), n=40)
