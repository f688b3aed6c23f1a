"""Plain GRU sequence forward and backward through time on given input-gate
pre-activations gi [T*n, 3H] — what ppo_gru_seq_fwd_ws / ppo_gru_seq_bwd_ws compute —
in float64 (the reference) or fp32 (the precision yardstick), torch on the CPU.

A restatement of oracle/ppo_oracle.py gru_sequence_cache / gru_backward (which
test_oracle_golden.py pins to the reference) with gi = x·W_ihᵀ + b_ih taken as an
input, as the kernels take it; tests/test_gru_ref_cpu.py holds the two together.
Rows of step t are t*n .. t*n + n - 1, gate order (r, z, n), h_in(t) = h(t-1)·m(t).

Also here, because the GPU tests and the CPU checks of the comparison logic share
them: the inputs of tests/test_gru_sequence.py (seq_inputs), its tolerance rule
(seq_tol, check_close) and its guard-row check (check_guard)."""
import functools

import numpy as np
import torch

# (T, n, H, use_idx): the smallest shapes that leave one 32-row group
SEQ_SHAPES = [(4, 33, 64, False), (3, 64, 128, True), (5, 40, 256, True), (2, 70, 512, False), (6, 97, 256, True)]
GUARD = 64          # NaN rows behind every output buffer
FLOOR = 2e-5        # the single-step bound of test_gru_step_kernels_vs_float64


def mask_plane(masks, T, n, idx=None):
    """the masks the kernels apply, [T][n]: direct (masks [T*n]) or through the
    minibatch index into a [T*N] plane, m[t][j] = masks[idx[t*n + j]]"""
    m = torch.as_tensor(masks).reshape(-1)
    if idx is not None:
        m = m[torch.as_tensor(idx).reshape(-1)]
    return m.reshape(T, n)


def gru_seq_forward(h0, whh, bhh, gi, m, dtype=torch.float64):
    """h0 [n, H], whh [3H, H], bhh [3H], gi [T*n, 3H], m [T, n] (mask_plane) ->
    dict of [T*n, H] tensors: h (the outputs), r, z, n, ghn = W_hn·h_in + b_hn, hin"""
    T, n = m.shape
    H = h0.shape[1]
    h0, whh, bhh, gi, m = (torch.as_tensor(t).to(dtype) for t in (h0, whh, bhh, gi, m))
    gi = gi.reshape(T, n, 3 * H)
    out = {k: [] for k in ("h", "r", "z", "n", "ghn", "hin")}
    h = h0
    for t in range(T):
        hin = h * m[t][:, None]
        gh = hin @ whh.t() + bhh
        r = torch.sigmoid(gi[t][:, :H] + gh[:, :H])
        z = torch.sigmoid(gi[t][:, H:2 * H] + gh[:, H:2 * H])
        ghn = gh[:, 2 * H:]
        nn = torch.tanh(gi[t][:, 2 * H:] + r * ghn)
        h = (1 - z) * nn + z * hin
        for k, v in (("h", h), ("r", r), ("z", z), ("n", nn), ("ghn", ghn), ("hin", hin)):
            out[k].append(v)
    return {k: torch.cat(v, 0) for k, v in out.items()}


def gru_seq_backward(dout, sv, whh, m, dtype=torch.float64):
    """BPTT over the saved gates sv = {r, z, n, ghn, hin} ([T*n, H] each) with
    dout [T*n, H] = dL/d(outputs) -> dict:
      dgi, dgh [T*n, 3H]  the gate gradients of every step;
      dhz [n, H]          what ppo_gru_seq_bwd_ws leaves in dhz: the buffer is
                          rewritten by every cell backward, last by step 0's, so it
                          ends as dh'(0)·z(0) with dh'(0) = dout(0) + carry;
      carry [n, H]        what it leaves in carry: the loop runs t = T-1 .. 1 and step
                          t writes (dgh(t)·W_hh + dh'(t)·z(t))·m(t), the gradient
                          flowing into h(t-1); the last one computed is step 1's (the
                          carry step 0's cell backward consumed).  There is no carry
                          for h0: m(0) is never applied in the backward.  T = 1
                          writes none (None here)."""
    T, n = m.shape
    H = whh.shape[1]
    dout, whh, m = (torch.as_tensor(t).to(dtype) for t in (dout, whh, m))
    sv = {k: torch.as_tensor(v).to(dtype).reshape(T, n, H) for k, v in sv.items()}
    do = dout.reshape(T, n, H)
    dgi, dgh = [None] * T, [None] * T
    carry, last, dhz = torch.zeros(n, H, dtype=dtype), None, None
    for t in range(T - 1, -1, -1):
        r, z, nn, ghn, hin = (sv[k][t] for k in ("r", "z", "n", "ghn", "hin"))
        dh = do[t] + carry
        dn = dh * (1 - z)
        dz = dh * (hin - nn)
        dan = dn * (1 - nn * nn)
        dar = dan * ghn * r * (1 - r)
        daz = dz * z * (1 - z)
        dgi[t] = torch.cat([dar, daz, dan], 1)
        dgh[t] = torch.cat([dar, daz, dan * r], 1)
        dhz = dh * z
        if t > 0:
            carry = (dgh[t] @ whh + dhz) * m[t][:, None]
            last = carry
    return {"dgi": torch.cat(dgi, 0), "dgh": torch.cat(dgh, 0), "dhz": dhz, "carry": last}


def check_mask_conditions(m):
    """the input conditions of the sequence tests, on m [T][n] (mask_plane): among the
    rows of groups >= 1 (row >= 32), at steps t >= 1 (step 0's mask acts on h0 only in
    the forward and never in the backward), one row is cut (mask 0 at some step) and
    one carries through (mask 1 at every step).  A second group of a single row
    (n = 33) cannot hold two such rows: that row must then show both values.
    Returns the number of zero entries counted."""
    m = np.asarray(m)
    T, n = m.shape
    assert n > 32 and T >= 2, (T, n)
    g = m[1:, 32:]
    zeros = int((g == 0).sum())
    assert zeros >= 1, "no masked row past the first group at t >= 1"
    if n - 32 > 1:
        assert (g == 1).all(0).any(), "no row past the first group with mask 1 throughout"
    else:
        assert (g == 1).any(), "the second group's only row is masked at every step"
    return zeros


@functools.lru_cache(maxsize=None)
def seq_inputs(T, n, H, use_idx):
    """inputs of one sequence shape (CPU fp32 tensors; seed T*n + H) with the float64
    reference and the fp32 yardstick of both directions, computed once per shape.
    The backward's saves are the float64 forward's gates rounded to fp32 — a real
    forward, and its reference is computed from those same fp32 values."""
    g = torch.Generator().manual_seed(T * n + H)
    N = n + 7
    if use_idx:
        masks = (torch.rand(T * N, generator=g) >= 0.25).float()
        envs = torch.randperm(N, generator=g)[:n]
        idx = (torch.arange(T)[:, None] * N + envs[None, :]).reshape(-1)
    else:
        masks = (torch.rand(T * n, generator=g) >= 0.25).float()
        idx = None
    d = {"T": T, "n": n, "H": H, "masks": masks, "idx": idx,
         "h0": 0.5 * torch.randn(n, H, generator=g),
         "whh": torch.randn(3 * H, H, generator=g) / H ** 0.5,
         "bhh": 0.1 * torch.randn(3 * H, generator=g),
         "gi": torch.randn(T * n, 3 * H, generator=g),
         "dout": torch.randn(T * n, H, generator=g)}
    m = mask_plane(masks, T, n, idx)
    d["m"] = m
    args = (d["h0"], d["whh"], d["bhh"], d["gi"], m)
    d["fwd64"] = gru_seq_forward(*args)
    d["fwd32"] = gru_seq_forward(*args, dtype=torch.float32)
    d["saves"] = {k: d["fwd64"][k].float() for k in ("r", "z", "n", "ghn", "hin")}
    d["bwd64"] = gru_seq_backward(d["dout"], d["saves"], d["whh"], m)
    d["bwd32"] = gru_seq_backward(d["dout"], d["saves"], d["whh"], m, dtype=torch.float32)
    return d


def seq_tol(ref64, yard32, floor=FLOOR):
    """the bound of one tensor: max(floor · max(max|ref|, 1), 2 x the fp32 CPU
    yardstick's own max error against float64 on the same inputs) -> (tol, yardstick)"""
    ref64 = torch.as_tensor(ref64).double()
    yard = (torch.as_tensor(yard32).double() - ref64).abs().max().item()
    return max(floor * max(ref64.abs().max().item(), 1.0), 2.0 * yard), yard


def check_close(name, got, ref64, yard32, n=None, tag=""):
    """got (fp32, CPU) finite and within seq_tol of ref64; prints the measured error
    and, where it fails, the error per (step, 32-row group) so a wrong row offset or a
    misplaced mask can be located.  n: rows per step (None: the tensor is one step)."""
    got = torch.as_tensor(got).double()
    ref64 = torch.as_tensor(ref64).double()
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    tol, yard = seq_tol(ref64, yard32)
    finite = bool(torch.isfinite(got).all())
    err = (got - ref64).abs()
    e = err.max().item() if finite else float("nan")
    print(f"{tag} {name}: max|err| {e:.3e}  fp32 yardstick {yard:.3e}  bound {tol:.3e}  max|ref| "
          f"{ref64.abs().max().item():.3f}", flush=True)
    if not finite or e > tol:
        rows = n if n is not None else got.shape[0]
        per = torch.nan_to_num(err, nan=float("inf")).reshape(-1, rows, got.shape[1]).amax(2)   # [steps][rows]
        G = (rows + 31) // 32
        table = [[per[t, 32 * x:32 * x + 32].max().item() for x in range(G)] for t in range(per.shape[0])]
        for t, line in enumerate(table):
            print(f"  step {t}: " + " ".join(f"g{x}={v:.2e}" for x, v in enumerate(line)), flush=True)
    assert finite, (tag, name, "non-finite output rows", int((~torch.isfinite(got)).any(1).sum()))
    assert e <= tol, (tag, name, e, tol, yard)
    return e


def check_guard(name, buf, rows):
    """buf [rows + GUARD][...] was NaN before the launch: the rows behind `rows`
    still are (nothing stored past the last row)"""
    tail = torch.as_tensor(buf)[rows:]
    assert tail.shape[0] == GUARD, (name, tail.shape)
    bad = ~torch.isnan(tail)
    assert not bad.any(), (name, "stored past row", rows, "guard rows hit", bad.any(-1).nonzero().reshape(-1).tolist()[:8])
