"""float64 references, seeded case generators and the comparisons of the direct conv1
kernel tests (tests/test_conv1_cpu.py, tests/test_conv1_gpu.py); the structure and the
vocabulary are conv_ref.py's, whose compare(), bit packers, U, S_LIMIT and resolve_b are
used as they are.

Layouts are the kernels' (include/ppo_hip.h): observation rows [C][84][84] (u8 or fp32),
raw RGB frames [84][84][3] u8, the output and dz NHWC [B][20][20][32], weights in the torch
layout [32][C][8][8], mask bits u32 [B][400], split-K slabs [Z][32][C * 64] + bias partials
[Z][32].  Image b of a launch is storage row idx[b], or row0 + b where idx is None.

src   what the rows are              decoded input x the convolution sees
u8    bytes u                        u / 255 (the kernels sum w u and scale once)
f32   fp32 values                    themselves
rgb   frames, mode raw               u8 colours + the transposed grey plane truncated to u8
rgb   frames, mode norm / div255     (u - mean) / std, and the transposed grey of that:
                                     `dec` the reference chain (oracle.obs_oracle.
                                     preprocess_batch: every element rounded to fp32), `aff`
                                     the same chain in float64 without those roundings

Integer cases (conv_ref's reasoning: S <= 2^22 asserted, every partial sum exact):
  narrow   weights, dz and fp32 observations at most 8 significant bits, pixels the whole
           range 0 .. 255; dz of the weight gradients is thinned (most entries zero) so that
           B * 400 terms stay below the limit
  wide_x   the streamed fp32 operand 22 bits wide at disjoint sites (fp32 observations of
           the forward, dz of the weight gradients), the other {-1, 0, 1} ({0, 1}: pixels)
  wide_w   the roles swapped (weights of the forward, fp32 observations of the gradient)
The u8 epilogue is relu(A * fl32(1/255) + b) with A the exact integer sum: u8_forms().

S_e of the real cases (|got - ref| <= k 2^-24 S_e): the magnitude of the terms added,
  u8, f32            Σ|w||x| + |b|, x = u / 255 or the fp32 value
  rgb fused decode   the same on the fp32-decoded input (`dec`)
  rgb affine fold    the uncancelled Σ|Weff| (u + |mean|) / |std| + |b|, the grey weights
                     folded as rgbaff_prep_kernel folds them: |w| over the planes
                     P_c = (u_c + |mean_c|) / |std| and the transposed Σ_c k_c P_c
  weight gradients   Σ|dz||x| over the same x (P for the affine fold), Σ|dz| for the bias
"""
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

from oracle import obs_oracle as OO

from helpers.conv_ref import (S_LIMIT, U, _ints, _lattice_sites, _one_per, _wide, compare, drop_lo,  # noqa: F401
                              pack_u32, resolve_b, unpack_u32)

R255 = float(np.float32(1.0) / np.float32(255.0))   # fl32(1/255) as the kernels write it
KG = tuple(float(np.float32(v)) for v in (0.299, 0.587, 0.114))
STD_NORM = 36.31282043457031
SRCS = ("u8", "f32", "rgb")
KINDS = ("narrow", "wide_x", "wide_w", "real")

# k of the real-valued bound, per operation: 4 x the worst ratio torch CPU fp32 (F.conv2d /
# conv2d_weight on fl32(u / 255), on the fp32 rows or on the fp32-decoded frames) reaches over
# real_cases(256), rounded up to a whole number, not below 8.  Measured worst yardstick
# ratios: fwd 6.34 (rgb norm against the float64 chain, B = 515), wgrad 4.97 (f32 C = 12,
# B = 7); test_conv1_cpu.py::test_k_comes_from_the_yardstick recomputes them.
K = {"fwd": 26.0, "wgrad": 20.0}


def mean_plane(seed=0):
    """a NormalizeWrapper mean file's shape and range, fp32-representable [84][84][3]"""
    return np.random.default_rng(seed).uniform(20, 80, (84, 84, 3)).astype(np.float32).astype(np.float64)


def mode_args(mode):
    """(mean float64 [84][84][3] or None, std) the entry points take for a decode mode"""
    return {"norm": (mean_plane(), STD_NORM), "div255": (None, 255.0), "raw": (None, 1.0)}[mode]


# ------------------------------------------------------------------ operations
def fwd(x, w, bias):
    """pre-activation z [B][20][20][32] of conv(x [B][C][84][84], w [32][C][8][8]) + bias"""
    return F.conv2d(x, w, bias, stride=4).permute(0, 2, 3, 1).contiguous()


def wgrad(dz, x):
    """(dW [32][C][8][8], db [32]) of dz [B][20][20][32] over x [B][C][84][84]"""
    dy = dz.permute(0, 3, 1, 2)
    return torch.nn.grad.conv2d_weight(x, (32, x.shape[1], 8, 8), dy, stride=4), dz.sum((0, 1, 2))


def rows_of(B, idx=None, row0=0):
    """the storage rows a launch of B images reads"""
    return torch.arange(row0, row0 + B) if idx is None else torch.as_tensor(idx)[:B]


def decode(frames, mode):
    """the reference chain: [N][84][84][3] u8 -> [N][4][84][84], every element fp32"""
    mean, std = mode_args(mode)
    f = frames.numpy()
    if mode == "norm":
        return torch.from_numpy(OO.preprocess_batch(f, mean=mean, std=std)).double()
    return torch.from_numpy(OO.preprocess_batch(f, div255=(mode == "div255"))).double()


def _planes(col):
    """colour planes [N][84][84][3] float64 -> [N][4][84][84] with the transposed grey"""
    grey = (col[..., 0] * KG[0] + col[..., 1] * KG[1]) + col[..., 2] * KG[2]
    return torch.cat([col.permute(0, 3, 1, 2), grey.transpose(1, 2).unsqueeze(1)], 1).contiguous()


def decode64(frames, mode):
    """the same chain in float64 without the per-element fp32 roundings (raw mode: the
    chain itself, whose integers no rounding touches)"""
    if mode == "raw":
        return decode(frames, mode)
    mean, std = mode_args(mode)
    f = frames.double()
    return _planes((f - torch.from_numpy(mean)) / std if mean is not None else f / std)


def uncancelled(frames, mode):
    """the affine fold's magnitudes: (u + |mean|) / |std| and their transposed grey"""
    mean, std = mode_args(mode)
    m = torch.from_numpy(mean).abs() if mean is not None else 0.0
    return _planes((frames.double() + m) / abs(std))


# ------------------------------------------------------------------ the u8 epilogue
def u8_forms(A, bias):
    """the two fp32 values relu(A * fl32(1/255) + b) can take for an exact integer sum A
    [..][32] (float64) and an integer bias [32]: the contracted fl32(A r + b) and the
    separate fl32(fl32(A r) + b).  A r is a product of two 24-bit values and the sums stay
    below 53 bits, so float64 forms both exactly and .float() rounds once."""
    p = A * R255
    fused = (p + bias).float()
    separate = (p.float().double() + bias).float()
    return torch.relu(fused), torch.relu(separate)


def compare_u8(got, A, bias, bits=None, what=""):
    """every element of got equals one of u8_forms() bit for bit; the mask bits are
    (got > 0).  With a zero bias both forms are fl32(A r): plain equality."""
    f0, f1 = (f.to(got.device) for f in u8_forms(A, bias.double()))
    assert got.shape == f0.shape, f"{what}: shape {tuple(got.shape)}"
    bad = ~((got == f0) | (got == f1))
    if bad.any():
        first = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements are neither fl32(A r + b) nor "
                             f"fl32(fl32(A r) + b), first at {first}: got {got[tuple(first)].item()!r}, want "
                             f"{f0[tuple(first)].item()!r} or {f1[tuple(first)].item()!r}")
    if bits is not None:
        want = pack_u32(got > 0)
        if not torch.equal(bits, want):
            raise AssertionError(f"{what}: {int((bits != want).sum())} mask words differ from (out > 0)")


def reduced(total, scale, pre=None):
    """ppo_wgrad_reduce of exact integer slab sums: fl32(Σ * fl32(scale)) (+ pre)"""
    v = total * float(np.float32(scale))
    return (v if pre is None else v + pre).float()


# ------------------------------------------------------------------ generators
def _thin_dz(g, B, wide_sites=None):
    """dz [B][20][20][32] with about 400 non-zero entries per channel: 15 in 16 of them in
    1 .. 15, the others odd in 129 .. 255 (8 significant bits), random sign"""
    shape = (B, 20, 20, 32)
    on = torch.rand(shape, generator=g) < 1.0 / B
    small = _ints(g, shape, 1, 15)
    big = _ints(g, shape, 64, 127) * 2 + 1
    mag = torch.where(torch.rand(shape, generator=g) < 1.0 / 16, big, small)
    sign = _ints(g, shape, 0, 1) * 2 - 1
    return torch.where(on, mag * sign, torch.zeros(()))


def _nchw_sites(sites):
    b, y, x, c = sites
    return b, c, y, x


@functools.lru_cache(maxsize=None)
def make_case(op, src, kind, C, B, mode=None, seed=0):
    """a seeded case on the CPU with its float64 references:
      rows   the B storage rows (u8 / fp32 [B][C][84][84], rgb frames u8 [B][84][84][3])
      x      the decoded float64 input [B][C][84][84] (rgb real: x the fp32 chain `dec`,
             x_aff the float64 chain, P the affine fold's magnitudes)
      fwd    w, bias -> z, ref = relu(z), S; u8 integer cases also A = Σ w u (no bias)
             rgb real: z / ref / S against `dec`, z_aff / ref_aff / S_aff against the truth
      wgrad  dz -> ref_w, ref_b, S_w, S_b in the decoded scale (u8 integer cases: of the
             bytes, the slab's scale; multiply by the reduce's 1/255)
    Integer kinds assert max S <= 2^22 and their operand widths."""
    assert op in ("fwd", "wgrad") and src in SRCS and kind in KINDS
    assert src != "rgb" or (C == 4 and mode in ("raw", "norm", "div255"))
    assert (src == "rgb") == (mode is not None)
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * SRCS.index(src) + 101 * (op == "wgrad") + 13 * B
                                      + 1009 * C + KINDS.index(kind) + 17 * len(mode or ""))
    c = types.SimpleNamespace(op=op, src=src, kind=kind, C=C, B=B, mode=mode, exact=kind != "real")
    assert c.exact == (mode in (None, "raw")) or src != "rgb", "norm / div255 have no integer form"
    bytes_ = src != "f32"
    x_shape, w_shape, red = (B, C, 84, 84), (32, C, 8, 8), C * 64
    rgb_shape = (B, 84, 84, 3)
    tern = lambda shape: _ints(g, shape, -1, 1)  # noqa: E731
    # ---- the observation rows
    wide_obs = (op, kind) in (("fwd", "wide_x"), ("wgrad", "wide_w"))
    assert not (wide_obs and bytes_), "bytes cannot be wide"
    unit_obs = c.exact and kind != "narrow" and not wide_obs
    if bytes_:
        hi = 1 if unit_obs else 255
        c.rows = torch.randint(0, hi + 1, rgb_shape if src == "rgb" else x_shape, generator=g).to(torch.uint8)
        if src == "rgb" and kind == "real" and B >= 2:
            c.rows[0], c.rows[1] = 0, 255
    elif kind == "real":
        c.rows = torch.randn(x_shape, generator=g)
    elif wide_obs and op == "fwd":
        c.rows = _wide(g, x_shape, 2 ** 20 // red, False, _nchw_sites(_lattice_sites(g, B, 84, 8, C)))
    elif wide_obs:    # one 22-bit element per input channel in the whole batch
        sites = _one_per(g, C, B) + (torch.arange(C),) + _one_per(g, C, 84, 84)
        c.rows = _wide(g, x_shape, max(2 ** 20 // (B * 400), 1), False, sites)
    else:
        c.rows = tern(x_shape) if unit_obs else _ints(g, x_shape, -127, 127)
    if src == "rgb":
        c.x = decode(c.rows, mode)
        if kind == "real":
            c.x_aff, c.P = decode64(c.rows, mode), uncancelled(c.rows, mode)
    else:
        c.x = c.rows.double()
    scale = 1.0 / 255.0 if src == "u8" and not c.exact else 1.0   # integer u8 cases stay in bytes
    xs = c.x * scale
    if op == "fwd":
        if kind == "narrow":
            c.w, c.bias = _ints(g, w_shape, -64, 64), _ints(g, (32,), -20, 20)
        elif kind == "wide_w":
            c.w = _wide(g, w_shape, 2 ** 20 // red, False, (torch.arange(32),) + _one_per(g, 32, C, 8, 8))
            c.bias = _ints(g, (32,), -20, 20)
        elif kind == "wide_x":
            c.w, c.bias = tern(w_shape), _ints(g, (32,), -20, 20)
        else:
            c.w, c.bias = torch.randn(w_shape, generator=g) * 0.05, torch.randn(32, generator=g) * 0.1
        w64, b64 = c.w.double(), c.bias.double()
        if src == "u8" and c.exact:
            c.A = fwd(xs, w64, None)
            c.z = c.A * R255 + b64      # exact in float64: only its sign and the forms are used
            c.ref = None
        else:
            c.z = fwd(xs, w64, b64)
            c.ref = torch.relu(c.z)
        c.S = fwd(xs.abs(), w64.abs(), b64.abs())
        s_max = c.S.max().item()
        if src == "rgb" and kind == "real":
            c.z_aff = fwd(c.x_aff, w64, b64)
            c.ref_aff = torch.relu(c.z_aff)
            c.S_aff = fwd(c.P, w64.abs(), b64.abs())
    else:
        if kind == "narrow":
            c.dz = _thin_dz(g, B)
        elif kind == "wide_x":   # one 22-bit dz per output channel in the whole batch
            sites = _one_per(g, 32, B, 20, 20) + (torch.arange(32),)
            c.dz = _wide(g, (B, 20, 20, 32), max(2 ** 20 // (B * 400), 1), False, sites)
        elif kind == "wide_w":
            c.dz = tern((B, 20, 20, 32))
        else:
            c.dz = torch.randn((B, 20, 20, 32), generator=g)
        set_wgrad_refs(c, c, rows_of(B))
        s_max = max(c.S_w.max().item(), c.S_b.max().item())
    c.s_max = s_max
    if c.exact:
        assert s_max <= S_LIMIT, f"{case_id(c)}: max S = {s_max} exceeds 2^22"
        for name in ("w", "bias", "dz"):
            t = getattr(c, name, None)
            assert t is None or torch.equal(t, t.round()), name
        assert torch.equal(c.x, c.x.round()), "decoded input"
        wide = {"fwd": ("rows", "w"), "wgrad": ("dz", "rows")}[op]
        for i, name in enumerate(wide):
            t = getattr(c, name).float()
            if kind == ("wide_x", "wide_w")[i]:
                assert t.abs().max() >= 2 ** 21 and not torch.equal(t, drop_lo(t)), name
            else:
                assert torch.equal(t, t.bfloat16().float()), name
        if bytes_ and kind == "narrow":
            assert len(torch.unique(c.rows)) == 256, "pixels must use the whole byte range"
    return c


def set_wgrad_refs(out, c, rows):
    """the weight-gradient references of case c with image b = storage row rows[b], set on
    `out`: ref_w, ref_b, S_w, S_b (and the _aff forms of real rgb cases)"""
    rows = torch.as_tensor(rows)
    scale = 1.0 / 255.0 if c.src == "u8" and not c.exact else 1.0
    xs, dz = c.x.index_select(0, rows) * scale, c.dz.double()
    out.ref_w, out.ref_b = wgrad(dz, xs)
    out.S_w, out.S_b = wgrad(dz.abs(), xs.abs())
    if c.src == "rgb" and c.kind == "real":
        out.ref_w_aff, _ = wgrad(dz, c.x_aff.index_select(0, rows))
        out.S_w_aff, _ = wgrad(dz.abs(), c.P.index_select(0, rows))
    if c.exact:
        assert max(out.S_w.max().item(), out.S_b.max().item()) <= S_LIMIT
    return out


@functools.lru_cache(maxsize=None)
def wgrad_refs(op, src, kind, C, B, mode, rows):
    """set_wgrad_refs of make_case(...) for a tuple of storage rows, cached"""
    return set_wgrad_refs(types.SimpleNamespace(), make_case(op, src, kind, C, B, mode), torch.tensor(rows))


def case_id(c):
    return f"conv1-{c.op}-{c.src}{'-' + c.mode if c.mode else ''}-C{c.C}-{c.kind}-B{c.B}"


def yardstick(c, **replace):
    """torch CPU fp32 of the case's operation: F.conv2d / conv2d_weight on fl32(u / 255), on
    the fp32 rows or on the fp32-decoded frames (or on `replace`d tensors: x, w, bias, dz).
    fwd -> (relu(z), z); wgrad -> (dW, db)."""
    x = replace.get("x", c.x.float() / 255.0 if c.src == "u8" else c.x.float())
    if c.op == "fwd":
        z = fwd(x, replace.get("w", c.w), replace.get("bias", c.bias))
        return torch.relu(z), z
    return wgrad(replace.get("dz", c.dz), x)


def ratio(got, ref, S):
    """worst |got - ref| / (2^-24 S)"""
    return ((got.double() - ref).abs() / (U * S)).max().item()


def yardstick_ratio(c):
    """the worst ratio the yardstick reaches on a real case, over every reference the
    kernels of that case are held to"""
    if c.op == "fwd":
        out, _ = yardstick(c)
        r = ratio(out, c.ref, c.S)
        return max(r, ratio(out, c.ref_aff, c.S_aff)) if c.src == "rgb" else r
    gw, gb = yardstick(c)
    r = max(ratio(gw, c.ref_w, c.S_w), ratio(gb, c.ref_b, c.S_b))
    return max(r, ratio(gw, c.ref_w_aff, c.S_w_aff)) if c.src == "rgb" else r


# ------------------------------------------------------------------ the assertions
def check_fwd(c, out, bits=None, *, aff=False, rows=None, bias=None, what=""):
    """The forward assertion of case c on a kernel's output `out` [n][20][20][32] (and its
    mask words), image b being the case's row rows[b] (None: row b).  u8 integer cases:
    compare_u8 with `bias` (None: the case's; the zero bias makes it plain equality).
    Other integer cases: conv_ref.compare, exact.  Real cases: within K["fwd"] 2^-24 S_e of
    the reference (aff: the float64 chain and the uncancelled S_e), decided mask bits equal
    (z > 0).  The bits equal (out > 0) everywhere.  Returns the worst ratio."""
    sel = (lambda t: t) if rows is None else (lambda t: t.index_select(0, torch.as_tensor(rows)))
    what = what or case_id(c)
    if c.src == "u8" and c.exact:
        compare_u8(out, sel(c.A), c.bias if bias is None else bias, bits, what)
        return 0.0
    assert bias is None
    ref, S, z = (c.ref_aff, c.S_aff, c.z_aff) if aff else (c.ref, c.S, c.z)
    worst = compare(out, sel(ref), exact=c.exact, S=sel(S), k=K["fwd"], bits=bits, layout="u32", z=sel(z), what=what)
    if bits is not None:
        assert torch.equal(bits, pack_u32(out > 0)), f"{what}: mask words differ from (out > 0)"
    return worst


def check_wgrad(c, refs, gw, gb, *, aff=False, scale=1.0, pre=None, what=""):
    """The weight-gradient assertion on ppo_wgrad_reduce's results gw [32][C][8][8] and gb
    [32] against refs (set_wgrad_refs).  Integer cases: gw == fl32(Σ scale (+ pre_w)), gb ==
    Σ (+ pre_b) bit for bit.  Real cases (u8: scale 1/255 given to the reduce, the references
    are in the decoded scale): within K["wgrad"] 2^-24 S_e.  Returns the worst ratio."""
    what = what or case_id(c)
    if c.exact:
        pw, pb = (None, None) if pre is None else pre
        compare(gw, reduced(refs.ref_w, scale, pw).double(), exact=True, what=what + " dW")
        compare(gb, reduced(refs.ref_b, 1.0, pb).double(), exact=True, what=what + " db")
        return 0.0
    ref_w, S_w = (refs.ref_w_aff, refs.S_w_aff) if aff else (refs.ref_w, refs.S_w)
    return max(compare(gw, ref_w, exact=False, S=S_w, k=K["wgrad"], what=what + " dW"),
               compare(gb, refs.ref_b, exact=False, S=refs.S_b, k=K["wgrad"], what=what + " db"))


def check_slabs(c, refs, slab, slab_b, B, *, walks_images, what=""):
    """every slab and bias-partial entry written (the prefill is NaN); the slabs of blocks
    that walk images b = z, z + Z, ... and hold none (z >= B) exactly zero; on integer cases
    the float64 sum of the slabs equals the reference exactly"""
    what = what or case_id(c)
    for s in (slab, slab_b):
        assert not torch.isnan(s).any(), f"{what}: slab entries left unwritten"
        if walks_images:
            assert (s[B:] == 0).all(), f"{what}: an idle block's slab is not zero"
    if c.exact:
        compare(slab.double().sum(0).view(refs.ref_w.shape), refs.ref_w, exact=True, what=what + " slab sum")
        compare(slab_b.double().sum(0), refs.ref_b, exact=True, what=what + " bias partial sum")


# ------------------------------------------------------------------ the GPU test matrix
FWD_B = (1, 2, 5, 16, 17, 33, "C+3", "2C+3")     # image-resident paths and the trunk
TILE_B = (1, 2, 5, 33, "C+3")                    # tile GEMM: 400 rows per image, 256-row tiles
WIDE_B = (5, 17, "2C+3")
REAL_B = (1, 17, "2C+3")
OTHER_C = (1, 3, 12)
SMALL_C = (1, 2, 3, 4, 5, 8, 12)
WGRAD_BZ = ((1, 1), (1, 4), (2, 1), (3, 1), (3, 2), (4, 1), (5, 1), (5, 2), (7, 2), (7, 3), (9, 2), (33, 5),
            (64, 64), (300, "engine"))
WGRAD_SUB_BZ = ((7, 2), (9, 2), (300, "engine"))
DEEP_B, DEEP_BASE = 8200, 37
ADDR_B = 17


OTHER_B = (5, 33)
SMALL_B = (1, 4, 5)

# forward path -> (src, decode mode, ((kind, batch sizes), ...)); C = 4
FWD_PATHS = {
    "u8_img": ("u8", None, (("narrow", FWD_B), ("wide_w", WIDE_B), ("real", REAL_B))),
    "u8_tile": ("u8", None, (("narrow", TILE_B), ("wide_w", (5, "C+3")), ("real", (1, "C+3")))),
    "f32_img": ("f32", None, (("narrow", FWD_B), ("wide_x", WIDE_B), ("wide_w", WIDE_B), ("real", REAL_B))),
    "rgb_raw": ("rgb", "raw", (("narrow", FWD_B), ("wide_w", WIDE_B))),
    "rgb_norm": ("rgb", "norm", (("real", REAL_B),)),
    "rgb_div255": ("rgb", "div255", (("real", REAL_B),)),
    "trunk": ("u8", None, (("narrow", FWD_B),)),
}
# weight-gradient path -> (src, decode mode, C, kinds on WGRAD_SUB_BZ besides narrow everywhere)
WGRAD_PATHS = {
    "u8_kw9": ("u8", None, 4, ("wide_x", "real")),
    "u8_kw10": ("u8", None, 4, ("wide_x", "real")),
    "u8_kw8": ("u8", None, 4, ("wide_x", "real")),
    "u8_kw5": ("u8", None, 4, ("wide_x", "real")),
    "u8_half": ("u8", None, 4, ()),                       # products 1: narrow only
    "f32": ("f32", None, 4, ("wide_x", "wide_w", "real")),
    "f32_routed": ("f32", None, 4, ("wide_x", "wide_w", "real")),
    "rgb_raw": ("rgb", "raw", 4, ("wide_x",)),
    "rgb_norm": ("rgb", "norm", 4, ("real",)),            # no integer form: real only
    "rgb_div255": ("rgb", "div255", 4, ("real",)),
}
for _src in ("u8", "f32"):
    for _C in OTHER_C:
        WGRAD_PATHS[f"{_src}_C{_C}"] = (_src, None, _C, ("wide_x", "real") + (("wide_w",) if _src == "f32" else ()))


def fwd_params():
    return [(p, kind, B) for p, (_, _, kinds) in FWD_PATHS.items() for kind, Bs in kinds for B in Bs]


def wgrad_params():
    out = []
    for p, (src, mode, C, _) in WGRAD_PATHS.items():
        narrow = mode in (None, "raw")
        out += [(p, B, Z) for B, Z in (WGRAD_BZ if narrow else WGRAD_SUB_BZ)]
        if C != 4:
            out.append((p, 1, 16))     # the tile GEMM: more slices than k-tiles
    return out


def wgrad_kinds(path, B, Z):
    _, mode, _, extra = WGRAD_PATHS[path]
    sub = (B, Z) in WGRAD_SUB_BZ
    return (("narrow",) if mode in (None, "raw") else ()) + (extra if sub else ())


def matrix(n_cu):
    """the make_case arguments of every case tests/test_conv1_gpu.py runs on a device of
    n_cu compute units"""
    out = []
    for p, kind, B in fwd_params():
        src, mode, _ = FWD_PATHS[p]
        out.append(("fwd", src, kind, 4, resolve_b(B, n_cu), mode))
    for src in ("u8", "f32"):
        out += [("fwd", src, kind, C, B, None) for C in OTHER_C for B in OTHER_B for kind in ("narrow", "real")]
        out += [("fwd", src, kind, C, B, None) for C in SMALL_C for B in SMALL_B for kind in ("narrow", "real")]
    for src, mode, kind in (("u8", None, "narrow"), ("f32", None, "narrow"), ("rgb", "norm", "real")):
        out.append(("fwd", src, kind, 4, DEEP_BASE, mode))
    for src, mode, kind in (("u8", None, "narrow"), ("f32", None, "narrow"), ("rgb", "raw", "narrow"),
                            ("rgb", "norm", "real")):
        out += [(op, src, kind, 4, ADDR_B, mode) for op in ("fwd", "wgrad")]
    out += [(op, src, "narrow", C, ADDR_B, None) for op in ("fwd", "wgrad") for src in ("u8", "f32") for C in (3,)]
    for p, B, Z in wgrad_params():
        src, mode, C, _ = WGRAD_PATHS[p]
        out += [("wgrad", src, kind, C, B, mode) for kind in wgrad_kinds(p, B, Z)]
    out += [("wgrad", src, "narrow", 4, B, mode) for src, mode in (("u8", None), ("f32", None), ("rgb", "raw"))
            for B in (512, 5)]
    return sorted(set(out), key=str)


def real_cases(n_cu):
    """the real cases of matrix(n_cu): K is taken over these"""
    return [a for a in matrix(n_cu) if a[2] == "real"]
