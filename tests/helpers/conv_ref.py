"""float64 references, seeded case generators and the one comparison of the direct
conv2 / conv3 kernel tests (tests/test_conv_cpu.py, tests/test_conv_gpu.py).

Layouts are the kernels' (include/ppo_hip.h): activations and gradients NHWC, weights
in the torch layout [co][ci][ky][kx] (ppo_pack_weights reorders them), mask bits u32
[B][400], u64 [B][81] and u16 [B][49][2].  Every reference is torch.nn.functional in
the dtype of its arguments: float64 arguments give the reference, float32 arguments the
yardstick (torch CPU fp32 of the same operation), absolute values the per-element
magnitude S = Σ|x||w| (+ |bias|) that the bound of the real-valued cases scales with.

Integer cases: the split-bf16 kernels sum exact part products in fp32, so on small
integer inputs every partial sum is an exactly representable integer as long as
S <= 2^24; the generators assert S <= 2^22 (a factor 4 of room for the |hi| + |mid| +
|lo| >= |x| of a round-to-nearest split).  The kernel must then equal float64 bit for
bit in any summation order.
  narrow   every tensor at most 8 significant bits: the hi plane alone (products 1, 6, 9)
  wide_x   the streamed operand (activations of the forward, dz of the gradients) holds
           integers of up to 22 significant bits (hi, mid and lo planes), the other
           operand {-1, 0, 1} (products 6, 9)
  wide_w   the roles swapped: wide weights (forward, dgrad) or wide activations (wgrad)
  real     relu(randn) activations, randn dz, randn masks, weights 0.05 randn, biases
           0.1 randn (the scales of test_gpu_parity.py's _packed)
"""
import functools
import types

import torch
import torch.nn.functional as F

LAYERS = {
    2: dict(cin=32, cout=64, ks=4, st=2, hi=20, ho=9),
    3: dict(cin=64, cout=32, ks=3, st=1, hi=9, ho=7),
}
OPS = ("fwd", "dgrad", "wgrad")
S_LIMIT = float(2 ** 22)
U = 2.0 ** -24   # fp32 unit roundoff

# k of the real-valued bound |got - ref| <= k 2^-24 S_e, per operation: 4 x the worst
# ratio torch CPU fp32 reaches over all real cases of the operation (matrix(256): B = 1,
# 17, 515 forward and dgrad; B = 7, 40, 300 weight gradient), rounded up to a whole
# number, not below 8.  Measured worst yardstick ratios: fwd 4.93 (conv2, B = 515),
# dgrad 5.54 (conv3, B = 515), wgrad 4.57 (conv2, B = 7);
# test_conv_cpu.py::test_k_comes_from_the_yardstick recomputes them.
K = {"fwd": 20.0, "dgrad": 23.0, "wgrad": 19.0}


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------ operations
def fwd(layer, a, w, bias):
    """pre-activation z [B][ho][ho][co] of conv(a [B][hi][hi][ci], w) + bias"""
    L = LAYERS[layer]
    return _nhwc(F.conv2d(_nchw(a), w, bias, stride=L["st"]))


def dgrad(layer, dz, w, mask):
    """[mask > 0] conv_transpose(dz, w): the input gradient behind the ReLU of the
    layer below, whose saved output is `mask` (any real tensor of the input's shape)"""
    L = LAYERS[layer]
    g = _nhwc(F.conv_transpose2d(_nchw(dz), w, stride=L["st"]))
    return torch.where(mask > 0, g, torch.zeros((), dtype=g.dtype))


def wgrad(layer, dz, a):
    """(dW [co][ci][ky][kx], db [co]): the convolution of the input with dz as a dilated
    kernel, images in the channel role"""
    L = LAYERS[layer]
    x = _nchw(a).transpose(0, 1)      # [ci][B][hi][hi]
    k = _nchw(dz).transpose(0, 1)     # [co][B][ho][ho]
    gw = F.conv2d(x, k, dilation=L["st"])[:, :, :L["ks"], :L["ks"]]   # [ci][co][ky][kx]
    return gw.transpose(0, 1).contiguous(), dz.sum((0, 1, 2))


# ------------------------------------------------------------------ mask bits
def _pack(live, width, dtype):
    """live [..., n * width] bool -> [..., n] words of `dtype`, bit j of word t = element
    width t + j (two's complement: the top bit makes the word negative)"""
    v = live.reshape(*live.shape[:-1], -1, width).to(torch.int64)
    wts = torch.ones(width, dtype=torch.int64) << torch.arange(width, dtype=torch.int64)
    if width == 64:
        wts[63] = torch.iinfo(torch.int64).min
    word = (v * wts.to(v.device)).sum(-1)
    if width < 64:
        word = torch.where(word >= (1 << (width - 1)), word - (1 << width), word)
    return word.to(dtype)


def _unpack(words, width):
    sh = torch.arange(width, dtype=torch.int64, device=words.device)
    return ((words.to(torch.int64).unsqueeze(-1) >> sh) & 1).bool().reshape(*words.shape[:-1], -1)


def pack_u32(live):
    """[B][20][20][32] bool -> int32 [B][400] (ppo_conv1_fwd_mask / ppo_conv2_dgrad_bits)"""
    return _pack(live.reshape(live.shape[0], 400, 32), 32, torch.int32).reshape(-1, 400)


def pack_u64(live):
    """[B][9][9][64] bool -> int64 [B][81] (ppo_conv2_fwd_mask / ppo_conv3_dgrad_bits)"""
    return _pack(live.reshape(live.shape[0], 81, 64), 64, torch.int64).reshape(-1, 81)


def pack_u16(live):
    """[B][7][7][32] bool -> int16 [B][49][2] (ppo_conv3_fwd_mask)"""
    return _pack(live.reshape(live.shape[0], 49, 32), 16, torch.int16)


def unpack_u32(words):
    return _unpack(words.reshape(-1, 400, 1), 32).reshape(-1, 20, 20, 32)


def unpack_u64(words):
    return _unpack(words.reshape(-1, 81, 1), 64).reshape(-1, 9, 9, 64)


def unpack_u16(words):
    return _unpack(words.reshape(-1, 49, 2), 16).reshape(-1, 7, 7, 32)


PACK = {"u32": pack_u32, "u64": pack_u64, "u16": pack_u16}
UNPACK = {"u32": unpack_u32, "u64": unpack_u64, "u16": unpack_u16}


# ------------------------------------------------------------------ generators
def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _wide(g, shape, background, nonneg, sites):
    """integers of up to 22 significant bits: a background of |v| <= `background` (hi and
    mid planes) and, at `sites` (index tuples no two of which meet in one output's sum),
    odd values in [2^21, 3 * 2^20): 22 significant bits, a non-zero lo plane"""
    t = _ints(g, shape, 0 if nonneg else -background, background)
    big = (torch.randint(2 ** 20, 3 * 2 ** 19, (len(sites[0]),), generator=g) * 2 + 1).float()
    if not nonneg:
        big = big * (torch.randint(0, 2, big.shape, generator=g) * 2 - 1).float()
    t[sites] = big
    return t


def _lattice_sites(g, B, size, step, channels):
    """per image a lattice of pixels `step` apart (random origin), one random channel
    each: two of them never lie in one step x step window"""
    bs, ys, xs, cs = [], [], [], []
    for b in range(B):
        oy, ox = (int(v) for v in torch.randint(0, step, (2,), generator=g))
        for y in range(oy, size, step):
            for x in range(ox, size, step):
                bs.append(b), ys.append(y), xs.append(x)
                cs.append(int(torch.randint(0, channels, (1,), generator=g)))
    return tuple(torch.tensor(v) for v in (bs, ys, xs, cs))


def _one_per(g, n, *dims):
    """for each i < n one random index into dims"""
    return tuple(torch.randint(0, d, (n,), generator=g) for d in dims)


def _narrow_ranges(red):
    """(activation max, dz max) of a narrow weight-gradient case of reduction length red:
    the widest pair of the ladder whose worst case red * amax * dzmax stays <= 2^21"""
    for amax, dmax in ((15, 7), (7, 3), (3, 1), (1, 1)):
        if red * amax * dmax <= 2 ** 21:
            return amax, dmax
    raise AssertionError(f"no narrow integer range for a reduction of {red} terms")


@functools.lru_cache(maxsize=None)
def make_case(layer, op, kind, B, seed=0):
    """a seeded case (tensors float32, on the CPU) with its float64 reference:
      fwd    a, w, bias            -> z (pre-activation), ref = relu(z), S
      dgrad  dz, w, m (the mask)   -> ref, S (0 where masked)
      wgrad  dz, a                 -> ref_w, ref_b, S_w, S_b
    Integer kinds assert max S <= 2^22 and that S bounds a non-trivial result."""
    L = LAYERS[layer]
    ci, co, ks, hi, ho = L["cin"], L["cout"], L["ks"], L["hi"], L["ho"]
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * layer + 101 * OPS.index(op) + 13 * B
                                      + ("narrow", "wide_x", "wide_w", "real").index(kind))
    c = types.SimpleNamespace(layer=layer, op=op, kind=kind, B=B, exact=kind != "real")
    a_shape, dz_shape, w_shape = (B, hi, hi, ci), (B, ho, ho, co), (co, ci, ks, ks)
    tern = lambda shape: _ints(g, shape, -1, 1)  # noqa: E731
    if op == "fwd":
        red = ks * ks * ci
        if kind == "narrow":
            c.a, c.w, c.bias = _ints(g, a_shape, 0, 15), _ints(g, w_shape, -3, 3), _ints(g, (co,), -20, 20)
        elif kind == "wide_x":
            c.a = _wide(g, a_shape, 2 ** 20 // red, True, _lattice_sites(g, B, hi, ks, ci))
            c.w, c.bias = tern(w_shape), _ints(g, (co,), -20, 20)
        elif kind == "wide_w":
            sites = (torch.arange(co),) + _one_per(g, co, ci, ks, ks)
            c.w = _wide(g, w_shape, 2 ** 20 // red, False, sites)
            c.a, c.bias = tern(a_shape), _ints(g, (co,), -20, 20)
        else:
            c.a = torch.relu(torch.randn(a_shape, generator=g))
            c.w, c.bias = torch.randn(w_shape, generator=g) * 0.05, torch.randn(co, generator=g) * 0.1
        c.z = fwd(layer, c.a.double(), c.w.double(), c.bias.double())
        c.ref = torch.relu(c.z)
        c.S = fwd(layer, c.a.double().abs(), c.w.double().abs(), c.bias.double().abs())
        s_max = c.S.max().item()
    elif op == "dgrad":
        red = ks * ks * co   # an upper bound: conv2's stride leaves 2 x 2 of the 4 x 4 taps
        if kind == "narrow":
            c.dz, c.w, c.m = _ints(g, dz_shape, -7, 7), _ints(g, w_shape, -3, 3), _ints(g, a_shape, -3, 3)
        elif kind == "wide_x":
            c.dz = _wide(g, dz_shape, 2 ** 20 // red, False, _lattice_sites(g, B, ho, ks, co))
            c.w, c.m = tern(w_shape), _ints(g, a_shape, -3, 3)
        elif kind == "wide_w":
            sites = _one_per(g, ci, co) + (torch.arange(ci),) + _one_per(g, ci, ks, ks)
            c.w = _wide(g, w_shape, 2 ** 20 // red, False, sites)
            c.dz, c.m = tern(dz_shape), _ints(g, a_shape, -3, 3)
        else:
            c.dz, c.m = torch.randn(dz_shape, generator=g), torch.randn(a_shape, generator=g)
            c.w = torch.randn(w_shape, generator=g) * 0.05
        c.ref = dgrad(layer, c.dz.double(), c.w.double(), c.m)
        c.S = dgrad(layer, c.dz.double().abs(), c.w.double().abs(), c.m)
        s_max = c.S.max().item()
    else:
        red = B * ho * ho
        if kind == "narrow":
            amax, dmax = _narrow_ranges(red)
            c.a, c.dz = _ints(g, a_shape, 0, amax), _ints(g, dz_shape, -dmax, dmax)
        elif kind == "wide_x":    # one 22-bit dz per output channel in the whole batch
            sites = _one_per(g, co, B, ho, ho) + (torch.arange(co),)
            c.dz = _wide(g, dz_shape, max(2 ** 20 // red, 1), False, sites)
            c.a = tern(a_shape)
        elif kind == "wide_w":    # one 22-bit activation per input channel in the whole batch
            sites = _one_per(g, ci, B, hi, hi) + (torch.arange(ci),)
            c.a = _wide(g, a_shape, max(2 ** 20 // red, 1), True, sites)
            c.dz = tern(dz_shape)
        else:
            c.a, c.dz = torch.relu(torch.randn(a_shape, generator=g)), torch.randn(dz_shape, generator=g)
        c.ref_w, c.ref_b = wgrad(layer, c.dz.double(), c.a.double())
        c.S_w, c.S_b = wgrad(layer, c.dz.double().abs(), c.a.double().abs())
        s_max = max(c.S_w.max().item(), c.S_b.max().item())
    c.s_max = s_max
    if c.exact:
        assert s_max <= S_LIMIT, f"{case_id(c)}: max S = {s_max} exceeds 2^22"
        for name in ("a", "w", "bias", "dz", "m"):
            t = getattr(c, name, None)
            assert t is None or torch.equal(t, t.round()), name
        wide = {"fwd": ("a", "w"), "dgrad": ("dz", "w"), "wgrad": ("dz", "a")}[op]
        for i, name in enumerate(wide):
            t = getattr(c, name)
            if kind == ("wide_x", "wide_w")[i]:
                assert t.abs().max() >= 2 ** 21 and not torch.equal(t, drop_lo(t)), name
            else:   # at most 8 significant bits: the hi plane holds it
                assert torch.equal(t, t.bfloat16().float()), name
    return c


def drop_lo(t):
    """t with the lo plane of its three-way bf16 split dropped (hi + mid: 16 bits)"""
    hi = t.bfloat16().float()
    return hi + (t - hi).bfloat16().float()


def case_id(c):
    return f"conv{c.layer}-{c.op}-{c.kind}-B{c.B}"


def yardstick(c, **replace):
    """torch CPU fp32 of the case's operation on its own inputs (or on `replace`d ones:
    the planted errors of test_conv_cpu.py).  fwd -> relu(z) and z; dgrad -> dx;
    wgrad -> (dW, db)."""
    t = {n: replace.get(n, getattr(c, n, None)) for n in ("a", "w", "bias", "dz", "m")}
    if c.op == "fwd":
        z = fwd(c.layer, t["a"], t["w"], t["bias"])
        return torch.relu(z), z
    if c.op == "dgrad":
        return dgrad(c.layer, t["dz"], t["w"], t["m"])
    return wgrad(c.layer, t["dz"], t["a"])


# ------------------------------------------------------------------ the comparison
def compare(got, ref, *, exact, S=None, k=None, bits=None, layout=None, z=None, what=""):
    """The one assertion of the conv tests; returns the worst |got - ref| / (2^-24 S).
    exact (integer cases): torch.equal on the values, and on the packed mask bits
      against (z > 0).  No tolerance.
    real: every element within k 2^-24 S_e of ref; the mask bits equal (z > 0) wherever
      |z| exceeds that element's bound.
    got / bits may live on the GPU; ref, S and z are moved to them."""
    dev = got.device
    ref = ref.to(dev)
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    if exact:
        same = torch.equal(got, ref) if got.dtype == ref.dtype else torch.equal(got.double(), ref)
        if not same:
            bad = (got.double() != ref.double()) | torch.isnan(got)
            first = bad.nonzero()[0].tolist()
            raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from float64, first at "
                                 f"{first}: got {got[tuple(first)].item()!r}, want {ref[tuple(first)].item()!r}")
        if bits is not None:
            want = PACK[layout]((z > 0)).to(dev)
            assert bits.shape == want.shape, f"{what}: bits shape {tuple(bits.shape)}"
            if not torch.equal(bits, want):
                bad = (bits != want).nonzero()
                raise AssertionError(f"{what}: {len(bad)} mask words differ, first at {bad[0].tolist()}")
        return 0.0
    assert k is not None and S is not None
    bound = (k * U) * S.to(dev)
    err = (got.double() - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    over = err > bound
    ratio = torch.where(S.to(dev) > 0, err / (U * S.to(dev)), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                        torch.zeros_like(err)))
    worst = ratio.max().item()
    if over.any():
        first = over.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(over.sum())} elements beyond {k} * 2^-24 * S (worst ratio {worst:.2f}), "
                             f"first at {first}: got {got[tuple(first)].item()!r}, want {ref[tuple(first)].item()!r}")
    if bits is not None:
        z = z.to(dev)
        live = UNPACK[layout](bits)
        decided = z.abs() > bound
        wrong = decided & (live != (z > 0))
        if wrong.any():
            raise AssertionError(f"{what}: {int(wrong.sum())} decided mask bits differ, first at "
                                 f"{wrong.nonzero()[0].tolist()}")
    return worst


# ------------------------------------------------------------------ the GPU test matrix
FWD_B = (1, 2, 5, 16, 17, 33, "C+3", "2C+3")
WIDE_B = (5, 17, "2C+3")
REAL_B = (1, 17, "2C+3")
WGRAD_BZ = ((1, 1), (1, 4), (2, 1), (3, 2), (7, 1), (7, 2), (8, 3), (33, 5), (40, 3), (64, 64), (300, "engine"))
WGRAD_WIDE_BZ = ((7, 2), (40, 3), (1, 4))
WGRAD_REAL_BZ = ((7, 1), (40, 3), (300, "engine"))
DEEP_B, DEEP_BASE = 8200, 37


def resolve_b(B, n_cu):
    return {"C+3": n_cu + 3, "2C+3": 2 * n_cu + 3}.get(B, B)


def matrix(n_cu):
    """every (layer, op, kind, B) case tests/test_conv_gpu.py runs on a device of n_cu
    compute units (the deep walk's base images included)"""
    out = []
    for layer in (2, 3):
        for op in ("fwd", "dgrad"):
            out += [(layer, op, "narrow", resolve_b(B, n_cu)) for B in FWD_B]
            out += [(layer, op, kind, resolve_b(B, n_cu)) for kind in ("wide_x", "wide_w") for B in WIDE_B]
            out += [(layer, op, "real", resolve_b(B, n_cu)) for B in REAL_B]
            out.append((layer, op, "narrow", DEEP_BASE))
        out += [(layer, "wgrad", "narrow", B) for B, _ in WGRAD_BZ]
        out += [(layer, "wgrad", kind, B) for kind in ("wide_x", "wide_w") for B, _ in WGRAD_WIDE_BZ]
        out += [(layer, "wgrad", "real", B) for B, _ in WGRAD_REAL_BZ]
    return sorted(set(out), key=str)
