"""CPU checks of tests/helpers/conv_ref.py: the float64 conv2 / conv3 references equal
torch float64 autograd of relu(conv), the mask-bit packers round-trip, every case
tests/test_conv_gpu.py runs (on a 256-CU device) meets its generator's precondition,
the integer cases are exact in torch fp32 too (a summation order other than
float64's), and the comparison used on the GPU accepts the fp32 yardstick (torch CPU
fp32 of the same operation) on every real case and rejects planted errors — shown by
handing it the yardstick computed from deliberately wrong inputs or ops in the
kernel's place."""
import pytest
import torch
import torch.nn.functional as F

from helpers import conv_ref as R

N_CU = 256   # the MI355X; the GPU test reads the device's own count
MATRIX = R.matrix(N_CU)
MIDS = [f"conv{l}-{op}-{kind}-B{B}" for l, op, kind, B in MATRIX]


def _case_compare(c, got):
    """R.compare of an operation's result `got` (the yardstick's return value, or a
    tampered copy) against case c, as the GPU tests call it"""
    k = R.K[c.op]
    if c.op == "fwd":
        out, bits, layout = got
        return R.compare(out, c.ref, exact=c.exact, S=c.S, k=k, bits=bits, layout=layout, z=c.z, what=R.case_id(c))
    if c.op == "dgrad":
        return R.compare(got, c.ref, exact=c.exact, S=c.S, k=k, what=R.case_id(c))
    r1 = R.compare(got[0], c.ref_w, exact=c.exact, S=c.S_w, k=k, what=R.case_id(c) + " dW")
    r2 = R.compare(got[1], c.ref_b, exact=c.exact, S=c.S_b, k=k, what=R.case_id(c) + " db")
    return max(r1, r2)


def _fwd_got(c, **replace):
    """what a forward kernel with a mask epilogue returns: relu(z) and the packed bits of
    its own output"""
    out, _ = R.yardstick(c, **replace)
    layout = "u64" if c.layer == 2 else "u16"
    return out, R.PACK[layout](out > 0), layout


def _got(c, **replace):
    return _fwd_got(c, **replace) if c.op == "fwd" else R.yardstick(c, **replace)


# ------------------------------------------------------------------ the helper itself
@pytest.mark.parametrize("layer", [2, 3])
def test_float64_helper_equals_autograd(layer):
    """dgrad and wgrad of the helper == float64 autograd of relu(conv(relu(u), w) + b)
    with respect to u, w and b, to 1e-12 relative."""
    L = R.LAYERS[layer]
    g = torch.Generator().manual_seed(layer)
    B = 3
    u = torch.randn(B, L["hi"], L["hi"], L["cin"], generator=g, dtype=torch.float64, requires_grad=True)
    w = (torch.randn(L["cout"], L["cin"], L["ks"], L["ks"], generator=g, dtype=torch.float64) * 0.05).requires_grad_()
    b = (torch.randn(L["cout"], generator=g, dtype=torch.float64) * 0.1).requires_grad_()
    r = torch.randn(B, L["ho"], L["ho"], L["cout"], generator=g, dtype=torch.float64)
    x = torch.relu(u)
    z = F.conv2d(x.permute(0, 3, 1, 2), w, b, stride=L["st"]).permute(0, 2, 3, 1)
    assert torch.equal(z.detach(), R.fwd(layer, x.detach(), w.detach(), b.detach()))
    (torch.relu(z) * r).sum().backward()
    dz = (r * (z > 0)).detach()
    gw, gb = R.wgrad(layer, dz, x.detach())
    for got, ref in ((R.dgrad(layer, dz, w.detach(), x.detach()), u.grad), (gw, w.grad), (gb, b.grad)):
        assert got.shape == ref.shape
        assert (got - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()


@pytest.mark.parametrize("layout,shape", [("u32", (3, 20, 20, 32)), ("u64", (3, 9, 9, 64)), ("u16", (3, 7, 7, 32))])
def test_bit_packers_round_trip(layout, shape):
    g = torch.Generator().manual_seed(5)
    live = torch.rand(shape, generator=g) > 0.5
    live.view(3, -1, shape[-1])[0, 0] = True    # all-ones words: the sign bit of every width
    live.view(3, -1, shape[-1])[1, 1] = False
    words = R.PACK[layout](live)
    assert words.shape == {"u32": (3, 400), "u64": (3, 81), "u16": (3, 49, 2)}[layout]
    assert torch.equal(R.UNPACK[layout](words), live)
    # bit j of word t is channel width * t + j, by hand on one pixel
    width = {"u32": 32, "u64": 64, "u16": 16}[layout]
    px = live.view(3, -1, shape[-1])[2, 5].reshape(-1, width)
    want = [sum(int(bit) << j for j, bit in enumerate(row)) for row in px.tolist()]
    got = words.reshape(3, -1, shape[-1] // width)[2, 5].tolist()
    assert [v & ((1 << width) - 1) for v in got] == want


# ------------------------------------------------------------------ every GPU case
@pytest.mark.parametrize("layer,op,kind,B", MATRIX, ids=MIDS)
def test_case_precondition_and_yardstick(layer, op, kind, B):
    """make_case asserts the generator's precondition (integers, plane use, max S <=
    2^22).  Integer cases: torch fp32 equals float64 exactly.  Real cases: the comparison
    accepts the fp32 yardstick with the operation's k, at a quarter of it (k is 4 x the
    yardstick's worst ratio)."""
    c = R.make_case(layer, op, kind, B)
    assert c.s_max > 0
    worst = _case_compare(c, _got(c))
    if c.exact:
        assert c.s_max <= 2 ** 22
    else:
        print(f"yardstick ratio {R.case_id(c)}: {worst:.3f}")
        assert 4 * worst <= R.K[op]


def test_k_comes_from_the_yardstick():
    """K[op] = 4 x the worst ratio |fp32 - ref| / (2^-24 S) torch CPU fp32 reaches over the
    real cases of the operation, rounded up to a whole number, not below 8."""
    worst = {op: 0.0 for op in R.OPS}
    for layer, op, kind, B in MATRIX:
        if kind == "real":
            c = R.make_case(layer, op, kind, B)
            worst[op] = max(worst[op], _case_compare(c, _got(c)))
    print("worst yardstick ratios", worst)
    for op in R.OPS:
        assert R.K[op] >= 8 and 4 * worst[op] <= R.K[op]
        assert R.K[op] <= max(8, 4 * worst[op] * 1.5), "k is far above 4 x the yardstick: re-derive it"


# ------------------------------------------------------------------ planted errors
def _rejects(c, got):
    with pytest.raises(AssertionError):
        _case_compare(c, got)


WG = [(layer, kind, B) for layer in (2, 3) for kind, B in (("narrow", 7), ("narrow", 40), ("real", 7), ("real", 40))]


@pytest.mark.parametrize("layer,kind,B", WG)
def test_rejects_image_left_out(layer, kind, B):
    c = R.make_case(layer, "wgrad", kind, B)
    for b in (0, B - 1):
        dz = c.dz.clone()
        dz[b] = 0
        _rejects(c, R.yardstick(c, dz=dz))


@pytest.mark.parametrize("layer,kind,B", WG)
def test_rejects_last_image_twice(layer, kind, B):
    """the block's last image, re-read past the end, counted — in both gradients, and in
    the bias gradient only"""
    c = R.make_case(layer, "wgrad", kind, B)
    gw, gb = R.yardstick(c)
    gw2, gb2 = R.yardstick(c, dz=torch.cat([c.dz, c.dz[-1:]]), a=torch.cat([c.a, c.a[-1:]]))
    _rejects(c, (gw2, gb2))
    _rejects(c, (gw, gb2))
    _case_compare(c, (gw, gb))


@pytest.mark.parametrize("layer,kind,B", WG)
def test_rejects_dropped_reduction_pixel(layer, kind, B):
    """the last pixel of the reduction (conv2: 80, the one past the 72 + 8 slot order;
    conv3: 48) dropped"""
    c = R.make_case(layer, "wgrad", kind, B)
    dz = c.dz.clone()
    dz[:, -1, -1] = 0
    _rejects(c, R.yardstick(c, dz=dz))


@pytest.mark.parametrize("layer,kind,B", WG)
def test_rejects_stray_value_in_idle_slab(layer, kind, B):
    """split partials summed as ppo_wgrad_reduce sums them, an idle block's slab holding
    one stray value instead of zeros"""
    c = R.make_case(layer, "wgrad", kind, B)
    gw, gb = R.yardstick(c)
    for which in (0, 1):
        slabs = [torch.stack([t, torch.zeros_like(t), torch.zeros_like(t)]) for t in (gw, gb)]
        _case_compare(c, tuple(s.sum(0) for s in slabs))
        slabs[which][2].view(-1)[17] = 1.0
        _rejects(c, tuple(s.sum(0) for s in slabs))


FD = [(layer, op, kind) for layer in (2, 3) for op in ("fwd", "dgrad") for kind in ("narrow", "real")]


@pytest.mark.parametrize("row", [0, -1])
@pytest.mark.parametrize("layer,op,kind", FD)
def test_rejects_shifted_tap_in_border_row(layer, op, kind, row):
    """one tap reading its neighbour's pixel, in the top or the bottom output row only"""
    c = R.make_case(layer, op, kind, 5)
    w = c.w.clone()
    ky = 0 if row == 0 else -1    # the one tap row a dgrad border row is fed by
    w[:, :, ky, 0], w[:, :, ky, 1] = c.w[:, :, ky, 1], c.w[:, :, ky, 0]
    good, bad = _got(c), _got(c, w=w)
    if op == "fwd":
        out = good[0].clone()
        out[:, row] = bad[0][:, row]
        _rejects(c, (out, R.PACK[good[2]](out > 0), good[2]))
    else:
        out = good.clone()
        out[:, row] = bad[:, row]
        _rejects(c, out)


@pytest.mark.parametrize("kind", ["narrow", "real"])
@pytest.mark.parametrize("layer,pixel", [(2, 72), (3, 42)])
def test_rejects_zeroed_lone_pixel(layer, pixel, kind):
    """the output pixel a launch (conv2: 72) or a wave (conv3: 42) of its own computes,
    left at zero in one image"""
    c = R.make_case(layer, "fwd", kind, 17)
    out, bits, layout = _got(c)
    ho = R.LAYERS[layer]["ho"]
    for b in (0, 16):
        bad = out.clone()
        bad[b, pixel // ho, pixel % ho] = 0
        _rejects(c, (bad, R.PACK[layout](bad > 0), layout))
        _rejects(c, (bad, bits, layout))


@pytest.mark.parametrize("kind", ["narrow", "real"])
@pytest.mark.parametrize("layer", [2, 3])
def test_rejects_flipped_mask_bit(layer, kind):
    c = R.make_case(layer, "fwd", kind, 5)
    out, bits, layout = _got(c)
    bound = R.K["fwd"] * R.U * c.S
    for want_live in (True, False):   # a decided element of either sign
        e = (((c.z > 0) == want_live) & (c.z.abs() > bound)).nonzero()[3].tolist()
        live = R.UNPACK[layout](bits).clone()
        live[tuple(e)] = not want_live
        _rejects(c, (out, R.PACK[layout](live), layout))


@pytest.mark.parametrize("layer,op,kind", [(l, op, k) for l in (2, 3) for op in R.OPS for k in ("wide_x", "wide_w")])
def test_wide_cases_reject_dropped_lo_plane(layer, op, kind):
    """the wide operand truncated to its hi and mid planes (16 bits)"""
    B = 7 if op == "wgrad" else 5
    c = R.make_case(layer, op, kind, B)
    name = {"fwd": ("a", "w"), "dgrad": ("dz", "w"), "wgrad": ("dz", "a")}[op][kind == "wide_w"]
    _rejects(c, _got(c, **{name: R.drop_lo(getattr(c, name))}))
