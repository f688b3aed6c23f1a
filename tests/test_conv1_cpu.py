"""CPU checks of tests/helpers/conv1_ref.py: the float64 conv1 references equal torch float64
autograd of relu(conv) for C in {1, 3, 4, 12}, the decode reference equals the oracle's
preprocess_batch in all three modes, every case tests/test_conv1_gpu.py runs (on a 256-CU
device) meets its generator's precondition, the u8 epilogue reference accepts both
contraction forms and nothing else, and the assertions used on the GPU accept the fp32
yardstick (torch CPU fp32 of the same operation) on every real case and reject planted
errors, each in a single image or element.  Every planted error is also put to the bound
the older conv1 tests use, max|err| <= 1e-5 max|ref| (printed: DESIGN.md §3 lists which
of them it lets through)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import obs_oracle as OO

from helpers import conv1_ref as R

N_CU = 256   # the MI355X; the GPU test reads the device's own count
MATRIX = R.matrix(N_CU)
MIDS = ["-".join(str(v) for v in a if v is not None) for a in MATRIX]


def _like_kernel(c, x=None, w=None):
    """what a correct forward kernel returns for case c (or for a tampered decoded input x /
    weights w): the u8 integer form relu(fl32(A r + b)), else the fp32 yardstick"""
    if c.src == "u8" and c.exact:
        A = R.fwd(c.x if x is None else x, (c.w if w is None else w).double(), None)
        return R.u8_forms(A, c.bias.double())[0]
    rep = {}
    if x is not None:
        rep["x"] = (x / 255.0 if c.src == "u8" else x).float()
    if w is not None:
        rep["w"] = w
    return R.yardstick(c, **rep)[0]


def _like_reduce(c, dz=None, x=None):
    """(gw, gb) a correct weight-gradient kernel + reduce return (u8: the reduce scales by
    1/255; integer u8 cases sum the bytes exactly first)"""
    dz = c.dz if dz is None else dz
    x = c.x if x is None else x
    if c.exact:
        gw, gb = R.wgrad(dz.double(), x)
        return R.reduced(gw, _scale(c)), gb.float()
    return R.wgrad(dz, (x / 255.0 if c.src == "u8" else x).float())


def _scale(c):
    return 1.0 / 255.0 if c.src == "u8" else 1.0


def _refs(c, rows=None):
    return R.set_wgrad_refs(type("refs", (), {})(), c, R.rows_of(c.B) if rows is None else rows)


OLD = {}


def _old_bound(name, got, ref):
    """the older tests' bound on the planted result: True if it lets the error through"""
    ok = (got.double() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()
    OLD.setdefault(name, []).append(ok)
    print(f"old bound 1e-5 max|ref| on '{name}': {'passes' if ok else 'rejects'}")


def _fwd_ref(c, rows=None):
    ref = torch.relu(c.A * R.R255 + c.bias.double()) if c.src == "u8" and c.exact else c.ref
    return ref if rows is None else ref.index_select(0, torch.as_tensor(rows))


def _rejects_fwd(name, c, out, bits=None, rows=None, **kw):
    with pytest.raises(AssertionError):
        R.check_fwd(c, out, bits, rows=rows, **kw)
    _old_bound(name, out, _fwd_ref(c, rows))


def _rejects_wgrad(name, c, refs, gw, gb, **kw):
    with pytest.raises(AssertionError):
        R.check_wgrad(c, refs, gw, gb, scale=_scale(c), **kw)
    s = _scale(c) if c.exact else 1.0
    _old_bound(name, gw, refs.ref_w * s)


# ------------------------------------------------------------------ the helper itself
@pytest.mark.parametrize("C", [1, 3, 4, 12])
def test_float64_helper_equals_autograd(C):
    """fwd and wgrad of the helper == float64 autograd of relu(conv(x, w) + b) with respect
    to w and b, to 1e-12 relative; the rows a launch reads are idx[b] or row0 + b."""
    g = torch.Generator().manual_seed(C)
    B = 3
    x = torch.randn(B, C, 84, 84, generator=g, dtype=torch.float64)
    w = (torch.randn(32, C, 8, 8, generator=g, dtype=torch.float64) * 0.05).requires_grad_()
    b = (torch.randn(32, generator=g, dtype=torch.float64) * 0.1).requires_grad_()
    r = torch.randn(B, 20, 20, 32, generator=g, dtype=torch.float64)
    z = F.conv2d(x, w, b, stride=4).permute(0, 2, 3, 1)
    assert torch.equal(z.detach(), R.fwd(x, w.detach(), b.detach()))
    (torch.relu(z) * r).sum().backward()
    gw, gb = R.wgrad((r * (z > 0)).detach(), x)
    for got, ref in ((gw, w.grad), (gb, b.grad)):
        assert got.shape == ref.shape
        assert (got - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()
    assert R.rows_of(3, None, 5).tolist() == [5, 6, 7] and R.rows_of(2, [4, 1, 4]).tolist() == [4, 1]


@pytest.mark.parametrize("mode", ["norm", "div255", "raw"])
def test_decode_reference_equals_the_oracle(mode):
    """decode() is preprocess_batch; decode64() differs from it by fp32 roundings only (raw:
    not at all), the grey plane transposed and, in raw mode, truncated to u8."""
    g = torch.Generator().manual_seed(3)
    frames = torch.randint(0, 256, (3, 84, 84, 3), dtype=torch.uint8, generator=g)
    mean, std = R.mode_args(mode)
    kw = dict(mean=mean, std=std) if mode == "norm" else dict(div255=(mode == "div255"))
    want = OO.preprocess_batch(frames.numpy(), **kw)
    assert want.dtype == np.float32 and want.shape == (3, 4, 84, 84)
    dec, d64 = R.decode(frames, mode), R.decode64(frames, mode)
    assert torch.equal(dec, torch.from_numpy(want).double())
    if mode == "raw":
        assert torch.equal(d64, dec) and torch.equal(dec, dec.floor())
        assert torch.equal(dec[:, :3], frames.permute(0, 3, 1, 2).double())
    else:
        assert ((d64 - dec).abs() <= 4 * R.U * R.uncancelled(frames, mode)).all()
        assert not torch.equal(d64, dec)
    f = frames.double()
    grey = (f[..., 0] * R.KG[0] + f[..., 1] * R.KG[1] + f[..., 2] * R.KG[2])
    if mode == "raw":
        assert (dec[:, 3] - grey.transpose(1, 2).floor()).abs().max() <= 1    # transposed, truncated
        assert (dec[:, 3] - grey.floor()).abs().max() > 1
    assert (R.uncancelled(frames, mode) >= d64.abs() * (1 - 1e-6)).all()


def test_u8_epilogue_accepts_both_contraction_forms_and_nothing_else():
    c = R.make_case("fwd", "u8", "narrow", 4, 2)
    fused, separate = R.u8_forms(c.A, c.bias.double())
    differ = fused != separate
    assert differ.any(), "the case must tell the two forms apart"
    R.compare_u8(fused, c.A, c.bias)
    R.compare_u8(separate, c.A, c.bias)
    R.compare_u8(torch.where(torch.rand(fused.shape) < 0.5, fused, separate), c.A, c.bias)
    e = tuple(differ.nonzero()[0].tolist())
    lo, hi = min(fused[e], separate[e]), max(fused[e], separate[e])
    for v in (torch.nextafter(lo, torch.tensor(-1e30)), torch.nextafter(hi, torch.tensor(1e30))):
        bad = fused.clone()
        bad[e] = v
        with pytest.raises(AssertionError):
            R.compare_u8(bad, c.A, c.bias)
    # zero bias: one form, fl32(A r); the float64 conv of u / 255 is not it everywhere
    zero = torch.zeros(32)
    f0, f1 = R.u8_forms(c.A, zero.double())
    assert torch.equal(f0, f1)
    R.compare_u8(f0, c.A, zero)
    plain = torch.relu(R.fwd(c.x / 255.0, c.w.double(), None)).float()
    assert not torch.equal(plain, f0)
    # the reduce: fl32(Σ s), s = fl32(1/255), not Σ / 255
    tot = torch.tensor([255.0 * 3, 1000003.0, 4194303.0], dtype=torch.float64)
    assert torch.equal(R.reduced(tot, 1.0 / 255.0), (tot * R.R255).float())
    assert torch.equal(R.reduced(tot, 0.5, torch.tensor([1.0, -2.0, 3.0], dtype=torch.float64)),
                       torch.tensor([383.5, 499999.5, 2097154.5]))


# ------------------------------------------------------------------ every GPU case
@pytest.mark.parametrize("args", MATRIX, ids=MIDS)
def test_case_precondition_and_yardstick(args):
    """make_case asserts the generator's precondition (integers, operand widths, the whole
    byte range, max S <= 2^22); wide sites are disjoint: no output's sum holds two 22-bit
    values.  Integer cases: what a correct kernel returns passes the exact assertion.  Real
    cases: the assertion accepts the fp32 yardstick (test_k_comes_from_the_yardstick holds it
    to a quarter of k)."""
    c = R.make_case(*args)
    assert c.s_max > 0 and (not c.exact or c.s_max <= 2 ** 22)
    if c.kind in ("wide_x", "wide_w"):
        wide_obs = (c.op, c.kind) in (("fwd", "wide_x"), ("wgrad", "wide_w"))
        big_x = (c.x.abs() >= 2 ** 21).double() if wide_obs else None
        if c.op == "fwd":
            hits = R.fwd(big_x, torch.ones_like(c.w, dtype=torch.float64), None) if wide_obs else \
                (c.w.abs() >= 2 ** 21).sum((1, 2, 3)).double()
        else:
            big_dz = (c.dz.abs() >= 2 ** 21).double()
            hits = R.wgrad(torch.ones_like(big_dz), big_x)[0] if wide_obs else big_dz.sum((0, 1, 2))
        assert hits.max().item() == 1, "two wide values meet in one sum"
    if c.op == "fwd":
        out = _like_kernel(c)
        worst = R.check_fwd(c, out, R.pack_u32(out > 0))
        if c.src == "rgb" and not c.exact:
            worst = max(worst, R.check_fwd(c, out, R.pack_u32(out > 0), aff=True))
    else:
        refs = _refs(c)
        gw, gb = _like_reduce(c)
        worst = R.check_wgrad(c, refs, gw, gb, scale=_scale(c))
        if c.src == "rgb" and not c.exact:
            worst = max(worst, R.check_wgrad(c, refs, gw, gb, aff=True))
    if not c.exact:
        print(f"yardstick ratio {R.case_id(c)}: {worst:.3f}")


def test_k_comes_from_the_yardstick():
    """K[op] = 4 x the worst ratio |fp32 - ref| / (2^-24 S_e) torch CPU fp32 reaches over the
    real cases of the operation, rounded up to a whole number, not below 8."""
    worst = {"fwd": (0.0, ""), "wgrad": (0.0, "")}
    for args in R.real_cases(N_CU):
        c = R.make_case(*args)
        worst[c.op] = max(worst[c.op], (R.yardstick_ratio(c), R.case_id(c)))
    print("worst yardstick ratios", worst)
    for op, (r, _) in worst.items():
        assert R.K[op] >= 8 and 4 * r <= R.K[op], (op, r)
        assert R.K[op] <= max(8, 4 * r * 1.5), "k is far above 4 x the yardstick: re-derive it"


# ------------------------------------------------------------------ planted errors
B_P = 5
WG = [("u8", "narrow", None), ("u8", "real", None), ("f32", "narrow", None), ("f32", "real", None),
      ("rgb", "narrow", "raw"), ("rgb", "real", "norm")]
FW = WG


@pytest.mark.parametrize("src,kind,mode", WG)
def test_rejects_image_left_out_or_counted_twice(src, kind, mode):
    c = R.make_case("wgrad", src, kind, 4, B_P, mode)
    refs = _refs(c)
    R.check_wgrad(c, refs, *_like_reduce(c), scale=_scale(c))
    for b in (0, B_P - 1):
        dz = c.dz.clone()
        dz[b] = 0
        _rejects_wgrad("an image left out", c, refs, *_like_reduce(c, dz=dz))
    twice = _like_reduce(c, dz=torch.cat([c.dz, c.dz[-1:]]), x=torch.cat([c.x, c.x[-1:]]))
    _rejects_wgrad("an image counted twice", c, refs, *twice)
    with pytest.raises(AssertionError):   # in the bias gradient only
        R.check_wgrad(c, refs, _like_reduce(c)[0], twice[1], scale=_scale(c))


@pytest.mark.parametrize("src,kind,mode", WG)
def test_rejects_wrong_rows(src, kind, mode):
    """row0 off by one (every image reads its neighbour's row) and the idx gather replaced
    by row0 + b, forward and weight gradient"""
    idx = [3, 0, 4, 0, 2]
    for name, true_rows, read_rows in (("row0 off by one", list(range(B_P)), [1, 2, 3, 4, 0]),
                                       ("idx gather replaced by row0 + b", idx, list(range(B_P)))):
        c = R.make_case("fwd", src, kind, 4, B_P, mode)
        R.check_fwd(c, _like_kernel(c).index_select(0, torch.tensor(true_rows)), rows=true_rows)
        _rejects_fwd(name, c, _like_kernel(c).index_select(0, torch.tensor(read_rows)), rows=true_rows)
        c = R.make_case("wgrad", src, kind, 4, B_P, mode)
        refs = _refs(c, true_rows)
        R.check_wgrad(c, refs, *_like_reduce(c, x=c.x[true_rows]), scale=_scale(c))
        _rejects_wgrad(name, c, refs, *_like_reduce(c, x=c.x[read_rows]))


def _one_image(c, bad_x=None, bad_w=None, b=B_P - 1):
    """a correct forward result with image b's rows computed from the tampered input"""
    good, bad = _like_kernel(c), _like_kernel(c, x=bad_x, w=bad_w)
    out = good.clone()
    out[b] = bad[b]
    return out


@pytest.mark.parametrize("src,kind,mode", FW)
def test_rejects_single_image_forward_errors(src, kind, mode):
    c = R.make_case("fwd", src, kind, 4, B_P, mode)
    x = c.x.clone()
    x[:, [0, 1]] = c.x[:, [1, 0]]
    _rejects_fwd("two channels swapped", c, _one_image(c, bad_x=x))
    w = c.w.clone()      # tap (ky 3, kx 5) reads the element of tap (3, 6) and the reverse
    w[:, :, 3, 5], w[:, :, 3, 6] = c.w[:, :, 3, 6], c.w[:, :, 3, 5]
    _rejects_fwd("a tap in the kx >= 4 half shifted by one element", c, _one_image(c, bad_w=w))
    x = c.x.clone()
    x[..., 83] = 0
    _rejects_fwd("input column 83 dropped", c, _one_image(c, bad_x=x))
    cw = R.make_case("wgrad", src, kind, 4, B_P, mode)
    xw = cw.x.clone()
    xw[-1, :, :, 83] = 0
    _rejects_wgrad("input column 83 dropped", cw, _refs(cw), *_like_reduce(cw, x=xw))


@pytest.mark.parametrize("kind,mode", [("narrow", "raw"), ("real", "norm"), ("real", "div255")])
def test_rejects_grey_plane_errors(kind, mode):
    c = R.make_case("fwd", "rgb", kind, 4, B_P, mode)
    x = c.x.clone()
    x[:, 3] = c.x[:, 3].transpose(1, 2)
    _rejects_fwd("the grey plane not transposed", c, _one_image(c, bad_x=x, b=2))
    if mode == "raw":
        f = c.rows.float()
        grey = ((f[..., 0] * np.float32(0.299) + f[..., 1] * np.float32(0.587)) + f[..., 2] * np.float32(0.114))
        x = c.x.clone()
        x[:, 3] = grey.transpose(1, 2).double()
        assert not torch.equal(x, c.x)
        _rejects_fwd("the grey plane not truncated in raw mode", c, _one_image(c, bad_x=x, b=2))


@pytest.mark.parametrize("kind", ["narrow", "real"])
def test_rejects_single_element_u8_errors(kind):
    c = R.make_case("fwd", "u8", kind, 4, B_P)
    e = tuple((c.x[:, :, 8:76, 8:76] >= 128).nonzero()[11].tolist())
    e = (e[0], e[1], e[2] + 8, e[3] + 8)
    x = c.x.clone()
    x[e] -= 128
    _rejects_fwd("the pixel's top bit cleared", c, _like_kernel(c, x=x))
    out = _like_kernel(c)
    pre = (c.A * R.R255 if c.exact else c.z - c.bias.double())
    o = tuple((pre > 1.0).nonzero()[5].tolist())
    out[o] = torch.relu(pre[o] / 255.0 + c.bias[o[-1]]).float()
    _rejects_fwd("the 1/255 applied twice", c, out)
    cw = R.make_case("wgrad", "u8", kind, 4, B_P)
    refs = _refs(cw)
    gw, gb = _like_reduce(cw)
    gw = gw.clone()
    gw.view(-1)[1234] = gw.view(-1)[1234] / 255.0
    _rejects_wgrad("the 1/255 applied twice", cw, refs, gw, gb)


@pytest.mark.parametrize("src,kind,mode", FW)
def test_rejects_flipped_mask_bit(src, kind, mode):
    c = R.make_case("fwd", src, kind, 4, B_P, mode)
    out = _like_kernel(c)
    bits = R.pack_u32(out > 0)
    R.check_fwd(c, out, bits)
    bound = R.K["fwd"] * R.U * c.S
    for want_live in (True, False):   # a decided element of either sign
        e = (((c.z > 0) == want_live) & (c.z.abs() > bound)).nonzero()[3].tolist()
        live = R.unpack_u32(bits).clone()
        live[tuple(e)] = not want_live
        with pytest.raises(AssertionError):
            R.check_fwd(c, out, R.pack_u32(live))
    OLD.setdefault("a flipped mask bit", []).append(False)   # the older tests compare the bits with (out > 0) too


@pytest.mark.parametrize("src,kind,mode", WG)
def test_rejects_stray_value_in_idle_slab(src, kind, mode):
    """split partials summed as ppo_wgrad_reduce sums them, an idle block's slab holding one
    stray value instead of zeros"""
    c = R.make_case("wgrad", src, kind, 4, B_P, mode)
    refs = _refs(c)
    raw_w, raw_b = R.wgrad(c.dz.double(), c.x) if c.exact else _like_reduce(c)
    for which in (0, 1):
        slabs = [torch.stack([t, torch.zeros_like(t), torch.zeros_like(t)]) for t in (raw_w, raw_b)]
        if c.exact:
            R.check_slabs(c, refs, slabs[0].view(3, 32, -1), slabs[1], 1, walks_images=True)
        slabs[which][2].view(-1)[17] = 1.0
        with pytest.raises(AssertionError):
            R.check_slabs(c, refs, slabs[0].view(3, 32, -1), slabs[1], 1, walks_images=True)
        tot_w, tot_b = (s.sum(0) for s in slabs)
        got = (R.reduced(tot_w, _scale(c)), tot_b.float()) if c.exact else (tot_w, tot_b)
        with pytest.raises(AssertionError):
            R.check_wgrad(c, refs, *got, scale=_scale(c))
        if which == 0:
            _old_bound("a stray value in an idle block's slab", got[0], refs.ref_w * (_scale(c) if c.exact else 1.0))


WIDE = [("fwd", "u8", "wide_w", None), ("fwd", "f32", "wide_x", None), ("fwd", "f32", "wide_w", None),
        ("fwd", "rgb", "wide_w", "raw"), ("wgrad", "u8", "wide_x", None), ("wgrad", "f32", "wide_x", None),
        ("wgrad", "f32", "wide_w", None), ("wgrad", "rgb", "wide_x", "raw")]


@pytest.mark.parametrize("op,src,kind,mode", WIDE)
def test_wide_cases_reject_dropped_lo_plane(op, src, kind, mode):
    """the wide operand truncated to its hi and mid planes (16 bits)"""
    c = R.make_case(op, src, kind, 4, 7 if op == "wgrad" else 5, mode)
    if op == "fwd":
        cut = dict(w=R.drop_lo(c.w)) if kind == "wide_w" else dict(x=R.drop_lo(c.x.float()).double())
        _rejects_fwd("a dropped lo plane", c, _like_kernel(c, **cut))
    else:
        cut = dict(dz=R.drop_lo(c.dz)) if kind == "wide_x" else dict(x=R.drop_lo(c.x.float()).double())
        _rejects_wgrad("a dropped lo plane", c, _refs(c), *_like_reduce(c, **cut))


def test_old_bound_summary():
    """not an assertion of the kernels: prints, per planted error, in how many of its cases
    the older bound max|err| <= 1e-5 max|ref| would have let it through (run the file with
    -s; the planted-error tests above fill the table)"""
    for name, oks in sorted(OLD.items()):
        print(f"old bound: '{name}' passes in {sum(oks)} of {len(oks)} planted cases")
