"""The conv2 / conv3 kernels (conv2.hip, conv3.hip, their forward bodies, small.hip's
forwards) through the C ABI against float64 (tests/helpers/conv_ref.py), element by
element: all ten entry points — ppo_conv{2,3}_fwd, _fwd_mask, _dgrad, _dgrad_bits, _wgrad
(+ ppo_wgrad_reduce with the conv column map) — at the batch sizes where image-walking
kernels go wrong (B = 1, below and above small_b, around the 16-image lone tile, below
the grid, blocks of 2 and of 3 images, 32-33 images per block past the lone kernel's
512-block cap) and, for the weight gradients, split counts Z = 1, Z > B, odd images
per block and the engine's own Z.

Integer cases (narrow: the hi plane, products 1 / 6 / 9; wide: all three planes of one
operand, products 6 / 9) are asserted with torch.equal against float64: no tolerance.
Real cases are bounded per element by k 2^-24 Σ|x||w| (conv_ref.K).

Every input lies between two NaN-filled guard images (all-ones words for mask bits),
every output is prefilled with NaN between sentinel guards that are compared bit for
bit after the launches: an access one image outside [0, B) lands in allocated memory
and shows in the values."""
import pytest
import torch

from helpers import conv_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _hip():
    from a2c_ppo_acktr import _hip
    return _hip


def _s():
    return torch.cuda.current_stream().cuda_stream


def _cus(gpu):
    return torch.cuda.get_device_properties(gpu).multi_processor_count


class _Knobs:
    """ppo_tune_set(name, value) for the block (None: leave it), the old values restored"""

    def __init__(self, **kv):
        self.kv = {k.encode(): v for k, v in kv.items() if v is not None}

    def __enter__(self):
        self.keep = {k: _hip().call("ppo_tune_get", k) for k in self.kv}
        try:
            for k, v in self.kv.items():
                _hip().call("ppo_tune_set", k, v)
        except BaseException:
            self.__exit__()
            raise

    def __exit__(self, *exc):
        for k, v in self.keep.items():
            _hip().call("ppo_tune_set", k, v)


def _guarded(t, gpu):
    """t ([n][...], CPU or GPU) as rows 1 .. n of a device allocation of n + 2 rows, the
    two others NaN (floats) or all-ones words (mask bits)"""
    buf = torch.empty((t.shape[0] + 2,) + tuple(t.shape[1:]), dtype=t.dtype, device=gpu)
    buf[0] = buf[-1] = NAN if t.dtype.is_floating_point else -1
    view = buf[1:-1]
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 8 == 0
    return view


class _Out:
    """an output of n rows prefilled with NaN (all-ones words for bits) between two
    sentinel rows; check() asserts the sentinels bit for bit"""

    def __init__(self, gpu, shape, dtype=torch.float32):
        self.buf = torch.empty((shape[0] + 2,) + tuple(shape[1:]), dtype=dtype, device=gpu)
        self.raw = self.buf.view(-1).view(torch.uint8)
        self.row = self.raw.numel() // (shape[0] + 2)
        pat = torch.tensor([0xA5, 0xA5, 0x5A, 0x5A], dtype=torch.uint8, device=gpu)
        reps = -(-self.row // 4)
        self.pattern = pat.repeat(reps)[:self.row]
        self.raw[:self.row] = self.pattern
        self.raw[-self.row:] = self.pattern
        self.t = self.buf[1:-1]
        self.t.fill_(NAN if dtype.is_floating_point else -1)

    def ptr(self):
        return self.t.data_ptr()

    def check(self, what):
        assert torch.equal(self.raw[:self.row], self.pattern), f"{what}: wrote before the output"
        assert torch.equal(self.raw[-self.row:], self.pattern), f"{what}: wrote past the output"


def _pack_weights(gpu, layer, w):
    """ppo_pack_weights of w in its layer's slot (zeros elsewhere) -> (keep-alive, forward
    operand, dgrad operand)"""
    Hh, H = _hip(), 64
    w2 = w.cuda() if layer == 2 else torch.zeros(64, 32, 4, 4, device=gpu)
    w3 = w.cuda() if layer == 3 else torch.zeros(32, 64, 3, 3, device=gpu)
    w4 = torch.zeros(H, 1568, device=gpu)
    packed = torch.zeros(Hh.call("ppo_packed_weights_size", H), device=gpu)
    offs = torch.zeros(6, dtype=torch.int64)
    Hh.call("ppo_packed_offsets", H, offs.data_ptr())
    Hh.call("ppo_pack_weights", w2.contiguous().data_ptr(), w3.contiguous().data_ptr(), w4.data_ptr(), H,
            packed.data_ptr(), _s())
    torch.cuda.synchronize()
    pk = [packed.data_ptr() + 4 * int(o) for o in offs]
    return packed, (pk[0] if layer == 2 else pk[1]), (pk[5] if layer == 2 else pk[4])


def _products(kind):
    return {"narrow": (1, 6, 9), "real": (6,)}.get(kind, (6, 9))


def _shapes(layer, B):
    L = R.LAYERS[layer]
    return (B, L["hi"], L["hi"], L["cin"]), (B, L["ho"], L["ho"], L["cout"])


FWD_BITS = {2: ("u64", torch.int64, (81,)), 3: ("u16", torch.int16, (49, 2))}
DGRAD_BITS = {2: ("u32", torch.int32), 3: ("u64", torch.int64)}


def _run_fwd(gpu, layer, B, a, wf, bias, masked):
    """ppo_conv{layer}_fwd or _fwd_mask -> (_Out of relu(z), _Out of the bits or None)"""
    Hh = _hip()
    out = _Out(gpu, _shapes(layer, B)[1])
    if not masked:
        Hh.call(f"ppo_conv{layer}_fwd", a.data_ptr(), B, wf, bias.data_ptr(), out.ptr(), _s())
        return out, None
    _, dtype, per = FWD_BITS[layer]
    bits = _Out(gpu, (B,) + per, dtype)
    Hh.call(f"ppo_conv{layer}_fwd_mask", a.data_ptr(), B, wf, bias.data_ptr(), out.ptr(), bits.ptr(), _s())
    return out, bits


def _run_dgrad(gpu, layer, B, dz, wd, mask, bits):
    Hh = _hip()
    out = _Out(gpu, _shapes(layer, B)[0])
    name = f"ppo_conv{layer}_dgrad" + ("_bits" if bits else "")
    Hh.call(name, dz.data_ptr(), B, wd, mask.data_ptr(), out.ptr(), _s())
    return out


def _fwd_dgrad_params():
    ps = []
    for layer in (2, 3):
        ps += [(layer, "narrow", B) for B in R.FWD_B]
        ps += [(layer, kind, B) for kind in ("wide_x", "wide_w") for B in R.WIDE_B]
        ps += [(layer, "real", B) for B in R.REAL_B]
    return ps


FD_PARAMS = _fwd_dgrad_params()
FD_IDS = [f"conv{l}-{k}-B{B}" for l, k, B in FD_PARAMS]


@pytest.mark.parametrize("layer,kind,B", FD_PARAMS, ids=FD_IDS)
def test_fwd_vs_float64(gpu, layer, kind, B):
    """ppo_conv{2,3}_fwd and _fwd_mask: integer cases bit for bit equal to float64 under
    every product count they are exact for, real cases within k 2^-24 S per element; the
    masked form equals the plain one bit for bit and its bits are (z > 0).  B <= small_b
    runs the image-resident kernels (small_b = 0) and, unmasked, small.hip's."""
    B = R.resolve_b(B, _cus(gpu))
    c = R.make_case(layer, "fwd", kind, B)
    keep, wf, _ = _pack_weights(gpu, layer, c.w)
    a, bias = _guarded(c.a, gpu), _guarded(c.bias.view(1, -1), gpu)
    layout = FWD_BITS[layer][0]
    small_b = _hip().call("ppo_tune_get", b"small_b")
    assert small_b == 4
    worst = 0.0
    for products in _products(kind):
        for sb in ((0, None) if B <= small_b else (None,)):
            what = f"{R.case_id(c)} products={products} small_b={sb}"
            with _Knobs(products=products, small_b=sb):
                plain, _ = _run_fwd(gpu, layer, B, a, wf, bias, False)
                masked, bits = _run_fwd(gpu, layer, B, a, wf, bias, True)
                torch.cuda.synchronize()
            for o in (plain, masked, bits):
                o.check(what)
            worst = max(worst, R.compare(plain.t, c.ref, exact=c.exact, S=c.S, k=R.K["fwd"], what=what))
            R.compare(masked.t, c.ref, exact=c.exact, S=c.S, k=R.K["fwd"], bits=bits.t, layout=layout, z=c.z,
                      what=what + " (mask form)")
            if sb is None and B <= small_b:
                continue   # small.hip's forward and the image-resident masked one: two kernels
            assert torch.equal(plain.t, masked.t), what + ": the mask form differs from the plain one"
            assert torch.equal(bits.t, R.PACK[layout](masked.t > 0)), what + ": bits are not (out > 0)"
    if not c.exact:
        print(f"kernel ratio {R.case_id(c)}: {worst:.3f}")


@pytest.mark.parametrize("layer,kind,B", FD_PARAMS, ids=FD_IDS)
def test_dgrad_vs_float64(gpu, layer, kind, B):
    """ppo_conv{2,3}_dgrad (fp32 mask) and _dgrad_bits (the same mask packed on the host):
    equal to float64 as above, and to each other bit for bit.  (The input-gradient launchers
    have no small-batch path: B <= small_b runs the image-resident kernels as it is.)"""
    B = R.resolve_b(B, _cus(gpu))
    c = R.make_case(layer, "dgrad", kind, B)
    keep, _, wd = _pack_weights(gpu, layer, c.w)
    layout, _ = DGRAD_BITS[layer]
    dz, m = _guarded(c.dz, gpu), _guarded(c.m, gpu)
    mbits = _guarded(R.PACK[layout](c.m > 0), gpu)
    worst = 0.0
    for products in _products(kind):
        what = f"{R.case_id(c)} products={products}"
        with _Knobs(products=products):
            plain = _run_dgrad(gpu, layer, B, dz, wd, m, False)
            frombits = _run_dgrad(gpu, layer, B, dz, wd, mbits, True)
            torch.cuda.synchronize()
        plain.check(what)
        frombits.check(what + " (bits form)")
        worst = max(worst, R.compare(plain.t, c.ref, exact=c.exact, S=c.S, k=R.K["dgrad"], what=what))
        R.compare(frombits.t, c.ref, exact=c.exact, S=c.S, k=R.K["dgrad"], what=what + " (bits form)")
        assert torch.equal(plain.t, frombits.t), what + ": the bits form differs from the fp32-mask one"
    if not c.exact:
        print(f"kernel ratio {R.case_id(c)}: {worst:.3f}")


@pytest.mark.parametrize("stagger", [0, 3])
@pytest.mark.parametrize("op", ["fwd", "dgrad"])
@pytest.mark.parametrize("layer", [2, 3])
def test_deep_walk(gpu, layer, op, stagger):
    """B = 8,200: 32 or 33 images per persistent block (the steady state of the two-stage
    rotation and of conv2 dgrad's deferred stores, and their tail), 513 lone tiles for the
    512 blocks of conv2_fwd_lone_kernel.  Image b is base[b % 37] of a 37-image narrow
    integer case, gathered on the device; the result must equal ref[b % 37] bit for bit,
    compared on the device, plain and mask / bits forms, stagger 0 and 3."""
    B, nb = R.DEEP_B, R.DEEP_BASE
    c = R.make_case(layer, op, "narrow", nb)
    keep, wf, wd = _pack_weights(gpu, layer, c.w)
    idx = torch.arange(B, device=gpu) % nb
    ref32 = c.ref.float()
    assert torch.equal(ref32.double(), c.ref)
    want = ref32.cuda().index_select(0, idx)
    what = f"{R.case_id(c)} deep walk stagger={stagger}"
    with _Knobs(stagger=stagger):
        if op == "fwd":
            a, bias = _guarded(c.a.cuda().index_select(0, idx), gpu), _guarded(c.bias.view(1, -1), gpu)
            outs = [_run_fwd(gpu, layer, B, a, wf, bias, False)[0]]
            masked, bits = _run_fwd(gpu, layer, B, a, wf, bias, True)
            outs.append(masked)
        else:
            layout, _ = DGRAD_BITS[layer]
            dz, m = _guarded(c.dz.cuda().index_select(0, idx), gpu), _guarded(c.m.cuda().index_select(0, idx), gpu)
            mbits = _guarded(R.PACK[layout](c.m > 0).cuda().index_select(0, idx), gpu)
            outs = [_run_dgrad(gpu, layer, B, dz, wd, m, False), _run_dgrad(gpu, layer, B, dz, wd, mbits, True)]
        torch.cuda.synchronize()
    for o in outs:
        o.check(what)
        R.compare(o.t, want, exact=True, what=what)
    if op == "fwd":
        bits.check(what)
        layout = FWD_BITS[layer][0]
        want_bits = R.PACK[layout](c.z > 0).cuda().index_select(0, idx)
        assert torch.equal(bits.t, want_bits), what + ": mask bits"


# ------------------------------------------------------------------ weight gradients
WG_DIMS = {2: (64, 512, 4, 32, 4), 3: (32, 576, 3, 64, 5)}   # M, NW, reduce a, b, engine tiles


def _wg_params():
    ps = []
    for layer in (2, 3):
        ps += [(layer, "narrow", B, Z) for B, Z in R.WGRAD_BZ]
        ps += [(layer, kind, B, Z) for kind in ("wide_x", "wide_w") for B, Z in R.WGRAD_WIDE_BZ]
        ps += [(layer, "real", B, Z) for B, Z in R.WGRAD_REAL_BZ]
    return ps


WG_PARAMS = _wg_params()
WG_IDS = [f"conv{l}-{k}-B{B}-Z{Z}" for l, k, B, Z in WG_PARAMS]


def _engine_z(gpu, layer, B):
    """the split count of _engine.py's weight-gradient launch"""
    tiles = WG_DIMS[layer][4]
    R_ = B * R.LAYERS[layer]["ho"] ** 2
    return _hip().call("ppo_wgrad_splits", R_, tiles, max(_cus(gpu), -(-B // 512)) * tiles, 16)


def _run_wgrad(gpu, layer, B, Z, dz, a):
    Hh = _hip()
    M, NW = WG_DIMS[layer][:2]
    slab, slab_b = _Out(gpu, (Z, M, NW)), _Out(gpu, (Z, M))
    Hh.call(f"ppo_conv{layer}_wgrad", dz.data_ptr(), a.data_ptr(), B, Z, slab.ptr(), slab_b.ptr(), _s())
    return slab, slab_b


def _reduce(gpu, layer, Z, slab, slab_b, gw, gb, scale, accumulate):
    M, NW, ka, kb, _ = WG_DIMS[layer]
    _hip().call("ppo_wgrad_reduce", slab.ptr(), slab_b.ptr(), Z, M, NW, 1, ka, kb, gw.ptr(), gb.ptr(), scale,
                accumulate, _s())


@pytest.mark.parametrize("layer,kind,B,Z", WG_PARAMS, ids=WG_IDS)
def test_wgrad_vs_float64(gpu, layer, kind, B, Z):
    """ppo_conv{2,3}_wgrad + ppo_wgrad_reduce (conv column map): dW and db equal to float64
    (integers: bit for bit; real: per element), every slab entry written, the slabs of
    blocks without an image exactly zero."""
    Z = _engine_z(gpu, layer, B) if Z == "engine" else Z
    c = R.make_case(layer, "wgrad", kind, B)
    L = R.LAYERS[layer]
    dz, a = _guarded(c.dz, gpu), _guarded(c.a, gpu)
    worst = 0.0
    for products in _products(kind):
        what = f"{R.case_id(c)} Z={Z} products={products}"
        with _Knobs(products=products):
            slab, slab_b = _run_wgrad(gpu, layer, B, Z, dz, a)
            gw, gb = _Out(gpu, (L["cout"], L["cin"], L["ks"], L["ks"])), _Out(gpu, (1, L["cout"]))
            _reduce(gpu, layer, Z, slab, slab_b, gw, gb, 1.0, 0)
            torch.cuda.synchronize()
        for o in (slab, slab_b, gw, gb):
            o.check(what)
        for s in (slab.t, slab_b.t):
            assert not torch.isnan(s).any(), what + ": slab entries left unwritten"
            assert (s[B:] == 0).all(), what + ": an idle block's slab is not zero"
        worst = max(worst, R.compare(gw.t, c.ref_w, exact=c.exact, S=c.S_w, k=R.K["wgrad"], what=what + " dW"),
                    R.compare(gb.t[0], c.ref_b, exact=c.exact, S=c.S_b, k=R.K["wgrad"], what=what + " db"))
    if not c.exact:
        print(f"kernel ratio {R.case_id(c)} Z={Z}: {worst:.3f}")


@pytest.mark.parametrize("layer", [2, 3])
def test_wgrad_reduce_scale_and_accumulate(gpu, layer):
    """ppo_wgrad_reduce(scale = 0.5, accumulate = 1) with the conv column map onto an
    integer-prefilled gradient: exactly prefill + 0.5 dW for the weights and prefill + db
    for the bias (the bias sums are unscaled)."""
    B, Z = 7, 2
    c = R.make_case(layer, "wgrad", "narrow", B)
    L = R.LAYERS[layer]
    g = torch.Generator().manual_seed(layer)
    pre_w = torch.randint(-50, 51, c.ref_w.shape, generator=g).double()
    pre_b = torch.randint(-50, 51, (1, L["cout"]), generator=g).double()
    dz, a = _guarded(c.dz, gpu), _guarded(c.a, gpu)
    slab, slab_b = _run_wgrad(gpu, layer, B, Z, dz, a)
    gw, gb = _Out(gpu, c.ref_w.shape), _Out(gpu, (1, L["cout"]))
    gw.t.copy_(pre_w)
    gb.t.copy_(pre_b)
    _reduce(gpu, layer, Z, slab, slab_b, gw, gb, 0.5, 1)
    torch.cuda.synchronize()
    for o in (slab, slab_b, gw, gb):
        o.check(f"conv{layer} reduce")
    R.compare(gw.t, pre_w + 0.5 * c.ref_w, exact=True, what=f"conv{layer} dW, scale 0.5 accumulated")
    R.compare(gb.t, pre_b + c.ref_b.view(1, -1), exact=True, what=f"conv{layer} db, accumulated")
