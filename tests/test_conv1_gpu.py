"""The conv1 kernels (conv1.hip, conv1_fwd_body.h, conv1f.hip, conv1w.hip, rgbaff.hip, the
first phase of trunk.hip, small.hip's small_conv1_kernel) through the C ABI against float64
(tests/helpers/conv1_ref.py), element by element: the eleven entry points —
ppo_conv1_fwd, _fwd_mask, _fwd_f32, _fwd_rgb, ppo_trunk_fwd, ppo_conv1_wgrad, _wgrad_f32,
_wgrad_rgb (+ ppo_wgrad_reduce kind 0) — over their dispatch matrix (u8 / fp32 rows and raw
RGB frames, fused decode and affine fold, the tile GEMM of the other channel counts and of
conv1_fwd 9, the small-batch kernel, the four u8 weight-gradient kernels and the
half-precision one) at the batch sizes where image-walking kernels go wrong, every
prefetch depth of the weight gradients (blocks of 0, 1, 2, 3, 4, 5 and 16 / 17 images),
the three row-addressing forms, rows beyond 2^32 bytes and B = 8,200.

Integer cases are asserted bit for bit (u8 rows: against the two forms of the epilogue
relu(A fl32(1/255) + b)); real cases are bounded per element by k 2^-24 S_e (conv1_ref.K).
Observation rows lie between guard images (NaN; all 255 for bytes), dz between NaN images;
every output, mask word, slab and bias partial is prefilled with NaN (all-ones words)
between sentinel rows that are compared bit for bit after the launches."""
import pytest
import torch

from helpers import conv1_ref as R
from test_conv_gpu import _cus, _guarded, _hip, _Knobs, _Out, _s

pytestmark = pytest.mark.gpu

NAN = float("nan")
BEFORE = 5     # guard rows in front of the storage rows


def _ptr(t):
    return None if t is None else t.data_ptr()


def _at(o):
    """the address of an _Out's first row (of its trailing sentinel, where it has no rows)"""
    return None if o is None else o.buf[1:].data_ptr()


class _Rows:
    """the case's storage rows behind BEFORE guard images and in front of one (NaN; all 255
    for bytes), and the three ways a launch addresses them"""

    def __init__(self, rows, gpu):
        n = rows.shape[0]
        self.buf = torch.empty((BEFORE + n + 1,) + tuple(rows.shape[1:]), dtype=rows.dtype, device=gpu)
        self.buf.fill_(NAN if rows.dtype.is_floating_point else 255)
        self.buf[BEFORE:BEFORE + n].copy_(rows)
        self.n, self.gpu = n, gpu

    def args(self, form="row0=0", rows=None):
        """(obs pointer, idx pointer or None, row0) of a launch over the case's rows `rows`
        (idx form; None: 0 .. n-1); the idx tensor is kept alive on self"""
        if form == "idx":
            r = torch.arange(self.n) if rows is None else torch.as_tensor(rows)
            self.idx = (r + BEFORE).to(torch.int64).to(self.gpu)
            return self.buf.data_ptr(), self.idx.data_ptr(), 0
        assert rows is None
        if form == "row0=0":
            return self.buf[BEFORE:].data_ptr(), None, 0
        assert form == "row0=5" and BEFORE == 5
        return self.buf.data_ptr(), None, BEFORE


def _products(kind):
    return {"narrow": (1, 6, 9), "real": (6,)}.get(kind, (6, 9))


def _mean_std(c, gpu):
    if c.src != "rgb":
        return None, 1.0
    mean, std = R.mode_args(c.mode)
    return (None if mean is None else torch.from_numpy(mean).float().to(gpu)), std


def _run_fwd(gpu, c, entry, addr, B, w, bias, masked, mean=None, std=1.0):
    """one forward launch of `entry` (u8 / f32: ppo_conv1_fwd(_mask) with obs_is_u8 1 / 0;
    f32x: ppo_conv1_fwd_f32; rgb: ppo_conv1_fwd_rgb) -> (_Out of relu(z), _Out of the bits or
    None)"""
    Hh = _hip()
    obs, idx, row0 = addr
    out = _Out(gpu, (B, 20, 20, 32))
    bits = _Out(gpu, (B, 400), torch.int32) if masked else None
    if entry in ("u8", "f32"):
        head = (obs, int(entry == "u8"), idx, row0, c.C, B, w.data_ptr(), bias.data_ptr(), _at(out))
        if masked:
            Hh.call("ppo_conv1_fwd_mask", *head, _at(bits), _s())
        else:
            Hh.call("ppo_conv1_fwd", *head, _s())
    elif entry == "f32x":
        Hh.call("ppo_conv1_fwd_f32", obs, idx, row0, B, w.data_ptr(), bias.data_ptr(), _at(out),
                _at(bits), _s())
    else:
        Hh.call("ppo_conv1_fwd_rgb", obs, idx, row0, B, _ptr(mean), std, w.data_ptr(), bias.data_ptr(), _at(out),
                _at(bits), _s())
    return out, bits


def _fwd_both(gpu, c, entry, addr, B, w, b1, what, mean=None, std=1.0, **check):
    """the plain and the mask form of one forward: both asserted against the case, the two
    outputs bit-equal, guards intact.  Returns (plain output, worst ratio)."""
    plain, _ = _run_fwd(gpu, c, entry, addr, B, w, b1, False, mean, std)
    masked, bits = _run_fwd(gpu, c, entry, addr, B, w, b1, True, mean, std)
    torch.cuda.synchronize()
    for o in (plain, masked, bits):
        o.check(what)
    worst = R.check_fwd(c, plain.t, what=what, **check)
    R.check_fwd(c, masked.t, bits.t, what=what + " (mask form)", **check)
    assert torch.equal(plain.t, masked.t), what + ": the mask form differs from the plain one"
    return plain.t, worst


FWD_PARAMS = [p for p in R.fwd_params() if p[0] != "trunk"]
FWD_KNOBS = {"u8_img": dict(conv1_fwd=0), "u8_tile": dict(conv1_fwd=9)}


@pytest.mark.parametrize("path,kind,B", FWD_PARAMS, ids=[f"{p}-{k}-B{B}" for p, k, B in FWD_PARAMS])
def test_fwd_vs_float64(gpu, path, kind, B):
    """Every C = 4 forward path but the trunk, plain and mask form, small_b = 0: integer
    cases bit for bit under every product count they are exact for (u8 rows: both bias
    forms, and plain equality with a zero bias), real cases within k 2^-24 S_e.  fp32 rows:
    ppo_conv1_fwd(obs_is_u8 = 0) is bit-equal to ppo_conv1_fwd_f32.  Frames: the fused decode
    (rgb_aff 0) against the reference chain, the affine fold (rgb_aff 1) against the float64
    chain; the raw mode takes the fused decode under both settings."""
    src, mode, _ = R.FWD_PATHS[path]
    B = R.resolve_b(B, _cus(gpu))
    c = R.make_case("fwd", src, kind, 4, B, mode)
    st = _Rows(c.rows, gpu)
    w, bias, zero = c.w.to(gpu), c.bias.to(gpu), torch.zeros(32, device=gpu)
    mean, std = _mean_std(c, gpu)
    entry = {"u8": "u8", "f32": "f32x", "rgb": "rgb"}[src]
    worst = {}
    for products in _products(kind):
        for aff in ((0, 1) if src == "rgb" else (None,)):
            what = f"{path} {R.case_id(c)} products={products} rgb_aff={aff}"
            folded = bool(aff) and mode != "raw"
            with _Knobs(products=products, small_b=0, rgb_aff=aff, **FWD_KNOBS.get(path, {})):
                out, r = _fwd_both(gpu, c, entry, st.args(), B, w, bias, what, mean, std, aff=folded)
                if src == "u8" and c.exact:
                    _fwd_both(gpu, c, entry, st.args(), B, w, zero, what + " zero bias", bias=torch.zeros(32))
                if src == "f32":
                    routed, _ = _fwd_both(gpu, c, "f32", st.args(), B, w, bias, what + " (routed)")
                    assert torch.equal(routed, out), what + ": ppo_conv1_fwd differs from ppo_conv1_fwd_f32"
            key = "fold" if folded else "decode" if src == "rgb" else path
            worst[key] = max(worst.get(key, 0.0), r)
    if not c.exact:
        for key, r in worst.items():
            print(f"kernel ratio fwd {key} {R.case_id(c)}: {r:.3f}")


@pytest.mark.parametrize("B", R.OTHER_B)
@pytest.mark.parametrize("C", R.OTHER_C)
@pytest.mark.parametrize("src", ["u8", "f32"])
def test_fwd_other_channel_counts(gpu, src, C, B):
    """C in {1, 3, 12}, B > small_b: the tile GEMM with 64, 192 and 768 columns against its
    256-column tile, plain and mask form (relu_bits_kernel)."""
    for kind in ("narrow", "real"):
        c = R.make_case("fwd", src, kind, C, B)
        st = _Rows(c.rows, gpu)
        w, bias = c.w.to(gpu), c.bias.to(gpu)
        what = f"{R.case_id(c)}"
        with _Knobs(small_b=0):
            _, r = _fwd_both(gpu, c, src, st.args(), B, w, bias, what)
            if src == "u8" and c.exact:
                _fwd_both(gpu, c, src, st.args(), B, w, torch.zeros(32, device=gpu), what + " zero bias",
                          bias=torch.zeros(32))
        if not c.exact:
            print(f"kernel ratio fwd tile_C{C} {R.case_id(c)}: {r:.3f}")


@pytest.mark.parametrize("C", R.SMALL_C)
@pytest.mark.parametrize("src", ["u8", "f32"])
def test_fwd_small_batch(gpu, src, C):
    """The unmasked forward at and around small_b (default 4): B = 1 and 4, and B = 5 with
    small_b 5 (small.hip's kernel where it has one: C <= 8) and with small_b 4 (the large-batch
    kernel).  Every channel count must give the same correct result on either side of the
    threshold: a 12-channel policy acts with 4 environments as it does with 5."""
    assert _hip().call("ppo_tune_get", b"small_b") == 4
    for kind in ("narrow", "real"):
        for B, small_b in ((1, None), (4, None), (5, 5), (5, 4)):
            c = R.make_case("fwd", src, kind, C, B)
            st = _Rows(c.rows, gpu)
            w, bias = c.w.to(gpu), c.bias.to(gpu)
            what = f"{R.case_id(c)} small_b={small_b}"
            with _Knobs(small_b=small_b):
                for form in ("row0=0", "idx", "row0=5"):
                    rows = [B - 1 - b for b in range(B)] if form == "idx" else None
                    out, _ = _run_fwd(gpu, c, src, st.args(form, rows), B, w, bias, False)
                    torch.cuda.synchronize()
                    out.check(what)
                    r = R.check_fwd(c, out.t, rows=rows, what=f"{what} {form}")
                if src == "u8" and c.exact:
                    out, _ = _run_fwd(gpu, c, src, st.args(), B, w, torch.zeros(32, device=gpu), False)
                    torch.cuda.synchronize()
                    R.check_fwd(c, out.t, bias=torch.zeros(32), what=what + " zero bias")
            if not c.exact:
                print(f"kernel ratio fwd small {R.case_id(c)} small_b={small_b}: {r:.3f}")


# ------------------------------------------------------------------ the fused trunk
def _trunk_weights(gpu, seed=0):
    """real conv2 / conv3 weights packed by ppo_pack_weights -> (keep-alive, w2p, b2, w3p, b3)"""
    Hh, H = _hip(), 64
    g = torch.Generator().manual_seed(seed)
    w2 = (torch.randn(64, 32, 4, 4, generator=g) * 0.05).to(gpu)
    w3 = (torch.randn(32, 64, 3, 3, generator=g) * 0.05).to(gpu)
    b2, b3 = (torch.randn(64, generator=g) * 0.1).to(gpu), (torch.randn(32, generator=g) * 0.1).to(gpu)
    w4 = torch.zeros(H, 1568, device=gpu)
    packed = torch.zeros(Hh.call("ppo_packed_weights_size", H), device=gpu)
    offs = torch.zeros(6, dtype=torch.int64)
    Hh.call("ppo_packed_offsets", H, offs.data_ptr())
    Hh.call("ppo_pack_weights", w2.data_ptr(), w3.data_ptr(), w4.data_ptr(), H, packed.data_ptr(), _s())
    torch.cuda.synchronize()
    return (packed, b2, b3), packed.data_ptr() + 4 * int(offs[0]), b2, packed.data_ptr() + 4 * int(offs[1]), b3


def _run_trunk(gpu, addr, B, w, bias, tw, masked):
    Hh = _hip()
    _, w2p, b2, w3p, b3 = tw
    obs, idx, row0 = addr
    a1, a2, a3 = _Out(gpu, (B, 20, 20, 32)), _Out(gpu, (B, 9, 9, 64)), _Out(gpu, (B, 7, 7, 32))
    m1 = _Out(gpu, (B, 400), torch.int32) if masked else None
    m2 = _Out(gpu, (B, 81), torch.int64) if masked else None
    Hh.call("ppo_trunk_fwd", obs, idx, row0, B, w.data_ptr(), bias.data_ptr(), _at(a1), _at(m1),
            w2p, b2.data_ptr(), _at(a2), _at(m2), w3p, b3.data_ptr(), _at(a3), _s())
    return a1, a2, a3, m1, m2


def _check_trunk(gpu, c, addr, B, w, bias, tw, what, **check):
    """ppo_trunk_fwd, fused (no masks) and with masks: a1 / m1 against the case and bit-equal
    to ppo_conv1_fwd(_mask); a2, a3, m2 bit-equal to ppo_conv2_fwd(_mask) / ppo_conv3_fwd of
    that a1"""
    Hh = _hip()
    _, w2p, b2, w3p, b3 = tw
    for masked in (False, True):
        a1, a2, a3, m1, m2 = _run_trunk(gpu, addr, B, w, bias, tw, masked)
        o1, ob1 = _run_fwd(gpu, c, "u8", addr, B, w, bias, masked)
        o2, o3 = _Out(gpu, (B, 9, 9, 64)), _Out(gpu, (B, 7, 7, 32))
        ob2 = _Out(gpu, (B, 81), torch.int64)
        if masked:
            Hh.call("ppo_conv2_fwd_mask", _at(a1), B, w2p, b2.data_ptr(), _at(o2), _at(ob2), _s())
        else:
            Hh.call("ppo_conv2_fwd", _at(a1), B, w2p, b2.data_ptr(), _at(o2), _s())
        Hh.call("ppo_conv3_fwd", _at(a2), B, w3p, b3.data_ptr(), _at(o3), _s())
        torch.cuda.synchronize()
        w_ = f"{what} masked={masked}"
        for o in (a1, a2, a3, o1, o2, o3) + ((m1, m2, ob1, ob2) if masked else ()):
            o.check(w_)
        R.check_fwd(c, a1.t, m1.t if masked else None, what=w_, **check)
        assert torch.equal(a1.t, o1.t), w_ + ": a1 differs from ppo_conv1_fwd"
        assert torch.equal(a2.t, o2.t), w_ + ": a2 differs from ppo_conv2_fwd of a1"
        assert torch.equal(a3.t, o3.t), w_ + ": a3 differs from ppo_conv3_fwd of a2"
        assert not torch.isnan(a3.t).any()
        if masked:
            assert torch.equal(m1.t, ob1.t), w_ + ": m1 differs from ppo_conv1_fwd_mask"
            assert torch.equal(m2.t, ob2.t), w_ + ": m2 differs from ppo_conv2_fwd_mask"
    return a1.t


@pytest.mark.parametrize("B", R.FWD_B)
def test_trunk_fwd(gpu, B):
    B = R.resolve_b(B, _cus(gpu))
    c = R.make_case("fwd", "u8", "narrow", 4, B)
    st = _Rows(c.rows, gpu)
    tw = _trunk_weights(gpu)
    with _Knobs(small_b=0, conv1_fwd=0):
        _check_trunk(gpu, c, st.args(), B, c.w.to(gpu), c.bias.to(gpu), tw, f"trunk {R.case_id(c)}")


# ------------------------------------------------------------------ B = 8,200
@pytest.mark.parametrize("path", ["u8_img", "f32_img", "rgb_fold", "trunk"])
def test_fwd_deep_walk(gpu, path):
    """B = 8,200, idx[b] = b mod 37 over 37 base images: 32 or 33 images per persistent
    block.  The 37-image result is asserted against float64; the deep result must equal it,
    tiled, bit for bit (compared on the device), mask words included."""
    B, nb = R.DEEP_B, R.DEEP_BASE
    src, mode, kind = {"u8_img": ("u8", None, "narrow"), "f32_img": ("f32", None, "narrow"),
                       "rgb_fold": ("rgb", "norm", "real"), "trunk": ("u8", None, "narrow")}[path]
    c = R.make_case("fwd", src, kind, 4, nb, mode)
    st = _Rows(c.rows, gpu)
    w, bias = c.w.to(gpu), c.bias.to(gpu)
    mean, std = _mean_std(c, gpu)
    deep_rows = torch.arange(B) % nb
    tile = deep_rows.to(gpu)
    what = f"{path} deep walk"
    with _Knobs(small_b=0, conv1_fwd=0, rgb_aff=1):
        if path == "trunk":
            tw = _trunk_weights(gpu)
            base = _check_trunk(gpu, c, st.args("idx"), nb, w, bias, tw, what + " base")
            a1, a2, a3, _, _ = _run_trunk(gpu, st.args("idx", deep_rows), B, w, bias, tw, False)
            b1, b2_, b3_, _, _ = _run_trunk(gpu, st.args("idx"), nb, w, bias, tw, False)
            torch.cuda.synchronize()
            for deep, small in ((a1, b1), (a2, b2_), (a3, b3_)):
                deep.check(what)
                assert torch.equal(deep.t, small.t.index_select(0, tile)), what
            assert torch.equal(b1.t, base)
            return
        entry = {"u8": "u8", "f32": "f32x", "rgb": "rgb"}[src]
        base, _ = _fwd_both(gpu, c, entry, st.args("idx"), nb, w, bias, what + " base", mean, std, aff=src == "rgb")
        out, bits = _run_fwd(gpu, c, entry, st.args("idx", deep_rows), B, w, bias, True, mean, std)
        torch.cuda.synchronize()
        out.check(what)
        bits.check(what)
        assert torch.equal(out.t, base.index_select(0, tile)), what + ": differs from the tiled 37-image result"
        assert torch.equal(bits.t, R.pack_u32(base > 0).index_select(0, tile)), what + ": mask words"


# ------------------------------------------------------------------ weight gradients
def _engine_z(gpu, B):
    """the split count of _engine.py's conv1 weight-gradient launch"""
    return _hip().call("ppo_wgrad_splits", B * 400, 1, max(_cus(gpu), -(-B // 512)), 16)


def _run_wgrad(gpu, c, entry, addr, B, Z, dz, mean=None, std=1.0, slabs=None):
    """one weight-gradient launch (entries as _run_fwd's) -> (slab _Out, bias-partial _Out)"""
    Hh = _hip()
    obs, idx, row0 = addr
    slab, slab_b = slabs or (_Out(gpu, (Z, 32, c.C * 64)), _Out(gpu, (Z, 32)))
    if entry in ("u8", "f32"):
        Hh.call("ppo_conv1_wgrad", dz.data_ptr(), obs, int(entry == "u8"), idx, row0, c.C, B, Z, _at(slab),
                _at(slab_b), _s())
    elif entry == "f32x":
        Hh.call("ppo_conv1_wgrad_f32", dz.data_ptr(), obs, idx, row0, B, Z, _at(slab), _at(slab_b), _s())
    else:
        Hh.call("ppo_conv1_wgrad_rgb", dz.data_ptr(), obs, idx, row0, B, _ptr(mean), std, Z, _at(slab), _at(slab_b),
                _s())
    return slab, slab_b


def _reduce(gpu, c, Z, slab, slab_b, scale, accumulate=0, pre=None):
    gw, gb = _Out(gpu, (32, c.C, 8, 8)), _Out(gpu, (1, 32))
    if pre is not None:
        gw.t.copy_(pre[0])
        gb.t.copy_(pre[1].view(1, 32))
    _hip().call("ppo_wgrad_reduce", _at(slab), _at(slab_b), Z, 32, c.C * 64, 0, 0, 0, _at(gw), _at(gb), scale,
                accumulate, _s())
    return gw, gb


def _wgrad_checked(gpu, c, entry, addr, rows, B, Z, dz, what, *, mean=None, std=1.0, aff=False, walks=True):
    """launch + reduce + every assertion of one weight gradient; returns the worst ratio"""
    refs = R.wgrad_refs(c.op, c.src, c.kind, c.C, c.B, c.mode, tuple(int(r) for r in rows))
    scale = 1.0 / 255.0 if c.src == "u8" else 1.0
    slab, slab_b = _run_wgrad(gpu, c, entry, addr, B, Z, dz, mean, std)
    gw, gb = _reduce(gpu, c, Z, slab, slab_b, scale)
    torch.cuda.synchronize()
    for o in (slab, slab_b, gw, gb):
        o.check(what)
    if aff and not c.exact:     # the fold's slab is written by three kernels: only "written" holds per block
        assert not torch.isnan(slab.t).any() and not torch.isnan(slab_b.t).any(), what + ": slab entries left unwritten"
    else:
        R.check_slabs(c, refs, slab.t, slab_b.t, B, walks_images=walks, what=what)
    return R.check_wgrad(c, refs, gw.t, gb.t[0], aff=aff, scale=scale, what=what)


# path -> (entry, knobs, product counts of the narrow case (None: _products))
WG_RUN = {
    "u8_kw9": ("u8", dict(conv1_wgrad=9), (6, 9)),
    "u8_kw10": ("u8", dict(conv1_wgrad=10), (6,)),
    "u8_kw8": ("u8", dict(conv1_wgrad=8), (6,)),
    "u8_kw5": ("u8", dict(conv1_wgrad=5), (6,)),
    "u8_half": ("u8", dict(conv1_wgrad=9), (1,)),
    "f32": ("f32x", {}, None),
    "f32_routed": ("f32", {}, (6,)),
    "rgb_raw": ("rgb", {}, None),
    "rgb_norm": ("rgb", {}, None),
    "rgb_div255": ("rgb", {}, None),
}
WG_PARAMS = R.wgrad_params()


@pytest.mark.parametrize("path,B,Z", WG_PARAMS, ids=[f"{p}-B{B}-Z{Z}" for p, B, Z in WG_PARAMS])
def test_wgrad_vs_float64(gpu, path, B, Z):
    """Every weight-gradient path + ppo_wgrad_reduce kind 0 (scale 1/255 for u8 rows): every
    slab and bias-partial entry written, idle blocks' slabs zero, the float64 sum of the
    slabs equal to the reference on integer cases, dW and db bit for bit (integers) or
    within k 2^-24 S_e (real).  Rows gathered through idx, as the engine passes them."""
    src, mode, C, _ = R.WGRAD_PATHS[path]
    entry, knobs, narrow_products = WG_RUN.get(path, (src, {}, (6,)))
    kinds = R.wgrad_kinds(path, B, Z)
    Z = _engine_z(gpu, B) if Z == "engine" else Z
    for kind in kinds:
        c = R.make_case("wgrad", src, kind, C, B, mode)
        st = _Rows(c.rows, gpu)
        dz = _guarded(c.dz, gpu)
        mean, std = _mean_std(c, gpu)
        rows = list(range(B))
        products = (narrow_products if kind == "narrow" and narrow_products else _products(kind))
        for np_ in (p for p in products if path != "u8_half" or p == 1):
            for aff in ((0, 1) if src == "rgb" else (None,)):
                folded = bool(aff) and mode != "raw"
                what = f"{path} {R.case_id(c)} Z={Z} products={np_} rgb_aff={aff}"
                with _Knobs(products=np_, rgb_aff=aff, **knobs):
                    r = _wgrad_checked(gpu, c, entry, st.args("idx"), rows, B, Z, dz, what, mean=mean, std=std,
                                       aff=folded, walks=C == 4)
                if not c.exact:
                    key = "fold" if folded else "decode" if src == "rgb" else path
                    print(f"kernel ratio wgrad {key} {R.case_id(c)} Z={Z}: {r:.3f}")


def test_wgrad_reduce_scales(gpu):
    """ppo_wgrad_reduce on the exact integer slabs of u8 rows: fl32(Σ s) for s = 1, s = 1/255
    and, accumulated onto an integer prefill, s = 0.5; the bias sums are unscaled."""
    B, Z = 7, 2
    c = R.make_case("wgrad", "u8", "narrow", 4, B)
    refs = R.wgrad_refs(c.op, c.src, c.kind, c.C, c.B, c.mode, tuple(range(B)))
    st = _Rows(c.rows, gpu)
    slab, slab_b = _run_wgrad(gpu, c, "u8", st.args("idx"), B, Z, _guarded(c.dz, gpu))
    g = torch.Generator().manual_seed(1)
    pre = (torch.randint(-50, 51, (32, 4, 8, 8), generator=g).double(), torch.randint(-50, 51, (32,), generator=g).double())
    for scale, acc in ((1.0, 0), (1.0 / 255.0, 0), (0.5, 1)):
        gw, gb = _reduce(gpu, c, Z, slab, slab_b, scale, acc, pre if acc else None)
        torch.cuda.synchronize()
        for o in (slab, slab_b, gw, gb):
            o.check(f"reduce scale {scale}")
        R.check_wgrad(c, refs, gw.t, gb.t[0], scale=scale, pre=pre if acc else None, what=f"reduce scale {scale}")


WIDE_P1 = [("fwd", "u8", "wide_w"), ("fwd", "f32", "wide_x"), ("fwd", "f32", "wide_w"), ("wgrad", "u8", "wide_x"),
           ("wgrad", "f32", "wide_x"), ("wgrad", "f32", "wide_w")]


@pytest.mark.parametrize("op,src,kind", WIDE_P1, ids=["-".join(p) for p in WIDE_P1])
def test_wide_cases_are_inexact_under_products_1(gpu, op, src, kind):
    """The wide cases reach the mid and lo planes of the kernels themselves: under
    `products` 1 (one bf16 product) the same launches must miss float64."""
    B = 5 if op == "fwd" else 7
    c = R.make_case(op, src, kind, 4, B)
    st = _Rows(c.rows, gpu)
    entry = {"u8": "u8", "f32": "f32x"}[src]
    scale = 1.0 / 255.0 if src == "u8" else 1.0
    with _Knobs(products=1, small_b=0):
        if op == "fwd":
            out, _ = _run_fwd(gpu, c, entry, st.args(), B, c.w.to(gpu), c.bias.to(gpu), False)
            torch.cuda.synchronize()
            out.check(R.case_id(c))
            with pytest.raises(AssertionError, match="differ|neither"):
                R.check_fwd(c, out.t)
        else:
            refs = R.wgrad_refs(c.op, c.src, c.kind, c.C, c.B, c.mode, tuple(range(B)))
            slab, slab_b = _run_wgrad(gpu, c, entry, st.args("idx"), B, 2, _guarded(c.dz, gpu))
            gw, gb = _reduce(gpu, c, 2, slab, slab_b, scale)
            torch.cuda.synchronize()
            for o in (slab, slab_b, gw, gb):
                o.check(R.case_id(c))
            with pytest.raises(AssertionError, match="differ"):
                R.check_wgrad(c, refs, gw.t, gb.t[0], scale=scale)


ROW_TABLE = [("u8_kw5", "u8", None, dict(conv1_wgrad=5, products=6)), ("u8_half", "u8", None, dict(products=1)),
             ("f32", "f32", None, {}), ("rgb_raw", "rgb", "raw", dict(rgb_aff=0))]


@pytest.mark.parametrize("name,src,mode,knobs", ROW_TABLE, ids=[r[0] for r in ROW_TABLE])
def test_wgrad_row_table_limit(gpu, name, src, mode, knobs):
    """The kernels that keep a row table of their block's images (conv1_wgrad_parts_kernel,
    conv1_wgrad_x6_kernel) hold 512 rows: (B, Z) = (512, 1) is accepted and exact, (513, 1)
    is refused with the limit in ppo_last_error() and leaves slab and bias partials
    untouched."""
    B = 512
    c = R.make_case("wgrad", src, "narrow", 4, B, mode)
    st = _Rows(c.rows, gpu)
    dz = _guarded(torch.cat([c.dz, c.dz[:1]]), gpu)     # a 513th dz image, never to be read
    mean, std = _mean_std(c, gpu)
    entry = {"u8": "u8", "f32": "f32x", "rgb": "rgb"}[src]
    with _Knobs(**knobs):
        _wgrad_checked(gpu, c, entry, st.args("idx"), range(B), B, 1, dz, f"{name} (512, 1)", mean=mean, std=std)
        slabs = (_Out(gpu, (1, 32, 256)), _Out(gpu, (1, 32)))
        with pytest.raises(_hip().HipError, match="512"):
            _run_wgrad(gpu, c, entry, st.args("row0=0"), B + 1, 1, dz, mean, std, slabs=slabs)
        torch.cuda.synchronize()
    for o in slabs:
        o.check(f"{name} (513, 1)")
        assert torch.isnan(o.t).all(), f"{name} (513, 1): the refused launch wrote its slab"


def test_wgrad_fold_workspace_regrows(gpu):
    """The affine fold's library-held per-stream workspace: Z = 7, then Z = 513 (beyond its
    first 512 blocks: freed and reallocated), then Z = 7 again on one stream, all correct."""
    B = 9
    c = R.make_case("wgrad", "rgb", "real", 4, B, "norm")
    st = _Rows(c.rows, gpu)
    dz = _guarded(c.dz, gpu)
    mean, std = _mean_std(c, gpu)
    with _Knobs(rgb_aff=1, products=6):
        for Z in (7, 513, 7):
            _wgrad_checked(gpu, c, "rgb", st.args("idx"), range(B), B, Z, dz, f"fold workspace Z={Z}", mean=mean, std=std,
                           aff=True)


# ------------------------------------------------------------------ row addressing
ADDR = [("u8_img", "u8", None, "narrow", 4, dict(conv1_fwd=0, conv1_wgrad=9)),
        ("u8_tile_kw10", "u8", None, "narrow", 4, dict(conv1_fwd=9, conv1_wgrad=10)),
        ("u8_kw8", "u8", None, "narrow", 4, dict(conv1_wgrad=8)),
        ("u8_kw5", "u8", None, "narrow", 4, dict(conv1_wgrad=5)),
        ("u8_half", "u8", None, "narrow", 4, dict(products=1)),
        ("u8_C3", "u8", None, "narrow", 3, {}),
        ("f32", "f32", None, "narrow", 4, {}),
        ("f32_C3", "f32", None, "narrow", 3, {}),
        ("rgb_decode", "rgb", "raw", "narrow", 4, dict(rgb_aff=0)),
        ("rgb_fold", "rgb", "norm", "real", 4, dict(rgb_aff=1))]
FORMS = {"idx": [11, 3, 16, 0, 7, 3, 9, 1, 15, 2, 14, 4, 13, 5, 12, 6, 10], "row0=0": None, "row0=5": None}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name,src,mode,kind,C,knobs", ADDR, ids=[a[0] for a in ADDR])
def test_row_addressing(gpu, name, src, mode, kind, C, knobs, form):
    """B = 17 through every path, forward (plain and mask form) and weight gradient: idx out
    of order with a repeated row, idx NULL with row0 = 0, idx NULL with row0 = 5 behind five
    guard rows."""
    B = R.ADDR_B
    rows = FORMS[form]
    assert rows is None or (len(rows) == B and len(set(rows)) == B - 1)
    entry = {"u8": "u8", "f32": "f32x" if C == 4 else "f32", "rgb": "rgb"}[src]
    folded = name == "rgb_fold"
    with _Knobs(small_b=0, **knobs):
        c = R.make_case("fwd", src, kind, C, B, mode)
        st = _Rows(c.rows, gpu)
        mean, std = _mean_std(c, gpu)
        w, bias = c.w.to(gpu), c.bias.to(gpu)
        _fwd_both(gpu, c, entry, st.args(form, rows), B, w, bias, f"{name} fwd {form}", mean, std, aff=folded, rows=rows)
        if name == "u8_img":
            _check_trunk(gpu, c, st.args(form, rows), B, w, bias, _trunk_weights(gpu), f"trunk {form}", rows=rows)
        c = R.make_case("wgrad", src, kind, C, B, mode)
        st = _Rows(c.rows, gpu)
        _wgrad_checked(gpu, c, entry, st.args(form, rows), rows or range(B), B, 5, _guarded(c.dz, gpu),
                       f"{name} wgrad {form}", mean=mean, std=std, aff=folded, walks=C == 4)


@pytest.mark.parametrize("src,mode", [("u8", None), ("f32", None), ("rgb", "raw")])
def test_rows_beyond_4gib(gpu, src, mode):
    """Rows gathered from one 4.4 GB allocation (uninitialised but for the gathered rows and
    their guard neighbours) at byte offsets below 2^31, between 2^31 and 2^32 and above
    2^32: forward and the default weight gradient, narrow case, B = 5."""
    B = 5
    cf, cw = (R.make_case(op, src, "narrow", 4, B, mode) for op in ("fwd", "wgrad"))
    row_bytes = cf.rows[0].numel() * cf.rows.element_size()
    total = 4_400_000_000 // row_bytes
    big = torch.empty((total,) + tuple(cf.rows.shape[1:]), dtype=cf.rows.dtype, device=gpu)
    at = [((1 << 32) + (1 << 25)) // row_bytes, (1 << 30) // row_bytes, (3 << 30) // row_bytes,
          (1 << 31) // row_bytes, total - 2]
    assert at[1] * row_bytes < 2 ** 31 <= at[2] * row_bytes < 2 ** 32 < at[0] * row_bytes
    assert at[3] * row_bytes < 2 ** 31 < (at[3] + 1) * row_bytes and (at[4] + 1) * row_bytes > 2 ** 32
    idx = torch.tensor(at, dtype=torch.int64, device=gpu)
    mean, std = _mean_std(cf, gpu)
    entry = {"u8": "u8", "f32": "f32x", "rgb": "rgb"}[src]
    for c in (cf, cw):
        for b, r in enumerate(at):
            big[r - 1] = big[r + 1] = NAN if src == "f32" else 255
        for b, r in enumerate(at):
            big[r].copy_(c.rows[b])
        addr = (big.data_ptr(), idx.data_ptr(), 0)
        what = f"{R.case_id(c)} rows beyond 2^32 bytes"
        with _Knobs(small_b=0):
            if c.op == "fwd":
                _fwd_both(gpu, c, entry, addr, B, c.w.to(gpu), c.bias.to(gpu), what, mean, std)
            else:
                _wgrad_checked(gpu, c, entry, addr, range(B), B, 2, _guarded(c.dz, gpu), what, mean=mean, std=std)


# ------------------------------------------------------------------ empty launches
def _untouched(outs, what):
    torch.cuda.synchronize()
    for o in outs:
        if o is not None:
            o.check(what)
            assert (torch.isnan(o.t) if o.t.dtype.is_floating_point else o.t == -1).all(), what + ": wrote"


def test_empty_launches_write_nothing(gpu):
    """B = 0 (and, for the weight gradients, Z = 0) returns 0 and writes nothing, for every
    entry point and every u8 weight-gradient kernel: a zero-row output lies directly in front
    of its trailing sentinel row, slabs keep their prefill."""
    tw = _trunk_weights(gpu)
    for src, mode, C in (("u8", None, 4), ("u8", None, 3), ("f32", None, 4), ("f32", None, 3), ("rgb", "raw", 4),
                         ("rgb", "norm", 4)):
        c = R.make_case("wgrad", src, "real" if mode == "norm" else "narrow", C, 2, mode)
        st = _Rows(c.rows, gpu)
        mean, std = _mean_std(c, gpu)
        w, bias = torch.ones(32, C, 8, 8, device=gpu), torch.ones(32, device=gpu)
        dz = _guarded(c.dz, gpu)
        entries = {"u8": ("u8",), "f32": ("f32", "f32x") if C == 4 else ("f32",), "rgb": ("rgb",)}[src]
        for entry in entries:
            what = f"{entry} C={C} {mode} empty launch"
            for masked in (False, True):
                _untouched(_run_fwd(gpu, c, entry, st.args(), 0, w, bias, masked, mean, std), what)
            for kw in (9, 10, 8, 5) if (src, C) == ("u8", 4) else (None,):
                for aff in (0, 1) if src == "rgb" else (None,):
                    for B, Z in ((0, 3), (2, 0), (0, 0)):
                        slabs = (_Out(gpu, (3, 32, C * 64)), _Out(gpu, (3, 32)))
                        with _Knobs(conv1_wgrad=kw, rgb_aff=aff):
                            _run_wgrad(gpu, c, entry, st.args(), B, Z, dz, mean, std, slabs=slabs)
                        _untouched(slabs, f"{what} wgrad B={B} Z={Z}")
        if (src, C) == ("u8", 4):
            for masked in (False, True):
                _untouched(_run_trunk(gpu, st.args(), 0, w, bias, tw, masked), "trunk empty launch")
