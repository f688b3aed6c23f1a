"""ppo_conv3_dgrad_bits on 16-image tiles (knob conv3_dgrad_group = 1, conv3.hip) against
the per-image kernel (knob 0): the two must agree bit for bit, torch.equal, on real-valued
dz3 and random mask bits under products 1, 6 and 9.  B = 15 falls back to the per-image
kernel; 16, 32: whole groups; 17, 31, 33: ragged last groups of 1 and of 15 images;
16 C + 21: a second group for the first blocks of the persistent grid and a ragged last
group of 5.  One narrow integer case (B = 17) is compared with float64, no tolerance.

Guards and sentinels as in test_conv_gpu.py: inputs between NaN / all-ones images, outputs
prefilled with NaN between sentinel rows."""
import pytest
import torch

from helpers import conv_ref as R
from test_conv_gpu import _Knobs, _Out, _cus, _guarded, _pack_weights, _run_dgrad

pytestmark = pytest.mark.gpu

GROUP_B = (15, 16, 17, 31, 32, 33, "16C+21")


def _resolve(B, n_cu):
    return 16 * n_cu + 21 if B == "16C+21" else B


@pytest.mark.parametrize("B", GROUP_B, ids=[f"B{B}" for B in GROUP_B])
def test_group_equals_per_image(gpu, B):
    B = _resolve(B, _cus(gpu))
    g = torch.Generator(device=gpu).manual_seed(4099 + B)
    w = torch.randn(32, 64, 3, 3, device=gpu, generator=g) * 0.05
    keep, _, wd = _pack_weights(gpu, 3, w)
    dz = _guarded(torch.randn(B, 7, 7, 32, device=gpu, generator=g), gpu)
    mbits = _guarded(torch.randint(-2 ** 63, 2 ** 63 - 1, (B, 81), dtype=torch.int64, device=gpu, generator=g), gpu)
    for products in (1, 6, 9):
        what = f"conv3 dgrad bits B={B} products={products}"
        outs = []
        for group in (0, 1):
            with _Knobs(products=products, conv3_dgrad_group=group):
                outs.append(_run_dgrad(gpu, 3, B, dz, wd, mbits, True))
        torch.cuda.synchronize()
        for o, group in zip(outs, (0, 1)):
            o.check(f"{what} group={group}")
            assert not torch.isnan(o.t).any(), f"{what} group={group}: output elements left unwritten"
        assert outs[0].t.abs().max() > 0, what + ": a zero result compares nothing"
        same = torch.equal(outs[0].t, outs[1].t)
        if not same:
            bad = (outs[0].t != outs[1].t).nonzero()
            raise AssertionError(f"{what}: {len(bad)} elements differ between the group and the per-image kernel, "
                                 f"first at {bad[0].tolist()}")


def test_group_vs_float64(gpu):
    B = 17
    c = R.make_case(3, "dgrad", "narrow", B)
    keep, _, wd = _pack_weights(gpu, 3, c.w)
    dz = _guarded(c.dz, gpu)
    mbits = _guarded(R.PACK["u64"](c.m > 0), gpu)
    for products in (1, 6, 9):
        what = f"{R.case_id(c)} products={products} group kernel"
        with _Knobs(products=products, conv3_dgrad_group=1):
            out = _run_dgrad(gpu, 3, B, dz, wd, mbits, True)
            torch.cuda.synchronize()
        out.check(what)
        R.compare(out.t, c.ref, exact=True, what=what)
