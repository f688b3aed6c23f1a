"""The A2C row loss in the six heads train kernels (ppo_heads_train_a2c,
ppo_heads_gauss_train_a2c, ppo_heads_bern_train_a2c + their reduces) through the C ABI
against float64 (tests/helpers/a2c_ref.py), at the smallest shapes that reach each code
path: generic / FAST / LDS-weight kernels, AMAX 8 / 16, partial and empty waves, a second
block, gathered rows and row0 offsets, separate critic features.  The storage planes passed
hold only actions and returns (the entry points take nothing else); output buffers are
prefilled with NaN.  Bounds: cat_ref.check_grads (1e-5 of the tensor's largest entry) and
check_losses (rtol 2e-5, atol 1e-6), as for the PPO kernels."""
import numpy as np
import pytest
import torch

from helpers import a2c_ref as R

pytestmark = pytest.mark.gpu

VC, EC = R.VC, R.EC
NAN = float("nan")

# H, A, B, rows, separate critic features, feat_act
CAT = [
    (64, 1, 1, 0, False, 0),          # single row; A = 1
    (64, 3, 37, "idx", False, 1),     # generic, partial wave, empty waves
    (64, 8, 129, 5, False, 1),        # FAST HC = 1 (its own A2C instantiation), second block, row0
    (128, 6, 37, "idx", True, 2),     # dfeat_v
    (256, 5, 37, "idx", True, 2),     # generic HC = 4 (its own A2C instantiation)
    (512, 6, 37, "idx", False, 1),    # generic HC = 8 (its own A2C instantiation)
    (512, 8, 130, "idx", False, 1),   # LDS-weight kernel / register kernel
    (512, 16, 300, 11, False, 0),     # AMAX = 16 FAST
]
GAUSS = [
    (64, 3, 37, "idx", False, 1),     # generic HC = 1 (its own A2C instantiation)
    (64, 8, 129, 5, False, 1),        # FAST
    (128, 6, 37, "idx", True, 2),     # separate critic features
    (512, 8, 130, "idx", False, 1),   # LDS-weight kernel
]
BERN = [
    (64, 3, 37, "idx", False, 1),
    (64, 8, 129, 5, False, 1),
    (128, 6, 37, "idx", True, 2),
    (256, 8, 130, "idx", False, 0),   # FAST HC = 4 (its own A2C instantiation)
    (512, 8, 130, "idx", False, 1),
]
ALL = [("cat",) + c for c in CAT] + [("gauss",) + c for c in GAUSS] + [("bern",) + c for c in BERN]
TRAIN = {"cat": "ppo_heads_train_a2c", "gauss": "ppo_heads_gauss_train_a2c", "bern": "ppo_heads_bern_train_a2c"}


def _id(case):
    return "-".join(str(int(x) if isinstance(x, bool) else x) for x in case)


def _hip():
    from a2c_ppo_acktr import _hip
    return _hip


def _s():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(x):
    return None if x is None else x.data_ptr()


class _Knob:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.keep = _hip().call("ppo_tune_get", self.name)
        if self.value is not None:
            _hip().call("ppo_tune_set", self.name, self.value)

    def __exit__(self, *exc):
        _hip().call("ppo_tune_set", self.name, self.keep)


def _run(gpu, c, lds=None, actions=None):
    """train_a2c + reduce of case c -> (raw outputs, gradients, loss_acc)"""
    Hh = _hip()
    kind, H, A, B, rows, sep_v = c["kind"], c["H"], c["A"], c["B"], c["rows"], c["sep_v"]
    gauss = kind == "gauss"
    t = {k: _dev(c[k]) for k in ("feat", "wc", "bc", "wa", "ba", "ret")}
    t["actions"] = _dev(c["actions"] if actions is None else actions)
    ls = _dev(c["logstd"]) if gauss else None
    fv = _dev(c["feat_v"]) if sep_v else None
    idx = _dev(c["sr"]) if rows == "idx" else None
    nblk = Hh.call("ppo_heads_train_blocks", B)
    nb = 1 + (2 * A if gauss else A)
    out = {"dfeat": torch.full((B, H), NAN, device=gpu),
           "dfeat_v": torch.full((B, H), NAN, device=gpu) if sep_v else None,
           "part_w": torch.full((nblk * (1 + A) * H,), NAN, device=gpu),
           "part_b": torch.full((nblk * nb,), NAN, device=gpu),
           "part_l": torch.full((nblk * 4,), NAN, device=gpu)}
    with _Knob(b"heads_lds", lds):
        Hh.call(TRAIN[kind], _p(t["feat"]), _p(fv), B, H, _p(t["wc"]), _p(t["bc"]), _p(t["wa"]), _p(t["ba"]),
                *((_p(ls),) if gauss else ()), A, _p(idx), 0 if rows == "idx" else rows, _p(t["actions"]),
                _p(t["ret"]), VC, EC, 1.0 / B, c["feat_act"], _p(out["dfeat"]), _p(out["dfeat_v"]),
                _p(out["part_w"]), _p(out["part_b"]), _p(out["part_l"]), _s())
    torch.cuda.synchronize()
    g = {"g_wc": torch.full((H,), NAN, device=gpu), "g_bc": torch.full((1,), NAN, device=gpu),
         "g_wa": torch.full((A, H), NAN, device=gpu), "g_ba": torch.full((A,), NAN, device=gpu),
         "g_logstd": torch.full((A,), NAN, device=gpu) if gauss else None}
    acc = torch.zeros(4, dtype=torch.float64, device=gpu)
    if gauss:
        Hh.call("ppo_heads_gauss_reduce", _p(out["part_w"]), _p(out["part_b"]), _p(out["part_l"]), nblk, H, A,
                _p(g["g_wc"]), _p(g["g_bc"]), _p(g["g_wa"]), _p(g["g_ba"]), _p(g["g_logstd"]), _p(acc), 1.0 / B, 1.0,
                _s())
    else:
        Hh.call("ppo_heads_reduce", _p(out["part_w"]), _p(out["part_b"]), _p(out["part_l"]), nblk, H, A,
                _p(g["g_wc"]), _p(g["g_bc"]), _p(g["g_wa"]), _p(g["g_ba"]), _p(acc), 1.0 / B, 1.0, 0, _s())
    torch.cuda.synchronize()
    g["dfeat"], g["dfeat_v"] = out["dfeat"], out["dfeat_v"]
    return out, g, acc.cpu().numpy()


@pytest.mark.parametrize("case", ALL, ids=[_id(c) for c in ALL])
def test_a2c_train_kernel_vs_float64(gpu, case):
    """train_a2c + reduce: dfeat, dfeat_v, the head gradients (and g_logstd for Box) vs the
    float64 closed form, max |err| <= 1e-5 * max(max|ref|, 1e-3) per tensor; losses rtol
    2e-5, atol 1e-6 (slot 0 stores 2 (R - v)^2, so the reduce's 0.5 gives mean((R - v)^2));
    no bad action counted; no NaN left in any partial; a second launch is bit-identical."""
    c = R.build_case(*case)
    out, g, acc = _run(gpu, c)
    out2, _, _ = _run(gpu, c)
    for k in ("part_w", "part_b", "part_l", "dfeat"):
        assert not torch.isnan(out[k]).any(), k
        assert torch.equal(out[k], out2[k]), k
    assert float(out["part_l"].view(-1, 4)[:, 3].sum()) == 0.0 and acc[3] == 0.0
    R.check_grads(g, c["ref"])
    print("losses", acc[:3], "ref", c["ref"]["losses"])
    R.check_losses(acc, c["ref"]["losses"])


LDS = [("cat", 512, 8, 130, "idx", False, 1), ("gauss", 512, 8, 130, "idx", False, 1),
       ("bern", 512, 8, 130, "idx", False, 1)]


@pytest.mark.parametrize("case", LDS, ids=[c[0] for c in LDS])
def test_a2c_lds_and_register_kernels_agree(gpu, case):
    """(512, 8) through the LDS-weight kernel (heads_lds 1) and the register kernel (0):
    both meet the float64 bounds, and they differ from each other by no more than the
    bound either must meet against float64."""
    c = R.build_case(*case)
    got = {}
    for lds in (1, 0):
        out, g, acc = _run(gpu, c, lds=lds)
        print("heads_lds", lds)
        R.check_grads(g, c["ref"])
        R.check_losses(acc, c["ref"]["losses"])
        got[lds] = g
    for k, r in c["ref"].items():
        if k == "losses" or r is None:
            continue
        d = float((got[1][k].double() - got[0][k].double()).abs().max())
        assert d <= R.C.grad_bound(r), (k, d)


def _bad_rows(c, at, values):
    acts = c["actions"].copy()
    for row, v in zip(at, values):
        if c["kind"] == "cat":
            acts[c["sr"][row]] = v
        else:
            acts[c["sr"][row], 1] = v
    return acts


BAD = [(("cat", 64, 3, 37, "idx", False, 1), [-1, 3, 2 ** 32 + 1]),
       (("cat", 512, 8, 130, "idx", False, 1), [-1, 8, 2 ** 32 + 1]),
       (("gauss", 64, 3, 37, "idx", False, 1), [float("nan"), float("inf"), float("-inf")]),
       (("bern", 64, 3, 37, "idx", False, 1), [0.5, 2.0, float("nan")])]


@pytest.mark.parametrize("case,values", BAD, ids=["cat-generic", "cat-lds", "gauss", "bern"])
def test_a2c_bad_actions_are_counted(gpu, case, values):
    """A stored action outside [0, A) (Discrete), non-finite (Box) or not in {0, 1}
    (MultiBinary) on three rows of the first block (rows 0, 7, 19): part_loss slot 3 and
    loss_acc[3] count exactly 3; dfeat of every other row stays finite, and so do the
    partials of every other block (B = 130 has a second one)."""
    c = R.build_case(*case)
    at = [0, 7, 19]
    out, g, acc = _run(gpu, c, actions=_bad_rows(c, at, values))
    assert float(out["part_l"].view(-1, 4)[:, 3].sum()) == 3.0 and acc[3] == 3.0
    keep = np.setdiff1d(np.arange(c["B"]), at)
    assert torch.isfinite(out["dfeat"][torch.from_numpy(keep).cuda()]).all()
    nblk = out["part_l"].numel() // 4
    if nblk > 1:
        for k in ("part_w", "part_b", "part_l"):
            assert torch.isfinite(out[k].view(nblk, -1)[1:]).all(), k
