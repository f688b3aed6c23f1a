"""CPU checks of tests/helpers/cat_ref.py: the float64 Categorical loss head equals
torch float64 autograd of the reference's loss, every case of tests/test_heads_gpu.py
meets its input margins, and the comparison used on the GPU accepts the fp32
yardstick (torch CPU fp32 autograd of the same loss) and rejects planted errors —
shown by handing it the yardstick computed from a deliberately wrong loss in the
kernel's place."""
import numpy as np
import pytest
import torch

from helpers import cat_ref as C

IDS = [C.case_id(c) for c in C.CASES]


@pytest.mark.parametrize("A", [1, 3, 16])
@pytest.mark.parametrize("use_clipped", [True, False])
def test_float64_helper_equals_autograd(A, use_clipped):
    """cat_loss_head_grads / cat_logp_entropy == torch float64 autograd of the
    reference's loss (algo/ppo.py:61-81 with FixedCategorical) to 1e-12 relative, on a
    batch holding rows with a clipped ratio, rows inside the range, a ratio of exactly
    1, and rows on both sides of the value clip."""
    B, clip, vc, ec = 64, 0.1, 0.5, 0.01
    g = np.random.default_rng(7 + A)
    value, logits = g.normal(size=B), g.normal(size=(B, A)) * 2
    actions = g.integers(0, A, B)
    lp, ent = C.cat_logp_entropy(logits, actions)
    old_logp = lp + g.normal(size=B) * 0.15
    old_logp[:3] = lp[:3]
    adv, ret = g.normal(size=B), g.normal(size=B)
    vpred = value + g.normal(size=B) * 0.2
    r = C.cat_loss_head_grads(value, logits, actions, old_logp, adv, vpred, ret, clip, vc, ec, use_clipped)
    ratio = np.exp(lp - old_logp)
    out = (ratio < 1 - clip) | (ratio > 1 + clip)
    far = np.abs(value - vpred) > clip
    assert out.sum() >= 5 and (~out).sum() >= 5 and far.sum() >= 5 and (~far).sum() >= 5
    t = lambda x: torch.tensor(x, dtype=torch.float64)  # noqa: E731
    v, z = t(value).requires_grad_(), t(logits).requires_grad_()
    total, vl, al, e, logp = C.torch_loss(v, z, torch.from_numpy(actions), t(old_logp), t(adv), t(vpred), t(ret),
                                          clip, vc, ec, use_clipped)
    total.backward()
    for got, ref in ((r["value_loss"], vl), (r["action_loss"], al), (r["entropy"], e), (r["logp"], logp), (lp, logp),
                     (ent.mean(), e), (r["g_value"], v.grad), (r["g_logits"], z.grad)):
        ref = ref.detach().numpy()
        assert np.abs(np.asarray(got) - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1e-3)
    if A == 1:
        assert not r["g_logits"].any() and not ent.any() and not lp.any()


@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_cases_meet_their_margins(case):
    """Every row of every case is at least MARGIN from each branch point its tests
    depend on, within MAX_SEEDS seeds; logits stay within the softmax's easy range."""
    c = C.build_case(*case)
    H, A, B = case[:3]
    print(f"seed {c['seed']} (start {1000 * H + 10 * A + B}, {c['seeds_tried']} tried), margins {c['margins']}, "
          f"torch fp32 log-prob error {c['torch_fp32_err']:.2e}")
    want = {"ratio"} | ({"vclip", "vmax"} if case[6] else set()) | ({"sample", "mode"} if A >= 2 else set())
    assert set(c["margins"]) == want
    assert all(v >= C.MARGIN for v in c["margins"].values())
    assert c["seeds_tried"] <= C.MAX_SEEDS and c["zmax"] < 8.0 and c["torch_fp32_err"] < 5e-6
    assert c["actions"][c["sr"]].min() >= 0 and c["actions"][c["sr"]].max() < A
    assert len(set(c["sr"].tolist())) == B and c["sr"].max() < c["R"]
    if B >= 37:
        assert len(set(c["actions"][c["sr"]].tolist())) == A   # every action occurs


@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_comparison_accepts_the_yardstick(case):
    c = C.build_case(*case)
    y = C.torch_head_grads(c)
    C.check_grads(y, c["ref"])
    C.check_losses(y["losses"], c["ref"]["losses"])
    # and float64 autograd from the features down agrees with the reference itself
    y64 = C.torch_head_grads(c, dtype=torch.float64)
    for k in C.GRAD_NAMES:
        if c["ref"][k] is not None:
            assert np.abs(y64[k] - c["ref"][k]).max() <= 1e-12 * max(np.abs(c["ref"][k]).max(), 1e-3), k


@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_comparison_rejects_planted_errors(case):
    """The fp32 yardstick computed from a wrong loss: the entropy term dropped from
    the logit gradient, the other value-loss branch, and g_wa's last two rows
    exchanged.  At A = 1 the entropy gradient is identically 0 and g_wa has one row,
    so the first and third do not exist there."""
    c = C.build_case(*case)
    A = case[1]
    ref = c["ref"]
    if A >= 2:
        with pytest.raises(AssertionError):
            C.check_grads(C.torch_head_grads(c, ec=0.0), ref)
        y = C.torch_head_grads(c)
        y["g_wa"] = y["g_wa"][list(range(A - 2)) + [A - 1, A - 2]]
        with pytest.raises(AssertionError):
            C.check_grads(y, ref)
    swapped = C.torch_head_grads(c, use_clipped=not c["use_clipped"])
    with pytest.raises(AssertionError):
        C.check_grads(swapped, ref)
    with pytest.raises(AssertionError):
        C.check_losses(swapped["losses"], ref["losses"])


def test_comparison_rejects_nan_and_shape():
    c = C.build_case(*C.CASES[1])
    y = C.torch_head_grads(c)
    y["g_ba"] = y["g_ba"].copy()
    y["g_ba"][-1] = np.nan
    with pytest.raises(AssertionError):
        C.check_grads(y, c["ref"])
