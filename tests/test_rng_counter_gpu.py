"""The sampling counter as a word in device memory, through the C ABI: for each of the
three heads families the _dc entry point with the word set to c equals the by-value
entry point with counter = c bit for bit (value, action, log-prob, entropy), across
the counters where a 32-bit slip would show, the batch sizes on both sides of
launch_act's two-rows-per-wave threshold, the HC x AMAX x FAST instantiations, with
and without separate critic features; the kernels never write the word (it sits
between guard words); ppo_rng_advance adds with 64-bit wrap-around."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")
SEED = 0x9E3779B97F4A7C15
COUNTERS = (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1)
BATCHES = (1, 5, 300, 4097)   # 4097: the first size with two rows per wave in launch_act
GUARD_LO, GUARD_HI = 0x5A5A5A5A5A5A5A5A, 0x3C3C3C3C3C3C3C3C
CAT_SHAPES = ((64, 8), (64, 6), (96, 12), (512, 16))   # (64, 8) and (512, 16): FAST without feat_v
FLOAT_SHAPES = ((64, 1), (64, 8), (64, 16))            # A = 1, one in between (FAST at AMAX 8), the maximum


def _hip():
    from a2c_ppo_acktr import _hip
    return _hip


def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(x):
    return None if x is None else x.data_ptr()


def _i64(c):
    """the 64 bits of c as the int64 a torch tensor holds"""
    c &= 2 ** 64 - 1
    return c - 2 ** 64 if c >> 63 else c


class _Word:
    """one counter word between two guard words"""

    def __init__(self, gpu, c=0):
        self.buf = torch.tensor([GUARD_LO, _i64(c), GUARD_HI], dtype=torch.int64, device=gpu)
        self.ptr = self.buf.data_ptr() + 8

    def set(self, c):
        self.buf[1] = _i64(c)

    def check(self, c):
        assert self.buf.tolist() == [GUARD_LO, _i64(c), GUARD_HI]


_INPUTS = {}


def _inputs(gpu, H, A, N, flat=False):
    """features, critic features and head parameters (made once per shape, never changed);
    flat: zero actor weights, a near-uniform policy"""
    key = (H, A, N, flat)
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(1000 * H + 10 * A + N)
        r = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
        t = {"feat": r(N, H), "feat_v": r(N, H), "wc": r(H) / H ** 0.5, "bc": r(1),
             "wa": r(A, H) * (0.0 if flat else 1.0 / H ** 0.5), "ba": r(A) * (0.01 if flat else 0.3),
             "logstd": r(A) * 0.3, "noise": torch.rand(N, A, generator=g) + 0.05}
        _INPUTS[key] = {k: v.to(gpu).contiguous() for k, v in t.items()}
    return _INPUTS[key]


def _act(family, dc, t, N, H, A, counter, sep_v, noise=False):
    """one act call -> (value, action, log-prob, entropy); outputs prefilled with NaN / -1"""
    gpu = t["feat"].device
    val, lp, ent = (torch.full((N,), NAN, device=gpu) for _ in range(3))
    if family == "cat":
        act = torch.full((N,), -1, dtype=torch.int64, device=gpu)
    else:
        act = torch.full((N, A), NAN, device=gpu)
    head = [_p(t["feat"]), _p(t["feat_v"]) if sep_v else None, N, H, _p(t["wc"]), _p(t["bc"]), _p(t["wa"]),
            _p(t["ba"])]
    if family == "gauss":
        head.append(_p(t["logstd"]))
    name = {"cat": "ppo_heads_act", "gauss": "ppo_heads_gauss_act", "bern": "ppo_heads_bern_act"}[family]
    _hip().call(name + ("_dc" if dc else ""), *head, A, _p(t["noise"]) if noise else None, SEED, counter, 0, None,
                _p(val), _p(act), _p(lp), _p(ent), _s())
    return val, act, lp, ent


CASES = ([("cat", H, A) for H, A in CAT_SHAPES] + [("gauss", H, A) for H, A in FLOAT_SHAPES]
         + [("bern", H, A) for H, A in FLOAT_SHAPES])


@pytest.mark.parametrize("sep_v", [False, True], ids=["shared", "feat_v"])
@pytest.mark.parametrize("N", BATCHES)
@pytest.mark.parametrize("family,H,A", CASES, ids=[f"{f}-H{H}-A{A}" for f, H, A in CASES])
def test_device_counter_equals_by_value(gpu, family, H, A, N, sep_v):
    t = _inputs(gpu, H, A, N)
    w = _Word(gpu)
    seen = []
    for c in COUNTERS:
        w.set(c)
        ref = _act(family, False, t, N, H, A, c, sep_v)
        got = _act(family, True, t, N, H, A, w.ptr, sep_v)
        w.check(c)   # the kernel never writes the word or its neighbours
        for name, a, b in zip(("value", "action", "logp", "entropy"), ref, got):
            assert torch.equal(a, b), (name, c)
        seen.append(got[1].clone())
    if N * A >= 300:   # and the counter is used: 2^32 - 1 and 2^32 do not alias 0 or each other
        assert not torch.equal(seen[0], seen[2]) and not torch.equal(seen[2], seen[3])
        assert not torch.equal(seen[0], seen[3])


@pytest.mark.parametrize("family,H,A", [("cat", 96, 12), ("gauss", 64, 8), ("bern", 64, 16)])
def test_host_noise_leaves_the_word_unused(gpu, family, H, A):
    """noise given: the word is not used (two values, one result) but is still read through a
    valid pointer, and the result is the by-value call's"""
    N = 300
    t = _inputs(gpu, H, A, N)
    w = _Word(gpu, 7)
    ref = _act(family, False, t, N, H, A, 7, False, noise=True)
    got = _act(family, True, t, N, H, A, w.ptr, False, noise=True)
    w.check(7)
    w.set(2 ** 40 + 3)
    other = _act(family, True, t, N, H, A, w.ptr, False, noise=True)
    w.check(2 ** 40 + 3)
    for a, b, c in zip(ref, got, other):
        assert torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize("family,A", [("cat", 8), ("gauss", 3), ("bern", 5)])
def test_two_counters_sample_differently(gpu, family, A):
    N, H = 300, 64
    t = _inputs(gpu, H, A, N, flat=True)
    w = _Word(gpu, 11)
    a = _act(family, True, t, N, H, A, w.ptr, False)
    w.set(12)
    b = _act(family, True, t, N, H, A, w.ptr, False)
    w.check(12)
    assert torch.equal(a[0], b[0])             # the value does not depend on the counter
    differ = (a[1] != b[1]).reshape(N, -1).any(1).float().mean().item()
    print(f"rows whose action differs between counters 11 and 12: {differ:.2f}")
    # near-uniform over 8 actions / 2^5 patterns / a continuum: independent draws differ in
    # >= 7/8 of the rows in expectation; one quarter is > 30 sigma below that at N = 300
    assert differ > 0.25


@pytest.mark.parametrize("c,by", [(2 ** 32 - 1, 1), (5, 2 ** 33), (2 ** 64 - 1, 1), (0, 0), (2 ** 63, 2 ** 63)])
def test_rng_advance(gpu, c, by):
    w = _Word(gpu, c)
    _hip().call("ppo_rng_advance", w.ptr, by, _s())
    w.check((c + by) % 2 ** 64)


def test_rng_advances_compose_on_one_stream(gpu):
    w = _Word(gpu, 2 ** 64 - 2)
    for by in (1, 1, 2 ** 32):
        _hip().call("ppo_rng_advance", w.ptr, by, _s())
    w.check(2 ** 32)
    # the hand-off a captured graph makes: act reads c, the advance follows it on the stream
    t = _inputs(gpu, 64, 8, 300)
    first = _act("cat", True, t, 300, 64, 8, w.ptr, False)
    _hip().call("ppo_rng_advance", w.ptr, 1, _s())
    second = _act("cat", True, t, 300, 64, 8, w.ptr, False)
    w.check(2 ** 32 + 1)
    for c, got in ((2 ** 32, first), (2 ** 32 + 1, second)):
        for a, b in zip(_act("cat", False, t, 300, 64, 8, c, False), got):
            assert torch.equal(a, b), c
