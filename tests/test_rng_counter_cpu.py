"""The device-memory RNG counter's C ABI without a GPU: the three _dc act entry points
and ppo_rng_advance are declared, exported and bound, the ABI version is unchanged,
and each refuses a NULL counter before it touches the device."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ppo_hip.h")

# name -> the by-value sibling whose argument list it shares (None: no sibling)
SYMBOLS = {"ppo_heads_act_dc": "ppo_heads_act", "ppo_heads_gauss_act_dc": "ppo_heads_gauss_act",
           "ppo_heads_bern_act_dc": "ppo_heads_bern_act", "ppo_rng_advance": None}


def _decl(src, name):
    m = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)", src, re.M)
    assert m, name + " is not declared in include/ppo_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_symbols_declared_exported_and_bound():
    from a2c_ppo_acktr import _hip
    src = open(HEADER).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _hip.LIB_PATH], capture_output=True, text=True, check=True)
    exported = {ln.split()[-1] for ln in out.stdout.splitlines() if ln.strip()}
    for name, sibling in SYMBOLS.items():
        args = _decl(src, name)
        assert name in exported, name + " is not exported by libppo_hip.so"
        assert len(args) == len(_hip.SIGNATURES[name]), name
        assert hasattr(_hip.lib(), name) and getattr(_hip.lib(), name).argtypes == _hip.SIGNATURES[name]
        if sibling is None:
            continue
        # the sibling's arguments, `unsigned long long counter` replaced by a pointer to the word
        want = ["const unsigned long long* counter" if a == "unsigned long long counter" else a
                for a in _decl(src, sibling)]
        assert args == want, name
        sig = list(_hip.SIGNATURES[sibling])
        k = _decl(src, sibling).index("unsigned long long counter")
        assert sig[k] is _hip.c_ull
        sig[k] = _hip.c_p
        assert _hip.SIGNATURES[name] == sig, name
    assert _decl(src, "ppo_rng_advance") == ["unsigned long long* counter", "unsigned long long by", "void* stream"]
    assert _hip.SIGNATURES["ppo_rng_advance"] == [_hip.c_p, _hip.c_ull, _hip.c_p]


def test_abi_version_unchanged():
    from a2c_ppo_acktr import _hip
    assert _hip.call("ppo_abi_version") == 3   # symbols were only added


def _null_counter_args(name):
    """valid sizes, every pointer NULL (the counter among them): only the argument checks may run"""
    from a2c_ppo_acktr import _hip
    if name == "ppo_rng_advance":
        return [None, 1, None]
    args = []
    for i, t in enumerate(_hip.SIGNATURES[name]):
        args.append(None if t is _hip.c_p else 0)
    src = open(HEADER).read()
    names = [a.split()[-1].lstrip("*") for a in _decl(src, name)]
    for k, v in (("N", 4), ("H", 64), ("A", 3)):
        args[names.index(k)] = v
    assert args[names.index("counter")] is None
    return args


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_null_counter_is_refused_without_a_device(name):
    """PPO_EARG (1001) and a message naming the function, from the check that precedes every
    HIP call: this runs where no device exists"""
    from a2c_ppo_acktr import _hip
    fn = getattr(_hip.lib(), name)
    rc = fn(*_null_counter_args(name))
    assert rc == 1001, (name, rc)
    msg = _hip.lib().ppo_last_error().decode()
    assert name in msg and "counter" in msg and "NULL" in msg, msg
    with pytest.raises(_hip.HipError, match=name):
        _hip.call(name, *_null_counter_args(name))
