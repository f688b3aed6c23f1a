#!/usr/bin/env python3
"""Batch-1 evaluation act (GraphedActor and eager), for a rocprofv3 kernel-trace
of the per-kernel latency chain (bench.py eval_latency's workload).

  --u8           uint8 observations (CNN bases)
  --base NAME    cnn_rec (default: CNNBase + GRU, H = 256, 14 vector obs), cnn (H = 512),
                 mlp (MLPBase, 4 inputs, H = 64), mlp_rec (MLPBase + GRU, 7 inputs, H = 64)
  --sample       also time sampled acting: eager Policy.act(deterministic=False), a
                 GraphedActor(sample=True) through act() and replay(), and the
                 ppo_rng_advance launch on its own
  --rounds N     rounds of 100 synchronised acts per line (default 1); with N > 1 each
                 line prints min / median / max over the rounds
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ppo-dash_amd")]
import torch  # noqa: E402

from a2c_ppo_acktr.evaluation import GraphedActor  # noqa: E402
from a2c_ppo_acktr.model import CNNBase, MLPBase, Policy  # noqa: E402
from a2c_ppo_acktr.synthetic import Discrete  # noqa: E402


def _opt(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


dev = torch.device("cuda:0")
base = _opt("--base", "cnn_rec")
rounds = int(_opt("--rounds", "1"))
sample = "--sample" in sys.argv
cls, shape, recurrent, H, V = {"cnn_rec": (CNNBase, (4, 84, 84), True, 256, 14), "cnn": (CNNBase, (4, 84, 84), False, 512, 0),
                               "mlp": (MLPBase, (4,), False, 64, 0), "mlp_rec": (MLPBase, (5,), True, 64, 2)}[base]
torch.manual_seed(1)
pol = Policy(shape, Discrete(8), base=cls, base_kwargs={"recurrent": recurrent, "hidden_size": H}, vector_obs_len=V)
pol.to(dev)
u8 = "--u8" in sys.argv
obs = (torch.randint(0, 256, (1,) + shape, dtype=torch.uint8, device=dev) if u8 else torch.rand(1, *shape, device=dev))
vec, m = torch.rand(1, V, device=dev), torch.ones(1, 1, device=dev)
h0 = torch.zeros(1, pol.recurrent_hidden_state_size, device=dev)


def timed(name, step):
    """rounds x 100 acts, each synchronised by reading the action"""
    for _ in range(10):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(100):
            step().item()
        ms.append((time.perf_counter() - t0) * 10)
    ms.sort()
    if rounds == 1:
        print(name, ms[0], "ms per act", flush=True)
    else:
        print(name, f"min {ms[0]:.4f} median {ms[len(ms) // 2]:.4f} max {ms[-1]:.4f}", "ms per act", flush=True)


def through_act(fn):
    state = {"h": h0}

    def step():
        with torch.no_grad():
            _, a, _, state["h"] = fn(state["h"])
        return a
    return step


def through_replay(ga):
    ga.obs.copy_(obs)
    ga.vec.copy_(vec)
    return lambda: ga.replay()[1]


ga = GraphedActor(pol)
timed("eager", through_act(lambda h: pol.act(obs, vec, h, m, deterministic=True)))
timed("graph", through_act(lambda h: ga.act(obs, vec, h, m)))
timed("replay", through_replay(GraphedActor(pol, carry_hidden=True)))
if sample:
    from a2c_ppo_acktr._hip import call, stream
    gs = GraphedActor(pol, sample=True)
    timed("eager sampled", through_act(lambda h: pol.act(obs, vec, h, m, deterministic=False)))
    timed("graph sampled", through_act(lambda h: gs.act(obs, vec, h, m)))
    gr = GraphedActor(pol, carry_hidden=True, sample=True)
    timed("replay sampled", through_replay(gr))
    # the advance launch on its own: 100 launches back to back on the stream, one synchronisation
    word = torch.zeros(1, dtype=torch.int64, device=dev)
    for _ in range(max(rounds, 1)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(100):
            call("ppo_rng_advance", word.data_ptr(), 1, stream())
        torch.cuda.synchronize()
        print("rng_advance eager launch", (time.perf_counter() - t0) * 10, "ms per launch", flush=True)
