"""Cost of one A2C update against one PPO pass over the same rows: CNNBase (hidden 512,
Discrete(8)), 4096 envs x 5 steps of u8 frames, A2C_ACKTR.update against
PPO(ppo_epoch=1, num_mini_batch=1).update on the same storage, same process, alternating.
A2C runs PPO's kernels once, without the advantage normalisation pass and with an optimizer
that touches three arrays instead of four, so it should not be slower (the project's A/B
bar is 2 %).  Prints the median time of each and env-steps/s of the
update alone (no rollout).

    python tools/a2c_probe.py [--envs 4096] [--steps 5] [--rounds 10]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ppo-dash_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    from a2c_ppo_acktr import model as M
    from a2c_ppo_acktr.algo import A2C_ACKTR, PPO
    from a2c_ppo_acktr.storage import RolloutStorage
    from a2c_ppo_acktr.synthetic import Discrete
    dev = torch.device("cuda:0")
    T, N, A = a.steps, a.envs, 8
    torch.manual_seed(0)
    pol = M.Policy((4, 84, 84), Discrete(A), base=M.CNNBase, base_kwargs={"recurrent": False, "hidden_size": a.hidden})
    pol.to(dev)
    # lr 0: both optimizers run their full step and leave the shared policy where it is
    agents = {"a2c": A2C_ACKTR(pol, 0.5, 0.01, lr=0.0, eps=1e-5, alpha=0.99, max_grad_norm=0.5),
              "ppo_1x1": PPO(pol, 0.1, 1, 1, 0.5, 0.01, lr=0.0, eps=1e-5, max_grad_norm=0.5)}
    st = RolloutStorage(T, N, (4, 84, 84), [0], Discrete(A), 1, obs_dtype=torch.uint8, device=dev)
    g = torch.Generator(device=dev).manual_seed(1)
    st.obs.copy_(torch.randint(0, 256, st.obs.shape, dtype=torch.uint8, device=dev, generator=g))
    st.actions.copy_(torch.randint(0, A, st.actions.shape, device=dev, generator=g))
    st.action_log_probs.copy_(torch.log(torch.rand(st.action_log_probs.shape, device=dev, generator=g)) * 0.1 - 2.0)
    st.value_preds.copy_(torch.randn(st.value_preds.shape, device=dev, generator=g) * 0.1)
    st.rewards.copy_(torch.randn(st.rewards.shape, device=dev, generator=g))
    st.compute_returns(torch.zeros(N, 1, device=dev), True, 0.99, 0.95, False)
    times = {k: [] for k in agents}
    for r in range(a.warmup + a.rounds):
        for name, agent in agents.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            losses = agent.update(st)
            torch.cuda.synchronize()
            if r >= a.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
            assert all(np.isfinite(losses)), (name, losses)
    med = {k: float(np.median(v)) for k, v in times.items()}
    for k, v in times.items():
        print("%-8s ms per update %s median %.3f spread %.3f  env-steps/s %.0f" % (
            k, [round(x, 3) for x in v], med[k], max(v) - min(v), T * N / (med[k] * 1e-3)))
    print("a2c / ppo_1x1 = %.4f" % (med["a2c"] / med["ppo_1x1"]))


if __name__ == "__main__":
    main()
