"""A2C on CartPole in float64 on the CPU: the restated update of tests/helpers/a2c_ref.py
(autograd of algo/a2c_acktr.py:45-51, 71-72, clip_grad_norm_, torch.optim.RMSprop) on the
oracle's CartPole, with the reference's A2C defaults (T = 5, lr 7e-4, eps 1e-5, alpha 0.99,
gamma 0.99, no GAE, value_loss_coef 0.5, entropy_coef 0.01, max_grad_norm 0.5).  Prints the
mean length of the episodes that finished in each tenth of the run: the curve
tests/test_a2c_update_gpu.py::test_a2c_learns_cartpole's N and update count were chosen from.

    python tools/a2c_cartpole_ref.py --envs 32 --updates 1000
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ppo-dash_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from helpers import a2c_ref as R  # noqa: E402
from oracle import ppo_oracle as O  # noqa: E402


def run(N, updates, seed=0, T=5, lr=7e-4, eps=1e-5, alpha=0.99, gamma=0.99, vc=0.5, ec=0.01, max_norm=0.5):
    from a2c_ppo_acktr import model as M
    from a2c_ppo_acktr.synthetic import Discrete
    torch.manual_seed(seed)
    pol = M.Policy((4,), Discrete(2), base=M.MLPBase, base_kwargs={"recurrent": False})
    P = [p.detach().double().clone().requires_grad_() for p in pol.parameters()]
    opt = torch.optim.RMSprop(P, lr, eps=eps, alpha=alpha)
    state, steps, obs, *_ = O.cartpole_step(np.zeros((N, 4), np.float32), np.zeros(N, np.int32), None, 3, 0)
    counter, lengths = 0, []
    for u in range(updates):
        rows, acts, rews, masks = [], [], [], []
        for t in range(T):
            x = torch.from_numpy(obs).double()
            with torch.no_grad():
                _, z = R.policy_forward("mlp", P, x, None, None, None)
            a = torch.distributions.Categorical(logits=z).sample().numpy()
            counter += 1
            state, steps, nobs, r, m, _, ep = O.cartpole_step(state, steps, a, 3, counter)
            lengths += [(u, float(e)) for e in ep[ep > 0]]
            rows.append(x), acts.append(torch.from_numpy(a)), rews.append(r), masks.append(m)
            obs = nobs
        with torch.no_grad():
            ret, _ = R.policy_forward("mlp", P, torch.from_numpy(obs).double(), None, None, None)
            ret = ret.numpy()
        returns = []
        for t in reversed(range(T)):   # storage.py:116-121 without GAE
            ret = ret * gamma * masks[t] + rews[t]
            returns.insert(0, torch.from_numpy(ret.copy()))
        value, z = R.policy_forward("mlp", P, torch.cat(rows), None, None, None)
        total, *_ = R.torch_loss("cat", value, z, torch.cat(acts), torch.cat(returns), vc, ec)
        opt.zero_grad()
        total.backward()
        torch.nn.utils.clip_grad_norm_(P, max_norm)
        opt.step()
    return lengths


def tenths(lengths, updates):
    out = []
    for k in range(10):
        sel = [e for u, e in lengths if k * updates // 10 <= u < (k + 1) * updates // 10]
        out.append(float(np.mean(sel)) if sel else float("nan"))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=32)
    ap.add_argument("--updates", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    t = tenths(run(a.envs, a.updates, a.seed), a.updates)
    print("envs", a.envs, "updates", a.updates, "mean episode length per tenth:", " ".join("%.1f" % x for x in t))
    print("late / early = %.2f" % (t[-1] / t[0]))
