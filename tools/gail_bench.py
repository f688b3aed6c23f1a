#!/usr/bin/env python
"""GAIL timings on the MI355X (needs the GPU; there is no fallback):

  (a) one discriminator minibatch at B = 128, D = 23 (obs 17 + action 6), Hd = 100:
      the fused pipeline (ppo_gail_train, ppo_gail_reduce, ppo_grad_sumsq, ppo_clip_adam:
      four launches, policy rows gathered in the kernel) against gail.py's loop body as
      torch autograd + torch.optim.Adam on the same device, fed rows that are already
      gathered and on the device (which favours torch); and a whole update() of 8 pairs,
      host loader and copies included, against the reference-text loop over the same loader
      and this package's feed_forward_generator.
  (b) predict_rewards at N = 4096, T = 128 (two launches) against the per-step form with
      the reference's per-step device->host copy and numpy RunningMeanStd update.

Times are device-event times around windows that end in a synchronise, the median of
--repeats windows after a warm-up of every shape.  Prints one JSON line per measurement.

    python tools/gail_bench.py [--repeats 7] [--only NAME] [--out profiles/gail_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F
import torch.utils.data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ppo-dash_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def window_ms(fn, iters):
    """device time of `iters` calls of fn, ended by a synchronise -> ms per call"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def median_ms(fn, iters, repeats, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = sorted(window_ms(fn, iters) for _ in range(repeats))
    return {"ms": t[len(t) // 2], "min_ms": t[0], "max_ms": t[-1], "iters": iters, "repeats": repeats}


def torch_pair(discr, opt, x_e, x_p, sync_loss=False):
    """gail.py:69-95 for one pair in plain torch: two forwards, BCE, the gradient penalty
    (compute_grad_pen: its own torch.rand draw and copy), backward, Adam"""
    d_p, d_e = discr.trunk(x_p), discr.trunk(x_e)
    loss = (F.binary_cross_entropy_with_logits(d_e, torch.ones_like(d_e)) +
            F.binary_cross_entropy_with_logits(d_p, torch.zeros_like(d_p)))
    A = 6
    loss = loss + discr.compute_grad_pen(x_e[:, :-A], x_e[:, -A:], x_p[:, :-A], x_p[:, -A:])
    out = loss.item() if sync_loss else None
    opt.zero_grad()
    loss.backward()
    opt.step()
    return out


class HostRMS(object):
    """baselines' RunningMeanStd(shape=()) on the host, numpy moments as the reference takes them"""

    def __init__(self):
        self.mean, self.var, self.count = np.zeros(()), np.ones(()), 1e-4

    def update(self, x):
        bm, bv, bc = np.mean(x, axis=0), np.var(x, axis=0), x.shape[0]
        delta, tot = bm - self.mean, self.count + bc
        m2 = self.var * self.count + bv * bc + np.square(delta) * self.count * bc / tot
        self.mean, self.var, self.count = self.mean + delta * bc / tot, m2 / tot, tot


def torch_rewards(discr, st, gamma, state):
    """gail.py:98-111 per step, as run.py:236-241 drives it: one D2H copy per step"""
    T = st.num_steps
    with torch.no_grad():
        for t in range(T):
            d = discr.trunk(torch.cat([st.obs[t], st.actions[t]], dim=1))
            s = torch.sigmoid(d)
            r = s.log() - (1 - s).log()
            if state["returns"] is None:
                state["returns"] = r.clone()
            state["returns"] = state["returns"] * st.masks[t] * gamma + r
            state["rms"].update(state["returns"].cpu().numpy())
            st.rewards[t].copy_(r / float(np.sqrt(state["rms"].var.reshape(-1)[0] + 1e-8)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="", help="measure only the lines whose name contains this")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gail_bench: no MI355X visible; nothing is measured on the CPU")
    from a2c_ppo_acktr import synthetic as S
    from a2c_ppo_acktr._hip import call, stream
    from a2c_ppo_acktr.algo import gail
    from a2c_ppo_acktr.storage import RolloutStorage

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    od, A, Hd, B = 17, 6, 100, 128
    D = od + A
    lines = []

    def emit(name, measure, **kw):
        if args.only not in name:
            return
        line = dict({"bench": name}, **kw)
        line.update(measure())
        lines.append(line)
        print(json.dumps(line), flush=True)

    # ------------------------------------------------------------ (a) update
    T, N = 64, 16                                   # T N = 1024 rows = 8 minibatches of 128
    st = RolloutStorage(T, N, (od,), [0], S.Box(shape=(A,)), 1, device=dev)
    st.obs.normal_()
    st.actions.normal_()
    ds = torch.utils.data.TensorDataset(torch.randn(1024, od), torch.randn(1024, A))
    loader = torch.utils.data.DataLoader(ds, batch_size=B, shuffle=True, drop_last=True)
    discr = gail.Discriminator(D, Hd, dev)
    P = discr.numel
    x_e = torch.randn(B, D, device=dev)
    alpha = torch.rand(B, device=dev)
    idx = torch.randperm(T * N)[:B].to(dev)
    x_p = torch.cat([st.obs[:T].reshape(T * N, od)[idx], st.actions.reshape(T * N, A)[idx]], 1)
    nblk = call("ppo_gail_train_blocks", B)
    pg, pl = torch.empty(nblk * P, device=dev), torch.empty(nblk * 3, device=dev)
    acc = torch.zeros(4, dtype=torch.float64, device=dev)

    def fused_pair():
        s = stream()
        call("ppo_gail_train", discr.flat.data_ptr(), D, Hd, B, st.obs.data_ptr(), od, None, 0, st.actions.data_ptr(),
             A, T * N, idx.data_ptr(), 0, x_e.data_ptr(), alpha.data_ptr(), 10.0, pg.data_ptr(), pl.data_ptr(), s)
        call("ppo_gail_reduce", pg.data_ptr(), pl.data_ptr(), nblk, P, B, 10.0, discr.grad.data_ptr(),
             acc.data_ptr(), s)
        discr.optimizer._step_flat(discr)

    emit("update_pair_fused", lambda: median_ms(fused_pair, 200, args.repeats, 20), B=B, D=D, Hd=Hd, launches=4)
    ref = gail.Discriminator(D, Hd, dev)
    opt = torch.optim.Adam(ref.trunk.parameters())
    emit("update_pair_torch_autograd", lambda: median_ms(lambda: torch_pair(ref, opt, x_e, x_p), 50, args.repeats, 10),
         B=B, D=D, Hd=Hd)

    def torch_update():
        gen = st.feed_forward_generator(None, mini_batch_size=loader.batch_size)
        for (e_s, e_a), pb in zip(loader, gen):
            torch_pair(ref, opt, torch.cat([e_s.to(dev), e_a.to(dev)], 1), torch.cat([pb[0], pb[3]], 1), True)

    emit("update_8_pairs_fused", lambda: median_ms(lambda: discr.update(loader, st), 5, args.repeats, 2), pairs=8)
    emit("update_8_pairs_torch_autograd", lambda: median_ms(torch_update, 3, args.repeats, 1), pairs=8)

    # ----------------------------------------------------------- (b) rewards
    T, N = 128, 4096
    st = RolloutStorage(T, N, (od,), [0], S.Box(shape=(A,)), 1, device=dev)
    st.obs.normal_()
    st.actions.normal_()
    st.masks.copy_((torch.rand_like(st.masks) > 0.01).float())
    flop = 2.0 * T * N * (D * Hd + Hd * Hd + Hd)

    def with_rate(key, fn):
        r = median_ms(fn, 10, args.repeats, 2)
        return dict(r, **{key: flop / (r["ms"] * 1e-3) / 1e12})

    emit("predict_rewards_fused", lambda: with_rate("end_to_end_tflops", lambda: discr.predict_rewards(st, 0.99)),
         T=T, N=N, launches=2, algorithmic_gflop=flop / 1e9)
    s = stream()
    out = torch.empty(T * N, device=dev)
    emit("reward_kernel_alone", lambda: with_rate("tflops", lambda: call(
        "ppo_gail_reward", discr.flat.data_ptr(), D, Hd, st.obs.data_ptr(), od, None, 0, st.actions.data_ptr(), A, 0,
        T * N, out.data_ptr(), s)), T=T, N=N)
    state = {"returns": None, "rms": HostRMS()}
    emit("predict_reward_per_step_torch_host_rms",
         lambda: median_ms(lambda: torch_rewards(discr, st, 0.99, state), 2, args.repeats, 1), T=T, N=N)
    steps = gail.Discriminator(D, Hd, dev)

    def fused_steps():
        for t in range(T):
            steps.predict_reward(st.obs[t], st.actions[t], 0.99, st.masks[t])

    emit("predict_reward_per_step_fused", lambda: median_ms(fused_steps, 2, args.repeats, 1), T=T, N=N,
         launches=2 * T)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
