#!/usr/bin/env python3
"""Golden vectors for MultiBinary action spaces (Bernoulli) — CONTAINER ONLY, a
sibling of gen_golden_gauss.py: it imports the reference's own modules through
gen_golden.load_ref and records arrays only (tests/golden/bern.npz,
tests/golden/bern_update.npz).

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_bern.py [bern] [bern_update]
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from gen_golden import flat_params, load_ref, param_names, save  # noqa: E402


class MultiBinary:  # duck-typed gym.spaces.MultiBinary (storage.py:24, model.py:36)
    def __init__(self, n):
        self.n = n
        self.shape = (n,)


MIN_MARGIN = 1e-4   # smallest |u - p| a recorded draw may have (the engine's p is ~1e-6 off)


# ---------------------------------------------------------------------------
# MLPBase submodules + Bernoulli(64, 3) (distributions.py:45-56, 93-104); the
# submodules are driven directly, as gen_golden.gen_mlp does
# ---------------------------------------------------------------------------
def gen_bern(M, D):
    torch.manual_seed(5)
    base = M.MLPBase(4, recurrent=False, hidden_size=64)
    head = D.Bernoulli(64, 3)
    x = torch.randn(8, 4)
    with torch.no_grad():
        value = base.critic_linear(base.critic(x))
        feat = base.actor(x)
        dist = head(feat)
        rs = torch.get_rng_state()
        action = dist.sample()
        after = torch.get_rng_state()
        torch.set_rng_state(rs)
        u = torch.empty(8, 3).uniform_()
        # torch.bernoulli(probs) is (u < probs) on the uniform_() draw, generator included
        assert torch.equal(torch.get_rng_state(), after)
        assert torch.equal(action, (u < dist.probs).float())
        assert float((u - dist.probs).abs().min()) >= MIN_MARGIN
        logp = dist.log_probs(action)
    save("bern.npz", base_params=flat_params(base), base_names=param_names(base),
         head_params=flat_params(head), head_names=param_names(head), x=x.numpy(), value=value.numpy(),
         actor_features=feat.numpy(), logits=dist.logits.numpy(), probs=dist.probs.numpy(),
         uniform_noise=u.numpy(), rng_state=rs.numpy(), action=action.numpy(), log_probs=logp.numpy(),
         entropy=dist.entropy().numpy(), mode=dist.mode().numpy())


# ---------------------------------------------------------------------------
# One PPO iteration of CNNBase + Bernoulli(hidden, 3): gen_golden.gen_cnn_update's
# recipe with MultiBinary(3), lowres observations, the uniform draw of every step
# ---------------------------------------------------------------------------
def gen_bern_update(S, M, P, *, hidden=64, N=4, T=4, E=2, Mb=2, lr=1e-3, A=3, seed=1, fname="bern_update.npz"):
    torch.manual_seed(seed)
    pol = M.Policy((4, 84, 84), MultiBinary(A), base=M.CNNBase,
                   base_kwargs={"recurrent": False, "hidden_size": hidden}, vector_obs_len=0)
    with torch.no_grad():
        # start from bf16-representable parameters: the fp32 record of the initial
        # parameters then compresses to about half its size (the fixture's size limit)
        for q in pol.parameters():
            q.copy_(q.bfloat16().float())
    agent = P.PPO(pol, 0.1, E, Mb, 0.5, 0.001, lr=lr, eps=1e-5, max_grad_norm=0.5)
    st = S.RolloutStorage(T, N, (4, 84, 84), [0], MultiBinary(A), pol.recurrent_hidden_state_size)
    init = flat_params(pol)
    genv = torch.Generator().manual_seed(123)

    def frame():
        lo = torch.randint(0, 256, (N, 4, 21, 21), dtype=torch.uint8, generator=genv)
        return lo.repeat_interleave(4, 2).repeat_interleave(4, 3).contiguous()

    obs_u8 = np.zeros((T + 1, N, 4, 84, 84), np.uint8)
    o0 = frame()
    obs_u8[0] = o0.numpy()
    st.obs[0].copy_(o0.float() / 255.0)
    noise, values, actions, logps, rewards, masks = [], [], [], [], [], []
    margin = float("inf")
    for step in range(T):
        with torch.no_grad():
            rs = torch.get_rng_state()
            value, action, logp, hxs = pol.act(st.obs[step], st.vector_obs[step],
                                               st.recurrent_hidden_states[step], st.masks[step])
            after = torch.get_rng_state()
            torch.set_rng_state(rs)
            u = torch.empty(N, A).uniform_()
            assert torch.equal(torch.get_rng_state(), after)
            torch.set_rng_state(after)
            _, feat, _ = pol.base(st.obs[step], st.vector_obs[step], st.recurrent_hidden_states[step],
                                  st.masks[step])
            probs = pol.dist(feat).probs
            assert torch.equal(action, (u < probs).float())
            # a replayed action must not flip on the engine's ~1e-6 difference in p: pick another seed
            margin = min(margin, float((u - probs).abs().min()))
            assert margin >= MIN_MARGIN, (seed, step, margin)
        o = frame()
        rew = torch.rand(N, 1, generator=genv)
        done = torch.rand(N, generator=genv) < 0.3
        mk = torch.FloatTensor([[0.0] if d else [1.0] for d in done])
        obs_u8[step + 1] = o.numpy()
        st.insert(o.float() / 255.0, torch.zeros(N, 0), hxs, action, logp, value, rew, mk, torch.ones(N, 1))
        noise.append(u.numpy()); values.append(value.numpy()); actions.append(action.numpy())
        logps.append(logp.numpy()); rewards.append(rew.numpy()); masks.append(mk.numpy())
    with torch.no_grad():
        next_value = pol.get_value(st.obs[-1], st.vector_obs[-1], st.recurrent_hidden_states[-1],
                                   st.masks[-1]).detach()
    st.compute_returns(next_value, True, 0.99, 0.95, False)
    returns = st.returns.numpy().copy()
    vpreds = st.value_preds.numpy().copy()
    rng_before_update = torch.get_rng_state()
    vl, al, ent = agent.update(st)
    rng_after_update = torch.get_rng_state()
    torch.set_rng_state(rng_before_update)
    perms = np.stack([torch.randperm(N * T).numpy() for _ in range(E)]).astype(np.int64)
    assert torch.equal(torch.get_rng_state(), rng_after_update)
    final = flat_params(pol)
    # How far the reference's own fp32 arithmetic is from float64 on the recorded
    # rollout (same initial parameters, observations, actions, rewards, masks and
    # minibatch permutations; the reference's modules under a float64 default dtype):
    # the replay test's bounds are the Categorical replay's as long as this stays
    # under half of each (printed; see DESIGN.md and the test's docstring)
    torch.set_default_dtype(torch.float64)
    orig_randperm = torch.randperm
    try:
        pol64 = M.Policy((4, 84, 84), MultiBinary(A), base=M.CNNBase,
                         base_kwargs={"recurrent": False, "hidden_size": hidden}, vector_obs_len=0)
        with torch.no_grad():
            off = 0
            for q in pol64.parameters():
                q.copy_(torch.from_numpy(init[off:off + q.numel()]).double().view_as(q))
                off += q.numel()
        agent64 = P.PPO(pol64, 0.1, E, Mb, 0.5, 0.001, lr=lr, eps=1e-5, max_grad_norm=0.5)
        st64 = S.RolloutStorage(T, N, (4, 84, 84), [0], MultiBinary(A), pol64.recurrent_hidden_state_size)
        o64 = (torch.from_numpy(obs_u8).float() / 255.0).double()
        st64.obs[0].copy_(o64[0])
        for step in range(T):
            with torch.no_grad():
                act64 = torch.from_numpy(actions[step]).double()
                v64, lp64, _, hxs = pol64.evaluate_actions(st64.obs[step], st64.vector_obs[step],
                                                           st64.recurrent_hidden_states[step], st64.masks[step], act64)
            st64.insert(o64[step + 1], torch.zeros(N, 0), hxs, act64, lp64, v64,
                        torch.from_numpy(rewards[step]).double(), torch.from_numpy(masks[step]).double(),
                        torch.ones(N, 1))
        with torch.no_grad():
            nv64 = pol64.get_value(st64.obs[-1], st64.vector_obs[-1], st64.recurrent_hidden_states[-1],
                                   st64.masks[-1]).detach()
        st64.compute_returns(nv64, True, 0.99, 0.95, False)
        queue = [torch.from_numpy(q) for q in perms]
        torch.randperm = lambda n, **k: queue.pop(0)
        l64 = agent64.update(st64)
        assert not queue
        dist = {"values": np.abs(st64.value_preds[:T].numpy() - np.stack(values)).max(),
                "log_probs": np.abs(st64.action_log_probs.numpy() - np.stack(logps)).max(),
                "returns": np.abs(st64.returns.numpy() - returns).max(),
                "losses_rel": max(abs(a - b) / max(abs(a), 1e-12) for a, b in zip(l64, (vl, al, ent))),
                "losses_abs": max(abs(a - b) for a, b in zip(l64, (vl, al, ent))),
                "final_params": np.abs(np.concatenate([q.detach().reshape(-1).numpy() for q in pol64.parameters()])
                                       - final).max()}
    finally:
        torch.randperm = orig_randperm
        torch.set_default_dtype(torch.float32)
    print(f"{fname}: seed {seed}, min |u - p| over {T * N * A} draws {margin:.2e}")
    print(f"{fname}: fp32 record vs float64 on the recorded rollout: "
          + ", ".join(f"{k} {v:.2e}" for k, v in dist.items()))
    save(fname, init_params=init, final_params=final, names=param_names(pol), obs_u8=obs_u8,
         uniform_noise=np.stack(noise), values=np.stack(values), actions=np.stack(actions),
         action_log_probs=np.stack(logps), rewards=np.stack(rewards), masks=np.stack(masks),
         next_value=next_value.numpy(), returns=returns, value_preds_after=vpreds, perms=perms,
         losses=np.array([vl, al, ent]), coefs=np.array([0.1, 0.5, 0.001]),
         meta=np.array([hidden, N, T, E, Mb, A]), lr=np.array([lr]), min_margin=np.array([margin]),
         fp64_distance_names=np.array(list(dist)), fp64_distance=np.array([float(v) for v in dist.values()]))


def main():
    torch.set_num_threads(1)
    want = set(sys.argv[1:])
    S, M, D, P = load_ref("B")
    if not want or "bern" in want:
        gen_bern(M, D)
    if not want or "bern_update" in want:
        gen_bern_update(S, M, P)


if __name__ == "__main__":
    main()
