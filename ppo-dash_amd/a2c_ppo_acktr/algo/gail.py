"""GAIL — drop-in for a2c_ppo_acktr/algo/gail.py (reference
ppo-dash-training/pytorch-a2c-ppo-acktr-gail/a2c_ppo_acktr/algo/gail.py:12-165).

Discriminator keeps the reference's network (trunk = Linear(D, Hd) - Tanh - Linear(Hd, Hd)
- Tanh - Linear(Hd, 1), built in the same order, so the same seed gives the same initial
parameters), its loss (BCE of expert rows against 1 and of policy rows against 0, plus
lambda mean (|dd/dx(x_m)| - 1)^2 on rows mixed with alpha ~ U[0, 1)), Adam with torch's
defaults and no clipping, and its reward normalisation by the running standard deviation
of the discounted returns.  update() keeps the reference's loop and its draws on the
default CPU generator (DataLoader's, one torch.randperm(T N) at the first policy batch,
one torch.rand(B, 1) per pair), but each (expert, policy) pair is four launches
(csrc/gail.hip): the policy rows are gathered from the storage planes inside the train
kernel, the double backward of the penalty is analytic, and the loss sums stay on the
device (one device->host copy per update).  predict_rewards() is new: the rewards of a
whole rollout in two launches, written into rollouts.rewards, with no host round trip.

The class is implemented as the reference's functions are written, not as this fork of
the reference calls them: update() there takes policy_batch[2] for the action (in this
fork's generator index 2 is the hidden state; the action is index 3), and run.py calls
predict_reward with five positional arguments.  Here state = obs, concatenated with
vector_obs when the storage has one, and action = the stored action.

Two deliberate departures from gail.py:
 1. The reward is the logit d itself.  gail.py:101-103 computes log s - log(1 - s) with s =
    sigmoid(d), which equals d in exact arithmetic; in fp32 it loses precision as 1 - s
    cancels (5.0e-6 off at |d| <= 4, 3.5e-5 at |d| <= 6) and is +-inf from |d| ~ 17.
 2. The per-step batch moments of the returns are float64 sums of the fp32 returns in a
    fixed order (the reference: numpy's float32 pairwise mean / var), merged into float64
    {mean, var, count} on the device as baselines' RunningMeanStd merges them.

Not supported (TypeError / NotImplementedError): image observations, Discrete actions,
non-fp32 planes (Policy.half() storage), hidden_dim outside the kernels' limits (a multiple
of 4 in [4, 128]), an input_dim whose parameters do not fit the LDS (hidden_dim 100:
input_dim > 145), and torch.distributed runs (the discriminator gradient would need its
own all-reduce).
"""
import torch
import torch.nn as nn
import torch.utils.data
from torch import autograd

from .._hip import call, stream
from .ppo import FlatAdam

LDS_BYTES = 160 * 1024   # per CU on the MI355X
LAMBDA = 10.0   # compute_grad_pen's default lambda_, the only one update() uses


class _DeviceRMS(object):
    """ret_rms: baselines' RunningMeanStd(shape=()) whose {mean, var, count} are three
    float64 words on the device; reading an attribute copies them to the host."""

    def __init__(self, words):
        self._words = words

    mean = property(lambda self: self._words[0].item())
    var = property(lambda self: self._words[1].item())
    count = property(lambda self: self._words[2].item())


def _rms_words(device):
    return torch.tensor([0.0, 1.0, 1e-4], dtype=torch.float64, device=device)


class Discriminator(nn.Module):
    def __init__(self, input_dim, hidden_dim, device):
        super(Discriminator, self).__init__()
        if hidden_dim % 4 != 0 or not 4 <= hidden_dim <= 128:
            raise NotImplementedError("Discriminator: hidden_dim={} (the HIP kernels take a multiple of 4 in "
                                      "[4, 128]; the reference uses 100)".format(hidden_dim))
        if input_dim < 2:
            raise NotImplementedError("Discriminator: input_dim={} (state and action: at least 2)".format(input_dim))
        if call("ppo_gail_lds_bytes", input_dim, hidden_dim) > LDS_BYTES:
            raise NotImplementedError("Discriminator: input_dim={} with hidden_dim={} does not fit the {} KB of LDS "
                                      "the kernels keep the parameters in (hidden_dim 100: input_dim <= 145)".format(
                                          input_dim, hidden_dim, LDS_BYTES // 1024))
        self.device = torch.device(device)
        self.input_dim, self.hidden_dim = int(input_dim), int(hidden_dim)
        self.trunk = nn.Sequential(
            nn.Linear(input_dim, hidden_dim), nn.Tanh(),
            nn.Linear(hidden_dim, hidden_dim), nn.Tanh(),
            nn.Linear(hidden_dim, 1)).to(device)
        self.trunk.train()
        self._flatten()
        self.optimizer = FlatAdam(self.trunk.parameters())   # torch.optim.Adam()'s defaults
        self.returns = None
        self._rms = _rms_words(self.device)
        self.ret_rms = _DeviceRMS(self._rms)
        self._loss_acc = None
        self._parts = None

    # ------------------------------------------------------------ flat buffer
    def _flatten(self):
        """the parameters become views of one flat fp32 buffer (as _Engine._flatten)"""
        params = list(self.trunk.parameters())
        dev = params[0].device
        n = sum(p.numel() for p in params)
        flat, grad = torch.empty(n, device=dev), torch.zeros(n, device=dev)
        off = 0
        with torch.no_grad():
            for p in params:
                k = p.numel()
                flat[off:off + k].copy_(p.data.reshape(-1))
                p.data = flat[off:off + k].view_as(p)
                p.grad = grad[off:off + k].view_as(p)
                off += k
        self.flat, self.grad, self.numel = flat, grad, n

    def _bind(self):
        """-> the flat buffer; rebuilt when a .to() / .float() rebound the parameters"""
        off, base = 0, self.flat.data_ptr()
        for p in self.trunk.parameters():
            if p.data_ptr() != base + 4 * off or p.dtype != torch.float32:
                if p.dtype != torch.float32:
                    raise TypeError("Discriminator: fp32 parameters only (got {})".format(p.dtype))
                self._flatten()
                break
            off += p.numel()
        return self.flat

    def _require_gpu(self, what):
        dev = next(self.trunk.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("Discriminator.{}: the discriminator lives on {}; the HIP engine has no CPU "
                               "path (construct it with the MI355X device)".format(what, dev))
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            raise NotImplementedError("Discriminator.{}: torch.distributed is initialised; multi-GPU GAIL would "
                                      "need an all-reduce of the discriminator gradient".format(what))
        self.device = dev
        if self._rms.device != dev:
            self._rms = self._rms.to(dev)
            self.ret_rms = _DeviceRMS(self._rms)
        if self.returns is not None and self.returns.device != dev:
            self.returns = self.returns.to(dev)
        self._bind()
        return dev

    def _planes(self, rollouts, what):
        """(obs, obs_dim, vector_obs | None, V, actions, A, rows) of a RolloutStorage"""
        obs, vec, act = rollouts.obs, rollouts.vector_obs, rollouts.actions
        if obs.dim() != 3:
            raise NotImplementedError("Discriminator.{}: observations of shape {} (1-D observations only, as "
                                      "run.py asserts for --gail)".format(what, tuple(obs.shape[2:])))
        if act.dtype == torch.int64:
            raise NotImplementedError("Discriminator.{}: Discrete (int64) actions; GAIL here takes Box "
                                      "actions".format(what))
        if obs.dtype == torch.float16:
            raise NotImplementedError("Discriminator.{}: fp16 observation plane (Policy.half() storage); the "
                                      "discriminator kernels read fp32".format(what))
        for name, t in (("obs", obs), ("vector_obs", vec), ("actions", act)):
            if t.dtype != torch.float32:
                raise TypeError("Discriminator.{}: {} must be torch.float32, got {}".format(what, name, t.dtype))
            if t.device != self.device:
                raise RuntimeError("Discriminator.{}: {} is on {}, the discriminator on {} (the HIP engine has "
                                   "no CPU path)".format(what, name, t.device, self.device))
        od, V, A = obs.shape[2], (vec.shape[2] if vec.dim() == 3 else 0), act.shape[2]
        if od + V + A != self.input_dim:
            raise TypeError("Discriminator.{}: input_dim={} but obs {} + vector_obs {} + action {} = {}".format(
                what, self.input_dim, od, V, A, od + V + A))
        T, N = rollouts.rewards.size()[0:2]
        return obs, od, (vec if V else None), V, act, A, T, N

    # -------------------------------------------------------------- reference
    def compute_grad_pen(self, expert_state, expert_action, policy_state, policy_action, lambda_=10):
        """gail.py:30-56 in plain torch (autograd with create_graph): the on-device yardstick
        of the train kernel's penalty.  Draws torch.rand(B, 1) on the CPU generator."""
        alpha = torch.rand(expert_state.size(0), 1)
        expert_data = torch.cat([expert_state, expert_action], dim=1)
        policy_data = torch.cat([policy_state, policy_action], dim=1)
        alpha = alpha.expand_as(expert_data).to(expert_data.device)
        mixup = (alpha * expert_data + (1 - alpha) * policy_data).detach().requires_grad_(True)
        disc = self.trunk(mixup)
        grad, = autograd.grad(outputs=disc, inputs=mixup, grad_outputs=torch.ones_like(disc), create_graph=True,
                              retain_graph=True, only_inputs=True)
        return lambda_ * (grad.norm(2, dim=1) - 1).pow(2).mean()

    # ----------------------------------------------------------------- update
    def update(self, expert_loader, rollouts, obsfilt=None):
        """gail.py:58-96: one Adam step per (expert batch, policy minibatch) pair; returns
        the mean loss over the pairs."""
        dev = self._require_gpu("update")
        self.train()
        obs, od, vec, V, act, A, T, N = self._planes(rollouts, "update")
        D, Hd, P = self.input_dim, self.hidden_dim, self.numel
        batch_size, mbs = T * N, expert_loader.batch_size
        if self._loss_acc is None or self._loss_acc.device != dev:
            self._loss_acc = torch.zeros(4, dtype=torch.float64, device=dev)
        else:
            self._loss_acc.zero_()
        s = stream()
        n, perm = 0, None
        for expert_state, expert_action in expert_loader:      # zip(...): the expert side is drawn first
            if perm is None:
                # feed_forward_generator's first step: SubsetRandomSampler's permutation (storage.py:138-141)
                perm = torch.randperm(batch_size).to(dev, non_blocking=True)
            start = n * mbs
            if start + mbs > batch_size:    # drop_last: the policy side of the zip is exhausted
                break
            B = expert_state.size(0)
            if B != mbs:
                raise ValueError("Discriminator.update: expert batch of {} rows against a policy minibatch of {} "
                                 "(build the expert DataLoader with drop_last=True)".format(B, mbs))
            alpha = torch.rand(B, 1)                            # compute_grad_pen's draw (gail.py:36)
            if obsfilt is not None:
                expert_state = torch.as_tensor(obsfilt(expert_state.numpy(), update=False))
            host = torch.empty(B * D + B)
            rows = host[:B * D].view(B, D)
            if expert_state.size(1) + expert_action.size(1) != D:
                raise TypeError("Discriminator.update: expert state {} + action {} != input_dim {}".format(
                    expert_state.size(1), expert_action.size(1), D))
            rows[:, :expert_state.size(1)] = expert_state
            rows[:, expert_state.size(1):] = expert_action
            host[B * D:] = alpha.view(-1)
            pair = host.to(dev, non_blocking=True)              # expert rows and alpha: one H2D copy
            nblk = call("ppo_gail_train_blocks", B)
            if self._parts is None or self._parts[0].numel() < nblk * P or self._parts[0].device != dev:
                self._parts = (torch.empty(nblk * P, device=dev), torch.empty(nblk * 3, device=dev))
            pg, pl = self._parts
            call("ppo_gail_train", self.flat.data_ptr(), D, Hd, B, obs.data_ptr(), od,
                 None if vec is None else vec.data_ptr(), V, act.data_ptr(), A, batch_size,
                 perm[start:start + mbs].data_ptr(), 0, pair.data_ptr(), pair.data_ptr() + 4 * B * D, LAMBDA,
                 pg.data_ptr(), pl.data_ptr(), s)
            call("ppo_gail_reduce", pg.data_ptr(), pl.data_ptr(), nblk, P, B, LAMBDA, self.grad.data_ptr(),
                 self._loss_acc.data_ptr(), s)
            self.optimizer._step_flat(self)                     # Σg² partials + Adam, no clipping
            n += 1
        loss = self._loss_acc[0].item() if n else 0             # one D2H per update
        return loss / n

    # ---------------------------------------------------------------- rewards
    def _returns_for(self, first, N):
        if self.returns is None:
            self.returns = first.clone().view(N, 1)             # gail.py:104-105
        elif self.returns.numel() != N:
            raise RuntimeError("Discriminator: returns holds {} lanes, this call has {}".format(
                self.returns.numel(), N))
        elif not self.returns.is_contiguous() or self.returns.dtype != torch.float32:
            self.returns = self.returns.float().contiguous()
        return self.returns

    def predict_reward(self, state, action, gamma, masks, update_rms=True):
        """gail.py:98-111 for one step: state [N, S], action [N, A], masks [N, 1] on the
        device -> scaled rewards [N, 1]."""
        dev = self._require_gpu("predict_reward")
        self.eval()
        for name, t in (("state", state), ("action", action), ("masks", masks)):
            if t.dtype != torch.float32:
                raise TypeError("Discriminator.predict_reward: {} must be torch.float32, got {}".format(name,
                                                                                                       t.dtype))
            if t.device != dev:
                raise RuntimeError("Discriminator.predict_reward: {} is on {}; the HIP engine has no CPU "
                                   "path".format(name, t.device))
        if state.dim() != 2 or action.dim() != 2 or state.size(1) + action.size(1) != self.input_dim:
            raise TypeError("Discriminator.predict_reward: state {} and action {} for input_dim {}".format(
                tuple(state.shape), tuple(action.shape), self.input_dim))
        N = state.size(0)
        state, action, masks = state.contiguous(), action.contiguous(), masks.contiguous()
        reward = torch.empty(N, 1, device=dev)
        s = stream()
        call("ppo_gail_reward", self.flat.data_ptr(), self.input_dim, self.hidden_dim, state.data_ptr(),
             state.size(1), None, 0, action.data_ptr(), action.size(1), 0, N, reward.data_ptr(), s)
        ret = self._returns_for(reward, N)
        call("ppo_gail_returns", reward.data_ptr(), masks.data_ptr(), ret.data_ptr(), self._rms.data_ptr(), 1, N,
             float(gamma), int(bool(update_rms)), s)
        return reward

    def predict_rewards(self, rollouts, gamma, update_rms=True):
        """predict_reward for steps 0 .. T-1 of a rollout (run.py:236-241's loop) in two
        launches: rollouts.rewards[:T] is overwritten with the scaled rewards of (obs[t],
        vector_obs[t], actions[t]) under masks[t].  Equal, bit for bit, to T predict_reward
        calls.  No host synchronisation.  Returns rollouts.rewards."""
        dev = self._require_gpu("predict_rewards")
        self.eval()
        obs, od, vec, V, act, A, T, N = self._planes(rollouts, "predict_rewards")
        rew, masks = rollouts.rewards, rollouts.masks
        if rew.dtype != torch.float32 or masks.dtype != torch.float32 or not rew.is_contiguous():
            raise TypeError("Discriminator.predict_rewards: rewards and masks must be contiguous torch.float32")
        s = stream()
        call("ppo_gail_reward", self.flat.data_ptr(), self.input_dim, self.hidden_dim, obs.data_ptr(), od,
             None if vec is None else vec.data_ptr(), V, act.data_ptr(), A, 0, T * N, rew.data_ptr(), s)
        ret = self._returns_for(rew[0], N)
        call("ppo_gail_returns", rew.data_ptr(), masks.data_ptr(), ret.data_ptr(), self._rms.data_ptr(), T, N,
             float(gamma), int(bool(update_rms)), s)
        return rew

    # ------------------------------------------------------------- checkpoint
    def checkpoint_state(self):
        """What state_dict() (the reference's keys: the trunk) leaves out: the running moments,
        the carried returns and Adam's state — plain tensors and builtins on the host."""
        sd = self.optimizer.state_dict()
        cpu = lambda t: None if t is None else t.detach().cpu().clone()   # noqa: E731
        return {"input_dim": self.input_dim, "hidden_dim": self.hidden_dim,
                "trunk": {k: cpu(v) for k, v in self.state_dict().items()},
                "rms": cpu(self._rms), "returns": cpu(self.returns),
                "optimizer": {"step": int(sd["step"]), "exp_avg": cpu(sd["exp_avg"]),
                              "exp_avg_sq": cpu(sd["exp_avg_sq"]),
                              "param_groups": [{k: (list(v) if isinstance(v, tuple) else v)
                                                for k, v in sd["param_groups"][0].items()}]}}

    def load_checkpoint_state(self, st):
        if (st["input_dim"], st["hidden_dim"]) != (self.input_dim, self.hidden_dim):
            raise ValueError("discriminator checkpoint is {}x{}, this one {}x{}".format(
                st["input_dim"], st["hidden_dim"], self.input_dim, self.hidden_dim))
        self.load_state_dict(st["trunk"])     # copies in place: the flat views stay bound
        dev = next(self.trunk.parameters()).device
        self._rms = st["rms"].to(dev, torch.float64).clone()
        self.ret_rms = _DeviceRMS(self._rms)
        self.returns = None if st["returns"] is None else st["returns"].to(dev).clone()
        o = st["optimizer"]
        pg = dict(o["param_groups"][0])
        pg["betas"] = tuple(pg["betas"])
        mv = lambda t: None if t is None else t.to(dev).clone()   # noqa: E731
        self.optimizer.load_state_dict({"step": o["step"], "exp_avg": mv(o["exp_avg"]),
                                        "exp_avg_sq": mv(o["exp_avg_sq"]), "param_groups": [pg]})


class ExpertDataset(torch.utils.data.Dataset):
    """gail.py:114-165 on the host: num_trajectories trajectories picked by one
    torch.randperm, each subsampled every subsample_frequency steps from an offset drawn
    by one torch.randint (in that order, on the default CPU generator); item i is the
    (state, action) pair i of the kept steps, trajectory by trajectory.  file_name is a
    torch.save'd dict of tensors {states [n, L, S], actions [n, L, A], lengths [n], ...}."""

    def __init__(self, file_name, num_trajectories=4, subsample_frequency=20):
        everything = torch.load(file_name)
        perm = torch.randperm(everything['states'].size(0))
        idx = perm[:num_trajectories]
        start_idx = torch.randint(0, subsample_frequency, size=(num_trajectories, ))
        self.trajectories = {}
        for k, v in everything.items():
            picked = v[idx]
            if k == 'lengths':
                self.trajectories[k] = picked // subsample_frequency
            else:
                self.trajectories[k] = torch.stack([picked[i, int(start_idx[i])::subsample_frequency]
                                                    for i in range(num_trajectories)])
        lengths = [int(x) for x in self.trajectories['lengths']]
        self.length = sum(lengths)
        self.get_idx = [(traj, i) for traj, n in enumerate(lengths) for i in range(n)]

    def __len__(self):
        return self.length

    def __getitem__(self, i):
        traj, j = self.get_idx[i]
        return self.trajectories['states'][traj][j], self.trajectories['actions'][traj][j]
