"""PPO — drop-in for a2c_ppo_acktr/algo/ppo.py (reference
ppo-dash-training/pytorch-a2c-ppo-acktr-gail/a2c_ppo_acktr/algo/ppo.py:7-96).

update(rollouts) keeps the reference's semantics — advantages normalised over
all T*N samples (:35-37), ppo_epoch passes of num_mini_batch minibatches cut
from torch.randperm on the default CPU generator (:43-51, bit-identical index
sets), clipped surrogate + clipped value loss + entropy (:61-81),
clip_grad_norm_ + Adam (:82-84), mean losses returned as floats (:86-96) —
but each minibatch is one fused HIP pipeline with no autograd: the obs rows
are gathered inside conv1, the loss gradient is analytic, and the losses are
accumulated on the device (one device->host copy per update instead of three
per minibatch).

Multi-GPU (new; the reference's PPO path has no collectives):
with torch.distributed initialised each rank owns its own env lanes and
storage; per update one 3-double all-reduce makes the advantage statistics
global, per minibatch one all-reduce (RCCL over xGMI) sums the flat gradient,
and clip + Adam run on the averaged gradient so all ranks stay identical.
"""
import torch

from .. import _dist
from .._hip import call
from ._flat import FlatOptimizer, GuardedUpdate


class FlatAdam(FlatOptimizer):
    """torch.optim.Adam-compatible façade over one flat parameter buffer.
    param_groups[0]['lr'] is read at every step (utils.update_linear_schedule)."""

    STATE = ("exp_avg", "exp_avg_sq")
    NAME, NOUN = "Adam", "moments"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None):
        super().__init__(params, {"lr": lr, "betas": betas, "eps": eps, "weight_decay": 0, "amsgrad": False},
                         max_grad_norm)

    def _apply(self, eng, n, scale, max_norm, gi, gd, sk, s):
        g = self.param_groups[0]
        b1, b2 = g["betas"]
        call("ppo_clip_adam_guarded", eng.flat.data_ptr(), eng.grad.data_ptr(), self.exp_avg.data_ptr(),
             self.exp_avg_sq.data_ptr(), n, self._partials.data_ptr(), scale, max_norm, float(g["lr"]),
             float(b1), float(b2), float(g["eps"]), self.step_count, self._norm.data_ptr(), gi, gd, sk, s)


class PPO(GuardedUpdate):
    def __init__(self,
                 actor_critic,
                 clip_param,
                 ppo_epoch,
                 num_mini_batch,
                 value_loss_coef,
                 entropy_coef,
                 lr=None,
                 eps=None,
                 max_grad_norm=None,
                 use_clipped_value_loss=True):
        self.actor_critic = actor_critic
        self.clip_param = clip_param
        self.ppo_epoch = ppo_epoch
        self.num_mini_batch = num_mini_batch
        self.value_loss_coef = value_loss_coef
        self.entropy_coef = entropy_coef
        self.max_grad_norm = max_grad_norm
        self.use_clipped_value_loss = use_clipped_value_loss
        self.optimizer = FlatAdam(actor_critic.parameters(), lr=lr, eps=eps, max_grad_norm=max_grad_norm)
        self._loss_acc = None
        if _dist.active():
            # one-time parameter broadcast so every rank starts from rank 0's weights
            eng = actor_critic.hip_engine()
            _dist.broadcast_params(eng.flat)
            eng.epoch += 1

    def update(self, rollouts):
        eng = self.actor_critic.hip_engine()
        advantages = rollouts.normalized_advantages()            # ppo.py:35-37
        self._begin_update(eng)   # zeroes the loss sums, arms the device guards of every clip + Adam
        hp = {"clip": float(self.clip_param), "value_coef": float(self.value_loss_coef),
              "entropy_coef": float(self.entropy_coef), "use_clipped_value_loss": bool(self.use_clipped_value_loss)}
        num_steps, num_processes = rollouts.rewards.size()[0:2]
        if self.actor_critic.is_recurrent:
            self._update_recurrent(eng, rollouts, advantages, hp, num_processes)
            return self._losses()
        batch_size = num_processes * num_steps
        assert batch_size >= self.num_mini_batch, (
            "PPO requires the number of processes ({}) "
            "* number of steps ({}) = {} "
            "to be greater than or equal to the number of PPO mini batches ({})."
            "".format(num_processes, num_steps, batch_size, self.num_mini_batch))
        mini_batch_size = batch_size // self.num_mini_batch
        for e in range(self.ppo_epoch):
            # SubsetRandomSampler's draw (storage.py:138-141), same generator
            perm = torch.randperm(batch_size).to(eng.device, non_blocking=True)
            for start in range(0, batch_size - mini_batch_size + 1, mini_batch_size):
                idx = perm[start:start + mini_batch_size]
                eng.train_minibatch(rollouts, advantages, idx, hp, self._loss_acc, self.optimizer)
        return self._losses()

    def _update_recurrent(self, eng, rollouts, advantages, hp, num_processes):
        """recurrent_generator semantics (storage.py:162-223): env order from
        torch.randperm(N) on the default CPU generator, N//M whole sequences per
        minibatch, BPTT over the full rollout."""
        assert num_processes >= self.num_mini_batch, (
            "PPO requires the number of processes ({}) "
            "to be greater than or equal to the number of "
            "PPO mini batches ({}).".format(num_processes, self.num_mini_batch))
        per = num_processes // self.num_mini_batch
        for e in range(self.ppo_epoch):
            perm = torch.randperm(num_processes)
            for start in range(0, num_processes, per):
                if start + per > num_processes:
                    raise IndexError("index {} is out of bounds for dimension 0 with size {}".format(
                        num_processes, num_processes))
                envs = perm[start:start + per].to(eng.device, non_blocking=True)
                eng.train_minibatch_rec(rollouts, advantages, envs, hp, self._loss_acc, self.optimizer)

    def _losses(self):
        num_updates = self.ppo_epoch * self.num_mini_batch        # ppo.py:90 (not the drop_last count)
        return self._finish_update("PPO.update", num_updates, self.ppo_epoch)
