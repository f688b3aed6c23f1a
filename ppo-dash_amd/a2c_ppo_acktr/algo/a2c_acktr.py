"""A2C — drop-in for a2c_ppo_acktr/algo/a2c_acktr.py (reference
ppo-dash-training/pytorch-a2c-ppo-acktr-gail/a2c_ppo_acktr/algo/a2c_acktr.py:8-80),
the algorithm arguments.py selects by default.

update(rollouts) keeps the reference's semantics — evaluate_actions over all T*N
rows in storage order, from recurrent_hidden_states[0] and masks[:-1] (:38-43),
advantages = returns[:-1] - values, value loss advantages.pow(2).mean() with no
0.5, action loss -(advantages.detach() * log_probs).mean() (:45-51), no advantage
normalisation and no permutation, one backward of value_loss * value_loss_coef +
action_loss - dist_entropy * entropy_coef (:70-72), clip_grad_norm_ + RMSprop
(:30-31, :74-78), the three losses returned as floats (:80) — as one HIP
minibatch: PPO's pipeline (algo/ppo.py) run once over every row, with A2C's row
loss in the heads kernels (ppo_heads_*_train_a2c) and the fused clip + RMSprop
(ppo_clip_rmsprop_guarded) as the optimizer.  Recurrent policies take the
recurrent minibatch of all N envs in order: BPTT over the full T.

The reference's own call at :38-43 passes four arguments to an evaluate_actions
that takes five in that tree (model.py:72; vector_inputs was added for PPO and
this call site was not updated), so it raises TypeError as it stands.  What is
implemented is the text of update() with rollouts.vector_obs[:-1] in the position
PPO's generators pass it.

ACKTR (acktr=True: the K-FAC optimizer, kfac.py, and the sampled-Fisher pass
:53-68) is not implemented.

The update is one minibatch: no chunking, no gradient accumulation.  Its
workspace grows with T*N.  Multi-GPU goes through the same _dist
calls as PPO (parameter broadcast, gradient all-reduce, guard and loss
all-reduces); there are no advantage statistics to reduce.
"""
import torch

from .. import _dist
from .._hip import call
from ._flat import FlatOptimizer, GuardedUpdate


class FlatRMSprop(FlatOptimizer):
    """torch.optim.RMSprop-compatible façade over one flat parameter buffer (no
    momentum, not centered, no weight decay: the reference's construction, :30-31).
    param_groups[0]['lr'] is read at every step (utils.update_linear_schedule)."""

    STATE = ("square_avg",)
    NAME, NOUN = "RMSprop", "averages"

    def __init__(self, params, lr=1e-2, eps=1e-8, alpha=0.99, max_grad_norm=None):
        super().__init__(params, {"lr": lr, "momentum": 0, "alpha": alpha, "eps": eps, "centered": False,
                                  "weight_decay": 0}, max_grad_norm)

    def _apply(self, eng, n, scale, max_norm, gi, gd, sk, s):
        g = self.param_groups[0]
        if g["momentum"] or g["centered"] or g["weight_decay"]:
            raise NotImplementedError("FlatRMSprop: momentum, centered and weight_decay are not implemented")
        call("ppo_clip_rmsprop_guarded", eng.flat.data_ptr(), eng.grad.data_ptr(), self.square_avg.data_ptr(), n,
             self._partials.data_ptr(), scale, max_norm, float(g["lr"]), float(g["alpha"]), float(g["eps"]),
             self._norm.data_ptr(), gi, gd, sk, s)


class A2C_ACKTR(GuardedUpdate):
    def __init__(self,
                 actor_critic,
                 value_loss_coef,
                 entropy_coef,
                 lr=None,
                 eps=None,
                 alpha=None,
                 max_grad_norm=None,
                 acktr=False):
        if acktr:
            raise NotImplementedError("ACKTR (the K-FAC optimizer) is outside the MI355X engine's scope; "
                                      "use acktr=False (A2C) or algo.PPO")
        self.actor_critic = actor_critic
        self.acktr = acktr
        self.value_loss_coef = value_loss_coef
        self.entropy_coef = entropy_coef
        self.max_grad_norm = max_grad_norm
        self.optimizer = FlatRMSprop(actor_critic.parameters(), lr, eps=eps, alpha=alpha,
                                     max_grad_norm=max_grad_norm)
        if _dist.active():
            # one-time parameter broadcast so every rank starts from rank 0's weights
            eng = actor_critic.hip_engine()
            _dist.broadcast_params(eng.flat)
            eng.epoch += 1

    def update(self, rollouts):
        eng = self.actor_critic.hip_engine()
        self._begin_update(eng)   # zeroes the loss sums, arms the device guards of the clip + RMSprop
        hp = {"loss": "a2c", "value_coef": float(self.value_loss_coef), "entropy_coef": float(self.entropy_coef)}
        num_steps, num_processes = rollouts.rewards.size()[0:2]
        if self.actor_critic.is_recurrent:
            # :38-43 evaluate_actions on recurrent_hidden_states[0] and masks[:-1]: every env, in order
            envs = torch.arange(num_processes, device=eng.device)
            eng.train_minibatch_rec(rollouts, None, envs, hp, self._loss_acc, self.optimizer)
        else:
            idx = torch.arange(num_steps * num_processes, device=eng.device)
            eng.train_minibatch(rollouts, None, idx, hp, self._loss_acc, self.optimizer)
        return self._finish_update("A2C_ACKTR.update", 1, 1)
