"""What FlatAdam (algo/ppo.py) and FlatRMSprop (algo/a2c_acktr.py) share: a
torch.optim-compatible façade over the engine's one flat parameter buffer.

A step is: all-reduce of the flat gradient (world_size > 1) -> Σg² partials ->
one fused clip + update kernel, skipped on the device when a guard is set.  A
subclass names its state buffers (STATE, each a flat fp32 tensor the size of the
parameters, zero before the first step), what to call them in an error message,
and launches its kernel in _apply().
"""
import torch

from .. import _dist
from .._hip import call, stream


class FlatOptimizer(object):
    STATE = ()          # attribute names of the state buffers, in state_dict order
    NAME = "optimizer"  # "<NAME> state holds ..." when the state has another size
    NOUN = "values"

    def __init__(self, params, group, max_grad_norm=None):
        self.param_groups = [dict({"params": list(params)}, **group)]
        self.max_grad_norm = max_grad_norm
        self.step_count = 0
        for k in self.STATE:
            setattr(self, k, None)
        self._partials = None
        self.last_grad_norm = None
        self._norm = None
        # (int32 [1] error word, float64 [1] bad-action count, int* skipped-step count)
        # set by the update: a guarded step is skipped on the device (on every rank
        # when any rank's guard is set, _dist.global_guard)
        self.guard = None
        self._gflag = None

    def zero_grad(self, set_to_none=False):
        for p in self.param_groups[0]["params"]:
            if p.grad is not None:
                p.grad.zero_()

    def _bind_state(self, eng):
        n = eng.numel
        state = [getattr(self, k) for k in self.STATE]
        if state[0] is None:
            for k in self.STATE:
                setattr(self, k, torch.zeros(n, device=eng.device))
        elif any(t is None or t.numel() != n for t in state):
            raise RuntimeError(f"{self.NAME} state holds {state[0].numel()} {self.NOUN} for {n} parameters "
                               "(optimizer state of a different policy?)")
        elif any(t.device != eng.device for t in state):
            # restored on another device (e.g. a checkpoint loaded before .to(device)):
            # keep the state — the step count assumes it
            for k, t in zip(self.STATE, state):
                setattr(self, k, t.to(eng.device, torch.float32).contiguous())

    def _step_flat(self, eng):
        """all-reduce (G>1) -> Σg² partials -> fused clip + update on eng.flat."""
        n = eng.numel
        self._bind_state(eng)
        if self._partials is None or self._partials.device != eng.device:   # also after load_state_dict
            self._partials = torch.empty(call("ppo_grad_partials_count", n), dtype=torch.float64, device=eng.device)
            self._norm = torch.zeros(1, dtype=torch.float64, device=eng.device)
        scale = _dist.allreduce_grads(eng.grad)   # (waits for the fc + heads bucket the backward started)
        self.step_count += 1
        s = stream()
        call("ppo_grad_sumsq", eng.grad.data_ptr(), n, scale, self._partials.data_ptr(), s)
        mn = self.max_grad_norm if self.max_grad_norm is not None else -1.0
        gi = gd = sk = None
        if self.guard is not None:
            err, bad, sk = self.guard
            if _dist.active():
                # the gradient is already summed over ranks: any rank's failure skips the
                # step on every rank (one 8-byte all-reduce), so all ranks stay identical
                if self._gflag is None or self._gflag.device != eng.device:
                    self._gflag = torch.zeros(1, dtype=torch.float64, device=eng.device)
                gd = _dist.global_guard(err, bad, self._gflag).data_ptr()
            else:
                gi, gd = err.data_ptr(), bad.data_ptr()
        self._apply(eng, n, scale, float(mn), gi, gd, sk, s)

    def _apply(self, eng, n, scale, max_norm, gi, gd, sk, s):
        raise NotImplementedError

    def state_dict(self):
        sd = {"step": self.step_count}
        sd.update((k, getattr(self, k)) for k in self.STATE)
        sd["param_groups"] = [{k: v for k, v in self.param_groups[0].items() if k != "params"}]
        return sd

    def load_state_dict(self, sd):
        self.step_count = int(sd["step"])
        for k in self.STATE:
            setattr(self, k, sd[k])
        self.param_groups[0].update(sd["param_groups"][0])


class GuardedUpdate(object):
    """The device-guard protocol of an update (PPO.update, A2C_ACKTR.update): loss_acc holds
    {value loss, action loss, entropy} sums, the count of stored actions outside [0, A)
    (Box: of rows with a non-finite stored action; MultiBinary: of rows with a component
    that is not 0 or 1), and (filled at the end) the persistent-GRU timeout flag.  The
    class using it has actor_critic and optimizer."""

    _loss_acc = None

    def _begin_update(self, eng):
        if self._loss_acc is None or self._loss_acc.device != eng.device:
            self._loss_acc = torch.zeros(5, dtype=torch.float64, device=eng.device)
        else:
            self._loss_acc.zero_()
        # device guards of every clip + optimizer step of this update: a persistent-GRU
        # timeout (status[0]) or an out-of-range stored action (loss_acc[3]) turns the step
        # into a no-op on the device, counted in status[1]; _finish_update() raises
        eng.status[:2].zero_()
        self.optimizer.guard = (eng.status[0:1], self._loss_acc[3:4], eng.status_ptr(1))

    def _finish_update(self, name, num_updates, passes):
        """-> the three mean losses; raises what the reference would have.  passes: how
        often the update visits each stored row (PPO: ppo_epoch)."""
        eng = self.actor_critic.hip_engine()
        self._loss_acc[4].copy_(eng.status[0])    # the timeout flag travels with the losses (one all-reduce):
        _dist.allreduce_losses(self._loss_acc)     # every rank sees any rank's failure and raises with it
        acc = self._loss_acc.tolist()                              # one D2H per update
        self.optimizer.guard = None
        if acc[3] > 0 or acc[4] > 0:
            # the guarded steps were no-ops on the device: undo their step count so the
            # parameters, optimizer state and step counter are those of the last good step
            self.optimizer.step_count -= int(eng.status[1].item())
            eng.status[:2].zero_()
        if acc[4] > 0:
            # a persistent GRU sequence kernel gave up a bounded wait: no step used its outputs
            raise RuntimeError("{}: persistent GRU kernel timed out; the optimizer steps from that "
                               "minibatch on were skipped (ppo_gru_persist_set(0) selects the step "
                               "launches)".format(name))
        if acc[3] > 0 and getattr(eng, "gauss", False):
            # Box: a NaN / inf action makes every gradient of its minibatch non-finite
            raise ValueError("{}: {:.0f} non-finite stored action(s) in the rollout".format(
                name, acc[3] * _dist.world_size() / passes))
        if acc[3] > 0 and getattr(eng, "dist_kind", "cat") == "bern":
            # MultiBinary: torch's Bernoulli.log_prob raises ValueError for a value outside {0, 1}
            raise ValueError("{}: {:.0f} stored action(s) with a component that is not 0 or 1 in the "
                             "rollout".format(name, acc[3] * _dist.world_size() / passes))
        if acc[3] > 0:
            # the reference's log_probs gather (distributions.py:22) raises on such an index, before
            # its optimizer step; each pass visits every stored row once, hence / passes
            raise IndexError("{}: {:.0f} stored action(s) outside [0, {}) in the rollout".format(
                name, acc[3] * _dist.world_size() / passes, eng.A))
        return tuple(x / num_updates for x in acc[:3])
