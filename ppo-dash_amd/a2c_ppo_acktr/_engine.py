"""HIP execution engines behind Policy / PPO.

CNNEngine        CNNBase, feed-forward (model.py:169-199)
RecurrentEngine  CNNBase + [vector obs] + GRU (model.py:89-166, 192-199)
MLPEngine           MLPBase, feed-forward (model.py:202-234)
RecurrentMLPEngine  MLPBase + GRU in front of the towers (model.py:111-166, 224-234)

_Engine is their common base: the flat parameter / gradient buffers (every
nn.Parameter of the Policy is re-pointed to a view of one contiguous fp32 buffer,
so clip + Adam is one pass), the pack cache, the grow-only workspaces, the RNG
counter, the status words and the policy heads.  CNNEngine and MLPEngine are
siblings under it; _GRU holds the recurrent path both recurrent engines share.

Per PPO minibatch (every box is a libppo_hip.so kernel):
  conv1(obs rows gathered by index, u8) -> conv2 -> conv3 -> fc       (MFMA fwd)
  [recurrent: concat vector obs -> gi = x·W_ihᵀ -> T x fused GRU step]
  heads_train (value/logits/Categorical/PPO loss + dL/dlogits, dL/dfeature)
  [recurrent: T x (gate grads, dh·W_hh), dW_hh, dW_ih, dx]
  fc dgrad | fc wgrad | conv3 dgrad | conv3 wgrad | conv2 dgrad | conv2 wgrad | conv1 wgrad
  wgrad slab reduces -> flat grad  [RCCL all-reduce when world_size > 1]
  grad Σg² -> clip + Adam -> pack weights
"""
import collections
import contextlib

import os

import torch

from . import _dist
from ._hip import call, ptr, stream
from .distributions import Bernoulli, DiagGaussian

# ppo_trunk_fwd (conv1 -> conv2 -> conv3 in one launch) for u8 rows; PPO_FUSED_TRUNK=0
# runs the three launches (same-box A/B, tools/ab_bench.sh)
FUSED_TRUNK = os.environ.get("PPO_FUSED_TRUNK", "1") != "0"
FEAT = 32 * 7 * 7  # conv3 output, flattened


def _with_precision(fn):
    """Run an engine entry point at the policy's arithmetic precision: the split
    GEMMs' part-product count is 6 (fp32-accurate) normally and 1 — bf16-rounded
    operands, fp32 accumulation — after Policy.half() (T/run.py:84-85)."""
    def wrapper(self, *args, **kwargs):
        if not getattr(self.policy, "_half_mode", False):
            return fn(self, *args, **kwargs)
        prev = call("ppo_tune_get", b"products")
        if prev != 1:
            call("ppo_tune_set", b"products", 1)
        try:
            return fn(self, *args, **kwargs)
        finally:
            if prev != 1:
                call("ppo_tune_set", b"products", prev)
    wrapper.__name__, wrapper.__doc__ = fn.__name__, fn.__doc__
    return wrapper


class _Workspace:
    def __init__(self):
        self.bufs = {}
        self.version = 0   # bumped by every (re)allocation: a captured graph's buffers moved

    def get(self, name, numel, dtype=torch.float32, device=None):
        t = self.bufs.get(name)
        if t is None or t.numel() < numel or t.dtype != dtype or t.device != device:
            t = torch.empty(max(int(numel), 1), dtype=dtype, device=device)
            self.bufs[name] = t
            self.version += 1
        return t


# What tells the three heads kernel families apart on the host: the entry points (train:
# PPO's row loss, train_a2c: A2C's, same kernels and partials), whether
# DiagGaussian's logstd (parameter LS; its gradient doubles the bias partials) is passed
# after BA, and the action dtype.  Bernoulli's partials have Categorical's layouts, so
# ppo_heads_reduce sums both.
_HeadKind = collections.namedtuple("_HeadKind", "act train train_a2c reduce ls dtype")
_HEADS = {
    "cat": _HeadKind("ppo_heads_act", "ppo_heads_train", "ppo_heads_train_a2c", "ppo_heads_reduce", False,
                     torch.int64),
    "gauss": _HeadKind("ppo_heads_gauss_act", "ppo_heads_gauss_train", "ppo_heads_gauss_train_a2c",
                       "ppo_heads_gauss_reduce", True, torch.float32),
    "bern": _HeadKind("ppo_heads_bern_act", "ppo_heads_bern_train", "ppo_heads_bern_train_a2c", "ppo_heads_reduce",
                      False, torch.float32),
}


class _Engine:
    """What the four engines share.  A subclass __init__ sets its dimensions (H among them; A
    comes from the distribution), checks its limits and then calls this one; the subclass
    provides _pack_weights() and the parameter indices WC, BC, WA, BA, LS of the heads."""

    recurrent = False
    is_mlp = False   # 1-D observations (MLPBase) instead of [C,84,84] images

    def __init__(self, policy, device):
        self.policy = policy
        self.device = device
        self._bind_dist(policy)
        self.params = list(policy.parameters())
        self.ws = {"act": _Workspace(), "train": _Workspace()}
        self.act_ws = "act"   # workspace of the forward (act / get_value / evaluate) paths
        self.packed = None
        self._packed_key = None
        self.epoch = 0  # bumped by every in-place parameter write done by HIP kernels
        self._flatten()
        self.rng_seed = int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF
        self.rng_counter = 0
        # device status words: [0] persistent-GRU timeout of the running update
        # (sticky; gates clip + Adam), [1] optimizer steps skipped by a guard,
        # [2] persistent-GRU timeout of evaluate_sequence
        self.status = torch.zeros(4, dtype=torch.int32, device=self.device)
        self._rng_dev = None      # the sampling counter as a device word (rng_dev), allocated at first use
        self._device_counter = False

    def _bind_dist(self, policy):
        """Categorical or Bernoulli (dist.linear) or DiagGaussian (dist.fc_mean,
        dist.logstd._bias): the distribution's parameters are the last in
        policy.parameters() order."""
        self.dist_kind = ("gauss" if isinstance(policy.dist, DiagGaussian) else
                          "bern" if isinstance(policy.dist, Bernoulli) else "cat")
        self._head = _HEADS[self.dist_kind]
        self.gauss = self.dist_kind == "gauss"
        self.float_actions = self.dist_kind != "cat"   # float [B, A] actions (Box, MultiBinary)
        self.A = (policy.dist.fc_mean if self.gauss else policy.dist.linear).weight.shape[0]

    @property
    def rng_dev(self):
        """The sampling counter as one 8-byte word in device memory: what the kernels of a
        captured HIP graph read (a launch argument would freeze in the graph)."""
        if self._rng_dev is None:
            self._rng_dev = torch.zeros(1, dtype=torch.int64, device=self.device)
        return self._rng_dev

    def set_rng_dev(self, value):
        """rng_dev = value mod 2^64, as a stream-ordered fill"""
        v = int(value) & 0xFFFFFFFFFFFFFFFF
        self.rng_dev.fill_(v - (1 << 64) if v >> 63 else v)   # the int64 tensor holds the same 64 bits

    @contextlib.contextmanager
    def using_device_counter(self):
        """Inside, the heads read the sampling counter from rng_dev (the _dc entry points)
        and a launch of its own advances the word by one after them; the host rng_counter
        is left alone.  The caller keeps the two in step (evaluation.GraphedActor)."""
        prev, self._device_counter = self._device_counter, True
        try:
            yield self.rng_dev
        finally:
            self._device_counter = prev

    def status_ptr(self, i):
        return self.status.data_ptr() + 4 * i

    # ------------------------------------------------------------ parameters
    def _flatten(self):
        n = sum(p.numel() for p in self.params)
        flat = torch.empty(n, device=self.device)
        grad = torch.zeros(n, device=self.device)
        off = 0
        self.offsets = []
        with torch.no_grad():
            for p in self.params:
                k = p.numel()
                flat[off:off + k].copy_(p.data.reshape(-1))
                p.data = flat[off:off + k].view_as(p)
                p.grad = grad[off:off + k].view_as(p)
                self.offsets.append(off)
                off += k
        self.flat, self.grad, self.numel = flat, grad, n
        self.epoch += 1

    @contextlib.contextmanager
    def using_workspace(self, name):
        """Route the forward paths through workspace `name` (e.g. a captured HIP
        graph's own buffers, which no eager call may reallocate)."""
        self.ws.setdefault(name, _Workspace())
        prev, self.act_ws = self.act_ws, name
        try:
            yield self.ws[name]
        finally:
            self.act_ws = prev

    def is_bound(self):
        base = self.flat.data_ptr()
        for p, off in zip(self.params, self.offsets):
            if p.data.data_ptr() != base + 4 * off or not p.is_cuda:
                return False
        return True

    def ensure_bound(self):
        if not self.is_bound():
            self._flatten()

    def pv(self, i):
        """raw pointer of parameter i (in policy.parameters() order)"""
        return self.flat.data_ptr() + 4 * self.offsets[i]

    def gv(self, i):
        return self.grad.data_ptr() + 4 * self.offsets[i]

    def pack_key(self):
        """changes whenever a parameter was written: by torch (the tensors' versions) or in
        place by a HIP kernel (epoch)"""
        return (sum(p._version for p in self.params), self.epoch)

    def pack(self, force=False):
        """Refresh the packed weight planes (_pack_weights) if the parameters changed."""
        key = self.pack_key()
        if not force and self.packed is not None and key == self._packed_key:
            return
        self._pack_weights()
        self._packed_key = key

    # ------------------------------------------------------------------ heads
    def _heads(self, h, B, deterministic=False, noise=None, given=None, want_entropy=False, value_only=False,
               hv=None):
        kind = self._head
        value = torch.empty(B, 1, device=self.device)
        if value_only:
            action = logp = ent = None
        else:
            action = given if given is not None else torch.empty(B, self.A if self.float_actions else 1,
                                                                 dtype=kind.dtype, device=self.device)
            logp = torch.empty(B, 1, device=self.device)
            ent = torch.empty(B, device=self.device) if want_entropy else None
        if noise is not None:
            noise = noise.to(self.device, torch.float32).contiguous()
            if noise.shape != (B, self.A):
                raise RuntimeError(f"noise must be [{B},{self.A}]")
        if self._device_counter:   # using_device_counter(): the word, advanced by a launch after the heads
            counter, dc = self.rng_dev.data_ptr(), "_dc"
        else:
            self.rng_counter += 1
            counter, dc = self.rng_counter, ""
        if self.float_actions and given is not None and given.numel() != B * self.A:
            raise RuntimeError(f"actions must be [{B},{self.A}], got {tuple(given.shape)}")
        call(kind.act + dc, h.data_ptr(), ptr(hv), B, self.H, self.pv(self.WC), self.pv(self.BC),
             self.pv(self.WA), self.pv(self.BA), *((self.pv(self.LS),) if kind.ls else ()), self.A, ptr(noise),
             self.rng_seed, counter, int(bool(deterministic)),
             ptr(given.reshape(-1).contiguous() if given is not None else None, kind.dtype, "action"),
             value.data_ptr(), None if given is not None or value_only else action.data_ptr(),
             ptr(logp), ptr(ent), stream())
        if self._device_counter:
            call("ppo_rng_advance", self.rng_dev.data_ptr(), 1, stream())
        return value, action, logp, ent

    def mean(self, x):
        """model.py:77 dist.entropy().mean() on the device (0-d tensor)"""
        out = torch.empty((), device=self.device)
        call("ppo_mean_f32", x.data_ptr(), x.numel(), out.data_ptr(), stream())
        return out

    # --------------------------------------------------------------- training
    def _heads_train(self, storage, adv, idx, feat, B, hp, loss_acc, dfeat, feat_act, feat_v=None, dfeat_v=None):
        ws, dev, H, A, s, kind = self.ws["train"], self.device, self.H, self.A, stream(), self._head
        nblk = call("ppo_heads_train_blocks", B)
        part_w = ws.get("part_w", nblk * (1 + A) * H, device=dev)
        part_b = ws.get("part_b", nblk * (1 + (2 * A if kind.ls else A)), device=dev)
        part_l = ws.get("part_l", nblk * 4, device=dev)
        inv_b = 1.0 / B
        a2c = hp.get("loss") == "a2c"   # A2C_ACKTR.update: adv is None, the kernel forms returns - value itself
        clipped = 0 if a2c else int(hp["use_clipped_value_loss"])
        if self.float_actions and storage.actions.shape[-1] != A:
            raise RuntimeError(f"storage holds {storage.actions.shape[-1]} action dimensions, the policy {A}")
        actions = (ptr(storage.actions, kind.dtype, "storage.actions") if self.float_actions
                   else storage.actions.data_ptr())
        # what the row loss reads of the storage and its hyper-parameters: PPO's old log-probs,
        # advantages, value predictions, returns, clip and clipped-value flag; A2C's returns
        planes = ((storage.returns.data_ptr(),) if a2c else
                  (storage.action_log_probs.data_ptr(), adv.data_ptr(), storage.value_preds.data_ptr(),
                   storage.returns.data_ptr(), hp["clip"]))
        call(kind.train_a2c if a2c else kind.train, feat.data_ptr(), ptr(feat_v), B, H, self.pv(self.WC),
             self.pv(self.BC), self.pv(self.WA), self.pv(self.BA), *((self.pv(self.LS),) if kind.ls else ()), A,
             idx.data_ptr(), 0, actions, *planes, hp["value_coef"], hp["entropy_coef"], inv_b,
             *(() if a2c else (clipped,)), int(feat_act), dfeat.data_ptr(), ptr(dfeat_v), part_w.data_ptr(),
             part_b.data_ptr(), part_l.data_ptr(), s)
        # ppo_heads_gauss_reduce also writes logstd's gradient and takes no clipped-value flag
        call(kind.reduce, part_w.data_ptr(), part_b.data_ptr(), part_l.data_ptr(), nblk, H, A,
             self.gv(self.WC), self.gv(self.BC), self.gv(self.WA), self.gv(self.BA),
             *((self.gv(self.LS),) if kind.ls else ()), loss_acc.data_ptr(), inv_b, 1.0,
             *(() if kind.ls else (clipped,)), s)

    def _dense_wgrad(self, dy, x, R, N, K, kind, a, wi, bi):
        """dW[n][k] = Σ_r dy[r][n] x[r][k] (+ bias) -> grad planes wi, bi"""
        ws, dev, s = self.ws["train"], self.device, stream()
        tiles = ((N + 127) // 128) * ((K + 127) // 128)
        Z = call("ppo_wgrad_splits", R, tiles, 2048, 16)
        slab = ws.get("slab", Z * N * K, device=dev)
        slab_b = ws.get("slab_b", Z * N, device=dev)
        call("ppo_linear_wgrad", dy.data_ptr(), x.data_ptr(), R, N, K, Z, slab.data_ptr(), slab_b.data_ptr(), s)
        call("ppo_wgrad_reduce", slab.data_ptr(), slab_b.data_ptr(), Z, N, K, kind, a, 0, self.gv(wi), self.gv(bi),
             1.0, 0, s)

    def _finish_step(self, optimizer):
        optimizer._step_flat(self)
        self.epoch += 1
        self.pack(force=True)


class CNNEngine(_Engine):
    """Binds to a Policy whose base is a non-recurrent CNNBase."""

    # parameter indices in policy.parameters() order (named_parameters order)
    W1, B1, W2, B2, W3, B3, W4, B4, WC, BC, WA, BA, LS = range(13)   # LS: DiagGaussian's logstd (Box only)

    def __init__(self, policy, device):
        base = policy.base
        self.C = base.main[0].weight.shape[1]
        self.H = base.main[7].weight.shape[0]
        if self.H > 512 or self.H % 4 != 0:
            raise NotImplementedError(f"hidden_size {self.H}: the HIP engine supports multiples of 4 up to 512")
        if not self.recurrent and base.critic_linear.weight.shape[1] != self.H:
            raise NotImplementedError("vector observations with a non-recurrent CNNBase are not supported "
                                      "(the reference crashes there too: Categorical expects hidden_size inputs)")
        self.obs_decode = None   # (mean fp32 [84][84][3] device tensor | None, std) for raw u8 RGB frames
        self._n_cu = None   # CU count of the device, read at the first weight gradient
        self._mask_rows = None   # rows of the training forward whose ReLU mask bits the train workspace holds
        # weight gradients per layer: gradient rows M and columns NW, ppo_wgrad_reduce's (kind, ka, kb),
        # weight / bias parameter, reduction rows per sample, output tiles
        self._wgrad_layers = {
            "conv1": (32, self.C * 64, 0, 0, 0, self.W1, self.B1, 400, 1),
            "conv2": (64, 512, 1, 4, 32, self.W2, self.B2, 81, 4),
            "conv3": (32, 576, 1, 3, 64, self.W3, self.B3, 49, 5),
            "fc": (self.H, FEAT, 2, 32, 49, self.W4, self.B4, 1, ((self.H + 127) // 128) * 13),
        }
        super().__init__(policy, device)

    def _pack_weights(self):
        if self.packed is None:
            self.packed = torch.empty(call("ppo_packed_weights_size", self.H), device=self.device)
            offs = torch.zeros(6, dtype=torch.int64)
            call("ppo_packed_offsets", self.H, offs.data_ptr())
            self.poff = [int(x) for x in offs]
        call("ppo_pack_weights", self.pv(self.W2), self.pv(self.W3), self.pv(self.W4), self.H,
             self.packed.data_ptr(), stream())

    def pk(self, seg):
        """pointer to packed segment: 0 W2p 1 W3p 2 W4p 3 W4T 4 W3d 5 W2d"""
        return self.packed.data_ptr() + 4 * self.poff[seg]

    # ---------------------------------------------------------------- forward
    @staticmethod
    def _obs_args(obs):
        if obs.dtype == torch.uint8:
            return 1
        if obs.dtype == torch.float32:
            return 0
        raise TypeError(f"observations must be uint8, float32 or float16, got {obs.dtype}")

    @staticmethod
    def _is_rgb(obs):
        """raw u8 RGB frames [..., 84, 84, 3] (decoded inside conv1 by obs_decode)"""
        return obs.dtype == torch.uint8 and tuple(obs.shape[-3:]) == (84, 84, 3)

    def set_obs_decode(self, mean, std):
        """NormalizeWrapper + FrameStackMono(2) of raw RGB frames, fused into conv1:
        mean (fp32-representable [84][84][3], or None) and std (u/255: None, 255)."""
        if self.C != 4:
            raise NotImplementedError("the fused RGB decode produces FrameStackMono(2)'s 4 channels (C = 4)")
        if mean is not None:
            m64 = torch.as_tensor(mean, dtype=torch.float64).reshape(84, 84, 3)
            m32 = m64.to(torch.float32)
            if not torch.equal(m32.to(torch.float64), m64):
                raise ValueError("the fused decode needs fp32-representable means (NormalizeWrapper's files hold "
                                 "fp32 values); use ObsPreprocess into fp32 storage otherwise")
            mean = m32.contiguous().to(self.device)
        if not float(std):
            raise ValueError("std must be non-zero")
        self.obs_decode = (mean, float(std))

    def _conv1(self, obs, idx, B, a1, m1, s):
        """conv1 (+ ReLU, + mask bits when m1 is given) of B rows of obs"""
        if self._is_rgb(obs):
            if self.obs_decode is None:
                raise TypeError("raw u8 RGB frames need the fused decode: Policy.set_obs_decode(ObsPreprocess)")
            mean, std = self.obs_decode
            call("ppo_conv1_fwd_rgb", obs.data_ptr(), ptr(idx, torch.int64, "idx"), 0, B, ptr(mean), std,
                 self.pv(self.W1), self.pv(self.B1), a1.data_ptr(), ptr(m1), s)
        elif m1 is not None:
            call("ppo_conv1_fwd_mask", obs.data_ptr(), self._obs_args(obs), ptr(idx, torch.int64, "idx"), 0, self.C,
                 B, self.pv(self.W1), self.pv(self.B1), a1.data_ptr(), m1.data_ptr(), s)
        else:
            call("ppo_conv1_fwd", obs.data_ptr(), self._obs_args(obs), ptr(idx, torch.int64, "idx"), 0, self.C, B,
                 self.pv(self.W1), self.pv(self.B1), a1.data_ptr(), s)

    def _obs_f32(self, obs, idx, B, ws):
        """fp16 observations (RolloutStorage.half(), storage.py:48-58): the rows the
        trunk reads (idx into the plane, or the batch) converted to an fp32
        workspace; u8 / fp32 observations pass through."""
        if obs.dtype != torch.float16:
            return obs, idx
        x = ws.get("obs32", B * self.C * 84 * 84, device=self.device)
        call("ppo_gather_f16_to_f32", obs.data_ptr(), ptr(idx, torch.int64, "idx"), x.data_ptr(), B,
             self.C * 84 * 84, stream())
        return x, None

    def trunk(self, obs, idx, B, ws, out=None, ldo=None):
        """conv1..fc on B samples: obs is either a [B,C,84,84] batch (idx None) or the
        storage plane whose rows idx[b] are gathered inside conv1.  Writes the fc
        output (post-ReLU) to `out` (row stride ldo) or a workspace [B,H]."""
        dev = self.device
        obs, idx = self._obs_f32(obs, idx, B, ws)
        a1 = ws.get("a1", B * 400 * 32, device=dev)
        a2 = ws.get("a2", B * 81 * 64, device=dev)
        a3 = ws.get("a3", B * FEAT, device=dev)
        if out is None:
            out, ldo = ws.get("h", B * self.H, device=dev), self.H
        s = stream()
        train = ws is self.ws["train"]
        # training forward: conv1 and conv2 also write their ReLU masks as bits,
        # read by the conv2 / conv3 dgrads instead of the fp32 activations
        # (and conv3's, read by the fc dgrad instead of a3)
        m1 = ws.get("m1bits", B * 400, dtype=torch.int32, device=dev) if train else None
        m2 = ws.get("m2bits", B * 81, dtype=torch.int64, device=dev) if train else None
        m3 = ws.get("m3bits", B * 49, dtype=torch.int32, device=dev) if train else None
        if obs.dtype == torch.uint8 and self.C == 4 and not self._is_rgb(obs) and FUSED_TRUNK and not train:
            # u8 rows: conv1 -> conv2 -> conv3 in one persistent launch (ppo_trunk_fwd)
            call("ppo_trunk_fwd", obs.data_ptr(), ptr(idx, torch.int64, "idx"), 0, B, self.pv(self.W1),
                 self.pv(self.B1), a1.data_ptr(), None, self.pk(0), self.pv(self.B2), a2.data_ptr(), None,
                 self.pk(1), self.pv(self.B3), a3.data_ptr(), s)
        else:
            self._conv1(obs, idx, B, a1, m1[:B * 400] if train else None, s)
            if train:
                call("ppo_conv2_fwd_mask", a1.data_ptr(), B, self.pk(0), self.pv(self.B2), a2.data_ptr(),
                     m2.data_ptr(), s)
                call("ppo_conv3_fwd_mask", a2.data_ptr(), B, self.pk(1), self.pv(self.B3), a3.data_ptr(),
                     m3.data_ptr(), s)
            else:
                call("ppo_conv2_fwd", a1.data_ptr(), B, self.pk(0), self.pv(self.B2), a2.data_ptr(), s)
                call("ppo_conv3_fwd", a2.data_ptr(), B, self.pk(1), self.pv(self.B3), a3.data_ptr(), s)
        if train:
            self._mask_rows = B
        nb = call("ppo_fc_fwd_ws_bytes", B, self.H)   # rollout-sized B: split-K into a workspace slab
        if nb:
            fws = ws.get("fc_ws", nb // 4, device=dev)
            call("ppo_fc_fwd_ws", a3.data_ptr(), B, self.pk(2), self.pv(self.B4), self.H, out.data_ptr(), ldo,
                 fws.data_ptr(), nb, s)
        else:
            call("ppo_fc_fwd", a3.data_ptr(), B, self.pk(2), self.pv(self.B4), self.H, out.data_ptr(), ldo, s)
        return out

    def _check_obs(self, obs):
        obs = obs if obs.is_cuda else obs.to(self.device)
        if self.obs_decode is not None and self._is_rgb(obs) and obs.dim() == 4:
            return obs.contiguous()
        if tuple(obs.shape[1:]) != (self.C, 84, 84):
            raise RuntimeError(f"CNNBase expects [N,{self.C},84,84] observations"
                               + (" or raw [N,84,84,3] u8 frames" if self.obs_decode is not None else "")
                               + f", got {tuple(obs.shape)}")
        return obs.contiguous()

    @_with_precision
    def act(self, obs, deterministic=False, noise=None, given=None, want_entropy=False, value_only=False,
            vec=None, hxs=None, masks=None):
        """vec, hxs and masks are accepted for the engines' common signature and not used."""
        self.ensure_bound()
        self.pack()
        obs = self._check_obs(obs)
        B = obs.shape[0]
        h = self.trunk(obs, None, B, self.ws[self.act_ws])
        return self._heads(h, B, deterministic, noise, given, want_entropy, value_only)

    # --------------------------------------------------------------- training
    def _trunk_backward(self, B, dh, obs, idx):
        """dh: dL/d(fc pre-activation) [B,H] (ReLU mask applied) -> trunk gradients.  The dgrads
        read the ReLU mask bits that trunk() wrote on the train workspace for the same B rows."""
        if self._mask_rows != B:
            raise RuntimeError(f"_trunk_backward of {B} rows: the train workspace holds the ReLU masks of "
                               f"{self._mask_rows} (trunk() runs on it first)")
        ws, dev, s = self.ws["train"], self.device, stream()
        a1, a2, a3 = ws.bufs["a1"], ws.bufs["a2"], ws.bufs["a3"]
        dz3 = ws.get("dz3", B * FEAT, device=dev)
        dz2 = ws.get("dz2", B * 81 * 64, device=dev)
        dz1 = ws.get("dz1", B * 400 * 32, device=dev)
        call("ppo_fc_dgrad_bits", dh.data_ptr(), B, self.H, self.pk(3), ws.bufs["m3bits"].data_ptr(),
             dz3.data_ptr(), s)
        self._wgrad("fc", B, 1.0, s, "ppo_linear_wgrad", dh.data_ptr(), a3.data_ptr(), B, self.H, FEAT)
        # the fc + heads tail of the flat gradient (the last parameters in torch order,
        # 92 % of the bytes at H = 512) is final here: its all-reduce (G > 1) overlaps
        # the conv backward on a side stream (_dist.start_bucket); PPO's step waits for it
        _dist.start_bucket(self.grad[self.offsets[self.W4]:])
        call("ppo_conv3_dgrad_bits", dz3.data_ptr(), B, self.pk(4), ws.bufs["m2bits"].data_ptr(), dz2.data_ptr(), s)
        self._wgrad("conv3", B, 1.0, s, "ppo_conv3_wgrad", dz3.data_ptr(), a2.data_ptr(), B)
        call("ppo_conv2_dgrad_bits", dz2.data_ptr(), B, self.pk(5), ws.bufs["m1bits"].data_ptr(), dz1.data_ptr(), s)
        self._wgrad("conv2", B, 1.0, s, "ppo_conv2_wgrad", dz2.data_ptr(), a1.data_ptr(), B)
        if obs.dtype == torch.float16:   # the rows trunk() converted for this minibatch
            obs, idx = ws.bufs["obs32"], None
        if self._is_rgb(obs):   # decoded to fp32 by the kernel
            mean, std = self.obs_decode
            self._wgrad("conv1", B, 1.0, s, "ppo_conv1_wgrad_rgb", dz1.data_ptr(), obs.data_ptr(), ptr(idx), 0, B,
                        ptr(mean), std)
        else:   # u8 4-channel observations are staged as integers: 1/255 in the reduce
            self._wgrad("conv1", B, 1.0 / 255.0 if obs.dtype == torch.uint8 else 1.0, s, "ppo_conv1_wgrad",
                        dz1.data_ptr(), obs.data_ptr(), self._obs_args(obs), ptr(idx), 0, self.C, B)

    def _wgrad(self, layer, B, scale, s, entry, *args):
        """Weight + bias gradient of one trunk layer: `entry(*args, Z, slab, slab_b, s)` writes Z
        split-K partials, ppo_wgrad_reduce sums them (times scale) into the flat gradient."""
        M, NW, kind, ka, kb, wi, bi, rows, tiles = self._wgrad_layers[layer]
        ws, dev = self.ws["train"], self.device
        # the image-resident conv wgrad kernels walk any number of images per block:
        # one block per CU (their LDS allows no more) — measured conv3 0.80 -> 0.70 ms,
        # conv1 / conv2 -1 %, and 2-8x fewer split-K slabs to reduce
        if self._n_cu is None:
            self._n_cu = torch.cuda.get_device_properties(self.device).multi_processor_count
        target = 2048 if layer == "fc" else max(self._n_cu, -(-B // 512)) * tiles
        Z = call("ppo_wgrad_splits", B * rows, tiles, target, 16)
        slab = ws.get("slab", Z * M * NW, device=dev)
        slab_b = ws.get("slab_b", Z * M, device=dev)
        call(entry, *args, Z, slab.data_ptr(), slab_b.data_ptr(), s)
        call("ppo_wgrad_reduce", slab.data_ptr(), slab_b.data_ptr(), Z, M, NW, kind, ka, kb, self.gv(wi), self.gv(bi),
             scale, 0, s)

    @_with_precision
    def train_minibatch(self, storage, adv, idx, hp, loss_acc, optimizer):
        """Forward + backward + (all-reduce) + clip + Adam for one minibatch of
        storage rows idx (int64 [B], device)."""
        self.ensure_bound()
        self.pack()
        _dist.begin_minibatch()
        B = idx.numel()
        ws = self.ws["train"]
        h = self.trunk(storage.obs, idx, B, ws)
        dh = ws.get("dh", B * self.H, device=self.device)
        self._heads_train(storage, adv, idx, h, B, hp, loss_acc, dh, feat_act=1)
        self._trunk_backward(B, dh, storage.obs, idx)
        self._finish_step(optimizer)


class _GRU:
    """The recurrent path of RecurrentEngine and RecurrentMLPEngine (listed before the
    feed-forward engine in their bases): act, evaluate_sequence and train_minibatch_rec
    around the GRU kernels.  The GRU's parameters come first in policy.parameters() order.
    An engine provides H, I, Ip, the packed W_hhᵀ plane `whhT` and what differs:
      _gru_in(obs, vec, idx, B, ws) -> x_pad [B][Ip], gi [B][3H]; idx None: host-facing
                                       arguments, else rows idx of the storage planes
      _gru_out(hout, B, ws)         -> the heads' (feature, value feature | None)
      _gru_out_train(...)           -> heads_train on the GRU output; returns dL/d(hout)
      _gru_in_backward(...)         -> whatever lies before the GRU input x
      _check_storage(storage)       -> raises on storage planes the engine cannot read"""

    GIH, GHH, GBI, GBH = range(4)
    recurrent = True

    def _gru_seq_fwd(self, ws, h0, masks, idx, gi, T, n, hout, status, save=False):
        """persistent whole-sequence forward of n envs; save: keep the gates for BPTT.
        status: the error word a timeout sets.  -> (save buffers | None, counters)"""
        dev, H = self.device, self.H
        sv = {k: ws.get("s_" + k, T * n * H, device=dev) if save else None for k in ("r", "z", "n", "ghn", "hin")}
        cnt = ws.get("gru_cnt", call("ppo_gru_seq_counters", n), torch.int32, dev)
        if save:
            # error word status[0]: sticky for the update, gates every clip + Adam after a timeout;
            # no gradient bucket may still be reducing on a side stream beside the persistent launch
            _dist.assert_no_pending("train_minibatch_rec")
        call("ppo_gru_seq_fwd_ws", h0.data_ptr(), masks.data_ptr(), ptr(idx), self.pv(self.GHH), self.pv(self.GBH),
             gi.data_ptr(), T, n, H, hout.data_ptr(), ptr(sv["r"]), ptr(sv["z"]), ptr(sv["n"]), ptr(sv["ghn"]),
             ptr(sv["hin"]), cnt.data_ptr(), self.status_ptr(status), stream())
        return sv, cnt

    @_with_precision
    def act(self, obs, deterministic=False, noise=None, given=None, want_entropy=False, value_only=False,
            vec=None, hxs=None, masks=None):
        """Single step (model.py:112-115): returns (value, action, logp, entropy, hxs')."""
        self.ensure_bound()
        self.pack()
        B = obs.shape[0]
        ws = self.ws[self.act_ws]
        _, gi = self._gru_in(obs, vec, None, B, ws)
        hxs = hxs.to(self.device, torch.float32).reshape(B, self.H).contiguous()
        m = masks.to(self.device, torch.float32).reshape(B).contiguous() if masks is not None else None
        hout = torch.empty(B, self.H, device=self.device)
        call("ppo_gru_step_fwd", hxs.data_ptr(), ptr(m), None, self.pv(self.GHH), self.pv(self.GBH), gi.data_ptr(),
             B, self.H, hout.data_ptr(), None, None, None, None, None, stream())
        feat, feat_v = self._gru_out(hout, B, ws)
        value, action, logp, ent = self._heads(feat, B, deterministic, noise, given, want_entropy, value_only,
                                               hv=feat_v)
        return value, action, logp, ent, hout

    @_with_precision
    def evaluate_sequence(self, obs, vec, hxs, masks, action):
        """Multi-step branch (model.py:116-165): rows are t*N + n."""
        self.ensure_bound()
        self.pack()
        R, N = obs.shape[0], hxs.shape[0]
        T = R // N
        ws = self.ws[self.act_ws]
        _, gi = self._gru_in(obs, vec, None, R, ws)
        hxs = hxs.to(self.device, torch.float32).reshape(N, self.H).contiguous()
        m = masks.to(self.device, torch.float32).reshape(R).contiguous()
        hout = torch.empty(R, self.H, device=self.device)
        self._gru_seq_fwd(ws, hxs, m, None, gi, T, N, hout, status=2)
        if int(self.status[2].item()):   # stream-ordered read of the launch's error word
            self.status[2].zero_()
            raise RuntimeError("evaluate_actions: the persistent GRU kernel timed out (its outputs are invalid; "
                               "ppo_gru_persist_set(0) selects the per-step launches)")
        given = action.to(self.device, torch.float32 if self.float_actions else torch.int64)
        feat, feat_v = self._gru_out(hout, R, ws)
        value, _, logp, ent = self._heads(feat, R, want_entropy=True, given=given, hv=feat_v)
        return value, logp, ent, hout[(T - 1) * N:]

    def _check_storage(self, storage):
        pass

    @_with_precision
    def train_minibatch_rec(self, storage, adv, envs, hp, loss_acc, optimizer):
        """recurrent_generator minibatch (storage.py:162-223): whole T-sequences of
        the n envs `envs` (int64 device), BPTT over the full T, then one Adam step."""
        H = self.H
        # before anything is touched: ppo_gather_rows reads 4 H bytes per row of the hidden states
        if storage.recurrent_hidden_states.shape[-1] != H:
            raise RuntimeError(f"storage holds hidden states of width {storage.recurrent_hidden_states.shape[-1]}, "
                               f"the policy's GRU {H}")
        self._check_storage(storage)
        self.ensure_bound()
        self.pack()
        _dist.begin_minibatch()
        dev, s = self.device, stream()
        T, N, n = storage.num_steps, storage.rewards.shape[1], envs.numel()
        R = T * n
        ws = self.ws["train"]
        idx = ws.get("ridx", R, torch.int64, dev)[:R]
        call("ppo_rec_indices", envs.data_ptr(), n, T, N, idx.data_ptr(), s)
        h0 = ws.get("h0", n * H, device=dev)
        call("ppo_gather_rows", storage.recurrent_hidden_states.data_ptr(), envs.data_ptr(), h0.data_ptr(), n,
             4 * H, s)
        x, gi = self._gru_in(storage.obs, storage.vector_obs if self.V else None, idx, R, ws)
        hout = ws.get("hout", R * H, device=dev)
        masks = storage.masks
        sv, cnt = self._gru_seq_fwd(ws, h0, masks, idx, gi, T, n, hout, status=0, save=True)
        dout = self._gru_out_train(storage, adv, idx, hout, R, hp, loss_acc)
        # backward through time
        dgi = ws.get("dgi", R * 3 * H, device=dev)
        dgh = ws.get("dgh", R * 3 * H, device=dev)
        dhz = ws.get("dhz", n * H, device=dev)
        carry = ws.get("carry", n * H, device=dev)
        # persistent BPTT on the same counters (the forward has finished on this stream) and error word
        _dist.assert_no_pending("train_minibatch_rec bptt")
        call("ppo_gru_seq_bwd_ws", dout.data_ptr(), sv["r"].data_ptr(), sv["z"].data_ptr(), sv["n"].data_ptr(),
             sv["ghn"].data_ptr(), sv["hin"].data_ptr(), masks.data_ptr(), idx.data_ptr(), self.whhT, T, n, H,
             dgi.data_ptr(), dgh.data_ptr(), dhz.data_ptr(), carry.data_ptr(), cnt.data_ptr(), self.status_ptr(0), s)
        self._dense_wgrad(dgh, sv["hin"], R, 3 * H, H, 0, 0, self.GHH, self.GBH)
        self._dense_wgrad(dgi, x, R, 3 * H, self.Ip, 3, self.I, self.GIH, self.GBI)
        self._gru_in_backward(storage, dgi, x, R, idx)
        self._finish_step(optimizer)


class RecurrentEngine(_GRU, CNNEngine):
    """CNNBase(recurrent=True) + vector obs: x = cat(fc(obs), vec) -> GRU -> heads.
    Parameter order: gru.{weight_ih, weight_hh, bias_ih, bias_hh}, main.*, critic, dist."""

    W1, B1, W2, B2, W3, B3, W4, B4, WC, BC, WA, BA, LS = range(4, 17)

    def __init__(self, policy, device):
        gru = policy.base.gru
        self.V = policy.base.vector_obs_len
        H = policy.base.main[7].weight.shape[0]
        self.I = H + self.V
        self.Ip = (self.I + 3) // 4 * 4   # GEMM rows padded to 16-B multiples
        if gru.weight_ih_l0.shape != (3 * H, self.I) or H % 32 != 0:
            raise NotImplementedError("GRU engine needs hidden_size a multiple of 32 (<= 512)")
        self.gru_packed = None
        super().__init__(policy, device)

    def _pack_weights(self):
        super()._pack_weights()
        H, Ip = self.H, self.Ip
        if self.gru_packed is None:
            self.gru_packed = torch.empty(3 * H * Ip + 6 * H * H, device=self.device)
        gp = self.gru_packed.data_ptr()
        self.wih_pad, self.wihT, self.whhT = gp, gp + 4 * 3 * H * Ip, gp + 4 * (3 * H * Ip + 3 * H * H)
        call("ppo_gru_pack", self.pv(self.GIH), self.pv(self.GHH), H, self.I, Ip, self.wih_pad, self.wihT, self.whhT,
             stream())

    def _gru_in(self, obs, vec, idx, B, ws):
        """x_pad [B][Ip] = (fc(obs) | vector obs | 0-pad) and gi = x·W_ihᵀ + b_ih [B][3H]."""
        dev, s, H, Ip = self.device, stream(), self.H, self.Ip
        if idx is None:
            obs = self._check_obs(obs)
            vec = vec.to(dev, torch.float32).reshape(B, self.V).contiguous() if self.V else None
        x = ws.get("xpad", B * Ip, device=dev)
        self.trunk(obs, idx, B, ws, out=x, ldo=Ip)
        if Ip > H:
            src = vec if vec is not None else x   # V == 0: only the zero pad is written
            call("ppo_concat_cols", src.data_ptr(), ptr(idx if vec is not None else None), B,
                 self.V if vec is not None else 0, x.data_ptr(), Ip, H, Ip - H, s)
        gi = ws.get("gi", B * 3 * H, device=dev)
        call("ppo_linear_fwd_ex", x.data_ptr(), None, B, Ip, Ip, self.wih_pad, self.pv(self.GBI), 3 * H,
             gi.data_ptr(), 3 * H, 0, s)
        return x, gi

    def _gru_out(self, hout, B, ws):
        return hout, None

    def _gru_out_train(self, storage, adv, idx, hout, R, hp, loss_acc):
        dout = self.ws["train"].get("dout", R * self.H, device=self.device)
        self._heads_train(storage, adv, idx, hout, R, hp, loss_acc, dout, feat_act=0)
        return dout

    def _gru_in_backward(self, storage, dgi, x, R, idx):
        H = self.H
        dh = self.ws["train"].get("dh", R * H, device=self.device)
        call("ppo_linear_dgrad_ex", dgi.data_ptr(), R, 3 * H, self.wihT, H, x.data_ptr(), self.Ip, 1, dh.data_ptr(),
             stream())
        self._trunk_backward(R, dh, storage.obs, idx)


class MLPEngine(_Engine):
    """MLPBase (model.py:202-234): actor / critic towers Linear-tanh-Linear-tanh on
    x = cat(obs, vector_obs); value from the critic tower, logits from the actor's.
    Parameter order: actor.0, actor.2, critic.0, critic.2, critic_linear, dist."""

    AW1, AB1, AW2, AB2, CW1, CB1, CW2, CB2, WC, BC, WA, BA, LS = range(13)
    is_mlp = True

    def __init__(self, policy, device):
        base = policy.base
        if base.is_recurrent != self.recurrent:
            raise NotImplementedError("a recurrent MLPBase runs on RecurrentMLPEngine, a feed-forward one on "
                                      "MLPEngine (Policy.hip_engine() selects the engine)")
        self.H = base._hidden_size
        # x = cat(obs, vector_obs) feeds the GRU of a recurrent base, else the towers' first layers
        self.I = (base.gru.weight_ih_l0 if self.recurrent else base.actor[0].weight).shape[1]
        self.V = base.vector_obs_len
        self.obs_dim = self.I - self.V
        self.Ip = (self.I + 3) // 4 * 4
        if self.recurrent and (self.H % 32 != 0 or self.H > 512 or self.I < 1):
            raise NotImplementedError("GRU engine needs hidden_size a multiple of 32 (<= 512)")
        if self.H % 4 != 0 or self.H > 512:
            raise NotImplementedError(f"MLPBase hidden_size {self.H}: multiples of 4 up to 512")
        super().__init__(policy, device)

    def _pack_weights(self):
        H, Ip, s = self.H, self.Ip, stream()
        if self.packed is None:
            self.packed = torch.empty(2 * H * Ip + 2 * H * H, device=self.device)
        b = self.packed.data_ptr()
        self.aw1, self.cw1 = b, b + 4 * H * Ip
        self.aw2T, self.cw2T = b + 8 * H * Ip, b + 8 * H * Ip + 4 * H * H
        for w, dst in ((self.AW1, self.aw1), (self.CW1, self.cw1)):   # first layers padded to Ip inputs
            call("ppo_concat_cols", self.pv(w), None, H, self.I, dst, Ip, 0, Ip, s)
        call("ppo_transpose", self.pv(self.AW2), H, H, self.aw2T, s)
        call("ppo_transpose", self.pv(self.CW2), H, H, self.cw2T, s)

    def _rows(self, obs, vec, R):
        """host-facing arguments -> fp32 device rows [R][obs_dim], [R][V] | None"""
        obs = (obs if obs.is_cuda else obs.to(self.device)).to(torch.float32).reshape(R, -1).contiguous()
        if obs.shape[1] != self.obs_dim:
            raise RuntimeError(f"MLPBase expects [N,{self.obs_dim}] observations, got {tuple(obs.shape)}")
        v = vec.to(self.device, torch.float32).reshape(R, self.V).contiguous() if self.V else None
        return obs, v

    def _x(self, obs, vec, idx, B, ws):
        """x_pad [B][Ip] = (obs | vector obs | 0)"""
        dev, s = self.device, stream()
        x = ws.get("x", B * self.Ip, device=dev)
        call("ppo_concat_cols", obs.data_ptr(), ptr(idx), B, self.obs_dim, x.data_ptr(), self.Ip, 0,
             self.obs_dim if self.V else self.Ip, s)
        if self.V:
            call("ppo_concat_cols", vec.data_ptr(), ptr(idx), B, self.V, x.data_ptr(), self.Ip, self.obs_dim,
                 self.Ip - self.obs_dim, s)
        return x

    def _tower_in(self):
        """(width of the towers' input rows, actor.0 weight, critic.0 weight)"""
        return self.Ip, self.aw1, self.cw1

    def towers(self, x, B, ws):
        dev, H, s = self.device, self.H, stream()
        Ip, aw1, cw1 = self._tower_in()
        out = {}
        for name, w1, b1, w2, b2 in (("a", aw1, self.AB1, self.AW2, self.AB2),
                                     ("c", cw1, self.CB1, self.CW2, self.CB2)):
            h1 = ws.get(name + "1", B * H, device=dev)
            h2 = ws.get(name + "2", B * H, device=dev)
            call("ppo_linear_fwd_ex", x.data_ptr(), None, B, Ip, Ip, w1, self.pv(b1), H, h1.data_ptr(), H, 2, s)
            call("ppo_linear_fwd_ex", h1.data_ptr(), None, B, H, H, self.pv(w2), self.pv(b2), H, h2.data_ptr(), H, 2, s)
            out[name] = (h1, h2)
        return out

    @_with_precision
    def act(self, obs, deterministic=False, noise=None, given=None, want_entropy=False, value_only=False, vec=None,
            hxs=None, masks=None):
        """hxs and masks are accepted for the engines' common signature and not used."""
        self.ensure_bound()
        self.pack()
        B = obs.shape[0]
        obs, v = self._rows(obs, vec, B)
        ws = self.ws[self.act_ws]
        x = self._x(obs, v, None, B, ws)
        t = self.towers(x, B, ws)
        return self._heads(t["a"][1], B, deterministic, noise, given, want_entropy, value_only, hv=t["c"][1])

    def _towers_train(self, storage, adv, idx, x, B, hp, loss_acc, K, kind, width):
        """Towers on x [B][K], heads_train and the towers' weight gradients (kind / width:
        ppo_wgrad_reduce's column map of the first layers).  Returns dL/d(first-layer
        pre-activations) of the actor and the critic tower."""
        ws, dev, H = self.ws["train"], self.device, self.H
        t = self.towers(x, B, ws)
        da2 = ws.get("da2", B * H, device=dev)
        dc2 = ws.get("dc2", B * H, device=dev)
        self._heads_train(storage, adv, idx, t["a"][1], B, hp, loss_acc, da2, feat_act=2, feat_v=t["c"][1],
                          dfeat_v=dc2)
        d1s = []
        for name, d2, w1, b1, w2, b2, w2T in (("a", da2, self.AW1, self.AB1, self.AW2, self.AB2, self.aw2T),
                                               ("c", dc2, self.CW1, self.CB1, self.CW2, self.CB2, self.cw2T)):
            h1 = t[name][0]
            self._dense_wgrad(d2, h1, B, H, H, 0, 0, w2, b2)
            d1 = ws.get("d1" + name, B * H, device=dev)
            call("ppo_linear_dgrad_ex", d2.data_ptr(), B, H, w2T, H, h1.data_ptr(), H, 2, d1.data_ptr(), stream())
            self._dense_wgrad(d1, x, B, H, K, kind, width, w1, b1)
            d1s.append(d1)
        return d1s

    @_with_precision
    def train_minibatch(self, storage, adv, idx, hp, loss_acc, optimizer):
        self.ensure_bound()
        self.pack()
        _dist.begin_minibatch()
        B = idx.numel()
        x = self._x(storage.obs, storage.vector_obs if self.V else None, idx, B, self.ws["train"])
        self._towers_train(storage, adv, idx, x, B, hp, loss_acc, self.Ip, 3, self.I)
        self._finish_step(optimizer)


class RecurrentMLPEngine(_GRU, MLPEngine):
    """MLPBase(recurrent=True) (model.py:111-166, 224-234): x = cat(obs, vector_obs) -> GRU ->
    actor / critic towers on the GRU output (their first layers are H x H) -> heads.
    Parameter order: gru.{weight_ih, weight_hh, bias_ih, bias_hh}, actor.0, actor.2, critic.0,
    critic.2, critic_linear, dist.  The GRU input is the observation, so nothing flows back
    past W_ih; dL/d(GRU output) is the two towers' gradient in one ppo_linear_dgrad_pair."""

    AW1, AB1, AW2, AB2, CW1, CB1, CW2, CB2, WC, BC, WA, BA, LS = range(4, 17)

    def _pack_weights(self):
        H, Ip, s = self.H, self.Ip, stream()
        if self.packed is None:
            self.packed = torch.empty(3 * H * Ip + 3 * H * H + 4 * H * H, device=self.device)
        b = self.packed.data_ptr()
        self.wih_pad, self.whhT = b, b + 4 * 3 * H * Ip
        self.aw1T = self.whhT + 4 * 3 * H * H
        self.cw1T, self.aw2T, self.cw2T = (self.aw1T + 4 * H * H * i for i in (1, 2, 3))
        # W_ih zero-padded to Ip inputs; ppo_gru_pack's W_ih[:, :H]ᵀ plane is not built: the GRU
        # input gets no gradient here (and I < H is the usual case)
        call("ppo_concat_cols", self.pv(self.GIH), None, 3 * H, self.I, self.wih_pad, Ip, 0, Ip, s)
        call("ppo_transpose", self.pv(self.GHH), 3 * H, H, self.whhT, s)
        for w, dst in ((self.AW1, self.aw1T), (self.CW1, self.cw1T), (self.AW2, self.aw2T), (self.CW2, self.cw2T)):
            call("ppo_transpose", self.pv(w), H, H, dst, s)

    def _tower_in(self):
        return self.H, self.pv(self.AW1), self.pv(self.CW1)

    def _gru_in(self, obs, vec, idx, B, ws):
        """x_pad [B][Ip] = (obs | vector obs | 0) and gi [B][3H] = x_pad · W_ihᵀ + b_ih"""
        if idx is None:
            obs, vec = self._rows(obs, vec, B)
        x = self._x(obs, vec, idx, B, ws)
        gi = ws.get("gi", B * 3 * self.H, device=self.device)
        call("ppo_linear_fwd_ex", x.data_ptr(), None, B, self.Ip, self.Ip, self.wih_pad, self.pv(self.GBI),
             3 * self.H, gi.data_ptr(), 3 * self.H, 0, stream())
        return x, gi

    def _gru_out(self, hout, B, ws):
        t = self.towers(hout, B, ws)
        return t["a"][1], t["c"][1]

    def _check_storage(self, storage):
        if storage.obs.dtype != torch.float32 or storage.obs[0, 0].numel() != self.obs_dim:
            raise RuntimeError(f"MLPBase expects float32 [{self.obs_dim}] observation rows in the storage, got "
                               f"{storage.obs.dtype} {tuple(storage.obs.shape[2:])}")

    def _gru_out_train(self, storage, adv, idx, hout, R, hp, loss_acc):
        H = self.H
        d1a, d1c = self._towers_train(storage, adv, idx, hout, R, hp, loss_acc, H, 0, 0)
        # dL/d(GRU output): both towers' first layers in one launch, the actor's k range first
        dout = self.ws["train"].get("dout", R * H, device=self.device)
        call("ppo_linear_dgrad_pair", d1a.data_ptr(), self.aw1T, H, d1c.data_ptr(), self.cw1T, H, R, H,
             dout.data_ptr(), stream())
        return dout

    def _gru_in_backward(self, storage, dgi, x, R, idx):
        pass
