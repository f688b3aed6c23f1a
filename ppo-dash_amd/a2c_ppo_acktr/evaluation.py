"""Evaluation path: T/run_evaluation.py:25-122 steps one
env with Policy.act(obs, vector_obs, hxs, masks, deterministic) — batch 1, GRU
state carried across steps, masks zeroed on done.  At batch 1 every act is a
chain of ~10 tiny kernels, so launch overhead, not arithmetic, sets the step
latency.  GraphedActor records that chain once into a HIP graph (torch.cuda.graph
drives hipStreamBeginCapture on the current stream, which is where every
libppo_hip.so launch goes) and replays it per step: inputs are copied into
static buffers, one graph launch runs the whole forward.

The graph holds raw pointers, so everything it touches is kept stable: the
forward runs in the engine's own "graph" workspace (no eager act, get_value or
rollout at another batch size reallocates it), the packed weight planes are
refreshed in place before a replay when the parameters changed, and the graph is
re-captured when the flat parameter buffer or the packed planes were
reallocated (Policy re-bound, moved, or a new engine).

Any policy the HIP engines run can be graphed: CNNBase and MLPBase, feed-forward
and recurrent, with Discrete, Box or MultiBinary heads.  The buffer shapes come
from the engine: ga.obs is [num_envs, C, 84, 84] for a CNNBase and
[num_envs, obs_dim] fp32 for an MLPBase.

An actor is deterministic (sample=False, the default) or sampling (sample=True,
what the reference's evaluation does unless --cuda-deterministic is given); each
refuses the other kind of act.  A launch argument freezes inside a graph, so a
sampling actor's kernels read the RNG counter from a word in device memory
(engine.rng_dev, the ppo_heads_*_act_dc entry points) and a captured
ppo_rng_advance launch, after the heads on the same stream, adds one to it: every
replay samples with the next counter.  The captured chain stays linear, on one
stream.

One counter sequence: the k-th act of an engine uses counter k whether it ran
eagerly or as a replay.  Every replay adds one to the host's engine.rng_counter,
and the actor writes rng_counter + 1 into the word (a stream-ordered fill outside
the graph) after a capture, and in act() / refresh() when eager calls have moved
rng_counter since its last replay.  In 'host' sampling mode (set_sampling_mode)
the captured kernel reads its noise from the pointer-stable ga.noise [num_envs, A];
act() fills it with Policy._noise(n), the draw Policy.act makes on the default
CPU generator.  Switching the mode re-captures.

Two ways to drive it:
  act(obs, vec, hxs, masks)  Policy.act's signature; checks every call that the
                             graph is still valid (engine, buffers, precision,
                             sampling mode, parameter versions, RNG counter) and
                             copies the inputs in.
  replay()                   the evaluation loop's fast path: the caller writes
                             the next observation / masks (and, in 'host' sampling
                             mode, the noise) straight into the pointer-stable
                             inputs (ga.obs, ga.vec, ga.masks, ga.noise) and
                             the graph itself feeds its new hidden state back into
                             ga.hxs (carry_hidden=True); no host checks — call
                             refresh() after changing the parameters or after
                             eager acts / get_value calls on the same policy.
"""
import torch

from . import model as _model


class GraphedActor(object):
    def __init__(self, policy, num_envs=1, obs_dtype=torch.float32, device=None, warmup=2, carry_hidden=False,
                 sample=False):
        eng = policy.hip_engine(device)
        self.policy, self.device, self.warmup = policy, eng.device, warmup
        self.carry_hidden = bool(carry_hidden) and policy.is_recurrent
        self.sample = bool(sample)
        V = getattr(eng, "V", getattr(policy.base, "vector_obs_len", 0))
        Hh = policy.recurrent_hidden_state_size   # eng.H for a recurrent base, else 1
        dev = self.device
        if eng.is_mlp:   # MLPEngine / RecurrentMLPEngine: 1-D observations
            self.obs = torch.zeros(num_envs, eng.obs_dim, device=dev)
        else:
            self.obs = torch.zeros(num_envs, eng.C, 84, 84, dtype=obs_dtype, device=dev)
        self.vec = torch.zeros(num_envs, V, device=dev)
        self.hxs = torch.zeros(num_envs, Hh, device=dev)
        self.masks = torch.ones(num_envs, 1, device=dev)
        # 'host' sampling mode: the noise the captured heads kernel reads
        self.noise = torch.ones(num_envs, eng.A, device=dev) if self.sample else None
        self.captures = 0
        self._capture()

    def _capture(self):
        dev = self.device
        self.eng = self.policy.hip_engine(dev)
        self._mode = _model._SAMPLING["mode"] if self.sample else None
        if self.sample:
            self.eng.rng_dev   # allocated here, not on the side stream or in the graph's pool
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with self.eng.using_workspace("graph"):
            with torch.cuda.stream(side):   # warm-up: workspaces, packed weights, device attributes
                for _ in range(self.warmup):
                    self._act()
            torch.cuda.current_stream(dev).wait_stream(side)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.out = self._act()
                if self.carry_hidden:   # h' -> the next replay's h, inside the graph
                    self.hxs.copy_(self.out[3])
        self._key = self.eng.pack_key()
        self._ptrs = self._pointers()
        self.captures += 1
        if self.sample:   # the warm-up acts advanced the word; the host counter did not move
            self._sync_counter(force=True)

    def _act(self):
        with torch.no_grad():
            if not self.sample:
                return self.policy.act(self.obs, self.vec, self.hxs, self.masks, deterministic=True)
            # Policy.act (model.py:54-66) with the counter read from the device word and, in
            # 'host' mode, the noise from ga.noise
            with self.eng.using_device_counter():
                value, action, logp, _, hxs = _model.engine_act(
                    self.eng, self.obs, self.vec, self.hxs, self.masks, deterministic=False,
                    noise=self.noise if self._mode == "host" else None)
            return value, action, logp, hxs

    def _sync_counter(self, force=False):
        """the device word = the counter the next act uses (rng_counter + 1), rewritten when
        eager calls moved the host counter since this actor's last replay"""
        if force or self.eng.rng_counter != self._synced:
            self.eng.set_rng_dev(self.eng.rng_counter + 1)
            self._synced = self.eng.rng_counter

    def _replay(self):
        self.graph.replay()
        if self.sample:   # the captured ppo_rng_advance moved the word by one: the host counter follows
            self.eng.rng_counter += 1
            self._synced += 1
        return self.out

    def _pointers(self):
        """every buffer address baked into the graph that could be reallocated, and
        the arithmetic mode the kernels were captured with (Policy.half() / float()
        switch the GEMMs' part-product count, a launch argument frozen in the graph);
        for a sampling actor also the sampling mode (device counter or ga.noise)"""
        e = self.eng
        gp = getattr(e, "gru_packed", None)
        ws = e.ws["graph"]
        return (id(e), e.flat.data_ptr(), e.packed.data_ptr(), None if gp is None else gp.data_ptr(),
                id(ws), ws.version,   # any workspace reallocation bumps its version
                bool(getattr(self.policy, "_half_mode", False)),
                (_model._SAMPLING["mode"], e.rng_dev.data_ptr()) if self.sample else None)

    def refresh(self):
        """re-validate after the caller changed the policy (parameters updated in
        place, moved, re-bound, half()/float(), sampling mode) or ran eager acts on
        it: re-capture, re-pack or rewrite the device RNG counter as needed"""
        eng = self.policy.hip_engine(self.device)
        if eng is not self.eng or self._pointers() != self._ptrs:
            self._capture()
        elif self.eng.pack_key() != self._key:
            self.eng.pack(force=True)
            self._key = self.eng.pack_key()
        if self.sample:
            self._sync_counter()

    def replay(self):
        """one act (deterministic, or sampled for a sample=True actor) of the inputs in
        ga.obs / ga.vec / ga.hxs / ga.masks -> (value, action, log_prob, rnn_hxs) output
        buffers (overwritten by the next replay); with carry_hidden the new hidden
        state is already in ga.hxs.  A sampling actor's replay uses the next RNG
        counter and makes no check: call refresh() after eager acts or get_value
        calls on the same policy, which move the counter; in 'host' sampling mode
        fill ga.noise first."""
        return self._replay()

    def act(self, visual_inputs, vector_inputs, rnn_hxs, masks, deterministic=None):
        """Policy.act (model.py:54-66) for the captured batch -> (value, action, log_prob, rnn_hxs);
        deterministic defaults to the kind of act this actor captured"""
        if deterministic is None:
            deterministic = not self.sample
        if not deterministic and not self.sample:
            raise NotImplementedError("GraphedActor replays deterministic acting only; use Policy.act to sample")
        if deterministic and self.sample:
            raise NotImplementedError("this GraphedActor captured sampled acting (sample=True); build one with "
                                      "sample=False for deterministic acting")
        self.refresh()   # buffers moved: re-capture; parameters updated in place: re-pack
        for dst, src in ((self.obs, visual_inputs), (self.vec, vector_inputs), (self.hxs, rnn_hxs),
                         (self.masks, masks)):
            if dst.numel() and src is not dst:
                dst.copy_(src.reshape(dst.shape), non_blocking=True)
        if self.sample and self._mode == "host":
            self.noise.copy_(self.policy._noise(self.noise.shape[0]))
        # the graph's output buffers, overwritten by the next act (as torch.cuda.graphs
        # outputs are); the hidden state fed back in is copied before that happens
        return self._replay()
