"""Sampled acting replayed from a HIP graph (evaluation.GraphedActor(sample=True)) and
graphed MLPBase policies.  Two policies are built under one torch.manual_seed: one
acts eagerly with Policy.act(deterministic=False) at every step, the other mixes
GraphedActor.act, refresh() + replay(), eager acts, an eager get_value, an in-place
parameter update and a half() / float() round trip.  Step by step, value, action,
log-prob and hidden state must be equal bit for bit, and both engines' RNG counters
equal at the end: one counter sequence, however an act was run."""
import pytest
import torch

from a2c_ppo_acktr import model as M
from a2c_ppo_acktr.synthetic import Box, Discrete, MultiBinary

pytestmark = pytest.mark.gpu

STEPS = 12
SPACES = {"disc8": lambda: Discrete(8), "disc12": lambda: Discrete(12), "box3": lambda: Box(-1.0, 1.0, (3,)),
          "mbin5": lambda: MultiBinary(5)}
# name -> (base, obs shape, base_kwargs, vector_obs_len)
BASES = {"cnn": (M.CNNBase, (4, 84, 84), {"recurrent": False, "hidden_size": 64}, 0),
         "cnn_rec": (M.CNNBase, (4, 84, 84), {"recurrent": True, "hidden_size": 64}, 3),
         "mlp": (M.MLPBase, (4,), {"recurrent": False, "hidden_size": 64}, 0),
         "mlp_rec": (M.MLPBase, (5,), {"recurrent": True, "hidden_size": 32}, 2),   # I = 7 -> Ip = 8
         "cnn512": (M.CNNBase, (4, 84, 84), {"recurrent": False, "hidden_size": 512}, 0)}
# what the graphed side does at each step (the eager side acts once per step, and mirrors
# "value" / "update" / "half" / "float"):
#   act      ga.act
#   replay   ga.replay() on inputs written in place (the hidden state carried by the graph)
#   rreplay  ga.refresh(), then replay
#   eager    Policy.act on the graphed side's policy
#   value+   an eager get_value (it consumes a counter) before the step's own op
#   update+  parameters scaled in place, then refresh() before a replay
#   half+ / float+  Policy.half() / float(): the next ga.act re-captures
PATTERN = ("act", "act", "eager", "rreplay", "replay", "value+act", "eager", "rreplay", "update+rreplay",
           "half+act", "float+act", "replay")
MASK_ZERO_AT = 4   # a replay that relies on the carried hidden state


def _make(base, space, gpu, seed=11):
    cls, obs_shape, kw, V = BASES[base]
    torch.manual_seed(seed)
    pol = M.Policy(obs_shape, SPACES[space](), base=cls, base_kwargs=dict(kw), vector_obs_len=V).to(gpu)
    pol.hip_engine()   # rng_seed = this seed
    return pol


def _inputs(base, n, gpu):
    _, obs_shape, _, V = BASES[base]
    g = torch.Generator().manual_seed(3)
    return [(torch.rand(n, *obs_shape, generator=g).to(gpu), torch.rand(n, V, generator=g).to(gpu),
             torch.full((n, 1), 0.0 if t == MASK_ZERO_AT else 1.0, device=gpu)) for t in range(STEPS)]


def _prefix(pol, op, probe):
    """the part of a step both sides do eagerly"""
    for pre in op.split("+")[:-1]:
        if pre == "value":
            pol.get_value(*probe)
        elif pre == "update":
            with torch.no_grad():
                for p in pol.parameters():
                    p.mul_(1.01)
        elif pre == "half":
            pol.half()
        elif pre == "float":
            pol.float()


def _run_eager(pol, inputs, n):
    hx = torch.zeros(n, pol.recurrent_hidden_state_size, device=inputs[0][0].device)
    out = []
    for (obs, vec, m), op in zip(inputs, PATTERN):
        _prefix(pol, op, (obs, vec, hx, m))
        with torch.no_grad():
            v, a, lp, hx = pol.act(obs, vec, hx, m, deterministic=False)
        out.append((v, a, lp, hx))
    return out


def _run_graphed(pol, ga, inputs, n, host=False):
    hx = torch.zeros(n, pol.recurrent_hidden_state_size, device=inputs[0][0].device)
    out, carried = [], False
    for (obs, vec, m), op in zip(inputs, PATTERN):
        _prefix(pol, op, (obs, vec, hx, m))
        op = op.split("+")[-1]
        if op == "eager":
            with torch.no_grad():
                r = pol.act(obs, vec, hx, m, deterministic=False)
            carried = False
        elif op == "act":
            r = ga.act(obs, vec, hx, m)
            carried = ga.carry_hidden
        else:
            if op == "rreplay":
                ga.refresh()
            ga.obs.copy_(obs)
            ga.vec.copy_(vec)
            ga.masks.copy_(m)
            if not carried:   # the last step ran outside the graph
                ga.hxs.copy_(hx)
            if host:
                ga.noise.copy_(pol._noise(n))
            r = ga.replay()
            carried = ga.carry_hidden
            if carried:
                assert torch.equal(ga.hxs, r[3])
        r = tuple(x.clone() for x in r)   # the graph's output buffers are overwritten by the next replay
        hx = r[3]
        out.append(r)
    return out


def _interleave(gpu, base, space, n, host=False):
    from a2c_ppo_acktr.evaluation import GraphedActor
    inputs = _inputs(base, n, gpu)
    pol_e, pol_g = _make(base, space, gpu), _make(base, space, gpu)
    keep = torch.get_rng_state()
    ref = _run_eager(pol_e, inputs, n)
    state_e = torch.get_rng_state()
    torch.set_rng_state(keep)
    ga = GraphedActor(pol_g, num_envs=n, carry_hidden=True, sample=True)
    got = _run_graphed(pol_g, ga, inputs, n, host)
    state_g = torch.get_rng_state()
    eng = pol_g.hip_engine()
    A = eng.A
    for t, (r, g) in enumerate(zip(ref, got)):
        for name, a, b in zip(("value", "action", "logp", "hxs"), r, g):
            assert a.dtype == b.dtype and a.shape == b.shape, (t, PATTERN[t], name)
            assert torch.equal(a, b), (t, PATTERN[t], name)
        assert g[1].dtype == (torch.float32 if eng.float_actions else torch.int64)
        assert tuple(g[1].shape) == ((n, A) if eng.float_actions else (n, 1))
    assert pol_e.hip_engine().rng_counter == eng.rng_counter
    # sampling, not the mode: over 12 steps the actions are not all one step's
    assert any(not torch.equal(got[0][1], g[1]) for g in got[1:])
    assert ga.captures == 3   # built, half(), float()
    return keep, state_e, state_g


@pytest.mark.parametrize("n", [1, 4, 5])   # both sides of small_b = 4
@pytest.mark.parametrize("base", ["cnn", "cnn_rec", "mlp", "mlp_rec"])
def test_interleaved_sampling_is_one_counter_sequence(gpu, base, n):
    _interleave(gpu, base, "disc8", n)


@pytest.mark.parametrize("space", ["disc12", "box3", "mbin5"])
@pytest.mark.parametrize("base", ["cnn", "cnn_rec", "mlp", "mlp_rec"])
def test_interleaved_sampling_every_head(gpu, base, space):
    _interleave(gpu, base, space, 4)


def test_interleaved_sampling_production_shape(gpu):
    _interleave(gpu, "cnn512", "disc8", 1)


@pytest.mark.parametrize("base,space,n", [("cnn", "disc8", 1), ("cnn_rec", "mbin5", 4), ("mlp", "box3", 5),
                                          ("mlp_rec", "disc12", 4)])
def test_interleaved_sampling_host_mode(gpu, base, space, n):
    """'host' sampling mode: the noise is Policy._noise's draw on the default CPU generator
    on both sides, which leaves the generator in the same state"""
    keep = torch.get_rng_state()
    M.set_sampling_mode("host")
    try:
        start, state_e, state_g = _interleave(gpu, base, space, n, host=True)
        assert torch.equal(state_e, state_g)
        assert not torch.equal(start, state_e)   # and the draws were made
    finally:
        M.set_sampling_mode("device")
        torch.set_rng_state(keep)


def test_sampling_mode_switch_recaptures(gpu):
    from a2c_ppo_acktr.evaluation import GraphedActor
    pol_e, pol_g = _make("mlp", "disc8", gpu), _make("mlp", "disc8", gpu)
    ga = GraphedActor(pol_g, num_envs=4, sample=True)
    obs, vec, m = _inputs("mlp", 4, gpu)[0]
    hx = torch.zeros(4, 1, device=gpu)
    keep = torch.get_rng_state()
    try:
        for mode, grow in (("device", 0), ("host", 1), ("host", 0), ("device", 1)):
            M.set_sampling_mode(mode)
            before = ga.captures
            torch.manual_seed(5)
            with torch.no_grad():
                r = pol_e.act(obs, vec, hx, m, deterministic=False)
            torch.manual_seed(5)
            g = ga.act(obs, vec, hx, m)
            assert ga.captures == before + grow, mode
            for a, b in zip(r[:3], g[:3]):
                assert torch.equal(a, b), mode
    finally:
        M.set_sampling_mode("device")
        torch.set_rng_state(keep)


def test_each_kind_of_actor_refuses_the_other(gpu):
    from a2c_ppo_acktr.evaluation import GraphedActor
    pol = _make("mlp", "disc8", gpu)
    obs, vec, m = _inputs("mlp", 1, gpu)[0]
    hx = torch.zeros(1, 1, device=gpu)
    sampler = GraphedActor(pol, sample=True)
    with pytest.raises(NotImplementedError, match="sample=True"):
        sampler.act(obs, vec, hx, m, deterministic=True)
    det = GraphedActor(pol)
    with pytest.raises(NotImplementedError) as e:
        det.act(obs, vec, hx, m, deterministic=False)
    assert str(e.value) == "GraphedActor replays deterministic acting only; use Policy.act to sample"
    before = pol.hip_engine().rng_counter
    det.act(obs, vec, hx, m)
    sampler.act(obs, vec, hx, m)
    assert pol.hip_engine().rng_counter == before + 1   # only the sampled replay is a counted act


@pytest.mark.parametrize("base", ["mlp", "mlp_rec"])
@pytest.mark.parametrize("space", ["disc8", "box3"])
def test_deterministic_mlp_actor_equals_eager(gpu, base, space):
    from a2c_ppo_acktr.evaluation import GraphedActor
    n = 5
    pol = _make(base, space, gpu)
    ga = GraphedActor(pol, num_envs=n)
    assert tuple(ga.obs.shape) == (n, pol.hip_engine().obs_dim) and ga.obs.dtype == torch.float32
    hx_e = torch.zeros(n, pol.recurrent_hidden_state_size, device=gpu)
    hx_g = hx_e.clone()
    for t, (obs, vec, m) in enumerate(_inputs(base, n, gpu)[:6]):
        with torch.no_grad():
            ve, ae, le, hx_e = pol.act(obs, vec, hx_e, m, deterministic=True)
        vg, ag, lg, hx_g = ga.act(obs, vec, hx_g, m)
        for a, b in ((ve, vg), (ae, ag), (le, lg), (hx_e, hx_g)):
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), t
        hx_g = hx_g.clone()
        if t == 2:   # parameters trained in place between steps: the graph follows
            with torch.no_grad():
                for p in pol.parameters():
                    p.mul_(1.01)
