"""The ReLU decisions of the engine's training forward, and their check against
float64's: a gradient reference that takes the engine's decisions measures
arithmetic, not which pre-activations sit within a rounding of 0 — provided every
differing decision is shown to sit there."""
import torch

from oracle import torch_ref as TR


def engine_relu_masks(eng, B, H, h=None):
    """the ReLU decisions of the engine's training forward of the minibatch just run
    (its workspace activations a1..a3 and fc output h, NHWC -> the reference's NCHW);
    h: the fc output where it is not the workspace's [B][H] buffer (the recurrent
    engine writes it into the padded GRU input)"""
    bufs = eng.ws["train"].bufs
    a1 = bufs["a1"][:B * 12800].view(B, 20, 20, 32).permute(0, 3, 1, 2)
    a2 = bufs["a2"][:B * 5184].view(B, 9, 9, 64).permute(0, 3, 1, 2)
    a3 = bufs["a3"][:B * 1568].view(B, 7, 7, 32).permute(0, 3, 1, 2)
    if h is None:
        h = bufs["h"][:B * H].view(B, H)
    return [t > 0 for t in (a1, a2, a3, h)]


def check_relu_decisions(p, obs_in, ridx, masks, chunk=4096, rel=1e-5):
    """every ReLU decision of the engine agrees with float64's, except where the
    float64 pre-activation is within rel x that layer's max |pre-activation| of 0;
    returns the number of such flips per layer"""
    w1, b1, w2, b2, w3, b3, w4, b4 = [t.detach() for t in p[:8]]
    B = masks[0].shape[0]
    flips, worst, zmax = [0] * 4, [0.0] * 4, [0.0] * 4
    with torch.no_grad():
        for s in range(0, B, chunk):
            e = min(B, s + chunk)
            rows = slice(s, e) if ridx is None else ridx[s:e].to(obs_in.device)
            x = TR._decode(obs_in[rows], w1.device, torch.float64)
            z1 = TR.conv_unfold(x, w1, b1, 4)
            z2 = TR.conv_unfold(torch.relu(z1), w2, b2, 2)
            z3 = TR.conv_unfold(torch.relu(z2), w3, b3, 1)
            z4 = torch.nn.functional.linear(torch.relu(z3).reshape(e - s, -1), w4, b4)
            for k, z in enumerate((z1, z2, z3, z4)):
                d = (z > 0) != masks[k][s:e]
                zmax[k] = max(zmax[k], z.abs().max().item())
                if d.any():
                    flips[k] += int(d.sum())
                    worst[k] = max(worst[k], z[d].abs().max().item())
    for k in range(4):
        assert worst[k] <= rel * zmax[k], (k, flips, worst, zmax)
    return flips
