"""tests/backbone_ref.net restated under autograd with every non-linearity made explicit -- shared by
tests/test_backbone_train_host.py and tests/test_gpu_backbone_train.py.

Every ReLU is a multiplication by a 0/1 set and the max-pool is a gather by selection, so the function is linear in the
activations once the sets are fixed.  `net` either computes its own sets (pre-activation > 0; torch's max-pool rule: the first
window position, in row-major scan, that attains the maximum) and returns them, or replays given ones.  That is the convention of
tests/test_gpu_res5_train.py (_float64_stage): a gradient is compared with float64 arithmetic on the function the device actually
computed -- its own active sets -- because one unit that flips between two evaluations moves a weight gradient by ~1e-3, far
above any rounding.  With its own sets the result is backbone_ref.net's, bit for bit (tests/test_backbone_train_host.py).

Sets: {"stem": uint8 [N,64,PH,PW] -- 3 di + dj of the selected conv position (2p - 1 + di, 2q - 1 + dj), 9 where the pooled value is
0 --, "res2.0.y1" / ".y2" / ".out": bool [N,C,H,W], ...}; a key that is missing from a given dict is computed.
"""
import torch
import torch.nn.functional as F

import backbone_ref as br

NO_SEL = 9


def pool_select(act):
    """Post-ReLU conv map [N,C,CH,CW] -> sel uint8 [N,C,PH,PW] by torch's max-pool rule (9 where the maximum is 0)."""
    CW = act.shape[3]
    pooled, idx = F.max_pool2d(act.detach(), kernel_size=3, stride=2, padding=1, return_indices=True)
    PH, PW = pooled.shape[2:]
    p = torch.arange(PH).view(1, 1, PH, 1)
    q = torch.arange(PW).view(1, 1, 1, PW)
    code = 3 * (idx // CW - (2 * p - 1)) + (idx % CW - (2 * q - 1))
    assert int(code.min()) >= 0 and int(code.max()) <= 8
    return torch.where(pooled > 0, code, NO_SEL).to(torch.uint8)


def pool_index(sel, CH, CW):
    """sel [N,C,PH,PW] -> (flat index into CH x CW of the selected position, clamped where there is none; keep = sel < 9)."""
    PH, PW = sel.shape[2:]
    code = sel.long()
    keep = code < NO_SEL
    code = torch.where(keep, code, 4)                     # (the centre always exists)
    i = 2 * torch.arange(PH).view(1, 1, PH, 1) - 1 + code // 3
    j = 2 * torch.arange(PW).view(1, 1, 1, PW) - 1 + code % 3
    assert bool(((i >= 0) & (i < CH) & (j >= 0) & (j < CW))[keep.expand_as(i)].all()), "a selection outside the conv map"
    return (i.clamp(0, CH - 1) * CW + j.clamp(0, CW - 1)), keep


def pool_gather(act, sel):
    """The max-pool as a gather: act [N,C,CH,CW] (graph) at the positions sel names, 0 where sel is 9."""
    N, C, CH, CW = act.shape
    idx, keep = pool_index(sel, CH, CW)
    return act.flatten(2).gather(2, idx.flatten(2)).view(idx.shape) * keep.to(act.dtype)


def weights_of(state_dict, dtype):
    """The convolution weights of the state dict as leaves in `dtype` (the only trainable tensors: FrozenBN is buffers)."""
    return {k: v.detach().to(dtype).cpu().clone().requires_grad_(True) for k, v in state_dict.items()
            if k.endswith(".weight") and ".norm." not in k}


def net(state_dict, x, dtype=torch.float64, sets=None, weights=None, stages=("res2", "res3", "res4")):
    """backbone_ref.net under autograd -> (outputs {"stem", "res2", ...} NCHW with a graph, the sets used, the weight leaves)."""
    sd = {k: v.detach().to(dtype).cpu() for k, v in state_dict.items()}
    weights = weights_of(state_dict, dtype) if weights is None else weights
    given = {} if sets is None else sets
    used = {}

    def conv_bn(t, pre, stride=1, padding=0):
        t = F.conv2d(t, weights[pre + ".weight"], stride=stride, padding=padding)
        scale = sd[pre + ".norm.weight"] / (sd[pre + ".norm.running_var"] + br.EPS).sqrt()
        shift = sd[pre + ".norm.bias"] - sd[pre + ".norm.running_mean"] * scale
        return t * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)

    def relu(pre, key):
        m = given[key].cpu() if key in given else pre.detach() > 0
        assert m.dtype == torch.bool and m.shape == pre.shape, key
        used[key] = m
        return pre * m.to(pre.dtype)

    t = x.detach().to(dtype).cpu()
    pre = conv_bn(t, "stem.conv1", 2, 3)
    if "stem" in given:
        sel = given["stem"].cpu()
        act = pre                                          # a selected position is active by definition; sel == 9 passes nothing
    else:
        act = pre * (pre.detach() > 0).to(dtype)
        sel = pool_select(act)
    used["stem"] = sel
    t = pool_gather(act, sel)
    out = {"stem": t}
    for si, name in enumerate(stages):
        b = 0
        while f"{name}.{b}.conv1.weight" in sd:
            p = f"{name}.{b}"
            stride = 2 if (b == 0 and si > 0) else 1
            y = relu(conv_bn(t, p + ".conv1", stride), p + ".y1")
            y = relu(conv_bn(y, p + ".conv2", 1, 1), p + ".y2")
            y = conv_bn(y, p + ".conv3")
            sc = conv_bn(t, p + ".shortcut", stride) if p + ".shortcut.weight" in sd else t
            t = relu(y + sc, p + ".out")
            b += 1
        out[name] = t
    return out, used, weights


def grads(state_dict, x, G, dtype=torch.float64, sets=None, feature="res4"):
    """d (out[feature] . G).sum() / d weights in `dtype` -> (out[feature] detached, {weight key: gradient}, the sets used)."""
    out, used, weights = net(state_dict, x, dtype, sets)
    y = out[feature]
    (y * G.to(dtype).cpu()).sum().backward()
    return y.detach(), {k: w.grad for k, w in weights.items()}, used


def set_flips(a, b):
    """(differing units, units) over the keys two sets dicts share (the stem's selection counts per pooled element)."""
    diff = total = 0
    for k in a:
        if k in b:
            diff += int((a[k].cpu() != b[k].cpu()).sum())
            total += a[k].numel()
    return diff, total


def worst_relative(got, ref, keys=None):
    """max over the tensors of max |got - ref| / max |ref| -> (that figure, its key)."""
    worst, at = 0.0, None
    for k in (ref if keys is None else keys):
        top = float(ref[k].abs().max())
        assert top > 0, k
        e = float((got[k].detach().double().cpu() - ref[k].double()).abs().max()) / top
        if e > worst:
            worst, at = e, k
    return worst, at


def stem_wgrad(x, g, sel, scale, dtype=torch.float64):
    """The stem's weight gradient by the formula of include/locov_hip.h in `dtype` on the CPU, and its magnitude:
    gconv = g routed to the conv positions sel names (channels-last g, sel [N,PH,PW,64]);
    dw[o,c,u,v] = scale[o] sum gconv[n,i,j,o] x[n,c,2i-3+u,2j-3+v];  S = |scale| sum |gconv| |x|."""
    N, _, H, W = x.shape
    CH, CW = (H + 1) // 2, (W + 1) // 2
    xd, gd = x.detach().to(dtype).cpu(), g.detach().to(dtype).cpu().permute(0, 3, 1, 2)
    idx, keep = pool_index(sel.cpu().permute(0, 3, 1, 2), CH, CW)
    gconv = torch.zeros(N, 64, CH * CW, dtype=dtype).scatter_add_(2, idx.flatten(2), (gd * keep.to(dtype)).flatten(2)).view(N, 64, CH, CW)
    sc = scale.detach().to(dtype).cpu().view(-1, 1, 1, 1)
    dw = torch.nn.grad.conv2d_weight(xd, (64, 3, 7, 7), gconv, stride=2, padding=3) * sc
    S = torch.nn.grad.conv2d_weight(xd.abs(), (64, 3, 7, 7), gconv.abs(), stride=2, padding=3) * sc.abs()
    return dw, S, gconv
