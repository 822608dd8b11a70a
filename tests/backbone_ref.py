"""float64 restatements of the ResNet stem and of the whole C4 backbone (torch.nn.functional on the CPU), with the per-element
error bound of tests/split_ref.py for the stem -- shared by tests/test_backbone_host.py and tests/test_gpu_backbone.py.

Stem ([D2-upstream] BasicStem): conv 7x7 / stride 2 / pad 3 (3 -> 64), FrozenBN fold (scale, shift), ReLU, max-pool 3x3 / 2 / pad 1.
The convolution is a dot product of length K = 147 per element, so split_ref's gate applies to the conv + epilogue element by
element with the magnitude S = sum |x| |w| carried through the epilogue (split_ref.epilogue).  The pooled value is a maximum of
up to nine of those: |max_i (a_i + e_i) - max_i a_i| <= max_i |e_i|, so its bound is the maximum of the window's bounds (max-pool
of the bound map, whose padding is -inf: rows / columns that do not exist contribute nothing).  Results are channels-last
[N, PH, PW, 64] like the kernel's.

Net: the state dict of locov_amd.backbone.ResNet evaluated block by block in the requested dtype (float64: the reference).
"""
import torch
import torch.nn.functional as F

import split_ref as sr

STEM_K = 147
EPS = 1e-5


def stem_inputs(N, H, W, seed, variant="plain"):
    """(x [N,3,H,W], w [64,3,7,7], scale [64], shift [64]) fp32 CPU.  scale has both signs (|scale| in [0.5, 1.5]), shift spans
    [-2, 2]: a conv row / column that does not exist, if computed from zero padding, would give relu(shift) > 0 on half of the channels.
    variant "neg_shift": shift = -1e3 on channels 5, 17, 40 (their output is exactly 0); "corners": x is zero but for one pixel
    at each of the four image corners (per channel)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, 3, H, W, generator=g)
    w = torch.randn(64, 3, 7, 7, generator=g) * 0.1
    sign = torch.where(torch.rand(64, generator=g) < 0.5, -1.0, 1.0)
    scale = (0.5 + torch.rand(64, generator=g)) * sign
    shift = torch.rand(64, generator=g) * 4.0 - 2.0
    shift[0] = 2.0
    if variant == "neg_shift":
        shift[[5, 17, 40]] = -1e3
    elif variant == "corners":
        c = torch.zeros_like(x)
        for i in (0, H - 1):
            for j in (0, W - 1):
                c[:, :, i, j] = x[:, :, i, j] + 3.0
        x = c
    else:
        assert variant == "plain"
    return x, w, scale, shift


def stem(x, w, scale, shift) -> sr.Ref:
    """The float64 stem and its per-element bound, channels-last [N,PH,PW,64] (fold everything into E, as split_ref.segmean)."""
    xd, wd = x.detach().double().cpu(), w.detach().double().cpu()
    cl = lambda t: t.permute(0, 2, 3, 1)
    S = cl(F.conv2d(xd.abs(), wd.abs(), stride=2, padding=3))
    conv = sr.Ref(cl(F.conv2d(xd, wd, stride=2, padding=3)), S, torch.zeros_like(S), STEM_K)
    act = sr.epilogue(conv, scale=scale, shift=shift, relu=True)
    pool = lambda t: cl(F.max_pool2d(t.permute(0, 3, 1, 2).contiguous(), kernel_size=3, stride=2, padding=1)).contiguous()
    ref, bnd = pool(act.ref), pool(sr.bound(act))
    return sr.Ref(ref, torch.zeros_like(ref), (bnd - 4 * sr.U * ref.abs()).clamp_min(0), 1)


def randomize_frozen_bn(model, seed):
    """Random FrozenBN statistics in every norm of the model: weight, running_var in [0.5, 1.5], bias, running_mean ~ 0.1 N(0,1)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, buf in model.named_buffers():
            leaf = name.rsplit(".", 1)[-1]
            if leaf in ("weight", "running_var"):
                buf.copy_(0.5 + torch.rand(buf.shape, generator=g))
            elif leaf in ("bias", "running_mean"):
                buf.copy_(0.1 * torch.randn(buf.shape, generator=g))
    return model


def net(state_dict, x, stages=("res2", "res3", "res4"), dtype=torch.float64):
    """{"stem": ..., "res2": ..., ...} NCHW of the STRIDE_IN_1X1 / FrozenBN bottleneck ResNet held by `state_dict`, in `dtype` on
    the CPU.  The number of blocks of a stage and which ones have a projection shortcut are read from the keys."""
    sd = {k: v.detach().to(dtype).cpu() for k, v in state_dict.items()}

    def conv_bn(t, pre, stride=1, padding=0):
        t = F.conv2d(t, sd[pre + ".weight"], stride=stride, padding=padding)
        scale = sd[pre + ".norm.weight"] / (sd[pre + ".norm.running_var"] + EPS).sqrt()
        shift = sd[pre + ".norm.bias"] - sd[pre + ".norm.running_mean"] * scale
        return t * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)

    t = x.detach().to(dtype).cpu()
    t = F.max_pool2d(F.relu(conv_bn(t, "stem.conv1", 2, 3)), kernel_size=3, stride=2, padding=1)
    out = {"stem": t}
    for si, name in enumerate(stages):
        b = 0
        while f"{name}.{b}.conv1.weight" in sd:
            pre = f"{name}.{b}"
            stride = 2 if (b == 0 and si > 0) else 1
            y = F.relu(conv_bn(t, pre + ".conv1", stride))
            y = F.relu(conv_bn(y, pre + ".conv2", 1, 1))
            y = conv_bn(y, pre + ".conv3")
            sc = conv_bn(t, pre + ".shortcut", stride) if pre + ".shortcut.weight" in sd else t
            t = F.relu(y + sc)
            b += 1
        out[name] = t
    return out
