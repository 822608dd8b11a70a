"""The inputs that take the caption kernels (locov_amd/csrc/caption.hip) through every branch of their launch code, and the launch
rules restated from that file's comment block and include/locov_hip.h, so that tests/test_caption_cases.py can say without a GPU
which branch each case reaches and tests/test_gpu_caption_tiers.py runs them.

Launch rules:
  forward   caption_embed_kernel<VEC, MAXC>: float4 lanes (VEC = 4) when H % 4 == 0 and W, input_embeddings and, on the LayerNorm
            path, P, Tt, gamma, beta and encoded_tokens are 16-byte aligned and keep (if given) 4-byte aligned; scalar lanes
            otherwise.  MAXC register slots per lane: <4,4> up to H = 1024, <4,16> up to 4096; <1,4> up to 256, <1,16> up to 1024,
            <1,64> up to 4096.
  rank      one workgroup of 1024 threads, token n in round n / 1024, at most LOCOV_CAPTION_MAX_TOKENS = 8192 tokens.
  scatter   one wave per vocabulary row, at most 4096 workgroups of four waves: with V > 16384 a wave takes rows v, v + 16384, ...
            float4 lanes when H % 4 == 0 and the gradient rows and dW are 16-byte aligned.

Cases are (B, T, H, V) with the options of caption_ref.make_case, the smallest that reach each branch; the name of a forward case
begins with its tier.  Three things follow from the layout of make_case (a caption is [CLS], body, [SEP], padding on the last third)
and are not options:
  * B = 1, T = 4 has ONE body token, which carries the last planted boundary draw (selected, id kept); the cases with T >= 5
    have at least four and hold a mask, a noise and a keep outcome.
  * (2, 6, H, V) has four body tokens, three of which the rule replaces.  The scatter-grid cases therefore run their backward on
    the tokenizer's ids (masked language modelling inactive, draws = None), where every planted id keeps its token; row 0 gets its
    gradient from the padding.
  * The rule puts [MASK] on an eighth of the body tokens, a run of several hundred at N = 8192.  The pad_ids = "spread" case is
    there for short runs, so its backward runs on the tokenizer's ids as well.  Every other case runs with the rule on."""
import hashlib

import numpy as np

import caption_ref as cr

WAVE, RANK_THREADS, MAX_TOKENS, MAX_HIDDEN = 64, 1024, 8192, 4096
SCATTER_WAVES = 4096 * 4
MARK_ROWS = (16383, 16384, 32767, 32768)                  # either side of one and two scatter grids


def fwd_tier(H, aligned):
    if H % 4 == 0 and aligned:
        return "v4x4" if H <= 4 * WAVE * 4 else "v4x16"
    return "s1x4" if H <= WAVE * 4 else "s1x16" if H <= WAVE * 16 else "s1x64"


def rank_rounds(N):
    return -(-N // RANK_THREADS)


def scatter_form(H, V, aligned):
    return ("vec4" if H % 4 == 0 and aligned else "scalar", V > SCATTER_WAVES)


def _marks(V):
    return [r for r in dict.fromkeys(MARK_ROWS + (V - 1,)) if r < V]


# name: (shape, options of make_case)
FORWARD = {
    "v4x4_full_h1024": ((2, 5, 1024, 40), {}),
    "v4x16_first_h1028": ((2, 5, 1028, 40), {}),
    "v4x16_full_h4096": ((1, 4, 4096, 12), {}),
    "v4x4_one_vector_h4": ((2, 5, 4, 40), {}),
    "s1x4_two_lanes_h2": ((2, 5, 2, 40), {}),
    "s1x4_full_h256_W": ((2, 5, 256, 40), {"misalign": ("W",)}),
    "s1x16_first_h258": ((2, 5, 258, 40), {}),
    "s1x16_ragged_h1022": ((2, 5, 1022, 40), {}),
    "s1x16_full_h1024_P": ((2, 5, 1024, 40), {"misalign": ("P",)}),
    "s1x64_first_h1026": ((1, 4, 1026, 12), {}),
    "s1x64_ragged_h4094": ((1, 4, 4094, 12), {}),
    "s1x64_full_h4096_gamma": ((1, 4, 4096, 12), {"misalign": ("gamma",)}),
}
PREDICATE = {f"s1x4_h64_{k}": ((2, 5, 64, 50), {"misalign": (k,)}) for k in ("W", "P", "Tt", "gamma", "beta", "keep")}
RANK = {
    "rank2_n1025": ((25, 41, 8, 50), {}),
    "rank2_n2048": ((32, 64, 8, 50), {}),
    "rank8_n8192_long_run": ((64, 128, 8, 50), {}),
}
GRID = {f"grid_v{V}_h{H}": ((2, 6, H, V), {"plant_ids": _marks(V)}) for V in (16384, 16385, 32769) for H in (4, 6)}
PRODUCTION = {"production_v30522_h768": ((4, 32, 768, 30522), {"plant_ids": [16383, 16384, 30521]})}
LN_BWD = {
    "ln_n8192_spread": ((64, 128, 8, 4200), {"pad_ids": "spread"}),
    "s1x16_first_h258": FORWARD["s1x16_first_h258"],
}
LN_NULL_ARMS = {"ln_null_arms_h64": ((2, 5, 64, 50), {})}
RULE_OFF = tuple(GRID) + ("ln_n8192_spread",)
CASES = {**FORWARD, **PREDICATE, **RANK, **GRID, **PRODUCTION, **LN_BWD, **LN_NULL_ARMS}

_BUILT = {}


def case(name):
    """The inputs of one case, built once and shared: make_case's dictionary plus "name", "shape", "misalign", "rule" (whether the
    backward runs with masked language modelling on), "want" = expected_ints with the rule on and "want_bwd" = the integers that the
    backward case sees."""
    if name not in _BUILT:
        shape, opts = CASES[name]
        c = cr.make_case(*shape, seed=sum(shape), **opts)
        for k in cr.OPERANDS:                               # (an allocator that gives less than 16 bytes: place the aligned ones too)
            if k not in opts.get("misalign", ()) and c[k].ctypes.data % 16:
                c[k] = cr.offset_view(c[k], 0)
        c.update(name=name, shape=shape, misalign=tuple(opts.get("misalign", ())), rule=name not in RULE_OFF)
        c["want"] = cr.expected_ints(c)
        c["want_bwd"] = c["want"] if c["rule"] else cr.expected_ints(c, active=False)
        _BUILT[name] = c
    return _BUILT[name]


def aligned(c, layer_norm=True, keep=True):
    """The forward launch's alignment predicate on the case's own operands (W; with the LayerNorm path the four tables; with a keep
    mask its 4 bytes).  The outputs are fresh allocations."""
    names = ("W",) + (("P", "Tt", "gamma", "beta") if layer_norm else ())
    return all(c[k].ctypes.data % 16 == 0 for k in names) and not (layer_norm and keep and c["keep"].ctypes.data % 4)


def on_device(a):
    """The array on the device at the same offset from a 16-byte boundary as on the host."""
    import torch
    off = a.ctypes.data % 16
    if off == 0:
        return torch.from_numpy(a).cuda()
    buf = torch.empty(a.nbytes + off, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    t = buf[off:].view(torch.from_numpy(a).dtype).view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.is_contiguous() and t.data_ptr() % 16 == off
    return t


def checksum(c):
    """sha256 over every entry of a make_case dictionary: name, dtype, shape, bytes."""
    h = hashlib.sha256()
    for k in sorted(c):
        a = np.ascontiguousarray(c[k])
        h.update(f"{k}:{a.dtype.str}:{a.shape}:".encode())
        h.update(a.tobytes())
    return h.hexdigest()


# make_case(*shape, seed=sum(shape), p_noise=p_noise) as the tests of tests/test_gpu_caption.py call it, recorded before the options
DEFAULT_CHECKSUMS = {
    ((3, 7, 768, 50), 0.05): "eda1bfc4b9b6752585273015ca19309bdd1b17aa3363892040a7abb3cf89a71b",
    ((3, 7, 768, 50), 0.0): "8cc81ffbbe3dc4a5b4714fbdc9af3c63a282c24a3f7165ad2b3a3eea6b495c7f",
    ((2, 5, 64, 50), 0.05): "508b01b4aec3ab610771f872066e7a6521531c0b4c23809deeeba58074a8236b",
    ((2, 5, 64, 50), 0.0): "68aac48f43a7df6e06e0045a9d1a49ede9bd0e19aaffd00cde56cdbc633edb73",
    ((3, 7, 100, 37), 0.05): "319d72f600d195acfcc866bd2d5886c5e993b2b95ec234ff5273894dd6f769b4",
    ((3, 7, 100, 37), 0.0): "8e55501a9d00eb04e24a7d154a5054edc3b92742d8c3d3e2974b6bcf8ce1e8f4",
    ((4, 12, 64, 50), 0.05): "f2186e012839d74a27723c3c0391a689364a57d80d28079abb8c73ca312cbfd4",
    ((4, 12, 64, 50), 0.0): "98f721cbbd37a70564e8ae9d12004b91d6317aca52d4949f31922b4c8095e950",
}
