"""numpy restatement of the caption path (locov_amd/language_backbone.py, csrc/caption.hip): the masked-language-modelling rule of
ovr/modeling/language/transf_models.py:114-137 as its Python loop, the gather, the LayerNorm forward and backward in float64, and
the sequential scatter `for n in range(N): dW[id[n]] += g[n]`.  Also the shared inputs of the CPU and GPU tests."""
import numpy as np

P, P_MASK = 0.25, 0.5                                      # binary fractions: u / p == p_mask is attainable (0.125 / 0.25)
BELOW_P = np.nextafter(P, 0.0)                              # the next double below p: selected
AT_MASK = P * P_MASK                                        # exact: u / p == p_mask
BELOW_ONE = np.nextafter(1.0, 0.0)


def mlm_rule(ids, types, attn, special, draws, p, p_mask, p_noise, mask_id, len_tok, active=True):
    """The reference's loop, with draws[0] for np.random.rand() and draws[1] for np.random.randint(len(tokenizer)).  [B, T] int
    arrays in, (input_ids, special_tokens_mask, target_ids, mlm_mask) int64 out."""
    ids, special = np.array(ids, dtype=np.int64), np.array(special, dtype=np.int64)
    target, mlm_mask = ids.copy(), np.zeros_like(ids)
    p_mask_noise = float(p_mask) + float(p_noise)
    B, T = ids.shape
    for i in range(B):
        for j in range(T):
            if special[i, j] or not attn[i][j] or not active:
                continue
            prob = float(draws[0][i][j])
            if prob < p:
                mlm_mask[i, j] = 1
                prob /= p
                if prob < p_mask:
                    ids[i, j] = mask_id
                    special[i, j] = 1
                elif prob < p_mask_noise:
                    ids[i, j] = min(int(float(draws[1][i][j]) * len_tok), len_tok - 1)
    return ids, special, target, mlm_mask


def layer_norm_fwd(ids, types, W, Pe, Tt, gamma, beta, eps, keep=None, p_drop=0.0):
    """float64: dropout(LayerNorm(W[id] + Tt[type] + P[:T])); returns (y, xhat, rstd)."""
    W, Pe, Tt, gamma, beta = (np.asarray(a, dtype=np.float64) for a in (W, Pe, Tt, gamma, beta))
    x = W[ids] + Tt[types] + Pe[None, :ids.shape[1]]
    mean = x.mean(-1, keepdims=True)
    var = ((x - mean) ** 2).mean(-1, keepdims=True)          # biased
    rstd = 1.0 / np.sqrt(var + eps)
    xhat = (x - mean) * rstd
    y = xhat * gamma + beta
    if keep is not None:
        y = y * keep.astype(np.float64) / (1.0 - p_drop)
    return y, xhat, rstd


def layer_norm_bwd(g_enc, xhat, rstd, gamma, keep=None, p_drop=0.0):
    """float64: the gradient of layer_norm_fwd's y with respect to x."""
    g = np.asarray(g_enc, dtype=np.float64)
    if keep is not None:
        g = g * keep.astype(np.float64) / (1.0 - p_drop)
    gh = g * np.asarray(gamma, dtype=np.float64)
    return rstd * (gh - gh.mean(-1, keepdims=True) - xhat * (gh * xhat).mean(-1, keepdims=True))


def scatter(ids, g, V, dtype=np.float32):
    """dW[id[n]] += g[n], n ascending, in `dtype`, from zeros."""
    flat, g = np.asarray(ids).reshape(-1), np.asarray(g, dtype=dtype).reshape(-1, g.shape[-1])
    dW = np.zeros((V, g.shape[1]), dtype=dtype)
    for n in range(flat.shape[0]):
        dW[flat[n]] = dW[flat[n]] + g[n]
    return dW


OPERANDS = ("W", "P", "Tt", "gamma", "beta", "keep")        # what make_case's `misalign` may name


def offset_view(a, offset):
    """A contiguous copy of `a` that starts `offset` bytes past a 16-byte boundary of a larger allocation."""
    buf = np.empty(a.nbytes + 32, dtype=np.uint8)
    start = (-buf.ctypes.data) % 16 + offset
    v = buf[start:start + a.nbytes].view(a.dtype).reshape(a.shape)
    v[...] = a
    return v


def make_case(B, T, H, V, seed, p_noise=0.05, plant_ids=(), pad_ids="zero", misalign=()):
    """Tokens with heavy duplication (padding id 0 on the last third of every caption, one word ten times when there is room),
    [CLS] / [SEP] specials, and draws that contain the boundary values; tables for the LayerNorm path.

    The options leave the default case as it is, bit for bit (none of them draws from the generator):
      plant_ids   vocabulary ids forced onto body tokens, from the last body token backwards, tokens that the masked-language-
                  modelling rule never selects (draw >= p) first: those keep their id through the rule.  Their positions come back
                  as "plant_pos".
      pad_ids     "zero": as above.  "spread": every id that the layout repeats -- the padding, [CLS], [SEP] -- cycles through a
                  block reserved at the top of the vocabulary and the repeated word appears eight times, so that no id of the
                  tokenizer's output occurs more than 8 times unless the random body ids collide that often.
      misalign    names out of OPERANDS: each is a contiguous view that starts 4 bytes (`keep`: 1 byte) past a 16-byte boundary."""
    assert pad_ids in ("zero", "spread") and set(misalign) <= set(OPERANDS)
    rng = np.random.default_rng(seed)
    pad_from = T - T // 3
    spread = pad_ids == "spread"
    laid_out = B * (T - pad_from + 2)                        # padded positions, [CLS], [SEP]
    reserved = -(-laid_out // 8) if spread else 0
    ids = rng.integers(5, V - reserved, size=(B, T))
    if spread:
        block = (V - reserved + np.arange(laid_out) % reserved).reshape(B, T - pad_from + 2)
        ids[:, 0], ids[:, pad_from - 1], ids[:, pad_from:] = block[:, 0], block[:, 1], block[:, 2:]
    else:
        ids[:, 0], ids[:, pad_from - 1], ids[:, pad_from:] = 2, 3, 0
    body = [(i, j) for i in range(B) for j in range(1, pad_from - 1)]
    for i, j in (body[::2][:8 if spread else 10] if len(body) >= 20 else body[2:]):      # (21 tokens hold no ten free words: all but two of them)
        ids[i, j] = 7
    attn = np.ones((B, T), dtype=np.int64)
    attn[:, pad_from:] = 0
    special = 1 - attn
    special[:, 0] = special[:, pad_from - 1] = 1
    types = np.zeros((B, T), dtype=np.int64)
    types[B - 1, 1:pad_from] = 1
    draws = rng.random((2, B, T))
    bd = boundary_draws()
    for k, (u, r) in enumerate(bd):
        i, j = body[k % len(body)]
        draws[0, i, j], draws[1, i, j] = u, r
    draws[0, :, 0] = 0.0                                     # a special token with a draw that would select it
    draws[0, :, T - 1] = 0.0                                 # a padded token likewise
    scale = 0.5
    tables = {"W": (rng.standard_normal((V, H)) * scale).astype(np.float32), "P": (rng.standard_normal((T + 3, H)) * scale).astype(np.float32),
              "Tt": (rng.standard_normal((2, H)) * scale).astype(np.float32), "gamma": (1 + 0.2 * rng.standard_normal(H)).astype(np.float32),
              "beta": (0.1 * rng.standard_normal(H)).astype(np.float32)}
    keep = (rng.random((B, T, H)) >= 0.1).astype(np.uint8)
    case = {"ids": ids, "types": types, "attn": attn, "special": special, "draws": draws, "keep": keep, "p_noise": p_noise, "mask_id": 4,
            "len_tok": V - 2, "eps": 1e-12, "p_drop": 0.1, **tables}
    if len(plant_ids):
        assert len(plant_ids) <= len(body) and all(0 <= v < V for v in plant_ids)
        spots = sorted(reversed(body), key=lambda ij: draws[0][ij] < P)[:len(plant_ids)]      # (stable: never selected first)
        for (i, j), v in zip(spots, plant_ids):
            ids[i, j] = v
        case["plant_pos"] = np.array(spots, dtype=np.int64)
    for name in misalign:
        case[name] = offset_view(case[name], 1 if name == "keep" else 4)
    return case


def boundary_draws():
    """(u, r) pairs: u == p exactly (not selected); the next double below p (selected); u with u / p == p_mask exactly (not the mask
    branch: noise or keep); a noise draw with r just below 1.0 (id len_tok - 1); a plain mask, a plain noise, a plain keep."""
    assert AT_MASK / P == P_MASK
    return [(P, 0.5), (BELOW_P, BELOW_ONE), (AT_MASK, BELOW_ONE), (P * 0.52, BELOW_ONE), (P * 0.2, 0.3), (P * 0.53, 0.25), (P * 0.99, 0.5)]


def tokenized(case):
    return {"input_ids": case["ids"].tolist(), "token_type_ids": case["types"].tolist(), "attention_mask": case["attn"].tolist(),
            "special_tokens_mask": case["special"].tolist()}


def expected_ints(case, active=True):
    return mlm_rule(case["ids"], case["types"], case["attn"], case["special"], case["draws"], P, P_MASK, case["p_noise"], case["mask_id"],
                    case["len_tok"], active)
