"""The language backbone without a GPU (locov_amd/language_backbone.py): the numpy restatement (tests/caption_ref.py) against the
installed library's BertEmbeddings (tests/golden/g11_bert_embeddings.npz), the masked-language-modelling rule at its boundaries by
hand, the checkpoint keys, freeze(), the registry, the WordPiece tokenizer on a 12-line vocabulary, and the module's CPU torch
path against the restatement."""
import os
import warnings

import numpy as np
import pytest
import torch

import caption_ref as cr
from lsm_model_cases import SizedTokenizer, ToyTokenizer

VOCAB_LINES = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "a", "dog", "play", "##ing", "##s", ",", "cafe"]


@pytest.fixture(scope="module")
def g11(golden_dir):
    return np.load(os.path.join(golden_dir, "g11_bert_embeddings.npz"))


def _cfg(V=50, H=64, **lb):
    from locov_amd.config import get_cfg
    cfg = get_cfg()
    cfg.MODEL.DEVICE = "cpu"
    cfg.MODEL.LANGUAGE_BACKBONE.TYPE, cfg.MODEL.LANGUAGE_BACKBONE.PRETRAINED = "build_bertemb_backbone", False
    for k, v in lb.items():
        cfg.MODEL.LANGUAGE_BACKBONE[k] = v
    t = cfg.MODEL.MMSS_HEAD.TRANSFORMER
    t.MASKED_LANGUAGE_MODELING, t.MASKED_LANGUAGE_MODELING_PROB_NOISE = True, 0.05
    t.BERT_CONFIG.update(vocab_size=V, hidden_size=H, max_position_embeddings=32)
    return cfg


def _module(case, V, H, **lb):
    from locov_amd.language_backbone import build_language_backbone
    torch.manual_seed(0)
    cfg = _cfg(V, H, **lb)
    t = cfg.MODEL.MMSS_HEAD.TRANSFORMER
    t.MASKED_LANGUAGE_MODELING_PROB, t.MASKED_LANGUAGE_MODELING_PROB_MASK, t.MASKED_LANGUAGE_MODELING_PROB_NOISE = cr.P, cr.P_MASK, case["p_noise"]
    m = build_language_backbone(cfg, SizedTokenizer(case["len_tok"], case["mask_id"]))
    body = m.body
    with torch.no_grad():
        body.embeddings.copy_(torch.from_numpy(case["W"]))
        body.bert_model.position_embeddings.weight[:case["P"].shape[0]].copy_(torch.from_numpy(case["P"]))
        body.bert_model.token_type_embeddings.weight.copy_(torch.from_numpy(case["Tt"]))
        body.bert_model.LayerNorm.weight.copy_(torch.from_numpy(case["gamma"]))
        body.bert_model.LayerNorm.bias.copy_(torch.from_numpy(case["beta"]))
    return m


# ------------------------------------------------------------------------------------------------------- restatement against g11

def test_restatement_equals_the_library_embeddings(g11):
    sd = {k: g11["sd." + k] for k in g11["keys"]}
    for name in ("a", "b"):
        ids, types, want = g11[name + ".ids"], g11[name + ".types"], g11[name + ".out"]
        y, _, _ = cr.layer_norm_fwd(ids, types, sd["word_embeddings.weight"], sd["position_embeddings.weight"],
                                    sd["token_type_embeddings.weight"], sd["LayerNorm.weight"], sd["LayerNorm.bias"], float(g11["eps"]))
        err = float(np.abs(y - want).max())
        print(f"g11 {name}: restatement (float64) vs library (fp32) max abs {err:.3e}")
        assert err <= 8 * np.finfo(np.float32).eps * float(np.abs(want).max())      # the library's own fp32 rounding over 64 terms
        assert (ids == 0).any()                                                   # the padding row is an ordinary row


def test_layer_norm_backward_restatement_against_float64_autograd():
    case = cr.make_case(2, 5, 64, 50, seed=3)
    ids, types = case["ids"], case["types"]
    x = torch.from_numpy(case["W"].astype(np.float64)[ids] + case["Tt"].astype(np.float64)[types] + case["P"].astype(np.float64)[None, :5])
    x.requires_grad_(True)
    g = torch.from_numpy(np.random.default_rng(1).standard_normal(x.shape))
    keep = torch.from_numpy(case["keep"].astype(np.float64))
    y = torch.nn.functional.layer_norm(x, (64,), torch.from_numpy(case["gamma"].astype(np.float64)), torch.from_numpy(case["beta"].astype(np.float64)),
                                       1e-12) * keep / 0.9
    y.backward(g)
    _, xhat, rstd = cr.layer_norm_fwd(ids, types, case["W"], case["P"], case["Tt"], case["gamma"], case["beta"], 1e-12)
    dx = cr.layer_norm_bwd(g.numpy(), xhat, rstd, case["gamma"], case["keep"], 0.1)
    assert np.abs(dx - x.grad.numpy()).max() <= 1e-12 * max(1.0, float(np.abs(dx).max()))


# ------------------------------------------------------------------------------------------------------- the rule's boundaries

def test_mlm_rule_boundaries_by_hand():
    from locov_amd import ops
    from locov_amd.language_backbone import caption_rule
    p, pm = cr.P, cr.P_MASK
    (u_p, _), (u_below, _), (u_eq, _) = cr.boundary_draws()[:3]
    assert u_p == p and u_below < p and u_eq / p == pm
    #        CLS  u==p  below-p  q==p_mask  noise,r~1  mask  keep  SEP  PAD
    ids = [[2, 10, 11, 12, 13, 14, 15, 3, 0]]
    special = [[1, 0, 0, 0, 0, 0, 0, 1, 1]]
    attn = [[1, 1, 1, 1, 1, 1, 1, 1, 0]]
    types = [[0] * 9]
    u = [[0.0, u_p, u_below, u_eq, p * 0.52, p * 0.2, p * 0.99, 0.0, 0.0]]
    r = [[0.5, 0.5, 0.5, cr.BELOW_ONE, cr.BELOW_ONE, 0.5, 0.5, 0.5, 0.5]]
    for p_noise, want_ids in ((0.05, [2, 10, 11, 47, 47, 4, 15, 3, 0]), (0.0, [2, 10, 11, 12, 13, 4, 15, 3, 0])):
        got = cr.mlm_rule(ids, types, attn, special, [u, r], p, pm, p_noise, 4, 48)
        assert got[0].tolist() == [want_ids]
        assert got[1].tolist() == [[1, 0, 0, 0, 0, 1, 0, 1, 1]]                   # [MASK] becomes special; nothing else does
        assert got[2].tolist() == ids and got[3].tolist() == [[0, 0, 1, 1, 1, 1, 1, 0, 0]]
        t = lambda a, dt=torch.int64: torch.tensor(a, dtype=dt)
        tg = caption_rule(t(ids), t(types), t(attn), t(special), t([u, r], torch.float64), ops.CaptionMlm(p, pm, pm + p_noise, 4, 48))
        for a, b in zip(got, tg):
            assert a.tolist() == b.tolist()
    off = cr.mlm_rule(ids, types, attn, special, [u, r], p, pm, 0.05, 4, 48, active=False)
    assert off[0].tolist() == ids and off[1].tolist() == special and not off[3].any()


def test_stored_draws_mask_a_token_in_every_caption():
    """What the GPU model test relies on: with no masked token the MLM loss is NaN by the reference's definition."""
    import lsm_model_cases as mc
    tok = ToyTokenizer()(mc.captions(), max_length=mc.T)
    out = cr.mlm_rule(tok["input_ids"], tok["token_type_ids"], tok["attention_mask"], tok["special_tokens_mask"], mc.mlm_draws(), 0.15, 0.9,
                      0.0, mc.MASK, mc.VOCAB)
    assert (out[3].sum(axis=1) >= 1).all() and (out[0] == mc.MASK).sum(axis=1).min() >= 1


# ------------------------------------------------------------------------------------------------------- checkpoint keys, freeze

def test_state_dict_keys_match_the_library_and_old_buffers_are_dropped(g11):
    from locov_amd.language_backbone import build_language_backbone
    m = build_language_backbone(_cfg(), ToyTokenizer())
    keys = list(m.state_dict())
    assert keys == ["body.embeddings"] + ["body.bert_model." + k for k in g11["keys"]]
    assert m.body.embeddings is m.body.bert_model.word_embeddings.weight and m.out_channels == 64
    sd = {"body.bert_model." + k: torch.from_numpy(g11["sd." + k]) for k in g11["keys"]}
    sd["body.embeddings"] = sd["body.bert_model.word_embeddings.weight"]
    sd["body.bert_model.position_ids"] = torch.arange(32)[None]
    sd["body.bert_model.token_type_ids"] = torch.zeros(1, 32, dtype=torch.int64)
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.body.embeddings, sd["body.embeddings"])
    with pytest.raises(RuntimeError, match="Unexpected"):
        m.load_state_dict({**sd, "body.bert_model.other": torch.zeros(1)}, strict=True)


@pytest.mark.parametrize("freeze", [True, False])
def test_freeze(freeze):
    from locov_amd.language_backbone import build_language_backbone
    m = build_language_backbone(_cfg(FREEZE=freeze), ToyTokenizer())
    grads = {n for n, p in m.named_parameters() if p.requires_grad}
    assert grads == (set() if freeze else {"body.embeddings"})                     # (named_parameters reports a shared one once)
    assert m.body.bert_model.word_embeddings.weight.requires_grad == (not freeze)
    assert not m.body.bert_model.position_embeddings.weight.requires_grad and not m.body.bert_model.LayerNorm.weight.requires_grad


def test_registry_unknown_type_and_missing_tokenizer():
    import locov_amd
    from locov_amd import language_backbone as lb
    assert "build_bertemb_backbone" in lb.LANGUAGE_BACKBONES_REGISTRY and "build_bert_backbone" not in lb.LANGUAGE_BACKBONES_REGISTRY
    assert locov_amd.build_language_backbone is lb.build_language_backbone and locov_amd.BertEmbedding is lb.BertEmbedding
    cfg = _cfg()
    cfg.MODEL.LANGUAGE_BACKBONE.TYPE = "build_bert_backbone"                       # the reference's default: the 12-layer BERT, not built
    with pytest.raises(AssertionError, match="build_bert_backbone is not registered"):
        lb.build_language_backbone(cfg, ToyTokenizer())
    with pytest.raises(ValueError, match="VOCAB_FILE"):
        lb.build_language_backbone(_cfg())
    with pytest.raises(ValueError, match="does not fit"):
        lb.build_language_backbone(_cfg(V=40), ToyTokenizer())
    src = open(lb.__file__).read()
    assert "import transformers" not in src and "from transformers" not in src and "from_pretrained(" not in src


def test_pretrained_warns_once_and_initialises_like_untrained():
    from locov_amd import language_backbone as lb
    lb._WARNED_PRETRAINED = False
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        a = lb.build_language_backbone(_cfg(PRETRAINED=True), ToyTokenizer())
        lb.build_language_backbone(_cfg(PRETRAINED=True), ToyTokenizer())
    assert sum("nothing is downloaded" in str(x.message) for x in w) == 1
    assert 0.01 < float(a.body.embeddings.std()) < 0.03


# ------------------------------------------------------------------------------------------------------- tokenizer

def test_wordpiece_tokenizer_on_a_twelve_line_vocabulary(tmp_path):
    from locov_amd.language_backbone import WordPieceTokenizer, build_language_backbone
    path = tmp_path / "vocab.txt"
    path.write_text("\n".join(VOCAB_LINES) + "\n", encoding="utf-8")
    tok = WordPieceTokenizer(str(path))
    assert len(tok) == 12 and tok.mask_token_id == 4
    out = tok(["A dog, playing Café!", "dogs " + "x" * 101 + " plays playing a a a a"], max_length=8)
    #  [CLS] a dog , play ##ing cafe [SEP]   -- "!" is not in the vocabulary but the caption is truncated before it
    assert out["input_ids"][0] == [2, 5, 6, 10, 7, 8, 11, 3]
    assert out["attention_mask"][0] == [1] * 8 and out["special_tokens_mask"][0] == [1, 0, 0, 0, 0, 0, 0, 1]
    #  [CLS] dog ##s [UNK] play ##s play [SEP]   -- a 101-character word is [UNK]; truncated to 6 word pieces
    assert out["input_ids"][1] == [2, 6, 9, 1, 7, 9, 7, 3]
    short = tok(["dog xyz"], max_length=7)
    assert short["input_ids"] == [[2, 6, 1, 3, 0, 0, 0]] and short["attention_mask"] == [[1, 1, 1, 1, 0, 0, 0]]
    assert short["special_tokens_mask"] == [[1, 0, 0, 1, 1, 1, 1]] and short["token_type_ids"] == [[0] * 7]
    assert tok.encode("playings") == [7, 8, 9] and tok.encode("!") == [1]
    m = build_language_backbone(_cfg(V=12, VOCAB_FILE=str(path)))                 # the default tokenizer, from the config key
    assert isinstance(m.body.tokenizer, WordPieceTokenizer)
    got = m.body(["a dog"])
    assert tuple(got["input_ids"].shape) == (1, 70) and got["target_ids"][0, :4].tolist() == [2, 5, 6, 3]     # (the ids before the rule)


# ------------------------------------------------------------------------------------------------------- the module's CPU path

@pytest.mark.parametrize("add_pos", [False, True])
def test_cpu_torch_path_equals_the_restatement(add_pos):
    B, T, H, V = 3, 7, 64, 50
    case = cr.make_case(B, T, H, V, seed=11)
    m = _module(case, V, H, ADD_POSITION_EMBEDDING=add_pos).train()
    out = m.body.forward_tokenized(cr.tokenized(case), torch.from_numpy(case["draws"]))
    ids, special, target, mlm_mask = cr.expected_ints(case)
    assert mlm_mask.sum() >= 3 and (ids == case["mask_id"]).any() and (ids != target).sum() > (ids == case["mask_id"]).sum()
    for k, want in (("input_ids", ids), ("token_type_ids", case["types"]), ("attention_mask", case["attn"]), ("special_tokens_mask", special),
                    ("target_ids", target), ("mlm_mask", mlm_mask)):
        assert out[k].dtype == torch.int64 and np.array_equal(out[k].numpy(), want), k
    assert np.array_equal(out["input_embeddings"].detach().numpy().view(np.int32), case["W"][ids].view(np.int32))
    if not add_pos:
        assert out["encoded_tokens"] is out["input_embeddings"]
        return
    # (training draws its own keep mask; the comparison runs on the module's expression with the stored mask)
    y64, _, _ = cr.layer_norm_fwd(ids, case["types"], case["W"], case["P"], case["Tt"], case["gamma"], case["beta"], 1e-12, case["keep"], 0.1)
    got = m.body.bert_model(torch.from_numpy(ids), torch.from_numpy(case["types"]), torch.from_numpy(case["keep"]))
    err = float(np.abs(got.detach().numpy() - y64).max())
    print(f"CPU torch fp32 LayerNorm path vs float64: max abs {err:.3e} (the yardstick of the GPU gate)")
    assert err <= 16 * np.finfo(np.float32).eps * float(np.abs(y64).max())
    m.eval()
    ev = m.body.forward_tokenized(cr.tokenized(case), torch.from_numpy(case["draws"]))     # ..._VALIDATION True: the rule still runs
    assert np.array_equal(ev["mlm_mask"].numpy(), mlm_mask)
    y64e, _, _ = cr.layer_norm_fwd(ids, case["types"], case["W"], case["P"], case["Tt"], case["gamma"], case["beta"], 1e-12)
    assert np.abs(ev["encoded_tokens"].detach().numpy() - y64e).max() <= 16 * np.finfo(np.float32).eps * float(np.abs(y64e).max())


def test_eval_without_validation_changes_nothing_and_mlm_off_has_no_target_keys():
    case = cr.make_case(2, 5, 64, 50, seed=2)
    m = _module(case, 50, 64).eval()
    m.body.mlm_during_validation = False
    out = m.body.forward_tokenized(cr.tokenized(case), torch.from_numpy(case["draws"]))
    assert np.array_equal(out["input_ids"].numpy(), case["ids"]) and np.array_equal(out["target_ids"].numpy(), case["ids"])
    assert not out["mlm_mask"].any() and np.array_equal(out["special_tokens_mask"].numpy(), case["special"])
    m.body.mlm = False
    out = m.body.forward_tokenized(cr.tokenized(case))
    assert set(out) == {"input_ids", "token_type_ids", "attention_mask", "special_tokens_mask", "encoded_tokens", "input_embeddings"}


def test_forward_of_text_equals_forward_tokenized_and_ids_are_validated():
    case = cr.make_case(2, 5, 64, 50, seed=2)
    m = _module(case, 50, 64).eval()
    m.body.mlm_during_validation = False
    texts = ["w10 w11", "w12"]
    a, b = m.body(texts), m.body.forward_tokenized(m.body.tokenizer(texts, max_length=70))
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a) and tuple(a["input_ids"].shape) == (2, 70)
    bad = cr.tokenized(case)
    bad["input_ids"][0][1] = 50
    with pytest.raises(ValueError, match="outside the word table"):
        m.body.forward_tokenized(bad)
    bad = cr.tokenized(case)
    bad["token_type_ids"][0][1] = 2
    with pytest.raises(ValueError, match="token type"):
        m.body.forward_tokenized(bad)
    with pytest.raises(ValueError, match="draws must be float64"):
        m.train().body.forward_tokenized(cr.tokenized(case), torch.zeros(2, 2, 5))
