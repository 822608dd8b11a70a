"""CPU-side checks of locov_amd.transformer_head: the reference's surface (state-dict keys, strict loading of a reference checkpoint,
the decoder tying, the requires_grad switches, the builder, the exceptions) against tests/golden/g10_transformer_head.npz, and the
float64 yardstick of the GPU tests (tests/transformer_ref.py) against the reference's own outputs stored there."""
import json
import os
from types import SimpleNamespace as ns

import numpy as np
import pytest
import torch
from torch import nn

import transformer_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G10 = np.load(os.path.join(ROOT, "tests", "golden", "g10_transformer_head.npz"))
KEYS = [str(k) for k in G10["keys"]]
V_DIM, L_DIM, LOC_DIM = 40, 64, 2
CASES = [("h2", 1, ""), ("h2", 3, ""), ("h2", 3, "zero_"), ("h1", 1, ""), ("h1", 3, "")]
INPUT_NAMES = ("region_features", "region_mask", "region_loc", "mvm_mask", "target_region_features", "encoded_tokens",
               "attention_mask", "mlm_mask", "target_ids")


class Backbone(nn.Module):
    def __init__(self, vocab=100, hidden=64):
        super().__init__()
        self.embeddings = nn.Parameter(torch.zeros(vocab, hidden))


def make_cfg(tag="h2", distill=True, **over):
    t = json.loads(str(G10["cfg_" + tag]))
    t.update(over)
    return ns(MODEL=ns(MMSS_HEAD=ns(TRANSFORMER=ns(**{**t, "BERT_CONFIG": dict(t["BERT_CONFIG"])}), DISTILLATION_LOSS=distill)))


def make_head(tag="h2", distill=True, **over):
    from locov_amd.transformer_head import TransformerHead
    return TransformerHead(make_cfg(tag, distill, **over), V_DIM, L_DIM, LOC_DIM, Backbone())


def state_dict():
    return {k: torch.from_numpy(G10["sd/" + k]) for k in KEYS}


def inputs(B, zero=False):
    inp = {k: torch.from_numpy(G10[f"b{B}_{k}"]) for k in INPUT_NAMES}
    if zero:
        inp["mlm_mask"] = torch.zeros_like(inp["mlm_mask"])
    return inp


def test_state_dict_keys_and_strict_loading():
    head = make_head()
    assert sorted(head.state_dict().keys()) == sorted(KEYS)
    assert list(head.state_dict().keys()) == KEYS                                    # the reference's order as well
    head.load_state_dict(state_dict(), strict=True)
    for k in KEYS:
        assert torch.equal(head.state_dict()[k], torch.from_numpy(G10["sd/" + k])), k
    listed = ["backbone.embeddings", "v2l_projection.weight", "visual_emb.image_location_embeddings.bias", "visual_emb.LayerNorm.weight",
              "encoder.layer.1.attention.self.value.bias", "encoder.layer.0.attention.output.LayerNorm.weight",
              "encoder.layer.0.intermediate.dense.weight", "encoder.layer.1.output.LayerNorm.bias", "pooler.dense.bias",
              "heads.predictions.bias", "heads.predictions.transform.LayerNorm.weight", "heads.predictions.decoder.weight",
              "heads.predictions.decoder.bias", "heads.bi_seq_relationship.weight", "heads.imagePredictions.transform.dense.bias",
              "heads.imagePredictions.decoder.weight"]
    assert set(listed) <= set(KEYS)


def test_tying():
    head = make_head()
    assert head.heads.predictions.decoder.weight is head.backbone.embeddings
    assert head.heads.predictions.decoder.bias is head.heads.predictions.bias
    head.load_state_dict(state_dict(), strict=True)                                  # loading keeps the tie
    assert head.heads.predictions.decoder.weight is head.backbone.embeddings
    with pytest.raises(AssertionError):
        from locov_amd.transformer_head import TransformerHead
        TransformerHead(make_cfg(), V_DIM, L_DIM, LOC_DIM, Backbone(vocab=99))


def test_init_weights_and_pretrained_copy():
    torch.manual_seed(0)
    head = make_head()
    w = head.encoder.layer[0].intermediate.dense.weight
    with torch.no_grad():
        assert abs(float(w.std()) - 0.02) < 0.004 and float(head.encoder.layer[1].output.dense.bias.abs().max()) == 0.0
        ln = head.heads.predictions.transform.LayerNorm
        assert float(ln.weight.min()) == 1.0 == float(ln.weight.max()) and float(ln.bias.abs().max()) == 0.0

    class Pretrained(Backbone):
        def __init__(self):
            super().__init__()
            self.bert_model = nn.Module()
            self.bert_model.encoder = nn.Module()
            self.bert_model.encoder.layer = nn.ModuleList([nn.Module()])
            att = nn.Module()
            att.self = nn.Module()
            att.self.query = nn.Linear(64, 64)
            att.self.key = nn.Linear(32, 64)                                         # another shape: not copied
            self.bert_model.encoder.layer[0].attention = att
    from locov_amd.transformer_head import TransformerHead
    bb = Pretrained()
    head = TransformerHead(make_cfg(pretrained_weights=True), V_DIM, L_DIM, LOC_DIM, bb)
    assert torch.equal(head.encoder.layer[0].attention.self.query.weight, bb.bert_model.encoder.layer[0].attention.self.query.weight)
    assert torch.equal(head.encoder.layer[0].attention.self.query.bias, bb.bert_model.encoder.layer[0].attention.self.query.bias)
    assert head.encoder.layer[0].attention.self.key.weight.shape == (64, 64)


def test_requires_grad_switches():
    frozen = lambda h: sorted(n for n, p in h.named_parameters() if not p.requires_grad)
    image = sorted("heads.imagePredictions." + n for n in ("transform.dense.weight", "transform.dense.bias", "transform.LayerNorm.weight",
                                                            "transform.LayerNorm.bias", "decoder.weight", "decoder.bias"))
    match = ["heads.bi_seq_relationship.bias", "heads.bi_seq_relationship.weight", "pooler.dense.bias", "pooler.dense.weight"]
    assert frozen(make_head(MVM_LOSS="", MMM_LOSS="cross_entropy")) == image
    assert frozen(make_head(distill=False, MVM_LOSS="", MMM_LOSS="")) == sorted(image + match)
    assert frozen(make_head(MVM_LOSS="reconstruction_error", MMM_LOSS="cross_entropy")) == []
    assert frozen(make_head(distill=False, MVM_LOSS="contrastive_cross_entropy", MMM_LOSS="")) == sorted(match)


def test_builder_and_unknown_names():
    import locov_amd
    from locov_amd.transformer_head import TransformerHead, build_transformer_head
    assert locov_amd.TransformerHead is TransformerHead and locov_amd.build_transformer_head is build_transformer_head
    head = build_transformer_head("TransformerHead", make_cfg(), V_DIM, L_DIM, LOC_DIM, Backbone())
    assert isinstance(head, TransformerHead) and (head.v_dim, head.l_dim, head.loc_dim) == (V_DIM, L_DIM, LOC_DIM)
    with pytest.raises(KeyError, match="MLPHead"):
        build_transformer_head("MLPHead", make_cfg(), V_DIM, L_DIM, LOC_DIM, Backbone())
    with pytest.raises(NotImplementedError):                                         # the constructor, as the reference
        make_head(MVM_LOSS="l2")
    head = make_head(MMM_LOSS="binary")                                              # the forward, as the reference
    inp = inputs(1)
    with pytest.raises(NotImplementedError):
        head(inp, inp)


def test_config_defaults_are_the_references():
    from locov_amd.config import get_cfg
    from locov_amd.transformer_head import TransformerHead
    cfg = get_cfg()
    t = cfg.MODEL.MMSS_HEAD.TRANSFORMER
    assert (t.MVM_LOSS, t.MMM_LOSS, t.MVM_LOSS_NUM_NEGATIVE, t.pretrained_weights) == ("", "", 128, False)
    b = t.BERT_CONFIG
    assert (b.vocab_size, b.hidden_size, b.num_hidden_layers, b.num_attention_heads, b.intermediate_size) == (30522, 768, 12, 12, 3072)
    assert (b.hidden_act, b.hidden_dropout_prob, b.attention_probs_dropout_prob, b.initializer_range, b.layer_norm_eps) == \
        ("gelu", 0.1, 0.1, 0.02, 1e-12)
    assert cfg.MODEL.MMSS_HEAD.DISTILLATION_LOSS is False
    cfg.merge_from_list(["MODEL.MMSS_HEAD.TRANSFORMER.BERT_CONFIG.num_hidden_layers", 1, "MODEL.MMSS_HEAD.TRANSFORMER.BERT_CONFIG.vocab_size",
                         50, "MODEL.MMSS_HEAD.TRANSFORMER.BERT_CONFIG.intermediate_size", 64])
    head = TransformerHead(cfg, 16, 768, 2, Backbone(vocab=50, hidden=768))          # a CfgNode serves as well as a namespace
    assert len(head.encoder.layer) == 1 and head.encoder.layer[0].attention.self.num_attention_heads == 12


def test_module_does_not_import_transformers():
    src = open(os.path.join(ROOT, "locov_amd", "transformer_head.py")).read()
    assert "import transformers" not in src and "from transformers" not in src


@pytest.mark.parametrize("tag,B,zero", CASES)
def test_float64_restatement_reproduces_the_reference(tag, B, zero):
    """The yardstick checks itself: within the recorded max |reference fp32 - float64| of every stored quantity."""
    p = f"{tag}_b{B}_{zero}"
    heads = json.loads(str(G10["cfg_" + tag]))["BERT_CONFIG"]["num_attention_heads"]
    sd = {k: v.double().requires_grad_(k in tr.GRAD_NAMES) for k, v in state_dict().items()}
    losses, info, pw = tr.head_forward(sd, inputs(B, bool(zero)), heads, 2)
    assert list(losses) == [str(n) for n in G10[p + "loss_names"]] and list(info) == [str(n) for n in G10[p + "info_names"]]
    assert float((pw.detach() - torch.from_numpy(G10[p + "trans"]).double()).abs().max()) <= float(G10[p + "trans_f64_diff"])
    for v, want, tol in zip(losses.values(), G10[p + "losses"], G10[p + "losses_f64_diff"]):
        if np.isnan(want):
            assert zero and torch.isnan(v)
        else:
            assert abs(float(v.detach()) - float(want)) <= float(tol)
    np.testing.assert_array_equal(np.array([float(v) for v in info.values()], np.float32), G10[p + "info"])
    if zero:
        assert np.isnan(G10[p + "losses"][0]) and G10[p + "info"][0] == 0.0          # pinned: NaN MLM loss, accuracy 0
        return
    sum(losses.values()).backward()
    for name in tr.GRAD_NAMES:
        diff = float((sd[name].grad - torch.from_numpy(G10[p + "grad/" + name]).double()).abs().max())
        assert diff <= float(G10[p + "grad_f64_diff/" + name]), (name, diff)
