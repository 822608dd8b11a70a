"""Writes tests/golden/g11_bert_embeddings.npz: the state dict and the eval-mode outputs of the installed `transformers` library's
BertEmbeddings, what the reference's BertEmbedding holds as `bert_model` (ovr/modeling/language/transf_models.py:94).

Run by hand where `transformers` is installed (python tests/golden/make_golden_g11.py); no test imports `transformers`.  The model is
built from a config object -- never from_pretrained -- with HF_HUB_OFFLINE=1: nothing is downloaded.  The script itself checks
that the keys are the five the port expects and that the output equals layer_norm(W[id] + Tt[type] + P[:T], eps = 1e-12).
"""
import os

os.environ["HF_HUB_OFFLINE"] = "1"
os.environ["TRANSFORMERS_OFFLINE"] = "1"

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ["word_embeddings.weight", "position_embeddings.weight", "token_type_embeddings.weight", "LayerNorm.weight", "LayerNorm.bias"]


def main():
    import transformers
    from transformers import BertConfig, BertModel
    torch.manual_seed(1111)
    cfg = BertConfig(vocab_size=50, hidden_size=64, num_hidden_layers=1, num_attention_heads=4, intermediate_size=128,
                     max_position_embeddings=32)
    emb = BertModel(cfg).embeddings.eval()
    with torch.no_grad():                                    # a LayerNorm that is not the identity, a padding row that is not zero
        emb.LayerNorm.weight.add_(0.1 * torch.randn(64))
        emb.LayerNorm.bias.add_(0.1 * torch.randn(64))
        emb.word_embeddings.weight[0].normal_(0.0, 0.02)
    sd = emb.state_dict()
    assert list(sd) == KEYS, list(sd)
    g = torch.Generator().manual_seed(7)
    out = {"keys": np.array(list(sd)), "transformers_version": np.array(transformers.__version__), "eps": np.array(cfg.layer_norm_eps)}
    out.update({"sd." + k: v.numpy() for k, v in sd.items()})
    for name, (B, T) in (("a", (2, 9)), ("b", (3, 32))):
        ids = torch.randint(0, 50, (B, T), generator=g)
        ids[0, -2:] = 0
        types = torch.randint(0, 2, (B, T), generator=g)
        with torch.no_grad():
            y = emb(input_ids=ids, token_type_ids=types)
            want = torch.nn.functional.layer_norm(sd[KEYS[0]][ids] + sd[KEYS[2]][types] + sd[KEYS[1]][:T], (64,), sd[KEYS[3]], sd[KEYS[4]],
                                                  cfg.layer_norm_eps)
        assert torch.allclose(y, want, rtol=0, atol=1e-6), float((y - want).abs().max())
        out.update({f"{name}.ids": ids.numpy(), f"{name}.types": types.numpy(), f"{name}.out": y.numpy()})
    path = os.path.join(HERE, "g11_bert_embeddings.npz")
    np.savez(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes) with transformers {transformers.__version__}")


if __name__ == "__main__":
    main()
