#!/usr/bin/env python
"""
Generates tests/golden/g9_grounding_module_grad.npz by running the REFERENCE's own GroundingModule under autograd
(ovr/modeling/roi_heads/box_emb_grounding_head.py:60-256, loaded as make_golden.py loads it).

    python tests/golden/make_golden_g9.py            # needs the reference checkout (LOCOV_REFERENCE)

On g6's inputs (image_emb [37, 48], nine classes of 1-5 tokens) and one seeded upstream gradient gy [37, 10], for each of
g6's eight configurations (dot / cosine x softmax / hardmax x temperature 1 / 10):
    <tag>_grad        d sum(scores * gy) / d image_emb -- under cosine with respect to the input BEFORE normalize_vec (the
                      predictor normalises in front of the module, :423-424), so the normalisation's backward is on the path
    <tag>_grad_att    softmax only: the same with an upstream gradient gatt [37, 10, 5] on the attention as well
    <tag>_f64_diff, <tag>_f64_diff_att
                      for the record: max |reference fp32 gradient - float64 restatement (tests/token_ref.py)|, what a gate on
                      these vectors has to leave room for
The fixture holds inputs and outputs only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg          # noqa: E402  (its loaders; it writes nothing on import)
import token_ref                  # noqa: E402


def main():
    assert os.path.isdir(mg.REF), f"reference not found at {mg.REF}"
    mg.install_standins()
    mg.cuda_to_cpu_shim()
    mg.load("ovr.misc", "ovr/misc.py")
    lm = mg.load("ovr.modeling.logged_module", "ovr/modeling/logged_module.py")
    begh = mg.load("ovr.modeling.roi_heads.box_emb_grounding_head", "ovr/modeling/roi_heads/box_emb_grounding_head.py")

    g6 = np.load(os.path.join(HERE, "g6_grounding_module.npz"))
    ntok = [int(n) for n in g6["ntok"]]
    embs = {k: torch.from_numpy(g6[f"emb{k}"]) for k in range(len(ntok))}
    img = torch.from_numpy(g6["image_emb"])
    R, K1, tmax = img.shape[0], len(ntok) + 1, max(ntok)
    gen = torch.Generator().manual_seed(mg.SEED + 9)
    gy = torch.randn(R, K1, generator=gen)
    gatt = torch.randn(R, K1, tmax, generator=gen)
    g9 = {"gy": gy.numpy(), "gatt": gatt.numpy()}

    def f64(metric, align, temp, with_att):
        x0 = img.double().requires_grad_(True)
        x = token_ref.normalize(x0) if metric == "cosine" else x0
        scores, att, _ = token_ref.grounding_module(x, [embs[k] for k in range(len(ntok))], metric, align, temp)
        loss = (scores * gy.double()).sum()
        if with_att:
            loss = loss + (att * gatt.double()).sum()
        return torch.autograd.grad(loss, x0)[0]

    for metric, norm in (("dot", False), ("cosine", True)):
        for align in ("softmax", "hardmax"):
            for temp in (1.0, 10.0):
                tag = f"{metric}_{align}_t{int(temp)}"
                gm = begh.GroundingModule(img.shape[1], len(ntok), tmax, local_metric=metric, alignment=align, temperature=temp,
                                          normalize_emb=norm)
                gm.set_class_embeddings({k: v.clone() for k, v in embs.items()}, "cpu")
                for with_att in ((False, True) if align == "softmax" else (False,)):
                    x0 = img.clone().requires_grad_(True)
                    x = lm.normalize_vec(x0, dim=1) if norm else x0
                    scores, att = gm(x)
                    np.testing.assert_array_equal(scores.detach().numpy(), g6[tag + "_scores"])      # g6's own run, again
                    loss = (scores * gy).sum()
                    if with_att:
                        loss = loss + (att * gatt).sum()
                    grad = torch.autograd.grad(loss, x0)[0]
                    sfx = "_att" if with_att else ""
                    g9[f"{tag}_grad{sfx}"] = grad.numpy()
                    diff = float((grad.double() - f64(metric, align, temp, with_att)).abs().max())
                    g9[f"{tag}_f64_diff{sfx}"] = np.float64(diff)
                    print(f"{tag}{sfx}: max|grad| {float(grad.abs().max()):.4g}  max|fp32 - f64| {diff:.3g}")
    out = os.path.join(HERE, "g9_grounding_module_grad.npz")
    np.savez_compressed(out, **g9)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
