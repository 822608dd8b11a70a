"""Without a GPU: every case of tests/caption_cases.py reaches the branch of csrc/caption.hip's launch code that its name says, judged
from its shapes and the alignment of its operands under the restated launch rules alone; the branches listed there are all reached;
the planted ids, the padding and the boundary draws are what the GPU tests rely on; and caption_ref.make_case without options still
produces the inputs that tests/test_gpu_caption.py has always run on."""
import numpy as np
import pytest

import caption_cases as cc
import caption_ref as cr


def _N(c):
    return c["shape"][0] * c["shape"][1]


@pytest.mark.parametrize("name", list(cc.FORWARD) + list(cc.PREDICATE))
def test_forward_case_reaches_the_tier_in_its_name(name):
    c = cc.case(name)
    B, T, H, V = c["shape"]
    tier = name.split("_")[0]
    mis = c["misalign"]
    for k in cr.OPERANDS:
        assert (c[k].ctypes.data % (4 if k == "keep" else 16) != 0) == (k in mis), k
        assert c[k].flags["C_CONTIGUOUS"]
    assert H <= cc.MAX_HIDDEN and _N(c) <= cc.MAX_TOKENS
    # the LayerNorm launch with a keep mask; without one a misaligned keep is not an operand, and the gather-only launch sees W alone
    assert cc.fwd_tier(H, cc.aligned(c)) == tier
    assert cc.fwd_tier(H, cc.aligned(c, keep=False)) == (tier if mis != ("keep",) else "v4x4")
    assert cc.fwd_tier(H, cc.aligned(c, layer_norm=False)) == (tier if not mis or mis == ("W",) else "v4x4" if H <= 1024 else "v4x16")
    if mis:
        assert H % 4 == 0                                                                  # scalar because of the operand alone
        assert cc.fwd_tier(H, True)[0] == "v"


def test_tier_edges_of_the_restated_rule():
    assert [cc.fwd_tier(H, True) for H in (4, 1024, 1028, 4096)] == ["v4x4", "v4x4", "v4x16", "v4x16"]
    assert [cc.fwd_tier(H, True) for H in (2, 1022, 1026, 4094)] == ["s1x4", "s1x16", "s1x64", "s1x64"]
    assert [cc.fwd_tier(H, False) for H in (4, 256, 260, 1024, 1028, 4096)] == ["s1x4", "s1x4", "s1x16", "s1x16", "s1x64", "s1x64"]
    assert [cc.rank_rounds(N) for N in (1, 1024, 1025, 2048, 2049, 8192)] == [1, 1, 2, 2, 3, 8]
    assert cc.scatter_form(8, 16384, True) == ("vec4", False) and cc.scatter_form(6, 16385, True) == ("scalar", True)
    assert cc.scatter_form(8, 50, False) == ("scalar", False)


@pytest.mark.parametrize("name", list(cc.RANK) + list(cc.GRID) + list(cc.PRODUCTION) + list(cc.LN_BWD))
def test_backward_case_reaches_the_rounds_and_the_scatter_form_in_its_name(name):
    c = cc.case(name)
    B, T, H, V = c["shape"]
    ids = c["want_bwd"][0]
    assert _N(c) <= cc.MAX_TOKENS and 0 <= ids.min() and ids.max() < V
    if name in cc.RANK:
        assert cc.rank_rounds(_N(c)) == int(name.split("_")[0][4:])
        assert _N(c) == int(name.split("_")[1][1:])
    form, strided = cc.scatter_form(H, V, True)                                           # (gradient rows and dW are fresh allocations)
    assert form == ("vec4" if H % 4 == 0 else "scalar")
    if name in cc.GRID or name in cc.PRODUCTION:
        assert strided == (V > 16384)
        planted = [int(ids[i, j]) for i, j in c["plant_pos"]]
        assert planted == list(cc.CASES[name][1]["plant_ids"]) and (ids == 0).any()       # every planted id keeps its token; row 0: padding
        want_rows = [r for r in cc.MARK_ROWS + (V - 1,) if r < V]
        assert set(want_rows) <= set(planted)
        if strided:
            assert max(planted) >= 16384 and min(planted) < 16384
    if name in cc.RULE_OFF:
        assert not c["rule"] and np.array_equal(ids, c["ids"])
    else:
        assert c["rule"]


def test_every_branch_is_reached_by_some_case():
    fwd = [cc.case(n) for n in list(cc.FORWARD) + list(cc.PREDICATE)]
    assert {cc.fwd_tier(c["shape"][2], cc.aligned(c)) for c in fwd} == {"v4x4", "v4x16", "s1x4", "s1x16", "s1x64"}
    full = {(cc.fwd_tier(c["shape"][2], cc.aligned(c)), c["shape"][2]) for c in fwd}
    assert {("v4x4", 1024), ("v4x16", 4096), ("s1x4", 256), ("s1x16", 1024), ("s1x64", 4096)} <= full          # every tier filled
    assert {("v4x16", 1028), ("s1x16", 258), ("s1x64", 1026)} <= full                                           # and entered at its edge
    assert {c["misalign"] for c in fwd if c["shape"] == (2, 5, 64, 50)} == {(k,) for k in cr.OPERANDS}
    bwd = [cc.case(n) for n in list(cc.RANK) + list(cc.GRID) + list(cc.PRODUCTION) + list(cc.LN_BWD)]
    assert {1, 2, 8} <= {cc.rank_rounds(_N(c)) for c in bwd}
    forms = {cc.scatter_form(c["shape"][2], c["shape"][3], True) for c in bwd}
    assert forms == {("vec4", False), ("vec4", True), ("scalar", False), ("scalar", True)}
    assert {c["shape"][3] for c in bwd if c["name"] in cc.GRID} == {16384, 16385, 32769}
    assert cc.case("production_v30522_h768")["shape"] == (4, 32, 768, 30522)


def test_run_lengths_of_the_two_n8192_cases():
    spread, zero = cc.case("ln_n8192_spread"), cc.case("rank8_n8192_long_run")
    assert _N(spread) == _N(zero) == 8192
    assert np.bincount(spread["ids"].reshape(-1)).max() <= 8                              # the tokenizer's ids: no id more than 8 times
    counts = np.bincount(spread["want"][0].reshape(-1))                                   # with the rule on, [MASK] would be a long run:
    assert counts.argmax() == spread["mask_id"] and counts.max() > 500                    # the backward case runs on the tokenizer's ids
    assert not spread["rule"] and np.array_equal(spread["want_bwd"][0], spread["ids"])
    assert (zero["ids"] == 0).sum() > 2000 and (zero["want"][0] == 0).sum() > 2000
    assert (zero["ids"] == 0).sum() == 64 * (128 // 3)


@pytest.mark.parametrize("key", list(cc.DEFAULT_CHECKSUMS))
def test_make_case_without_options_is_unchanged(key):
    shape, p_noise = key
    c = cr.make_case(*shape, seed=sum(shape), p_noise=p_noise)
    assert "plant_pos" not in c
    assert cc.checksum(c) == cc.DEFAULT_CHECKSUMS[key]


@pytest.mark.parametrize("name", list(cc.CASES))
def test_boundary_draws_survive_the_options(name):
    c = cc.case(name)
    B, T, H, V = c["shape"]
    ids, special, target, mlm_mask = c["want"]
    assert np.array_equal(target, c["ids"])
    mask = (mlm_mask == 1) & (ids == c["mask_id"]) & (special == 1)
    noise = (mlm_mask == 1) & (ids != target) & (ids != c["mask_id"])
    keep = (mlm_mask == 1) & (ids == target)
    body = (T - T // 3 - 2) * B
    if body == 1:                                                                          # B = 1, T = 4: the last planted draw alone
        assert (B, T) == (1, 4) and mlm_mask.sum() == 1 and keep[0, 1]
    else:
        assert body >= 4 and mask.any() and noise.any() and keep.any()
        assert (ids == c["len_tok"] - 1).any()                                             # the noise draw just below 1.0
    assert not mlm_mask[:, 0].any() and not mlm_mask[:, T - 1].any()                       # a special and a padded token with draw 0.0
