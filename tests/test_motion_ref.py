"""CPU: the restatement tests/motion_ref.py against the reference's own VanillaTemporalModule, through golden g20 (tests/golden/make_golden_motion.py:
in_channels 64, 4 heads, two blocks of two Temporal_Self attentions, position encoding with max_len 24, seeded weights with a non-zero proj_out, input
[2, 64, 5, 3, 2])."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_ref as R  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g20_motion_module.pt")
CFG = R.Cfg(channels=64, num_heads=4, num_blocks=2, attn_per_block=2, max_len=24)


@pytest.fixture(scope="module")
def g20():
    g = torch.load(GOLD)
    assert os.path.getsize(GOLD) < 512 * 1024
    return {"sd": {k: v.float() for k, v in g["state_dict"].items()}, "x": g["input"], "y": g["output"]}


def test_fixture_pins_something(g20):
    assert tuple(g20["x"].shape) == (2, 64, 5, 3, 2) and g20["y"].shape == g20["x"].shape
    assert g20["sd"]["temporal_transformer.proj_out.weight"].abs().max() > 0
    assert (g20["y"] - g20["x"]).abs().max() > 0.1
    assert {k: tuple(v.shape) for k, v in g20["sd"].items()} == R.state_dict_shapes(CFG)


def test_fp32_restatement_reproduces_the_reference(g20):
    """the project's bar for the CLIP and T5 restatements: 1e-5 x max(1, |want|) elementwise"""
    got = R.forward(g20["sd"], CFG, g20["x"], dtype=torch.float32)
    want = g20["y"]
    frac = ((got - want).abs() / (1e-5 * want.abs().clamp(min=1.0))).max().item()
    print(f"g20: max |got - want| = {(got - want).abs().max().item():.3e}, worst fraction of the bound {frac:.3f}, max|want| {want.abs().max().item():.2f}")
    assert frac <= 1.0


def test_a_loaded_position_table_replaces_the_formula(g20):
    """published checkpoints carry ...pos_encoder.pe [1, max_len, C]; with the same sinusoid under that key the result is unchanged, and another
    table changes it"""
    base = R.forward(g20["sd"], CFG, g20["x"], dtype=torch.float32)
    sd = dict(g20["sd"])
    for b in range(CFG.num_blocks):
        for i in range(CFG.attn_per_block):
            sd[f"temporal_transformer.transformer_blocks.{b}.attention_blocks.{i}.pos_encoder.pe"] = R.position_table(24, 64)
    assert torch.equal(R.forward(sd, CFG, g20["x"], dtype=torch.float32), base)
    sd["temporal_transformer.transformer_blocks.0.attention_blocks.0.pos_encoder.pe"] = R.position_table(24, 64).flip(1)
    assert not torch.equal(R.forward(sd, CFG, g20["x"], dtype=torch.float32), base)
