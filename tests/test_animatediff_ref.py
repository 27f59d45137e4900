"""CPU: the restatement tests/animatediff_ref.py against the reference's own AnimateDiff UNet3DConditionModel and pnp_utils, through golden g21
(tests/golden/make_golden_animatediff.py: block_out_channels (32, 32, 64, 64), layers_per_block 2, cross_attention_dim 16, 2 heads, 8 norm groups, the
v2 kwargs with 2 motion heads, a non-zero proj_out and max_len 24, input [3, 4, 3, 16, 16]; everything in float64; weights drawn from the seed, not
stored)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import animatediff_ref as R  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "g21_animatediff_unet.pt")
CASES = {"stock": None, "pnp0": 0, "pnp24": 24, "pnp25": 25}


@pytest.fixture(scope="module")
def g21():
    assert os.path.getsize(GOLD) < 512 * 1024
    return torch.load(GOLD)


@pytest.fixture(scope="module")
def sd(g21):
    return R.random_state_dict(R.G21_CFG, seed=g21["seed"])


def test_fixture_pins_something(g21):
    assert tuple(g21["sample"].shape) == (3, 4, 3, 16, 16) and g21["sample"].dtype == torch.float64
    assert all(g21[k].shape == g21["sample"].shape and g21[k].dtype == torch.float64 for k in CASES)
    assert "state_dict" not in g21, "weights are drawn from the seed, not stored"
    names = dict(g21["names"])
    assert sum(k.endswith("temporal_transformer.proj_out.weight") for k in names) == 21, "2 per down block, 3 per up block, 1 in the mid block"
    assert names == R.state_dict_shapes(R.G21_CFG)
    assert [k for k, _ in g21["names"]] == list(R.state_dict_shapes(R.G21_CFG)), "the module tree's order"


@pytest.mark.parametrize("case", list(CASES))
def test_fp64_restatement_reproduces_the_reference(g21, sd, case):
    """the project's bar (test_motion_ref.py): 1e-5 x max(1, |want|) elementwise"""
    idx = CASES[case]
    got = R.unet_forward(sd, R.G21_CFG, g21["sample"], g21["timestep"], g21["text"], pnp=None if idx is None else dict(idx=idx, eta1=g21["eta1"], eta2=g21["eta2"]))
    want = g21[case]
    frac = ((got - want).abs() / (1e-5 * want.abs().clamp(min=1.0))).max().item()
    print(f"g21 {case}: max |got - want| = {(got - want).abs().max().item():.3e}, worst fraction of the bound {frac:.3e}, max|want| {want.abs().max().item():.2f}")
    assert frac <= 1.0


def test_report_carries_the_worst_fraction():
    text = open(os.path.join(HERE, "golden", "REPORT_animatediff.txt")).read()
    for case in CASES:
        line = [ln for ln in text.splitlines() if ln.startswith("g21_" + case + " ")]
        assert len(line) == 1 and float(line[0].rsplit(":", 1)[1]) <= 1.0, line


def test_the_window_is_exclusive_at_the_top(g21, sd):
    """idx 25 = eta2 * 50 equals the stock forward bit for bit, in the reference (the fixture) and in the restatement; inside the window only
    branch 2 changes"""
    assert torch.equal(g21["pnp25"], g21["stock"])
    stock = R.unet_forward(sd, R.G21_CFG, g21["sample"], g21["timestep"], g21["text"])
    assert torch.equal(R.unet_forward(sd, R.G21_CFG, g21["sample"], g21["timestep"], g21["text"], pnp=dict(idx=25, eta1=0.0, eta2=0.5)), stock)
    for k in ("pnp0", "pnp24"):
        assert torch.equal(g21[k][:2], g21["stock"][:2]) and (g21[k][2] - g21["stock"][2]).abs().max() > 1e-3
    assert not torch.equal(g21["pnp0"], g21["pnp24"]), "beta depends on idx"
    assert R.in_window(0, 0.0, 0.5) and R.in_window(24, 0.0, 0.5) and not R.in_window(25, 0.0, 0.5)
    assert not R.in_window(9, 0.2, 0.5) and R.in_window(10, 0.2, 0.5), "eta1 is scaled by 50 (the SD path compares idx with eta1 itself)"


def test_zero_proj_out_is_the_per_frame_2d_unet(sd, g21):
    """zero_initialize: every motion module returns its input, so the UNet with motion modules equals the one configured without"""
    cfg0 = dict(R.G21_CFG, motion_levels=(False,) * 4, motion_mid_block=False)
    zero = R.random_state_dict(R.G21_CFG, seed=g21["seed"], zero_motion=True)
    a = R.unet_forward(zero, R.G21_CFG, g21["sample"], g21["timestep"], g21["text"])
    b = R.unet_forward({k: v for k, v in zero.items() if ".motion_modules." not in k}, cfg0, g21["sample"], g21["timestep"], g21["text"])
    assert torch.equal(a, b)
    assert (a - g21["stock"]).abs().max() > 1e-3, "the modules of the fixture do something"


def test_mirror_keeps_the_reference_names_and_shapes(g21):
    from univst_amd.backbones.animatediff.models.unet import UNet3DConditionModel
    m = UNet3DConditionModel(**R.reference_kwargs(R.G21_CFG))
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(s)) for k, s in g21["names"]]
    assert m.config.use_inflated_groupnorm is True and m.config.motion_module_kwargs["num_attention_heads"] == 2
    assert m._motion_mask == 15 and m._motion_mid
