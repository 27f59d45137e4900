"""CPU: the fp32 restatement of torchvision's raft_large (tests/raft_ref.py) against closed forms — it is the yardstick the native
estimator is held to (tests/test_gpu_raft.py), so its lookup order, pooling, border handling and upsampling are pinned here."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raft_ref as R  # noqa: E402


def _onehot_pair(h, w, y0, x0, dx, dy):
    f1 = torch.zeros(1, 8, h, w)
    f2 = torch.zeros(1, 8, h, w)
    f1[0, 0, y0, x0] = 1.0
    f2[0, 0, y0 + dy, x0 + dx] = 1.0          # fmap2 = fmap1 shifted by (dx, dy)
    return f1, f2


@pytest.mark.parametrize("dx,dy", [(2, 0), (0, 3), (-3, 0), (0, -1), (1, 2)])
def test_lookup_peak_channel_follows_the_a_moves_x_rule(dx, dy):
    """channel a*9 + b of level 0 samples x + (a - 4), y + (b - 4): a shift in x only moves a, a shift in y only moves b"""
    h, w, y0, x0 = 16, 20, 7, 9
    f1, f2 = _onehot_pair(h, w, y0, x0, dx, dy)
    feats = R.index_pyramid(R.build_pyramid(f1, f2), R.make_coords_grid(1, h, w))
    row = feats[0, :81, y0, x0]
    assert int(row.argmax()) == (dx + 4) * 9 + (dy + 4)
    assert row.max().item() == pytest.approx(1.0 / 8 ** 0.5, rel=1e-5) and (row > 1e-6).sum() == 1


def test_pooling_of_an_odd_sized_level_drops_the_last_row_and_column():
    g = torch.Generator().manual_seed(1)
    f1, f2 = torch.randn(1, 8, 17, 25, generator=g), torch.randn(1, 8, 17, 25, generator=g)
    pyr = R.build_pyramid(f1, f2)
    assert [tuple(p.shape[-2:]) for p in pyr] == [(17, 25), (8, 12), (4, 6), (2, 3)]
    l0 = pyr[0][:, 0]
    want = l0[:, :16, :24].reshape(-1, 8, 2, 12, 2).mean(dim=(2, 4))
    assert torch.allclose(pyr[1][:, 0], want, atol=1e-6)
    poked = l0.clone()
    poked[:, 16, :] += 100.0
    poked[:, :, 24] += 100.0
    assert torch.equal(torch.nn.functional.avg_pool2d(poked[:, None], 2, 2), pyr[1])


def test_samples_outside_the_volume_are_zero():
    g = torch.Generator().manual_seed(2)
    h, w = 16, 16
    f1, f2 = torch.randn(1, 8, h, w, generator=g), torch.randn(1, 8, h, w, generator=g)
    pyr = R.build_pyramid(f1, f2)
    far = R.make_coords_grid(1, h, w) * 0 - 100.0          # level 3 still samples at -12.5 + 4 < -1
    assert R.index_pyramid(pyr, far).abs().max().item() == 0.0
    # centroid (0, 0): every tap with a < 3 (x <= -2) or b < 3 is outside at level 0; (a, b) = (4, 4) is the volume's corner value
    z = R.index_pyramid(pyr, R.make_coords_grid(1, h, w) * 0)
    lvl0 = z[0, :81, 5, 5].view(9, 9)
    assert lvl0[:3].abs().max() == 0 and lvl0[:, :3].abs().max() == 0
    assert lvl0[4, 4].item() == pytest.approx(pyr[0][5 * w + 5, 0, 0, 0].item(), abs=1e-6)
    # one pixel past the last column with a fraction: only the x0 = w - 1 tap contributes, weight 0.75
    c = R.make_coords_grid(1, h, w) * 0
    c[:, 0] = w - 1 + 0.25
    c[:, 1] = 3.0
    v = R.index_pyramid(pyr, c)[0, 4 * 9 + 4, 2, 2]
    assert v.item() == pytest.approx(0.75 * pyr[0][2 * w + 2, 0, 3, w - 1].item(), abs=1e-5)


def test_convex_upsample_with_a_constant_mask_is_the_box_mean():
    g = torch.Generator().manual_seed(3)
    flow = torch.randn(1, 2, 5, 7, generator=g)
    up = R.upsample_flow(flow, torch.full((1, 576, 5, 7), 0.3))
    box = torch.nn.functional.avg_pool2d(8 * flow, 3, stride=1, padding=1, count_include_pad=True)
    want = box.repeat_interleave(8, dim=2).repeat_interleave(8, dim=3)
    assert up.shape == (1, 2, 40, 56) and torch.allclose(up, want, atol=1e-5)


def test_state_dict_keys_are_torchvisions():
    sd = R.RAFT().state_dict()
    for k, shape in {"feature_encoder.convnormrelu.0.weight": (64, 3, 7, 7), "feature_encoder.layer2.0.downsample.0.bias": (96,),
                     "context_encoder.layer3.1.convnormrelu2.1.running_var": (128,), "context_encoder.conv.weight": (256, 128, 1, 1),
                     "update_block.motion_encoder.convcorr1.0.weight": (256, 324, 1, 1), "update_block.motion_encoder.conv.0.weight": (126, 256, 3, 3),
                     "update_block.recurrent_block.convgru1.convz.weight": (128, 384, 1, 5), "update_block.recurrent_block.convgru2.convq.weight": (128, 384, 5, 1),
                     "update_block.flow_head.conv2.weight": (2, 256, 3, 3), "mask_predictor.convrelu.0.weight": (256, 128, 3, 3),
                     "mask_predictor.conv.bias": (576,)}.items():
        assert tuple(sd[k].shape) == shape, k
    assert not any("feature_encoder" in k and ".1." in k and "layer" not in k.split(".1.")[0][-6:] and k.endswith("running_mean") for k in sd)
    assert sum(v.numel() for k, v in sd.items() if v.dtype.is_floating_point and "running" not in k) == 5257536      # raft_large's parameter count


def test_restatement_equals_torchvision_raft_large():
    """pins the restatement to the third-party definition where torchvision is installed (it is not on the project's machines: skipped there)"""
    tv = pytest.importorskip("torchvision")
    from torchvision.models.optical_flow import raft_large
    sd = R.random_state_dict(0, 1.0, 6.0)
    ref = raft_large(weights=None).eval()
    ref.load_state_dict(sd, strict=True)
    mine = R.RAFT().eval()
    mine.load_state_dict(ref.state_dict(), strict=True)
    a, b = R.make_images(128, 136)
    with torch.no_grad():
        want = ref(R.preprocess(a), R.preprocess(b))[-1]
    got = mine(R.preprocess(a), R.preprocess(b))[-1]
    assert (got - want).abs().max().item() < 1e-5 * max(1.0, want.abs().max().item())
