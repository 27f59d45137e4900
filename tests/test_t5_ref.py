"""CPU: tests/t5_ref.py — the restatement the native T5 encoder is tested against — held to the installed transformers T5EncoderModel at tiny
random configs (inner width 128 != d_model 64), at sequence lengths below, at and past relative_attention_max_distance."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import t5_ref as R  # noqa: E402

TINY = R.Cfg(vocab_size=96, d_model=64, d_ff=128, num_layers=2, num_heads=2, d_kv=64)


@pytest.fixture(scope="module")
def pair():
    """(state dict, transformers module with it loaded), built once"""
    transformers = pytest.importorskip("transformers")
    sd = R.random_state_dict(TINY, seed=4)
    m = transformers.T5EncoderModel(transformers.T5Config(**R.hf_config(TINY), is_encoder_decoder=False, use_cache=False, dropout_rate=0.0)).eval()
    full = dict(sd)
    full["encoder.embed_tokens.weight"] = sd["shared.weight"]
    missing, unexpected = m.load_state_dict(full, strict=False)
    assert not unexpected and not [k for k in missing if "embed_tokens" not in k and "shared" not in k], (missing, unexpected)
    return sd, m


@pytest.mark.parametrize("S", [1, 17, 140])
def test_restatement_equals_transformers(pair, S):
    """fp32 on the CPU, B = 2; 140 > max_distance 128, so the saturated bucket occurs.  Tolerance 1e-5 x max(1, |want|)"""
    sd, m = pair
    ids = R.make_ids(TINY, 2, S, seed=S)
    with torch.no_grad():
        want = m(input_ids=ids).last_hidden_state
        got = R.forward(sd, TINY, ids, dtype=torch.float32)
    err = ((got - want).abs() / want.abs().clamp(min=1.0)).max().item()
    print(f"S={S}: worst |got - want| / max(1, |want|) = {err:.2e}, max|want| {want.abs().max().item():.2f}")
    assert got.shape == want.shape == (2, S, TINY.d_model) and err <= 1e-5
    if S == 140:
        pos = torch.arange(S)
        b = R.relative_position_bucket(pos[None, :] - pos[:, None])
        assert b.max().item() == 31 and b.min().item() == 0 and (b == 15).any()      # both saturated buckets are in use


def test_embedding_key_forms_and_residual_dtype():
    sd = R.random_state_dict(TINY, seed=5)
    alt = {("encoder.embed_tokens.weight" if k == "shared.weight" else k): v for k, v in sd.items()}
    ids = R.make_ids(TINY, 2, 17, seed=1)
    a, b = R.forward(sd, TINY, ids, dtype=torch.float32), R.forward(alt, TINY, ids, dtype=torch.float32)
    assert torch.equal(a, b)
    c = R.forward(sd, TINY, ids, dtype=torch.float16, residual_dtype=torch.float32)
    assert c.dtype == torch.float16 and (c.float() - a).abs().max().item() < 0.05


def test_random_weights_give_peaked_attention():
    """the scores of the random weights are neither uniform nor saturated: standard deviation in the 2 - 4 window (prints it)"""
    sd = R.random_state_dict(TINY, seed=6)
    sc = []
    R.forward(sd, TINY, R.make_ids(TINY, 2, 140, seed=2), dtype=torch.float64, scores_out=sc)
    stds = [s.std().item() for s in sc]
    print("score std per layer:", [f"{s:.2f}" for s in stds])
    assert all(2.0 <= s <= 4.0 for s in stds)
