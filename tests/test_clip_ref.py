"""CPU: the CLIP text-tower restatement (tests/clip_ref.py), the yardstick of the native encoder's GPU tests, against transformers itself (tiny
randomly initialised models, nothing is downloaded) and against closed forms that need no transformers."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_ref as R  # noqa: E402

QK_WIDEN = 3.0
TINY = dict(vocab_size=96, hidden_size=128, intermediate_size=256, num_heads=2, max_positions=77)


def close(got, want, what):
    """the parity bound: 1e-5 x max(1, |want|) elementwise (fp32 arithmetic on both sides, different summation orders)"""
    err = ((got - want).abs() / want.abs().clamp(min=1.0)).max().item()
    print(f"{what}: max err / max(1, |want|) = {err:.2e}")
    assert err <= 1e-5, what


# ------------------------------------------------------------------------------------------------------------ parity with transformers
@pytest.mark.parametrize("projected", [False, True])
@pytest.mark.parametrize("act,eos,layers", [("quick_gelu", 2, 2), ("gelu", 2, 3), ("quick_gelu", 7, 3), ("gelu", 7, 2)])
def test_restatement_equals_transformers(act, eos, layers, projected):
    tr = pytest.importorskip("transformers")
    hf_cfg = tr.CLIPTextConfig(vocab_size=96, hidden_size=128, intermediate_size=256, num_hidden_layers=layers, num_attention_heads=2,
                               max_position_embeddings=77, hidden_act=act, projection_dim=64, eos_token_id=eos, bos_token_id=0, pad_token_id=1)
    torch.manual_seed(layers * 10 + eos)
    m = (tr.CLIPTextModelWithProjection if projected else tr.CLIPTextModel)(hf_cfg).eval().float()
    with torch.no_grad():      # the default init gives near-uniform attention: widen q / k so the softmax matters (score std printed below)
        for n, p in m.named_parameters():
            if ".q_proj." in n or ".k_proj." in n:
                p.mul_(QK_WIDEN)
    cfg = R.cfg_from_hf(hf_cfg, projected)
    assert cfg == R.Cfg(hidden_act=act, eos_token_id=eos, num_layers=layers, projection_dim=64 if projected else 0, **TINY)
    ids = R.make_ids(cfg, 3, 77, seed=eos, eos_at=[5, 76, 30])
    with torch.no_grad():
        want = m(input_ids=ids, output_hidden_states=True)
    sd = m.state_dict()
    bare = R.strip_prefix(sd)
    prefixed = {(k if k == "text_projection.weight" else "text_model." + k): v for k, v in bare.items()}
    assert set(R.state_dict_shapes(cfg)) == {k for k in bare if not k.endswith("position_ids")}
    for form, weights in (("bare keys", bare), ("text_model. keys", prefixed)):
        sc = []
        got = R.forward(weights, cfg, ids, dtype=torch.float32, scores_out=sc)
        print(f"{form}: visible score std of layer 0: {sc[0][:, :, torch.ones(77, 77, dtype=torch.bool).tril()].std().item():.2f}")
        assert len(got["hidden_states"]) == layers + 1 == len(want.hidden_states)
        close(got["last_hidden_state"], want.last_hidden_state, f"{form}: last_hidden_state")
        close(got["hidden_states"][-2], want.hidden_states[-2], f"{form}: hidden_states[-2]")
        close(got["hidden_states"][0], want.hidden_states[0], f"{form}: hidden_states[0]")
        if projected:
            close(got["text_embeds"], want.text_embeds, f"{form}: text_embeds")
            assert torch.equal(want[0], want.text_embeds)
        else:
            close(got["pooler_output"], want.pooler_output, f"{form}: pooler_output")
            assert torch.equal(want[0], want.last_hidden_state)


# ------------------------------------------------------------------------------------------------------------ closed forms
@pytest.fixture(scope="module")
def tiny():
    cfg = R.Cfg(hidden_act="gelu", eos_token_id=7, num_layers=2, projection_dim=64, **TINY)
    return cfg, R.random_state_dict(cfg, seed=1)


def test_causality(tiny):
    """ids that differ from position p on leave the rows before p of every hidden state exactly equal"""
    cfg, sd = tiny
    p = 29
    a = R.make_ids(cfg, 2, 77, seed=3)
    b = a.clone()
    b[:, p:] = R.make_ids(cfg, 2, 77, seed=4)[:, p:]
    assert not torch.equal(a[:, p], b[:, p])
    ra, rb = R.forward(sd, cfg, a), R.forward(sd, cfg, b)
    for x, y in zip(ra["hidden_states"] + (ra["last_hidden_state"],), rb["hidden_states"] + (rb["last_hidden_state"],)):
        assert torch.equal(x[:, :p], y[:, :p])
        assert not torch.equal(x[:, p:], y[:, p:])


def test_pooling_rows(tiny):
    cfg, sd = tiny
    ids = R.make_ids(cfg, 3, 77, seed=5, eos_at=[5, 76, None])      # EOS at position 5, at the 77th position, nowhere
    ids[0, 40] = cfg.eos_token_id                                      # a second EOS behind the first does not count
    assert R.eos_positions(ids, cfg.eos_token_id).tolist() == [5, 76, 0]
    out = R.forward(sd, cfg, ids)
    for b, p in enumerate([5, 76, 0]):
        assert torch.equal(out["pooler_output"][b], out["last_hidden_state"][b, p])
    assert torch.allclose(out["text_embeds"], out["pooler_output"] @ sd["text_projection.weight"].double().t(), rtol=0, atol=1e-12)
    # the legacy rule (eos_token_id == 2): the position of the largest id
    legacy = torch.tensor([[0, 9, 95, 3, 94, 1], [4, 5, 4, 4, 4, 4], [1, 2, 3, 50, 2, 60]])
    assert R.eos_positions(legacy, 2).tolist() == [2, 1, 5]
    assert R.eos_positions(legacy, 4).tolist() == [0, 0, 0]
    assert R.eos_positions(legacy, 3).tolist() == [3, 0, 2]


def test_state_dict_shapes_at_clip_l_size():
    """key names and shapes of the SD-v1.5 text encoder against a literal table (the 49408-row embedding is never materialised)"""
    s = R.state_dict_shapes(R.CLIP_L)
    assert len(s) == 2 + 12 * 16 + 2
    table = {"embeddings.token_embedding.weight": (49408, 768), "embeddings.position_embedding.weight": (77, 768),
             "encoder.layers.0.self_attn.k_proj.weight": (768, 768), "encoder.layers.0.self_attn.k_proj.bias": (768,),
             "encoder.layers.0.self_attn.v_proj.weight": (768, 768), "encoder.layers.0.self_attn.v_proj.bias": (768,),
             "encoder.layers.0.self_attn.q_proj.weight": (768, 768), "encoder.layers.0.self_attn.q_proj.bias": (768,),
             "encoder.layers.0.self_attn.out_proj.weight": (768, 768), "encoder.layers.0.self_attn.out_proj.bias": (768,),
             "encoder.layers.0.layer_norm1.weight": (768,), "encoder.layers.0.layer_norm1.bias": (768,),
             "encoder.layers.0.mlp.fc1.weight": (3072, 768), "encoder.layers.0.mlp.fc1.bias": (3072,),
             "encoder.layers.0.mlp.fc2.weight": (768, 3072), "encoder.layers.0.mlp.fc2.bias": (768,),
             "encoder.layers.0.layer_norm2.weight": (768,), "encoder.layers.0.layer_norm2.bias": (768,),
             "final_layer_norm.weight": (768,), "final_layer_norm.bias": (768,)}
    for k, shape in table.items():
        assert s[k] == shape, k
        if k.startswith("encoder.layers.0."):
            assert s[k.replace("layers.0.", "layers.11.")] == shape
    assert "encoder.layers.12.mlp.fc1.weight" not in s and "text_projection.weight" not in s
    g = R.state_dict_shapes(R.CLIP_BIGG)
    assert g["text_projection.weight"] == (1280, 1280) and g["encoder.layers.31.mlp.fc1.weight"] == (5120, 1280) and len(g) == 2 + 32 * 16 + 2 + 1
    small = R.random_state_dict(R.Cfg(num_layers=1, projection_dim=32, **TINY), seed=0, prefix="text_model.")
    assert "text_projection.weight" in small and all(k.startswith("text_model.") for k in small if k != "text_projection.weight")
    assert {k: tuple(v.shape) for k, v in R.strip_prefix(small).items()} == R.state_dict_shapes(R.Cfg(num_layers=1, projection_dim=32, **TINY))


@pytest.mark.parametrize("width,heads,inter", [(128, 2, 256), (768, 12, 3072)])
def test_random_weights_give_peaked_attention(width, heads, inter):
    """random_state_dict's q / k gain: the visible scaled scores of every layer have a standard deviation of 2 - 3.5 (its docstring records
    the measured values), so the softmax of the GPU tests is far from uniform"""
    cfg = R.Cfg(vocab_size=96, hidden_size=width, intermediate_size=inter, num_layers=2, num_heads=heads)
    sc = []
    R.forward(R.random_state_dict(cfg, seed=2), cfg, R.make_ids(cfg, 3, 77, seed=1, eos_at=[5, 76, 30]), dtype=torch.float64, scores_out=sc)
    vis = torch.ones(77, 77, dtype=torch.bool).tril()
    for l, s in enumerate(sc):
        sd_ = s[:, :, vis].std().item()
        print(f"hidden {width}, layer {l}: visible score std {sd_:.2f}")
        assert 2.0 <= sd_ <= 3.5
