"""CPU: the UNIVST_T5_ENCODER switch of the SD3 entry points (univst_amd/src/sd3/_common.py load_t5_encoder) and the parts of
NativeT5Encoder.from_pretrained that run before the library is touched: config checks and the weight-file reader.  No GPU, no checkpoint."""
import json

import pytest
import torch

from univst_amd.src.sd3 import _common
from univst_amd.text import NativeT5Encoder, T5EncoderOutput, read_weight_files, t5_config_from_dir, t5_tensors


def test_unknown_mode_is_an_error(monkeypatch, tmp_path):
    monkeypatch.setenv("UNIVST_T5_ENCODER", "fast")
    with pytest.raises(ValueError, match="UNIVST_T5_ENCODER='fast': 'stock' or 'native'"):
        _common.load_t5_encoder(str(tmp_path), "text_encoder_3", torch.float16)


def test_native_needs_fp16_and_a_local_directory(monkeypatch, tmp_path):
    monkeypatch.setenv("UNIVST_T5_ENCODER", "native")
    with pytest.raises(ValueError, match="fp16 only"):
        _common.load_t5_encoder(str(tmp_path), "text_encoder_3", torch.float32)
    with pytest.raises(FileNotFoundError, match="needs a local directory"):
        _common.load_t5_encoder(str(tmp_path), "text_encoder_3", torch.float16)
    (tmp_path / "text_encoder_3").mkdir()
    with pytest.raises(FileNotFoundError, match="config.json not found"):
        _common.load_t5_encoder(str(tmp_path), "text_encoder_3", torch.float16)


def test_the_clip_switch_does_not_move_t5(monkeypatch, tmp_path):
    """UNIVST_TEXT_ENCODER keeps its meaning: alone it leaves T5 on the stock path (which then asks transformers for the missing directory)"""
    pytest.importorskip("transformers")
    monkeypatch.setenv("UNIVST_TEXT_ENCODER", "native")
    monkeypatch.delenv("UNIVST_T5_ENCODER", raising=False)
    with pytest.raises(Exception) as e:
        _common.load_t5_encoder(str(tmp_path), "text_encoder_3", torch.float16)
    assert "UNIVST_T5_ENCODER" not in str(e.value)


def test_from_pretrained_refuses_other_architectures_and_feed_forwards(tmp_path):
    d = tmp_path / "m" / "text_encoder_3"
    d.mkdir(parents=True)
    (d / "config.json").write_text(json.dumps({"architectures": ["CLIPTextModel"]}))
    with pytest.raises(ValueError, match="T5EncoderModel only"):
        NativeT5Encoder.from_pretrained(str(tmp_path / "m"))
    (d / "config.json").write_text(json.dumps({"architectures": ["T5EncoderModel"], "feed_forward_proj": "relu"}))
    with pytest.raises(ValueError, match="feed_forward_proj = 'relu'"):
        NativeT5Encoder.from_pretrained(str(tmp_path / "m"))
    (d / "config.json").write_text(json.dumps({"architectures": ["T5EncoderModel"], "feed_forward_proj": "gated-gelu", "d_model": 64}))
    got_dir, raw = t5_config_from_dir(str(tmp_path / "m"))
    assert got_dir == str(d) and raw["d_model"] == 64
    with pytest.raises(FileNotFoundError, match="no model.safetensors"):
        NativeT5Encoder.from_pretrained(str(tmp_path / "m"))


def _tensors():
    g = torch.Generator().manual_seed(0)
    return {"shared.weight": torch.randn(8, 4, generator=g).half(), "encoder.block.0.layer.0.layer_norm.weight": torch.randn(4, generator=g).half(),
            "encoder.block.1.layer.1.DenseReluDense.wo.weight": torch.randn(4, 8, generator=g).half(), "encoder.final_layer_norm.weight": torch.randn(4, generator=g).half()}


def _same(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_weight_files_single_sharded_and_bin(tmp_path):
    from safetensors.torch import save_file
    sd = _tensors()
    keys = list(sd)
    for i, name in enumerate(("model.safetensors", "model.fp16.safetensors")):
        d = tmp_path / f"single{i}"
        d.mkdir()
        save_file(sd, str(d / name))
        assert _same(read_weight_files(str(d)), sd)
    for i, (index, stem) in enumerate((("model.safetensors.index.json", "model"), ("model.fp16.safetensors.index.json", "model.fp16"))):
        d = tmp_path / f"sharded{i}"
        d.mkdir()
        files = [f"{stem}-0000{j + 1}-of-00002.safetensors" for j in range(2)]
        save_file({k: sd[k] for k in keys[:2]}, str(d / files[0]))
        save_file({k: sd[k] for k in keys[2:]}, str(d / files[1]))
        (d / index).write_text(json.dumps({"metadata": {"total_size": 1}, "weight_map": {k: files[0 if j < 2 else 1] for j, k in enumerate(keys)}}))
        assert _same(read_weight_files(str(d)), sd)
        (d / files[1]).unlink()
        with pytest.raises(FileNotFoundError, match="00002-of-00002"):
            read_weight_files(str(d))
    d = tmp_path / "bin"
    d.mkdir()
    torch.save(sd, str(d / "pytorch_model.bin"))
    assert _same(read_weight_files(str(d)), sd)
    with pytest.raises(FileNotFoundError, match="no model.safetensors"):
        read_weight_files(str(tmp_path))


def test_tied_embedding_under_either_name_is_kept_once():
    sd = _tensors()
    emb = sd["shared.weight"]
    other = {k: v for k, v in sd.items() if k != "shared.weight"}
    for form in ({"shared.weight": emb}, {"encoder.embed_tokens.weight": emb}, {"shared.weight": emb, "encoder.embed_tokens.weight": emb.clone()}):
        got = t5_tensors({**form, **other, "decoder.block.0.layer.0.layer_norm.weight": emb, "lm_head.weight": emb, "encoder.position_ids": torch.arange(3)})
        assert _same(got, sd) and got["shared.weight"] is emb


def test_output_object_indexes_like_transformers():
    a = torch.zeros(1)
    o = T5EncoderOutput(a)
    assert o[0] is a and o.last_hidden_state is a and o["last_hidden_state"] is a and len(o) == 1 and o.to_tuple() == (a,)
