"""CPU: the UNIVST_TEXT_ENCODER switch of the entry points (univst_amd/src/sd/_common.py load_text_encoder, shared with src/sd3) and the parts of
NativeCLIPText.from_pretrained that run before the library is touched.  No GPU, no checkpoint."""
import json

import pytest
import torch

from univst_amd.src.sd import _common
from univst_amd.text import CLIPTextOutput, NativeCLIPText


def test_native_needs_fp16_and_a_local_directory(monkeypatch, tmp_path):
    monkeypatch.setenv("UNIVST_TEXT_ENCODER", "native")
    with pytest.raises(ValueError, match="fp16 only"):
        _common.load_text_encoder(str(tmp_path), "text_encoder", torch.float32, projected=False)
    with pytest.raises(FileNotFoundError, match="needs a local directory"):
        _common.load_text_encoder(str(tmp_path), "text_encoder", torch.float16, projected=False)
    (tmp_path / "text_encoder").mkdir()
    with pytest.raises(FileNotFoundError, match="config.json not found"):
        _common.load_text_encoder(str(tmp_path), "text_encoder", torch.float16, projected=True)


def test_unknown_mode_is_an_error(monkeypatch, tmp_path):
    monkeypatch.setenv("UNIVST_TEXT_ENCODER", "fast")
    with pytest.raises(ValueError, match="'stock' or 'native'"):
        _common.load_text_encoder(str(tmp_path), "text_encoder", torch.float16, projected=False)


def test_from_pretrained_refuses_other_architectures_and_missing_weights(tmp_path):
    d = tmp_path / "m" / "text_encoder_3"
    d.mkdir(parents=True)
    (d / "config.json").write_text(json.dumps({"architectures": ["T5EncoderModel"]}))
    with pytest.raises(ValueError, match="CLIPTextModel / CLIPTextModelWithProjection only"):
        NativeCLIPText.from_pretrained(str(tmp_path / "m"), subfolder="text_encoder_3")
    (d / "config.json").write_text(json.dumps({"architectures": ["CLIPTextModel"]}))
    with pytest.raises(FileNotFoundError, match="no model.safetensors"):
        NativeCLIPText.from_pretrained(str(tmp_path / "m"), subfolder="text_encoder_3")


def test_output_object_indexes_like_transformers():
    a, b = torch.zeros(1), torch.ones(1)
    o = CLIPTextOutput([("last_hidden_state", a), ("pooler_output", b), ("hidden_states", None)])
    assert o[0] is a and o[1] is b and len(o) == 2 and o["pooler_output"] is b and o.hidden_states is None and o.to_tuple() == (a, b)
    p = CLIPTextOutput([("text_embeds", b), ("last_hidden_state", a), ("hidden_states", (a, a))])
    assert p[0] is b and p[2] == (a, a) and p.text_embeds is b
