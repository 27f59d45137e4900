"""CPU: the MX-fp8 entries (univst_mxfp8_quantize, univst_linear_mxfp8, univst_sd3_joint_attention_mx) are in the header, the binding and the
library; what they refuse, they refuse before any device call (this box has no GPU: a launch or an allocation would fail with UNIVST_ERR_HIP, not
UNIVST_ERR_ARG); the model's switch and the CLI flag validate their values and default to fp16."""
import argparse
import ctypes as C
import os
import re
import subprocess
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("univst_mxfp8_quantize", "univst_linear_mxfp8", "univst_sd3_joint_attention_mx")
ERR_ARG, ERR_UNSUPPORTED = -1, -3
P = 0x10000          # a well-aligned address that is never dereferenced: every call below must return before it touches the device


@pytest.fixture(scope="module")
def lib():
    from univst_amd import _native
    if not os.path.exists(_native.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return _native.load()


def test_entries_exist_in_header_binding_and_library(lib):
    from univst_amd import _native
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "univst.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _native.lib_path()], capture_output=True, text=True, check=True).stdout
    for name in ENTRIES:
        assert re.search(rf"\bint {name}\s*\(", src), f"{name} is not declared in include/univst.h"
        assert name in _native.SIGNATURES and hasattr(lib, name)
        assert re.search(rf" T {name}$", out, flags=re.M), f"{name} is not exported"
    assert "univst_sd3_mx_weights" in src
    assert [f[0] for f in _native.Sd3MxWeights._fields_] == ["qkv", "qkv_scale", "add_qkv", "add_qkv_scale"]
    # the new attention entry takes the old one's arguments plus the MX weights
    old, new = _native.SIGNATURES["univst_sd3_joint_attention"], _native.SIGNATURES["univst_sd3_joint_attention_mx"]
    assert new[0] is old[0] and new[1][:-1] == old[1] and new[1][-1] is C.POINTER(_native.Sd3MxWeights)
    assert int(re.search(r"#define UNIVST_ABI_VERSION (\d+)", src).group(1)) == 3


def _err(lib):
    return lib.univst_last_error().decode()


@pytest.mark.parametrize("M,N,K,what", [(64, 64, 192, "K"), (64, 64, 64, "K"), (64, 24, 128, "N"), (64, 8, 128, "N"), (0, 64, 128, "M")])
def test_linear_mxfp8_refuses_shapes_before_any_launch(lib, M, N, K, what):
    assert lib.univst_linear_mxfp8(P, P, P, P, None, P, N, M, N, K, None) == ERR_ARG
    assert "linear_mxfp8" in _err(lib) and f"{what}=" in _err(lib)


def test_linear_mxfp8_refuses_null_and_misaligned_arguments(lib):
    for i in (0, 1, 2, 3, 5):                     # Xq, Xs, Wq, Ws, Y; the bias (4) may be NULL
        a = [P, P, P, P, None, P]
        a[i] = None
        assert lib.univst_linear_mxfp8(*a, 64, 64, 64, 128, None) == ERR_ARG and "null" in _err(lib)
    assert lib.univst_linear_mxfp8(P, P, P, P, None, P, 48, 64, 64, 128, None) == ERR_ARG and "ldy" in _err(lib)          # ldy < N
    assert lib.univst_linear_mxfp8(P, P, P, P, None, P, 66, 64, 64, 128, None) == ERR_ARG and "ldy" in _err(lib)          # 8-byte stores
    assert lib.univst_linear_mxfp8(P + 8, P, P, P, None, P, 64, 64, 64, 128, None) == ERR_ARG and "aligned" in _err(lib)


def test_mxfp8_quantize_refuses_before_any_launch(lib):
    assert lib.univst_mxfp8_quantize(P, 48, 4, 48, P, P, None) == ERR_ARG and "multiple of the 32-element MX block" in _err(lib)
    assert lib.univst_mxfp8_quantize(P, 64, 0, 64, P, P, None) == ERR_ARG
    assert lib.univst_mxfp8_quantize(P, 32, 4, 64, P, P, None) == ERR_ARG and "ldx" in _err(lib)                             # ldx < K
    assert lib.univst_mxfp8_quantize(P, 68, 4, 64, P, P, None) == ERR_ARG and "ldx" in _err(lib)                             # 16-byte loads
    for a in ((None, P, P), (P, None, P), (P, P, None)):
        assert lib.univst_mxfp8_quantize(a[0], 64, 4, 64, a[1], a[2], None) == ERR_ARG and "null" in _err(lib)


def _attn_call(lib, Cin, C_, fused=True, mx=True, enc=True):
    from univst_amd import _native
    heads, hd = C_ // 64, 64
    w = _native.Sd3AttnWeights()
    step = C_ * Cin * 2
    for base, trio in ((0x100000, ("to_q", "to_k", "to_v")), (0x800000, ("add_q", "add_k", "add_v"))):
        for i, n in enumerate(trio):
            setattr(w, n, base + i * (step if fused else step + 64))
    w.to_out = 0x1000000
    m = _native.Sd3MxWeights(P, P, P, P) if mx else None
    return lib.univst_sd3_joint_attention_mx(C.byref(w), P, P if enc else None, 6, 64, 8 if enc else 0, Cin, heads, hd, 2, 0, 0.0, 1e-6, P, P if enc else None,
                                             None, None, None, C.byref(m) if m is not None else None)


def test_attention_mx_refuses_widths_and_layouts_before_any_device_call(lib):
    assert _attn_call(lib, 64, 128) == ERR_ARG and "Cin=64 must be a multiple of 128" in _err(lib)
    assert _attn_call(lib, 192, 128) == ERR_ARG and "multiple of 128" in _err(lib)
    assert _attn_call(lib, 128, 128, fused=False) == ERR_ARG and "consecutive" in _err(lib)
    from univst_amd import _native
    w = _native.Sd3AttnWeights(to_q=0x100000, to_k=0x100000 + 128 * 128 * 2, to_v=0x100000 + 2 * 128 * 128 * 2, to_out=0x1000000)
    m = _native.Sd3MxWeights(P, None, None, None)
    rc = lib.univst_sd3_joint_attention_mx(C.byref(w), P, None, 6, 64, 0, 128, 2, 64, 2, 0, 0.0, 1e-6, P, None, None, None, None, C.byref(m))
    assert rc == ERR_ARG and "scales are required" in _err(lib)


def _tiny(heads):
    from univst_amd.backbones.video_diffusion_sd3.models.transformer_3D_model import CustomSD3Transformer2DModel
    return CustomSD3Transformer2DModel(sample_size=32, patch_size=2, in_channels=16, num_layers=2, attention_head_dim=64, num_attention_heads=heads,
                                       joint_attention_dim=64, caption_projection_dim=64 * heads, pooled_projection_dim=32, out_channels=16,
                                       pos_embed_max_size=24, dual_attention_layers=(0,), qk_norm="rms_norm")


def test_set_qkv_dtype_validates_and_defaults_to_fp16(monkeypatch):
    monkeypatch.delenv("UNIVST_SD3_QKV", raising=False)
    m = _tiny(2)
    attns = [m.transformer_blocks[0].attn, m.transformer_blocks[0].attn2, m.transformer_blocks[1].attn]
    assert m.qkv_dtype == "fp16" and all(a.qkv_dtype == "fp16" for a in attns)
    assert m.set_qkv_dtype("mxfp8") is m and m.qkv_dtype == "mxfp8" and all(a.qkv_dtype == "mxfp8" for a in attns)
    m.set_qkv_dtype("fp16")
    assert m.qkv_dtype == "fp16" and all(a.qkv_dtype == "fp16" for a in attns)
    with pytest.raises(ValueError, match="'fp16' or 'mxfp8'"):
        m.set_qkv_dtype("fp8")
    with pytest.raises(ValueError, match="inner dim 64 is not a multiple of 128"):
        _tiny(1).set_qkv_dtype("mxfp8")
    attns[1]._uv_frame_shard = types.SimpleNamespace(world=2)          # what parallel.Sd3FrameShard.attach leaves on the attention modules
    with pytest.raises(RuntimeError, match=r"frame-sharded \(world 2\)"):
        m.set_qkv_dtype("mxfp8")
    assert m.qkv_dtype == "fp16" and all(a.qkv_dtype == "fp16" for a in attns)          # nothing was switched
    attns[1]._uv_frame_shard = types.SimpleNamespace(world=1)
    m.set_qkv_dtype("mxfp8")


def test_environment_switch_sets_the_dtype_at_construction(monkeypatch):
    monkeypatch.setenv("UNIVST_SD3_QKV", "mxfp8")
    m = _tiny(2)
    assert m.qkv_dtype == "mxfp8" and m.transformer_blocks[1].attn.qkv_dtype == "mxfp8"
    with pytest.raises(ValueError, match="multiple of 128"):
        _tiny(1)
    monkeypatch.setenv("UNIVST_SD3_QKV", "int8")
    with pytest.raises(ValueError, match="'fp16' or 'mxfp8'"):
        _tiny(2)


def test_binding_refuses_an_unknown_qkv_dtype_and_a_width_the_mfma_does_not_take():
    from univst_amd import _native
    with pytest.raises(ValueError, match="qkv_dtype must be 'fp16' or 'mxfp8'"):
        _native.sd3_joint_attention({}, torch.zeros(1, 1, 8), None, 1, qkv_dtype="bf16")
    g = torch.Generator().manual_seed(0)
    sd = {f"{n}.weight": torch.randn(64, 64, generator=g) for n in ("to_q", "to_k", "to_v")}
    sd["to_out.0.weight"] = torch.randn(64, 64, generator=g)
    with pytest.raises(RuntimeError, match="multiple of 128, got 64"):
        _native.Sd3AttnParams(sd, "cpu").mx()


def test_cli_flag_parses_and_defaults_to_fp16():
    from univst_amd.src.sd3._common import add_common_args
    p = add_common_args(argparse.ArgumentParser())
    assert p.parse_args([]).qkv_dtype == "fp16"
    assert p.parse_args(["--qkv_dtype", "mxfp8"]).qkv_dtype == "mxfp8"
    with pytest.raises(SystemExit):
        p.parse_args(["--qkv_dtype", "fp4"])
    a = p.parse_args([])                       # the reference's flags and defaults are untouched
    assert a.time_steps == 50 and a.seed == 33 and a.weight_dtype == torch.float16


def test_cli_flag_outranks_the_environment_switch(monkeypatch):
    """build_pipeline leaves a model alone that already has the flag's value and switches one that does not, whatever UNIVST_SD3_QKV made of it"""
    from univst_amd.src.sd3 import _common
    monkeypatch.setenv("UNIVST_SD3_QKV", "mxfp8")
    m = _tiny(2)
    assert m.qkv_dtype == "mxfp8"
    monkeypatch.setattr(_common, "load_sd3_vae", lambda *a: None)
    monkeypatch.setattr(_common, "load_transformer", lambda *a: m)
    monkeypatch.setattr(_common, "load_t5_encoder", lambda *a: torch.nn.Identity())
    import univst_amd.src.sd._common as sdc
    monkeypatch.setattr(sdc, "load_text_encoder", lambda *a, **k: torch.nn.Identity())
    monkeypatch.setattr(torch.nn.Module, "cuda", lambda self, *a, **k: self)
    import transformers
    for cls in ("CLIPTokenizer", "T5TokenizerFast"):
        monkeypatch.setattr(getattr(transformers, cls), "from_pretrained", classmethod(lambda c, *a, **k: None))
    monkeypatch.setattr(_common, "_flow_match_scheduler", lambda: types.SimpleNamespace(from_pretrained=lambda *a, **k: None))
    try:
        _common.build_pipeline("nowhere", torch.float16, qkv_dtype="fp16")
    except Exception:
        pass                                   # the pipeline object itself is not what this test is about: the switch is set before it is built
    assert m.qkv_dtype == "fp16" and all(a.qkv_dtype == "fp16" for a in m._attentions())
