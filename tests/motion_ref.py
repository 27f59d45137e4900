"""The AnimateDiff motion module restated as plain torch functions over a state dict: the yardstick of the native module (univst_amd/motion.py,
csrc/motion.hip).

``VanillaTemporalModule`` (backbones/animatediff/models/motion_module.py) wraps ``TemporalTransformer3DModel``; its ``VersatileAttention`` derives from
diffusers' ``Attention`` and calls ``head_to_batch_dim`` / ``get_attention_scores`` / ``batch_to_head_dim``, its feed-forward is diffusers'
``FeedForward(geglu)``.  This file restates the forward pass so that the arithmetic can run in fp64 (the reference of the GPU tests), fp32 (parity with
the reference module, tests/test_motion_ref.py against golden g20) or fp16 (what the reference pipeline's ``unet.to(fp16).cuda()`` computes: the error
yardstick of the GPU tests).

    per frame:  h = proj_in(GroupNorm(32, C, eps 1e-6)(x)) over rows = pixels
    per block:  per attention i:  h = attn_i(LayerNorm_i(h)) + h;   then  h = ff2(geglu(ff1(LayerNorm_ff(h)))) + h
    attn:       rows regrouped (b f) n c -> (b n) f c;  t = t + pe[:F];  softmax(d^-0.5 to_q(t) to_k(t)^T) to_v(t) per head over the F frames;
                to_out[0] (bias);  regrouped back
    y = proj_out(h) + x

Keys are the module's state-dict names ("temporal_transformer.proj_in.weight", ...).  The position table is a non-persistent buffer of the reference
(absent from its state dict) and is computed from the formula unless the state dict carries ``...attention_blocks.i.pos_encoder.pe`` [1, max_len, C],
as published AnimateDiff checkpoints do."""
import math
from dataclasses import dataclass

import torch
import torch.nn.functional as F


@dataclass
class Cfg:
    channels: int = 320
    num_heads: int = 8
    num_blocks: int = 1                    # num_transformer_block
    attn_per_block: int = 2                # len(attention_block_types), all "Temporal_Self"
    norm_groups: int = 32
    max_len: int = 24                      # temporal_position_encoding_max_len
    position_encoding: bool = True
    gn_eps: float = 1e-6
    ln_eps: float = 1e-5


def state_dict_shapes(cfg):
    """key -> shape, in the module's registration order"""
    C = cfg.channels
    t = "temporal_transformer."
    s = {t + "norm.weight": (C,), t + "norm.bias": (C,), t + "proj_in.weight": (C, C), t + "proj_in.bias": (C,)}
    for b in range(cfg.num_blocks):
        p = t + f"transformer_blocks.{b}."
        for i in range(cfg.attn_per_block):
            a = p + f"attention_blocks.{i}."
            s[a + "to_q.weight"] = s[a + "to_k.weight"] = s[a + "to_v.weight"] = s[a + "to_out.0.weight"] = (C, C)
            s[a + "to_out.0.bias"] = (C,)
        for i in range(cfg.attn_per_block):
            s[p + f"norms.{i}.weight"] = s[p + f"norms.{i}.bias"] = (C,)
        s[p + "ff.net.0.proj.weight"], s[p + "ff.net.0.proj.bias"] = (8 * C, C), (8 * C,)
        s[p + "ff.net.2.weight"], s[p + "ff.net.2.bias"] = (C, 4 * C), (C,)
        s[p + "ff_norm.weight"] = s[p + "ff_norm.bias"] = (C,)
    s[t + "proj_out.weight"], s[t + "proj_out.bias"] = (C, C), (C,)
    return s


def random_state_dict(cfg, seed=0, qk_gain=1.6):
    """Seeded fp32 weights with the module's keys.  Linears are N(0, 1/fan_in) (unit-variance outputs for unit-variance inputs); to_q / to_k carry the
    extra factor ``qk_gain`` so that the scaled scores have a standard deviation of about qk_gain^2 (peaked attention: uniform attention tests
    nothing); proj_out is NOT zero (a zero proj_out returns the input and pins nothing)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in state_dict_shapes(cfg).items():
        if ("norm" in k) and k.endswith(".weight"):
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        elif k.endswith(".bias"):
            t = 0.1 * torch.randn(shape, generator=g)
        else:
            t = torch.randn(shape, generator=g) / math.sqrt(shape[1])
            if ".to_q." in k or ".to_k." in k:
                t = t * qk_gain
        sd[k] = t
    return sd


def position_table(max_len, C):
    """PositionalEncoding's buffer [1, max_len, C] in fp32: pe[f, 2i] + 1j pe[f, 2i + 1] = exp(1j f w_i) with w_i = exp(-2i ln(10000) / C), every step
    in fp32 (within one fp32 unit of the reference's buffer: golden g20 is reproduced through this table, tests/test_motion_ref.py)"""
    w = torch.exp(torch.arange(0, C, 2, dtype=torch.float32) * (-math.log(10000.0) / C))
    angle = torch.arange(max_len, dtype=torch.float32).unsqueeze(1) * w
    return torch.view_as_real(torch.polar(torch.ones_like(angle), angle)).flip(-1).reshape(1, max_len, C)


def attention(sd, a, t, heads, pe):
    """t [(b n), F, C] -> the same shape: diffusers' Attention pieces the reference calls (head_to_batch_dim, get_attention_scores = softmax of
    baddbmm(beta 0, alpha scale), bmm, batch_to_head_dim) and to_out[0]"""
    Bn, Fr, C = t.shape
    d = C // heads
    if pe is not None:
        t = t + pe[:, :Fr]
    split = lambda u: u.reshape(Bn, Fr, heads, d).permute(0, 2, 1, 3).reshape(Bn * heads, Fr, d)      # noqa: E731
    q, k, v = split(F.linear(t, sd[a + "to_q.weight"])), split(F.linear(t, sd[a + "to_k.weight"])), split(F.linear(t, sd[a + "to_v.weight"]))
    sc = torch.baddbmm(torch.empty(Bn * heads, Fr, Fr, dtype=q.dtype, device=q.device), q, k.transpose(-1, -2), beta=0, alpha=d ** -0.5)
    o = torch.bmm(sc.softmax(dim=-1).to(v.dtype), v)
    o = o.reshape(Bn, heads, Fr, d).permute(0, 2, 1, 3).reshape(Bn, Fr, C)
    return F.linear(o, sd[a + "to_out.0.weight"], sd[a + "to_out.0.bias"])


def forward(sd, cfg, x, dtype=torch.float64):
    """x [B, C, F, H, W] -> the same shape.  Weights and activations are cast to ``dtype`` (fp16: every op rounds to fp16 as torch's fp16 modules do)."""
    sd = {k: v.to(device=x.device, dtype=dtype) for k, v in sd.items()}
    x = x.to(dtype)
    B, C, Fr, H, W = x.shape
    N = H * W
    t = "temporal_transformer."
    xf = x.permute(0, 2, 1, 3, 4).reshape(B * Fr, C, H, W)
    h = F.group_norm(xf, cfg.norm_groups, sd[t + "norm.weight"], sd[t + "norm.bias"], cfg.gn_eps)
    h = h.permute(0, 2, 3, 1).reshape(B * Fr, N, C)
    h = F.linear(h, sd[t + "proj_in.weight"], sd[t + "proj_in.bias"])
    for b in range(cfg.num_blocks):
        p = t + f"transformer_blocks.{b}."
        for i in range(cfg.attn_per_block):
            a = p + f"attention_blocks.{i}."
            pe = None
            if cfg.position_encoding:
                pe = sd[a + "pos_encoder.pe"] if a + "pos_encoder.pe" in sd else position_table(cfg.max_len, C).to(device=x.device, dtype=dtype)
            n = F.layer_norm(h, (C,), sd[p + f"norms.{i}.weight"], sd[p + f"norms.{i}.bias"], cfg.ln_eps)
            n = n.reshape(B, Fr, N, C).permute(0, 2, 1, 3).reshape(B * N, Fr, C)
            o = attention(sd, a, n, cfg.num_heads, pe)
            h = o.reshape(B, N, Fr, C).permute(0, 2, 1, 3).reshape(B * Fr, N, C) + h
        n = F.layer_norm(h, (C,), sd[p + "ff_norm.weight"], sd[p + "ff_norm.bias"], cfg.ln_eps)
        val, gate = F.linear(n, sd[p + "ff.net.0.proj.weight"], sd[p + "ff.net.0.proj.bias"]).chunk(2, dim=-1)
        h = F.linear(val * F.gelu(gate), sd[p + "ff.net.2.weight"], sd[p + "ff.net.2.bias"]) + h
    h = F.linear(h, sd[t + "proj_out.weight"], sd[t + "proj_out.bias"])
    y = h.reshape(B * Fr, H, W, C).permute(0, 3, 1, 2) + xf
    return y.reshape(B, Fr, C, H, W).permute(0, 2, 1, 3, 4).contiguous()
