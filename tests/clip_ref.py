"""The CLIP text tower restated as plain torch functions over a state dict: the yardstick of the native encoder (univst_amd/text.py, csrc/clip.hip).

``transformers.CLIPTextModel`` / ``CLIPTextModelWithProjection`` are third-party code; this file restates their forward pass from the published
definition (models/clip/modeling_clip.py: CLIPTextEmbeddings, CLIPEncoderLayer, CLIPAttention, CLIPMLP, CLIPTextTransformer) so that the arithmetic
can run in fp64 (the reference of the GPU tests), fp32 (parity with transformers, tests/test_clip_ref.py) or fp16 (what the reference pipeline's
``text_encoder.to(fp16).cuda()`` computes: the error yardstick of the GPU tests).

    x = token_embedding[ids] + position_embedding[0..S)
    per layer:  x += out_proj(softmax_causal((q_proj(ln1 x) * d^-0.5) k_proj(ln1 x)^T) v_proj(ln1 x));   x += fc2(act(fc1(ln2 x)))
    last_hidden_state = final_layer_norm(x);  pooled = last_hidden_state[b, eos position];  text_embeds = text_projection(pooled) (no bias)

State-dict keys are transformers': real checkpoints (and transformers 4.x) prefix every key of the tower with ``text_model.``, transformers 5.x drops the
prefix for CLIPTextModel; ``strip_prefix`` accepts both.  ``text_projection.weight`` is top level in both."""
import math
from dataclasses import dataclass

import torch
import torch.nn.functional as F


@dataclass
class Cfg:
    vocab_size: int = 49408
    hidden_size: int = 768
    intermediate_size: int = 3072
    num_layers: int = 12
    num_heads: int = 12
    max_positions: int = 77
    hidden_act: str = "quick_gelu"        # or "gelu" (exact, erf)
    layer_norm_eps: float = 1e-5
    projection_dim: int = 0               # 0: no text_projection (CLIPTextModel)
    eos_token_id: int = 2                 # 2: the legacy rule (argmax of the ids)


CLIP_L = Cfg()
OPENCLIP_H = Cfg(hidden_size=1024, intermediate_size=4096, num_layers=23, num_heads=16, hidden_act="gelu")
CLIP_BIGG = Cfg(hidden_size=1280, intermediate_size=5120, num_layers=32, num_heads=20, hidden_act="gelu", projection_dim=1280)


def cfg_from_hf(config, projected):
    """a transformers CLIPTextConfig -> Cfg"""
    return Cfg(vocab_size=config.vocab_size, hidden_size=config.hidden_size, intermediate_size=config.intermediate_size,
               num_layers=config.num_hidden_layers, num_heads=config.num_attention_heads, max_positions=config.max_position_embeddings,
               hidden_act=config.hidden_act, layer_norm_eps=config.layer_norm_eps, projection_dim=config.projection_dim if projected else 0,
               eos_token_id=config.eos_token_id)


def state_dict_shapes(cfg):
    """key (without the ``text_model.`` prefix) -> shape, in transformers' order"""
    C, I = cfg.hidden_size, cfg.intermediate_size
    s = {"embeddings.token_embedding.weight": (cfg.vocab_size, C), "embeddings.position_embedding.weight": (cfg.max_positions, C)}
    for l in range(cfg.num_layers):
        p = f"encoder.layers.{l}."
        for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
            s[p + f"self_attn.{n}.weight"] = (C, C)
            s[p + f"self_attn.{n}.bias"] = (C,)
        s[p + "layer_norm1.weight"] = s[p + "layer_norm1.bias"] = (C,)
        s[p + "mlp.fc1.weight"], s[p + "mlp.fc1.bias"] = (I, C), (I,)
        s[p + "mlp.fc2.weight"], s[p + "mlp.fc2.bias"] = (C, I), (C,)
        s[p + "layer_norm2.weight"] = s[p + "layer_norm2.bias"] = (C,)
    s["final_layer_norm.weight"] = s["final_layer_norm.bias"] = (C,)
    if cfg.projection_dim:
        s["text_projection.weight"] = (cfg.projection_dim, C)
    return s


def random_state_dict(cfg, seed=0, qk_gain=1.6, prefix=""):
    """Seeded fp32 weights with the tower's keys (``prefix`` = "text_model." gives the checkpoint form; text_projection.weight stays top level).

    transformers' default init (std 0.02 everywhere) gives pre-softmax scores of ~1e-3, i.e. uniform attention over the visible keys, which tests
    nothing.  Here the linears are N(0, 1/fan_in) (unit-variance outputs for unit-variance inputs) and the q / k projection weights carry the extra
    factor ``qk_gain``: q and k elements then have a standard deviation of about qk_gain and the scaled scores q.k / 8 over d = 64 one of about
    qk_gain^2.  Measured on the fp64 restatement with qk_gain = 1.6 and random ids (B = 3, S = 77; visible entries of every layer and head):
    score standard deviation 2.52 / 2.39 (layer 0 / 1) at hidden 128 / 2 heads, 2.62 / 2.61 at 768 / 12 heads
    (tests/test_clip_ref.py::test_random_weights_give_peaked_attention prints them and holds the 2 - 3.5 window)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in state_dict_shapes(cfg).items():
        if k.endswith("token_embedding.weight"):
            t = torch.randn(shape, generator=g) * 0.5
        elif k.endswith("position_embedding.weight"):
            t = torch.randn(shape, generator=g) * 0.3
        elif "layer_norm" in k and k.endswith(".weight"):
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        elif k.endswith(".bias"):
            t = 0.1 * torch.randn(shape, generator=g)
        else:
            t = torch.randn(shape, generator=g) / math.sqrt(shape[1])
            if ".q_proj." in k or ".k_proj." in k:
                t = t * qk_gain
        sd[k if k == "text_projection.weight" else prefix + k] = t
    return sd


def strip_prefix(sd):
    """one optional leading ``text_model.`` off every key"""
    return {(k[len("text_model."):] if k.startswith("text_model.") else k): v for k, v in sd.items()}


def eos_positions(ids, eos_token_id):
    """the row ``pooler_output`` takes: legacy configs (eos_token_id == 2) the position of the largest id; otherwise the first position that holds
    eos_token_id, 0 when none does"""
    if eos_token_id == 2:
        return ids.argmax(dim=-1)
    return (ids == eos_token_id).int().argmax(dim=-1)


def activation(x, name):
    if name == "quick_gelu":
        return x * torch.sigmoid(1.702 * x)
    if name == "gelu":
        return F.gelu(x)
    raise ValueError(f"hidden_act {name!r}: the CLIP text towers use quick_gelu or gelu")


def forward(sd, cfg, ids, dtype=torch.float64, scores_out=None):
    """ids int64 [B, S] -> dict(last_hidden_state [B,S,C], hidden_states (L + 1 residual streams before the final LN), pooler_output [B,C],
    text_embeds [B,P] or None).  Weights and activations are cast to ``dtype`` (fp16: every op rounds to fp16 as torch's fp16 modules do).
    scores_out: a list that receives every layer's scaled, unmasked scores [B, heads, S, S]."""
    sd = {k: v.to(device=ids.device, dtype=dtype) for k, v in strip_prefix(sd).items()}
    B, S = ids.shape
    C, Hn = cfg.hidden_size, cfg.num_heads
    d = C // Hn
    x = sd["embeddings.token_embedding.weight"][ids] + sd["embeddings.position_embedding.weight"][:S]
    future = torch.ones(S, S, dtype=torch.bool, device=ids.device).triu(1)
    hs = [x]
    for l in range(cfg.num_layers):
        p = f"encoder.layers.{l}."
        h = F.layer_norm(x, (C,), sd[p + "layer_norm1.weight"], sd[p + "layer_norm1.bias"], cfg.layer_norm_eps)
        lin = lambda n, t: F.linear(t, sd[p + n + ".weight"], sd[p + n + ".bias"])      # noqa: E731
        heads = lambda t: t.view(B, S, Hn, d).transpose(1, 2)                           # noqa: E731
        q, k, v = heads(lin("self_attn.q_proj", h) * d ** -0.5), heads(lin("self_attn.k_proj", h)), heads(lin("self_attn.v_proj", h))
        sc = q @ k.transpose(-1, -2)
        if scores_out is not None:
            scores_out.append(sc)
        a = torch.softmax(sc.masked_fill(future, float("-inf")), dim=-1) @ v
        x = x + lin("self_attn.out_proj", a.transpose(1, 2).reshape(B, S, C))
        h = F.layer_norm(x, (C,), sd[p + "layer_norm2.weight"], sd[p + "layer_norm2.bias"], cfg.layer_norm_eps)
        x = x + lin("mlp.fc2", activation(lin("mlp.fc1", h), cfg.hidden_act))
        hs.append(x)
    last = F.layer_norm(x, (C,), sd["final_layer_norm.weight"], sd["final_layer_norm.bias"], cfg.layer_norm_eps)
    pooled = last[torch.arange(B, device=ids.device), eos_positions(ids, cfg.eos_token_id)]
    emb = F.linear(pooled, sd["text_projection.weight"]) if cfg.projection_dim else None
    return dict(last_hidden_state=last, hidden_states=tuple(hs), pooler_output=pooled, text_embeds=emb)


def make_ids(cfg, B, S, seed=0, eos_at=None):
    """random ids below the EOS id's rivals: every id is in [0, vocab) and differs from eos_token_id / the maximum id except where ``eos_at[b]`` (a
    position, or None for a row without EOS) puts it.  For the legacy rule the EOS stand-in is the largest id, vocab - 1."""
    g = torch.Generator().manual_seed(seed)
    eos = cfg.vocab_size - 1 if cfg.eos_token_id == 2 else cfg.eos_token_id
    ids = torch.randint(0, cfg.vocab_size - 1, (B, S), generator=g)
    ids[ids == eos] = (eos + 1) % (cfg.vocab_size - 1)
    for b, p in enumerate(eos_at or []):
        if p is not None:
            ids[b, p] = eos
    return ids
