"""The T5 encoder stack restated as plain torch functions over a state dict: the yardstick of the native encoder (univst_amd/text.py NativeT5Encoder,
csrc/t5.hip).

``transformers.T5EncoderModel`` is third-party code; this file restates its forward pass from the published definition (models/t5/modeling_t5.py:
T5LayerNorm, T5Attention with its relative-position bias, T5DenseGatedActDense, T5Block, T5Stack as an encoder) so that the arithmetic can run in
fp64 (the reference of the GPU tests), fp32 (parity with transformers, tests/test_t5_ref.py), fp16 (what the reference pipeline's
``text_encoder_3.to(fp16).cuda()`` computes: the error yardstick of the GPU tests) or fp16 with an fp32 residual stream (``residual_dtype``).

    x = embed[ids]
    per layer:  x += o(softmax(q(h) k(h)^T + bias[head][bucket(j - i)]) v(h)),  h = rms(x) * g1        (no 1/sqrt(d) scaling)
                x += wo(gelu_new(wi_0(h)) * wi_1(h)),                            h = rms(x) * g2
    last_hidden_state = rms(x) * g_final            rms(x) = x * rsqrt(mean(x^2) + eps): no mean subtraction, no bias anywhere

Only the v1.1 form (``feed_forward_proj = "gated-gelu"``) is restated.  transformers' fp16 path clamps a block's output when it holds an inf; the
restatement does not (the clamp never fires below the fp16 range, and beyond it the all-fp16 result is not meaningful either way).  State-dict
keys are transformers'; the tied embedding may be ``shared.weight`` or ``encoder.embed_tokens.weight``."""
import math
from dataclasses import dataclass

import torch
import torch.nn.functional as F


@dataclass
class Cfg:
    vocab_size: int = 32128
    d_model: int = 4096
    d_ff: int = 10240
    num_layers: int = 24
    num_heads: int = 64
    d_kv: int = 64
    num_buckets: int = 32
    max_distance: int = 128
    layer_norm_eps: float = 1e-6


T5_XXL = Cfg()
_REL = "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"


def hf_config(cfg):
    """Cfg -> the fields of transformers' T5Config that the encoder reads"""
    return dict(vocab_size=cfg.vocab_size, d_model=cfg.d_model, d_ff=cfg.d_ff, num_layers=cfg.num_layers, num_heads=cfg.num_heads, d_kv=cfg.d_kv,
                relative_attention_num_buckets=cfg.num_buckets, relative_attention_max_distance=cfg.max_distance, layer_norm_epsilon=cfg.layer_norm_eps,
                feed_forward_proj="gated-gelu")


def state_dict_shapes(cfg, embed_key="shared.weight"):
    C, I, Fd = cfg.d_model, cfg.num_heads * cfg.d_kv, cfg.d_ff
    s = {embed_key: (cfg.vocab_size, C)}
    for l in range(cfg.num_layers):
        p = f"encoder.block.{l}.layer."
        s[p + "0.SelfAttention.q.weight"] = s[p + "0.SelfAttention.k.weight"] = s[p + "0.SelfAttention.v.weight"] = (I, C)
        s[p + "0.SelfAttention.o.weight"] = (C, I)
        if l == 0:
            s[_REL] = (cfg.num_buckets, cfg.num_heads)
        s[p + "0.layer_norm.weight"] = (C,)
        s[p + "1.DenseReluDense.wi_0.weight"] = s[p + "1.DenseReluDense.wi_1.weight"] = (Fd, C)
        s[p + "1.DenseReluDense.wo.weight"] = (C, Fd)
        s[p + "1.layer_norm.weight"] = (C,)
    s["encoder.final_layer_norm.weight"] = (C,)
    return s


def random_state_dict(cfg, seed=0, qk_gain=0.56, embed_scale=1.0, bias_std=1.0, embed_key="shared.weight", out_gain=1.0, embed_clamp=None):
    """Seeded fp32 weights with the encoder's keys.  The linears are N(0, 1/fan_in) (unit-variance outputs for the unit-variance rows RMSNorm gives)
    and the q / k weights carry ``qk_gain``: T5 applies no 1/sqrt(d) scaling, so the scores q.k over d = 64 have a standard deviation of about
    8 qk_gain^2 = 2.5, to which the relative-position bias (std ``bias_std``) is added: peaked, not uniform, attention.  ``embed_scale`` is the
    standard deviation of the embedding table (``embed_clamp`` bounds its entries, e.g. to what an fp16 table can hold) and ``out_gain`` scales the
    two output projections o and wo, i.e. what every sub-layer adds to the residual stream: together they set the size of the stream."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in state_dict_shapes(cfg, embed_key).items():
        if k == embed_key:
            t = torch.randn(shape, generator=g) * embed_scale
            if embed_clamp is not None:
                t = t.clamp(-embed_clamp, embed_clamp)
        elif k == _REL:
            t = torch.randn(shape, generator=g) * bias_std
        elif k.endswith("layer_norm.weight"):
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:
            t = torch.randn(shape, generator=g) / math.sqrt(shape[1])
            if ".q.weight" in k or ".k.weight" in k:
                t = t * qk_gain
            if ".o.weight" in k or ".wo.weight" in k:
                t = t * out_gain
        sd[k] = t
    return sd


def make_ids(cfg, B, S, seed=0):
    return torch.randint(0, cfg.vocab_size, (B, S), generator=torch.Generator().manual_seed(seed))


def relative_position_bucket(rel, num_buckets=32, max_distance=128):
    """T5Attention._relative_position_bucket, bidirectional: rel = memory position - query position (int64 tensor)"""
    num_buckets //= 2
    ret = (rel > 0).to(torch.long) * num_buckets
    n = rel.abs()
    max_exact = num_buckets // 2
    large = max_exact + (torch.log(n.float() / max_exact) / math.log(max_distance / max_exact) * (num_buckets - max_exact)).to(torch.long)
    large = torch.min(large, torch.full_like(large, num_buckets - 1))
    return ret + torch.where(n < max_exact, n, large)


def position_bias(sd, cfg, S, device):
    """[heads, S, S]: relative_attention_bias[bucket(j - i)] for query i and key j"""
    pos = torch.arange(S, device=device)
    bucket = relative_position_bucket(pos[None, :] - pos[:, None], cfg.num_buckets, cfg.max_distance)
    return sd[_REL][bucket].permute(2, 0, 1)


def gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * torch.pow(x, 3.0))))


def rms_norm(x, w, eps):
    """T5LayerNorm: the variance in fp32 (or wider), the normalised row cast to the weight's dtype, then the product"""
    xf = x.float() if x.dtype in (torch.float16, torch.bfloat16) else x
    return w * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)).to(w.dtype)


def forward(sd, cfg, ids, dtype=torch.float64, residual_dtype=None, scores_out=None, stream_out=None):
    """ids int64 [B, S] -> last_hidden_state [B, S, d_model] in ``dtype``.  Weights and sub-layer arithmetic are cast to ``dtype`` (fp16: every op
    rounds to fp16 as torch's fp16 modules do; the softmax runs in fp32 as T5Attention's does); the residual stream x is kept in
    ``residual_dtype`` (default: ``dtype``).  scores_out: a list that receives every layer's biased scores [B, heads, S, S]; stream_out: one that
    receives the residual stream after the embedding and after every layer."""
    rdt = residual_dtype or dtype
    sd = {k: v.to(device=ids.device, dtype=dtype) for k, v in sd.items()}
    embed = sd["shared.weight"] if "shared.weight" in sd else sd["encoder.embed_tokens.weight"]
    B, S = ids.shape
    Hn, d = cfg.num_heads, cfg.d_kv
    x = embed[ids].to(rdt)
    bias = position_bias(sd, cfg, S, ids.device)
    if stream_out is not None:
        stream_out.append(x)
    for l in range(cfg.num_layers):
        p = f"encoder.block.{l}.layer."
        h = rms_norm(x, sd[p + "0.layer_norm.weight"], cfg.layer_norm_eps)
        heads = lambda t: t.view(B, S, Hn, d).transpose(1, 2)                           # noqa: E731
        q, k, v = (heads(F.linear(h, sd[p + f"0.SelfAttention.{n}.weight"])) for n in "qkv")
        sc = q @ k.transpose(-1, -2) + bias
        if scores_out is not None:
            scores_out.append(sc)
        pr = torch.softmax(sc.float() if dtype == torch.float16 else sc, dim=-1).to(dtype)
        a = (pr @ v).transpose(1, 2).reshape(B, S, Hn * d)
        x = x + F.linear(a, sd[p + "0.SelfAttention.o.weight"]).to(rdt)
        h = rms_norm(x, sd[p + "1.layer_norm.weight"], cfg.layer_norm_eps)
        ff = gelu_new(F.linear(h, sd[p + "1.DenseReluDense.wi_0.weight"])) * F.linear(h, sd[p + "1.DenseReluDense.wi_1.weight"])
        x = x + F.linear(ff, sd[p + "1.DenseReluDense.wo.weight"]).to(rdt)
        if stream_out is not None:
            stream_out.append(x)
    return rms_norm(x, sd["encoder.final_layer_norm.weight"], cfg.layer_norm_eps)
