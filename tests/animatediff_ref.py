"""The AnimateDiff UNet3D (backbones/animatediff/models/unet.py as animatediff-v2.yaml configures it) and its PnP ``attn1`` forward
(backbones/animatediff/pnp_utils.py:18-109) restated as plain torch functions over a state dict, in any dtype: the yardstick of the native graph
(csrc/unet.hip behind ``univst_unet_create_animatediff``).  fp64 is the truth of the GPU tests, fp16 what the reference pipeline's
``unet.to(fp16).cuda()`` computes (their error yardstick), and tests/test_animatediff_ref.py holds the restatement to the reference's own classes
through golden g21 (tests/golden/make_golden_animatediff.py).

    conv_in per frame;  per level:  resnet -> [spatial transformer] -> [motion module];  skips as in the SD UNet;  conv_norm_out, SiLU, conv_out
    resnet:       GroupNorm per frame (use_inflated_groupnorm, resnet.py:21-29) or over all frames of a branch, SiLU, conv, + time embedding, ...
    transformer:  per frame: GroupNorm(eps 1e-6), proj_in, attn1 over the frame's OWN tokens (attention.py:344: no key frames), attn2 (text), GEGLU
                  feed-forward, proj_out, + input.  No attn_temp.
    PnP attn1:    inside eta1 * 50 <= idx < eta2 * 50 the q / k / v of branch 2 are shifted (alpha 0.8, gamma 2.0); outside it the closure is the
                  stock attention.
    motion:       tests/motion_ref.py, behind every resnet / transformer pair of the levels that have one, and between the mid block's transformer
                  and its second resnet.

Reused: tests/motion_ref.py (the module) and what oracle/unet_ref.py exports (time embedding, SDPA, text attention, GEGLU, AdaIN, per-frame conv,
upsampler)."""
import importlib.util
import math
import os
import sys
import zlib

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_ref as M  # noqa: E402

try:
    from oracle import unet_ref as U
except ImportError:      # (the golden generator keeps the repository root off sys.path so that the reference's `backbones` package wins)
    _spec = importlib.util.spec_from_file_location("_univst_oracle_unet_ref",
                                                   os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "unet_ref.py"))
    U = importlib.util.module_from_spec(_spec)
    _spec.loader.exec_module(U)

PNP_LAYERS = U.PNP_LAYERS
ALPHA, GAMMA = 0.8, 2.0


def make_cfg(block_out_channels=(320, 640, 1280, 1280), layers_per_block=2, cross_attention_dim=768, attention_head_dim=8, norm_num_groups=32,
             use_inflated_groupnorm=True, motion_levels=(True, True, True, True), motion_mid_block=True, motion_heads=8, motion_blocks=1, motion_attn=2,
             max_len=24, position_encoding=True):
    """attention_head_dim is the HEAD COUNT per level, as the reference's blocks use it (unet_blocks.py:343-344)"""
    return dict(in_channels=4, out_channels=4, block_out_channels=tuple(block_out_channels), layers_per_block=layers_per_block,
                cross_attention_dim=cross_attention_dim, attention_head_dim=attention_head_dim, norm_num_groups=norm_num_groups, norm_eps=1e-5,
                flip_sin_to_cos=True, freq_shift=0, use_inflated_groupnorm=bool(use_inflated_groupnorm), motion_levels=tuple(bool(v) for v in motion_levels),
                motion_mid_block=bool(motion_mid_block), motion_heads=motion_heads, motion_blocks=motion_blocks, motion_attn=motion_attn, max_len=max_len,
                position_encoding=bool(position_encoding))


# the golden's configuration (tests/golden/make_golden_animatediff.py): layers_per_block must be 2 (PnP indexes attentions[2]) and every width a
# multiple of 32 (the module's GroupNorm has 32 groups)
G21_CFG = make_cfg(block_out_channels=(32, 32, 64, 64), cross_attention_dim=16, attention_head_dim=2, norm_num_groups=8, motion_heads=2, max_len=24)


def reference_kwargs(cfg):
    """the reference constructor's arguments for ``cfg``"""
    res = tuple(2 ** i for i in range(4) if cfg["motion_levels"][i])
    return dict(in_channels=cfg["in_channels"], out_channels=cfg["out_channels"], block_out_channels=cfg["block_out_channels"],
                layers_per_block=cfg["layers_per_block"], cross_attention_dim=cfg["cross_attention_dim"], attention_head_dim=cfg["attention_head_dim"],
                norm_num_groups=cfg["norm_num_groups"], norm_eps=cfg["norm_eps"], use_inflated_groupnorm=cfg["use_inflated_groupnorm"],
                use_motion_module=bool(res) or cfg["motion_mid_block"], motion_module_resolutions=res, motion_module_mid_block=cfg["motion_mid_block"],
                motion_module_type="Vanilla",
                motion_module_kwargs=dict(num_attention_heads=cfg["motion_heads"], num_transformer_block=cfg["motion_blocks"],
                                          attention_block_types=("Temporal_Self",) * cfg["motion_attn"], temporal_position_encoding=cfg["position_encoding"],
                                          temporal_position_encoding_max_len=cfg["max_len"], temporal_attention_dim_div=1, zero_initialize=False),
                unet_use_cross_frame_attention=False, unet_use_temporal_attention=False)


def motion_cfg(cfg, channels):
    return M.Cfg(channels=channels, num_heads=cfg["motion_heads"], num_blocks=cfg["motion_blocks"], attn_per_block=cfg["motion_attn"], norm_groups=32,
                 max_len=cfg["max_len"], position_encoding=cfg["position_encoding"])


def motion_prefixes(cfg):
    """prefix -> width of every motion module, e.g. "down_blocks.0.motion_modules.1." """
    boc, L = cfg["block_out_channels"], cfg["layers_per_block"]
    out = {}
    for i in range(4):
        if cfg["motion_levels"][i]:
            for j in range(L):
                out[f"down_blocks.{i}.motion_modules.{j}."] = boc[i]
            for j in range(L + 1):
                out[f"up_blocks.{3 - i}.motion_modules.{j}."] = boc[i]
    if cfg["motion_mid_block"]:
        out["mid_block.motion_modules.0."] = boc[3]
    return out


def state_dict_shapes(cfg):
    """every key of the reference model's ``state_dict()`` for ``cfg`` with its shape, in the module tree's order"""
    boc, ted, D, L = cfg["block_out_channels"], cfg["block_out_channels"][0] * 4, cfg["cross_attention_dim"], cfg["layers_per_block"]
    s = {}

    def conv(p, ci, co, k):
        s[p + ".weight"], s[p + ".bias"] = (co, ci, k, k), (co,)

    def lin(p, ci, co, bias=True):
        s[p + ".weight"] = (co, ci)
        if bias:
            s[p + ".bias"] = (co,)

    def norm(p, c):
        s[p + ".weight"] = s[p + ".bias"] = (c,)

    def res(p, ci, co):
        norm(p + ".norm1", ci); conv(p + ".conv1", ci, co, 3); lin(p + ".time_emb_proj", ted, co); norm(p + ".norm2", co); conv(p + ".conv2", co, co, 3)
        if ci != co:
            conv(p + ".conv_shortcut", ci, co, 1)

    def attn(p, c, kv):
        lin(p + ".to_q", c, c, False); lin(p + ".to_k", kv, c, False); lin(p + ".to_v", kv, c, False); lin(p + ".to_out.0", c, c)

    def tr(p, c):
        norm(p + ".norm", c); conv(p + ".proj_in", c, c, 1)
        b = p + ".transformer_blocks.0"
        attn(b + ".attn1", c, c); norm(b + ".norm1", c); attn(b + ".attn2", c, D); norm(b + ".norm2", c)
        lin(b + ".ff.net.0.proj", c, 8 * c); lin(b + ".ff.net.2", 4 * c, c); norm(b + ".norm3", c)
        conv(p + ".proj_out", c, c, 1)

    def mm(p, c, on):
        if on:
            for k, shape in M.state_dict_shapes(motion_cfg(cfg, c)).items():
                s[p + "." + k] = shape

    conv("conv_in", cfg["in_channels"], boc[0], 3)
    lin("time_embedding.linear_1", boc[0], ted); lin("time_embedding.linear_2", ted, ted)
    out = boc[0]
    for i in range(4):
        inp, out = out, boc[i]
        p = f"down_blocks.{i}"
        if i < 3:
            for j in range(L):
                tr(f"{p}.attentions.{j}", out)
        for j in range(L):
            res(f"{p}.resnets.{j}", inp if j == 0 else out, out)
        for j in range(L):
            mm(f"{p}.motion_modules.{j}", out, cfg["motion_levels"][i])
        if i != 3:
            conv(f"{p}.downsamplers.0.conv", out, out, 3)
    rev = list(reversed(boc))
    out = rev[0]
    for i in range(4):
        prev, out = out, rev[i]
        inp = rev[min(i + 1, 3)]
        p = f"up_blocks.{i}"
        if i > 0:
            for j in range(L + 1):
                tr(f"{p}.attentions.{j}", out)
        for j in range(L + 1):
            res(f"{p}.resnets.{j}", (prev if j == 0 else out) + (inp if j == L else out), out)
        for j in range(L + 1):
            mm(f"{p}.motion_modules.{j}", out, cfg["motion_levels"][3 - i])
        if i != 3:
            conv(f"{p}.upsamplers.0.conv", out, out, 3)
    tr("mid_block.attentions.0", boc[3])
    res("mid_block.resnets.0", boc[3], boc[3]); res("mid_block.resnets.1", boc[3], boc[3])
    mm("mid_block.motion_modules.0", boc[3], cfg["motion_mid_block"])
    norm("conv_norm_out", boc[0])
    conv("conv_out", boc[0], cfg["out_channels"], 3)
    return s


def random_state_dict(cfg, seed=21, zero_motion=False, qk_gain=1.6):
    """Seeded fp32 weights under the reference's names; weights are never stored, every user draws them again.  Each tensor has its own generator
    seeded by (seed, crc32(name)), so any subset can be regenerated.  Matrices and convs are N(0, 1 / fan_in) (unit-variance outputs for
    unit-variance inputs), norm weights 1 + 0.1 N, norm biases 0.05 N, other biases 0.02 N; to_q / to_k of every attention carry ``qk_gain`` so that
    the softmaxes are peaked (uniform attention tests nothing).  The motion modules' proj_out is NOT zero unless ``zero_motion`` (the state of a
    UNet with no motion checkpoint loaded: zero_initialize)."""
    sd = {}
    for name, shape in state_dict_shapes(cfg).items():
        g = torch.Generator(device="cpu").manual_seed((seed * 1000003 + zlib.crc32(name.encode())) % (2 ** 31))
        is_norm = len(shape) == 1 and (".norm" in name or "_norm" in name) and not name.endswith("to_out.0.bias")
        if zero_motion and ".motion_modules." in name and ".proj_out." in name:
            t = torch.zeros(shape)
        elif is_norm:
            t = 1.0 + 0.1 * torch.randn(shape, generator=g) if name.endswith("weight") else 0.05 * torch.randn(shape, generator=g)
        elif name.endswith(".bias"):
            t = 0.02 * torch.randn(shape, generator=g)
        else:
            t = torch.randn(shape, generator=g) / math.sqrt(math.prod(shape[1:]))
            if ".to_q." in name or ".to_k." in name:
                t = t * qk_gain
        sd[name] = t
    return sd


def in_window(idx, eta1, eta2):
    """pnp_utils.py:45 of this backbone: exclusive at the top, eta1 scaled"""
    return idx >= eta1 * 50 and idx < eta2 * 50


def attn1_forward(sd, p, x, heads, pnp):
    """x [(b f), N, C]: diffusers' Attention on the frame's own tokens (pnp None: attention.py:344), or the PnP closure (pnp_utils.py:20-98 with
    clip_length None) with pnp = dict(idx, eta1, eta2[, alpha, gamma])"""
    q, k, v = (U._lin(sd, p + n, x, bias=False) for n in (".to_q", ".to_k", ".to_v"))
    if pnp is not None and in_window(pnp["idx"], pnp.get("eta1", 0.0), pnp.get("eta2", 0.5)):
        c = q.shape[0] // 3
        alpha, gamma = pnp.get("alpha", ALPHA), pnp.get("gamma", GAMMA)
        beta = U.pnp_beta(pnp["idx"], pnp.get("eta1", 0.0), pnp.get("eta2", 0.5))
        q, k, v = q.clone(), k.clone(), v.clone()
        q[2 * c:] = alpha * q[:c] + (1 - alpha) * q[2 * c:]
        k[2 * c:] = beta * U.attention_adain(k[2 * c:], k[c:2 * c]) + (1 - beta) * k[c:2 * c]
        v[2 * c:] = beta * U.attention_adain(v[2 * c:], v[c:2 * c]) + (1 - beta) * v[c:2 * c]
        q[2 * c:] = gamma * q[2 * c:]
    return U._lin(sd, p + ".to_out.0", U.sdpa(q, k, v, heads))


def group_norm(sd, p, x, groups, eps, per_frame):
    """x [b, c, f, h, w]: InflatedGroupNorm (per frame) or nn.GroupNorm on the 5-D tensor (over all frames)"""
    if not per_frame:
        return F.group_norm(x, groups, sd[p + ".weight"], sd[p + ".bias"], eps)
    b, c, f, h, w = x.shape
    y = F.group_norm(x.permute(0, 2, 1, 3, 4).reshape(b * f, c, h, w), groups, sd[p + ".weight"], sd[p + ".bias"], eps)
    return y.view(b, f, c, h, w).permute(0, 2, 1, 3, 4)


def resnet_block(sd, p, x, temb, cfg):
    """resnet.py:182-212"""
    g, eps, pf = cfg["norm_num_groups"], cfg["norm_eps"], cfg["use_inflated_groupnorm"]
    h = U.pseudo_conv3d(sd, p + ".conv1", F.silu(group_norm(sd, p + ".norm1", x, g, eps, pf)))
    h = h + U._lin(sd, p + ".time_emb_proj", F.silu(temb))[:, :, None, None, None]
    h = U.pseudo_conv3d(sd, p + ".conv2", F.silu(group_norm(sd, p + ".norm2", h, g, eps, pf)))
    if (p + ".conv_shortcut.weight") in sd:
        x = U.pseudo_conv3d(sd, p + ".conv_shortcut", x, padding=0)
    return x + h


def transformer_model(sd, p, x, ctx, heads, groups, pnp):
    """attention.py:165-212 + :327-371.  x [b, c, f, h, w], ctx [b, T, D]"""
    b, c, f, h, w = x.shape
    y = x.permute(0, 2, 1, 3, 4).reshape(b * f, c, h, w)
    res = y
    y = F.conv2d(F.group_norm(y, groups, sd[p + ".norm.weight"], sd[p + ".norm.bias"], 1e-6), sd[p + ".proj_in.weight"], sd[p + ".proj_in.bias"])
    y = y.permute(0, 2, 3, 1).reshape(b * f, h * w, c)
    t = p + ".transformer_blocks.0"
    ln = lambda n, u: F.layer_norm(u, (c,), sd[t + f".{n}.weight"], sd[t + f".{n}.bias"], 1e-5)      # noqa: E731
    y = attn1_forward(sd, t + ".attn1", ln("norm1", y), heads, pnp) + y
    y = U.plain_attention(sd, t + ".attn2", ln("norm2", y), ctx.repeat_interleave(f, 0), heads) + y
    y = U.feed_forward_geglu(sd, t + ".ff", ln("norm3", y)) + y
    y = F.conv2d(y.view(b * f, h, w, c).permute(0, 3, 1, 2), sd[p + ".proj_out.weight"], sd[p + ".proj_out.bias"]) + res
    return y.view(b, f, c, h, w).permute(0, 2, 1, 3, 4).contiguous()


def unet_forward(sd, cfg, sample, timestep, encoder_hidden_states, pnp=None, dtype=torch.float64):
    """unet.py:323-466.  sample [B, 4, F, H, W], encoder_hidden_states [B, T, D] -> eps of sample's shape, in ``dtype`` on sample's device.
    ``pnp``: None (attn1 not registered) or dict(idx, eta1, eta2[, alpha, gamma]) for the 8 decoder layers."""
    sd = {k: v.to(device=sample.device, dtype=dtype) for k, v in sd.items()}
    x, ctx = sample.to(dtype), encoder_hidden_states.to(device=sample.device, dtype=dtype)
    boc, L, groups = cfg["block_out_channels"], cfg["layers_per_block"], cfg["norm_num_groups"]
    hd = cfg["attention_head_dim"]
    hl = (hd,) * 4 if isinstance(hd, int) else tuple(hd)
    B = x.shape[0]
    t = torch.as_tensor(timestep, device=x.device).reshape(-1).expand(B)
    emb = U.timestep_sinusoid(t, boc[0], cfg["flip_sin_to_cos"], cfg["freq_shift"]).to(dtype)
    emb = U._lin(sd, "time_embedding.linear_2", F.silu(U._lin(sd, "time_embedding.linear_1", emb)))
    mods = motion_prefixes(cfg)

    def motion(p, u):
        if p not in mods:
            return u
        sub = {k[len(p):]: v for k, v in sd.items() if k.startswith(p)}
        return M.forward(sub, motion_cfg(cfg, mods[p]), u, dtype=dtype)

    x = U.pseudo_conv3d(sd, "conv_in", x)
    skips = [x]
    for i in range(4):
        p = f"down_blocks.{i}"
        for j in range(L):
            x = resnet_block(sd, f"{p}.resnets.{j}", x, emb, cfg)
            if i < 3:
                x = transformer_model(sd, f"{p}.attentions.{j}", x, ctx, hl[i], groups, None)
            x = motion(f"{p}.motion_modules.{j}.", x)
            skips.append(x)
        if i != 3:
            x = U.pseudo_conv3d(sd, f"{p}.downsamplers.0.conv", x, stride=2)
            skips.append(x)
    x = resnet_block(sd, "mid_block.resnets.0", x, emb, cfg)
    x = transformer_model(sd, "mid_block.attentions.0", x, ctx, hl[3], groups, None)
    x = motion("mid_block.motion_modules.0.", x)
    x = resnet_block(sd, "mid_block.resnets.1", x, emb, cfg)
    for i in range(4):
        p = f"up_blocks.{i}"
        for j in range(L + 1):
            x = resnet_block(sd, f"{p}.resnets.{j}", torch.cat([x, skips.pop()], dim=1), emb, cfg)
            if i > 0:
                x = transformer_model(sd, f"{p}.attentions.{j}", x, ctx, hl[3 - i], groups, pnp if (pnp is not None and j in PNP_LAYERS.get(i, [])) else None)
            x = motion(f"{p}.motion_modules.{j}.", x)
        if i != 3:
            x = U.upsample(sd, f"{p}.upsamplers.0", x)
    x = F.silu(group_norm(sd, "conv_norm_out", x, groups, cfg["norm_eps"], cfg["use_inflated_groupnorm"]))
    return U.pseudo_conv3d(sd, "conv_out", x)
