"""TEST INFRASTRUCTURE: fp32 restatement of diffusers' plain ``AutoencoderKL`` — the SD3 / SD3.5 16-channel VAE, SD-v1.5's image VAE — as plain torch
functions over a state dict with that class's parameter names.

PARITY UNPINNED.  The class is third-party code that is absent here.  This file restates its PUBLISHED definition (diffusers 0.35:
``models/autoencoders/autoencoder_kl.py`` AutoencoderKL, ``models/autoencoders/vae.py`` Encoder / Decoder, ``models/unets/unet_2d_blocks.py``
DownEncoderBlock2D / UpDecoderBlock2D / UNetMidBlock2D, ``models/resnet.py`` ResnetBlock2D, ``models/upsampling.py`` Upsample2D,
``models/downsampling.py`` Downsample2D, ``models/attention_processor.py`` Attention + AttnProcessor2_0).  tests/test_klvae_ref.py holds it to the
project's independent restatement of the temporal VAE (oracle/vae_ref.py) on the layers the two networks share; tests/test_gpu_klvae.py holds the
native graph (csrc/vae.hip, univst_klvae_*) to it, and to the third-party class itself where diffusers can be imported.

All GroupNorm eps are 1e-6; the mid block is resnet, one-head attention (head_dim = C), resnet whatever ``layers_per_block`` is.
"""
import torch
import torch.nn.functional as F

SD3_VAE_CONFIG = dict(in_channels=3, out_channels=3, latent_channels=16, block_out_channels=(128, 256, 512, 512), layers_per_block=2,
                      norm_num_groups=32, scaling_factor=1.5305, shift_factor=0.0609, use_quant_conv=False, use_post_quant_conv=False)

# fp32 convolutions as im2col + matmul (torch's fp32 convolution is slow on this ROCm build; same products and sums, another summation order).
# Images are processed one after another in row bands so that the unfolded operand stays below ~2 GB.
CONV_VIA_MATMUL = False


def _conv2d(x, w, b=None, padding=0, stride=1):
    if not CONV_VIA_MATMUL:
        return F.conv2d(x, w, b, padding=padding, stride=stride)
    n, cin, H, W = x.shape
    cout, _, kh, kw = w.shape
    Ho, Wo = (H + 2 * padding - kh) // stride + 1, (W + 2 * padding - kw) // stride + 1
    wm = w.reshape(cout, cin * kh * kw)
    xp = F.pad(x, (padding, padding, padding, padding))
    band = max(1, int(2e9 // (cin * kh * kw * Wo * 4)))          # output rows per unfold
    out = torch.empty(n, cout, Ho, Wo, device=x.device, dtype=x.dtype)
    for i in range(n):
        for r0 in range(0, Ho, band):
            r1 = min(Ho, r0 + band)
            rows = xp[i:i + 1, :, r0 * stride:(r1 - 1) * stride + kh]
            y = torch.matmul(wm, F.unfold(rows, (kh, kw), stride=stride)[0])          # [cout, (r1 - r0) * Wo]
            if b is not None:
                y = y + b[:, None]
            out[i, :, r0:r1] = y.view(cout, r1 - r0, Wo)
    return out


def _gn(x, sd, p, groups):
    return F.group_norm(x, groups, sd[p + ".weight"], sd[p + ".bias"], 1e-6)


def resnet2d(sd, p, x, groups):
    """ResnetBlock2D(temb_channels=None, eps=1e-6, output_scale_factor=1): norm1 -> silu -> conv1 -> norm2 -> silu -> conv2, + (1x1 conv of) x"""
    h = _conv2d(F.silu(_gn(x, sd, p + ".norm1", groups)), sd[p + ".conv1.weight"], sd[p + ".conv1.bias"], padding=1)
    h = _conv2d(F.silu(_gn(h, sd, p + ".norm2", groups)), sd[p + ".conv2.weight"], sd[p + ".conv2.bias"], padding=1)
    if p + ".conv_shortcut.weight" in sd:
        x = _conv2d(x, sd[p + ".conv_shortcut.weight"], sd[p + ".conv_shortcut.bias"])
    return x + h


def attention(sd, p, x, groups):
    """Attention(heads=1, dim_head=C, norm_num_groups, eps=1e-6, bias=True, residual_connection=True): GroupNorm over the flattened tokens,
    softmax(q k^T / sqrt(C)) v, to_out, + x; image by image"""
    B, C, H, W = x.shape
    h = F.group_norm(x.reshape(B, C, H * W), groups, sd[p + ".group_norm.weight"], sd[p + ".group_norm.bias"], 1e-6).transpose(1, 2)
    q = F.linear(h, sd[p + ".to_q.weight"], sd[p + ".to_q.bias"])
    k = F.linear(h, sd[p + ".to_k.weight"], sd[p + ".to_k.bias"])
    v = F.linear(h, sd[p + ".to_v.weight"], sd[p + ".to_v.bias"])
    o = torch.empty_like(q)
    step = max(1, int(1e9 // (H * W * 4)))            # query rows per softmax: the fp32 score block stays below ~1 GB
    for i in range(B):
        for r0 in range(0, H * W, step):
            s = torch.matmul(q[i, r0:r0 + step], k[i].t()) * (C ** -0.5)
            o[i, r0:r0 + step] = torch.matmul(torch.softmax(s, dim=-1), v[i])
    o = F.linear(o, sd[p + ".to_out.0.weight"], sd[p + ".to_out.0.bias"])
    return o.transpose(1, 2).reshape(B, C, H, W) + x


def mid_block(sd, p, x, groups):
    x = resnet2d(sd, p + ".resnets.0", x, groups)
    x = attention(sd, p + ".attentions.0", x, groups)
    return resnet2d(sd, p + ".resnets.1", x, groups)


def decode(sd, z, cfg=SD3_VAE_CONFIG):
    """AutoencoderKL.decode(z).sample: z [N, latent, h, w] -> [N, out_channels, 8h, 8w]"""
    g, boc, L = cfg["norm_num_groups"], cfg["block_out_channels"], cfg["layers_per_block"]
    if cfg.get("use_post_quant_conv", False):
        z = _conv2d(z, sd["post_quant_conv.weight"], sd["post_quant_conv.bias"])
    x = _conv2d(z, sd["decoder.conv_in.weight"], sd["decoder.conv_in.bias"], padding=1)
    x = mid_block(sd, "decoder.mid_block", x, g)
    for b in range(4):
        for l in range(L + 1):
            x = resnet2d(sd, f"decoder.up_blocks.{b}.resnets.{l}", x, g)
        if b < 3:
            x = F.interpolate(x, scale_factor=2.0, mode="nearest")
            x = _conv2d(x, sd[f"decoder.up_blocks.{b}.upsamplers.0.conv.weight"], sd[f"decoder.up_blocks.{b}.upsamplers.0.conv.bias"], padding=1)
    x = F.silu(_gn(x, sd, "decoder.conv_norm_out", g))
    return _conv2d(x, sd["decoder.conv_out.weight"], sd["decoder.conv_out.bias"], padding=1)


def encode_moments(sd, x, cfg=SD3_VAE_CONFIG):
    """AutoencoderKL.encode(x).latent_dist.parameters: x [N, in_channels, H, W] -> [N, 2*latent, H/8, W/8] (mean | logvar)"""
    g, L = cfg["norm_num_groups"], cfg["layers_per_block"]
    x = _conv2d(x, sd["encoder.conv_in.weight"], sd["encoder.conv_in.bias"], padding=1)
    for b in range(4):
        for l in range(L):
            x = resnet2d(sd, f"encoder.down_blocks.{b}.resnets.{l}", x, g)
        if b < 3:       # Downsample2D(padding=0): pad right / bottom by one, stride-2 conv without padding
            x = _conv2d(F.pad(x, (0, 1, 0, 1)), sd[f"encoder.down_blocks.{b}.downsamplers.0.conv.weight"], sd[f"encoder.down_blocks.{b}.downsamplers.0.conv.bias"], stride=2)
    x = mid_block(sd, "encoder.mid_block", x, g)
    x = F.silu(_gn(x, sd, "encoder.conv_norm_out", g))
    x = _conv2d(x, sd["encoder.conv_out.weight"], sd["encoder.conv_out.bias"], padding=1)
    if cfg.get("use_quant_conv", False):
        x = _conv2d(x, sd["quant_conv.weight"], sd["quant_conv.bias"])
    return x
