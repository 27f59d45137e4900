"""Host-side mirror of backbones/animatediff/pnp_utils.py of the reference: same four names, same arguments.  ``register_*`` only record state on
the attention modules; the injected attention (the AdaIN-guided q / k / v shift in front of the frame's own self-attention) runs inside the native
AnimateDiff UNet graph (csrc/unet.hip, csrc/pnp.hip).  What differs from the SD path's closure: the window is ``eta1 * 50 <= idx < eta2 * 50``
(pnp_utils.py:45: exclusive at the top, eta1 scaled), alpha = 0.8 and gamma = 2.0 (:47-49), and no key frames are gathered (attn1 is called without
``clip_length``).  ``attention_adain`` / ``latent_adain`` are the same functions as the SD path's and call the HIP kernels directly."""
from ..video_diffusion_sd.pnp_utils import attention_adain, latent_adain  # noqa: F401

# pnp_utils.py:8,102 — {up_block: [attention indices]}
PNP_LAYERS = {1: [1, 2], 2: [0, 1, 2], 3: [0, 1, 2]}
ALPHA, GAMMA = 0.8, 2.0      # pnp_utils.py:47,49


def register_time(model, t):
    """pnp_utils.py:7-15"""
    for res, blocks in PNP_LAYERS.items():
        for block in blocks:
            tb = model.unet.up_blocks[res].attentions[block].transformer_blocks[0]
            setattr(tb.attn1, "idx", t)
            setattr(tb.attn2, "idx", t)


def register_spatial_attention_pnp(model, eta1=0.0, eta2=0.5):
    """pnp_utils.py:18-109: mark the 8 decoder attn1 layers as PnP layers (window eta1 * 50 <= idx < eta2 * 50)"""
    for res, blocks in PNP_LAYERS.items():
        for block in blocks:
            m = model.unet.up_blocks[res].attentions[block].transformer_blocks[0].attn1
            setattr(m, "eta1", eta1)
            setattr(m, "eta2", eta2)
            setattr(m, "_univst_native_pnp", True)
