"""Model-level error of the MX-fp8 q | k | v switch (profiles/sd3_mxfp8_qkv.txt (c)): one three-branch SD3.5-medium forward at 1024 px, inside the
shift window, against oracle/sd3_ref.sd3_transformer in fp32 on the device — the set-up of tests/test_gpu_sd3.py
test_sd35_medium_three_branch_forward_at_1024px_vs_oracle — once with qkv_dtype fp16 and once with mxfp8.  Run once by hand; not part of the suite.

    python tools/sd3_mxfp8_parity.py [--idx 12]
"""
import argparse
import json
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from oracle import sd3_ref  # noqa: E402
from univst_amd.backbones.video_diffusion_sd3 import pnp_utils  # noqa: E402
from univst_amd.backbones.video_diffusion_sd3.models.transformer_3D_model import sd35_medium  # noqa: E402


def errs(got, ref):
    e = got.float() - ref.float()
    return e.abs().max().item() / ref.abs().max().item(), (e.pow(2).mean().sqrt() / ref.float().pow(2).mean().sqrt()).item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--idx", type=int, default=12)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    torch.manual_seed(1905)
    with torch.device("cuda"):
        m = sd35_medium()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("norm_q.weight") or n.endswith("norm_k.weight") or "norm_added" in n:
                p.copy_(1.0 + 0.2 * torch.randn_like(p))
    m = m.half().requires_grad_(False)
    pnp_utils.register_spatial_attention_pnp(types.SimpleNamespace(transformer=m), eta1=0.0, eta2=0.6)
    Fc, hl, T = 3, 128, 77 + 256
    for proc in m.attn_processors.values():
        proc.clip_length = Fc
    g = torch.Generator(device="cuda").manual_seed(7)
    lat = torch.randn(3 * Fc, 16, hl, hl, generator=g, device="cuda").half()
    lat[2 * Fc:] = lat[2 * Fc:] * 1.2 + 0.1
    enc = torch.randn(1, T, 4096, generator=g, device="cuda").half().expand(3 * Fc, -1, -1).contiguous()
    pooled = torch.randn(1, 2048, generator=g, device="cuda").half().expand(3 * Fc, -1).contiguous()
    t = torch.tensor([437.0], device="cuda")
    got = {}
    for qd in ("fp16", "mxfp8"):
        m.set_qkv_dtype(qd)
        got[qd] = m(hidden_states=lat, timestep=t.expand(3 * Fc), encoder_hidden_states=enc, pooled_projections=pooled, return_dict=False,
                    joint_attention_kwargs={"idx": a.idx})[0].float()
    torch.cuda.synchronize()
    P = {k: v.float() for k, v in m.state_dict().items()}
    sd3_ref.SDPA_MAX_BATCH = 1
    with torch.no_grad():
        want = sd3_ref.sd3_transformer(P, m.config, lat.float(), enc.float(), pooled.float(), t,
                                       attn_kw=dict(idx=a.idx, shift=True, eta1=0.0, eta2=0.6, clip_length=Fc))
    out = {}
    for qd in ("fp16", "mxfp8"):
        mx, rms = errs(got[qd], want)
        out[qd] = {"max_rel_to_max": mx, "rel_rms": rms}
        print(f"SD3.5-medium 3x{Fc} frames at 1024 px, idx {a.idx}, qkv {qd}: max {mx:.3e} of max|ref|, relative rms {rms:.3e} (vs the fp32 oracle)")
    mx, rms = errs(got["mxfp8"], got["fp16"])
    out["mxfp8_vs_fp16"] = {"max_rel_to_max": mx, "rel_rms": rms}
    print(f"mxfp8 against the fp16 model: max {mx:.3e}, relative rms {rms:.3e}")
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
