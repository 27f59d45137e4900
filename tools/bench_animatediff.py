"""ms per denoising step of the native AnimateDiff UNet3D (univst_unet_create_animatediff through the mirror
univst_amd/backbones/animatediff/models/unet.py) at the size a user runs: SD-v1.5 widths (320 / 640 / 1280 / 1280, 8 heads, 768-wide text), the
animatediff-v2.yaml motion modules (21, 8 heads, one block of two Temporal_Self attentions, position encoding), three branches x 16 frames of 64x64
latents, PnP registered inside its window.  Synthetic seeded weights with a non-zero proj_out: the graph does not depend on their values, only on no
module being skipped.

    python tools/bench_animatediff.py [--steps 20] [--warmup 3] [--variants motion:0,motion:1 | fold:0,fold:1] [--out profiles/animatediff_step.json]

Variants are timed ALTERNATELY in one process (step of A, step of B, step of A, ...), each step bracketed by its own pair of HIP events after
`warmup` steps of every variant; a figure is the median (min, max) over `steps`.
  motion:1 / motion:0   the UNet with its 21 modules against the same weights with every proj_out zero (all modules skipped: the per-frame 2-D UNet).
                        The difference is what the modules cost inside the step.
  fold:0 / fold:1       option motion_fold (only where the library has it built; a refused value ends the run with the library's message).
`--once` runs a single step of motion:1 after one warm-up step and exits: the body of a kernel-trace run."""
import argparse
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

B, FR, H, W, TEXT_LEN = 3, 16, 64, 64, 77


def build(zero_motion, options):
    import animatediff_ref as R
    from univst_amd.backbones.animatediff import pnp_utils
    from univst_amd.backbones.animatediff.models.unet import UNet3DConditionModel
    cfg = R.make_cfg(max_len=24)
    m = UNet3DConditionModel(**R.reference_kwargs(cfg))
    m.load_state_dict(R.random_state_dict(cfg, seed=21, zero_motion=zero_motion), strict=True)
    m = m.half().cuda().eval()
    for k, v in options.items():
        m.set_native_option(k, v)
    pipe = types.SimpleNamespace(unet=m)
    pnp_utils.register_spatial_attention_pnp(pipe, eta1=0.0, eta2=0.5)
    pnp_utils.register_time(pipe, 10)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--variants", type=str, default="motion:1,motion:0")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_animatediff measures on the GPU only"
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, 4, FR, H, W, generator=g).half().cuda()
    txt = torch.randn(B, TEXT_LEN, 768, generator=g).half().cuda()
    if a.once:
        m = build(False, {})
        m(x, 481, txt)
        torch.cuda.synchronize()
        m(x, 481, txt)
        torch.cuda.synchronize()
        print(json.dumps({"once": True, "arena_high_water": m.native_query("arena_high_water"), "motion_active": m.native_query("motion_active")}))
        return
    names = [v.strip() for v in a.variants.split(",") if v.strip()]
    models = {}
    for v in names:
        kind, val = v.split(":")
        models[v] = build(zero_motion=(kind == "motion" and val == "0"), options={"motion_fold": int(val)} if kind == "fold" else {})
    outs = {}
    for _ in range(a.warmup):
        for v in names:
            outs[v] = models[v](x, 481, txt).sample
    torch.cuda.synchronize()
    ms = {v: [] for v in names}
    for _ in range(a.steps):
        for v in names:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            models[v](x, 481, txt)
            e1.record()
            e1.synchronize()
            ms[v].append(e0.elapsed_time(e1))
    res = {"what": "native AnimateDiff UNet3D step, SD-v1.5 widths, 3 x 16 x 64 x 64 latents, PnP inside the window (idx 10), 21 motion modules",
           "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup,
           "timing": "HIP events around each step, the variants alternating; median (min, max) over the steps",
           "variants": {v: {"ms_per_step": round(statistics.median(ms[v]), 3), "ms_min_max": [round(min(ms[v]), 3), round(max(ms[v]), 3)],
                            "ms_first_half_median": round(statistics.median(ms[v][:len(ms[v]) // 2]), 3),
                            "ms_second_half_median": round(statistics.median(ms[v][len(ms[v]) // 2:]), 3),
                            "motion_active": int(models[v].native_query("motion_active")), "arena_high_water": int(models[v].native_query("arena_high_water")),
                            "arena_bytes": int(models[v].native_query("arena_bytes")), "finite": bool(torch.isfinite(outs[v]).all())} for v in names}}
    if "motion:1" in ms and "motion:0" in ms:
        res["modules_ms_per_step"] = round(statistics.median(ms["motion:1"]) - statistics.median(ms["motion:0"]), 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
