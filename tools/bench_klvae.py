"""Seconds per decode / encode of the native plain AutoencoderKL (univst_amd/vae.py NativeAutoencoderKL, the SD3 VAE) and of the torch-fp16
restatement (tests/klvae_ref.py, what the reference's ``vae.to(fp16).cuda()`` computes) in ONE process.  Random weights: the graph does not
depend on their values.

    python tools/bench_klvae.py [--images 16] [--latent 128] [--out profiles/klvae_native.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_klvae.py --trace-one        # one warm-up and one decode of ONE image, nothing else

SD3 widths (128, 256, 512, 512), default budgets.  Native: median of 5 wall-clock timed calls (device synchronised) after a warm-up; torch fp16:
median of 3 after a warm-up, two images at a time with torch's own convolutions.  The VAE runs twice per clip: it is off bench.py's metric."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), ts


def main():
    import klvae_ref as R
    from univst_amd import synth, vae
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--latent", type=int, default=128)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-one", action="store_true")
    a = ap.parse_args()
    cfg = dict(R.SD3_VAE_CONFIG)
    sd = synth.klvae_state_dict(cfg, seed=21)
    v = vae.NativeAutoencoderKL(sd, cfg)
    n, lat = a.images, a.latent
    z = torch.randn(n, 16, lat, lat, generator=torch.Generator().manual_seed(6)).half().cuda()
    if a.trace_one:
        for _ in range(2):
            v.decode(z[:1])
            torch.cuda.synchronize()
        return
    x = (torch.rand(n, 3, 8 * lat, 8 * lat, generator=torch.Generator().manual_seed(7)) * 2 - 1).half().cuda()
    out = {"images": n, "pixels": 8 * lat}
    out["native_decode_s"], out["native_decode_all"] = timed(lambda: v.decode(z), 5)
    out["decode_passes"], out["decode_chunks"], out["decode_arena"] = v.query("passes"), v.query("attn_chunks"), v.query("arena_high_water")
    out["native_encode_s"], out["native_encode_all"] = timed(lambda: v.encode(x), 5)
    out["encode_passes"], out["encode_arena"] = v.query("passes"), v.query("arena_high_water")
    h = {k: t.half() for k, t in sd.items()}

    def t16(fn, inp):
        with torch.no_grad():
            return torch.cat([fn(h, inp[i:i + 2], cfg) for i in range(0, n, 2)])
    out["torch_fp16_decode_s"], out["torch_fp16_decode_all"] = timed(lambda: t16(R.decode, z), 3)
    out["torch_fp16_encode_s"], out["torch_fp16_encode_all"] = timed(lambda: t16(R.encode_moments, x), 3)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
