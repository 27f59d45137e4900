"""ms per image pair of the native RAFT-large (univst_amd/flow.py) with HIP-event timing, and its split into encoders, correlation volume and the
12 updates (+ upsampling).  Random weights: the graph does not depend on their values.

    python tools/bench_flow.py [--size 512] [--calls 30] [--warmup 5] [--out profiles/flow_native_512.json]

The stages are timed through the library's own stage entries (univst_raft_encode, univst_raft_corr_pyramid); "updates" is the rest of a full call.
Every figure is the median over `calls` back-to-back calls after `warmup` calls, each bracketed by its own pair of events."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def random_state_dict(seed=0):
    """raft_large's tensors by name and shape (torchvision's keys), seeded random values"""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def conv(name, co, ci, kh, kw, bn=None):
        sd[name + ".weight"] = torch.randn(co, ci, kh, kw, generator=g) / (ci * kh * kw) ** 0.5
        sd[name + ".bias"] = torch.randn(co, generator=g) * 0.05
        if bn:
            sd[bn + ".weight"], sd[bn + ".bias"] = torch.rand(co, generator=g) + 0.5, torch.randn(co, generator=g) * 0.1
            sd[bn + ".running_mean"], sd[bn + ".running_var"] = torch.randn(co, generator=g) * 0.1, torch.rand(co, generator=g) + 0.5
    for enc, bn in (("feature_encoder", False), ("context_encoder", True)):
        cna = lambda m, co, ci, k: conv(m + ".0", co, ci, k, k, m + ".1" if bn else None)
        cna(enc + ".convnormrelu", 64, 3, 7)
        ch = [64, 64, 96, 128]
        for L in (1, 2, 3):
            for B in (0, 1):
                p, ci = f"{enc}.layer{L}.{B}", ch[L - 1] if B == 0 else ch[L]
                cna(p + ".convnormrelu1", ch[L], ci, 3)
                cna(p + ".convnormrelu2", ch[L], ch[L], 3)
                if B == 0 and L > 1:
                    cna(p + ".downsample", ch[L], ci, 1)
        conv(enc + ".conv", 256, 128, 1, 1)
    me = "update_block.motion_encoder."
    for n, co, ci, k in (("convcorr1", 256, 324, 1), ("convcorr2", 192, 256, 3), ("convflow1", 128, 2, 7), ("convflow2", 64, 128, 3), ("conv", 126, 256, 3)):
        conv(me + n + ".0", co, ci, k, k)
    for d, (kh, kw) in ((1, (1, 5)), (2, (5, 1))):
        for c in ("convz", "convr", "convq"):
            conv(f"update_block.recurrent_block.convgru{d}.{c}", 128, 384, kh, kw)
    conv("update_block.flow_head.conv1", 256, 128, 3, 3)
    conv("update_block.flow_head.conv2", 2, 256, 3, 3)
    conv("mask_predictor.convrelu.0", 256, 128, 3, 3)
    conv("mask_predictor.conv", 576, 256, 1, 1)
    return sd


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    assert a.calls >= 20, "at least 20 timed calls"
    from univst_amd import flow
    net = flow.NativeRAFT.from_state_dict(random_state_dict())
    g = torch.Generator().manual_seed(1)
    img1 = torch.randint(0, 256, (a.size, a.size, 3), generator=g, dtype=torch.uint8).cuda()
    img2 = torch.randint(0, 256, (a.size, a.size, 3), generator=g, dtype=torch.uint8).cuda()
    fh = a.size // 8
    n = fh * fh
    fmap, _, _ = net.encode(img1, img2)
    total = timed(lambda: net(img1, img2), a.calls, a.warmup)
    enc = timed(lambda: net.encode(img1, img2), a.calls, a.warmup)
    vol = timed(lambda: flow.corr_pyramid(fmap[0], fmap[1], fh, fh), a.calls, a.warmup)
    pyr_bytes = 4 * sum(n * (fh >> l) ** 2 for l in range(4))
    res = {"what": "native RAFT-large, one image pair, 12 flow updates", "device": torch.cuda.get_device_name(0), "size": a.size, "calls": a.calls, "warmup": a.warmup,
           "timing": "HIP events around each call, median (min, max) over the calls",
           "ms_per_pair": round(total[0], 3), "ms_per_pair_min_max": [round(total[1], 3), round(total[2], 3)],
           "ms_encoders": round(enc[0], 3), "ms_volume_and_pyramid": round(vol[0], 3), "ms_12_updates_and_upsample": round(total[0] - enc[0] - vol[0], 3),
           "volume_bytes_level0": 4 * n * n, "pyramid_bytes": pyr_bytes, "volume_gflop": round(2.0 * n * n * 256 / 1e9, 2)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
