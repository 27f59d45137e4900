"""ms per call of the frame-axis attention operator (univst_temporal_attention) and of the whole native motion module (univst_amd/motion.py), each next
to the torch-fp16 path on the same box, with HIP-event timing.  Random weights: the graph does not depend on their values.

    python tools/bench_motion.py [--calls 30] [--warmup 5] [--out profiles/motion_native.json]

Shapes: the four levels of a 16 x 512 x 512 three-branch AnimateDiff step, B = 3 branches, F = 16 frames, 8 heads:
N = 4096 / C = 320, N = 1024 / C = 640, N = 256 / C = 1280, N = 64 / C = 1280.

Operator: the native kernel reads q | k | v rows in place; the torch path is what the reference's attention does with those rows — regroup
``(b f) n c -> (b n) f c`` per head (one transposed copy each of q, k, v), ``F.scaled_dot_product_attention``, regroup back.  The line carries the
fraction of the 8 TB/s HBM peak at the operator's compulsory bytes = rows x 4C x 2 (3C halfs read, C written per row).
Module: ``NativeMotionModule.forward_rows`` against the torch-fp16 restatement (tests/motion_ref.py) on the [B, C, F, H, W] tensor.

The two implementations are timed ALTERNATELY in one process (native call, torch call, native call, ...), each call bracketed by its own pair of
events after `warmup` calls of both; every figure is the median over `calls`."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8e12
LEVELS = ((4096, 320), (1024, 640), (256, 1280), (64, 1280))      # (N, C)
B, FR, HEADS = 3, 16, 8


def timed_pair(fa, fb, calls, warmup):
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ms = ([], [])
    for _ in range(calls):
        for i, fn in enumerate((fa, fb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[i].append(e0.elapsed_time(e1))
    return [(statistics.median(m), min(m), max(m)) for m in ms]


def torch_attention(qkv, N, Cw):
    """the torch fp16 path on the same rows: q carries the scale already, so scale = 1"""
    d = Cw // HEADS
    x = qkv.view(B, FR, N, 3, HEADS, d).permute(3, 0, 2, 4, 1, 5).reshape(3, B * N, HEADS, FR, d)      # the regrouped copy
    o = F.scaled_dot_product_attention(x[0], x[1], x[2], scale=1.0)
    return o.view(B, N, HEADS, FR, d).permute(0, 3, 1, 2, 4).reshape(B * FR * N, Cw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    assert a.calls >= 20, "at least 20 timed calls"
    import motion_ref as R
    from univst_amd import _native
    from univst_amd.motion import NativeMotionModule
    op_rows, mod_rows = [], []
    for N, Cw in LEVELS:
        rows, d = B * FR * N, Cw // HEADS
        g = torch.Generator(device="cuda").manual_seed(N)
        qkv = torch.randn(rows, 3 * Cw, generator=g, device="cuda", dtype=torch.float32)
        qkv[:, :2 * Cw] *= (3.0 / d ** 0.5) ** 0.5
        qkv = qkv.half()
        out = torch.empty(rows, Cw, device="cuda", dtype=torch.float16)
        with torch.no_grad():
            err = (_native.temporal_attention(qkv, B, FR, N, HEADS, d, out=out).float() - torch_attention(qkv, N, Cw).float()).abs().max().item()
            nat, ref = timed_pair(lambda: _native.temporal_attention(qkv, B, FR, N, HEADS, d, out=out), lambda: torch_attention(qkv, N, Cw), a.calls, a.warmup)
        nbytes = rows * 4 * Cw * 2
        op_rows.append({"N": N, "C": Cw, "head_dim": d, "rows": rows, "bytes": nbytes, "native_ms": round(nat[0], 4),
                        "native_ms_min_max": [round(nat[1], 4), round(nat[2], 4)], "native_hbm_fraction": round(nbytes / (nat[0] * 1e-3) / HBM_PEAK, 3),
                        "torch_fp16_ms": round(ref[0], 4), "torch_fp16_ms_min_max": [round(ref[1], 4), round(ref[2], 4)],
                        "max_abs_diff_to_torch": round(err, 5)})
        del qkv, out
        cfg = R.Cfg(channels=Cw, num_heads=HEADS, num_blocks=1, attn_per_block=2, max_len=32)
        sd = {k: v.half().cuda() for k, v in R.random_state_dict(cfg, seed=Cw).items()}
        mod = NativeMotionModule(sd, config=dict(num_attention_heads=HEADS, num_transformer_block=1, temporal_position_encoding=True,
                                                 temporal_position_encoding_max_len=32))
        side = int(N ** 0.5)
        x5 = torch.randn(B, Cw, FR, side, side, generator=g, device="cuda", dtype=torch.float32).half()
        xr = x5.permute(0, 2, 3, 4, 1).reshape(rows, Cw).contiguous()
        with torch.no_grad():
            nat, ref = timed_pair(lambda: mod.forward_rows(xr, B, FR, N), lambda: R.forward(sd, cfg, x5, dtype=torch.float16), a.calls, a.warmup)
        mod_rows.append({"N": N, "C": Cw, "rows": rows, "native_ms": round(nat[0], 4), "native_ms_min_max": [round(nat[1], 4), round(nat[2], 4)],
                         "torch_fp16_ms": round(ref[0], 4), "torch_fp16_ms_min_max": [round(ref[1], 4), round(ref[2], 4)],
                         "arena_high_water": mod.query("arena_high_water")})
        del mod, sd, x5, xr
        torch.cuda.empty_cache()
    res = {"what": "AnimateDiff motion module, B = 3, F = 16, 8 heads: frame-axis attention operator and whole module, native library vs torch fp16",
           "device": torch.cuda.get_device_name(0), "calls": a.calls, "warmup": a.warmup,
           "timing": "HIP events around each call, the two alternating; median (min, max) over the calls", "hbm_peak_bytes_per_s": HBM_PEAK,
           "operator": op_rows, "module": mod_rows}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
