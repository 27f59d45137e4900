"""ms per encode of the native CLIP text tower (univst_amd/text.py) and of the torch-fp16 restatement (tests/clip_ref.py, what the reference's
``text_encoder.to(fp16).cuda()`` computes) with HIP-event timing.  Random weights: the graph does not depend on their values.

    python tools/bench_text.py [--calls 30] [--warmup 5] [--out profiles/text_native.json]
    python tools/bench_text.py --model t5 [--calls 30] [--warmup 5] [--out profiles/text_t5_native.json]

Towers: CLIP-L (768 / 12 heads / 12 layers, no projection) and CLIP-bigG (1280 / 20 heads / 32 layers, projection 1280) at B = 1 and 3, S = 77.
The two implementations are timed ALTERNATELY in one process (native call, torch call, native call, ...), each call bracketed by its own pair of
events after `warmup` calls of both; every figure is the median over `calls`.  The encoder runs a few times per clip: it is off bench.py's metric.

``--model t5``: the native T5 encoder (NativeT5Encoder) at T5 v1.1-XXL size (24 layers, d_model 4096, 64 heads, d_ff 10240; 4.7 G parameters) at
S = 256, B = 1 and 3, against the torch-fp16 restatement (tests/t5_ref.py), the same way.  One call reads every layer's weights once (9.4 GB of
fp16): the line carries that floor at the 8 TB/s HBM peak next to the measured figures."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def random_state_dict(cfg, shapes, seed=0):
    """the tower's tensors by name and shape, seeded fp16 values made on the device (bigG has 0.7 G parameters)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    sd = {}
    for k, shape in shapes.items():
        t = torch.randn(shape, generator=g, device="cuda", dtype=torch.float32)
        if "layer_norm" in k and k.endswith(".weight"):
            t = 1.0 + 0.1 * t
        elif k.endswith(".bias"):
            t = 0.1 * t
        elif "embedding" in k:
            t = 0.4 * t
        else:
            t = t / shape[1] ** 0.5
        sd[k] = t.half()
    return sd


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


def t5_rows(calls, warmup):
    import t5_ref as R
    from univst_amd.text import NativeT5Encoder
    cfg = R.T5_XXL
    g = torch.Generator(device="cuda").manual_seed(0)
    sd = {}
    for k, shape in R.state_dict_shapes(cfg).items():      # seeded fp16 values made on the device, scaled as R.random_state_dict scales them
        t = torch.randn(shape, generator=g, device="cuda", dtype=torch.float16)
        if k.endswith("layer_norm.weight"):
            t = 1.0 + 0.1 * t
        elif len(shape) == 2 and "relative_attention_bias" not in k and k != "shared.weight":
            t = t * ((0.56 if ".q.weight" in k or ".k.weight" in k else 1.0) / shape[1] ** 0.5)
        sd[k] = t
    enc = NativeT5Encoder.from_state_dict(sd, R.hf_config(cfg))
    per_call = sum(v.numel() * 2 for k, v in sd.items() if k != "shared.weight")      # every layer's weights, once
    rows = []
    for B in (1, 3):
        ids = R.make_ids(cfg, B, 256, seed=B).cuda()
        with torch.no_grad():
            nat, ref = timed_pair(lambda: enc(ids), lambda: R.forward(sd, cfg, ids, dtype=torch.float16), calls, warmup)
        rows.append({"encoder": "T5-v1.1-XXL", "B": B, "S": 256, "native_ms": round(nat[0], 3), "native_ms_min_max": [round(nat[1], 3), round(nat[2], 3)],
                     "torch_fp16_ms": round(ref[0], 3), "torch_fp16_ms_min_max": [round(ref[1], 3), round(ref[2], 3)]})
    return {"what": "T5 encoder, one encode: native library (fp32 residual stream) vs the torch-fp16 restatement", "device": torch.cuda.get_device_name(0),
            "calls": calls, "warmup": warmup, "timing": "HIP events around each call, the two alternating; median (min, max) over the calls",
            "weight_bytes_read_per_call": per_call, "weight_read_floor_ms_at_8TBs": round(per_call / 8e12 * 1e3, 3),
            "handle_weight_bytes": enc.query("weight_bytes"), "arena_high_water": enc.arena_high_water(), "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("clip", "t5"), default="clip")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    assert a.calls >= 20, "at least 20 timed calls"
    if a.model == "t5":
        line = json.dumps(t5_rows(a.calls, a.warmup))
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    import clip_ref as R
    from univst_amd.text import NativeCLIPText
    rows = []
    for name, cfg in (("CLIP-L", R.CLIP_L), ("CLIP-bigG", R.CLIP_BIGG)):
        sd = random_state_dict(cfg, R.state_dict_shapes(cfg))
        enc = NativeCLIPText.from_state_dict(sd, dict(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
                                                      num_hidden_layers=cfg.num_layers, num_attention_heads=cfg.num_heads, max_position_embeddings=cfg.max_positions,
                                                      hidden_act=cfg.hidden_act, layer_norm_eps=cfg.layer_norm_eps, projection_dim=cfg.projection_dim or 768,
                                                      eos_token_id=cfg.eos_token_id))
        for B in (1, 3):
            ids = R.make_ids(cfg, B, 77, seed=B, eos_at=[20] * B).cuda()
            with torch.no_grad():
                nat, ref = timed_pair(lambda: enc(ids), lambda: R.forward(sd, cfg, ids, dtype=torch.float16), a.calls, a.warmup)
            rows.append({"tower": name, "B": B, "S": 77, "native_ms": round(nat[0], 3), "native_ms_min_max": [round(nat[1], 3), round(nat[2], 3)],
                         "torch_fp16_ms": round(ref[0], 3), "torch_fp16_ms_min_max": [round(ref[1], 3), round(ref[2], 3)]})
        del enc, sd
        torch.cuda.empty_cache()
    res = {"what": "CLIP text tower, one encode: native library vs the torch-fp16 restatement", "device": torch.cuda.get_device_name(0), "calls": a.calls,
           "warmup": a.warmup, "timing": "HIP events around each call, the two alternating; median (min, max) over the calls", "rows": rows}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
