"""GEMM-level timing of the MX-fp8 q | k | v projection against the fp16 one (profiles/sd3_mxfp8_qkv.txt (a)).

    python tools/bench_mxfp8.py [--rounds 3] [--iters 10]

Shapes of an SD3.5-medium step at 16 x 1024^2, three branches: the image stream (M = 196 608 rows) and the text stream (M = 15 984 = 48 x 333 rows),
N = 4 608 (q | k | v), K = 1 536.  Per round and shape, in this order, on one device: univst_linear (fp16), univst_mxfp8_quantize of the activation
rows, univst_linear_mxfp8, and quantise + MX linear back to back (what the attention op runs per call; the weight is quantised once, outside).
Times are device events around `iters` launches after a warm-up; rates are 2 M N K over the time, against the fp16 roof and the 2 x MX roof."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from univst_amd import _native  # noqa: E402

PEAK_F16, PEAK_MX = 2.5e15, 5.0e15          # dense MFMA rates of the MI355X: fp16 / bf16, and block-scaled e4m3
HBM = 8.0e12


def timeit(f, iters):
    f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--json", default=None, help="also write the rows here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mxfp8: needs the GPU (no CPU path)")
    N, K = 4608, 1536
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).half().cuda()
    b = (0.1 * torch.randn(N, generator=g)).half().cuda()
    wq, ws = _native.mxfp8_quantize(w)
    rows = []
    for M in (196608, 15984):
        x = torch.randn(M, K, generator=g).half().cuda()
        out = torch.empty(M, N, device="cuda", dtype=torch.float16)
        xq, xs = _native.mxfp8_quantize(x)
        fl = 2.0 * M * N * K
        arms = {
            "fp16 linear": lambda: _native.linear(x, w, bias=b, out=out),
            "quantise": lambda: _native.mxfp8_quantize(x),
            "mx linear": lambda: _native.linear_mxfp8(xq, xs, wq, ws, bias=b, out=out),
            "quantise + mx linear": lambda: _native.linear_mxfp8(*_native.mxfp8_quantize(x), wq, ws, bias=b, out=out),
        }
        for r in range(a.rounds):
            for name, f in arms.items():
                ms = timeit(f, a.iters)
                row = dict(M=M, N=N, K=K, arm=name, round=r, ms=round(ms, 4))
                if name == "quantise":
                    row["GBps"] = round(M * K * (2 + 1 + 1 / 32) / ms / 1e6, 1)
                    print(f"M={M:6d} round {r} {name:22s} {ms:8.3f} ms  {row['GBps']:8.1f} GB/s ({row['GBps'] * 1e9 / HBM:.0%} of {HBM / 1e12:.0f} TB/s)")
                else:
                    tf = fl / ms / 1e9
                    row.update(TFLOPs=round(tf, 1), of_fp16_roof=round(tf * 1e12 / PEAK_F16, 3), of_mx_roof=round(tf * 1e12 / PEAK_MX, 3))
                    print(f"M={M:6d} round {r} {name:22s} {ms:8.3f} ms  {tf:7.1f} TFLOP/s  {row['of_fp16_roof']:.0%} of the fp16 roof, "
                          f"{row['of_mx_roof']:.0%} of the MX roof")
                rows.append(row)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
