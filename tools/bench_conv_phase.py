"""A/B of the UNet's three upsampler convs (16 x 512 x 512 three-branch step, 48 images): conv_patch_kernel in its 9-tap form over the nearest-x2
upsampled input (univst_conv3x3_patch, weights [Co][Ci/32][9][32]) against its phase form (univst_conv3x3_up2_phase: four 2x2-tap convs over the source
image, weights [4][Co][Ci/32][4][32]) — interleaved rounds in one process, random operands, best of the rounds.  TFLOP/s are ALGORITHMIC (2 M N 9 Cin)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from univst_amd import _native

SHAPES = [(640, 32), (1280, 16), (1280, 8)]      # (C, source side): 32x32 -> 64x64, 16x16 -> 32x32, 8x8 -> 16x16


def timeit(f, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main(rounds=5, iters=10):
    tot_a = tot_b = 0.0
    for C, H in SHAPES:
        imgs = 48
        x = torch.randn(imgs, H, H, C, device="cuda", dtype=torch.float16)
        w = torch.randn(C, C, 3, 3, device="cuda", dtype=torch.float16) * 0.02
        w32 = w.reshape(C, C // 32, 32, 9).permute(0, 1, 3, 2).contiguous()
        w4 = _native.conv_up2_phase_weights(w)
        b = torch.randn(C, device="cuda", dtype=torch.float16)
        fa = lambda: _native.conv3x3_patch(x, w32, bias=b, upsample=True)
        fb = lambda: _native.conv3x3_up2_phase(x, w4, bias=b)
        ya, yb = fa(), fb()
        err = (ya.float() - yb.float()).abs().max().item() / ya.float().abs().max().item()
        ta, tb = [], []
        for _ in range(rounds):
            ta.append(timeit(fa, iters))
            tb.append(timeit(fb, iters))
        fl = 2.0 * imgs * 4 * H * H * C * 9 * C
        a, bb = min(ta), min(tb)
        tot_a += a
        tot_b += bb
        print(f"up-conv {C}->{C} {H}x{H}->{2 * H}x{2 * H}: 9-tap {a:7.4f} ms {fl / a / 1e9:7.1f} TF | phase {bb:7.4f} ms {fl / bb / 1e9:7.1f} TF (algorithmic) | "
              f"x{a / bb:.3f} | rounds 9-tap {' '.join(f'{t:.4f}' for t in ta)} | phase {' '.join(f'{t:.4f}' for t in tb)} | rel diff {err:.1e}", flush=True)
    print(f"sum: 9-tap {tot_a:.4f} ms, phase {tot_b:.4f} ms, x{tot_a / tot_b:.3f}")


if __name__ == "__main__":
    main()
