"""The static style branch against the three-branch step it replaces (DESIGN.md "Static style branch"), SD-v1.5 widths, 16 x 64 x 64 latents:

    step inside the PnP window (idx 10): the existing three-branch forward on a repeated style  vs  style_bank (one frame) + forward_static_style (B = 2)
    style-inversion step:                the single-branch forward at F = 16                     vs  at F = 1

Both arms of a pair run in ONE process and alternate round by round (as tools/ab.sh alternates builds): the yardstick is the existing step in this
very run.  Before timing, the static step's stylised eps is compared with the three-branch one on the same inputs.  Synthetic weights
(univst_amd.synth), device events around `--iters` calls per round.  Prints one line per figure and, with --out, writes them to that file:

    python tools/bench_static_style.py --out profiles/static_style.txt
"""
import argparse
import os
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(arms, rounds, iters, warmup):
    """arms: {name: fn} -> {name: [ms per call of every round]}; the arms take turns inside every round"""
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            out[k].append(timed(fn, iters))
    return out


def line(name, ms):
    return f"{name}: mean {sum(ms) / len(ms):.3f} ms, min {min(ms):.3f}, max {max(ms):.3f} over {len(ms)} rounds"


def main(a):
    from univst_amd import synth
    from univst_amd.backbones.video_diffusion_sd import pnp_utils
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = "cuda"
    F, h = a.frames, a.latent
    unet = synth.build_unet(device=dev, seed=33)
    pipe = types.SimpleNamespace(unet=unet)
    content, style, text3, _ = synth.synth_transfer_inputs(F=F, h=h, w=h, n=1, device=dev)
    frame = style[0][:, :, :1].contiguous()
    rep = frame.expand(-1, -1, F, -1, -1).contiguous()
    x3 = torch.cat([content[0], rep, content[1]])
    x2, t2 = torch.cat([content[0], content[1]]), text3[::2].contiguous()
    t = 781
    lines = [f"static style bench: SD-v1.5 widths, F = {F}, {h} x {h} latents, idx {a.idx}, {a.rounds} rounds x {a.iters} calls, {torch.cuda.get_device_name(0)}"]

    # ---- the style-inversion step (PnP not registered yet: the inversion runs the stock key sources)
    inv = alternate({"inversion step F=%d" % F: lambda: unet(rep, t, encoder_hidden_states=text3[1:2]),
                     "inversion step F=1": lambda: unet(frame, t, encoder_hidden_states=text3[1:2])}, a.rounds, a.iters, a.warmup)

    # ---- the step inside the window
    pnp_utils.register_spatial_attention_pnp(pipe)
    pnp_utils.register_time(pipe, a.idx)
    bank = unet.style_bank(frame, t, text3[1:2])
    assert bank is not None, f"idx {a.idx} is outside the PnP window"

    def static_step():
        unet.style_bank(frame, t, text3[1:2], bank=bank)
        return unet.forward_static_style(x2, t, t2, bank).sample

    def bank_only():
        unet.style_bank(frame, t, text3[1:2], bank=bank)

    ref = unet(x3, t, encoder_hidden_states=text3).sample[2].float()
    got = static_step()[1].float()
    d = (got - ref).abs().max().item() / ref.abs().max().item()
    lines.append(f"static vs three-branch stylised eps on the same inputs: max |diff| = {d:.3e} of max|eps|")
    assert d < 5e-3, d
    step = alternate({"three-branch step (style repeated)": lambda: unet(x3, t, encoder_hidden_states=text3),
                      "static step (bank + B=2)": static_step, "  of which the bank call": bank_only}, a.rounds, a.iters, a.warmup)
    for k, v in list(step.items()) + list(inv.items()):
        lines.append(line(k, v))
    # how much of the one-frame call is the host enqueueing its launches: the host clock up to the last enqueue, then up to the drained stream
    torch.cuda.synchronize()
    n = 4 * a.iters
    t0 = time.perf_counter()
    for _ in range(n):
        bank_only()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    lines.append(f"bank call, host clock over {n} calls: enqueue {1e3 * (t1 - t0) / n:.3f} ms per call, until the stream is drained {1e3 * (t2 - t0) / n:.3f} ms per call")
    m = lambda d_, k: sum(d_[k]) / len(d_[k])
    three, static = m(step, "three-branch step (style repeated)"), m(step, "static step (bank + B=2)")
    lines.append(f"static / three-branch = {static / three:.3f} (frame-forwards: {2 * F + 1} / {3 * F} = {(2 * F + 1) / (3 * F):.3f})")
    lines.append(f"inversion F=1 / F={F} = {m(inv, 'inversion step F=1') / m(inv, 'inversion step F=%d' % F):.3f} (frame-forwards: 1 / {F})")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=16)
    p.add_argument("--latent", type=int, default=64)
    p.add_argument("--idx", type=int, default=10)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--iters", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--out", type=str, default="")
    main(p.parse_args())
