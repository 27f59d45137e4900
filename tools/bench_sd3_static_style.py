"""The SD3 static style branch and the dead-branch skip against the three-branch step they replace, at the
BASELINE config-5 size: SD3.5-medium MM-DiT (random-init weights), 16 frames x 1024 x 1024 (4096 image + 333 text tokens per frame):

    three-branch step (B = 3F, style frame repeated), inside the window    what every step costs today
    static step inside the window: style_bank (one frame) + forward_static_style (B = 2F)
    single-branch step outside the window (B = F)                          skip_dead_branches
    style-inversion step at F frames  vs  at one frame (clip_length = batch)

All arms run in ONE process and take turns round by round, so the yardstick is the existing step in this very run.  Before timing, the static step's
stylised velocity is compared with the three-branch one on the same inputs.  Device events around `--iters` calls per round.  The frame-forward counts
next to the measured ratios are a WORK count, not a prediction: the one-frame call is launch-bound.  Prints one line per figure and, with --out, writes
them to that file:

    python tools/bench_sd3_static_style.py --out profiles/sd3_static_style.txt
"""
import argparse
import os
import sys
import time

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
    return f"{name}: mean {sum(ms) / len(ms):.2f} ms, min {min(ms):.2f}, max {max(ms):.2f} over {len(ms)} rounds"


def main(a):
    from univst_amd.backbones.video_diffusion_sd3 import pnp_utils
    from univst_amd.backbones.video_diffusion_sd3.models.transformer_3D_model import CustomSD3Transformer2DModel, SD35_MEDIUM_CONFIG
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = "cuda"
    F, hl, T = a.frames, a.latent, 77 + 256
    cfg = dict(SD35_MEDIUM_CONFIG)
    if a.layers:
        cfg.update(num_layers=a.layers, dual_attention_layers=tuple(i for i in cfg["dual_attention_layers"] if i < a.layers))
    torch.manual_seed(33)
    with torch.device(dev):
        model = CustomSD3Transformer2DModel(**cfg)
    model = model.half().requires_grad_(False)
    g = torch.Generator(device=dev).manual_seed(5)
    rn = lambda *sh: torch.randn(*sh, generator=g, device=dev, dtype=torch.float16)          # noqa: E731
    pe, pp = rn(1, T, cfg["joint_attention_dim"]).repeat(3 * F, 1, 1), rn(1, cfg["pooled_projection_dim"]).repeat(3 * F, 1)
    content, frame, lat = rn(F, 16, hl, hl), rn(1, 16, hl, hl), rn(F, 16, hl, hl)
    rep = frame.expand(F, -1, -1, -1).contiguous()
    x3, x2 = torch.cat([content, rep, lat]), torch.cat([content, lat])
    t = torch.tensor(437.0, device=dev)
    lines = [f"SD3 static style bench: {cfg['num_layers']} blocks x {model.inner_dim} wide, F = {F}, {hl} x {hl} latents ({(hl // 2) ** 2} image + {T} text "
             f"tokens per frame), idx {a.idx} inside / {a.idx_out} outside the window, {a.rounds} rounds x {a.iters} calls, {torch.cuda.get_device_name(0)}"]

    def forward(x, idx):
        B = x.shape[0]
        return model(hidden_states=x, timestep=t.expand(B), encoder_hidden_states=pe[:B], pooled_projections=pp[:B], return_dict=False,
                     joint_attention_kwargs={"idx": idx})[0]

    # ---- the style-inversion step: the inversion entry points run the CrossFrameProcessors; a batch is one clip
    procs = {n: pnp_utils.CrossFrameProcessor() for n in model.attn_processors}
    model.set_attn_processor(procs)

    def inversion(x):
        for p in procs.values():
            p.clip_length = x.shape[0]
        return forward(x, 0)

    inv = alternate({f"inversion step F={F}": lambda: inversion(rep), "inversion step F=1": lambda: inversion(frame)}, a.rounds, a.iters, a.warmup)

    # ---- the transfer step
    pnp_utils.register_spatial_attention_pnp(type("P", (), {"transformer": model})())
    for p in model.attn_processors.values():
        p.clip_length = F
    bank = model.style_bank(frame, t.expand(1), pe[:1], pp[:1], a.idx)
    assert bank is not None, f"idx {a.idx} is outside the shift window"
    assert model.style_bank(frame, t.expand(1), pe[:1], pp[:1], a.idx_out) is None, f"idx {a.idx_out} is inside the shift window"

    def static_step():
        model.style_bank(frame, t.expand(1), pe[:1], pp[:1], a.idx, bank)
        return model.forward_static_style(x2, t.expand(2 * F), pe[:2 * F], pp[:2 * F], a.idx, bank)

    def bank_only():
        model.style_bank(frame, t.expand(1), pe[:1], pp[:1], a.idx, bank)

    ref = forward(x3, a.idx)[2 * F:].float()
    got = static_step()[F:].float()
    d = (got - ref).abs().max().item() / ref.abs().max().item()
    r = ((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()
    lines.append(f"static vs three-branch stylised velocity on the same inputs: max |diff| = {d:.3e} of max |v|, rms {r:.3e}")
    lines.append(f"bank: {len(bank.buffers())} attention modules x [{(hl // 2) ** 2}, {2 * model.inner_dim}] fp16 = {bank.nbytes() / 1e9:.3f} GB")
    assert d < 6e-3 and r < 1.5e-3, (d, r)
    names = ("three-branch step inside the window (style repeated)", "static step inside the window (bank + B=2F)", "  of which the bank call",
             "three-branch step outside the window", "two-branch step outside the window (static_style alone)",
             "single-branch step outside the window (skip_dead_branches)")
    step = alternate({names[0]: lambda: forward(x3, a.idx), names[1]: static_step, names[2]: bank_only, names[3]: lambda: forward(x3, a.idx_out),
                      names[4]: lambda: forward(x2, a.idx_out), names[5]: lambda: forward(lat, a.idx_out)}, a.rounds, a.iters, a.warmup)
    for k, v in list(step.items()) + list(inv.items()):
        lines.append(line(k, v))
    torch.cuda.synchronize()
    n = 2 * a.iters
    t0 = time.perf_counter()
    for _ in range(n):
        bank_only()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    lines.append(f"bank call, host clock over {n} calls: enqueue {1e3 * (t1 - t0) / n:.2f} ms per call, until the stream is drained {1e3 * (t2 - t0) / n:.2f} ms per call")
    m = lambda d_, k: sum(d_[k]) / len(d_[k])          # noqa: E731
    spread = lambda v: (max(v) - min(v)) / (sum(v) / len(v))          # noqa: E731
    three_in, static_in, three_out, two_out, one_out = (m(step, names[i]) for i in (0, 1, 3, 4, 5))
    lines.append(f"run-to-run spread inside an arm, (max - min) / mean: three-branch {100 * spread(step[names[0]]):.2f} %, static {100 * spread(step[names[1]]):.2f} %, "
                 f"single-branch {100 * spread(step[names[5]]):.2f} %")
    lines.append(f"inside the window: static / three-branch = {static_in / three_in:.3f} (frame-forwards: {2 * F + 1} / {3 * F} = {(2 * F + 1) / (3 * F):.3f})")
    lines.append(f"outside the window: single-branch / three-branch = {one_out / three_out:.3f} (frame-forwards: {F} / {3 * F} = {1 / 3:.3f}); "
                 f"two-branch / three-branch = {two_out / three_out:.3f} ({2 * F} / {3 * F} = {2 / 3:.3f})")
    n_in = sum(1 for i in range(50) if i <= 0.6 * 50)
    both = n_in * static_in + (50 - n_in) * one_out
    today = n_in * three_in + (50 - n_in) * three_out
    work = (n_in * (2 * F + 1) + (50 - n_in) * F) / (50 * 3 * F)
    lines.append(f"50 steps, eta2 = 0.6 ({n_in} inside, {50 - n_in} outside), transformer time only: both switches {both / 1e3:.2f} s against {today / 1e3:.2f} s = "
                 f"{both / today:.3f} (frame-forwards: {work:.3f}); static_style alone {(n_in * static_in + (50 - n_in) * two_out) / today:.3f}; "
                 f"skip_dead_branches alone {(n_in * three_in + (50 - n_in) * one_out) / today:.3f}")
    lines.append(f"inversion F=1 / F={F} = {m(inv, 'inversion step F=1') / m(inv, f'inversion step F={F}'):.3f} (frame-forwards: 1 / {F} = {1 / F:.3f})")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=16)
    p.add_argument("--latent", type=int, default=128)
    p.add_argument("--layers", type=int, default=0, help="0: the 24 blocks of SD3.5-medium; fewer for a quick look")
    p.add_argument("--idx", type=int, default=10)
    p.add_argument("--idx_out", type=int, default=40)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--iters", type=int, default=2)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--out", type=str, default="")
    main(p.parse_args())
