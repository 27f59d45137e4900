"""GPU: proj_out of a spatial transformer folded into the K loop of the block's second feed-forward linear (``kcat_fold``, csrc/unet.hip
Fwd::transformer; weights composed by univst_linear_compose at finalize):

    Wp (W2 mid + b2 + tb + h3) + bp + x  =  [Wp W2 | Wp] [mid | h3] + (Wp (b2 + tb) + bp) + x

The composition is held to an fp64 rounding bound element by element; the UNet with the fold is held to the project's yardstick for a
regrouping of fp16 roundings: its error against the fp32 oracle is at most twice the error of the unfolded graph in the same test."""
import threading
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_ref, synth_inputs as si  # noqa: E402


def errs(got, ref):
    got, ref = got.float().cpu(), ref.float().cpu()
    e = got - ref
    return e.abs().max().item() / ref.abs().max().item(), (e.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()


def tiny_unet(trivial=True, seed=33):
    from univst_amd.backbones.video_diffusion_sd.models.unet_3d_condition import UNetPseudo3DConditionModel
    cfg = unet_ref.TINY_CONFIG
    sd = unet_ref.synth_state_dict(cfg, seed=seed, trivial_temporal=trivial)
    unet = UNetPseudo3DConditionModel(block_out_channels=cfg["block_out_channels"], cross_attention_dim=cfg["cross_attention_dim"],
                                      attention_head_dim=cfg["attention_head_dim"], norm_num_groups=cfg["norm_num_groups"])
    unet.load_state_dict(sd)
    return unet.half().cuda(), sd, cfg


def tiny_inputs(F_=4, h=16, w=16, D=32):
    x = torch.cat([si.content_latent(50, F_, h, w), si.style_latent(50, F_, h, w), si.content_latent(49, F_, h, w)])
    ctx = si.text_embedding(D).expand(3, -1, -1).contiguous()
    return x.half().cuda(), ctx.half().cuda()


# ------------------------------------------------------------------------------------------------------------------ the composition
# C, K2: the tiny UNet's block; the SD-v1.5 64x64 level; widths that no 256-thread block divides (the bias column lands inside a block / opens a new one)
@pytest.mark.parametrize("Cw,K2,with_tb", [(32, 128, True), (320, 1280, True), (40, 168, False), (248, 8, True)])
def test_linear_compose_holds_the_fp64_rounding_bound(Cw, K2, with_tb):
    """every element: |w - w64| <= 2^-11 |w64| + C 2^-24 sum_j |Wp||W2| (one fp16 rounding of an fp32 sum of C products of fp16 values); the pass-through
    columns are Wp bit for bit; the bias likewise with two more fp32 additions.  NaN guard rows in front of and behind both outputs stay intact."""
    from univst_amd import _native
    g = torch.Generator().manual_seed(Cw * 7 + K2)
    wp = (torch.randn(Cw, Cw, generator=g) / Cw ** 0.5).half().cuda()
    w2 = (torch.randn(Cw, K2, generator=g) / K2 ** 0.5).half().cuda()
    b2, tb, bp = [(0.1 * torch.randn(Cw, generator=g)).half().cuda() for _ in range(3)]
    KT = K2 + Cw
    wbuf = torch.full((Cw + 2, KT), float("nan"), dtype=torch.float16, device="cuda")
    bbuf = torch.full((3, Cw), float("nan"), dtype=torch.float16, device="cuda")
    _native.check(_native.load().univst_linear_compose(wp.data_ptr(), w2.data_ptr(), b2.data_ptr(), tb.data_ptr() if with_tb else None, bp.data_ptr(), Cw, K2,
                                                       wbuf[1].data_ptr(), bbuf[1].data_ptr(), _native.stream_ptr()), "linear_compose")
    torch.cuda.synchronize()
    assert torch.isnan(wbuf[0]).all() and torch.isnan(wbuf[-1]).all() and torch.isnan(bbuf[0]).all() and torch.isnan(bbuf[2]).all(), "guard rows were written"
    w, b = wbuf[1:-1].double(), bbuf[1].double()
    wp64, w264 = wp.double(), w2.double()
    ref = wp64 @ w264
    mag = wp64.abs() @ w264.abs()
    bound = 2.0 ** -11 * ref.abs() + Cw * 2.0 ** -24 * mag
    ratio = ((w[:, :K2] - ref).abs() / bound).max().item()
    assert torch.equal(wbuf[1:-1, K2:], wp), "the pass-through columns must be Wp itself"
    bsum = b2.double() + (tb.double() if with_tb else 0.0)
    bref = wp64 @ bsum + bp.double()
    bmag = wp64.abs() @ bsum.abs() + bp.double().abs()
    bbound = 2.0 ** -11 * bref.abs() + (Cw + 2) * 2.0 ** -24 * bmag
    bratio = ((b - bref).abs() / bbound).max().item()
    print(f"linear_compose C={Cw} K2={K2}: worst error / bound: weight {ratio:.3f}, bias {bratio:.3f}")
    assert ratio <= 1.0 and bratio <= 1.0, (ratio, bratio)
    # the binding allocates its own outputs: same bits
    w_b, b_b = _native.linear_compose(wp, w2, b2, tb if with_tb else None, bp)
    assert torch.equal(w_b, wbuf[1:-1]) and torch.equal(b_b, bbuf[1])


# ------------------------------------------------------------------------------------------------------------------ the UNet graph
def _fold_vs_parent(unet, x, ctx, cases, oracle):
    """cases: (pnp idx, timestep).  Runs option 0 then 3 (both folds asked for; the proj_out fold is the one that exists) on the same handle; asserts
    determinism, that the switch changes the graph,
    e_fold <= 2 e_parent against the oracle, and that the fold did not raise the arena's high-water mark (the mark only grows: equal after = not higher)."""
    from univst_amd import _native
    from univst_amd.backbones.video_diffusion_sd import pnp_utils
    pipe = types.SimpleNamespace(unet=unet)
    pnp_utils.register_spatial_attention_pnp(pipe)
    outs, hw = {}, {}
    for opt in (0, 3):
        unet.set_native_option("kcat_fold", opt)
        for idx, t in cases:
            pnp_utils.register_time(pipe, idx)
            a = unet(x, t, encoder_hidden_states=ctx).sample
            b = unet(x, t, encoder_hidden_states=ctx).sample
            assert torch.equal(a, b), f"kcat_fold={opt}: two runs differ"
            assert torch.isfinite(a.float()).all()
            outs[opt, idx] = a
        hw[opt] = _native.unet_query(unet._native_handle, "arena_high_water")
    print(f"arena high-water: parent {hw[0] / 2**20:.1f} MiB, after the folded runs {hw[3] / 2**20:.1f} MiB")
    assert hw[3] == hw[0], "the fold raised the arena's high-water mark"
    for idx, t in cases:
        assert not torch.equal(outs[0, idx], outs[3, idx]), "the switch did not change the graph"
        ref = oracle(idx, t)
        (m0, r0), (m1, r1) = errs(outs[0, idx], ref), errs(outs[3, idx], ref)
        print(f"pnp idx {idx}: parent max {m0:.3e} rms {r0:.3e} | folded max {m1:.3e} rms {r1:.3e}")
        assert m1 <= 2 * m0 and r1 <= 2 * r0, (idx, m0, r0, m1, r1)


def test_tiny_unet_fold_on_the_128_wide_path_vs_oracle():
    """C = 32 / 64: the K = 5C GEMM (160 / 320: a ragged last k tile, the second source starting inside a k tile) runs on the 128-wide kernel; inside
    (idx 10) and outside (idx 30) the PnP window"""
    unet, sd, cfg = tiny_unet()
    x, ctx = tiny_inputs()

    def oracle(idx, t):
        with torch.no_grad():
            return unet_ref.unet_forward(sd, cfg, x.float().cpu(), t, ctx.float().cpu(), pnp_idx=idx, exact_temporal=False)[0]
    _fold_vs_parent(unet, x, ctx, [(10, 781), (30, 381)], oracle)


def test_sd15_widths_fold_on_the_direct_path_vs_oracle():
    """SD-v1.5 widths, B = 3, F = 4, 64x64 latents: at the 64x64 level (49 152 rows = 192 / 256 tiles) the K = 5C GEMM over the two sources [mid | h3] runs on
    the direct 256x320 tile with the GroupNorm statistics from its epilogue, at the 32x32 and 16x16 levels on the 128-wide kernel, at the 8x8 level with
    split-K.  Oracle: the fp32 restatement with torch ops on the device."""
    from univst_amd import synth
    unet = synth.build_unet(device="cuda", seed=7)
    cfg = unet_ref.SD15_CONFIG
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 4, 4, 64, 64, generator=g).half().cuda()
    ctx = torch.randn(1, 77, 768, generator=g).half().cuda().expand(3, -1, -1).contiguous()
    sd = {k: v.float() for k, v in unet.state_dict().items()}

    def oracle(idx, t):
        with torch.no_grad():
            return unet_ref.unet_forward(sd, cfg, x.float(), t, ctx.float(), pnp_idx=idx, exact_temporal=False)[0]
    _fold_vs_parent(unet, x, ctx, [(12, 741), (40, 181)], oracle)


def test_trained_temporal_attention_keeps_the_two_launches():
    """a block with a TRAINED temporal attention has a non-linear stage between ff.net.2 and proj_out: the graph must take the parent's path there, bit for
    bit.  (The checkpoint also trains every resnet's temporal conv; the conv_shortcut tail that an active temporal conv would have to refuse is not built.)"""
    from univst_amd.backbones.video_diffusion_sd import pnp_utils
    unet, sd, cfg = tiny_unet(trivial=False)
    x, ctx = tiny_inputs()
    pipe = types.SimpleNamespace(unet=unet)
    pnp_utils.register_spatial_attention_pnp(pipe)
    pnp_utils.register_time(pipe, 10)
    unet.set_native_option("kcat_fold", 0)
    want = unet(x, 781, encoder_hidden_states=ctx).sample
    unet.set_native_option("kcat_fold", 3)
    got = unet(x, 781, encoder_hidden_states=ctx).sample
    assert torch.equal(got, want)


def test_frame_sharded_equals_unsharded_with_the_fold():
    """two ranks (host threads on one GPU) with the fold on reproduce the unsharded folded forward: the chain is row-local, only summation orders differ"""
    from univst_amd.backbones.video_diffusion_sd import pnp_utils
    from univst_amd.parallel import FrameShard, ThreadLoopbackComm
    F_, h, w, world = 4, 16, 16, 2
    x, ctx = tiny_inputs(F_, h, w)
    ref_unet, _, _ = tiny_unet()
    ref_unet.set_native_option("kcat_fold", 3)
    ref_pipe = types.SimpleNamespace(unet=ref_unet)
    pnp_utils.register_spatial_attention_pnp(ref_pipe)
    ref = {}
    for idx, t in ((10, 781), (30, 381)):
        pnp_utils.register_time(ref_pipe, idx)
        ref[idx] = ref_unet(x, t, encoder_hidden_states=ctx).sample
    shared = ThreadLoopbackComm.Shared(world)
    results, errors = {}, []

    def run(rank):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                unet, _, _ = tiny_unet()
                unet.set_native_option("kcat_fold", 3)
                pipe = types.SimpleNamespace(unet=unet)
                pnp_utils.register_spatial_attention_pnp(pipe)
                sh = FrameShard(rank, world, F_, comm=ThreadLoopbackComm(shared, rank))
                sh.attach(unet, max_tokens=h * w)
                xl = sh.slice_frames(x)
                out = {}
                for idx, t in ((10, 781), (30, 381)):
                    pnp_utils.register_time(pipe, idx)
                    out[idx] = unet(xl, t, encoder_hidden_states=ctx).sample
                torch.cuda.current_stream().synchronize()
                results[rank] = out
        except Exception:
            import traceback
            errors.append(traceback.format_exc())
            shared.barrier.abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not errors, errors[0]
    for idx in (10, 30):
        got = torch.cat([results[r][idx] for r in range(world)], dim=2)
        mx, rms = errs(got, ref[idx])
        assert mx < 5e-3, (idx, mx, rms)


def test_option_values():
    """0 .. 3 as include/univst.h states them: bit 0 = proj_out fold; bit 1 (conv_shortcut tail) is accepted and selects nothing yet, so 1 and 3 run the
    same graph, as do 0 and 2 (checked here only as 'runs and is finite': what 2 computes changes when the tail is built)"""
    unet, _, _ = tiny_unet()
    x, ctx = tiny_inputs()
    outs = {}
    for v in (0, 1, 2, 3):
        unet.set_native_option("kcat_fold", v)
        outs[v] = unet(x[:1], 301, encoder_hidden_states=ctx[:1]).sample
        assert torch.isfinite(outs[v].float()).all()
    assert torch.equal(outs[1], outs[3]) and not torch.equal(outs[0], outs[1])
    for bad in (-1, 4):
        with pytest.raises(RuntimeError, match="kcat_fold"):
            unet.set_native_option("kcat_fold", bad)
    unet.set_native_option("kcat_fold", 3)
