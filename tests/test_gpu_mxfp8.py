"""GPU: the MX-fp8 q | k | v path (csrc/mxfp8.hip, univst_sd3_joint_attention_mx, CustomSD3Transformer2DModel.set_qkv_dtype).

The quantiser is held to tests/mxfp8_ref.py byte for byte.  The block-scaled MFMA linear is held to exact values first (operands on which quantisation is
the identity and every partial sum is exact in fp32, so the output must equal the float64 product rounded once to fp16, bit for bit: this is what catches
a wrong operand lane map, scale byte or opsel), then to the error of the fp16 linear on the same dequantised operands.  The attention op and the model are
compared with the fp16 code on fake-quantised inputs and weights: both sides compute the same products and differ only in the order of summation."""
import os
import types

import pytest
import torch

import mxfp8_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sd3_joint_attention_fp16_parent.pt")


@pytest.fixture(scope="module")
def nat():
    from univst_amd import _native
    _native.load()
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _native


def errs(got, ref):
    got, ref = got.float().cpu(), ref.float().cpu()
    e = got - ref
    return e.abs().max().item() / ref.abs().max().item(), (e.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()


# --------------------------------------------------------------------------- quantise
def _quant_input(rows, K, variant, seed):
    """normal draws at scales 1e-3, 1, 1e3 (one per 32-block, in turn), and three special blocks placed at the first, middle and last block in an order
    that `variant` rotates (a one-block input takes one special per variant): an all-zero block, a block whose maximum is a power of two, a block whose
    maximum is the fp16 value just above 448 * 2^e."""
    g = torch.Generator().manual_seed(seed)
    nb = K // 32
    x = torch.randn(rows, nb, 32, generator=g, dtype=torch.float64)
    scale = torch.tensor([1e-3, 1.0, 1e3], dtype=torch.float64)[(torch.arange(rows * nb) % 3).reshape(rows, nb)]
    x = (x * scale.unsqueeze(2)).to(torch.float16).to(torch.float64)
    n = rows * nb
    spots = sorted({0, n // 2, n - 1})
    for i, at in enumerate(spots):
        r, b = divmod(at, nb)
        kind = (i + variant) % 3
        if kind == 0:
            x[r, b] = 0.0
        elif kind == 1:
            x[r, b] = x[r, b].clamp(-1, 1) * 2.0 ** -3
            x[r, b, 7] = -(2.0 ** -2)                                     # scales to exactly 256
        else:
            x[r, b] = x[r, b].clamp(-1, 1) * 2.0 ** 2
            x[r, b, 31] = (448.0 + 0.25) * 2.0 ** -3                      # the next fp16 above 448 * 2^-3: takes the +1 step
    return x.reshape(rows, K).to(torch.float16)


@pytest.mark.parametrize("K", [32, 128, 384])
@pytest.mark.parametrize("rows", [1, 5, 257])
def test_quantize_bytes_and_scale_bytes_equal_the_restatement(nat, rows, K):
    for variant in range(3):
        x = _quant_input(rows, K, variant, 100 * rows + K + variant)
        buf = torch.full((rows, K + 8), 7.0, dtype=torch.float16, device="cuda")          # ldx = K + 8 > K
        buf[:, :K] = x.cuda()
        q, s = nat.mxfp8_quantize(buf[:, :K])
        qr, sr = R.quantize(x)
        assert q.shape == (rows, K) and s.shape == (rows, K // 32) and q.dtype == s.dtype == torch.uint8
        assert torch.equal(s.cpu(), sr), (variant, (s.cpu() != sr).nonzero()[:4])
        assert torch.equal(q.cpu(), qr), (variant, (q.cpu() != qr).nonzero()[:4])


# --------------------------------------------------------------------------- the linear: exact values
def _exact_operand(rows, K, seed):
    """{-2 .. 2} * 2^s with s in {-1, 0, 1} drawn per row AND per 32-block -> (fp16 values, bytes, scale bytes); quantisation is the identity on them"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-2, 3, (rows, K // 32, 32), generator=g).to(torch.float64)
    s = torch.randint(-1, 2, (rows, K // 32, 1), generator=g).to(torch.float64)
    x = (v * torch.pow(2.0, s)).reshape(rows, K).to(torch.float16)
    q, sc = R.quantize(x)
    assert torch.equal(R.dequantize(q, sc), x.to(torch.float64))
    return x, q, sc


_EXACT_W = {}


def _exact_weight(N, K):
    if (N, K) not in _EXACT_W:
        _EXACT_W[(N, K)] = _exact_operand(N, K, 7000 + N + K)
    return _EXACT_W[(N, K)]


@pytest.mark.parametrize("K", [128, 256, 1536])
@pytest.mark.parametrize("N", [16, 80, 320])
@pytest.mark.parametrize("M", [1, 17, 255, 513])
def test_linear_mxfp8_exact_values_bit_for_bit(nat, M, N, K):
    """products are multiples of 1/4 below 16 in magnitude and so are the bias values: every partial sum of up to 1536 of them, in any order, is exact in
    fp32 (|sum| * 4 < 2^24).  So Y is the float64 product (+ bias) rounded once to fp16.  513 x 320 is 5 x 3 tiles; the padding columns of Y stay."""
    x, xq, xs = _exact_operand(M, K, 31 * M + N + K)
    w, wq, ws = _exact_weight(N, K)
    bias = (torch.randint(-12, 13, (N,), generator=torch.Generator().manual_seed(N)).to(torch.float64) / 4).to(torch.float16)
    prod = x.to(torch.float64) @ w.to(torch.float64).T
    if K == 256:        # the claim above, checked on the CPU: an fp32 accumulation of these products loses nothing
        assert torch.equal((x.float() @ w.float().T).to(torch.float64), prod)
    dev = [t.cuda() for t in (xq, xs, wq, ws)]
    for b in (None, bias):
        want = (prod + (0 if b is None else b.to(torch.float64))).to(torch.float16)
        out = torch.full((M, N + 8), -3.0, dtype=torch.float16, device="cuda")            # ldy = N + 8 > N
        nat.linear_mxfp8(*dev, bias=None if b is None else b.cuda(), out=out)
        got = out.cpu()
        bad = (got[:, :N] != want).nonzero()
        assert bad.numel() == 0, (b is not None, bad.shape[0], bad[:6].tolist(), got[:, :N][tuple(bad[0])].item(), want[tuple(bad[0])].item())
        assert bool((got[:, N:] == -3.0).all()), "the linear wrote past column N"


def test_linear_mxfp8_random_operands_vs_the_fp16_linear(nat):
    """truth: the float64 product of the DEQUANTISED operands.  The fp16 linear on those same (fp16-exact) operands computes the same products with the
    same fp32 accumulation and one rounding; the MX linear may not be worse than twice that in the maximum norm (the convention of
    test_gpu_animatediff.py)."""
    g = torch.Generator().manual_seed(17)
    M, N, K = 300, 192, 1536
    x = torch.randn(M, K, generator=g).to(torch.float16)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.float16)
    bias = (0.1 * torch.randn(N, generator=g)).to(torch.float16)
    xq, xs = nat.mxfp8_quantize(x.cuda())
    wq, ws = nat.mxfp8_quantize(w.cuda())
    xd, wd = R.dequantize(xq.cpu(), xs.cpu()), R.dequantize(wq.cpu(), ws.cpu())
    assert torch.equal(xq.cpu(), R.quantize(x)[0]) and torch.equal(wq.cpu(), R.quantize(w)[0])
    truth = xd @ wd.T + bias.to(torch.float64)
    y_mx = nat.linear_mxfp8(xq, xs, wq, ws, bias=bias.cuda())
    y_ref = nat.linear(xd.to(torch.float16).cuda(), wd.to(torch.float16).cuda(), bias=bias.cuda())
    e_mx = (y_mx.cpu().to(torch.float64) - truth).abs().max().item()
    e_ref = (y_ref.cpu().to(torch.float64) - truth).abs().max().item()
    print(f"\nmxfp8 linear {M}x{N}x{K}: max |error| {e_mx:.3e}, fp16 linear on the dequantised operands {e_ref:.3e}, max |truth| {truth.abs().max().item():.3f}")
    assert e_ref > 0 and e_mx <= 2 * e_ref, (e_mx, e_ref)


# --------------------------------------------------------------------------- the attention op
def _attn_case(seed=41, C=128, heads=2, N=64, Nt=8, B=6):
    g = torch.Generator().manual_seed(seed)
    P = {}
    for nm in ("to_q", "to_k", "to_v", "add_q_proj", "add_k_proj", "add_v_proj", "to_out.0", "to_add_out"):
        P[nm + ".weight"] = (torch.randn(C, C, generator=g) / C ** 0.5).half()
        P[nm + ".bias"] = (0.1 * torch.randn(C, generator=g)).half()
    for nm in ("norm_q", "norm_k", "norm_added_q", "norm_added_k"):
        P[nm + ".weight"] = (1.0 + 0.2 * torch.randn(C // heads, generator=g)).half()
    hid = torch.randn(B, N, C, generator=g).half()
    hid[2 * B // 3:] = hid[2 * B // 3:] * 1.4 - 0.2
    enc = torch.randn(B, Nt, C, generator=g).half()
    return P, hid, enc


def _fq3(x):
    return R.fake_quantize(x.reshape(-1, x.shape[-1])).reshape(x.shape)


@pytest.mark.parametrize("B,N,Nt,clip", [(6, 64, 8, 2), (3, 25, 7, 1)])
@pytest.mark.parametrize("shift", [False, True])
def test_attention_mx_agrees_with_the_fp16_entry_on_fake_quantised_operands(nat, shift, B, N, Nt, clip):
    """B = 6 (three branches x two frames), 64 image + 8 text tokens, 2 heads x 64, q / k RMS norms, clip_length 2; and B = 3 with 25 + 7 tokens, where
    B N and B Nt are odd: the scale bytes of the image rows (75 x 4) then end off every 8- and 16-byte boundary, and the parts of the op's scratch
    behind them must still start aligned.  Rows and q | k | v weights are made MX-representable on the host, so the fp16 entry and the MX entry
    multiply the same numbers; bounds of test_gpu_sd3.py against its oracle."""
    P, hid, enc = _attn_case(N=N, Nt=Nt, B=B)
    hid, enc = _fq3(hid), _fq3(enc)
    for nm in ("to_q", "to_k", "to_v", "add_q_proj", "add_k_proj", "add_v_proj"):
        P[nm + ".weight"] = R.fake_quantize(P[nm + ".weight"])
    params = nat.Sd3AttnParams(P, torch.device("cuda"))
    kw = dict(clip_length=clip, shift=shift, idx=12, eta1=0.0, eta2=0.6)
    r_img, r_txt = nat.sd3_joint_attention(params, hid.cuda(), enc.cuda(), 2, **kw)
    nat.profile_enable(True)
    try:
        m_img, m_txt = nat.sd3_joint_attention(params, hid.cuda(), enc.cuda(), 2, qkv_dtype="mxfp8", **kw)
        torch.cuda.synchronize()
        syms = [s for v in nat.profile_symbols().values() for s in v]
    finally:
        nat.profile_enable(False)
        nat.profile_collect()
    assert any("linear_mxfp8_kernel" in s for s in syms), syms
    # the cached quantised weights are the restatement's bytes of the fused fp16 weights
    fused = torch.cat([P["to_q.weight"], P["to_k.weight"], P["to_v.weight"]])
    assert torch.equal(params.mx()["qkv"].cpu(), R.quantize(fused)[0]) and torch.equal(params.mx()["qkv_scale"].cpu(), R.quantize(fused)[1])
    for got, ref in ((m_img, r_img), (m_txt, r_txt)):
        mx, rms = errs(got, ref)
        print(f"\nattention mx vs fp16 on fake-quantised operands (B={B} N={N} shift={shift}): max {mx:.2e} rms {rms:.2e}")
        assert mx < 4e-3 and rms < 1e-3, (shift, mx, rms)
    # no text stream: the image-only call of attn2
    P2 = {k: v for k, v in P.items() if not k.startswith(("add_", "norm_added", "to_add_out"))}
    p2 = nat.Sd3AttnParams(P2, torch.device("cuda"))
    mx, rms = errs(nat.sd3_joint_attention(p2, hid.cuda(), None, 2, qkv_dtype="mxfp8", **kw), nat.sd3_joint_attention(p2, hid.cuda(), None, 2, **kw))
    assert mx < 4e-3 and rms < 1e-3, (shift, mx, rms)


def test_fp16_entry_reproduces_the_bits_recorded_before_the_body_was_shared(nat):
    """tests/golden/sd3_joint_attention_fp16_parent.pt: inputs, parameters and the outputs of univst_sd3_joint_attention recorded on the commit before
    the MX entry existed (shift off and on, text stream on).  The entry is now the shared body with mx == NULL: its launches, and so its bits, are the same."""
    g = torch.load(GOLDEN, weights_only=True)
    params = nat.Sd3AttnParams(g["params"], torch.device("cuda"))
    for shift in (False, True):
        img, txt = nat.sd3_joint_attention(params, g["hidden"].cuda(), g["enc"].cuda(), 2, clip_length=2, shift=shift, idx=12, eta1=0.0, eta2=0.6)
        assert torch.equal(img.cpu(), g[f"img_shift{int(shift)}"]) and torch.equal(txt.cpu(), g[f"txt_shift{int(shift)}"])


def test_attention_mx_refusals(nat):
    from univst_amd.parallel import EmulatedIpcComm
    # an input width that is no multiple of 128
    g = torch.Generator().manual_seed(3)
    P = {f"{n}.weight": torch.randn(64, 64, generator=g).half() for n in ("to_q", "to_k", "to_v", "to_out.0")}
    hid = torch.randn(6, 16, 64, generator=g).half().cuda()
    with pytest.raises(RuntimeError, match="multiple of 128"):
        nat.sd3_joint_attention(P, hid, None, 1, clip_length=2, qkv_dtype="mxfp8")
    mxw = nat.Sd3MxWeights(hid.data_ptr(), hid.data_ptr(), None, None)           # and the library's own refusal, past the binding's
    p = nat.Sd3AttnParams(P, hid.device)
    w = nat.Sd3AttnWeights(**{k: (p[k].data_ptr() if k in p else None) for k in nat.Sd3AttnWeights._NAMES})
    out = torch.empty_like(hid)
    import ctypes as C
    rc = nat.load().univst_sd3_joint_attention_mx(C.byref(w), hid.data_ptr(), None, 6, 16, 0, 64, 1, 64, 2, 0, 0.0, 1e-6, out.data_ptr(), None, None, None,
                                                  nat.stream_ptr(), C.byref(mxw))
    assert rc == -1 and b"Cin=64 must be a multiple of 128" in nat.load().univst_last_error()
    # a communicator of world > 1: unsupported, named
    P, hid, enc = _attn_case()
    comm = EmulatedIpcComm(1, 2, 1 << 20, wire_gbps=50.0, latency_us=2.0)
    try:
        with pytest.raises(RuntimeError, match=r"code -3.*frame shard \(world = 2\) is not built: the receiver-side projection of the halo rows"):
            nat.sd3_joint_attention(P, hid.cuda(), enc.cuda(), 2, clip_length=2, comm=comm.ptr, qkv_dtype="mxfp8")
    finally:
        comm.close()


# --------------------------------------------------------------------------- the model
def _tiny_sd3(seed=11):
    """a two-layer MM-DiT of width 128 (2 heads x 64), the first block with dual attention, the last one context-pre-only — built as test_gpu_sd3.py does"""
    from univst_amd.backbones.video_diffusion_sd3.models.transformer_3D_model import CustomSD3Transformer2DModel
    torch.manual_seed(seed)
    m = CustomSD3Transformer2DModel(sample_size=32, patch_size=2, in_channels=16, num_layers=2, attention_head_dim=64, num_attention_heads=2,
                                    joint_attention_dim=64, caption_projection_dim=128, pooled_projection_dim=32, out_channels=16, pos_embed_max_size=24,
                                    dual_attention_layers=(0,), qk_norm="rms_norm")
    for n, p in m.named_parameters():
        if n.endswith("norm_q.weight") or n.endswith("norm_k.weight") or "norm_added" in n:
            p.data = 1.0 + 0.2 * torch.randn_like(p)
    return m.half().cuda()


class _Shadow(torch.nn.Module):
    """what the processors read of an attention module, with other parameters behind it"""

    def __init__(self, attn, params):
        super().__init__()
        self.heads, self.norm_q, self._p = attn.heads, types.SimpleNamespace(eps=1e-6), params

    def state_dict(self, *a, **k):
        return self._p


def _fake_quant_processor(nat, base):
    """`base` (a processor class of pnp_utils) on fp16 kernels, with what the MX path quantises — the op's input rows and the q | k | v weights — replaced
    by their dequantised MX values (quantised by the kernel that the first test holds to the restatement, dequantised here in torch)"""
    table = R.e4m3_decode_table().cuda()

    def fq(x):
        q, s = nat.mxfp8_quantize(x.reshape(-1, x.shape[-1]).contiguous())
        v = table[q.long()].reshape(q.shape[0], -1, 32) * torch.pow(2.0, s.to(torch.float64) - 127).unsqueeze(2)
        return v.reshape(x.shape).to(torch.float16)

    class FakeQuant(base):
        def __call__(self, attn, hidden_states, encoder_hidden_states=None, *a, **k):
            sh = attn.__dict__.get("_fq_shadow")
            if sh is None:
                sd = {n: (fq(t) if n.split(".")[0] in ("to_q", "to_k", "to_v", "add_q_proj", "add_k_proj", "add_v_proj") and n.endswith("weight") else t)
                      for n, t in attn.state_dict().items()}
                sh = attn.__dict__["_fq_shadow"] = _Shadow(attn, sd)
            return super().__call__(sh, fq(hidden_states), None if encoder_hidden_states is None else fq(encoder_hidden_states), *a, **k)
    return FakeQuant


def test_model_switch_runs_the_mx_kernel_and_matches_the_fake_quantised_fp16_model(nat):
    from univst_amd.backbones.video_diffusion_sd3 import pnp_utils
    m = _tiny_sd3()
    procs = {n: pnp_utils.AttentionShiftProcessor(0.0, 0.6) for n in m.attn_processors}
    for p in procs.values():
        p.clip_length = 2                                                # three branches x two frames
    m.set_attn_processor(procs)
    g = torch.Generator().manual_seed(5)
    lat, enc, pooled = torch.randn(6, 16, 16, 16, generator=g).half().cuda(), torch.randn(6, 5, 64, generator=g).half().cuda(), torch.randn(6, 32, generator=g).half().cuda()
    t = torch.tensor([437.0]).cuda().expand(6)

    def run():
        return m(hidden_states=lat, timestep=t, encoder_hidden_states=enc, pooled_projections=pooled, return_dict=False, joint_attention_kwargs={"idx": 10})[0]

    plain = run()                                                        # idx 10 is inside the shift window [0, 30]
    m.set_qkv_dtype("mxfp8")
    nat.profile_enable(True)
    try:
        mx_out = run()
        torch.cuda.synchronize()
        syms = [s for v in nat.profile_symbols().values() for s in v]
    finally:
        nat.profile_enable(False)
        nat.profile_collect()
    assert any("linear_mxfp8_kernel" in s for s in syms), syms
    m.set_qkv_dtype("fp16")
    assert torch.equal(run(), plain), "switching back to fp16 does not reproduce the fp16 bits"
    FQ = _fake_quant_processor(nat, pnp_utils.AttentionShiftProcessor)
    fqp = {n: FQ(0.0, 0.6) for n in m.attn_processors}
    for p in fqp.values():
        p.clip_length = 2
    m.set_attn_processor(fqp)
    fake = run()
    mx, rms = errs(mx_out, fake)
    dmx, drms = errs(mx_out, plain)
    print(f"\ntiny MM-DiT, mxfp8 vs fake-quantised fp16: max {mx:.2e} rms {rms:.2e};  mxfp8 vs plain fp16 (recorded, not bounded): max {dmx:.3e} rms {drms:.3e}")
    assert torch.isfinite(mx_out.float()).all() and not torch.equal(fake, plain)
    assert mx < 4e-3 and rms < 1e-3, (mx, rms)
