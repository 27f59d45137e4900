"""GPU: the native T5 encoder (univst_amd/text.py NativeT5Encoder, csrc/t5.hip) against the restatement tests/t5_ref.py (held to transformers by
tests/test_t5_ref.py): the bidirectional attention operator with its relative-position bias against an fp64 softmax with a derived bound, memory
beyond an element's rows that must never reach its output, the whole encoder against the fp64 restatement with the torch-fp16 restatement's own error
as the yardstick, a residual stream beyond the fp16 range, the wrapper's contract and the pipeline hook."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_ref as CR  # noqa: E402
import t5_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
EPS16 = 2.0 ** -11          # unit roundoff of fp16
TW = 1023                   # bias table entries per head: delta + 511


# ------------------------------------------------------------------------------------------------------------ the attention operator
def t5_attention(qkv, table, B, S, heads):
    from univst_amd import _native
    out = torch.empty(max(B * S, 1), heads * 64, device=qkv.device, dtype=torch.float16)
    _native.check(_native.load().univst_t5_attention(_native.ptr(qkv), _native.ptr(table), B, S, heads, _native.ptr(out), _native.stream_ptr()), "t5_attention")
    return out[:B * S]


def make_qkv(B, S, heads, seed):
    """q | k | v rows [B*S, 3*heads*64] fp16 (T5 applies no scale: the scores ARE q.k, sigma_q sigma_k sqrt(64) = 3) and a bias table [heads][1023]
    of fp16-representable values with a standard deviation of 2"""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * S, 3, heads * 64, generator=g)
    qkv[:, :2] *= (3.0 / 8.0) ** 0.5
    table = (2.0 * torch.randn(heads, TW, generator=g)).half().float()
    return qkv.reshape(B * S, 3 * heads * 64).half(), table


def attention_ref64(qkv, table, B, S, heads):
    """fp64 softmax attention on the same fp16 inputs -> (o [B*S, heads*64], vmax = max over all S keys of |v[j, d]|, the biased scores)"""
    x = qkv.double().view(B, S, 3, heads, 64).permute(2, 0, 3, 1, 4)      # [3][B][heads][S][64]
    q, k, v = x[0], x[1], x[2]
    pos = torch.arange(S, device=qkv.device)
    sc = q @ k.transpose(-1, -2) + table.double()[:, (pos[None, :] - pos[:, None]) + 511]
    o = torch.softmax(sc, dim=-1) @ v
    back = lambda t: t.permute(0, 2, 1, 3).reshape(B * S, heads * 64)      # noqa: E731
    return back(o), back(v.abs().amax(dim=2, keepdim=True).expand_as(v)), sc


def check_attention(B, S, heads, seed):
    qkv, table = (t.cuda() for t in make_qkv(B, S, heads, seed))
    got = t5_attention(qkv, table, B, S, heads).double()
    want, vmax, sc = attention_ref64(qkv, table, B, S, heads)
    frac = ((got - want).abs() / (4 * EPS16 * vmax).clamp(min=1e-30)).max().item()
    print(f"S={S} heads={heads} B={B}: score std {sc.std().item() if S > 1 else 0.0:.2f}, worst |o - o64| / bound = {frac:.3f}")
    assert torch.isfinite(got).all() and frac <= 1.0


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("S", [1, 15, 16, 17, 33, 64, 65, 140, 256, 257, 512])
def test_attention_operator(S, heads, B):
    """every output element is a convex combination of the V rows, so |o - o64| <= 4 x 2^-11 x max_j |v_j| elementwise: one unit roundoff each for
    the fp16 rounding of P, the fp16 rounding of the output and the exp2 / fp32 accumulation error, and one spare"""
    check_attention(B, S, heads, seed=S * 100 + heads * 10 + B)


def test_attention_on_a_grid_of_more_than_two_rounds():
    """3 x 64 x 4 = 768 blocks: more than two rounds of the 256 compute units, under the same bound"""
    check_attention(3, 256, 64, seed=7)


@pytest.mark.parametrize("S", [17, 65])
def test_padding_and_neighbours_never_leak(S):
    """batch element 1's q | k | v rows set to +-6e4, then to NaN: element 0's output is bit-identical to the clean run (its blocks load nothing
    beyond their own S rows; the kernel's pad keys S .. are exact zeros with probability exactly 0), and element 1 shows the NaN"""
    B, heads = 2, 3
    C = heads * 64
    qkv, table = (t.cuda() for t in make_qkv(B, S, heads, seed=S))
    clean = t5_attention(qkv, table, B, S, heads).view(B, S, C)
    assert torch.isfinite(clean).all()
    g = torch.Generator().manual_seed(1)
    big = (torch.randint(0, 2, (S, 3 * C), generator=g).float() * 2 - 1).mul(6e4).half().cuda()
    for name, poison in (("+-6e4", big), ("NaN", torch.full_like(big, float("nan")))):
        x = qkv.clone().view(B, S, 3 * C)
        x[1] = poison
        out = t5_attention(x.view(B * S, 3 * C), table, B, S, heads).view(B, S, C)
        assert torch.equal(out[0].view(torch.int16), clean[0].view(torch.int16)), f"{name} in element 1 reached element 0"
        if name == "NaN":
            assert torch.isnan(out[1]).all(), "the poisoned element itself must see the poison (the test would otherwise prove nothing)"


def test_attention_refuses_bad_shapes():
    qkv, table = (t.cuda() for t in make_qkv(1, 8, 1, 0))
    with pytest.raises(RuntimeError, match="1 <= S <= 512"):
        t5_attention(qkv, table, 1, 0, 1)
    with pytest.raises(RuntimeError, match="1 <= S <= 512"):
        t5_attention(qkv, table, 1, 513, 1)
    flat = torch.zeros(8 * 192 + 8, device="cuda", dtype=torch.float16)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        t5_attention(flat[1:1 + 8 * 192], table, 1, 8, 1)


# ------------------------------------------------------------------------------------------------------------ the whole encoder
CONFIGS = {
    "tiny": (R.Cfg(vocab_size=96, d_model=64, d_ff=128, num_layers=2, num_heads=2), 140),
    "mid": (R.Cfg(vocab_size=512, d_model=512, d_ff=1024, num_layers=2, num_heads=8), 77),
    # split-K at K = 10240 and the 4096-wide RMSNorm
    "xxl-width": (R.Cfg(vocab_size=512, d_model=4096, d_ff=10240, num_layers=1, num_heads=64), 256),
}
# a residual stream beyond the fp16 range.  The embedding table is fp16 in the handle, so its entries fill that range (std 1.6e4, bounded by
# 6e4) and the stream passes it through what the sub-layers add: o and wo scaled to outputs of std ~1.2e4 (largest 5e4: finite as fp16 rows), so |x| reaches about 1e5
LARGE = dict(embed_scale=1.6e4, embed_clamp=6e4, out_gain=1.2e4)
_CASES = {}


def case(name, large=False):
    """weights, ids, the native handle and the restatement in fp64 and in torch fp16 (both on the GPU), built once per config"""
    key = (name, large)
    if key not in _CASES:
        from univst_amd.text import NativeT5Encoder
        cfg, S = CONFIGS[name]
        sd = R.random_state_dict(cfg, seed=len(name), **(LARGE if large else {}))
        ids = R.make_ids(cfg, 2, S, seed=3).cuda()
        with torch.no_grad():
            ref64 = R.forward(sd, cfg, ids, dtype=torch.float64)
            ref16 = R.forward(sd, cfg, ids, dtype=torch.float16)
            ref16_32 = R.forward(sd, cfg, ids, dtype=torch.float16, residual_dtype=torch.float32) if large else None
        enc = NativeT5Encoder.from_state_dict(sd, R.hf_config(cfg))
        _CASES[key] = types.SimpleNamespace(cfg=cfg, sd=sd, ids=ids, ref64=ref64, ref16=ref16, ref16_32=ref16_32, enc=enc)
    return _CASES[key]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_encoder_against_fp64_restatement(name):
    """yardstick: the reference runs this module as text_encoder_3.to(fp16).cuda(), i.e. the restatement in torch fp16 on this GPU, whose distance
    to the fp64 restatement is e_ref.  The native encoder must stay within 2 x e_ref (the factor covers a different but equally valid accumulation
    order: split-K, online softmax)."""
    c = case(name)
    got = c.enc(c.ids)[0]
    assert got.shape == c.ref64.shape and got.dtype == torch.float16
    e_nat, e_ref = (got.double() - c.ref64).abs().max().item(), (c.ref16.double() - c.ref64).abs().max().item()
    print(f"{name}: e_native {e_nat:.3e}, e_ref (torch fp16) {e_ref:.3e}, ratio {e_nat / e_ref:.2f}, max|want| {c.ref64.abs().max().item():.2f}")
    assert torch.isfinite(got).all() and e_nat <= 2 * e_ref


@pytest.mark.parametrize("name", ["tiny", "mid"])
def test_large_residual_stream(name):
    """|x| reaches about 1e5, past fp16: the all-fp16 restatement is not finite on this input, the native encoder (fp32 stream) is, and it stays
    within 2 x the error of the fp16 restatement with an fp32 residual stream"""
    c = case(name, large=True)
    xs = []
    R.forward(c.sd, c.cfg, c.ids, dtype=torch.float64, stream_out=xs)
    xmax = max(x.abs().max().item() for x in xs)
    got = c.enc(c.ids)[0]
    e_nat, e_ref = (got.double() - c.ref64).abs().max().item(), (c.ref16_32.double() - c.ref64).abs().max().item()
    print(f"{name} (large stream): max|x| {xmax:.3e}, e_native {e_nat:.3e}, e_ref (torch fp16, fp32 residual) {e_ref:.3e}, ratio {e_nat / e_ref:.2f}")
    assert xmax > 65504 and not torch.isfinite(c.ref16).all(), "the case must overflow an fp16 stream to prove anything"
    assert torch.isfinite(c.ref16_32).all() and torch.isfinite(got).all() and e_nat <= 2 * e_ref


# ------------------------------------------------------------------------------------------------------------ the wrapper's contract
def test_wrapper_contract():
    from univst_amd.text import NativeT5Encoder
    c = case("tiny")
    enc = c.enc
    o = enc(c.ids)
    assert o[0] is o.last_hidden_state and len(o) == 1 and tuple(o[0].shape) == (2, 140, 64) and o[0].dtype == torch.float16
    assert torch.equal(enc(c.ids, return_dict=False)[0], o[0])
    assert enc.dtype == torch.float16 and enc.device.type == "cuda" and enc.config.d_model == 64 and enc._h
    assert enc.to(torch.float16) is enc and enc.cuda() is enc and enc.requires_grad_(False) is enc and enc.eval() is enc
    with pytest.raises(RuntimeError, match="runs on the GPU only"):
        enc(c.ids.cpu())
    mask = torch.ones_like(c.ids)
    assert torch.equal(enc(c.ids, attention_mask=mask)[0], o[0])
    mask[0, 50:] = 0
    with pytest.raises(NotImplementedError):
        enc(c.ids, attention_mask=mask)
    with pytest.raises(NotImplementedError):
        enc(c.ids, output_hidden_states=True)
    for bad_id in (c.cfg.vocab_size, -1):
        bad = c.ids.clone()
        bad[1, 3] = bad_id
        with pytest.raises(IndexError):
            enc(bad)
    with pytest.raises(ValueError, match="1..512"):
        enc(torch.zeros(1, 513, dtype=torch.int64, device="cuda"))
    # the tied embedding under its other name, and both names at once
    alt = {("encoder.embed_tokens.weight" if k == "shared.weight" else k): v for k, v in c.sd.items()}
    assert torch.equal(NativeT5Encoder.from_state_dict(alt, R.hf_config(c.cfg))(c.ids)[0], o[0])
    both = NativeT5Encoder.from_state_dict({**alt, **c.sd}, R.hf_config(c.cfg))
    assert torch.equal(both(c.ids)[0], o[0]) and both.query("weight_bytes") == enc.query("weight_bytes") > 0
    # fp32 upload == fp16 upload of the same values
    half = NativeT5Encoder.from_state_dict({k: v.half() for k, v in c.sd.items()}, R.hf_config(c.cfg))
    assert torch.equal(half(c.ids)[0], o[0])


def test_sizes_in_turn_leave_the_arena_alone():
    """(2, 256), then (1, 17), then (2, 256) again: the first and third results are bit-identical and the third call does not move the high-water mark"""
    c = case("mid")
    a_ids, b_ids = R.make_ids(c.cfg, 2, 256, seed=11).cuda(), R.make_ids(c.cfg, 1, 17, seed=12).cuda()
    first = c.enc(a_ids)[0].clone()
    small = c.enc(b_ids)[0].clone()
    hw = c.enc.arena_high_water()
    third = c.enc(a_ids)[0]
    assert hw > 0 and c.enc.arena_high_water() == hw and torch.equal(first, third)
    assert torch.equal(small, c.enc(b_ids)[0]) and torch.isfinite(small).all()
    # the split-K partials of the K = 10240 linear live in the arena too
    wide = case("xxl-width")
    wide.enc(wide.ids)
    assert 0 < wide.enc.query("splitk_bytes") < wide.enc.arena_high_water()


def test_create_and_finalize_refuse_what_is_not_supported():
    from univst_amd.text import NativeT5Encoder
    cfg, _ = CONFIGS["tiny"]
    with pytest.raises(RuntimeError, match="d_kv 32"):
        NativeT5Encoder.from_state_dict({}, dict(R.hf_config(cfg), d_kv=32))
    with pytest.raises(RuntimeError, match="d_model 60"):
        NativeT5Encoder.from_state_dict({}, dict(R.hf_config(cfg), d_model=60))
    with pytest.raises(ValueError, match="feed_forward_proj"):
        NativeT5Encoder.from_state_dict({}, dict(R.hf_config(cfg), feed_forward_proj="relu"))
    sd = dict(case("tiny").sd)
    del sd["encoder.block.1.layer.1.DenseReluDense.wi_1.weight"]
    with pytest.raises(RuntimeError, match="encoder.block.1.layer.1.DenseReluDense.wi_1.weight"):
        NativeT5Encoder.from_state_dict(sd, R.hf_config(cfg))


def test_finalize_names_a_tensor_whose_shape_the_config_does_not_give():
    """DenseReluDense.wo.weight [d_model, d_ff] replaced by its transpose (64 x 128 -> 128 x 64): finalize names the key and says what is wrong with it"""
    from univst_amd.text import NativeT5Encoder
    c = case("tiny")
    sd = dict(c.sd)
    key = "encoder.block.1.layer.1.DenseReluDense.wo.weight"
    sd[key] = sd[key].t().contiguous()
    with pytest.raises(RuntimeError, match="which the config does not give") as e:
        NativeT5Encoder.from_state_dict(sd, R.hf_config(c.cfg))
    assert key in str(e.value)


def test_shared_readouts():
    """the read-outs every handle answers: the weights are counted and the slab holds the high-water mark"""
    c = case("tiny")
    c.enc(c.ids)
    assert c.enc.query("weight_bytes") > 0 and c.enc.query("arena_bytes") >= c.enc.query("arena_high_water") > 0


# ------------------------------------------------------------------------------------------------------------ the pipeline hook
def test_pipeline_encode_prompt_uses_the_native_t5_encoder():
    """CustomStableDiffusion3Pipeline.encode_prompt with NativeT5Encoder as text_encoder_3 (native CLIP towers, stub tokenizers): the T5 rows of the
    [B, 77 + S, joint_dim] result are the encoder's own output, the CLIP rows are what they are without a T5 encoder"""
    from univst_amd.backbones.video_diffusion_sd3.pipelines.custom_pipeline import CustomStableDiffusion3Pipeline
    from univst_amd.text import NativeCLIPText
    c = case("mid")
    ccfg = CR.Cfg(vocab_size=96, hidden_size=128, intermediate_size=512, num_layers=2, num_heads=2, hidden_act="gelu", projection_dim=128, eos_token_id=7)
    hf = dict(vocab_size=96, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, max_position_embeddings=77, hidden_act="gelu",
              layer_norm_eps=1e-5, projection_dim=128, eos_token_id=7)
    clips = [NativeCLIPText.from_state_dict(CR.random_state_dict(ccfg, seed=s), hf) for s in (1, 2)]
    clip_ids = CR.make_ids(ccfg, 2, 77, seed=5, eos_at=[9, 40])

    def tok(ids, max_len):
        table = {"a": ids[0].cpu(), "b": ids[1].cpu()}

        class Tok:          # the stub tokenizer: fixed ids per prompt
            model_max_length = max_len
            __call__ = lambda self, prompts, **kw: types.SimpleNamespace(input_ids=torch.stack([table[p] for p in prompts]))
        return Tok()

    tr = types.SimpleNamespace(device=torch.device("cuda"), config=types.SimpleNamespace(joint_attention_dim=512, sample_size=32))
    kw = dict(transformer=tr, scheduler=None, text_encoder=clips[0], text_encoder_2=clips[1], tokenizer=tok(clip_ids, 77), tokenizer_2=tok(clip_ids, 77))
    with_t5 = CustomStableDiffusion3Pipeline(text_encoder_3=c.enc, tokenizer_3=tok(c.ids, 77), **kw)
    without = CustomStableDiffusion3Pipeline(**kw)
    pe, _, pp, _ = with_t5.encode_prompt(prompt=["a", "b"], max_sequence_length=77)
    pe0, _, pp0, _ = without.encode_prompt(prompt=["a", "b"], max_sequence_length=77)
    assert pe.dtype == torch.float16 and tuple(pe.shape) == (2, 77 + 77, 512) and tuple(pp.shape) == (2, 256)
    assert torch.equal(pe[:, 77:], c.enc(c.ids)[0]) and pe[:, 77:].abs().max().item() > 0
    assert torch.equal(pe[:, :77], pe0[:, :77]) and torch.equal(pp, pp0) and pe[:, :77, 256:].abs().max().item() == 0 and pe[:, :77, :256].abs().max().item() > 0
