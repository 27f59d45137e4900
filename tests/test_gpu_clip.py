"""GPU: the native CLIP text tower (univst_amd/text.py, csrc/clip.hip) against the restatement tests/clip_ref.py (held to transformers by
tests/test_clip_ref.py): the causal attention operator against an fp64 softmax with a derived bound, masked memory that must never reach an
output, the whole encoder against the fp64 restatement with the torch-fp16 restatement's own error as the yardstick, causality end to end, the
wrapper's contract and the pipeline hook."""
import json
import os
import subprocess
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS16 = 2.0 ** -11          # unit roundoff of fp16


# ------------------------------------------------------------------------------------------------------------ the attention operator
def clip_attention(qkv, B, S, heads):
    from univst_amd import _native
    out = torch.empty(max(B * S, 1), heads * 64, device=qkv.device, dtype=torch.float16)
    _native.check(_native.load().univst_clip_attention(_native.ptr(qkv), B, S, heads, _native.ptr(out), _native.stream_ptr()), "clip_attention")
    return out[:B * S]


def make_qkv(B, S, heads, seed):
    """q | k | v rows [B*S, 3*heads*64] fp16; q carries the folded scale, so the scores ARE q.k: sigma_q sigma_k sqrt(64) = 3"""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * S, 3, heads * 64, generator=g)
    qkv[:, :2] *= (3.0 / 8.0) ** 0.5
    return qkv.reshape(B * S, 3 * heads * 64).half()


def attention_ref64(qkv, B, S, heads):
    """fp64 causal softmax attention on the same fp16 inputs -> (o [B*S, heads*64], vmax = max over the visible keys j <= i of |v[j, d]|)"""
    x = qkv.double().view(B, S, 3, heads, 64).permute(2, 0, 3, 1, 4)      # [3][B][heads][S][64]
    q, k, v = x[0], x[1], x[2]
    sc = (q @ k.transpose(-1, -2)).masked_fill(torch.ones(S, S, dtype=torch.bool, device=qkv.device).triu(1), float("-inf"))
    o = torch.softmax(sc, dim=-1) @ v
    back = lambda t: t.permute(0, 2, 1, 3).reshape(B * S, heads * 64)      # noqa: E731
    return back(o), back(v.abs().cummax(dim=2).values), sc


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("S", [1, 15, 16, 17, 33, 77])
def test_attention_operator(S, heads, B):
    """every output element is a convex combination of the visible V rows, so |o - o64| <= 4 x 2^-11 x max_{j <= i} |v_j| elementwise: one unit
    roundoff each for the fp16 rounding of P, the fp16 rounding of the output and the exp2 / fp32 accumulation error, and one spare"""
    qkv = make_qkv(B, S, heads, seed=S * 100 + heads * 10 + B).cuda()
    got = clip_attention(qkv, B, S, heads).double()
    want, vmax, sc = attention_ref64(qkv, B, S, heads)
    if S > 1:
        vis = torch.ones(S, S, dtype=torch.bool, device=sc.device).tril()
        print(f"S={S} heads={heads} B={B}: visible score std {sc[:, :, vis].std().item():.2f}", end="; ")
    bound = 4 * EPS16 * vmax
    frac = ((got - want).abs() / bound.clamp(min=1e-30)).max().item()
    print(f"S={S} heads={heads} B={B}: worst |o - o64| / bound = {frac:.3f}")
    assert torch.isfinite(got).all() and frac <= 1.0


@pytest.mark.parametrize("S,p", [(33, 20), (77, 20), (77, 70)])
def test_masked_memory_never_leaks(S, p):
    """K and V rows of positions j > p set to large finite values, then to NaN: the output rows <= p are bit-identical to the clean run (a masked
    probability is an exact 0 that is never multiplied with its V row; at S = 77 the kernel's own pad rows 77..79 sit next to the poisoned ones)"""
    B, heads = 2, 3
    C = heads * 64
    qkv = make_qkv(B, S, heads, seed=S + p).cuda()
    clean = clip_attention(qkv, B, S, heads).view(B, S, C)
    assert torch.isfinite(clean).all()
    g = torch.Generator().manual_seed(1)
    big = (torch.randint(0, 2, (B, S - 1 - p, 2 * C), generator=g).float() * 2 - 1).mul(6e4).half().cuda()
    for name, poison in (("+-6e4", big), ("NaN", torch.full_like(big, float("nan")))):
        x = qkv.clone().view(B, S, 3 * C)
        x[:, p + 1:, C:] = poison
        out = clip_attention(x.view(B * S, 3 * C), B, S, heads).view(B, S, C)
        assert torch.equal(out[:, :p + 1].view(torch.int16), clean[:, :p + 1].view(torch.int16)), f"{name} behind position {p} reached a row <= {p}"
        if name == "NaN":
            assert torch.isnan(out[:, p + 1:]).any(), "the poisoned rows themselves must see the poison (the test would otherwise prove nothing)"


def test_attention_refuses_bad_shapes():
    qkv = make_qkv(1, 8, 1, 0).cuda()
    with pytest.raises(RuntimeError, match="1 <= S <= 80"):
        clip_attention(qkv, 1, 81, 1)
    with pytest.raises(RuntimeError, match="1 <= S <= 80"):
        clip_attention(qkv, 1, 0, 1)


# ------------------------------------------------------------------------------------------------------------ the whole encoder
CONFIGS = {
    "tiny-quick_gelu": R.Cfg(vocab_size=96, hidden_size=128, intermediate_size=512, num_layers=2, num_heads=2, hidden_act="quick_gelu", projection_dim=128,
                             eos_token_id=2),
    "tiny-gelu": R.Cfg(vocab_size=96, hidden_size=128, intermediate_size=512, num_layers=2, num_heads=2, hidden_act="gelu", projection_dim=128, eos_token_id=7),
    "clip-l-width": R.Cfg(vocab_size=512, hidden_size=768, intermediate_size=3072, num_layers=2, num_heads=12, hidden_act="quick_gelu", eos_token_id=2),
    "bigg-width": R.Cfg(vocab_size=512, hidden_size=1280, intermediate_size=5120, num_layers=1, num_heads=20, hidden_act="gelu", projection_dim=1280,
                        eos_token_id=7),
}
_CASES = {}


def hf_config(cfg):
    return dict(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size, num_hidden_layers=cfg.num_layers,
                num_attention_heads=cfg.num_heads, max_position_embeddings=cfg.max_positions, hidden_act=cfg.hidden_act,
                layer_norm_eps=cfg.layer_norm_eps, projection_dim=cfg.projection_dim or 512, eos_token_id=cfg.eos_token_id)


def case(name):
    """weights, ids, the native handle and the restatement in fp64 and in torch fp16 (both on the GPU), built once per config"""
    if name not in _CASES:
        from univst_amd.text import NativeCLIPText
        cfg = CONFIGS[name]
        sd = R.random_state_dict(cfg, seed=len(name), prefix="text_model.")
        ids = R.make_ids(cfg, 3, 77, seed=3, eos_at=[5, 76, 30]).cuda()
        with torch.no_grad():
            ref64, ref16 = R.forward(sd, cfg, ids, dtype=torch.float64), R.forward(sd, cfg, ids, dtype=torch.float16)
        enc = NativeCLIPText.from_state_dict(sd, hf_config(cfg))
        _CASES[name] = types.SimpleNamespace(cfg=cfg, sd=sd, ids=ids, ref64=ref64, ref16=ref16, enc=enc)
    return _CASES[name]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_encoder_against_fp64_restatement(name):
    """yardstick: the reference runs this module as text_encoder.to(fp16).cuda(), i.e. the restatement in torch fp16 on this GPU, whose distance to
    the fp64 restatement is e_ref.  The native encoder must stay within 2 x e_ref (the factor covers a different but equally valid accumulation
    order: split-K, fp32 softmax) on the last hidden state, hidden_states[-2] and the pooled / projected output."""
    c = case(name)
    out = c.enc(c.ids, output_hidden_states=True)
    pooled_key = "text_embeds" if c.cfg.projection_dim else "pooler_output"
    trio = [("last_hidden_state", out.last_hidden_state, c.ref64["last_hidden_state"], c.ref16["last_hidden_state"]),
            ("hidden_states[-2]", out.hidden_states[-2], c.ref64["hidden_states"][-2], c.ref16["hidden_states"][-2]),
            (pooled_key, getattr(out, pooled_key), c.ref64[pooled_key], c.ref16[pooled_key])]
    assert len(out.hidden_states) == c.cfg.num_layers + 1
    ok = True
    for what, got, r64, r16 in trio:
        assert got.shape == r64.shape and got.dtype == torch.float16
        e_nat, e_ref = (got.double() - r64).abs().max().item(), (r16.double() - r64).abs().max().item()
        print(f"{name} {what}: e_native {e_nat:.3e}, e_ref (torch fp16) {e_ref:.3e}, ratio {e_nat / e_ref:.2f}, max|want| {r64.abs().max().item():.2f}")
        ok = ok and torch.isfinite(got).all().item() and e_nat <= 2 * e_ref
    assert ok


def test_native_causality():
    """two id tensors that differ only from position p on: bit-identical rows before p in every hidden state and in the last hidden state"""
    c = case("tiny-gelu")
    p = 29
    b = c.ids.clone()
    b[:, p:] = R.make_ids(c.cfg, 3, 77, seed=8).cuda()[:, p:]
    assert (b[:, p:] != c.ids[:, p:]).any(dim=1).all()
    oa, ob = c.enc(c.ids, output_hidden_states=True), c.enc(b, output_hidden_states=True)
    for x, y in zip(oa.hidden_states + (oa.last_hidden_state,), ob.hidden_states + (ob.last_hidden_state,)):
        assert torch.equal(x[:, :p], y[:, :p])
        assert not torch.equal(x[:, p:], y[:, p:])


# ------------------------------------------------------------------------------------------------------------ the wrapper's contract
def test_wrapper_contract():
    from univst_amd.text import NativeCLIPText
    c = case("tiny-gelu")          # projected, keys with the text_model. prefix
    bare = R.strip_prefix(c.sd)
    assert set(bare) != set(c.sd)
    other = NativeCLIPText.from_state_dict(bare, hf_config(c.cfg))
    a, b = c.enc(c.ids, output_hidden_states=True), other(c.ids, output_hidden_states=True)
    assert torch.equal(a.last_hidden_state, b.last_hidden_state) and torch.equal(a.text_embeds, b.text_embeds)
    assert a[0] is a.text_embeds and tuple(a[0].shape) == (3, 128) and len(a.hidden_states) == c.cfg.num_layers + 1
    assert all(torch.equal(x, y) for x, y in zip(a.hidden_states, b.hidden_states))
    assert c.enc(c.ids).hidden_states is None and torch.equal(c.enc(c.ids, return_dict=False)[0], a.text_embeds)
    # the plain model: out[0] is the last hidden state, pooler_output the EOS row of it
    plain = NativeCLIPText.from_state_dict({k: v for k, v in c.sd.items() if k != "text_projection.weight"}, hf_config(c.cfg))
    o = plain(c.ids)
    assert o[0] is o.last_hidden_state and torch.equal(o[0], a.last_hidden_state) and not hasattr(o, "text_embeds")
    pos = R.eos_positions(c.ids, c.cfg.eos_token_id)
    assert torch.equal(o.pooler_output, o.last_hidden_state[torch.arange(3, device="cuda"), pos])
    # module-like attributes the call sites touch
    assert plain.dtype == torch.float16 and plain.device.type == "cuda" and plain.config.use_attention_mask is False and plain._h
    assert plain.to(torch.float16) is plain and plain.cuda() is plain and plain.requires_grad_(False) is plain and plain.eval() is plain
    # inputs it refuses
    with pytest.raises(RuntimeError, match="runs on the GPU only"):
        plain(c.ids.cpu())
    mask = torch.ones_like(c.ids)
    assert torch.equal(plain(c.ids, attention_mask=mask)[0], o[0])
    mask[0, 50:] = 0
    with pytest.raises(NotImplementedError):
        plain(c.ids, attention_mask=mask)
    bad = c.ids.clone()
    bad[1, 3] = c.cfg.vocab_size
    with pytest.raises(IndexError):
        plain(bad)
    bad[1, 3] = -1
    with pytest.raises(IndexError):
        plain(bad)


def test_second_encode_leaves_the_arena_alone():
    c = case("tiny-quick_gelu")
    c.enc(c.ids, output_hidden_states=True)
    hw = c.enc.arena_high_water()
    assert hw > 0
    first = c.enc(c.ids, output_hidden_states=True)
    again = c.enc(c.ids)
    assert c.enc.arena_high_water() == hw
    assert torch.equal(first.last_hidden_state, again.last_hidden_state) and torch.equal(first.text_embeds, again.text_embeds)
    # the split-K partials of the K = 3072 linear live in the arena too (a launch without a workspace would allocate stream-ordered scratch)
    wide = case("clip-l-width")
    wide.enc(wide.ids)
    assert 0 < wide.enc.query("splitk_bytes") < wide.enc.arena_high_water()


def test_create_refuses_unsupported_towers():
    from univst_amd.text import NativeCLIPText
    cfg = CONFIGS["tiny-gelu"]
    with pytest.raises(RuntimeError, match="head dim of 64"):
        NativeCLIPText.from_state_dict({}, dict(hf_config(cfg), num_attention_heads=4))
    with pytest.raises(RuntimeError, match="max_positions"):
        NativeCLIPText.from_state_dict({}, dict(hf_config(cfg), max_position_embeddings=128))
    sd = dict(case("tiny-gelu").sd)
    del sd["text_model.encoder.layers.1.mlp.fc2.bias"]
    with pytest.raises(RuntimeError, match="encoder.layers.1.mlp.fc2.bias"):
        NativeCLIPText.from_state_dict(sd, hf_config(cfg))


def test_finalize_names_a_tensor_whose_shape_the_config_does_not_give():
    """mlp.fc1.weight [I, C] replaced by its transpose [C, I] (I = 512, C = 128): finalize names the key and says what is wrong with it"""
    from univst_amd.text import NativeCLIPText
    c = case("tiny-gelu")
    sd = dict(c.sd)
    key = "text_model.encoder.layers.1.mlp.fc1.weight"
    sd[key] = sd[key].t().contiguous()
    with pytest.raises(RuntimeError, match="which the config does not give") as e:
        NativeCLIPText.from_state_dict(sd, hf_config(c.cfg))
    assert "encoder.layers.1.mlp.fc1.weight" in str(e.value)


def test_shared_readouts():
    """the read-outs every handle answers: the weights are counted and the slab holds the high-water mark"""
    c = case("tiny-gelu")
    c.enc(c.ids)
    assert c.enc.query("weight_bytes") > 0 and c.enc.query("arena_bytes") >= c.enc.query("arena_high_water") > 0


_CHILD = """
import sys, torch
sys.path.insert(0, {root!r})
from univst_amd.text import NativeCLIPText
enc = NativeCLIPText.from_pretrained({path!r})
out = enc(torch.load({ids!r}).cuda(), output_hidden_states=True)
assert "transformers" not in sys.modules, "from_pretrained / encode imported transformers"
assert enc.with_projection and len(out.hidden_states) == 3
torch.save(dict(last=out.last_hidden_state.cpu(), emb=out[0].cpu()), {res!r})
"""


def test_from_pretrained_reads_a_transformers_directory_without_transformers(tmp_path):
    """<dir>/text_encoder/config.json + model.safetensors, the layout CLIPTextModelWithProjection.from_pretrained reads, loaded in a fresh process
    that never imports transformers"""
    from safetensors.torch import save_file
    from univst_amd.text import NativeCLIPText
    c = case("tiny-gelu")
    d = tmp_path / "sd3" / "text_encoder"
    d.mkdir(parents=True)
    (d / "config.json").write_text(json.dumps(dict(hf_config(c.cfg), architectures=["CLIPTextModelWithProjection"], model_type="clip_text_model")))
    save_file({k: v.contiguous() for k, v in c.sd.items()}, str(d / "model.safetensors"))
    torch.save(c.ids.cpu(), str(tmp_path / "ids.pt"))
    script = _CHILD.format(root=ROOT, path=str(tmp_path / "sd3"), ids=str(tmp_path / "ids.pt"), res=str(tmp_path / "res.pt"))
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    res = torch.load(str(tmp_path / "res.pt"))
    want = c.enc(c.ids)
    assert torch.equal(res["last"], want.last_hidden_state.cpu()) and torch.equal(res["emb"], want.text_embeds.cpu())
    with pytest.raises(FileNotFoundError):
        NativeCLIPText.from_pretrained(str(tmp_path / "nowhere"))
    with pytest.raises(FileNotFoundError):
        NativeCLIPText.from_pretrained(str(tmp_path / "sd3"), subfolder="text_encoder_2")


# ------------------------------------------------------------------------------------------------------------ the pipeline hook
@pytest.mark.parametrize("cfg_guidance", [False, True])
def test_pipeline_encode_prompt_uses_the_native_encoder(cfg_guidance):
    from univst_amd.backbones.video_diffusion_sd.pipelines.stable_diffusion import SpatioTemporalStableDiffusionPipeline
    from univst_amd.schedulers import DDIMScheduler
    from univst_amd.text import NativeCLIPText
    c = case("clip-l-width")
    enc = NativeCLIPText.from_state_dict(c.sd, hf_config(c.cfg))
    table = {"a": c.ids[0].cpu(), "b": c.ids[1].cpu(), "": c.ids[2].cpu()}

    class Tok:          # the stub tokenizer: fixed ids per prompt
        model_max_length = 77
        __call__ = lambda self, prompts, **kw: types.SimpleNamespace(input_ids=torch.stack([table[p] for p in ([prompts] if isinstance(prompts, str) else prompts)]))

    pipe = SpatioTemporalStableDiffusionPipeline(vae=None, text_encoder=enc, tokenizer=Tok(), unet=types.SimpleNamespace(device=torch.device("cuda")),
                                                 scheduler=DDIMScheduler())
    got = pipe._encode_prompt(["a", "b"], torch.device("cuda"), 1, cfg_guidance, None)
    want = enc(c.ids[:2])[0]
    if cfg_guidance:          # the empty negative prompt of both batch entries goes first
        want = torch.cat([enc(c.ids[2:3].expand(2, -1))[0], want])
    assert got.dtype == torch.float16 and tuple(got.shape) == (4 if cfg_guidance else 2, 77, 768) and torch.equal(got, want)
