"""CPU: the host-side relative-position bucket function of the native T5 encoder (univst_debug_t5_buckets, csrc/t5.hip uv_t5_bucket_table) against
transformers' T5Attention._relative_position_bucket, exactly, and the layout of the per-head bias table built from it.

transformers evaluates the logarithm in float32; the library in double.  For both settings below the float32 result of transformers equals the
float64 evaluation of the same formula for every |delta| <= 511 — checked on the CPU when this test was written, and re-checked here by
``test_float32_and_float64_agree`` — so the reference is unambiguous, including at the exact-power points."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import t5_ref as R  # noqa: E402

SETTINGS = [(32, 128), (64, 256)]
N = 512


def native_buckets(num_buckets, max_distance, n=N):
    from univst_amd import _native
    out = (C.c_int * max(2 * n - 1, 1))()
    _native.check(_native.load().univst_debug_t5_buckets(num_buckets, max_distance, n, out), "debug_t5_buckets")
    return torch.tensor(list(out))


def bucket64(rel, num_buckets, max_distance):
    num_buckets //= 2
    n, max_exact = rel.abs(), num_buckets // 2
    large = max_exact + (torch.log(n.double() / max_exact) / math.log(max_distance / max_exact) * (num_buckets - max_exact)).to(torch.long)
    return (rel > 0).long() * num_buckets + torch.where(n < max_exact, n, large.clamp(max=num_buckets - 1))


@pytest.mark.parametrize("num_buckets,max_distance", SETTINGS)
def test_buckets_equal_transformers(num_buckets, max_distance):
    t5 = pytest.importorskip("transformers.models.t5.modeling_t5")
    delta = torch.arange(-(N - 1), N)
    want = t5.T5Attention._relative_position_bucket(delta, bidirectional=True, num_buckets=num_buckets, max_distance=max_distance)
    got = native_buckets(num_buckets, max_distance)
    assert got.shape == want.shape == (2 * N - 1,) and torch.equal(got, want), (delta[got != want], got[got != want], want[got != want])
    assert torch.equal(R.relative_position_bucket(delta, num_buckets, max_distance), want)      # the restatement's own copy
    assert got.min().item() == 0 and got.max().item() == num_buckets - 1


@pytest.mark.parametrize("num_buckets,max_distance", SETTINGS)
def test_float32_and_float64_agree(num_buckets, max_distance):
    t5 = pytest.importorskip("transformers.models.t5.modeling_t5")
    delta = torch.arange(-(N - 1), N)
    want = t5.T5Attention._relative_position_bucket(delta, bidirectional=True, num_buckets=num_buckets, max_distance=max_distance)
    assert torch.equal(bucket64(delta, num_buckets, max_distance), want)


def test_shorter_range_is_the_middle_of_the_longer_one():
    full, part = native_buckets(32, 128), native_buckets(32, 128, n=17)
    assert torch.equal(part, full[N - 17:N + 16]) and native_buckets(32, 128, n=1).tolist() == [0]


def test_bad_settings_are_refused():
    with pytest.raises(RuntimeError, match="num_buckets"):
        native_buckets(2, 128)
    with pytest.raises(RuntimeError, match="max_distance"):
        native_buckets(32, 8)
    with pytest.raises(RuntimeError, match="n=0"):
        native_buckets(32, 128, n=0)


def bias_table(rel_bias, num_buckets, max_distance):
    """the table layout the attention kernel reads, [heads][delta + 511] with delta = key position - query position, from
    relative_attention_bias.weight [num_buckets, heads] (what T5::finalize builds on the host)"""
    return rel_bias.float()[native_buckets(num_buckets, max_distance)].t().contiguous()


def test_bias_table_layout():
    """table[h][(j - i) + 511] is transformers' position_bias[0, h, i, j] for every i, j < 512"""
    cfg = R.Cfg(num_heads=3)
    w = torch.randn(cfg.num_buckets, cfg.num_heads, generator=torch.Generator().manual_seed(0))
    table = bias_table(w, cfg.num_buckets, cfg.max_distance)
    assert tuple(table.shape) == (3, 2 * N - 1)
    want = R.position_bias({"encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight": w}, cfg, N, "cpu")      # [heads, i, j]
    pos = torch.arange(N)
    assert torch.equal(table[:, (pos[None, :] - pos[:, None]) + N - 1], want)
    assert torch.equal(table[:, N - 1], w[0]) and torch.equal(table[:, N], w[cfg.num_buckets // 2 + 1]) and torch.equal(table[:, N - 2], w[1])
