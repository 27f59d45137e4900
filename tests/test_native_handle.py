"""CPU: what every wrapper of a model handle goes through (univst_amd/_native.py ``build_handle`` and ``NativeHandle.merge_config``), driven by a
stub library and a stub stream: a failed load or finalize destroys the handle exactly once and names what failed, dtypes and 0-dim tensors arrive
as the C ABI takes them, and the config merge keeps the known keys only."""
import ctypes as C
import types

import pytest
import torch

from univst_amd import _native

HANDLE = 0x5EED


class StubStream:
    cuda_stream = 77
    synced = 0

    def synchronize(self):
        self.synced += 1


class StubLib:
    """univst_stub_* as plain Python: records every call; ``fail_load`` = index of the load that returns -1, ``fail_finalize`` likewise"""

    def __init__(self, fail_load=None, fail_finalize=False, with_finalize=True):
        self.fail_load, self.fail_finalize = fail_load, fail_finalize
        self.created, self.loads, self.finalized, self.destroyed = [], [], [], []
        if with_finalize:
            self.univst_stub_finalize = self._finalize

    def univst_last_error(self):
        return b"the stub's error text"

    def univst_stub_create(self, *args):
        self.created.append(args[:-1])
        args[-1]._obj.value = HANDLE      # (the byref'd c_void_p)
        return 0

    def univst_stub_load_tensor(self, h, key, ptr, dtype, shape, ndim, stream):
        n = 1
        for i in range(ndim):
            n *= shape[i]
        raw = ((C.c_uint16 if dtype == 0 else C.c_float) * n).from_address(ptr)
        data = torch.frombuffer(raw, dtype=torch.float16 if dtype == 0 else torch.float32).clone()
        self.loads.append(types.SimpleNamespace(h=h.value, key=key, dtype=dtype, shape0=shape[0], ndim=ndim, stream=stream, data=data))
        return -1 if self.fail_load == len(self.loads) - 1 else 0

    def _finalize(self, h, stream):
        self.finalized.append(h.value)
        return -1 if self.fail_finalize else 0

    def univst_stub_destroy(self, h):
        self.destroyed.append(h.value)
        return 0


def build(lib, items, other_dtype=torch.float16, stream=None, **kw):
    stream = stream or StubStream()
    return _native.build_handle(lib, "stub", ("cfg",), items, stream.cuda_stream, stream.synchronize, other_dtype=other_dtype, **kw)


ITEMS = [("a.weight", torch.ones(2, 3)), ("b.weight", torch.ones(4)), ("c.weight", torch.ones(1))]


def test_builds_loads_finalizes_and_synchronises():
    lib, st = StubLib(), StubStream()
    h = build(lib, ITEMS, stream=st)
    assert h.value == HANDLE and lib.created == [("cfg",)]
    assert [(l.key, l.h, l.stream) for l in lib.loads] == [(k.encode(), HANDLE, 77) for k, _ in ITEMS]
    assert lib.finalized == [HANDLE] and st.synced == 1 and lib.destroyed == []


def test_a_handle_without_finalize_is_loaded_and_synchronised():
    lib, st = StubLib(with_finalize=False), StubStream()
    assert build(lib, ITEMS, stream=st).value == HANDLE
    assert len(lib.loads) == 3 and st.synced == 1 and lib.destroyed == []


def test_failed_load_names_the_key_and_destroys_the_handle_once():
    lib = StubLib(fail_load=1)
    with pytest.raises(RuntimeError, match=r"stub_load_tensor\(b\.weight\).*the stub's error text"):
        build(lib, ITEMS)
    assert lib.destroyed == [HANDLE] and lib.finalized == [] and len(lib.loads) == 2
    lib = StubLib(fail_load=1)
    with pytest.raises(RuntimeError, match=r" load_tensor\(b\.weight\)"):      # the UNet mirrors' prefix
        build(lib, ITEMS, load_what="load_tensor")
    assert lib.destroyed == [HANDLE]


def test_failed_finalize_destroys_the_handle_once():
    lib, st = StubLib(fail_finalize=True), StubStream()
    with pytest.raises(RuntimeError, match="stub_finalize"):
        build(lib, ITEMS, stream=st)
    assert lib.destroyed == [HANDLE] and lib.finalized == [HANDLE] and len(lib.loads) == 3 and st.synced == 0


def test_an_exception_inside_the_items_destroys_the_handle_too():
    def items():
        yield ITEMS[0]
        raise KeyError("a lazy state dict that breaks")
    lib = StubLib()
    with pytest.raises(KeyError):
        build(lib, items())
    assert lib.destroyed == [HANDLE] and lib.finalized == []


@pytest.mark.parametrize("other,code", [(torch.float16, 0), (torch.float32, 1)])
def test_other_dtypes_arrive_as_asked_and_fp16_fp32_as_they_are(other, code):
    src = torch.tensor([[1.5, -2.0, 0.25], [3.0, 4.0, -0.5]])
    lib = StubLib()
    build(lib, [("bf", src.to(torch.bfloat16)), ("h", src.half()), ("f", src), ("d", src.double()), ("t", src.t())], other_dtype=other)
    assert [l.dtype for l in lib.loads] == [code, 0, 1, code, 1]
    for l in lib.loads[:4]:
        assert l.ndim == 2 and torch.equal(l.data.float(), src.flatten())
    assert torch.equal(lib.loads[4].data, src.t().contiguous().flatten())      # a transposed view goes up contiguous


def test_zero_dim_tensor_keeps_ndim_0_with_a_valid_shape_pointer():
    lib = StubLib()
    build(lib, [("mix_factor", torch.tensor(0.75))], other_dtype=torch.float32)
    l, = lib.loads
    assert l.ndim == 0 and l.shape0 == 0 and l.dtype == 1 and l.data.tolist() == [0.75]      # (shape[0] was readable: one zeroed element)


def test_merge_config_takes_dicts_and_objects_and_known_keys_only():
    merge = _native.NativeHandle.merge_config
    defaults = dict(a=1, b=2, c=None)
    assert merge(defaults, None) == defaults and merge(defaults, None) is not defaults
    assert merge(defaults, dict(a=5, zzz=9)) == dict(a=5, b=2, c=None)
    assert merge(defaults, types.SimpleNamespace(b=7, c=3, zzz=9)) == dict(a=1, b=7, c=3)
    for cfg in (dict(a=None, b=4), types.SimpleNamespace(a=None, b=4)):
        assert merge(defaults, cfg) == dict(a=1, b=4, c=None)
        assert merge(defaults, cfg, keep_none=True) == dict(a=None, b=4, c=None)
    assert defaults == dict(a=1, b=2, c=None)
