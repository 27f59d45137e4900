"""RAFT-large optical flow on the native library: the ``flow_fn`` of src/cal_optica_flow.py without torchvision.

``NativeRAFT`` stands where the reference builds torchvision's ``raft_large`` (src/cal_optica_flow.py:53-55): it takes that model's state
dict unchanged and runs one C-ABI call per image pair (univst_raft_*, csrc/raft.hip): 12 flow updates, final flow only, eval mode.  The
network is third-party: restated from its published definition, parity unpinned by the reference (tests/raft_ref.py is the yardstick)."""
import torch

from . import _native


def _check_size(h, w):
    if not (h % 8 == 0 and w % 8 == 0):
        raise ValueError(f"input image H and W should be divisible by 8, but got {h} (h) and {w} (w)")
    if h // 8 < 16 or w // 8 < 16:
        raise ValueError("Feature maps are too small to be down-sampled by the correlation pyramid. H and W of feature maps should be at least 16; "
                         f"got: {(h // 8, w // 8)}. Remember that input images to the model are downsampled by 8, so that means their dimensions "
                         "should be at least 8 * 16 = 128")


class NativeRAFT(_native.NativeHandle):
    _kind, _noun = "raft", "flow estimator"

    def __init__(self, state_dict, device="cuda"):
        self.device = torch.device(device)
        items = [(k, v) for k, v in state_dict.items() if torch.is_tensor(v) and not k.endswith("num_batches_tracked")]
        self._h = _native.load_handle("raft", (), items, other_dtype=torch.float32, device=device)

    from_state_dict = classmethod(lambda cls, sd, device="cuda": cls(sd, device=device))

    @classmethod
    def from_file(cls, path, device="cuda"):
        """a torchvision ``raft_large`` checkpoint: ``.pth`` / ``.pt`` (torch.save of the state dict) or ``.safetensors``"""
        if str(path).endswith(".safetensors"):
            from safetensors.torch import load_file
            sd = load_file(path)
        else:
            sd = torch.load(path, map_location="cpu")
            if isinstance(sd, dict) and "state_dict" in sd and not any(torch.is_tensor(v) for v in sd.values()):
                sd = sd["state_dict"]
        return cls(sd, device=device)

    def _img(self, t, what):
        if self._gpu_only(t, what).dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
            raise ValueError(f"NativeRAFT: {what} must be uint8 [H, W, 3], got {t.dtype} {tuple(t.shape)}")
        return t.contiguous()

    @torch.no_grad()
    def __call__(self, img1, img2):
        """img1, img2 uint8 [H, W, 3] (device) -> float32 [H, W, 2]: flow from img1 to img2 in pixels (x, y)"""
        a, b = self._img(img1, "img1"), self._img(img2, "img2")
        if a.shape != b.shape:
            raise ValueError(f"NativeRAFT: the two images differ in size: {tuple(a.shape)} and {tuple(b.shape)}")
        H, W, _ = a.shape
        _check_size(H, W)
        out = torch.empty(H, W, 2, device=a.device, dtype=torch.float32)
        _native.check(_native.load().univst_raft_forward(self._h, _native.ptr(a), _native.ptr(b), H, W, _native.ptr(out), _native.stream_ptr()), "raft_forward")
        return out

    # ---- stages of the same graph (tests, tools/bench_flow.py)
    @torch.no_grad()
    def encode(self, img1, img2):
        """-> fmap fp16 [2, N, 256] (image 1 | image 2), hidden fp32 [N, 128], context fp16 [N, 128]; N = (H/8)(W/8) rows, y-major"""
        a, b = self._img(img1, "img1"), self._img(img2, "img2")
        H, W, _ = a.shape
        _check_size(H, W)
        N = (H // 8) * (W // 8)
        fmap = torch.empty(2, N, 256, device=a.device, dtype=torch.float16)
        hid = torch.empty(N, 128, device=a.device, dtype=torch.float32)
        ctx = torch.empty(N, 128, device=a.device, dtype=torch.float16)
        _native.check(_native.load().univst_raft_encode(self._h, _native.ptr(a), _native.ptr(b), H, W, _native.ptr(fmap), _native.ptr(hid), _native.ptr(ctx),
                                                        _native.stream_ptr()), "raft_encode")
        return fmap, hid, ctx

    @torch.no_grad()
    def gru(self, hidden, context, motion, fh, fw):
        """one RecurrentBlock step: hidden fp32 [N, 128] (a new tensor comes back), context / motion fp16 [N, 128]"""
        h = hidden.to(torch.float32).contiguous().clone()
        c, m = context.to(torch.float16).contiguous(), motion.to(torch.float16).contiguous()
        assert h.is_cuda and tuple(h.shape) == tuple(c.shape) == tuple(m.shape) == (fh * fw, 128)
        _native.check(_native.load().univst_raft_gru(self._h, _native.ptr(h), _native.ptr(c), _native.ptr(m), fh, fw, _native.stream_ptr()), "raft_gru")
        return h


def corr_pyramid(fmap1, fmap2, fh, fw):
    """fmaps fp16 [N, 256] -> the four fp32 levels [N, fh >> l, fw >> l] (views of one buffer)"""
    assert fmap1.is_cuda and fmap1.dtype == torch.float16 and tuple(fmap1.shape) == tuple(fmap2.shape) == (fh * fw, 256)
    lib = _native.load()
    buf = torch.empty(lib.univst_raft_pyramid_floats(fh, fw), device=fmap1.device, dtype=torch.float32)
    _native.check(lib.univst_raft_corr_pyramid(_native.ptr(fmap1.contiguous()), _native.ptr(fmap2.contiguous()), fh, fw, _native.ptr(buf), _native.stream_ptr()),
                  "raft_corr_pyramid")
    N, off, levels = fh * fw, 0, []
    for l in range(4):
        n = N * (fh >> l) * (fw >> l)
        levels.append(buf[off:off + n].view(N, fh >> l, fw >> l))
        off += n
    return buf, levels


def corr_lookup(pyramid_buf, coords, fh, fw, want_f16=False):
    """pyramid_buf from corr_pyramid, coords fp32 [N, 2] (x, y) -> fp32 [N, 324] (and the fp16 [N, 328] conv operand rows)"""
    N = fh * fw
    assert coords.is_cuda and coords.dtype == torch.float32 and tuple(coords.shape) == (N, 2)
    o32 = torch.empty(N, 324, device=coords.device, dtype=torch.float32)
    o16 = torch.empty(N, 328, device=coords.device, dtype=torch.float16) if want_f16 else None
    _native.check(_native.load().univst_raft_corr_lookup(_native.ptr(pyramid_buf), _native.ptr(coords.contiguous()), fh, fw, _native.ptr(o32), _native.ptr(o16),
                                                         _native.stream_ptr()), "raft_corr_lookup")
    return (o32, o16) if want_f16 else o32


def convex_upsample(flow, mask, fh, fw):
    """flow fp32 [fh, fw, 2], mask fp16 [N, 576] (before the factor 0.25) -> fp32 [8 fh, 8 fw, 2]"""
    assert flow.is_cuda and flow.dtype == torch.float32 and mask.dtype == torch.float16 and tuple(mask.shape) == (fh * fw, 576)
    out = torch.empty(8 * fh, 8 * fw, 2, device=flow.device, dtype=torch.float32)
    _native.check(_native.load().univst_raft_convex_upsample(_native.ptr(flow.contiguous()), _native.ptr(mask.contiguous()), fh, fw, _native.ptr(out),
                                                             _native.stream_ptr()), "raft_convex_upsample")
    return out
