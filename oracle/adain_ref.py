"""float64 AdaIN references for tests/test_gpu_adain.py: the attention-feature shift of the UNet plugin (csrc/pnp.hip) and of the SD3
plugin (csrc/sd3.hip) on the fused q | k | v buffer, and the latent AdaIN that starts the loop.

The inputs are the fp16 values the operator is given (both sides start from the same numbers); everything after that is float64 and
two-pass.  The arithmetic is unet_ref.pnp_shift / attention_adain, sd3_ref.attention_adain and unet_ref.latent_adain (held to them in
tests/test_adain_cases.py).  Every reference also returns the intermediate terms its bound needs (oracle/adain_cases.py), and takes the
handles tests/test_adain_cases.py turns to show that a defect of the kernels would be seen: a per-row weight that enters the style
STATISTICS only (0: the row is dropped, 2: counted twice), statistics computed elsewhere, fewer LayerNorm columns, another blend source."""
from collections import namedtuple

import torch

EPS = 1e-5

# out [3FN, 3C]; mean, std [F, 2C] (style K | V columns); r, mu, A [F, N, 2, 1] (stylised row: 1 / sqrt(var + eps), mean, mean |x|);
# x, sty [F, N, 2, C] (stylised and blend-source K | V)
ShiftRef = namedtuple("ShiftRef", "out mean std r mu A x sty")
LatentRef = namedtuple("LatentRef", "out cmu csigma smu sstd")          # out [1, C, F, h, w]; cmu, csigma [C]; smu, sstd [C, F]


def style_stats(qkv, F, N, C, row_weight=None, unbiased=True):
    """per (frame, channel) mean / std over the N rows of the style branch's K | V columns -> (mean, std) [F, 2C] float64.
    row_weight [F * N]: weight of each style row in the sums (the count is the sum of the weights)."""
    sty = qkv[F * N:2 * F * N, C:3 * C].double().reshape(F, N, 2 * C)
    w = torch.ones(F, N, dtype=torch.float64) if row_weight is None else row_weight.double().reshape(F, N)
    cnt = w.sum(dim=1)[:, None]
    mean = (sty * w[..., None]).sum(dim=1) / cnt
    den = (cnt - 1).clamp_min(1.0) if unbiased else cnt                 # N = 1: the kernel divides by 1 as well
    var = (((sty - mean[:, None]) ** 2) * w[..., None]).sum(dim=1) / den
    return mean, var.sqrt()


def _blend(qkv, F, N, C, alpha, beta, gamma, mean, std, ln, r, mu, x, blend_branch):
    FN = F * N
    q = qkv.double()
    out = q.clone()
    out[2 * FN:, :C] = gamma * (alpha * q[:FN, :C] + (1.0 - alpha) * q[2 * FN:, :C])
    sty = q[blend_branch * FN:(blend_branch + 1) * FN, C:].reshape(F, N, 2, C)
    ad = ln * std.reshape(F, 1, 2, C) + mean.reshape(F, 1, 2, C)
    out[2 * FN:, C:] = (beta * ad + (1.0 - beta) * sty).reshape(FN, 2 * C)
    return ShiftRef(out, mean, std, r, mu, x.abs().mean(dim=-1, keepdim=True), x, sty)


def shift_ref(qkv, F, N, C, alpha, beta, gamma, row_weight=None, stats=None, ln_cols=None, blend_branch=1):
    """the UNet plugin's shift on the fused [3 F N, 3C] buffer (rows: content | style | stylised, columns: q | k | v):
        q2 <- gamma (alpha q0 + (1 - alpha) q2)
        k2 <- beta (LN_C(k2) sigma_s + m_s) + (1 - beta) k1          (same for v)
    m_s, sigma_s: style mean / unbiased std per (frame, channel) over N; LN_C: affine-free LayerNorm over C per stylised row, biased
    variance, eps 1e-5.  stats: (mean, std) [F, 2C] to use instead of the style's own; ln_cols: the LayerNorm sums stop at this column
    (still divided by C); blend_branch: the branch the (1 - beta) term is taken from."""
    mean, std = style_stats(qkv, F, N, C, row_weight) if stats is None else stats
    x = qkv[2 * F * N:, C:].double().reshape(F, N, 2, C)
    xs = x if ln_cols is None else x[..., :ln_cols]
    mu = xs.sum(dim=-1, keepdim=True) / C
    var = ((xs - mu) ** 2).sum(dim=-1, keepdim=True) / C
    r = 1.0 / torch.sqrt(var + EPS)
    return _blend(qkv, F, N, C, alpha, beta, gamma, mean, std, (x - mu) * r, r, mu, x, blend_branch)


def sd3_shift_ref(qkv, F, N, C, heads, alpha, beta, gamma, row_weight=None, cnt_row_weight=None, stats=None, joint=True, blend_branch=1):
    """the SD3 plugin's shift: as shift_ref, but the stylised K / V are normalised per (frame, head) over (N, d) JOINTLY (biased
    variance, eps 1e-5: F.instance_norm on [B, heads, N, d]).  cnt_row_weight [F * N]: weight of each stylised row in those sums.
    joint=False: per (row, head) over d only.  r, mu, A come back as [F, 1 or N, 2, C] (one value per head, repeated over its d columns)."""
    d = C // heads
    mean, std = style_stats(qkv, F, N, C, row_weight) if stats is None else stats
    x = qkv[2 * F * N:, C:].double().reshape(F, N, 2, heads, d)
    w = torch.ones(F, N, dtype=torch.float64) if cnt_row_weight is None else cnt_row_weight.double().reshape(F, N)
    w = w[:, :, None, None, None]
    dims = (1, 4) if joint else (4,)
    cnt = (w.expand_as(x)).sum(dim=dims, keepdim=True)
    mu = (x * w).sum(dim=dims, keepdim=True) / cnt
    var = (((x - mu) ** 2) * w).sum(dim=dims, keepdim=True) / cnt
    r = 1.0 / torch.sqrt(var + EPS)
    A = (x.abs() * w).sum(dim=dims, keepdim=True) / cnt
    rows = 1 if joint else N
    flat = lambda t: t.expand(F, rows, 2, heads, d).reshape(F, rows, 2, C)
    ref = _blend(qkv, F, N, C, alpha, beta, gamma, mean, std, ((x - mu) * r).reshape(F, N, 2, C), flat(r), flat(mu), x.reshape(F, N, 2, C),
                 blend_branch)
    return ref._replace(A=flat(A))


def latent_adain_ref(cnt, sty, sty_joint=False, cnt_per_frame=False, n_total=None, cnt_weight=None, sty_weight=None):
    """unet_ref.latent_adain on [1, C, F, h, w]: style mean / unbiased std per (channel, frame) over (h, w); content normalised per channel
    over (F, h, w) jointly, biased variance, eps 1e-5.  sty_joint: style statistics over (F, h, w); cnt_per_frame: content statistics per
    frame; n_total: the content mean and variance are sum / n_total and sumsq / n_total - mean^2 (what the sharded apply kernel makes of a
    wrong count); cnt_weight / sty_weight [1, C, F, h, w]: weight of each element in the STATISTICS (0: dropped, 2: counted twice)."""
    c, s = cnt.double(), sty.double()
    wc = torch.ones_like(c) if cnt_weight is None else cnt_weight.double()
    ws = torch.ones_like(s) if sty_weight is None else sty_weight.double()
    sdims = (0, 2, 3, 4) if sty_joint else (0, 3, 4)
    n_s = ws.sum(dim=sdims, keepdim=True)
    smu = (s * ws).sum(dim=sdims, keepdim=True) / n_s
    sstd = ((((s - smu) ** 2) * ws).sum(dim=sdims, keepdim=True) / (n_s - 1).clamp_min(1.0)).sqrt()
    cdims = (3, 4) if cnt_per_frame else (2, 3, 4)
    if n_total is None:
        n_c = wc.sum(dim=cdims, keepdim=True)
        cmu = (c * wc).sum(dim=cdims, keepdim=True) / n_c
        var = (((c - cmu) ** 2) * wc).sum(dim=cdims, keepdim=True) / n_c
    else:
        cmu = (c * wc).sum(dim=cdims, keepdim=True) / n_total
        var = ((c ** 2 * wc).sum(dim=cdims, keepdim=True) / n_total - cmu ** 2).clamp_min(0.0)
    out = (c - cmu) / torch.sqrt(var + EPS) * sstd + smu
    C, F = c.shape[1], c.shape[2]
    per = lambda t: t.expand(1, C, F, 1, 1).reshape(C, F)
    return LatentRef(out, per(cmu)[:, 0], per(var.sqrt())[:, 0], per(smu), per(sstd))
