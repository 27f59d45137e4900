"""float64 GroupNorm (+ SiLU) on NHWC rows: the reference of tests/test_gpu_groupnorm.py for csrc/norm.hip.

The inputs are the fp16 values the operator is given (both sides start from the same numbers); everything after that is float64 and
two-pass.  x2 is the second source of a virtual channel concat, rows_per_stat the statistics unit (one frame, or all frames of a branch),
row_weight an optional per-row weight that enters the STATISTICS only (tests/test_groupnorm_cases.py: what the output looks like when a
row is dropped from, or counted twice in, the sums)."""
from collections import namedtuple

import torch

GnRef = namedtuple("GnRef", "out z mean sigma")      # out, z: [rows, C] float64 (z before SiLU); mean, sigma: [S, G]


def groupnorm_ref(x1, gamma, beta, groups, eps, rows_per_stat, silu=False, x2=None, row_weight=None):
    x = x1.double() if x2 is None else torch.cat([x1.double(), x2.double()], dim=1)
    rows, C = x.shape
    assert rows % rows_per_stat == 0 and C % groups == 0
    S, cpg = rows // rows_per_stat, C // groups
    xg = x.reshape(S, rows_per_stat, groups, cpg)
    w = torch.ones(rows, dtype=torch.float64) if row_weight is None else row_weight.double()
    w = w.reshape(S, rows_per_stat, 1, 1)
    cnt = w.sum(dim=1, keepdim=True) * cpg                                      # [S, 1, 1, 1]
    mean = (xg * w).sum(dim=(1, 3), keepdim=True) / cnt                         # [S, 1, G, 1]
    var = (((xg - mean) ** 2) * w).sum(dim=(1, 3), keepdim=True) / cnt
    z = (xg - mean) / torch.sqrt(var + eps)
    z = z.reshape(rows, C) * gamma.double() + beta.double()
    out = z * torch.sigmoid(z) if silu else z
    return GnRef(out, z, mean.reshape(S, groups), var.sqrt().reshape(S, groups))


def fold_linear_ref(x, gamma, beta, groups, eps, rows_per_stat, w, bias=None):
    """-> (W_sets [S, N, C], bias32 [S, N]) in float64: the GroupNorm of x folded into the linear (w [N, C], bias) that consumes it,
    y = W_s x + b_s with W_s[n, k] = w[n, k] gamma_k r_{s, g(k)} and b_s[n] = bias[n] + sum_k w[n, k] (beta_k - mean_{s, g(k)} gamma_k r_{s, g(k)})."""
    ref = groupnorm_ref(x, gamma, beta, groups, eps, rows_per_stat)
    cpg = x.shape[1] // groups
    r = (1.0 / torch.sqrt(ref.sigma ** 2 + eps)).repeat_interleave(cpg, dim=1)   # [S, C]
    mean = ref.mean.repeat_interleave(cpg, dim=1)
    a = gamma.double() * r                                                        # [S, C]
    b = beta.double() - mean * a
    w = w.double()
    b32 = b @ w.T
    if bias is not None:
        b32 = b32 + bias.double()
    return w[None] * a[:, None, :], b32
