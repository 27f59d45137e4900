"""Inputs and fp64-oracle properties for the mask-propagation kernel tests (tests/test_gpu_maskprop.py on the GPU,
tests/test_maskprop_cases.py on the CPU).  TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

Everything a test needs to know about a case before the kernel runs — survivor counts, the gap at the top-k threshold, the share
of pixels whose arg-max is within rounding of a tie — is taken from oracle/maskprop_ref evaluated in float64, never from the code
under test.  Cases are built once per process (lru_cache) and must not be modified by their users.
"""
import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from . import maskprop_ref

T = 0.2                                   # the CLI's default temperature


# --------------------------------------------------------------------------- one propagation step: fp64 oracle
def ref_soft(src, tar, segs, topk, seed=1):
    """segs_tar of maskprop_ref.mask_propogation in float64 (src [Nsrc, C] rows, tar [hw, C], segs [ncls, Nsrc])."""
    torch.manual_seed(seed)
    return maskprop_ref.mask_propogation(src.double().T.contiguous(), tar.double(), segs.double(), T, topk)[0]


def ref_columns(src, tar, topk):
    """The thresholded, column-normalised affinity matrix [Nsrc, hw] of the fp64 oracle: its label product with the identity
    as labels.  exp() is never 0, so an entry is non-zero exactly where the oracle kept it."""
    with torch.random.fork_rng(devices=[]):
        return ref_soft(src, tar, torch.eye(src.shape[0], dtype=torch.float64), topk)


def ref_survivors(src, tar, topk):
    """entries the fp64 oracle keeps per target column (>= topk; more on a tie at the threshold) -> int64 [hw]"""
    return (ref_columns(src, tar, topk) != 0).sum(0)


def threshold_gap(src, tar, topk):
    """min over the columns of (a_k - a_{k+1}) / a_k for the k-th and (k+1)-th largest affinity of the fp64 oracle; None when
    there is no (k+1)-th entry.  (The oracle run with topk + 1 keeps both; the column normalisation cancels in the ratio.)"""
    if topk >= src.shape[0]:
        return None
    v = ref_columns(src, tar, topk + 1).sort(0, descending=True).values
    return ((v[topk - 1] - v[topk]) / v[topk - 1]).min().item()


def gap_bound(C):
    """worst-case fp32 rounding of two normalised C-term dot products, carried through exp(x / T)"""
    return 2 * (C + 4) * 2.0 ** -24 / T


def soft_tolerance(C, n_max):
    """|got - ref64| on a probability: C / T for the dot product's fp32 rounding carried through exp(x / T), n_max for the fp32
    sum of the survivors and the fma chain of the label product, 16 for expf, the division by T, the normalising division and
    the row normalisation; in units of 2^-23."""
    return (C / T + n_max + 16) * 2.0 ** -23


# --------------------------------------------------------------------------- lattice features: the survivor set is exact
def lattice_plans(topk):
    """(rows with cosine 1, 0.5, 0.25) towards one basis vector, per planned basis index"""
    return [(topk, 0, 0),          # exactly k, no tie
            (3, topk - 3, 0),      # k reached across two levels
            (topk + 1, 0, 0),      # a tie beyond k
            (10, 22, 0),           # 32 survivors: the longest compact list
            (10, 23, 0),           # 33: the first dense column
            (2, 5, 40),            # dense, three levels
            (1, 1, 1)]             # fewer than k above cosine 0: every source row ties at the threshold


def planned_survivors(plan, topk, Nsrc):
    tot = 0
    for n in plan:
        tot += n
        if tot >= topk:
            return tot
    return Nsrc


@functools.lru_cache(maxsize=None)
def lattice_case(C, topk, hw=200, Nsrc=700, ncls=5, zero_row=130, seed=3):
    """Target row i is the basis vector e_(i mod C) (row ``zero_row`` is all zeros: F.normalize's eps path).  A source row has
    1, 4 or 16 non-zeros of +-1 (norm 1, 2, 4); a planned row has +1 at its basis index c < P and the rest at indices >= P, a
    filler row lives at indices >= P only.  A dot product with a basis vector has one non-zero term, so equal-structure rows
    give bit-equal affinities in any arithmetic and the levels (cosine 1, 0.5, 0.25, 0, negative) are far apart."""
    g = torch.Generator().manual_seed(seed)
    plans = lattice_plans(topk)
    P = len(plans)

    def row(fixed, nnz):
        r = torch.zeros(C)
        idx = P + torch.randperm(C - P, generator=g)[:nnz - (fixed is not None)]
        r[idx] = torch.randint(0, 2, (len(idx),), generator=g).float() * 2 - 1
        if fixed is not None:
            r[fixed] = 1.0
        return r

    rows = [row(a, nnz) for a, plan in enumerate(plans) for nnz, n in zip((1, 4, 16), plan) for _ in range(n)]
    while len(rows) < Nsrc:
        rows.append(row(None, (1, 4, 16)[int(torch.randint(0, 3, (1,), generator=g))]))
    assert len(rows) == Nsrc
    src = torch.stack(rows)[torch.randperm(Nsrc, generator=g)].contiguous()
    tar = torch.zeros(hw, C)
    tar[torch.arange(hw), torch.arange(hw) % C] = 1.0
    tar[zero_row] = 0.0
    assert zero_row % C >= P
    segs = F.one_hot(torch.randint(0, ncls, (Nsrc,), generator=g), ncls).float().T.contiguous()
    cols = [[i for i in range(hw) if i % C == a and i != zero_row] for a in range(P)]
    surv = ref_survivors(src, tar, topk)
    return SimpleNamespace(src=src, tar=tar, segs=segs, C=C, topk=topk, plans=plans, cols=cols, zero_row=zero_row,
                           surv=surv, ref=ref_soft(src, tar, segs, topk))


LATTICE_CASES = [(48, 15), (48, 16), (50, 15), (50, 16)]        # C = 48: float4 loads, k-tail of 16; C = 50: scalar loads


# --------------------------------------------------------------------------- random features at ragged shapes
#               hw  Nsrc  C  ncls topk seed
RANDOM_CASES = [(200, 700, 70, 5, 15, 6),        # scalar loads, k-tail
                (200, 700, 40, 70, 16, 1),       # ncls > 64, transpose edges
                (130, 9, 36, 3, 9, 1),           # Nsrc < 16, topk == Nsrc
                (65, 300, 33, 5, 1, 1)]          # topk = 1, hw = 64 + 1


@functools.lru_cache(maxsize=None)
def random_case(hw, Nsrc, C, ncls, topk, seed):
    g = torch.Generator().manual_seed(seed)
    tar, src = torch.randn(hw, C, generator=g), torch.randn(Nsrc, C, generator=g)
    segs = F.one_hot(torch.randint(0, ncls, (Nsrc,), generator=g), ncls).float().T.contiguous()
    return SimpleNamespace(src=src, tar=tar, segs=segs, C=C, topk=topk, surv=ref_survivors(src, tar, topk),
                           gap=threshold_gap(src, tar, topk), ref=ref_soft(src, tar, segs, topk))


# --------------------------------------------------------------------------- finalize: upsample, norm_mask, arg-max
def smooth_field(ncls, h, w, seed, ctrl=(3, 5)):
    """smooth positive class fields [ncls, h, w] that sum to 1 over the classes: random control points, bicubic up, softmax"""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(1, ncls, *ctrl, generator=g)
    return torch.softmax(2.0 * F.interpolate(z, size=(h, w), mode="bicubic", align_corners=False)[0], dim=0).contiguous()


def finalize_ref(segs, H, W):
    """mask_propagation.py:60-69 in the dtype of ``segs`` [ncls, h, w] -> (uint8 {0, 255} mask [H, W], normalised field)"""
    up = F.interpolate(segs[None].clone(), size=(H, W), mode="bilinear", align_corners=False)[0]
    n = maskprop_ref.norm_mask(up)
    idx = torch.max(n, dim=0).indices
    return (idx != 0).to(torch.uint8) * 255, n


MARGIN = 1e-5             # see tests/test_gpu_maskprop.py::test_finalize_non_dyadic
#                   h   w    H    W  ncls seed
NON_DYADIC_CASES = [(34, 60, 270, 480, 5, 5), (17, 30, 135, 240, 7, 6)]


@functools.lru_cache(maxsize=None)
def non_dyadic_case(h, w, H, W, ncls, seed):
    segs = smooth_field(ncls, h, w, seed)
    mask32, _ = finalize_ref(segs, H, W)
    mask64, n64 = finalize_ref(segs.double(), H, W)
    top2 = n64.topk(2, dim=0).values
    return SimpleNamespace(segs=segs, mask32=mask32, mask64=mask64, near_tie=(top2[0] - top2[1]) < MARGIN)


# the norm_mask / arg-max edge classes, all 16 x 16 -> 128 x 128 (ratio 8: every interpolation weight is a multiple of 1/16, so a
# constant class stays bit-constant after the up-sampling and its min-max is exactly 0 / 0)
EDGE_CASES = ["zero_and_negative_class", "identical_classes_1_3", "identical_classes_0_2", "one_class", "first_mask_256",
              "constant_class_2", "constant_class_0"]


def edge_field(name, h=16, w=16):
    s = smooth_field(5, h, w, seed=2)
    if name == "zero_and_negative_class":          # max <= 0: norm_mask leaves both untouched
        s[1] = 0.0
        s[3] = -s[3]
    elif name == "identical_classes_1_3":          # the first of two equal maxima wins
        s[3] = s[1]
    elif name == "identical_classes_0_2":          # ... which is class 0 here: mask 0 wherever the pair leads
        s[2] = s[0]
    elif name == "one_class":                      # arg-max over one class: an all-zero mask
        s = s[:1].contiguous()
    elif name == "first_mask_256":                 # what a {0, 255} first mask produces: 256 classes, two of them populated
        f = torch.zeros(256, h, w)
        f[0], f[255] = s[0] + s[1], s[2] + s[3] + s[4]
        s = f
    elif name == "constant_class_2":               # 0 / 0 = NaN after the min-max; torch.max returns the first NaN's index
        s[2] = 0.5
    elif name == "constant_class_0":
        s[0] = 0.5
    else:
        raise KeyError(name)
    return s


def lattice_plan_report(case):
    """[(plan, survivors the plan says, survivor counts the fp64 oracle produced on the plan's columns)]"""
    Nsrc = case.src.shape[0]
    return [(p, planned_survivors(p, case.topk, Nsrc), sorted(set(case.surv[cols].tolist()))) for p, cols in zip(case.plans, case.cols)]
