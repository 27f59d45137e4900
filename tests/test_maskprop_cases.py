"""CPU: the inputs of tests/test_gpu_maskprop.py are what that file says they are.  Every property here is read off
oracle/maskprop_ref in float64 (oracle/maskprop_cases.py), so the GPU tests cannot degrade silently when a builder, a seed or a
shape is edited: the survivor count of every planned lattice column, the gap at the top-k threshold of every random case, the
share of near-tie pixels of the non-dyadic finalize inputs, and the oracle's own answer on the norm_mask edge classes."""
import pytest
import torch

from oracle import maskprop_ref, maskprop_cases as mc


def _fp32_oracle_error(case):
    torch.manual_seed(1)
    r32 = maskprop_ref.mask_propogation(case.src.T.contiguous(), case.tar, case.segs, mc.T, case.topk)[0]
    return (r32.double() - case.ref).abs().max().item()


@pytest.mark.parametrize("C,topk", mc.LATTICE_CASES)
def test_lattice_survivor_counts_are_the_planned_ones(C, topk):
    c = mc.lattice_case(C, topk)
    Nsrc = c.src.shape[0]
    report = mc.lattice_plan_report(c)
    for plan, planned, actual in report:
        assert actual == [planned], (plan, planned, actual)
    planned = [p for _, p, _ in report]
    assert planned[:2] == [topk, topk] and planned[2] == topk + 1                      # exactly k (one and two levels), one tie beyond k
    assert planned[3:] == [32, 33, 47, Nsrc]                                             # longest compact list, first dense column, dense, mass tie
    assert int(c.surv[c.zero_row]) == Nsrc                                               # a zero target row keeps every source ...
    assert (c.ref[:, c.zero_row] - c.segs.double().mean(1)).abs().max().item() < 1e-15   # ... and returns the class frequencies
    for b in range(0, c.tar.shape[0], 64):                                               # dense and compact columns share every 64-column block
        blk = c.surv[b:b + 64]
        assert (blk <= 32).any() and (blk > 32).any(), b
    assert int(c.surv.min()) >= topk
    # the tolerance the GPU test applies is not tighter than the reference's own fp32 error (observed 1.4e-7)
    assert _fp32_oracle_error(c) <= mc.soft_tolerance(C, int(c.surv.max()))


@pytest.mark.parametrize("hw,Nsrc,C,ncls,topk,seed", mc.RANDOM_CASES)
def test_random_cases_keep_clear_of_the_threshold(hw, Nsrc, C, ncls, topk, seed):
    c = mc.random_case(hw, Nsrc, C, ncls, topk, seed)
    if topk < Nsrc:
        assert c.gap > mc.gap_bound(C), (c.gap, mc.gap_bound(C))
    else:
        assert c.gap is None and int(c.surv.min()) == Nsrc                               # no (k + 1)-th entry: every source survives
    assert int(c.surv.min()) == int(c.surv.max()) == topk                                # random features: no ties
    assert _fp32_oracle_error(c) <= mc.soft_tolerance(C, topk)


@pytest.mark.parametrize("h,w,H,W,ncls,seed", mc.NON_DYADIC_CASES)
def test_non_dyadic_inputs_have_few_near_ties(h, w, H, W, ncls, seed):
    c = mc.non_dyadic_case(h, w, H, W, ncls, seed)
    assert c.near_tie.float().mean().item() <= 1e-3
    assert 0.5 < (c.mask32 != 0).float().mean().item() < 0.95                            # an all-zero or all-255 output cannot pass
    assert not ((c.mask32 != c.mask64) & ~c.near_tie).any()                              # the fp32 oracle itself obeys the exclusion rule
    assert (c.segs[:, 1:] - c.segs[:, :-1]).abs().max() < 1 and (c.segs[:, :, 1:] - c.segs[:, :, :-1]).abs().max() < 1   # slope per source pixel


@pytest.mark.parametrize("name", mc.EDGE_CASES)
def test_edge_fields_oracle_semantics(name):
    s = mc.edge_field(name)
    mask, n = mc.finalize_ref(s, 128, 128)
    fg = (mask != 0).float().mean().item()
    if name == "zero_and_negative_class":
        up = torch.nn.functional.interpolate(s[None], size=(128, 128), mode="bilinear", align_corners=False)[0]
        assert torch.equal(n[1], up[1]) and torch.equal(n[3], up[3]) and n[3].max() < 0  # left unscaled
        assert 0.05 < fg < 0.95
    elif name == "identical_classes_1_3":
        idx = n.max(dim=0).indices
        assert (idx == 1).any() and not (idx == 3).any() and 0.05 < fg < 0.95
    elif name == "identical_classes_0_2":
        idx = n.max(dim=0).indices
        assert (idx == 0).any() and not (idx == 2).any() and 0.05 < fg < 0.95
        assert ((idx == 0) & (n[0] == n[2])).any()                                       # a last-maximum rule would answer 255 there
    elif name == "one_class":
        assert fg == 0.0
    elif name == "first_mask_256":
        assert 0.05 < fg < 0.95
    elif name == "constant_class_2":
        assert torch.isnan(n[2]).all() and fg == 1.0                                     # the first NaN's index: class 2 everywhere
    elif name == "constant_class_0":
        assert torch.isnan(n[0]).all() and fg == 0.0
