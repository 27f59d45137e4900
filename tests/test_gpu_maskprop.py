"""GPU: csrc/maskprop.hip on the paths the square, ratio-8, random-feature tests never reach — ties at the top-k threshold, the
32 / 33 survivor boundary between the compact lists and the dense fallback, scalar loads and k-tails of the affinity GEMM, short
source lists, more than 64 classes, non-square and non-dyadic up-sampling, and norm_mask's edge classes (NaN included).

Soft labels are compared with oracle/maskprop_ref run in float64 under a derived bound (oracle/maskprop_cases.soft_tolerance):
    |got - ref64| <= (C / T + n_max + 16) * 2^-23,        n_max = the largest survivor count of the case (from the oracle)
— three orders of magnitude below the 1 / (n + 1) a wrong survivor set moves a label by.  Masks are compared bit for bit with the
fp32 oracle, except at a non-dyadic ratio (see test_finalize_non_dyadic).  What each case is built to contain is asserted from the
fp64 oracle alone, here and without a GPU in tests/test_maskprop_cases.py.  Every test prints its figures (pytest -s) before it
asserts and repeats them in the assertion message.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import maskprop_ref, maskprop_cases as mc, synth_inputs as si  # noqa: E402


def _args(**kw):
    from univst_amd.src import mask_propagation as mp
    a = mp.build_parser().parse_args([])
    assert a.temperature == mc.T
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _frame(c, topk=None):
    from univst_amd.src import mask_propagation as mp
    torch.manual_seed(1)                      # the oracle side (mc.ref_soft) seeds the host generator identically: both call torch.randperm
    got, _, _ = mp.mask_propogation(c.src.cuda(), c.tar.cuda(), c.segs.cuda(), _args(topk=c.topk if topk is None else topk))
    return got.cpu()


def _check_soft(tag, c, got):
    n_max = int(c.surv.max())
    tol = mc.soft_tolerance(c.C, n_max)
    err = (got.double() - c.ref).abs().max().item()
    msg = (f"{tag}: max|got - ref64| = {err:.3e}, bound {tol:.3e} (n_max {n_max}); {int((c.surv <= 32).sum())} compact + "
           f"{int((c.surv > 32).sum())} dense columns")
    print(msg)
    assert got.shape == c.ref.shape and torch.isfinite(got).all(), msg
    assert err <= tol, msg
    # a one-hot label row is exactly 0 where no survivor carries it, in any arithmetic (this decides the fore / background split)
    assert torch.equal(got == 0, c.ref == 0), msg


@pytest.mark.parametrize("C,topk", mc.LATTICE_CASES)
def test_lattice_ties_and_dense_fallback(C, topk):
    """Part 1: features whose survivor set is decided by exact arithmetic on both sides (mc.lattice_case).
    Observed on an MI355X, max|got - ref64| against the bound 1.14e-4 / 1.15e-4 (n_max 700), compact + dense columns:
    C=48 topk=15 7.1e-7 (68 + 132), C=48 topk=16 9.0e-7 (48 + 152), C=50 topk=15 6.8e-7 (88 + 112), C=50 topk=16 7.8e-7 (68 + 132)."""
    c = mc.lattice_case(C, topk)
    for plan, planned, actual in mc.lattice_plan_report(c):
        assert actual == [planned], (plan, planned, actual)
    assert {32, 33} <= set(c.surv[:64].tolist())                 # both sides of the compact / dense boundary inside one 64-column block
    got = _frame(c)
    again = _frame(c)
    assert torch.equal(got, again), "two runs of the same frame differ"
    _check_soft(f"lattice C={C} topk={topk}", c, got)
    zr = (got[:, c.zero_row].double() - c.segs.double().mean(1)).abs().max().item()
    assert zr <= mc.soft_tolerance(C, c.src.shape[0]), f"zero target row vs class frequencies: {zr:.3e}"


@pytest.mark.parametrize("hw,Nsrc,C,ncls,topk,seed", mc.RANDOM_CASES)
def test_random_features_ragged_shapes(hw, Nsrc, C, ncls, topk, seed):
    """Part 2: random features where hw, Nsrc, C, ncls are no multiples of the kernels' tiles.  The fp64 oracle's gap between the
    k-th and (k + 1)-th affinity of every column exceeds the fp32 rounding of the affinities, so both sides keep the same set.
    Observed on an MI355X (all columns compact), max|got - ref64| / bound in table order: 9.9e-8 / 4.5e-5, 8.3e-8 / 2.8e-5,
    1.5e-7 / 2.4e-5, 0 / 2.2e-5."""
    c = mc.random_case(hw, Nsrc, C, ncls, topk, seed)
    assert c.gap is None or c.gap > mc.gap_bound(C), (c.gap, mc.gap_bound(C))
    got = _frame(c)
    assert torch.equal(got, _frame(c))
    _check_soft(f"random hw={hw} Nsrc={Nsrc} C={C} ncls={ncls} topk={topk}", c, got)


@pytest.mark.parametrize("topk,Nsrc", [(17, 700), (12, 9), (0, 9)])
def test_bad_topk_is_a_loud_error(topk, Nsrc):
    c = mc.random_case(130, 9, 36, 3, 9, 1) if Nsrc == 9 else mc.random_case(200, 700, 70, 5, 15, 6)
    with pytest.raises(RuntimeError, match="topk"):
        _frame(c, topk=topk)
    _check_soft("after the error", c, _frame(c))                  # the library is still usable


def test_no_classes_is_a_loud_error():
    from types import SimpleNamespace
    c = mc.random_case(130, 9, 36, 3, 9, 1)
    with pytest.raises(RuntimeError, match="maskprop_frame"):          # an empty label tensor has no storage: the ABI layer or the launcher refuses
        _frame(SimpleNamespace(src=c.src, tar=c.tar, segs=c.segs[:0], topk=9))


# --------------------------------------------------------------------------- finalize
def _finalize(segs, H, W):
    from univst_amd.src import mask_propagation as mp
    ncls, h, w = segs.shape
    out = mp.norm_argmax_mask(segs.reshape(ncls, h * w).cuda(), h, w, H, W)
    assert out.shape == (H, W) and out.dtype == torch.uint8
    return out.cpu()


@pytest.mark.parametrize("h,w,H,W", [(12, 20, 96, 160), (12, 20, 12, 20)])
def test_finalize_non_square_bit_exact(h, w, H, W):
    """Part 3: h != w and H != W at ratio 8 and at ratio 1 (no up-sampling); smooth positive fields; bit-exact."""
    segs = mc.smooth_field(5, h, w, seed=3)
    ref, _ = mc.finalize_ref(segs, H, W)
    assert 0.05 < (ref != 0).float().mean().item() < 0.95
    got = _finalize(segs, H, W)
    diff = int((got != ref).sum())
    assert diff == 0, f"{diff} of {H * W} mask pixels differ from the fp32 oracle"


@pytest.mark.parametrize("h,w,H,W,ncls,seed", mc.NON_DYADIC_CASES)
def test_finalize_non_dyadic(h, w, H, W, ncls, seed):
    """Part 3: a ratio that is no power of two.  The compiler may contract (y + 0.5) * scale - 0.5 into an fma where torch's CPU
    kernel rounds twice: the source coordinate (at most 60) then differs by 1 ulp, about 4e-6; times a field slope below 1 per
    source pixel, plus a few ulp of the normalisation, that stays under 1e-5.  So a pixel may differ from the fp32 oracle only
    where the fp64 oracle's margin between its two largest normalised classes is below 1e-5 (mc.MARGIN), and at most 0.1 % of the
    pixels may be such (a condition on the inputs).  Every other pixel must match.
    Observed on an MI355X: 0 differing pixels on both inputs (excluded shares 2.3e-5 and 3.1e-5: 3 and 1 pixels)."""
    c = mc.non_dyadic_case(h, w, H, W, ncls, seed)
    share = c.near_tie.float().mean().item()
    assert share <= 1e-3, share
    assert 0.5 < (c.mask32 != 0).float().mean().item() < 0.95
    diff = _finalize(c.segs, H, W) != c.mask32
    msg = (f"({h}, {w}) -> ({H}, {W}) ncls={ncls}: {int(diff.sum())} differing pixels, {int((diff & ~c.near_tie).sum())} of them outside the "
           f"excluded share {share:.2e} ({int(c.near_tie.sum())} pixels)")
    print(msg)
    assert not (diff & ~c.near_tie).any(), msg


@pytest.mark.parametrize("name", mc.EDGE_CASES)
def test_finalize_edge_classes_bit_exact(name):
    """Part 3: norm_mask's edge classes (mc.edge_field) at (16, 16) -> (128, 128), bit-exact.  A constant positive class is NaN
    after the reference's min-max and torch.max returns the first NaN's index: that class takes every pixel."""
    segs = mc.edge_field(name)
    ref, _ = mc.finalize_ref(segs, 128, 128)
    if name.startswith("constant_class"):
        assert set(ref.unique().tolist()) == ({255} if name == "constant_class_2" else {0})
    got = _finalize(segs, 128, 128)
    diff = int((got != ref).sum())
    assert diff == 0, f"{name}: {diff} of {128 * 128} mask pixels differ from the fp32 oracle"


def test_non_square_chain_bit_exact():
    """Part 4: a 4-frame clip of 12 x 20 features (C = 40) with a 96 x 160 first mask through propagate_masks vs the live fp32
    oracle on the same host random stream; masks bit-exact."""
    from univst_amd.src import mask_propagation as mp
    feats = si.maskprop_features(F=4, h=12, w=20, C=40)
    first = si.soft_first_mask(96, 160)
    torch.manual_seed(33)
    masks = mp.propagate_masks(feats, first, _args(num_frames=4))
    torch.manual_seed(33)
    ref = maskprop_ref.video_mask_propagation(feats, first, num_frames=4)
    assert len(masks) == len(ref) == 4 and all(m.shape == (96, 160) for m in masks)
    diff = [int((a != b).sum()) for a, b in zip(masks, ref)]
    assert diff == [0, 0, 0, 0], f"mask pixels differing from the oracle, per frame: {diff}"
    assert all(0.02 < (np.asarray(m) != 0).mean() < 0.98 for m in ref[1:])
