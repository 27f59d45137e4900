"""GPU: every launch route of uv_launch_groupnorm (csrc/norm.hip) that the C ABI reaches on one GPU, at ragged shapes, element by element
against float64 (oracle/groupnorm_ref.py) — the one-launch kernel, the streaming three at every block geometry the UNet and the VAE use
(TR = 64 .. 1, the C / 8 > 256 block, the 512-chunk cap, chunks with fewer rows than thread-rows), and the fold tail.  The cases, their
sentinel rows and what each is for: oracle/groupnorm_cases.py; that they take the routes they are named for, and that one dropped or
double-counted sentinel row moves the output by more than 8 bounds: tests/test_groupnorm_cases.py (no GPU).

The bound follows the kernels' arithmetic.  With r = 1 / sqrt(sigma^2 + eps), z the pre-activation reference and rho = |mean| / sigma of the
element's group:

    pre   = [(|x| + |mean|) r |gamma| + |beta|] * 8 * 2^-24
          + |z - beta| (rho^2 + 8) 2^-25
    bound = 1.1 pre + 2^-11 |ref| + 2^-25

First line: gn_apply_kernel / gn_small_kernel compute sc = fl(rstd gamma), y = fl(fl(x - mean) sc + beta) in fp32 from an fp32 mean: each
rounding is 2^-24 of a term no larger than (|x| + |mean|) r |gamma| + |beta|, there are fewer than 8 of them.  (The kernels used to compute
x sc + fl(beta - mean sc); that met this bound too, but left a constant group 6.7 fp16 steps from beta on the streaming route, where the
case below asks for one: the rounding of beta - mean sc is the size of |mean| r, not of beta.)  Second line: the
statistics are exact up to the fp32 store of (sum, sumsq) — the pivoted sums are recombined in double — and the variance is sumsq / n - mean^2,
so the one rounding of sumsq is a relative variance error of (1 + rho^2) 2^-24 (the limit the comment at the top of gn_partial_kernel states),
half of that on rstd, and rstd multiplies z - beta; the + 8 holds the fp32 rounding of rstd itself and of the products above as they act on
z - beta.  Third line: SiLU has slope <= 1.1, the store rounds to the nearest fp16 (2^-11 relative, half the smallest subnormal step absolute).
The reference is float64 on the same fp16 inputs; the ratio err / bound is never taken against the kernel's own output.

Every test prints its figures (pytest -s) before it asserts and repeats them in the assertion message."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import groupnorm_cases as gc  # noqa: E402
from oracle.groupnorm_ref import fold_linear_ref  # noqa: E402


def _run(b):
    from univst_amd import _native
    c = b.case
    out = _native.groupnorm_nhwc(b.x1.cuda(), b.gamma.cuda(), b.beta.cuda(), c.G, c.eps, c.rps, silu=c.silu, x2=None if b.x2 is None else b.x2.cuda())
    torch.cuda.synchronize()
    return out.cpu()


def _fp16_step(v):
    """spacing of the fp16 numbers at |v| (float64 tensor)"""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14)))
    return 2.0 ** (e - 10)


@pytest.mark.parametrize("name", list(gc.CASES))
def test_groupnorm_case_against_float64(name):
    """One case of oracle/groupnorm_cases.CASES: the route it is named for, two identical runs, max(err / bound) <= 1 against float64.
    Where the fp16 store dominates, the ratio sits just under 1 by construction (2^-11 |ref| is the store's worst case): an fp32 emulation
    of the streaming arithmetic on the CPU gives 0.93 .. 0.996 for cases 1, 4, 7, 8 and 0.74 for the large-mean case."""
    b = gc.build(name)
    c = b.case
    assert {k: b.plan[k] for k in gc.EXPECT[name]} == gc.EXPECT[name], b.plan          # the route this case is here for
    got = _run(b)
    again = _run(b)
    assert got.shape == b.ref.out.shape and got.dtype == torch.float16
    assert torch.equal(got, again), f"{name}: two runs of the same call differ"       # norm.hip: fixed reduction orders
    err = (got.double() - b.ref.out).abs()
    ratio = err / gc.bound(b)
    worst = int(ratio.argmax())
    row, col = divmod(worst, c.C1 + c.C2)
    msg = (f"{name}: max(err / bound) = {ratio.max().item():.3f} at row {row} (unit {row // c.rps}, row {row % c.rps}) channel {col}: got {got[row, col].item():.6g}, "
           f"ref {b.ref.out[row, col].item():.6g}; max err {err.max().item():.3e}; route {b.plan['route']} TR {b.plan['TR']} nchunk {b.plan['nchunk']} x {b.plan['rpc']}")
    print(msg)
    assert torch.isfinite(got).all(), msg
    assert ratio.max().item() <= 1.0, msg
    if c.values == "const_group":        # the group's output is beta (through SiLU): within one fp16 step of it
        cpg = (c.C1 + c.C2) // c.G
        cols = slice(gc.CONST_GROUP * cpg, (gc.CONST_GROUP + 1) * cpg)
        want = b.beta.double()[cols]
        want = want * torch.sigmoid(want) if c.silu else want
        off = ((got[:, cols].double() - want).abs() / _fp16_step(want)).max().item()
        print(f"{name}: constant group, max |got - act(beta)| = {off:.3f} fp16 steps")
        assert off <= 1.0, f"{name}: constant group is {off:.3f} fp16 steps from act(beta)"


def test_fold_tail_against_float64():
    """gn_fold_linear_kernel behind the streaming statistics of case 1 (TR = 6, ragged last chunk), N = 37 (no multiple of the 4 rows per block).
    W_sets: the fp16 store and the rstd term, 2^-11 |ref| + |ref| (rho^2 + 8) 2^-25.  bias32: an fp32 sum of C products w * b_k in a fixed
    lane order, C max|w b_k| 2^-23, plus what the fp32 mean and rstd do to b_k = beta_k - mean gamma_k r:
    sum_k |w| |mean gamma_k r| (8 * 2^-24 + (rho^2 + 8) 2^-25)."""
    from univst_amd import _native
    b = gc.build("c01_tr6_ragged_last_chunk")
    c = b.case
    C, cpg = c.C1, c.C1 // c.G
    w, bias = gc.fold_weights(C)
    call = lambda: [t.cpu() for t in _native.groupnorm_fold_linear(b.x1.cuda(), b.gamma.cuda(), b.beta.cuda(), c.G, c.eps, c.rps, w.cuda(), bias.cuda())]
    wsets, b32 = call()
    wsets2, b32_2 = call()
    assert torch.equal(wsets, wsets2) and torch.equal(b32, b32_2), "two runs of the same call differ"
    ref_w, ref_b = fold_linear_ref(b.x1, b.gamma, b.beta, c.G, c.eps, c.rps, w, bias)
    assert wsets.shape == ref_w.shape == (c.S, gc.FOLD_N, C) and b32.shape == ref_b.shape == (c.S, gc.FOLD_N)
    mean, sigma = (t.repeat_interleave(cpg, dim=1) for t in (b.ref.mean, b.ref.sigma))          # [S, C]
    rstd_rel = ((mean / sigma) ** 2 + 8.0) * 2.0 ** -25
    r = 1.0 / torch.sqrt(sigma ** 2 + c.eps)
    bound_w = 2.0 ** -11 * ref_w.abs() + ref_w.abs() * rstd_rel[:, None, :]
    shift = (mean * b.gamma.double() * r).abs()                                                  # [S, C]
    bk = b.beta.double() - mean * b.gamma.double() * r
    wd = w.double().abs()
    bound_b = C * (wd[None] * bk.abs()[:, None, :]).amax(dim=2) * 2.0 ** -23 + (shift * (8 * 2.0 ** -24 + rstd_rel)) @ wd.T
    rw = ((wsets.double() - ref_w).abs() / bound_w).max().item()
    rb = ((b32.double() - ref_b).abs() / bound_b).max().item()
    msg = f"fold tail: max(err / bound) W_sets {rw:.3f}, bias32 {rb:.3f}"
    print(msg)
    assert torch.isfinite(wsets).all() and torch.isfinite(b32).all(), msg
    assert rw <= 1.0 and rb <= 1.0, msg
