"""Replays tests/data/dispatch_plan.txt on a GPU: every row that a stand-alone operator can express runs ONCE as a real call on zero
inputs, with a delay_us(1) marker kernel between rows, so that a kernel trace of this script lists per row what was launched:

    rocprofv3 --kernel-trace --output-format csv -d build/sweep -- python tools/dispatch_sweep.py
    UNIVST_LIB=/path/to/another/libunivst_hip.so rocprofv3 ... (the same table through another build of the library)
    python tools/dispatch_sweep.py --check build/sweep        # the trace against the table's expected column, row for row

Rows only the UNet graph / RAFT can express (GroupNorm statistics out, caller-held workspace, both weight copies, a misaligned output) and
the error rows are skipped; `--list` prints the rows that run."""
import csv
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BIAS, RES, ROWBIAS, LN_STATS, STATS_OUT, ACT, GATE, W32_ONLY, W32, GN_OUT, TAPINNER, Y_UNALIGNED, WORKSPACE = (1 << i for i in range(13))
GRAPH_ONLY = W32 | GN_OUT | Y_UNALIGNED | WORKSPACE


def rows():
    for line in open(os.path.join(ROOT, "tests", "data", "dispatch_plan.txt")):
        if line.strip() and not line.startswith("#"):
            left, want = line.rstrip("\n").split(" | ", 1)
            kind, *a = left.split()
            a = [int(x) for x in a]
            if " grid=" not in want:
                continue
            if kind == "gemm" and (a[6] & GRAPH_ONLY or a[15] != 0 or (a[1] == 1 and a[6] & (LN_STATS | STATS_OUT | ACT | GATE))):
                continue            # (explicit conv geometries exist inside the VAE only)
            if kind == "gemm" and a[1] == 0:    # the C ABI asks the graph's predicates first: rows they refuse cannot be called stand-alone
                pred = dict(re.findall(r"(\w+)=(\d)", want))
                ln_ok = a[5] == 2 or pred["geglu_consumer" if a[5] else "fold_consumer"] == "1"
                if (a[6] & LN_STATS and not ln_ok) or (a[6] & STATS_OUT and pred["fold_producer"] == "0") or (a[7] and pred["big_direct"] == "0"):
                    continue
            yield kind, a, want


def run():
    import torch
    from univst_amd import _native as nat
    z = lambda *s, dt=torch.float16: torch.zeros(*s, device="cuda", dtype=dt)
    for kind, a, _ in rows():
        if kind == "gemm":
            _, mode, M, N, K, geglu, fl, sets, C1, C2, Hs, Ws, up, stride, taps, _ = a
            bias = z(N) if fl & BIAS else None
            if mode == 0:
                No = N // 2 if geglu else N
                x, res = z(M, K), (z(M, No) if fl & RES else None)
                if sets:
                    nat.linear_sets(x, z(M // sets, N, K), z(M // sets, N, dt=torch.float32), sets, residual=res,
                                    stats_out=z(M, N // 160, 2, dt=torch.float32) if fl & STATS_OUT else None)
                elif fl & (LN_STATS | STATS_OUT):
                    f32 = lambda *s: z(*s, dt=torch.float32)
                    nat.linear_ln(x, z(N, K), bias=bias, residual=res, geglu=geglu, ln=(f32(M, K // 160, 2), f32(N), f32(N)) if fl & LN_STATS else None,
                                  stats_out=f32(M, N // 160, 2) if fl & STATS_OUT else None)
                elif fl & (ACT | GATE):
                    nat.linear_gated(x, z(N, K), bias=bias, residual=res, act=nat.ACT_GELU_TANH if fl & ACT else None, gate=z(1, N) if fl & GATE else None,
                                     rows_per_gate=M)
                else:
                    nat.linear(x, z(N, K), bias=bias, residual=res, geglu=geglu)
            else:
                imgs, Cout = M, N
                He, We = Hs << up, Ws << up
                Ho, Wo = (He - 1) // stride + 1, (We - 1) // stride + 1
                kw = dict(bias=bias, x2=z(imgs, Hs, Ws, C2) if C2 else None, rowbias=z(1, Cout) if fl & ROWBIAS else None, rows_per_rowbias=imgs * Ho * Wo,
                          residual=z(imgs, Ho, Wo, Cout) if fl & RES else None)
                x1 = z(imgs, Hs, Ws, C1)
                if fl & W32_ONLY:
                    nat.conv3x3_patch(x1, z(Cout, (C1 + C2) // 32, 9, 32), upsample=bool(up), **kw)
                elif fl & TAPINNER:
                    nat.conv_nhwc_tapinner(x1, z(Cout, (C1 + C2) // 64, 9, 64), upsample=bool(up), stride=stride, **kw)
                else:
                    nat.conv_nhwc(x1, z(Cout, taps, C1 + C2), upsample=bool(up), stride=stride, **kw)
        else:
            BF, heads, Nq, Nkv, nsrc, d, pre, fl, phase = a
            if fl & 2:
                continue            # the extra key segment has no stand-alone operator (univst_sd3_joint_attention builds it)
            q, kv = z(BF, Nq, heads * d), z(BF, Nkv, heads * d)
            idx = (torch.arange(BF, device="cuda", dtype=torch.int32)[:, None] - torch.arange(nsrc, device="cuda", dtype=torch.int32)[None]).clamp_(min=0).contiguous()
            logw = z(BF, nsrc, dt=torch.float32) if fl & 1 else None
            if phase == 0:
                nat.attention(q, kv, kv, idx, heads, src_logw=logw, q_prescaled=bool(pre))
            else:
                cnt = torch.full((BF,), nsrc, device="cuda", dtype=torch.int32)
                st = z(BF, heads, Nq, 2, dt=torch.float32)
                nat.attention_phase(q, kv, kv, idx, cnt, heads, out=z(BF, Nq, heads * d), state_out=st if phase == 1 else None, state_in=st if phase == 2 else None,
                                    src_logw=logw, q_prescaled=bool(pre))
        nat.check(nat.load().univst_debug_delay_us(1.0, nat.stream_ptr()), "delay_us")
    torch.cuda.synchronize()


def check(root):
    """the trace, cut at the marker kernels, against the expected column: (symbol, blocks, threads[, reduction]) per row"""
    recs = []
    for f in glob.glob(root + "/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            recs.append((int(r["Start_Timestamp"]), r["Kernel_Name"], int(r["Grid_Size_X"]) // max(int(r["Workgroup_Size_X"]), 1), int(r["Workgroup_Size_X"])))
    mangled = sorted({r[1] for r in recs if r[1].startswith("_Z")})
    if mangled:
        import subprocess
        plain = subprocess.run(["c++filt"], input="\n".join(n.replace(".kd", "") for n in mangled), capture_output=True, text=True, check=True).stdout.split("\n")
        names = dict(zip(mangled, plain))
        recs = [(t, names.get(n, n), g, b) for t, n, g, b in recs]
    recs.sort()
    groups, cur = [], []
    for _, name, g, b in recs:
        if "delay" in name:
            groups.append(cur)
            cur = []
        elif re.search(r"(gemm|geglu_xres|conv_patch|attn)[a-z0-9_]*kernel|splitk_reduce", name) and "permute" not in name:
            cur.append((re.sub(r"\s+", "", re.sub(r"^.*?([a-z0-9_]+kernel[a-z0-9_]*)(<[^(]*>)?\(.*$", r"\1\2", name)), g, b))
    want_rows = list(rows())
    want_rows = [w for w in want_rows if not (w[0] == "attn" and w[1][7] & 2)]
    bad = 0
    if len(groups) != len(want_rows):
        print(f"{len(groups)} marker-delimited groups in the trace, {len(want_rows)} rows ran")
        bad += 1
    for (kind, a, want), got in zip(want_rows, groups):
        m = re.match(r"(\S+) grid=(\d+) block=(\d+) splits=\d+( \+splitk_reduce)?", want)
        exp = [(m.group(1), int(m.group(2)), int(m.group(3)))] + ([("splitk_reduce_kernel",)] if m.group(4) else [])
        # a trace spells default template arguments out or not, as the compiler printed them: compare the family and the leading arguments
        ok = len(got) == len(exp) and got[0][1:] == exp[0][1:] and exp[0][0].split("<")[0] == got[0][0].split("<")[0] and \
            exp[0][0].rstrip(">").startswith(got[0][0].rstrip(">").replace("(anonymousnamespace)::", ""))
        if not ok:
            bad += 1
            print("MISMATCH", kind, a, "expected", exp, "traced", got)
    print(f"{len(want_rows)} rows, {bad} mismatches")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--list":
        for r in rows():
            print(*r)
    elif len(sys.argv) > 2 and sys.argv[1] == "--check":
        sys.exit(check(sys.argv[2]))
    else:
        run()
