"""A/B of the conv-module middle (everything between the two pointwise GEMMs: GLU + depthwise forward, norm + SiLU
forward, norm sums + norm-folded depthwise backward with its weight-gradient reduction) with GroupNorm(1, C)
against BatchNorm1d, on one MI355X in one process.  The legs alternate BN, GN, BN within every round, so the
two BatchNorm legs show the run-to-run spread a GN - BN difference has to exceed.  Shapes: Conformer-L at 15 s
(B 32, T 373) and at 60 s (B 8, T 1498), C 512, K 31, bf16.  HIP-event times, median over the rounds.
    python benchmarks/groupnorm_ab.py [calls per window] [rounds] [L15|L60]
(one shape alone: the target of a rocprofv3 --kernel-trace --stats run, profiles/group_norm/kernel_trace.txt)"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nn_conformer_for_speech_recognition_amd import ops  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 300
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 9
SHAPES = [s for s in (("L15", 32, 373), ("L60", 8, 1498)) if len(sys.argv) <= 3 or s[0] == sys.argv[3]]
C, K = 512, 31
bf = torch.bfloat16
if not torch.cuda.is_available():
    raise SystemExit("groupnorm_ab.py needs the GPU: no timing without one")


def legs(B, T):
    g = torch.Generator().manual_seed(0)
    a = torch.randn(B * T, 2 * C, generator=g).to("cuda", bf)
    w = (0.1 * torch.randn(C, K, generator=g)).cuda()
    bias = (0.1 * torch.randn(C, generator=g)).cuda()
    gamma = (1 + 0.1 * torch.randn(C, generator=g)).cuda()
    beta = (0.1 * torch.randn(C, generator=g)).cuda()
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    dz = torch.randn(B * T, C, generator=g).to("cuda", bf)
    ws = ops.convmod_ws(B, T, C, K, "cuda")

    def bn_fwd():
        y = ops.glu_dwconv_fwd(a, w, bias, B, T, C, K, ws)
        return (y,) + ops.bn_silu_fwd(y, gamma, beta, rm, rv, 0.1, 1e-5, True, B, T, C, ws, bf)

    def bn_bwd(s):
        y, _, mean, inv = s
        return ops.bn_silu_glu_dwconv_bwd(dz, y, gamma, beta, mean, inv, True, a, w, B, T, C, K, ws, bf)

    def gn_fwd():
        y = ops.glu_dwconv_fwd(a, w, bias, B, T, C, K, ws)
        return (y,) + ops.gn_silu_fwd(y, gamma, beta, 1e-5, B, T, C, ws, bf)

    def gn_bwd(s):
        y, _, mean, rstd = s
        return ops.gn_silu_glu_dwconv_bwd(dz, y, gamma, beta, mean, rstd, a, w, B, T, C, K, ws, bf)

    return [("BN a", bn_fwd, bn_bwd), ("GN", gn_fwd, gn_bwd), ("BN b", bn_fwd, bn_bwd)]


def window(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(N):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / N * 1e3


print(f"conv-module middle, C {C} K {K} bf16, {N} calls per window, median of {ROUNDS} rounds (min .. max), us per call")
for name, B, T in SHAPES:
    ls = legs(B, T)
    for _, fwd, bwd in ls:          # warm-up: code objects, allocator
        for _ in range(10):
            bwd(fwd())
    torch.cuda.synchronize()
    t = {leg: {"fwd": [], "bwd": []} for leg, _, _ in ls}
    for _ in range(ROUNDS):
        for leg, fwd, bwd in ls:
            saved = fwd()
            t[leg]["fwd"].append(window(fwd))
            t[leg]["bwd"].append(window(lambda: bwd(saved)))
    med = {}
    for leg, _, _ in ls:
        f, b = t[leg]["fwd"], t[leg]["bwd"]
        tot = [x + y for x, y in zip(f, b)]
        med[leg] = statistics.median(tot)
        print(f"{name} B {B} T {T}  {leg:5s} fwd {statistics.median(f):7.1f} ({min(f):.1f} .. {max(f):.1f})  "
              f"bwd {statistics.median(b):7.1f} ({min(b):.1f} .. {max(b):.1f})  "
              f"fwd+bwd {med[leg]:7.1f} ({min(tot):.1f} .. {max(tot):.1f})")
    bn = 0.5 * (med["BN a"] + med["BN b"])
    print(f"{name} GN - BN {med['GN'] - bn:+.1f} us ({(med['GN'] / bn - 1) * 100:+.1f} %), "
          f"spread between the BN legs {abs(med['BN a'] - med['BN b']):.1f} us")
