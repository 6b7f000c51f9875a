"""The device RNN-T loss (transducer.rnnt_loss: csrc/rnnt.hip) beside a restatement in torch device ops -- what a user
without this kernel writes today: log_softmax, two gathers and a Python loop over the lattice's anti-diagonals, the
gradient by autograd.  Forward + backward per call, on the same seeded inputs in the same process.

Shapes:
  words   B 32, T 373, U1 9,  V 64      the encoder length of the flagship workload, transcripts of a few words
  pieces  B 4,  T 373, U1 41, V 1024    forty word pieces over a 1024-entry vocabulary

Arms per shape (device events; eager launches and the output / workspace allocations included):
  kernel  rnnt_loss(reduction='sum') + backward: rnnt_prep, rnnt_lattice, rnnt_grad
  torch   the restatement below, forward + backward
Median and minimum over --rounds of the mean of --iters calls, the arms alternating within a round.

The kernels' algorithmic HBM traffic is 3 * B * T * U1 * V * 4 bytes (the logits read by rnnt_prep and by rnnt_grad,
the gradient written once); "hbm_share" is that over the call's time over the 8.0 TB/s HBM3E peak of the MI355X.  It is
an END-TO-END share of the forward + backward call (launch gaps, the lattice recursion and the autograd bookkeeping
included), not a kernel's share of peak; per-kernel times come from a profiler run of their own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o words -- \\
        python benchmarks/rnnt_loss.py --kernel-only --rounds 1 --iters 5 --shapes words

One JSON line on stdout; --out also writes a text table (the table of profiles/rnnt/times.txt; the per-kernel rows and
the reading there come from the profiler runs above and were added by hand)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"words": (32, 373, 9, 64), "pieces": (4, 373, 41, 1024)}
HBM_PEAK = 8.0e12


def torch_rnnt(x, targets, blank):
    """-sum_b ll_b in torch device ops, full lengths: alpha over the anti-diagonals d = t + u, one (B, cells) update
    per diagonal."""
    import torch
    B, T, U1, V = x.shape
    lp = torch.log_softmax(x, -1)
    b = lp[..., blank]                                                     # (B, T, U1)
    y = lp[:, :, :U1 - 1].gather(-1, targets[:, None, :, None].expand(B, T, U1 - 1, 1)).squeeze(-1)
    ninf = torch.full((B, 1), float("-inf"), device=x.device)
    alpha = {0: torch.zeros(B, 1, device=x.device)}                        # diagonal d: u from max(0, d-T+1) to min(d, U1-1)
    for d in range(1, T + U1 - 1):
        lo, hi = max(0, d - T + 1), min(d, U1 - 1)
        plo, phi = max(0, d - T), min(d - 1, U1 - 1)
        us = torch.arange(lo, hi + 1, device=x.device)
        prev = torch.cat([ninf, alpha[d - 1], ninf], 1)                    # prev[:, u - plo + 1] = alpha(d - 1, u)
        up_ok = (us <= phi) & (us >= plo)                                  # from (t - 1, u)
        up = prev[:, (us - plo + 1).clamp(0, phi - plo + 2)] + b[:, (d - 1 - us).clamp(0, T - 1), us]
        left_ok = (us - 1 >= plo) & (us - 1 <= phi)                        # from (t, u - 1)
        left = prev[:, (us - plo).clamp(0, phi - plo + 2)] + y[:, (d - us).clamp(0, T - 1), (us - 1).clamp(min=0)]
        up = torch.where(up_ok, up, ninf)
        left = torch.where(left_ok, left, ninf)
        alpha[d] = torch.logaddexp(up, left)
    ll = alpha[T + U1 - 2][:, 0] + b[:, T - 1, U1 - 1]
    return -ll.sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--kernel-only", action="store_true", help="skip the torch arm (profiler runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from nn_conformer_for_speech_recognition_amd import transducer
    if not torch.cuda.is_available():
        raise SystemExit("rnnt_loss.py measures on the GPU: none visible")
    arms, agree = {}, {}
    for name in a.shapes:
        B, T, U1, V = SHAPES[name]
        g = torch.Generator().manual_seed(a.seed)
        x = torch.randn(B, T, U1, V, generator=g).cuda().requires_grad_()
        tg = torch.randint(1, V, (B, U1 - 1), generator=g).cuda()

        def kernel(x=x, tg=tg):
            x.grad = None
            loss = transducer.rnnt_loss(x, tg, reduction="sum")
            loss.backward()
            return loss

        def restated(x=x, tg=tg):
            x.grad = None
            loss = torch_rnnt(x, tg, 0)
            loss.backward()
            return loss
        arms[f"{name}/kernel"] = kernel
        if not a.kernel_only:
            arms[f"{name}/torch"] = restated
            lk = kernel()
            gk = x.grad.clone()
            lt = restated()
            agree[name] = {"loss_rel": abs(float(lk.detach()) - float(lt.detach())) / abs(float(lt.detach())),
                           "grad_max_abs": float((gk - x.grad).abs().max())}
    for f in arms.values():
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, f in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / a.iters)
    med = {k: statistics.median(v) for k, v in times.items()}
    share = {}
    for name in a.shapes:
        B, T, U1, V = SHAPES[name]
        nbytes = 3 * B * T * U1 * V * 4
        share[name] = {"bytes": nbytes, "least_us": round(nbytes / HBM_PEAK * 1e6, 2),
                       "hbm_share_kernel": round(nbytes / HBM_PEAK / (med[f"{name}/kernel"] * 1e-6), 4)}
        if f"{name}/torch" in med:
            share[name]["hbm_share_torch"] = round(nbytes / HBM_PEAK / (med[f"{name}/torch"] * 1e-6), 4)
            share[name]["torch_over_kernel"] = round(med[f"{name}/torch"] / med[f"{name}/kernel"], 1)
    res = {"metric": "us per forward + backward call", "device": torch.cuda.get_device_name(), "iters": a.iters,
           "rounds": a.rounds, "shapes": {n: SHAPES[n] for n in a.shapes},
           "us_median": {k: round(v, 1) for k, v in med.items()},
           "us_min": {k: round(min(v), 1) for k, v in times.items()}, "hbm": share, "agree": agree}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"benchmarks/rnnt_loss.py on {res['device']}: us per forward + backward call, median (minimum) over "
                    f"{a.rounds} rounds of {a.iters} calls\n\n")
            f.write(f"  {'shape':8} {'B, T, U1, V':22} {'kernel':>18} {'torch ops':>22} {'ratio':>7} "
                    f"{'3BTU1V4 bytes':>14} {'least us':>9} {'share kernel':>13} {'share torch':>12}\n")
            for n in a.shapes:
                k, t = f"{n}/kernel", f"{n}/torch"
                tt = f"{med[t]:.1f} ({min(times[t]):.1f})" if t in med else "-"
                f.write(f"  {n:8} {str(SHAPES[n]):22} {med[k]:>9.1f} ({min(times[k]):.1f}) {tt:>22} "
                        f"{share[n].get('torch_over_kernel', '-'):>7} {share[n]['bytes']:>14} "
                        f"{share[n]['least_us']:>9} {share[n]['hbm_share_kernel']:>13} "
                        f"{share[n].get('hbm_share_torch', '-'):>12}\n")
            f.write("\n" + json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
