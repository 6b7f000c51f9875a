"""The device transducer greedy search (TransducerHead.decode: csrc/rnnt_greedy.hip, one launch) beside
TransducerHead.greedy_decode, the same search as a Python loop of torch ops over T * max_symbols steps -- what the
head offered before the kernel.  Same head, same input, same process; the two are checked to give the same tokens.

Shapes (B, T, V), H = J = 256, max_symbols 2:
  words   32, 373, 64      the encoder length of the flagship workload, a word vocabulary
  pieces  32, 373, 1024    the same over 1024 word pieces
Each shape twice, by the blank's bias (set from the distribution of the first decision's logits, so no tuning by hand):
  blank   the 0.99 quantile of (best label - blank): almost every frame closes on its first blank
  third   the 2/3 quantile: about one frame in three emits

Arms (device events around --iters calls, after --warmup calls; median and minimum over --rounds, the arms alternating
within a round; the two GEMMs that build ep and the cell's input table, the output allocations and the launch are all
inside the kernel arm's time):
  kernel  head.decode(enc, lengths, max_symbols=2)
  torch   head.greedy_decode(enc, lengths, max_symbols=2)

"us/decision" is the kernel arm's time over the decisions taken by the slowest utterance (its emitted tokens plus the
frames it closed with a blank): the length of the longest dependent chain in the launch.  The floor beside it is ONE
dependent L2-hit load, 180-225 cycles = 0.075-0.094 us at 2.4 GHz (the cycle-constants table of the MI355X guide): a
decision is at least one sweep of w_out that cannot start before the previous decision's token is known.

One JSON line on stdout; --out also writes the text table of profiles/rnnt_greedy/times.txt."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"words": (32, 373, 64), "pieces": (32, 373, 1024)}
REGIMES = {"blank": 0.99, "third": 2.0 / 3.0}
ENC, EMBED, HIDDEN, JOINT, MAX_SYMBOLS, BLANK = 256, 128, 256, 256, 2, 0
L2_HIT_US = (180 / 2400.0, 225 / 2400.0)


def make(torch, B, T, V, quantile, seed):
    from nn_conformer_for_speech_recognition_amd.transducer import TransducerHead
    torch.manual_seed(seed)
    head = TransducerHead(ENC, V, BLANK, embed=EMBED, hidden=HIDDEN, joint=JOINT).cuda()
    enc = torch.randn(B, T, ENC, generator=torch.Generator().manual_seed(seed + 1)).cuda()
    with torch.no_grad():
        head.out.weight.mul_(12.0)
        zero = torch.zeros(1, HIDDEN, device="cuda")
        start = torch.full((1,), BLANK, dtype=torch.int64, device="cuda")
        h, _ = head._cell(head.embedding(start), zero, zero)
        logits = head.out(torch.tanh(head.enc_proj(enc) + head.pred_proj(h)))          # the first decision of every frame
        labels = logits.clone()
        labels[..., BLANK] = float("-inf")
        gap = (labels.max(-1).values - logits[..., BLANK]).flatten()
        head.out.bias[BLANK] += torch.quantile(gap, quantile)
    lengths = torch.full((B,), T, dtype=torch.int32, device="cuda")
    return head, enc, lengths


def decisions(torch, out, T):
    """Per utterance: tokens emitted + frames closed by a blank (those with fewer than MAX_SYMBOLS tokens)."""
    res = []
    for b in range(out.tokens.shape[0]):
        n = int(out.counts[b])
        per_frame = torch.bincount(out.frames[b, :n].long(), minlength=T)
        res.append(n + int((per_frame < MAX_SYMBOLS).sum()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--torch-iters", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--kernel-only", action="store_true", help="skip the torch arm (profiler runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rnnt_greedy.py measures on the GPU: none visible")
    arms, info = {}, {}
    for name in a.shapes:
        B, T, V = SHAPES[name]
        for regime, q in REGIMES.items():
            key = f"{name}/{regime}"
            head, enc, lengths = make(torch, B, T, V, q, a.seed)
            out = head.decode(enc, lengths, max_symbols=MAX_SYMBOLS)
            dec = decisions(torch, out, T)
            info[key] = {"tokens": int(out.counts.sum()), "emit_per_frame": round(float(out.counts.sum()) / (B * T), 3),
                         "decisions_slowest": max(dec), "decisions_total": sum(dec)}
            arms[f"{key}/kernel"] = (lambda h=head, e=enc, n=lengths: h.decode(e, n, max_symbols=MAX_SYMBOLS), a.iters)
            if not a.kernel_only:
                loop = head.greedy_decode(enc, lengths, max_symbols=MAX_SYMBOLS)
                info[key]["same_tokens"] = bool(torch.equal(loop[0], out.tokens) and torch.equal(loop[1], out.counts))
                arms[f"{key}/torch"] = (lambda h=head, e=enc, n=lengths: h.greedy_decode(e, n, max_symbols=MAX_SYMBOLS),
                                        a.torch_iters)
    for f, _ in arms.values():
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, (f, iters) in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / iters)
    med = {k: statistics.median(v) for k, v in times.items()}
    for key, d in info.items():
        d["us_per_decision"] = round(med[f"{key}/kernel"] / d["decisions_slowest"], 3)
        if f"{key}/torch" in med:
            d["torch_over_kernel"] = round(med[f"{key}/torch"] / med[f"{key}/kernel"], 1)
    res = {"metric": "us per decode call", "device": torch.cuda.get_device_name(), "iters": a.iters,
           "torch_iters": a.torch_iters, "rounds": a.rounds, "shapes": {n: SHAPES[n] for n in a.shapes},
           "H": HIDDEN, "J": JOINT, "max_symbols": MAX_SYMBOLS, "us_median": {k: round(v, 1) for k, v in med.items()},
           "us_min": {k: round(min(v), 1) for k, v in times.items()}, "cases": info,
           "floor_us_one_l2_hit": [round(x, 3) for x in L2_HIT_US]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"benchmarks/rnnt_greedy.py on {res['device']}: us per decode call, median (minimum) over {a.rounds} "
                    f"rounds of {a.iters} (kernel) / {a.torch_iters} (torch loop) calls; H = J = {HIDDEN}, "
                    f"max_symbols {MAX_SYMBOLS}\n\n")
            f.write(f"  {'case':14} {'B, T, V':16} {'tokens/frame':>12} {'kernel':>20} {'torch loop':>26} {'ratio':>7} "
                    f"{'decisions (slowest)':>20} {'us/decision':>12} {'same tokens':>12}\n")
            for key, d in info.items():
                k, t = f"{key}/kernel", f"{key}/torch"
                tt = f"{med[t]:.1f} ({min(times[t]):.1f})" if t in med else "-"
                f.write(f"  {key:14} {str(SHAPES[key.split('/')[0]]):16} {d['emit_per_frame']:>12} "
                        f"{med[k]:>10.1f} ({min(times[k]):.1f}) {tt:>26} {d.get('torch_over_kernel', '-'):>7} "
                        f"{d['decisions_slowest']:>20} {d['us_per_decision']:>12} {str(d.get('same_tokens', '-')):>12}\n")
            f.write(f"\nfloor: one dependent L2-hit load, {L2_HIT_US[0]:.3f}-{L2_HIT_US[1]:.3f} us (180-225 cycles at 2.4 "
                    f"GHz)\n\n" + json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
