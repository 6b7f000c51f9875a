"""MWER training term at the label-pass shape (B 32, T 373, V 1024, hypotheses of <= 40 labels), N 4 and 8: device-event
time per forward + backward, rounds interleaved over the arms, median and minimum reported.  One JSON line on stdout;
--out also writes it to a file.

Arms, per N, on the same logits (planted along a random alignment of a 40-label target, as a model that fits its
labels gives) and the beam's own n-best list:
  mwer_N          ctc.mwer_loss forward + backward: beam search (--beam wide), edit distance, expected risk
  risk_N          its ctc.expected_risk_loss part alone, forward + backward (csrc/ctc_nbest.hip)
  composed_N      what a user could compose before: the logits expanded to B N rows, ctc.ctc_loss(reduction='none')
                  on them, weighted by the same c, forward + backward (N sweeps of the logits each way, a dense
                  (B N, T, V) gradient summed back over N)

The per-kernel split comes from a profiler run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o mwer -- \
        python benchmarks/mwer.py --rounds 1 --iters 5 --only-risk
    python benchmarks/mwer.py --split-from DIR        (reads every *kernel_stats.csv below DIR, no GPU)"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KERNELS = ("nbest_prep", "nbest_alpha", "nbest_weights", "nbest_beta", "nbest_grad")


def split_from(root):
    rows = {}
    for path in sorted(glob.glob(os.path.join(root, "**", "*kernel_stats.csv"), recursive=True)):
        entry = {}
        with open(path) as f:
            for r in csv.DictReader(f):
                for k in KERNELS:
                    if k in r["Name"]:
                        entry[k + "_us"] = round(float(r["AverageNs"]) / 1e3, 2)
                        entry[k + "_calls"] = int(r["Calls"])
                        break
        rows[os.path.basename(path).split("_kernel_stats")[0]] = entry
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--T", type=int, default=373)
    ap.add_argument("--V", type=int, default=1024)
    ap.add_argument("--labels", type=int, default=40)
    ap.add_argument("--nbest", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--beam", type=int, default=16)
    ap.add_argument("--noise", type=float, default=1.0)
    ap.add_argument("--plant", type=float, default=8.0)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--only-risk", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--split-from", default=None)
    a = ap.parse_args()
    if a.split_from:
        res = {"kernel_split": split_from(a.split_from)}
    else:
        import numpy as np
        import torch
        from nn_conformer_for_speech_recognition_amd import ctc
        from tests import ctc_align_ref as ar
        if not torch.cuda.is_available():
            raise SystemExit("mwer.py measures on the GPU: none visible")
        B, T, V, L = a.B, a.T, a.V, a.labels
        rng = np.random.default_rng(a.seed)
        x = ar.make_logits(a.seed, B, T, V, a.noise)      # noise well below the planted path: hypotheses of about L labels
        targets = [ar.make_target(rng, L, V, "bench") for _ in range(B)]
        for b in range(B):
            x[b] = ar.plant(x[b], targets[b], rng, a.plant)
        xd = torch.from_numpy(x).cuda().requires_grad_()
        tg = torch.tensor(targets, dtype=torch.int32).cuda()
        il = torch.full((B,), T, dtype=torch.int32).cuda()
        tl = torch.full((B,), L, dtype=torch.int32).cuda()
        arms, info = {}, {}
        for N in a.nbest:
            W = max(a.beam, N)
            with torch.no_grad():
                tokens, lens, scores = ctc.beam_search_decode(xd.detach(), il, beam_size=W, nbest=N)
                width = max(int(lens.max()), 1)
                hyps = tokens[..., :width].contiguous()
                lens = torch.where(scores == float("-inf"), torch.full_like(lens, -1), lens)
                risk = ctc.edit_distance(hyps, tg, lens, tl).distance.float()
                out = ctc.expected_risk_loss(xd.detach(), hyps, lens, risk, il)
                live = torch.isfinite(out.ll)
                rbar = (risk * live).sum(1, keepdim=True) / live.sum(1, keepdim=True).clamp(min=1)
                c = (out.post * ((risk - rbar) - out.loss[:, None])).reshape(-1)
                flat, flat_len = hyps.reshape(B * N, width).clamp(min=0), lens.reshape(-1).clamp(min=0)
                il_n = il.repeat_interleave(N)
            info[f"N{N}"] = {"hyp_labels_max": width, "hyp_labels_mean": round(float(lens.float().mean()), 1),
                             "live": int(live.sum()), "risk_mean": round(float(risk.mean()), 2),
                             "loss_mean": round(float(out.loss.mean()), 4)}

            def mwer(N=N, W=W):
                xd.grad = None
                ctc.mwer_loss(xd, tg, il, tl, nbest=N, beam_size=W)[0].sum().backward()

            def risk_only(hyps=hyps, lens=lens, risk=risk):
                xd.grad = None
                ctc.expected_risk_loss(xd, hyps, lens, risk, il).loss.sum().backward()

            def composed(N=N, flat=flat, flat_len=flat_len, il_n=il_n, c=c):
                xd.grad = None
                nll = ctc.ctc_loss(xd.repeat_interleave(N, 0), flat, il_n, flat_len, reduction="none",
                                   zero_infinity=True, batch_first=True)
                (nll * -c).sum().backward()

            arms[f"risk_{N}"] = risk_only
            if not a.only_risk:
                arms[f"mwer_{N}"] = mwer
                arms[f"composed_{N}"] = composed
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
        res = {"metric": "us per forward + backward (device events, eager launches, allocations included)",
               "B": B, "T": T, "V": V, "labels": L, "beam": a.beam, "iters": a.iters, "rounds": a.rounds,
               "inputs": info,
               "us_median": {k: round(statistics.median(v), 1) for k, v in times.items()},
               "us_min": {k: round(min(v), 1) for k, v in times.items()}}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
