"""CTC forced alignment alone at the label-pass shapes, beside greedy_decode and beam_search_decode (W 16) on the same
logits in the same process (fixed seed): device-event time per call, rounds interleaved over the arms, median and
minimum reported.  One JSON line on stdout; --out also writes it to a file.

Shapes (B, T, V 1024, labels per utterance): 32 x 373 with 1, 3 and 40 labels (1 and 3: the word vocabulary's own
transcripts, the single-wave recursion; 40: the multi-wave recursion), 8 x 1498 with 40 and 200 labels.  The logits are
planted along a random alignment of each target (tests/ctc_align_ref.plant), as a model that fits its labels gives.

The per-kernel split (align_prep / align_viterbi / align_backtrace) comes from a profiler run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o align -- \
        python benchmarks/align.py --rounds 1 --iters 5 --only-align
    python benchmarks/align.py --split-from DIR        (reads every *kernel_stats.csv below DIR, no GPU)

Kernel names repeat over the shapes in such a run, so the split is per kernel over all five shapes; --shapes picks
one (e.g. --shapes 8x1498x200) for a split of its own."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ["32x373x1", "32x373x3", "32x373x40", "8x1498x40", "8x1498x200"]


def split_from(root):
    rows = {}
    for path in sorted(glob.glob(os.path.join(root, "**", "*kernel_stats.csv"), recursive=True)):
        tag = os.path.basename(path).split("_kernel_stats")[0]
        entry = {}
        with open(path) as f:
            for r in csv.DictReader(f):
                for k in ("align_prep", "align_viterbi<true>", "align_viterbi<false>", "align_viterbi",
                          "align_backtrace"):
                    if k in r["Name"] and k + "_us" not in entry:
                        entry[k + "_us"] = round(float(r["AverageNs"]) / 1e3, 2)
                        entry[k + "_calls"] = int(r["Calls"])
                        break
        rows[tag] = entry
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--V", type=int, default=1024)
    ap.add_argument("--shapes", nargs="+", default=SHAPES, help="BxTxL")
    ap.add_argument("--beam", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--only-align", action="store_true")
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
            raise SystemExit("align.py measures on the GPU: none visible")
        arms, logits = {}, {}
        for shape in a.shapes:
            B, T, L = (int(v) for v in shape.split("x"))
            rng = np.random.default_rng(a.seed)
            if (B, T) not in logits:
                logits[(B, T)] = ar.make_logits(a.seed, B, T, a.V, 3.0)
            x = logits[(B, T)].copy()
            targets = [ar.make_target(rng, L, a.V, "bench") for _ in range(B)]
            for b in range(B):
                x[b] = ar.plant(x[b], targets[b], rng, 9.0)
            xd = torch.from_numpy(x).cuda()
            tg = torch.tensor(targets, dtype=torch.int32).cuda()
            il = torch.full((B,), T, dtype=torch.int32).cuda()
            tl = torch.full((B,), L, dtype=torch.int32).cuda()
            arms[f"align_{shape}"] = (lambda xd=xd, tg=tg, il=il, tl=tl: ctc.forced_align(xd, tg, il, tl))
            if not a.only_align and f"greedy_{B}x{T}" not in arms:
                arms[f"greedy_{B}x{T}"] = (lambda xd=xd: ctc.greedy_decode(xd, None, blank=0, pad=-1))
                arms[f"beam{a.beam}_{B}x{T}"] = (lambda xd=xd: ctc.beam_search_decode(xd, None, beam_size=a.beam,
                                                                                     blank=0, pad=-1))
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
        res = {"metric": "us per call (device events, eager launches, output and workspace allocation included)",
               "V": a.V, "iters": a.iters, "rounds": a.rounds,
               "us_median": {k: round(statistics.median(v), 2) for k, v in times.items()},
               "us_min": {k: round(min(v), 2) for k, v in times.items()}}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
