"""CTC prefix beam search decode alone at the label-pass shape (B 32, T 373, V 1024), beside greedy_decode on the
same logits (fixed seed): device-event time per call for each beam width, rounds interleaved over the widths, median
and minimum reported.  One JSON line on stdout; --out also writes it to a file.

The per-kernel split (beam_topk / beam_search / beam_backtrace) comes from a profiler run of its own, one width per
run so the kernel names are not mixed:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o w16 -- \
        python benchmarks/beam_decode.py --widths 16 --rounds 1
    python benchmarks/beam_decode.py --split-from DIR        (reads every *kernel_stats.csv below DIR, no GPU)

beam_topk is the HBM-bound kernel (each logits row read once: B T V 4 bytes; its GB/s is printed with the split);
beam_search is latency-bound (one workgroup per utterance, frames in sequence)."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def split_from(root, B, T, V):
    rows = {}
    for path in sorted(glob.glob(os.path.join(root, "**", "*kernel_stats.csv"), recursive=True)):
        tag = os.path.basename(path).split("_kernel_stats")[0]
        entry = {}
        with open(path) as f:
            for r in csv.DictReader(f):
                for k in ("beam_topk", "beam_search", "beam_backtrace", "greedy_argmax", "greedy_compact"):
                    if k in r["Name"]:
                        entry[k + "_us"] = round(float(r["AverageNs"]) / 1e3, 2)
                        entry[k + "_calls"] = int(r["Calls"])
        if "beam_topk_us" in entry:
            entry["beam_topk_GBps"] = round(B * T * V * 4 / (entry["beam_topk_us"] * 1e-6) / 1e9, 1)
        rows[tag] = entry
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--T", type=int, default=373)
    ap.add_argument("--V", type=int, default=1024)
    ap.add_argument("--widths", type=int, nargs="+", default=[1, 4, 16, 64, 128])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--split-from", default=None)
    a = ap.parse_args()
    if a.split_from:
        res = {"shape": [a.B, a.T, a.V], "kernel_split": split_from(a.split_from, a.B, a.T, a.V)}
    else:
        import torch
        from nn_conformer_for_speech_recognition_amd import ctc
        if not torch.cuda.is_available():
            raise SystemExit("beam_decode.py measures on the GPU: none visible")
        g = torch.Generator().manual_seed(a.seed)
        x = torch.randn(a.B, a.T, a.V, generator=g) * 3.0
        x[..., 0] += 3.0
        x = x.cuda()
        arms = {"greedy": lambda: ctc.greedy_decode(x, None, blank=0, pad=-1)}
        for w in a.widths:
            arms[f"beam{w}"] = (lambda w=w: ctc.beam_search_decode(x, None, beam_size=w, blank=0, pad=-1))
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
        res = {"metric": "us per decode call (device events, eager launches)", "shape": [a.B, a.T, a.V],
               "iters": a.iters, "rounds": a.rounds,
               "us_median": {k: round(statistics.median(v), 2) for k, v in times.items()},
               "us_min": {k: round(min(v), 2) for k, v in times.items()},
               "logits_bytes": a.B * a.T * a.V * 4}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
