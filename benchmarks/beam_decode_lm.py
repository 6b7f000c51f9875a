"""CTC prefix beam search with an n-gram LM fused in, at the label-pass shape (B 32, T 373, V 1024), beside the
lm=None decode of the same width on the same logits in the same process: device-event time per call, rounds
interleaved over the arms, median and minimum reported.  The LM is a random trigram of a few thousand n-grams on 24
raised tokens (tests/ctc_beam_lm_ref.py's sparse model).  One JSON line on stdout; --out also writes it to a file.

Arms: beam{W} (no LM), beam{W}_lm (default token_beam) for every width, and beam{W}_lm_k{K} for --token-beams.
--plain-only times the lm=None arms alone (the A/B of that path between two builds of the library: run it once per
build, CFM_LIB naming the other build, runs interleaved).

The per-kernel split comes from a profiler run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o w16 -- \
        python benchmarks/beam_decode_lm.py --widths 16 --rounds 1 --lm-only
    python benchmarks/beam_decode_lm.py --split-from DIR     (reads every *kernel_stats.csv below DIR, no GPU)"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--T", type=int, default=373)
    ap.add_argument("--V", type=int, default=1024)
    ap.add_argument("--widths", type=int, nargs="*", default=[4, 16, 30])
    ap.add_argument("--token-beams", type=str, nargs="*", default=["16:8"], help="W:K pairs timed besides the default K")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--lm-only", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--split-from", default=None)
    a = ap.parse_args()
    if a.split_from:
        from benchmarks.beam_decode import split_from
        res = {"shape": [a.B, a.T, a.V], "kernel_split": split_from(a.split_from, a.B, a.T, a.V)}
        for e in res["kernel_split"].values():
            if "beam_search_us" in e:
                e["beam_search_us_per_frame"] = round(e["beam_search_us"] / a.T, 3)
    else:
        import torch
        from nn_conformer_for_speech_recognition_amd import ctc
        if not torch.cuda.is_available():
            raise SystemExit("beam_decode_lm.py measures on the GPU: none visible")
        g = torch.Generator().manual_seed(a.seed)
        x = torch.randn(a.B, a.T, a.V, generator=g) * 3.0
        x[..., 0] += 3.0
        x[..., 1:25] += 6.0
        x = x.cuda()
        arms = {}
        lm_info = None
        if not a.plain_only:
            from tests.ctc_beam_lm_ref import random_lm
            lm = random_lm(5, a.V, n_bi=300, n_tri=3000, hot=24)
            t = lm.device_tables(x.device)
            lm_info = {"ngrams": len(lm.table32), "slots": t["mask"] + 1, "probe": t["probe"], "order": lm.order}
        for w in a.widths:
            if not a.lm_only:
                arms[f"beam{w}"] = (lambda w=w: ctc.beam_search_decode(x, None, beam_size=w, blank=0, pad=-1))
            if not a.plain_only:
                arms[f"beam{w}_lm"] = (lambda w=w: ctc.beam_search_decode(x, None, beam_size=w, blank=0, pad=-1, lm=lm,
                                                                          lm_weight=0.5, word_bonus=0.2))
        if not a.plain_only:
            for wk in a.token_beams:
                w, k = (int(v) for v in wk.split(":"))
                arms[f"beam{w}_lm_k{k}"] = (lambda w=w, k=k: ctc.beam_search_decode(
                    x, None, beam_size=w, blank=0, pad=-1, lm=lm, lm_weight=0.5, word_bonus=0.2, token_beam=k))
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
               "iters": a.iters, "rounds": a.rounds, "lm": lm_info,
               "library": os.environ.get("CFM_LIB", "in-tree"),
               "us_median": {k: round(statistics.median(v), 2) for k, v in times.items()},
               "us_min": {k: round(min(v), 2) for k, v in times.items()},
               "us_max": {k: round(max(v), 2) for k, v in times.items()}}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
