"""Time the libcfm BiLSTM decoder (csrc/lstm.hip) against torch.nn.LSTM (MIOpen) on the same GPU, and the batched
per-utterance recurrence (csrc/lstm_batched.hip) against the unbatched one on the same tokens.

  python benchmarks/lstm_bench.py [libcfm]     the unbatched legs: the reference decoder nn.LSTM(256, 512,
        bidirectional=True) over one unbatched sequence of L = B*T_enc steps (asrnn.py:38,252): L 1280 (native
        B 32 x 40 frames) and 11936 (L15: B 32 x 373); "libcfm" skips the MIOpen leg (profiling).  One JSON line
        per (impl, L) with forward and forward+backward ms.
  python benchmarks/lstm_bench.py batched      the same module on the same (B*T, 256) tokens as ONE sequence of
        L = B*T steps (2-D input) and as B sequences of T steps (3-D input), B 32 x T 40 and B 32 x T 373, forward
        (no_grad) and forward + backward.  After a warm-up the legs are interleaved, every repetition timed on its
        own; one JSON line per (shape, leg) with the minimum and the median, then one line per shape with the
        ratios unbatched minimum / batched median and the batched time per step.
  python benchmarks/lstm_bench.py batched-only the batched legs alone (the command to put under a kernel trace)."""
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, __file__.rsplit("/benchmarks/", 1)[0])
from nn_conformer_for_speech_recognition_amd.lstm import LSTM  # noqa: E402


def timeit(fn, n):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def batched(with_unbatched=True):
    dev = "cuda"
    for B, T, reps in ((32, 40, 7), (32, 373, 3)):
        torch.manual_seed(0)
        m = LSTM(256, 512, bidirectional=True, batch_first=True).to(dev)
        x2 = torch.randn(B * T, 256, device=dev, requires_grad=True)
        dy2 = torch.randn(B * T, 1024, device=dev)
        x3, dy3 = x2.view(B, T, 256), dy2.view(B, T, 1024)

        def fwd(x):
            with torch.no_grad():
                m(x)

        def fwdbwd(x, dy):
            y, _ = m(x)
            y.backward(dy)
        legs = {"batched_fwd": lambda: fwd(x3), "batched_fwd_bwd": lambda: fwdbwd(x3, dy3)}
        if with_unbatched:
            legs.update({"unbatched_fwd": lambda: fwd(x2), "unbatched_fwd_bwd": lambda: fwdbwd(x2, dy2)})
        for fn in legs.values():                                  # warm-up: every leg once, untimed
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in legs}
        for _ in range(reps):                                     # interleaved: one repetition of every leg in turn
            for k, fn in legs.items():
                ms[k].append(once(fn))
        res = {k: (min(v), statistics.median(v)) for k, v in ms.items()}
        for k, (lo, med) in res.items():
            print(json.dumps({"B": B, "T": T, "L": B * T, "leg": k, "reps": reps, "min_ms": round(lo, 3),
                              "median_ms": round(med, 3)}), flush=True)
        out = {"B": B, "T": T,
               "batched_us_per_step_fwd": round(res["batched_fwd"][1] * 1e3 / T, 3),
               "batched_us_per_step_fwd_bwd": round(res["batched_fwd_bwd"][1] * 1e3 / T, 3)}
        if with_unbatched:
            for p in ("fwd", "fwd_bwd"):
                out[f"unbatched_min_over_batched_median_{p}"] = round(res[f"unbatched_{p}"][0] / res[f"batched_{p}"][1], 2)
                out[f"batched_median_below_unbatched_min_{p}"] = res[f"batched_{p}"][1] < res[f"unbatched_{p}"][0]
        print(json.dumps(out), flush=True)
        LSTM.check_errors()


def main():
    dev = "cuda"
    only = sys.argv[1] if len(sys.argv) > 1 else None          # "libcfm": skip the MIOpen leg (profiling)
    if only in ("batched", "batched-only"):
        return batched(with_unbatched=only == "batched")
    for L in (1280, 11936):
        torch.manual_seed(0)
        ref = torch.nn.LSTM(256, 512, bidirectional=True).to(dev)
        mine = LSTM(256, 512, bidirectional=True).to(dev)
        mine.load_state_dict(ref.state_dict())
        x = torch.randn(L, 256, device=dev, requires_grad=True)
        dy = torch.randn(L, 1024, device=dev)
        n = 5 if L < 5000 else 2
        for name, m in (("libcfm", mine), ("torch_miopen", ref)):
            if only and name != only:
                continue
            def fwd():
                with torch.no_grad():
                    m(x)

            def fwdbwd():
                y, _ = m(x)
                y.backward(dy)
            f = timeit(fwd, n)
            fb = timeit(fwdbwd, n)
            print(json.dumps({"impl": name, "L": L, "fwd_ms": round(f, 3), "fwd_bwd_ms": round(fb, 3),
                              "us_per_step_fwd": round(f * 1e3 / L, 3)}), flush=True)


if __name__ == "__main__":
    main()
