"""What scale_parameter / weight_decay / capturable cost: Adafactor steps over bench.py's parameter
set (default L15) with random gradients, no model step around them.

    python benchmarks/adafactor_modes.py [--config L15 | --test-shapes] [--steps 50]
                                         [--modes base,scale,...] [--digest]

Prints one JSON line per mode: device-event time per step and the host's wall time per step (ms;
the loop ends in a synchronise), and the bytes per parameter the step's kernels have to move (read
+ written, from the shapes), so time can be set against HBM bandwidth.  --digest seeds the
parameters and gradients and adds a SHA-256 over every parameter and state tensor after the run:
two builds that launch the same kernels print the same digest.  For per-kernel times run it under
`rocprofv3 --kernel-trace --stats -- python ...` with one mode (the kernels are the ada_* family).

  base     scale_parameter=False (the reference's step: six launches)
  scale    scale_parameter=True  (+ one read of p in ada_sumsq, + one partial array)
  wd       scale_parameter=False, weight_decay=0.1
  cap      scale_parameter=True, relative_step=True, capturable=True, launched eagerly
  graph    the same, one captured graph replayed
"""
import argparse
import hashlib
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

MODES = {
    "base": dict(lr=2e-5, beta1=0.9, scale_parameter=False, relative_step=False),
    "scale": dict(lr=2e-5, beta1=0.9, scale_parameter=True, relative_step=False),
    "wd": dict(lr=2e-5, beta1=0.9, scale_parameter=False, relative_step=False, weight_decay=0.1),
    "cap": dict(beta1=0.9, scale_parameter=True, relative_step=True, capturable=True),
    "graph": dict(beta1=0.9, scale_parameter=True, relative_step=True, capturable=True),
}


# the shape list of tests/test_gpu_adafactor_full.py: the smallest shapes at which each kernel path is taken
TEST_SHAPES = [(37,), (5,), (4096,), (4097,), (64, 48), (300, 2304), (33, 3000), (16, 8, 3, 3), (8, 16, 1),
               (2, 70, 100), (64,), (24, 40)]


def digest_of(opt, params):
    h = hashlib.sha256()
    for t in [p.detach() for p in params] + [v for p in params for _, v in sorted(opt.state[p].items())
                                             if torch.is_tensor(v)]:
        h.update(t.cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def shapes_of(config):
    import bench
    name, L, d, H, ffn, K, B, secs, pos_enc = bench.CONFIGS[config]
    with torch.device("meta"):
        model = bench.EncoderCTC(L, d, H, ffn, K, 1024, 80, 100 * secs + 1, 0.1, torch.bfloat16, pos_enc, False)
    return [tuple(p.shape) for p in model.parameters() if p.requires_grad]


def bytes_per_param(shapes, scale):
    """Per element: ada_colpart/rows/cols read g (factored tensors; once or twice), ada_sumsq reads g (+ p
    with scale_parameter), ada_apply reads g, m, p and writes m, p.  Unfactored tensors read and write
    v in ada_sumsq as well.  Row / column statistics and partials are O(rows + columns) and left out."""
    total = sum(torch.Size(s).numel() for s in shapes)
    moved = 0
    for s in shapes:
        n = torch.Size(s).numel()
        if len(s) >= 2:
            wide = 64 <= s[-1] <= 2560
            moved += n * 4 * ((1 if wide else 2) + 1 + 5)
        else:
            moved += n * 4 * (3 + 5)
        if scale:
            moved += n * 4
    return moved / total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="L15")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--modes", default="base,scale,base,scale,wd,cap,graph")
    ap.add_argument("--test-shapes", action="store_true", help="the tests' shape list instead of --config")
    ap.add_argument("--digest", action="store_true")
    args = ap.parse_args()
    from nn_conformer_for_speech_recognition_amd.optim import Adafactor
    if not torch.cuda.is_available():
        raise SystemExit("adafactor_modes.py needs the GPU: it measures, there is no CPU path")
    shapes = TEST_SHAPES if args.test_shapes else shapes_of(args.config)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device="cpu").manual_seed(0)
    for mode in args.modes.split(","):
        cfg = MODES[mode]
        if args.digest:                 # every mode from the same parameters and gradients
            gen.manual_seed(0)
            torch.manual_seed(0)
        params = [torch.nn.Parameter((torch.randn(s, generator=gen) * 0.05).to(dev)) for s in shapes]
        for p in params:
            p.grad = torch.randn(p.shape, device=dev)
        opt = Adafactor(params, **cfg)
        for _ in range(args.warmup):
            opt.step()
        run = opt.step
        if mode == "graph":
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                opt.step()
            run = g.replay
            run()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        w0 = time.perf_counter()
        t0.record()
        for _ in range(args.steps):
            run()
        t1.record()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - w0) * 1e3 / args.steps
        ms = t0.elapsed_time(t1) / args.steps
        nparam = sum(p.numel() for p in params)
        bpp = bytes_per_param(shapes, cfg["scale_parameter"])
        rec = {"mode": mode, "config": "tests" if args.test_shapes else args.config, "tensors": len(params),
               "params": nparam, "ms_per_step": round(ms, 4), "wall_ms_per_step": round(wall, 4),
               "bytes_per_param": round(bpp, 2), "GBps": round(nparam * bpp / ms / 1e6, 1),
               "finite": bool(all(torch.isfinite(p).all() for p in params))}
        if args.digest:
            rec["sha256"] = digest_of(opt, params)
        print(json.dumps(rec), flush=True)
        del opt, params
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
