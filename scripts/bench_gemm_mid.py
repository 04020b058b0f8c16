#!/usr/bin/env python3
"""A/B of the decode-step Linear at 17 .. 64 rows: ops.gemm16_mid (csrc/gemm_mid.hip) against the path ops.gemm16 takes for those row
counts (128x128x32 tiles, variant 0), at the five Linear shapes of a Llama-2-7B decode step x m in {32, 64}, in both activation flows.

The two kernels alternate in one process, block by block.  Every launch of a block reads another copy of the weight (enough copies to
exceed 512 MB, more than the last-level cache holds), as a decode step reads each layer's weights once: the figure is a weight stream
out of HBM, not out of a warm cache.  Per shape: median us per launch over the blocks (device events around each block), the ratio,
and the achieved weight-stream rate n * kp * 2 bytes / time.  Prints ONE JSON line.

    python scripts/bench_gemm_mid.py [--rounds 5] [--launches 12]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llark_amd import ops  # noqa: E402

H, I, VOCAB = 4096, 11008, 32000
SHAPES = [("qkv", 3 * H, H, "f32"), ("o_proj", H, H, "resid"), ("gate_up", 2 * I, H, "swiglu"), ("down_proj", H, I, "resid"),
          ("lm_head", VOCAB, H, "f32")]


def bench_shape(name, n, k, kind, m, split, rounds, launches):
    g = torch.Generator(device="cuda").manual_seed(n + k + m)
    copies = max(2, -(-512 * 2 ** 20 // (n * k * 2)))
    ws = [(torch.randn(n, k, generator=g, device="cuda") * 0.02).bfloat16() for _ in range(copies)]
    a = torch.randn(m, k, generator=g, device="cuda")
    hi = a.bfloat16()
    lo = (a - hi.float()).bfloat16() if split else None
    epi = {"f32": ops.EPI_F32, "resid": ops.EPI_RESID, "swiglu": ops.EPI_SWIGLU_SPLIT if split else ops.EPI_SWIGLU16}[kind]
    c = torch.zeros(m, n, device="cuda") if kind != "swiglu" else None
    oh = torch.empty(m, n // 2, dtype=torch.bfloat16, device="cuda") if kind == "swiglu" else None
    ol = torch.empty_like(oh) if kind == "swiglu" and split else None
    scratch = torch.empty(ops.gemm16_mid_scratch_bytes(m, n, k, split, epi) // 4, device="cuda")
    kw = dict(c=c, resid=c if kind == "resid" else None, out_hi=oh, out_lo=ol)

    def mid(w):
        ops.gemm16_mid(hi, lo, w, None, n, epi, scratch, **kw)

    def tiled(w):
        ops.gemm16(hi, lo, w, None, n, epi, **kw)

    times = {"mid": [], "tiled": []}
    for fn in (mid, tiled):
        for w in ws:
            fn(w)                                             # warm up: code objects, every copy touched once
    torch.cuda.synchronize()
    for _ in range(rounds):
        for label, fn in (("mid", mid), ("tiled", tiled)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for j in range(launches):
                fn(ws[j % copies])
            e1.record()
            torch.cuda.synchronize()
            times[label].append(e0.elapsed_time(e1) * 1e3 / launches)
    t_mid, t_tiled = statistics.median(times["mid"]), statistics.median(times["tiled"])
    return {"shape": name, "n": n, "k": k, "m": m, "flow": "split" if split else "bf16", "weight_copies": copies,
            "mid_us": round(t_mid, 2), "tiled_us": round(t_tiled, 2), "tiled_over_mid": round(t_tiled / t_mid, 3),
            "mid_us_min_max": [round(min(times["mid"]), 2), round(max(times["mid"]), 2)],
            "tiled_us_min_max": [round(min(times["tiled"]), 2), round(max(times["tiled"]), 2)],
            "mid_weight_TBps": round(n * k * 2 / t_mid / 1e6, 3), "tiled_weight_TBps": round(n * k * 2 / t_tiled / 1e6, 3),
            "mid_scratch_MB": round(scratch.numel() * 4 / 2 ** 20, 2)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=12)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gemm_mid needs the GPU")
    rows = []
    for split in (True, False):
        for name, n, k, kind in SHAPES:
            for m in (32, 64):
                rows.append(bench_shape(name, n, k, kind, m, split, args.rounds, args.launches))
                torch.cuda.empty_cache()
    print(json.dumps({"bench": "gemm_mid_ab", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
                      "launches_per_block": args.launches, "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
