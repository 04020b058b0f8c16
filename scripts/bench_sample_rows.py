#!/usr/bin/env python3
"""Device time of the sampling launch (ops.sample_rows) next to what it replaces or follows, same process, alternating.

For 1 / 16 / 64 rows x vocab 32 003 (Llama with its audio tokens) and 50 435 (MPT) and the four parameter sets of the kernel tests:
  sample   -- ops.sample_rows with Philox draws, seen bitmaps, draw counters (what DeviceSampler launches);
  greedy   -- ops.decode_advance_rows on the same logits (the launch a greedy step makes; a sampled step makes both);
  torch    -- the callable the sampler replaces, softmax(logits / T) + multinomial, for the temperature-only set.
Each figure is the median over --rounds rounds of the mean of --iters back-to-back launches between two events; within a round the
candidates run in turn.  Logits: 3 * randn with five raised tokens per row (tests/sample_ref.py's family).  Writes
profiles/sample_rows.json and prints it as ONE JSON line.

    python scripts/bench_sample_rows.py [--iters 50] [--rounds 9] [--out profiles/sample_rows.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from llark_amd import ops  # noqa: E402

PARAM_SETS = {
    "T0.8": dict(temperature=0.8),
    "k50": dict(top_k=50),
    "p0.9": dict(top_p=0.9),
    "T0.7_k200_p0.95_th1.3": dict(temperature=0.7, top_k=200, top_p=0.95, repetition_penalty=1.3),
}


def event_us(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_rows.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sample_rows needs the GPU")
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    res = {"bench": "sample_rows", "device": ops.device_info()[1], "iters": args.iters, "rounds": args.rounds, "unit": "us per launch", "cells": []}
    for vocab in (32003, 50435):
        for rows in (1, 16, 64):
            logits = 3.0 * torch.randn((rows, vocab), generator=g, device=dev)
            up = torch.randint(0, vocab, (rows, 5), generator=g, device=dev)
            logits.scatter_add_(1, up, 6.0 + 4.0 * torch.rand((rows, 5), generator=g, device=dev))
            seen = torch.zeros((rows, (vocab + 31) // 32), dtype=torch.int32, device=dev)
            ids = torch.cat((torch.randint(0, vocab, (rows, 300), generator=g, device=dev), up[:, :2]), dim=1).reshape(-1).contiguous()
            ops.seen_mark_rows(ids, torch.arange(rows, dtype=torch.int32, device=dev) * 302, torch.full((rows,), 302, dtype=torch.int32, device=dev),
                               seen, vocab)
            seen0 = seen.clone()
            draws = torch.zeros((rows,), dtype=torch.int32, device=dev)
            sid = torch.arange(rows, dtype=torch.int64, device=dev)
            state = torch.full((rows,), ops.ROW_ACTIVE, dtype=torch.int32, device=dev)
            choice = torch.zeros((rows,), dtype=torch.int64, device=dev)
            nxt = torch.zeros((rows,), dtype=torch.int64, device=dev)

            def greedy():
                ops.decode_advance_rows(logits, state, nxt)

            for name, params in PARAM_SETS.items():
                def sample():
                    ops.sample_rows(logits, choice, state=state, seen=seen, draws=draws, stream_id=sid, seed=1, **params)

                def via_torch():
                    return torch.multinomial(torch.softmax(logits / max(params["temperature"], 1e-6), dim=-1), 1).view(-1)

                cands = {"sample": sample, "greedy": greedy}
                if set(params) == {"temperature"}:
                    cands["torch"] = via_torch
                for fn in cands.values():                        # warm: code objects, allocator
                    event_us(fn, 5)
                times = {k: [] for k in cands}
                for _ in range(args.rounds):
                    for k, fn in cands.items():
                        seen.copy_(seen0)                        # the sampler marks what it draws: every timing starts from the same bitmaps
                        times[k].append(event_us(fn, args.iters))
                cell = {"vocab": vocab, "rows": rows, "params": name}
                for k, v in times.items():
                    cell[k + "_us"] = round(statistics.median(v), 2)
                    cell[k + "_min_max_us"] = [round(min(v), 2), round(max(v), 2)]
                res["cells"].append(cell)
                print(json.dumps(cell), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
