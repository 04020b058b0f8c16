#!/usr/bin/env python3
"""Device time of the log-probability launch (ops.token_logprob_rows) next to what it replaces and to its yardstick, same process,
alternating.

For 1 / 16 / 64 rows x vocab 32 003 (Llama with its audio tokens) and 50 435 (MPT):
  logprob  -- ops.token_logprob_rows with rank and the per-slot history (what LogprobTracker launches);
  torch    -- the callable it replaces, torch.log_softmax(logits, -1).gather(-1, tokens);
  greedy   -- ops.decode_advance_rows on the same logits: the greedy step's launch, which reads the same rows once (the yardstick).
Each figure is the median over --rounds rounds of the mean of --iters back-to-back launches between two events; within a round the
candidates run in turn.  Logits: 3 * randn with five raised tokens per row (tests/logprob_ref.py's family); the targets are the rows'
greedy tokens.  Writes profiles/token_logprob_rows.json and prints it as ONE JSON line.

    python scripts/bench_logprob_rows.py [--iters 50] [--rounds 9] [--out profiles/token_logprob_rows.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "token_logprob_rows.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_logprob_rows needs the GPU")
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    res = {"bench": "token_logprob_rows", "device": ops.device_info()[1], "iters": args.iters, "rounds": args.rounds, "unit": "us per launch",
           "cells": []}
    for vocab in (32003, 50435):
        for rows in (1, 16, 64):
            logits = 3.0 * torch.randn((rows, vocab), generator=g, device=dev)
            up = torch.randint(0, vocab, (rows, 5), generator=g, device=dev)
            logits.scatter_add_(1, up, 6.0 + 4.0 * torch.rand((rows, 5), generator=g, device=dev))
            tokens = logits.argmax(-1)
            state = torch.full((rows,), ops.ROW_ACTIVE, dtype=torch.int32, device=dev)
            nxt = torch.zeros((rows,), dtype=torch.int64, device=dev)
            lp = torch.zeros((rows,), dtype=torch.float32, device=dev)
            rank = torch.zeros((rows,), dtype=torch.int32, device=dev)
            hist = torch.zeros((rows, 2048), dtype=torch.float32, device=dev)
            count = torch.zeros((rows,), dtype=torch.int32, device=dev)
            total = torch.zeros((rows,), dtype=torch.float32, device=dev)

            def logprob():
                ops.token_logprob_rows(logits, tokens, lp, rank=rank, state=state, hist=hist, count=count, total=total)

            def via_torch():
                return torch.log_softmax(logits, dim=-1).gather(-1, tokens[:, None])

            def greedy():
                ops.decode_advance_rows(logits, state, nxt)

            cands = {"logprob": logprob, "torch": via_torch, "greedy": greedy}
            for fn in cands.values():                            # warm: code objects, allocator
                event_us(fn, 5)
            want = via_torch().view(-1)
            assert float((lp - want).abs().max()) <= 1e-4, "the launch and the torch callable disagree"
            times = {k: [] for k in cands}
            for _ in range(args.rounds):
                for k, fn in cands.items():
                    count.zero_()
                    times[k].append(event_us(fn, args.iters))
            cell = {"vocab": vocab, "rows": rows}
            for k, v in times.items():
                cell[k + "_us"] = round(statistics.median(v), 2)
                cell[k + "_min_max_us"] = [round(min(v), 2), round(max(v), 2)]
            cell["logprob_over_greedy"] = round(cell["logprob_us"] / cell["greedy_us"], 3)
            cell["logprob_over_torch"] = round(cell["logprob_us"] / cell["torch_us"], 3)
            res["cells"].append(cell)
            print(json.dumps(cell), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
