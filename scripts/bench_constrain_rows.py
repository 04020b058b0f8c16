#!/usr/bin/env python3
"""Device time of the constraint launch (ops.constrain_rows) next to the sampling launch and to torch, same process, alternating.

For 1 / 16 / 64 rows x vocab 32 003 (Llama with its audio tokens) and 50 435 (MPT) x histories of 300 and 2 047 tokens, with
no_repeat_ngram_size = 3, three bad words, min_new_tokens on and the step's token appended, as a decode step launches it:
  constrain -- ops.constrain_rows writing the processed rows (what DeviceConstraints.process launches);
  sample    -- ops.sample_rows on the same logits with all four processors on (temperature 0.7, top-k 200, top-p 0.95, penalty 1.3);
  torch     -- a callable that applies the same bans -- n-gram, the three words, EOS -- to GPU tensors (unfold, compare,
               scatter_reduce, one masked column write per word; no transfer).
Condition: at every point constrain is no slower than sample in the same run (it streams the row once and selects nothing, the sampler
holds the row through two 32-step bisections); "condition_holds" says so, and the script names the slower cells and exits with
status 1 when it does not hold.  The ratio to torch is reported, not gated.
Each figure is the median over --rounds rounds of the mean of --iters back-to-back launches between two events; within a round the
candidates run in turn.  Histories draw from 500 tokens, so trigrams do recur.  Writes profiles/constrain_rows.json and prints it as ONE
JSON line.

    python scripts/bench_constrain_rows.py [--iters 50] [--rounds 9] [--out profiles/constrain_rows.json]
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

NGRAM, EOS, MIN_NEW = 3, 2, 1 << 20
WORDS = [[7], [11, 12], [13, 14, 15]]
SAMPLER = dict(temperature=0.7, top_k=200, top_p=0.95, repetition_penalty=1.3)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "constrain_rows.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_constrain_rows needs the GPU")
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    i32 = dict(dtype=torch.int32, device=dev)
    res = {"bench": "constrain_rows", "device": ops.device_info()[1], "iters": args.iters, "rounds": args.rounds, "unit": "us per launch",
           "no_repeat_ngram_size": NGRAM, "sampler": SAMPLER, "cells": []}
    for vocab in (32003, 50435):
        for rows in (1, 16, 64):
            logits = 3.0 * torch.randn((rows, vocab), generator=g, device=dev)
            up = torch.randint(0, vocab, (rows, 5), generator=g, device=dev)
            logits.scatter_add_(1, up, 6.0 + 4.0 * torch.rand((rows, 5), generator=g, device=dev))
            state = torch.full((rows,), ops.ROW_ACTIVE, **i32)
            for length in (300, 2047):
                width = length + args.iters + 8                    # every launch of a timing appends one token
                hist = torch.zeros((rows, width), **i32)
                hist[:, :length] = torch.randint(0, 500, (rows, length), generator=g, device=dev).to(torch.int32)
                hist_len0 = torch.full((rows,), length, **i32)
                hist_len = hist_len0.clone()
                prompt_len = torch.full((rows,), length // 2, **i32)
                last = torch.randint(0, 500, (rows,), generator=g, device=dev)
                bw_tokens = torch.tensor([t for w in WORDS for t in w], **i32)
                bw_off = torch.tensor([0, 1, 3, 6], **i32)
                out = torch.empty((rows, vocab), dtype=torch.float32, device=dev)
                status = torch.zeros((1,), **i32)
                seen = torch.zeros((rows, (vocab + 31) // 32), **i32)
                ops.seen_mark_rows(hist[:, :length].to(torch.int64).reshape(-1).contiguous(), torch.arange(rows, **i32) * length,
                                   torch.full((rows,), length, **i32), seen, vocab)
                seen0 = seen.clone()
                draws = torch.zeros((rows,), **i32)
                sid = torch.arange(rows, dtype=torch.int64, device=dev)
                choice = torch.zeros((rows,), dtype=torch.int64, device=dev)
                h64 = hist[:, :length].to(torch.int64)
                neg, pos = torch.full((), float("-inf"), device=dev), torch.full((), float("inf"), device=dev)

                def constrain():
                    ops.constrain_rows(logits, state=state, hist=hist, hist_len=hist_len, prompt_len=prompt_len, last_token=last,
                                       no_repeat_ngram_size=NGRAM, bw_tokens=bw_tokens, bw_off=bw_off, eos=EOS, min_new_tokens=MIN_NEW,
                                       out=out, status=status)

                def sample():
                    ops.sample_rows(logits, choice, state=state, seen=seen, draws=draws, stream_id=sid, seed=1, **SAMPLER)

                def via_torch():
                    h = torch.cat((h64, last[:, None]), dim=1)
                    win = h.unfold(1, NGRAM, 1)
                    match = (win[:, :, : NGRAM - 1] == h[:, None, -(NGRAM - 1):]).all(-1)
                    o = logits.scatter_reduce(1, win[:, :, NGRAM - 1], torch.where(match, neg, pos), reduce="amin")
                    o[:, EOS] = neg
                    for w in WORDS:                                # the last token of a word whose other tokens end the history
                        hit = torch.ones((rows,), dtype=torch.bool, device=dev)
                        for j, t in enumerate(w[:-1]):
                            hit = hit & (h[:, j - len(w) + 1] == t)
                        o[:, w[-1]] = torch.where(hit, neg, o[:, w[-1]])
                    return o

                cands = {"constrain": constrain, "sample": sample, "torch": via_torch}
                for fn in cands.values():                          # warm: code objects, allocator
                    hist_len.copy_(hist_len0)
                    event_us(fn, 5)
                times = {k: [] for k in cands}
                for _ in range(args.rounds):
                    for k, fn in cands.items():
                        seen.copy_(seen0)                          # every timing starts from the same bitmaps and the same lengths
                        hist_len.copy_(hist_len0)
                        times[k].append(event_us(fn, args.iters))
                assert int(status.item()) == 0, "a history row filled up: the timing did not append what it claims"
                cell = {"vocab": vocab, "rows": rows, "history": length}
                for k, v in times.items():
                    cell[k + "_us"] = round(statistics.median(v), 2)
                    cell[k + "_min_max_us"] = [round(min(v), 2), round(max(v), 2)]
                cell["no_slower_than_sample"] = cell["constrain_us"] <= cell["sample_us"]
                cell["torch_over_constrain"] = round(cell["torch_us"] / cell["constrain_us"], 2)
                res["cells"].append(cell)
                print(json.dumps(cell), file=sys.stderr, flush=True)
    res["condition_holds"] = all(c["no_slower_than_sample"] for c in res["cells"])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)
    slower = [c for c in res["cells"] if not c["no_slower_than_sample"]]
    if slower:
        for c in slower:
            print(f"CONDITION FAILED: vocab {c['vocab']} rows {c['rows']} history {c['history']}: constrain {c['constrain_us']} us > "
                  f"sample {c['sample_us']} us", file=sys.stderr, flush=True)
        raise SystemExit(1)


if __name__ == "__main__":
    main()
