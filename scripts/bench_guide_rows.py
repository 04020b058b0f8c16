#!/usr/bin/env python3
"""Device time of the guide launch (ops.guide_rows) next to the sampling launch, the constraint launch and torch, same process, alternating.

For 1 / 16 / 64 rows x vocab 32 003 (Llama with its audio tokens) and 50 435 (MPT) x a choice set of 24 sequences (the keys) and one of
1 000 sequences, as a decode step launches it -- every row steps from its set's root by a first token of the set, then the row is
streamed:
  guide     -- ops.guide_rows writing the processed rows and the open-column counts (what DeviceGuide.process launches);
  sample    -- ops.sample_rows on the same logits with all four processors on (temperature 0.7, top-k 200, top-p 0.95, penalty 1.3);
  constrain -- ops.constrain_rows (n-gram 3 over a 300-token history, three bad words, the EOS rule, the step's token appended);
  torch     -- a callable that does the same step and applies the same mask to GPU tensors (the children as a padded [nodes, widest
               fan-out] table: compare, gather, one scatter into a -inf mask, add; no transfer).
Condition: at every point guide is below sample in the same run (it streams the row once and selects nothing); "condition_holds" says so,
and the script names the other cells and exits with status 1 when it does not hold.  constrain and torch are reported, not gated.
Each figure is the median over --rounds rounds of the mean of --iters back-to-back launches between two events; within a round the
candidates run in turn.  Writes profiles/guide_rows.json and prints it as ONE JSON line.

    python scripts/bench_guide_rows.py [--iters 50] [--rounds 9] [--out profiles/guide_rows.json]
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
from llark_amd.m2t.guide import ChoiceSets  # noqa: E402

NGRAM, EOS, MIN_NEW, HISTORY = 3, 2, 1 << 20, 300
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


def choice_set(n_seq, vocab, seed):
    """n_seq distinct sequences of 2 .. 4 tokens whose first tokens come from a small alphabet, so that inner nodes fan out."""
    g = torch.Generator().manual_seed(seed)
    firsts = torch.randint(3, vocab, (max(4, n_seq // 25),), generator=g).tolist()
    seqs = set()
    while len(seqs) < n_seq:
        n = int(torch.randint(2, 5, (1,), generator=g))
        seqs.add((firsts[int(torch.randint(0, len(firsts), (1,), generator=g))],) + tuple(torch.randint(3, vocab, (n - 1,), generator=g).tolist()))
    return sorted(seqs)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guide_rows.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_guide_rows needs the GPU")
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    i32 = dict(dtype=torch.int32, device=dev)
    res = {"bench": "guide_rows", "device": ops.device_info()[1], "iters": args.iters, "rounds": args.rounds, "unit": "us per launch",
           "sampler": SAMPLER, "constrain": dict(no_repeat_ngram_size=NGRAM, history=HISTORY, bad_words=len(WORDS)), "cells": []}
    for vocab in (32003, 50435):
        for rows in (1, 16, 64):
            logits = 3.0 * torch.randn((rows, vocab), generator=g, device=dev)
            up = torch.randint(0, vocab, (rows, 5), generator=g, device=dev)
            logits.scatter_add_(1, up, 6.0 + 4.0 * torch.rand((rows, 5), generator=g, device=dev))
            state = torch.full((rows,), ops.ROW_ACTIVE, **i32)
            # the sampler's and the constraint launch's state, as scripts/bench_constrain_rows.py sets it up
            width = HISTORY + args.iters + 8
            hist = torch.zeros((rows, width), **i32)
            hist[:, :HISTORY] = torch.randint(0, 500, (rows, HISTORY), generator=g, device=dev).to(torch.int32)
            hist_len0 = torch.full((rows,), HISTORY, **i32)
            hist_len = hist_len0.clone()
            prompt_len = torch.full((rows,), HISTORY // 2, **i32)
            last_c = torch.randint(0, 500, (rows,), generator=g, device=dev)
            bw_tokens = torch.tensor([t for w in WORDS for t in w], **i32)
            bw_off = torch.tensor([0, 1, 3, 6], **i32)
            out_c = torch.empty((rows, vocab), dtype=torch.float32, device=dev)
            status_c = torch.zeros((1,), **i32)
            seen = torch.zeros((rows, (vocab + 31) // 32), **i32)
            ops.seen_mark_rows(hist[:, :HISTORY].to(torch.int64).reshape(-1).contiguous(), torch.arange(rows, **i32) * HISTORY,
                               torch.full((rows,), HISTORY, **i32), seen, vocab)
            seen0 = seen.clone()
            draws = torch.zeros((rows,), **i32)
            sid = torch.arange(rows, dtype=torch.int64, device=dev)
            choice = torch.zeros((rows,), dtype=torch.int64, device=dev)
            for n_seq in (24, 1000):
                seqs = choice_set(n_seq, vocab, n_seq)
                off, tok, node, term, roots = ChoiceSets([seqs]).table(vocab)
                fan = (off[1:] - off[:-1]).tolist()
                tab = tuple(t.to(dev) for t in (off, tok, node, term))
                node_in = torch.full((rows,), roots[0], **i32)
                node_out = torch.empty((rows,), **i32)
                firsts = tok[off[roots[0]]:off[roots[0] + 1]]
                last = firsts[torch.arange(rows) % firsts.numel()].to(device=dev, dtype=torch.int64)
                out = torch.empty((rows, vocab), dtype=torch.float32, device=dev)
                n_open = torch.zeros((rows,), **i32)
                status = torch.zeros((1,), **i32)
                # torch's form of the table: [nodes, widest fan-out], padded with a repeat of the node's first child (eos for a leaf)
                wide = max(max(fan), 1)
                pad_tok = torch.full((len(fan), wide), EOS, dtype=torch.int64)
                pad_node = torch.full((len(fan), wide), ops.GUIDE_CLOSED, dtype=torch.int64)
                for n, k in enumerate(fan):
                    if k:
                        pad_tok[n, :k], pad_tok[n, k:] = tok[off[n]:off[n] + k], tok[off[n]]
                        pad_node[n, :k], pad_node[n, k:] = node[off[n]:off[n] + k], node[off[n]]
                pad_tok, pad_node, term_d = pad_tok.to(dev), pad_node.to(dev), term.to(dev).bool()
                node64 = node_in.to(torch.int64)
                neg = torch.full((), float("-inf"), device=dev)

                def guide():
                    ops.guide_rows(logits, *tab, node_in, node_out, eos=EOS, state=state, last_token=last, out=out, n_open=n_open, status=status)

                def sample():
                    ops.sample_rows(logits, choice, state=state, seen=seen, draws=draws, stream_id=sid, seed=1, **SAMPLER)

                def constrain():
                    ops.constrain_rows(logits, state=state, hist=hist, hist_len=hist_len, prompt_len=prompt_len, last_token=last_c,
                                       no_repeat_ngram_size=NGRAM, bw_tokens=bw_tokens, bw_off=bw_off, eos=EOS, min_new_tokens=MIN_NEW,
                                       out=out_c, status=status_c)

                def via_torch():
                    hit = pad_tok[node64] == last[:, None]
                    nxt = torch.where(hit.any(1), pad_node[node64].gather(1, hit.int().argmax(1, keepdim=True))[:, 0], -2)
                    mask = torch.full_like(logits, float("-inf")).scatter_(1, pad_tok[nxt], 0.0)
                    mask[:, EOS] = torch.where(term_d[nxt], 0.0, neg)
                    return logits + mask, nxt

                want, want_node = via_torch()                      # the candidates do the same work: the same rows, the same nodes
                guide()
                torch.cuda.synchronize()
                assert torch.equal(node_out.to(torch.int64), want_node) and torch.equal(torch.isneginf(out), torch.isneginf(want))
                assert int(status.item()) == 0 and int(n_open.min()) > 0
                cands = {"guide": guide, "sample": sample, "constrain": constrain, "torch": via_torch}
                for fn in cands.values():                          # warm: code objects, allocator
                    hist_len.copy_(hist_len0)
                    event_us(fn, 5)
                times = {k: [] for k in cands}
                for _ in range(args.rounds):
                    for k, fn in cands.items():
                        seen.copy_(seen0)                          # every timing starts from the same bitmaps and the same lengths
                        hist_len.copy_(hist_len0)
                        times[k].append(event_us(fn, args.iters))
                assert int(status_c.item()) == 0, "a history row filled up: the timing did not append what it claims"
                cell = {"vocab": vocab, "rows": rows, "sequences": n_seq, "nodes": len(fan), "widest_fan_out": max(fan)}
                for k, v in times.items():
                    cell[k + "_us"] = round(statistics.median(v), 2)
                    cell[k + "_min_max_us"] = [round(min(v), 2), round(max(v), 2)]
                cell["below_sample"] = cell["guide_us"] < cell["sample_us"]
                cell["torch_over_guide"] = round(cell["torch_us"] / cell["guide_us"], 2)
                res["cells"].append(cell)
                print(json.dumps(cell), file=sys.stderr, flush=True)
    res["condition_holds"] = all(c["below_sample"] for c in res["cells"])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)
    slower = [c for c in res["cells"] if not c["below_sample"]]
    if slower:
        for c in slower:
            print(f"CONDITION FAILED: vocab {c['vocab']} rows {c['rows']} sequences {c['sequences']}: guide {c['guide_us']} us >= "
                  f"sample {c['sample_us']} us", file=sys.stderr, flush=True)
        raise SystemExit(1)


if __name__ == "__main__":
    main()
