#!/usr/bin/env python3
"""Device time of the beam step's two row launches (ops.beam_topk_rows + ops.beam_advance) next to the torch callable they replace, same
process, alternating.

For N examples x B beams (B = 4 with N = 4, B = 16 with N = 4: 16 and 64 rows) x vocab 32 003 (Llama with its audio tokens) and 50 435 (MPT):
  beam   -- ops.beam_topk_rows over the N * B rows, then ops.beam_advance over the N examples (candidates, merge, heap, trellis, copy list);
  torch  -- what HF's beam_search does with the same logits: log_softmax + beam scores, viewed as [N][B * V], topk(2B) -- the selection
            alone, without the scorer's Python loop over the candidates, which the advance launch also replaces.
Each figure is the median over --rounds rounds of the mean of --iters back-to-back launches between two events; within a round the
candidates run in turn.  Logits: 3 * randn with five raised tokens per row (tests/logprob_ref.py's family).  Writes
profiles/beam_rows.json and prints it as ONE JSON line.

    python scripts/bench_beam_rows.py [--iters 50] [--rounds 9] [--out profiles/beam_rows.json]
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
from llark_amd.m2t.beam import BeamSearch  # noqa: E402


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_rows.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_beam_rows needs the GPU")
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    res = {"bench": "beam_rows", "device": ops.device_info()[1], "iters": args.iters, "rounds": args.rounds, "unit": "us per step",
           "cells": []}
    for vocab in (32003, 50435):
        for n_ex, beams in ((4, 4), (4, 16)):
            rows = n_ex * beams
            logits = 3.0 * torch.randn((rows, vocab), generator=g, device=dev)
            up = torch.randint(0, vocab, (rows, 5), generator=g, device=dev)
            logits.scatter_add_(1, up, 6.0 + 4.0 * torch.rand((rows, 5), generator=g, device=dev))
            bs = BeamSearch(n_ex, beams, vocab, 1, dev)
            bs.admit([371] * n_ex)
            bs.score.copy_(-5.0 * torch.rand((rows,), generator=g, device=dev))
            state = torch.full((rows,), ops.ROW_ACTIVE, dtype=torch.int32, device=dev)
            score0, rank0, cur0 = bs.score.clone(), bs.rank_of_slot.clone(), bs.cur_len.clone()

            def topk():
                ops.beam_topk_rows(logits, score0, beams, bs.cand_score, bs.cand_token, bs.cand_logprob, state=state)

            def advance():
                ops.beam_advance(bs.cand_score, bs.cand_token, bs.cand_logprob, n_ex, beams, 0, -1, 0, 1.0, False, bs.score, bs.rank_of_slot,
                                 state, None, bs.cur_len, bs.next_ids, bs.heap, bs.heap_meta, bs.done, bs.trellis, bs.pairs, bs.pair_count)

            def beam():
                topk()
                advance()

            def via_torch():
                lp = torch.log_softmax(logits, dim=-1) + score0[:, None]
                return torch.topk(lp.view(n_ex, beams * vocab), 2 * beams, dim=1, largest=True, sorted=True)

            cands = {"beam": beam, "topk_rows": topk, "advance": advance, "torch": via_torch}
            for fn in cands.values():                            # warm: code objects, allocator
                event_us(fn, 5)
            # the two agree on the best candidate of every example (rank 0 of the merged order)
            bs.score.copy_(score0), bs.rank_of_slot.copy_(rank0), bs.cur_len.copy_(cur0)
            beam()
            want = via_torch()
            got = bs.score.view(n_ex, beams).max(dim=1).values
            assert float((got - want.values[:, 0]).abs().max()) <= 1e-4, "the launches and the torch callable disagree"
            times = {k: [] for k in cands}
            for _ in range(args.rounds):
                for k, fn in cands.items():
                    times[k].append(event_us(fn, args.iters))
            cell = {"vocab": vocab, "examples": n_ex, "beams": beams, "rows": rows}
            for k, v in times.items():
                cell[k + "_us"] = round(statistics.median(v), 2)
                cell[k + "_min_max_us"] = [round(min(v), 2), round(max(v), 2)]
            cell["beam_over_torch"] = round(cell["beam_us"] / cell["torch_us"], 3)
            res["cells"].append(cell)
            print(json.dumps(cell), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
