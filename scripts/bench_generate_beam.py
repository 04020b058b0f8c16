#!/usr/bin/env python3
"""The beam-search decode step at Llama-2-7B dimensions (random weights) against the greedy step at the same slot count, same run.

4 examples x 4 beams (16 slots) and 4 examples x 16 beams (64 slots): the prompts (303 - 321 positions: 240 audio frames + text) are prefilled
once per example and cloned (engine.clone_slots); then blocks of --steps engine.beam_step calls (decode step up to the logits +
beam_topk_rows + beam_advance + kv_copy_slots, one device-to-host transfer) and of --steps engine.decode_slots calls (greedy) alternate
on the same slots, wall time per block between synchronisations.  The K/V move is reported on its own: the launch timed alone between
two events on the copy list of each beam block's last step, and the bytes that list moves.  Random weights never close a hypothesis,
so every step runs all slots.  Writes profiles/bench_generate_beam.json and prints it as ONE JSON line.

    python scripts/bench_generate_beam.py [--steps 8] [--blocks 6] [--precision split] [--out profiles/bench_generate_beam.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_generate_inflight import RandomLlama, make_examples  # noqa: E402
from llark_amd import ops  # noqa: E402
from llark_amd.m2t.beam import BeamSearch  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--precision", default="split", choices=["split", "bf16"])
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_generate_beam.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_generate_beam needs the GPU")
    steps, blocks = args.steps, args.blocks
    examples = [e for e in make_examples(16, args.seed) if e[0].numel() > 300][:4]
    n_ex = len(examples)
    total = steps * (2 * blocks + 2) + 2
    max_seq = max(ids.numel() for ids, _, _ in examples) + 8 + total
    model = RandomLlama(args.precision, 64, max_seq)
    eng = model.engine
    d = eng.dims
    planes = 2 if eng.split else 1
    res = {"bench": "generate_beam", "model": "llama2-7b dims, random weights", "precision": args.precision, "examples": n_ex,
           "prompt_lens": [int(e[0].numel()) for e in examples], "steps_per_block": steps, "blocks": blocks, "beams": {}}
    for beams in (4, 16):
        n = n_ex * beams
        eng.init_slots(n)
        roots = [e * beams for e in range(n_ex)]
        logits = eng.prefill_slots([r[0].cuda() for r in examples], [(k, 1, r[1].cuda()) for k, r in enumerate(examples)], roots)
        for b in roots:
            eng.clone_slots(b, range(b + 1, b + beams))
        beam = BeamSearch(n_ex, beams, logits.shape[-1], total, eng.device)
        beam.admit([int(e[0].numel()) for e in examples])
        ids, _ = eng.beam_step(None, beam, logits=logits.repeat_interleave(beams, dim=0))
        ids = ids.clone()
        moves = []

        def block(kind):
            nonlocal ids
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                if kind == "beam":
                    ids, done = eng.beam_step(ids, beam)
                else:
                    ids, _, _ = eng.decode_slots(ids)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / steps * 1e3
            if kind == "beam":
                assert not any(done)
                cnt = beam.pair_count.cpu().tolist()
                pairs, pos, p0 = beam.pairs.cpu(), eng.slot_len.cpu(), beam.p0.cpu()
                span = [int(pos[pairs[e, i, 0]] - p0[pairs[e, i, 1]]) for e in range(n_ex) for i in range(cnt[e])]
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                mx = max(1, max(beam.len_host[e] - 1 - beam.p0_host[e] for e in range(n_ex)))
                a.record()
                for _ in range(10):                              # the same list again: the copies are idempotent
                    ops.kv_copy_slots(eng.k_cache, eng.vt_cache, beam.pairs, beam.pair_count, beam.p0, eng.slot_len, mx, eng.k_cache_lo, eng.vt_cache_lo)
                b.record()
                b.synchronize()
                moves.append({"pairs": sum(cnt), "bytes": sum(span) * d.num_hidden_layers * d.hidden_size * 2 * 2 * planes,
                              "us": a.elapsed_time(b) * 1e3 / 10})
            else:                                                # the greedy steps moved the slots on: the search's own lengths follow
                beam.len_host = [x + steps for x in beam.len_host]
                beam.cur_len += steps
            return ms

        block("beam"), block("greedy")                           # warm
        moves.clear()
        ms = {"beam": [], "greedy": []}
        for k in range(blocks):
            for kind in (("greedy", "beam") if k % 2 == 0 else ("beam", "greedy")):
                ms[kind].append(block(kind))
        med = {k: statistics.median(v) for k, v in ms.items()}
        cell = {"slots": n, "greedy_step_ms": round(med["greedy"], 4), "beam_step_ms": round(med["beam"], 4),
                "greedy_min_max_ms": [round(min(ms["greedy"]), 4), round(max(ms["greedy"]), 4)],
                "beam_min_max_ms": [round(min(ms["beam"]), 4), round(max(ms["beam"]), 4)],
                "excess_fraction_of_step": round(med["beam"] / med["greedy"] - 1.0, 4),
                "kv_move_pairs_per_step": round(statistics.mean(m["pairs"] for m in moves), 2),
                "kv_move_bytes_per_step": int(statistics.mean(m["bytes"] for m in moves)),
                "kv_move_us_per_step": round(statistics.median(m["us"] for m in moves), 2)}
        res["beams"][str(beams)] = cell
        print(json.dumps({str(beams): cell}), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
