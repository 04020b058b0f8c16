#!/usr/bin/env python3
"""Speculative greedy decoding at Llama-2-7B dimensions (random weights), one slot, a 371-position prompt (240 audio frames + text).

1. The block step (engine.decode_block, drafts handed in so that the block holds 1 / 2 / 4 / 8 rows) against the plain
   engine.decode_slots step: blocks of --steps calls alternate in one process on the same slot, wall time per block between
   synchronisations (host launch cost included, as in a real loop).  break_even = t(block) / t(plain) - 1: the accepted drafts per
   step above which the block step wins.
2. The block attention launch alone against `blk` rows-kernel launches at the same position (launch-to-launch time, host included).
3. generate(max_new_tokens=--new) plain, with a scripted perfect drafter built from the plain run's tokens (upper bound) and with a
   drafter that is always wrong (the overhead when nothing is accepted), K = 7, alternating; tokens/s, block steps, and whether the
   completion equals the plain run's token for token.

Writes profiles/bench_generate_speculative.json and prints it as ONE JSON line.

    timeout -k 10 400 python scripts/bench_generate_speculative.py [--steps 8] [--blocks 5] [--new 64] [--precision split]
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
from bench_generate_inflight import RandomLlama  # noqa: E402
from llark_amd import ops  # noqa: E402
from llark_amd.m2t import bench_support as BS  # noqa: E402

PROMPT = 371


def med(xs):
    return {"median": round(statistics.median(xs), 4), "range": [round(min(xs), 4), round(max(xs), 4)]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--precision", default="split", choices=["split", "bf16"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_generate_speculative.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_generate_speculative needs the GPU")
    steps, blocks = args.steps, args.blocks
    g = torch.Generator().manual_seed(3)
    frames = 240
    text = PROMPT - frames - 3
    ids = torch.tensor([1, BS.START] + [BS.PATCH] * frames + [BS.END] + torch.randint(3, 32000, (text,), generator=g).tolist())
    enc = torch.randn(frames, 4800, generator=g)
    sizes = (1, 2, 4, 8)
    max_seq = (PROMPT + 8 + steps * (blocks + 1) * (1 + sum(sizes)) + 7) // 8 * 8
    model = RandomLlama(args.precision, 1, max_seq)
    eng = model.engine
    res = {"bench": "generate_speculative", "model": "llama2-7b dims, random weights", "precision": args.precision, "prompt": PROMPT,
           "steps_per_block": steps, "blocks": blocks, "max_seq": max_seq}

    # ---- 1. the step
    eng.init_slots(1)
    logits = eng.prefill_slots([ids.cuda()], [(0, 1, enc.cuda())], [0])
    nxt, _ = eng.advance_slots(logits, advance=False)
    eng.init_block_decode(8)
    eng.start_block_decode([torch.cat((ids, nxt.cpu()))], [1 << 20])
    drafts = torch.randint(3, 32000, (1, 8), generator=g).cuda()

    def run(blk):
        nonlocal nxt
        nd = torch.tensor([blk - 1], dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            if blk == 0:
                nxt, _, _ = eng.decode_slots(nxt)
            else:
                eng.decode_block(k_max=7, drafts=drafts, n_drafts=nd)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    for blk in (0,) + sizes:
        run(blk)
    t = {blk: [] for blk in (0,) + sizes}
    for n in range(blocks):
        order = (0,) + sizes if n % 2 == 0 else tuple(reversed(sizes)) + (0,)
        for blk in order:
            t[blk].append(run(blk))
    res["step_ms"] = {"plain": med(t[0]), **{f"block{blk}": med(t[blk]) for blk in sizes}}
    res["break_even_accepted_per_step"] = {f"block{blk}": round(statistics.median(t[blk]) / statistics.median(t[0]) - 1, 3) for blk in sizes}
    res["final_position"] = eng.slot_len_host[0]

    # ---- 2. the attention launch alone, layer 0's caches at the prompt's end
    d = eng.dims
    nh, hd = d.num_attention_heads, d.head_dim
    kc, vc, kcl, vcl = eng._kv_views(0, 0, 1)
    ws = eng._block_ws
    pos = torch.tensor([PROMPT], dtype=torch.int32, device="cuda")
    att, attl = ws["att"], ws["att_lo"]
    att1, att1l = att[:1], (None if attl is None else attl[:1])
    rows_qkv = [ws["qkv"][i:i + 1].contiguous() for i in range(8)]
    pos_i = [torch.tensor([PROMPT + i], dtype=torch.int32, device="cuda") for i in range(8)]
    res["attention_us"] = {}
    for blk in sizes:
        blk_t = torch.tensor([blk], dtype=torch.int32, device="cuda")

        def block():
            ops.attn_decode_rope_block(ws["qkv"], 1, 8, nh, hd, blk_t, pos, eng.cos, eng.sin, kc, vc, att, kcl, vcl, attl)

        def rows():
            for i in range(blk):
                ops.attn_decode_rope_rows(rows_qkv[i], 1, nh, hd, pos_i[i], eng.cos, eng.sin, kc, vc, att1, kcl, vcl, att1l)

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(20):
                fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1e3 / 20

        timed(block), timed(rows)
        tb, tr = [], []
        for n in range(blocks):
            for fn, acc in ((block, tb), (rows, tr)) if n % 2 == 0 else ((rows, tr), (block, tb)):
                acc.append(timed(fn))
        res["attention_us"][f"block{blk}"] = {"block": med(tb), "rows": med(tr)}

    # ---- 3. generate
    inp = dict(input_ids=ids[None].cuda(), audio_encodings=enc[None].cuda(), max_new_tokens=args.new, eos_token_id=-1)
    plain = model.generate(**inp).cpu()
    new = plain[0, PROMPT:].tolist()
    drafters = {"plain": None, "perfect": lambda b, got: new[len(got):], "wrong": lambda b, got: [(x + 1) % 32000 for x in new[len(got):]]}
    tg = {k: [] for k in drafters}
    info = {}
    for n in range(3):
        for kind in (list(drafters) if n % 2 == 0 else list(reversed(drafters))):
            stats = {}
            model.speculation_drafter, model.speculation_stats = drafters[kind], stats
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = model.generate(**inp, **({} if kind == "plain" else dict(prompt_lookup_num_tokens=7)))
            torch.cuda.synchronize()
            tg[kind].append(args.new / (time.perf_counter() - t0))
            info[kind] = {"equals_plain": bool(torch.equal(out.cpu(), plain)), **stats}
    del model.speculation_drafter, model.speculation_stats
    res["generate_tokens_per_s"] = {k: {**med(tg[k]), **info[k]} for k in drafters}
    res["new_tokens"] = args.new
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
