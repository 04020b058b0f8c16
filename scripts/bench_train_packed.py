"""Ragged training step at 7B dimensions (random weights): the existing loop -- one right-padded ``forward_backward`` per micro-batch --
against ``--pack_sequences`` -- the whole optimizer step as ONE packed stream on the variable-length attention kernels -- for full
fine-tuning and for LoRA r = 64, in ONE process on one GPU, the two modes alternating step by step on the SAME trainer after warm-up.

    python scripts/bench_train_packed.py [--steps 5] [--warmup 2] [--layers 32] [--recipes full,lora] [--out profiles/train_packed.json]

8 examples per optimizer step (micro-batch 2 x accumulation 4): the LLark prompt (371 prompt-and-audio tokens) plus a response, total
lengths drawn with a fixed seed from 300..700 and printed.  Per recipe and mode: ms per optimizer step (median and every sample),
rows processed per step, and -- from one more packed step with an event pair around every launch -- the time of the variable-length
attention forward and backward calls (the backward call = row-dot + dK/dV + dQ kernels) summed over the layers."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from llark_amd import ops  # noqa: E402
from llark_amd.m2t.bench_support import END, FRAMES, START, VOCAB, make_prompt_ids  # noqa: E402
from llark_amd.m2t.data import pack_sequences  # noqa: E402
from llark_amd.m2t.engine import HipLlamaEngine, LlamaDims  # noqa: E402
from llark_amd.m2t.lora import LoraConfig  # noqa: E402
from llark_amd.m2t.train_engine import HipLlamaTrainer  # noqa: E402

PAD_ID = 0


def examples(args, mm, device):
    """the step's examples: (ids, labels, audio frames) per example, and the lengths"""
    gen = torch.Generator().manual_seed(args.seed)
    n = args.micro * args.accum
    prompt = make_prompt_ids(n, seed=100)
    P = prompt.shape[1]
    lengths = torch.randint(max(args.min_len, P + 1), args.max_len + 1, (n,), generator=gen).tolist()
    out = []
    for b, ln in enumerate(lengths):
        ids = torch.cat([prompt[b], torch.randint(3, 32000, (ln - P,), generator=gen)])
        labels = ids.clone()
        labels[:P] = -100
        out.append((ids, labels, torch.randn(FRAMES, mm, generator=gen).to(device)))
    return out, lengths


def build(recipe: str, args, device, s_total: int):
    dims = LlamaDims(vocab_size=VOCAB)
    dims.num_hidden_layers = args.layers
    # two cache slots hold the longest micro-batch of the loop AND the packed stream: no cache is reallocated when the modes alternate
    eng = HipLlamaEngine(dims, device, max_batch=args.micro, max_seq=ops.round_up(max(args.max_len, -(-s_total // args.micro)), 64), precision="bf16")
    g = torch.Generator(device=device).manual_seed(0)
    H, I = dims.hidden_size, dims.intermediate_size

    def n(*shape):
        return (torch.randn(*shape, generator=g, device=device, dtype=torch.float32) * 0.02).to(torch.bfloat16)

    ones = torch.ones(H, device=device)
    for i in range(dims.num_hidden_layers):
        eng.set_layer(i, n(H, H), n(H, H), n(H, H), n(H, H), n(I, H), n(I, H), n(H, I), ones, ones)
    eng.set_globals(n(VOCAB, H), ones, n(VOCAB, H), n(H, dims.mm_hidden_size), torch.zeros(H, device=device))
    kw = {"lora": LoraConfig(r=args.lora_r, alpha=16)} if recipe == "lora" else {}
    tr = HipLlamaTrainer(eng, lr=5e-5, embed_grad_tokens=[START, END], **kw)
    if recipe == "lora":                               # non-zero B: at the zero initialisation dA is identically zero
        for name, p in tr.params:
            if name.endswith(".lora_B"):
                p[:, : args.lora_r].normal_(0.0, 0.01, generator=g)
        tr._refresh_lora()
    return eng, tr


def loop_step(tr, micro_batches, accum):
    for k, (ids, labels, segs) in enumerate(micro_batches):
        tr.forward_backward(ids, segs, labels, 1.0 / accum, last_micro_batch=k == accum - 1)
    tr.step(1, max_grad_norm=1.0)


def packed_step(tr, plan):
    tr.forward_backward_packed(None, None, None, None, last_micro_batch=True, plan=plan)
    tr.step(1, max_grad_norm=1.0)


def measure(recipe: str, args, device) -> dict:
    torch.cuda.empty_cache()
    dims = LlamaDims(vocab_size=VOCAB)
    ex, lengths = examples(args, dims.mm_hidden_size, device)
    plan = pack_sequences([e[0] for e in ex], [e[1] for e in ex], [args.micro] * args.accum, [(b, 1, e[2]) for b, e in enumerate(ex)], PAD_ID)
    micro_batches = []
    for k in range(args.accum):
        grp = ex[k * args.micro: (k + 1) * args.micro]
        S = max(int(e[0].numel()) for e in grp)
        ids = torch.full((args.micro, S), PAD_ID, dtype=torch.long)
        labels = torch.full((args.micro, S), -100, dtype=torch.long)
        for b, e in enumerate(grp):
            ids[b, : e[0].numel()], labels[b, : e[0].numel()] = e[0], e[1]
        micro_batches.append((ids.to(device), labels.to(device), [(b, 1, e[2]) for b, e in enumerate(grp)]))
    eng, tr = build(recipe, args, device, plan.s_total)
    for _ in range(args.warmup):
        loop_step(tr, micro_batches, args.accum)
        packed_step(tr, plan)
    torch.cuda.synchronize()
    ms = {"loop": [], "packed": []}
    for _ in range(args.steps):                          # the two modes alternate: what else runs on the box hits both alike
        for mode in ("loop", "packed"):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            loop_step(tr, micro_batches, args.accum) if mode == "loop" else packed_step(tr, plan)
            t1.record()
            torch.cuda.synchronize()
            ms[mode].append(t0.elapsed_time(t1))
    kernel_ms = {}
    for mode in ("loop", "packed"):                      # one more step of each with an event pair around every timed launch
        ops.start_kernel_timing()
        loop_step(tr, micro_batches, args.accum) if mode == "loop" else packed_step(tr, plan)
        timers = ops.stop_kernel_timing()
        kernel_ms[mode] = {k: {"launches": v[0], "ms": round(v[1], 3)} for k, v in sorted(timers.items(), key=lambda kv: -kv[1][1])}
    med = statistics.median
    out = {"lengths": lengths, "tokens_per_step": sum(lengths),
           "loop": {"ms_per_step": round(med(ms["loop"]), 2), "ms_per_step_all": [round(x, 2) for x in ms["loop"]],
                    "rows_per_step": sum(int(m[0].numel()) for m in micro_batches), "weight_passes": args.accum, "kernel_ms": kernel_ms["loop"]},
           "packed": {"ms_per_step": round(med(ms["packed"]), 2), "ms_per_step_all": [round(x, 2) for x in ms["packed"]],
                      "rows_per_step": plan.s_total, "weight_passes": 1, "kernel_ms": kernel_ms["packed"]}}
    out["packed_over_loop"] = round(out["packed"]["ms_per_step"] / out["loop"]["ms_per_step"], 4)
    out["attention_varlen_ms"] = {k: v for k, v in kernel_ms["packed"].items() if k.startswith("attn_")}
    del eng, tr
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--micro", type=int, default=2)
    ap.add_argument("--accum", type=int, default=4)
    ap.add_argument("--min_len", type=int, default=300)
    ap.add_argument("--max_len", type=int, default=700)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--lora_r", type=int, default=64)
    ap.add_argument("--recipes", default="full,lora")
    ap.add_argument("--out", default=os.path.join("profiles", "train_packed.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    res = {"shape": {"layers": args.layers, "micro_batch": args.micro, "accumulation": args.accum, "lengths_from": [args.min_len, args.max_len],
                     "seed": args.seed, "lora_r": args.lora_r}, "device": torch.cuda.get_device_name(0)}
    for recipe in args.recipes.split(","):
        res[recipe] = measure(recipe, args, device)
        print(recipe, "lengths", res[recipe]["lengths"], flush=True)
        print(recipe, json.dumps({m: {k: v for k, v in res[recipe][m].items() if k != "kernel_ms"} for m in ("loop", "packed")}),
              json.dumps(res[recipe]["attention_varlen_ms"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
