#!/usr/bin/env python3
"""In-flight generation on the MPT backbone, and what the fused decode front returns: a same-run A/B of ``fuse_decode_qk``.

MPT-1B dimensions (d_model 2048, 16 heads, 24 blocks, expansion 4, vocabulary 50432, qk_ln, clip_qkv 6, no biases: the configuration
of mpt-1b-redpajama-200b) with random weights, synthetic examples: one 512-d audio frame (a CLAP clip) between its start / end tokens,
a prompt text of 8-80 tokens and a seeded answer budget of 16-256 tokens (random weights never stop on their own; keyword and EOS
stops are off).  For every slot count of --slots (default 1, 8, 16, 32, 64; above 16 the decode products run on ops.gemm16_mid) the
engine's ``fuse_decode_qk`` is switched off and on in THIS process, alternating which side goes first, and each side records

  * clips/s of ``generate_inflight`` over the examples (4 per slot, at least 8),
  * the wall-clock ms of the ragged decode step with every slot active,
  * the device time per step of the attention front -- everything between the qkv product and out_proj: one launch fused
    (``ops.mpt_attn_decode_rows``), four unfused (clamp_f32_, layernorm_f32_ x 2, attn_decode_rope_rows) -- from the ops kernel timers,

plus the fused / unfused ratios and the number of examples whose tokens are equal on both sides.  Prints ONE JSON line and writes it to
--out (default profiles/bench_mpt_generate_inflight.json).

    python scripts/bench_mpt_generate_inflight.py [--slots 1,8,16,32,64] [--precision split] [--seed 0] [--out FILE]
"""
import argparse
import json
import os
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from llark_amd import ops  # noqa: E402
from llark_amd.m2t.infer_driver import generate_inflight  # noqa: E402
from llark_amd.m2t.mpt_engine import HipMptEngine, MptDims  # noqa: E402

VOCAB, START, END, PATCH = 50432, 50431, 50430, 50429
MM = 512


class RandomMpt:
    """What generate_inflight needs of a WrappedMPTForCausalLM, over a HipMptEngine with random MPT-1B weights made on the device."""

    audio_patch_branch = True

    def __init__(self, precision: str, max_batch: int, max_seq: int):
        dims = MptDims(vocab_size=VOCAB, qk_ln=True, clip_qkv=6.0, mm_hidden_size=MM, max_seq_len=2048)
        eng = HipMptEngine(dims, "cuda", max_batch=max_batch, max_seq=max_seq, precision=precision)
        g = torch.Generator(device="cuda").manual_seed(0)
        D, E = dims.d_model, dims.expansion_ratio * dims.d_model

        def n(*shape):
            return torch.randn(*shape, generator=g, device="cuda", dtype=torch.float32) * 0.02

        sd = {"transformer.wte.weight": n(VOCAB, D), "transformer.norm_f.weight": torch.ones(D), "transformer.mm_projector.weight": n(D, MM),
              "transformer.mm_projector.bias": torch.zeros(D)}
        for i in range(dims.n_layers):
            p = f"transformer.blocks.{i}"
            sd[f"{p}.attn.Wqkv.weight"], sd[f"{p}.attn.out_proj.weight"] = n(3 * D, D), n(D, D)
            sd[f"{p}.ffn.up_proj.weight"], sd[f"{p}.ffn.down_proj.weight"] = n(E, D), n(D, E)
            for name in ("norm_1", "norm_2", "attn.q_ln", "attn.k_ln"):
                sd[f"{p}.{name}.weight"] = torch.ones(D)
        eng.load_state_dict(sd)
        self.engine = eng
        ac = types.SimpleNamespace(use_audio_start_end=True, audio_start_token=START, audio_end_token=END, audio_patch_token=PATCH)
        self.model = types.SimpleNamespace(audio_encoder_config=ac)

    def get_model(self):
        return self.model


def make_examples(n: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        text = int(torch.randint(8, 81, (1,), generator=g))
        budget = int(torch.randint(16, 257, (1,), generator=g))
        ids = torch.tensor([1, START, PATCH, END] + torch.randint(3, 50000, (text,), generator=g).tolist())
        out.append((ids, torch.randn(1, MM, generator=g), budget))
    return out


def run_inflight(model, examples, slots):
    return dict(generate_inflight(model, iter((ids, enc.cuda(), b) for ids, enc, b in examples), slots=slots, keywords=()))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


def full_step(model, examples, n_slots, steps=32):
    """every slot active: wall-clock ms per decode step, device ms per step of the attention front and of its attention launch"""
    eng = model.engine
    eng.init_slots(n_slots)
    rows = [examples[i % len(examples)] for i in range(n_slots)]
    logits = eng.prefill_slots([r[0].cuda() for r in rows], [(k, 1, r[1].cuda()) for k, r in enumerate(rows)], range(n_slots))
    ids = logits.argmax(-1)
    for _ in range(4):
        ids, _, _ = eng.decode_slots(ids)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ids, _, _ = eng.decode_slots(ids)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    ops.start_kernel_timing()
    for _ in range(4):
        ids, _, _ = eng.decode_slots(ids)
    tags = ops.stop_kernel_timing()
    attn = sum(v[1] for k, v in tags.items() if k in ("mpt_attn_decode_rows", "attn_decode_rope_rows")) / 4
    return {"decode_step_ms": round(ms, 3), "front_ms_per_step": round(tags["mpt_decode_front"][1] / 4, 3),
            "attention_launch_ms_per_step": round(attn, 3), "front_launches_per_block": 1 if eng.fuse_decode_qk else 4}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--slots", default="1,8,16,32,64", help="slot counts, 1 .. 64 each")
    ap.add_argument("--precision", default="split", choices=["split", "bf16"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_mpt_generate_inflight.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mpt_generate_inflight needs the GPU")
    slot_list = [int(x) for x in args.slots.split(",") if x]
    if not slot_list or any(not 1 <= n <= 64 for n in slot_list):
        ap.error(f"--slots takes counts in 1 .. 64, got {args.slots!r}")
    examples = make_examples(max(8, 4 * max(slot_list)), args.seed)
    max_seq = max(ids.numel() + b for ids, _, b in examples) + 8
    model = RandomMpt(args.precision, max(slot_list), max_seq)
    eng = model.engine
    for slots in slot_list:                                   # warm-up: every launch sequence once
        for fuse in (False, True):
            eng.fuse_decode_qk = fuse
            run_inflight(model, [(i, e, 4) for i, e, _ in examples[: max(8, slots)]], slots)
    res = {"bench": "mpt_generate_inflight", "model": "mpt-1b dims (qk_ln, clip_qkv 6), random weights", "precision": args.precision,
           "prompt_tokens": [min(e[0].numel() for e in examples), max(e[0].numel() for e in examples)],
           "launches_per_block": {"unfused": 11, "fused": 8}, "cells": []}
    for c, slots in enumerate(slot_list):
        ex = examples[: max(8, 4 * slots)]
        cell = {"slots": slots, "examples": len(ex), "generated_tokens": sum(e[2] for e in ex)}
        outs = {}
        for fuse in ((False, True) if c % 2 == 0 else (True, False)):
            eng.fuse_decode_qk = fuse
            o, t = timed(lambda: run_inflight(model, ex, slots))
            assert all(o[i].numel() == ex[i][0].numel() + ex[i][2] for i in range(len(ex)))
            outs[fuse] = o
            row = {"s": round(t, 3), "clips_per_s": round(len(ex) / t, 3), "tokens_per_s": round(cell["generated_tokens"] / t, 1)}
            row.update(full_step(model, ex, slots))
            cell["fused" if fuse else "unfused"] = row
        cell["outputs_equal"] = sum(torch.equal(outs[True][i].cpu(), outs[False][i].cpu()) for i in range(len(ex)))
        cell["fused_over_unfused"] = {k: round(cell["fused"][k] / cell["unfused"][k], 4)
                                      for k in ("clips_per_s", "decode_step_ms", "front_ms_per_step")}
        res["cells"].append(cell)
        print(json.dumps(cell), file=sys.stderr, flush=True)
    eng.fuse_decode_qk = True
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
