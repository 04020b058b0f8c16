#!/usr/bin/env python3
"""Normalised C-ABI launch trace of the Llama (and MPT) engine in every mode: 7B width, 2 layers, random weights, both precisions.

One line per launch: the symbol and every non-pointer argument verbatim; each pointer (and the stream handle) becomes a token numbered
by first appearance within its trace (p0, p1, ...), None stays None -- order, shapes, flags and aliasing without addresses.  A host-side
refactor of the engines must leave this output byte-identical:

    python scripts/engine_launch_trace.py > before.txt    # on the parent commit;  > after.txt on the branch;  diff before.txt after.txt
"""
import os
import sys
import types
from ctypes import c_void_p

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llark_amd import _lib, ops  # noqa: E402
from llark_amd.m2t import bench_support as BS  # noqa: E402

KNOBS = dict(fuse_decode_norm=False, fuse_decode_norm_a="auto", decode_graph=False, decode_replay=False, fuse_decode_rope=True,
             decode_chain=False, fuse_prefill_rope="auto", prefill_streams=1)


def show(title, calls):
    print(f"== {title}: {len(calls)} launches")
    tok = {}
    for _, name, args, _ in calls:
        sig = _lib._SIGS[name]
        print(name + "(" + ", ".join(repr(a) if sig[j] is not c_void_p or a is None else tok.setdefault(a, f"p{len(tok)}")
                                     for j, a in enumerate(args)) + ")")


def trace(title, fn):
    """The bf16 planes of spliced audio frames (ops.split16's results) are kept alive for the length of a trace.  This is not cosmetic:
    when those temporaries die IS a host-side property that a refactor can move, and without the pin it shows in the pointer tokens.
    When the splice became embed_splice, the planes started to die as that function returns instead of at the end of the caller's frame;
    in slot mode the caching allocator then hands their block to the head's x16, and the unpinned traces of the two versions differ in
    pointer numbering (same launches, order and non-pointer arguments).  The earlier free is safe -- allocation and use are ordered on
    one stream, and the side streams wait on the caller's -- but the pin hides it, so a change in a temporary's lifetime has to be
    judged by reading the code, not by this trace."""
    calls, pinned, split16 = [], [], ops.split16
    ops.split16 = lambda *a, **kw: pinned.append(split16(*a, **kw)) or pinned[-1]
    _lib.set_recorder(calls)
    try:
        fn()
    finally:
        _lib.set_recorder(None)
        ops.split16 = split16
    torch.cuda.synchronize()
    show(title, calls)


def llama(precision):
    w = BS.LLMWorkload(types.SimpleNamespace(batch=8, llm_precision=precision), "cuda", layers=2)
    eng, ids, emb = w.engine, w.ids, torch.randn(8, 16, 4800, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    fw = eng.forward_tokens

    def decode(B, steps=2, **kw):                              # short prefill, then greedy steps
        nxt = fw(ids[:B, :8], last_only=True)[:, -1].argmax(-1, keepdim=True)
        for _ in range(steps):
            nxt = fw(nxt, (), pos0=eng.cur_len, **kw)[:, -1].argmax(-1, keepdim=True)

    def replay():
        # Recorders do not nest, so the recording call's own LaunchList IS its trace.  A replay re-issues exactly that list through the
        # raw functions, which no recorder sees: there is nothing more to print for it.
        decode(1, steps=1)
        show(f"{precision} decode_replay B=1, recorded list", eng._dec[1]["list"].calls)

    def slots():
        eng.init_slots(4)
        rows = [ids[0, :5], ids[1, :40], ids[2, :7]]
        nxt = torch.zeros(4, dtype=torch.int64, device="cuda")
        nxt[[0, 1, 3]] = eng.prefill_slots(rows, [(1, 1, emb[1])], slots=[0, 1, 3]).argmax(-1)
        for _ in range(2):
            nxt, _, _ = eng.decode_slots(nxt)
        eng.release_slots([1])
        nxt[1] = eng.prefill_slots([ids[3, :33]], slots=[1]).argmax(-1)[0]
        eng.decode_slots(nxt)

    configs = [
        ("prefill B=8 S=371 auto", {}, lambda: fw(ids)),
        ("prefill B=2 S=5", {}, lambda: fw(ids[:2, :5])),
        ("prefill continuation S=40 at pos0=8", {}, lambda: (fw(ids[:, :8]), fw(ids[:, 8:48], pos0=8))),
        ("prefill fuse_rope=0", dict(fuse_prefill_rope="0"), lambda: fw(ids)),
        ("prefill fuse_rope=1 B=8 S=40", dict(fuse_prefill_rope="1"), lambda: fw(ids[:, :40])),
        ("prefill two streams B=8 S=371", dict(prefill_streams=2), lambda: fw(ids)),
        ("prefill num_layers=1", {}, lambda: fw(ids, num_layers=1)),
        ("prefill last_only", {}, lambda: fw(ids, last_only=True)),
        ("prefill return_hidden", {}, lambda: fw(ids, return_hidden=True)),
        ("prefill hidden_sink", {}, lambda: fw(ids[:, :40], hidden_sink=[])),
        ("prefill one audio segment", {}, lambda: fw(ids[:2], [(1, 1, emb[1])])),
        ("S=1 at pos0=0", {}, lambda: fw(ids[:1, :1])),
        ("decode B=1", {}, lambda: decode(1)),
        ("decode B=5", {}, lambda: decode(5)),
        ("decode B=1 hidden_sink", {}, lambda: decode(1, hidden_sink=[])),
        ("decode fuse_decode_norm B=1", dict(fuse_decode_norm=True), lambda: decode(1)),
        ("decode fuse_decode_norm B=5 hidden_sink", dict(fuse_decode_norm=True), lambda: decode(5, hidden_sink=[])),
        ("decode norm_a=1 B=5", dict(fuse_decode_norm_a="1"), lambda: decode(5)),
        ("decode norm_a=0 B=1", dict(fuse_decode_norm_a="0"), lambda: decode(1)),
        ("decode fuse_decode_rope=False B=1", dict(fuse_decode_rope=False), lambda: decode(1)),
        ("decode_graph B=1, first (eager) call", dict(decode_graph=True), lambda: decode(1, steps=1)),
        ("decode_chain B=1", dict(decode_chain=True), lambda: decode(1)),
        ("slot mode", {}, slots),
    ]
    for title, knobs, fn in configs:
        for k, v in {**KNOBS, **knobs}.items():
            setattr(eng, k, v)
        eng._dec.clear()
        trace(f"{precision} {title}", fn)
    for k, v in {**KNOBS, "decode_replay": True}.items():
        setattr(eng, k, v)
    eng._dec.clear()
    replay()


def mpt(precision):
    w = BS.MptWorkload(types.SimpleNamespace(batch=2, llm_precision=precision), "cuda")
    fw = w.engine.forward_tokens

    def run():
        nxt = fw(w.ids, [(1, 1, w.emb[1])], last_only=True, num_layers=2)[:, -1].argmax(-1, keepdim=True)
        fw(nxt, (), pos0=w.engine.cur_len, num_layers=2)

    trace(f"mpt {precision} prefill with one audio segment + decode", run)


if __name__ == "__main__":
    for p in ("bf16", "split"):
        llama(p)
        mpt(p)
