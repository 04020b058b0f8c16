"""MPT backbone on the HIP kernels: the arithmetic the reference reaches through
``WrappedMPTForCausalLM.forward`` (m2t/models/mpt.py:74-245,259-330 -> m2t/llava/model/mpt/modeling_mpt.py forward ->
blocks.py MPTBlock -> attention.py MultiheadAttention / scaled_multihead_dot_product_attention).

Per block:  LayerNorm -> fused Wqkv GEMM (-> clip_qkv clamp -> qk_ln LayerNorm over q and k) -> head split + KV-cache write
(the RoPE kernel with an identity rotation table) -> causal attention with the ALiBi bias (same flash / decode kernels as
Llama, slopes passed in) -> out_proj GEMM with the residual fused -> LayerNorm -> up_proj GEMM -> exact GELU -> down_proj
GEMM with the residual fused.  Final LayerNorm, logits against the TIED ``wte`` (x ``logit_scale``).  Head dim must be
128 (MPT-1B: 2048 / 16) -- the attention kernels are built for it.

Precision modes are those of the Llama engine: "split" (bf16 hi+lo operands, fp32-class, matches the reference's fp32 CPU
path) and "bf16" (single pass).  Weights are bf16 like ``model.to(bf16)`` of the reference recipe.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from .. import ops
from .engine import embed_splice


@dataclass
class MptDims:
    d_model: int = 2048
    n_heads: int = 16
    n_layers: int = 24
    expansion_ratio: int = 4
    vocab_size: int = 50432
    max_seq_len: int = 2048
    alibi_bias_max: int = 8
    qk_ln: bool = False
    clip_qkv: Optional[float] = None
    logit_scale: Optional[float] = None
    ln_eps: float = 1e-5
    mm_hidden_size: int = 512

    @property
    def head_dim(self) -> int:
        return self.d_model // self.n_heads


def alibi_slopes(n_heads: int, alibi_bias_max: int = 8) -> torch.Tensor:
    """m2t/llava/model/mpt/attention.py:462-469 (gen_slopes), as a flat fp32 [n_heads] vector."""
    n = 2 ** math.ceil(math.log2(n_heads))
    m = torch.arange(1, n + 1, dtype=torch.float32) * (alibi_bias_max / n)
    slopes = 1.0 / torch.pow(2, m)
    if n != n_heads:
        slopes = torch.cat([slopes[1::2], slopes[::2]])[:n_heads]
    return slopes.contiguous()


class _Block:
    __slots__ = ("wqkv", "bqkv", "wo", "bo", "wup", "bup", "wdown", "bdown", "n1w", "n1b", "n2w", "n2b", "qlw", "qlb", "klw", "klb")


class HipMptEngine:
    def __init__(self, dims: MptDims, device="cuda", max_batch: int = 8, max_seq: int = 512, precision: str = "split"):
        if precision not in ("split", "bf16"):
            raise ValueError(f"precision must be 'split' or 'bf16', got {precision!r}")
        if dims.head_dim != 128:
            raise NotImplementedError(f"the HIP attention kernels are built for head_dim 128 (MPT-1B: 2048/16); got {dims.head_dim}")
        if dims.d_model % 64 or dims.mm_hidden_size % 32:
            raise NotImplementedError("d_model must be a multiple of 64 and mm_hidden_size of 32")
        self.dims, self.device = dims, torch.device(device)
        self.precision, self.split = precision, precision == "split"
        self.max_batch, self.smax = max_batch, ops.round_up(max_seq, 8)
        self.blocks: List[Optional[_Block]] = [None] * dims.n_layers
        self.wte = self.normf_w = self.normf_b = self.proj_w = self.proj_b = None
        self.slopes = alibi_slopes(dims.n_heads, dims.alibi_bias_max).to(self.device)
        self.fuse_decode_rope = os.environ.get("LLARK_DECODE_FUSE_ROPE", "1") != "0"      # head split + cache append inside the decode attention launch
        # ragged decode step: clamp + qk_ln + head split + cache append inside the attention launch (ops.mpt_attn_decode_rows); off = the
        # four launches clamp_f32_, layernorm_f32_ x 2, attn_decode_rope_rows with the identity tables
        self.fuse_decode_qk = os.environ.get("LLARK_MPT_FUSE_DECODE_QK", "1") != "0"
        # identity rotation: the RoPE kernel then only splits heads, rounds to bf16 (hi/lo) and writes the KV cache
        self.cos = torch.ones((self.smax, 64), dtype=torch.float32, device=self.device)
        self.sin = torch.zeros((self.smax, 64), dtype=torch.float32, device=self.device)
        self._ws, self._ws_key = {}, None
        self.k_cache = self.vt_cache = self.k_cache_lo = self.vt_cache_lo = None
        self.cur_len = self.cur_batch = 0
        self._slot_ws = None
        self._clear_slots()

    # ---- weights -------------------------------------------------------------------------------
    def _bf16(self, t):
        return None if t is None else t.detach().to(device=self.device, dtype=torch.bfloat16).contiguous()

    def _f32(self, t):
        return None if t is None else t.detach().to(device=self.device, dtype=torch.float32).contiguous()

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        """Reference names: ``transformer.wte.weight``, ``transformer.blocks.N.{norm_1,norm_2}.{weight,bias}``,
        ``...attn.{Wqkv,out_proj,q_ln,k_ln}.*``, ``...ffn.{up_proj,down_proj}.*``, ``transformer.norm_f.*``,
        ``transformer.mm_projector.*`` (biases optional: ``no_bias`` models have none)."""
        d = self.dims
        for i in range(d.n_layers):
            p = f"transformer.blocks.{i}"
            B = _Block()
            B.wqkv, B.bqkv = self._bf16(sd[f"{p}.attn.Wqkv.weight"]), self._f32(sd.get(f"{p}.attn.Wqkv.bias"))
            B.wo, B.bo = self._bf16(sd[f"{p}.attn.out_proj.weight"]), self._f32(sd.get(f"{p}.attn.out_proj.bias"))
            B.wup, B.bup = self._bf16(sd[f"{p}.ffn.up_proj.weight"]), self._f32(sd.get(f"{p}.ffn.up_proj.bias"))
            B.wdown, B.bdown = self._bf16(sd[f"{p}.ffn.down_proj.weight"]), self._f32(sd.get(f"{p}.ffn.down_proj.bias"))
            B.n1w, B.n1b = self._f32(sd[f"{p}.norm_1.weight"]), self._f32(sd.get(f"{p}.norm_1.bias"))
            B.n2w, B.n2b = self._f32(sd[f"{p}.norm_2.weight"]), self._f32(sd.get(f"{p}.norm_2.bias"))
            if d.qk_ln:
                B.qlw, B.qlb = self._f32(sd[f"{p}.attn.q_ln.weight"]), self._f32(sd.get(f"{p}.attn.q_ln.bias"))
                B.klw, B.klb = self._f32(sd[f"{p}.attn.k_ln.weight"]), self._f32(sd.get(f"{p}.attn.k_ln.bias"))
            else:
                B.qlw = B.qlb = B.klw = B.klb = None
            for t in (B.wqkv, B.wo, B.wup, B.wdown):
                ops.attach_frag(t, t.shape[0])
            self.blocks[i] = B
        self.wte = self._bf16(sd["transformer.wte.weight"])
        ops.attach_frag(self.wte, self.wte.shape[0])
        self.normf_w, self.normf_b = self._f32(sd["transformer.norm_f.weight"]), self._f32(sd.get("transformer.norm_f.bias"))
        if "transformer.mm_projector.weight" in sd:
            self.proj_w, self.proj_b = self._bf16(sd["transformer.mm_projector.weight"]), self._f32(sd["transformer.mm_projector.bias"])

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """The weights under the reference's names (those of :meth:`load_state_dict`) as VIEWS of the engine's own tensors -- every MPT
        tensor is stored as the reference lays it out (bf16 matrices, fp32 LayerNorm gains / biases), so writing into a value updates
        the engine (checkpoint resume: llark_amd/m2t/checkpoint.py)."""
        names = (("attn.Wqkv.weight", "wqkv"), ("attn.Wqkv.bias", "bqkv"), ("attn.out_proj.weight", "wo"), ("attn.out_proj.bias", "bo"),
                 ("ffn.up_proj.weight", "wup"), ("ffn.up_proj.bias", "bup"), ("ffn.down_proj.weight", "wdown"), ("ffn.down_proj.bias", "bdown"),
                 ("norm_1.weight", "n1w"), ("norm_1.bias", "n1b"), ("norm_2.weight", "n2w"), ("norm_2.bias", "n2b"),
                 ("attn.q_ln.weight", "qlw"), ("attn.q_ln.bias", "qlb"), ("attn.k_ln.weight", "klw"), ("attn.k_ln.bias", "klb"))
        sd = {"transformer.wte.weight": self.wte}
        for i, B in enumerate(self.blocks):
            for ref, nm in names:
                t = getattr(B, nm)
                if t is not None:
                    sd[f"transformer.blocks.{i}.{ref}"] = t
        sd["transformer.norm_f.weight"] = self.normf_w
        if self.normf_b is not None:
            sd["transformer.norm_f.bias"] = self.normf_b
        if self.proj_w is not None:
            sd["transformer.mm_projector.weight"], sd["transformer.mm_projector.bias"] = self.proj_w, self.proj_b
        return sd

    # ---- buffers -------------------------------------------------------------------------------
    def _workspace(self, batch: int, s: int):
        if self._ws_key != (batch, s):
            self._ws, self._ws_key = self._alloc_workspace(batch, s), (batch, s)
        return self._ws

    def _alloc_workspace(self, batch: int, s: int):
        d, dev = self.dims, self.device
        rows, D, E = batch * s, d.d_model, d.expansion_ratio * d.d_model
        f32, bf = dict(dtype=torch.float32, device=dev), dict(dtype=torch.bfloat16, device=dev)
        ws = {"h": torch.empty((rows, D), **f32), "qkv": torch.empty((rows, 3 * D), **f32), "up": torch.empty((rows, E), **f32),
              "x16": torch.empty((rows, D), **bf), "q": torch.empty((batch, d.n_heads, s, 128), **bf),
              "att": torch.empty((rows, D), **bf), "act": torch.empty((rows, E), **bf)}
        for name in ("x16", "q", "att", "act"):
            ws[name + "_lo"] = torch.empty_like(ws[name]) if self.split else None
        return ws

    def reset(self, batch: int) -> None:
        d = self.dims
        if self.k_cache is None or self.k_cache.shape[1] != batch:
            ks = (d.n_layers, batch, d.n_heads, self.smax, 128)
            vs = (d.n_layers, batch, d.n_heads, 128, self.smax)
            z = lambda shp: torch.zeros(shp, dtype=torch.bfloat16, device=self.device)
            self.k_cache, self.vt_cache = z(ks), z(vs)
            self.k_cache_lo, self.vt_cache_lo = (z(ks), z(vs)) if self.split else (None, None)
        self.cur_len, self.cur_batch = 0, batch
        self._clear_slots()

    # ---- forward -------------------------------------------------------------------------------
    def _blocks_forward(self, ws, B: int, S: int, pos0: int, n_layers: int, slot0: int, variant: int = -1, row_lens=None) -> None:
        """The blocks on ws["h"] (B sequences of S tokens at positions pos0 ..) into KV-cache slots slot0 .. slot0 + B - 1: the uniform
        path (slot0 = 0, B = the whole cache) and the prefill of a run of ragged slots.  variant: the tile variant of the four
        products (-1: the library's choice); row_lens: the valid length of each right-padded row (slot prefill: :meth:`_attn_rows`)."""
        d = self.dims
        if slot0 < 0 or slot0 + B > self.k_cache.shape[1]:
            raise ValueError(f"KV-cache slots {slot0} .. {slot0 + B - 1} outside the {self.k_cache.shape[1]} allocated")
        h, D, E, nh = ws["h"], d.d_model, d.expansion_ratio * d.d_model, d.n_heads
        sp = self.split
        for i in range(n_layers):
            Bk = self.blocks[i]
            kc, vc = self.k_cache[i][slot0:slot0 + B], self.vt_cache[i][slot0:slot0 + B]
            kcl, vcl = (self.k_cache_lo[i][slot0:slot0 + B], self.vt_cache_lo[i][slot0:slot0 + B]) if sp else (None, None)
            ops.layernorm_bf16(h, Bk.n1w, Bk.n1b, d.ln_eps, ws["x16"], ws["x16_lo"])
            ops.gemm16(ws["x16"], ws["x16_lo"], Bk.wqkv, Bk.bqkv, 3 * D, ops.EPI_F32, c=ws["qkv"], variant=variant)
            if d.clip_qkv:
                ops.clamp_f32_(ws["qkv"], d.clip_qkv)
            if d.qk_ln:
                ops.layernorm_f32_(ws["qkv"][:, :D], Bk.qlw, Bk.qlb, d.ln_eps)
                ops.layernorm_f32_(ws["qkv"][:, D: 2 * D], Bk.klw, Bk.klb, d.ln_eps)
            if row_lens is not None:
                self._attn_rows(ws, S, pos0, row_lens, kc, vc, kcl, vcl)
            elif S == 1 and self.fuse_decode_rope:
                ops.attn_decode_rope(ws["qkv"], B, nh, 128, pos0, self.cos, self.sin, kc, vc, ws["att"], kcl, vcl, ws["att_lo"],
                                     alibi_slopes=self.slopes)
            else:
                ops.rope_split_heads(ws["qkv"], B, S, nh, 128, pos0, self.cos, self.sin, ws["q"], kc, vc, ws["q_lo"], kcl, vcl)
            if row_lens is not None or (S == 1 and self.fuse_decode_rope):
                pass
            elif S == 1:
                ops.attn_decode(ws["q"], kc, vc, B, nh, 128, pos0 + 1, ws["att"], ws["q_lo"], kcl, vcl, ws["att_lo"], alibi_slopes=self.slopes)
            else:
                ops.attn_prefill(ws["q"], kc, vc, B, S, nh, 128, pos0, ws["att"], ws["q_lo"], kcl, vcl, ws["att_lo"], alibi_slopes=self.slopes)
            ops.gemm16(ws["att"], ws["att_lo"], Bk.wo, Bk.bo, D, ops.EPI_RESID, c=h, resid=h, variant=variant)
            ops.layernorm_bf16(h, Bk.n2w, Bk.n2b, d.ln_eps, ws["x16"], ws["x16_lo"])
            ops.gemm16(ws["x16"], ws["x16_lo"], Bk.wup, Bk.bup, E, ops.EPI_F32, c=ws["up"], variant=variant)
            ops.gelu_split_bf16(ws["up"], ws["act"], ws["act_lo"])
            ops.gemm16(ws["act"], ws["act_lo"], Bk.wdown, Bk.bdown, D, ops.EPI_RESID, c=h, resid=h, variant=variant)

    def _attn_rows(self, ws, S: int, pos0: int, row_lens, kc, vc, kcl, vcl) -> None:
        """Head split, cache append and causal attention of a right-padded batch, one row at a time over its own length.  The ALiBi
        bias of the prefill kernel is slope * (key - (keys of the LAUNCH - 1)): equal to the per-query form only up to a constant per
        query, which the softmax cancels in exact arithmetic but not in its roundings -- so a row attended inside a batch padded to
        another row's length would not be bit-equal to the same row alone.  Launched per row (batch 1, s = its length) it is the same
        launch whatever run the row rides in; pad positions are neither appended to the caches nor attended."""
        nh = self.dims.n_heads
        for b, n in enumerate(row_lens):
            q = ws["q"].view(-1)[: nh * n * 128].view(1, nh, n, 128)
            ql = ws["q_lo"].view(-1)[: nh * n * 128].view(1, nh, n, 128) if self.split else None
            lo = (lambda t: t[b:b + 1]) if self.split else (lambda t: None)
            rows = slice(b * S, b * S + n)
            ops.rope_split_heads(ws["qkv"][rows], 1, n, nh, 128, pos0, self.cos, self.sin, q, kc[b:b + 1], vc[b:b + 1], ql, lo(kcl), lo(vcl))
            ops.attn_prefill(q, kc[b:b + 1], vc[b:b + 1], 1, n, nh, 128, pos0, ws["att"][rows], ql, lo(kcl), lo(vcl),
                             ws["att_lo"][rows] if self.split else None, alibi_slopes=self.slopes)

    def forward_tokens(self, input_ids: torch.Tensor, audio_segments: Sequence[Tuple[int, int, torch.Tensor]] = (), pos0: int = 0,
                       last_only: bool = False, return_hidden: bool = False, num_layers: Optional[int] = None) -> torch.Tensor:
        """input_ids (B,S) int64 on device; audio_segments as in HipLlamaEngine.forward_tokens (projected frames overwrite
        rows start+1 .. start+F).  Returns fp32 logits (B,S,V) (or (B,1,V) if last_only).  KV positions pos0..pos0+S-1 written."""
        d = self.dims
        assert self.wte is not None and all(b is not None for b in self.blocks), "weights not loaded"
        B, S = input_ids.shape
        if pos0 == 0:
            self.reset(B)
        assert B == self.cur_batch and pos0 == self.cur_len, "KV cache is out of sync with the requested positions"
        if pos0 + S > min(self.smax, d.max_seq_len):
            raise ValueError(f"Cannot forward input with past sequence length {pos0} and current sequence length {S}: "
                             f"this engine holds {min(self.smax, d.max_seq_len)} positions")
        ws = self._workspace(B, S)
        h, D, E, nh = ws["h"], d.d_model, d.expansion_ratio * d.d_model, d.n_heads
        sp = self.split
        embed_splice(input_ids, self.wte, h, audio_segments, self.proj_w, self.proj_b, sp)
        self._blocks_forward(ws, B, S, pos0, d.n_layers if num_layers is None else num_layers, 0)
        self.cur_len = pos0 + S
        if return_hidden:
            return h.view(B, S, D)
        if last_only and S > 1:
            hl = h.view(B, S, D)[:, -1].contiguous()
            x16 = torch.empty((B, D), dtype=torch.bfloat16, device=self.device)
            x16_lo = torch.empty_like(x16) if sp else None
            ops.layernorm_bf16(hl, self.normf_w, self.normf_b, d.ln_eps, x16, x16_lo)
            rows = B
        else:
            x16, x16_lo = ws["x16"], ws["x16_lo"]
            ops.layernorm_bf16(h, self.normf_w, self.normf_b, d.ln_eps, x16, x16_lo)
            rows = B * S
        logits = torch.empty((rows, d.vocab_size), dtype=torch.float32, device=self.device)
        ops.gemm16(x16, x16_lo, self.wte, None, d.vocab_size, ops.EPI_F32, c=logits)
        if d.logit_scale is not None:
            ops.scale_f32_(logits, float(d.logit_scale))
        return logits.view(B, -1, d.vocab_size)

    # ---- ragged mode: batch slots with their own cache lengths ---------------------------------------------------------
    # The surface and semantics of HipLlamaEngine's ragged mode (llark_amd/m2t/engine.py), so that the scheduler and EngineSlots of
    # infer_driver drive either engine: slot b of the KV cache holds one sequence of slot_len[b] tokens (-1 = idle); prefill_slots
    # fills slots at position 0 while the others keep their state, decode_slots runs one token for every slot at its own position,
    # release_slots frees slots for a refill.  There is no shared-prefix form: llark_attn_decode_rope_bf16_shared takes no ALiBi.
    # The bookkeeping is a copy of the Llama engine's without its lineages (whose methods are woven into that engine's fork_slots).
    MAX_SLOTS = 64
    SLOT_PREFILL_VARIANT = 12                                   # 128x256x64 LDS tiles (see _prefill_run)

    def _clear_slots(self) -> None:
        self.n_slots = 0
        self.slot_len = self.slot_state = None                 # device int32 [n_slots]: positions, ops.ROW_* states
        self.slot_len_host: List[int] = []
        self.slot_state_host: List[int] = []
        self.share_prefix = False

    def _limit(self) -> int:
        return min(self.smax, self.dims.max_seq_len)

    def init_slots(self, n_slots: int, share_prefix: bool = False) -> None:
        """Enter the ragged mode with `n_slots` idle slots (the KV cache is (re)sized to n_slots sequences)."""
        if share_prefix:
            raise NotImplementedError("share_prefix is not available on the MPT engine: the shared-prefix decode attention takes no ALiBi bias")
        top = min(self.max_batch, self.MAX_SLOTS)
        if not 1 <= n_slots <= top:
            raise ValueError(f"n_slots must be in 1 .. {top} (max_batch {self.max_batch}, decode GEMMs m <= {self.MAX_SLOTS}), got {n_slots}")
        try:
            self.reset(n_slots)
        except torch.cuda.OutOfMemoryError as e:
            d = self.dims
            per_slot = d.n_layers * d.d_model * self.smax * 2 * 2 * (2 if self.split else 1)
            raise RuntimeError(f"init_slots({n_slots}): the KV cache does not fit: {per_slot / 2**30:.2f} GiB per slot x {n_slots} slots "
                               f"(max_seq {self.smax}, precision {self.precision!r}); use fewer slots or a smaller max_seq") from e
        self.n_slots = n_slots
        self.slot_len = torch.full((n_slots,), -1, dtype=torch.int32, device=self.device)
        self.slot_state = torch.full((n_slots,), ops.ROW_IDLE, dtype=torch.int32, device=self.device)
        self.slot_len_host, self.slot_state_host = [-1] * n_slots, [ops.ROW_IDLE] * n_slots
        self._slot_workspace()                                  # a decode shape that gemm16_mid refuses is reported here

    def _check_slots(self, slots: Sequence[int]) -> List[int]:
        if self.n_slots == 0:
            raise RuntimeError("ragged mode is not active: call init_slots(n) first")
        slots = [int(b) for b in slots]
        if len(set(slots)) != len(slots) or any(not 0 <= b < self.n_slots for b in slots):
            raise ValueError(f"slots must be distinct and in 0 .. {self.n_slots - 1}, got {slots}")
        return slots

    def _set_slots(self, slots: List[int], lens: List[int], state: int) -> None:
        idx = torch.tensor(slots, dtype=torch.long, device=self.device)
        self.slot_len[idx] = torch.tensor(lens, dtype=torch.int32, device=self.device)
        self.slot_state[idx] = state
        for b, n in zip(slots, lens):
            self.slot_len_host[b], self.slot_state_host[b] = n, state

    def release_slots(self, slots: Sequence[int]) -> None:
        """Mark slots idle: the decode step leaves their caches alone and they emit the pad token."""
        slots = self._check_slots(slots)
        if slots:
            self._set_slots(slots, [-1] * len(slots), ops.ROW_IDLE)

    def prefill_slots(self, rows: Sequence[torch.Tensor], audio_segments: Sequence[Tuple[int, int, torch.Tensor]] = (),
                      slots: Optional[Sequence[int]] = None) -> torch.Tensor:
        """Prefill new sequences into the given slots at position 0; the other slots keep their caches and positions.
        rows: 1-D int64 token tensors (one per new sequence); audio_segments: (index into rows, position of <audio_start>, frames
        fp32 (F, mm)) as in forward_tokens; slots: the slot of each row (default 0 .. len(rows) - 1).  A run of contiguous slots is
        prefilled as ONE right-padded batch: every product and row-wise kernel runs on the whole batch, the attention per row over its
        own length (:meth:`_attn_rows`), so that a row's result does not depend on the run it rides in, bit for bit; pad positions
        write nothing to the caches.
        Returns fp32 logits [len(rows), V] of each row's LAST valid token; sets slot_len = row length, state active."""
        d = self.dims
        assert self.wte is not None and all(b is not None for b in self.blocks), "weights not loaded"
        slots = self._check_slots(range(len(rows)) if slots is None else slots)
        if len(slots) != len(rows):
            raise ValueError(f"{len(rows)} rows for {len(slots)} slots")
        rows = [r.reshape(-1).to(device=self.device, dtype=torch.int64) for r in rows]
        lens = [int(r.numel()) for r in rows]
        if any(n < 1 or n > self._limit() for n in lens):
            raise ValueError(f"row lengths {lens} must be in 1 .. max_seq {self._limit()}")
        logits = torch.empty((len(rows), d.vocab_size), dtype=torch.float32, device=self.device)
        order = sorted(range(len(rows)), key=lambda r: slots[r])
        runs: List[List[int]] = []
        for r in order:
            if runs and slots[r] == slots[runs[-1][-1]] + 1:
                runs[-1].append(r)
            else:
                runs.append([r])
        for run in runs:
            nb, S = len(run), max(lens[r] for r in run)
            ids = torch.zeros((nb, S), dtype=torch.int64, device=self.device)
            for i, r in enumerate(run):
                ids[i, : lens[r]] = rows[r]
            segs = [(i, start, frames) for i, r in enumerate(run) for (rr, start, frames) in audio_segments if rr == r]
            last = torch.tensor([i * S + lens[r] - 1 for i, r in enumerate(run)], dtype=torch.long, device=self.device)
            logits[torch.tensor(run, dtype=torch.long, device=self.device)] = self._prefill_run(ids, segs, slots[run[0]], last, [lens[r] for r in run])
        self._set_slots(slots, lens, ops.ROW_ACTIVE)
        return logits

    def _prefill_run(self, ids: torch.Tensor, segs, slot0: int, last: torch.Tensor, row_lens: List[int]) -> torch.Tensor:
        """A right-padded batch (valid lengths row_lens) through the blocks into cache slots slot0 .. at position 0; logits of the rows of
        h listed in `last`."""
        d = self.dims
        B, S = ids.shape
        ws = self._workspace(B, S)
        embed_splice(ids, self.wte, ws["h"], segs, self.proj_w, self.proj_b, self.split)
        # A row's result must not depend on the batch it rides in (a refill pads a run of slots to its longest prompt): the LDS-tile
        # kernels of gemm16 accumulate every output element in the same K order whatever the row count and tile shape, while the library's
        # own choice moves between the m <= 16 weight-streaming kernels, the tiles and the fragment-major kernels with their K cut as
        # the row count changes.  So the products of a slot prefill name their tile variant: 128x128x32 up to 128 rows, 128x256x64 above.
        ws["att"].zero_()                                         # pad rows of the attention output are never written (_attn_rows)
        if self.split:
            ws["att_lo"].zero_()
        self._blocks_forward(ws, B, S, 0, d.n_layers, slot0, variant=self.SLOT_PREFILL_VARIANT, row_lens=row_lens)
        hl = ws["h"].index_select(0, last)
        x16 = torch.empty((hl.shape[0], d.d_model), dtype=torch.bfloat16, device=self.device)
        x16_lo = torch.empty_like(x16) if self.split else None
        ops.layernorm_bf16(hl, self.normf_w, self.normf_b, d.ln_eps, x16, x16_lo)
        logits = torch.empty((hl.shape[0], d.vocab_size), dtype=torch.float32, device=self.device)
        ops.gemm16(x16, x16_lo, self.wte, None, d.vocab_size, ops.EPI_F32, c=logits, variant=self.SLOT_PREFILL_VARIANT)
        if d.logit_scale is not None:
            ops.scale_f32_(logits, float(d.logit_scale))
        return logits

    def _slot_workspace(self):
        """The decode step's own buffers: a refill prefill (other shapes) does not reallocate them."""
        n = self.n_slots
        if self._slot_ws is None or self._slot_ws["h"].shape[0] != n:
            d = self.dims
            D, E = d.d_model, d.expansion_ratio * d.d_model
            ws = self._alloc_workspace(n, 1)
            ws["logits"] = torch.empty((n, d.vocab_size), dtype=torch.float32, device=self.device)
            ws["next"] = torch.zeros((n,), dtype=torch.int64, device=self.device)
            ws["mid"] = None
            if 16 < n <= self.MAX_SLOTS:                       # scratch of ops.gemm16_mid: the largest of the step's five products
                need = [ops.gemm16_mid_scratch_bytes(n, nn, kp, self.split, epi) for nn, kp, epi in (
                    (3 * D, D, ops.EPI_F32), (D, D, ops.EPI_RESID), (E, D, ops.EPI_F32), (D, E, ops.EPI_RESID), (d.vocab_size, D, ops.EPI_F32))]
                if min(need) == 0:
                    raise ops._lib.LlarkHipError(f"gemm16_mid does not take this model's decode shapes (d_model {D}, ffn {E}, vocab "
                                                 f"{d.vocab_size}, {n} slots)")
                ws["mid"] = torch.empty((max(need) // 4,), dtype=torch.float32, device=self.device)
            self._slot_ws = ws
        return self._slot_ws

    def advance_slots(self, logits: torch.Tensor, eos: int = -1, pad: int = 0, out_col: Optional[torch.Tensor] = None,
                      choice: Optional[torch.Tensor] = None, advance: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
        """Token choice of every active slot from fp32 logits [n_slots, V] (greedy, or `choice` [n_slots] int64), EOS -> finished,
        pad for idle / finished slots, positions + 1 for active slots when `advance` (ops.decode_advance_rows, one launch).
        Returns (next ids on the device [n_slots] int64, their host copy -- the step's one device-to-host transfer)."""
        ws = self._slot_workspace()
        was_active = [st == ops.ROW_ACTIVE for st in self.slot_state_host]
        ops.decode_advance_rows(logits, self.slot_state, ws["next"], self.slot_len if advance else None, out_col, eos, pad,
                                choice=None if choice is None else choice.reshape(-1).to(torch.int64).contiguous())
        host = ws["next"].cpu()
        for b, act in enumerate(was_active):
            if act:
                if advance:
                    self.slot_len_host[b] += 1
                if eos >= 0 and int(host[b]) == eos:
                    self.slot_state_host[b] = ops.ROW_FINISHED
        return ws["next"], host

    def _gemm_slots(self, ws, a, a_lo, wt, bias, n: int, epilogue: int, **out) -> None:
        """A decode-step product: ops.gemm16 up to 16 slots, ops.gemm16_mid (the weights streamed once for 17 .. 64 rows) above."""
        if ws["mid"] is not None:
            ops.gemm16_mid(a, a_lo, wt, bias, n, epilogue, ws["mid"], **out)
        else:
            ops.gemm16(a, a_lo, wt, bias, n, epilogue, **out)

    def decode_slots(self, ids: torch.Tensor, eos: int = -1, pad: int = 0, out_col: Optional[torch.Tensor] = None,
                     sample=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """One decode step over all n_slots rows, each at its own position.  Per block: layernorm_bf16 -> qkv product ->
        ops.mpt_attn_decode_rows (clamp, qk_ln, head split, cache append and ALiBi attention over slot_len in one launch; with
        fuse_decode_qk off: clamp_f32_, layernorm_f32_ x 2, attn_decode_rope_rows with the identity tables) -> out_proj + residual ->
        layernorm_bf16 -> up_proj -> gelu_split_bf16 -> down_proj + residual; then norm_f, the tied wte head (x logit_scale) and
        advance_slots.  ids: int64 [n_slots] (the token of each slot at position slot_len; idle rows pass through the row-independent
        GEMMs harmlessly).  sample: optional callable logits -> int64 [n_slots] tokens; greedy otherwise.  Returns (next ids on the
        device, their host copy, the step's fp32 logits [n_slots, V] -- a buffer the next step overwrites)."""
        n, d = self.n_slots, self.dims
        if n == 0:
            raise RuntimeError("ragged mode is not active: call init_slots(n) first")
        full = [b for b in range(n) if self.slot_state_host[b] == ops.ROW_ACTIVE and self.slot_len_host[b] >= self._limit()]
        if full:
            raise ValueError(f"slot(s) {full} reached the engine's max_seq {self._limit()}")
        ids = ids.reshape(-1)
        assert ids.numel() == n and ids.dtype == torch.int64
        ws = self._slot_workspace()
        h, qkv, logits, pos = ws["h"], ws["qkv"], ws["logits"], self.slot_len
        x16, x16l, att, attl, act, actl = ws["x16"], ws["x16_lo"], ws["att"], ws["att_lo"], ws["act"], ws["act_lo"]
        D, E, nh, eps = d.d_model, d.expansion_ratio * d.d_model, d.n_heads, d.ln_eps
        ops.embed_gather(ids.contiguous(), self.wte, h)
        for i, Bk in enumerate(self.blocks):
            kc, vc = self.k_cache[i], self.vt_cache[i]
            kcl, vcl = (self.k_cache_lo[i], self.vt_cache_lo[i]) if self.split else (None, None)
            ops.layernorm_bf16(h, Bk.n1w, Bk.n1b, eps, x16, x16l)
            self._gemm_slots(ws, x16, x16l, Bk.wqkv, Bk.bqkv, 3 * D, ops.EPI_F32, c=qkv)
            with ops._timed("mpt_decode_front", 0.0):           # kernel timing: everything between the qkv product and out_proj, either form
                if self.fuse_decode_qk:
                    ops.mpt_attn_decode_rows(qkv, n, nh, 128, pos, d.clip_qkv, Bk.qlw, Bk.qlb, Bk.klw, Bk.klb, eps, kc, vc, att, kcl, vcl, attl,
                                             alibi_slopes=self.slopes)
                else:
                    if d.clip_qkv:
                        ops.clamp_f32_(qkv, d.clip_qkv)
                    if d.qk_ln:
                        ops.layernorm_f32_(qkv[:, :D], Bk.qlw, Bk.qlb, eps)
                        ops.layernorm_f32_(qkv[:, D: 2 * D], Bk.klw, Bk.klb, eps)
                    ops.attn_decode_rope_rows(qkv, n, nh, 128, pos, self.cos, self.sin, kc, vc, att, kcl, vcl, attl, alibi_slopes=self.slopes)
            self._gemm_slots(ws, att, attl, Bk.wo, Bk.bo, D, ops.EPI_RESID, c=h, resid=h)
            ops.layernorm_bf16(h, Bk.n2w, Bk.n2b, eps, x16, x16l)
            self._gemm_slots(ws, x16, x16l, Bk.wup, Bk.bup, E, ops.EPI_F32, c=ws["up"])
            ops.gelu_split_bf16(ws["up"], act, actl)
            self._gemm_slots(ws, act, actl, Bk.wdown, Bk.bdown, D, ops.EPI_RESID, c=h, resid=h)
        ops.layernorm_bf16(h, self.normf_w, self.normf_b, eps, x16, x16l)
        self._gemm_slots(ws, x16, x16l, self.wte, None, d.vocab_size, ops.EPI_F32, c=logits)
        if d.logit_scale is not None:
            ops.scale_f32_(logits, float(d.logit_scale))
        nxt, host = self.advance_slots(logits, eos, pad, out_col, None if sample is None else sample(logits))
        return nxt, host, logits
