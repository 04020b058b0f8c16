"""Native Llama-2 execution engine on the HIP kernels (weights in kernel layout, KV cache, workspaces).

This is what runs underneath :class:`llark_amd.m2t.llamav2.WrappedLlamav2ForCausalLM`; it replaces
the arithmetic the reference delegates to HF ``LlamaModel.forward`` + ``lm_head`` + ``mm_projector``
(m2t/models/llamav2.py:124,133,224-234,312).

HBM layout:
  embed      bf16 [V][H]                      lm_head  bf16 [V][H]
  per layer  wqkv bf16 [3H][H] (q|k|v rows)   wo bf16 [H][H]
             wgu  bf16 [2I][H]  rows interleaved in blocks of 32: [gate 32 | up 32] (SwiGLU epilogue)
             wdown bf16 [H][I]                norms fp32 [H]
  projector  bf16 [H][mm] + fp32 bias
  h          fp32 [B*S][H] residual stream (updated in place by GEMM epilogues)
  k_cache    bf16 [L][B][nh][Smax][128]       vt_cache bf16 [L][B][nh][128][Smax]  (V transposed)
"""
from __future__ import annotations

from collections import namedtuple
from dataclasses import dataclass
import os
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from .. import ops


@dataclass
class LlamaDims:
    hidden_size: int = 4096
    intermediate_size: int = 11008
    num_hidden_layers: int = 32
    num_attention_heads: int = 32
    vocab_size: int = 32000
    rms_norm_eps: float = 1e-5
    rope_theta: float = 10000.0
    mm_hidden_size: int = 4800
    max_position_embeddings: int = 4096

    @property
    def head_dim(self) -> int:
        return self.hidden_size // self.num_attention_heads


def interleave_gate_up(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    """[I][H] gate, up -> [2I][H] with rows [gate 0..31 | up 0..31 | gate 32..63 | up 32..63 | ...]."""
    I, H = gate.shape
    assert I % 32 == 0, "intermediate_size must be a multiple of 32"
    return torch.stack((gate.view(I // 32, 32, H), up.view(I // 32, 32, H)), dim=1).reshape(2 * I, H).contiguous()


def _uniform_segments(audio_segments, h: torch.Tensor, S: int, hidden: int):
    """(first batch row, start, clips, frames per clip, the (clips * frames, mm) fp32 matrix) when the segments are equal-length views of one
    contiguous fp32 tensor on h's device, in consecutive batch rows, at the same start; else None (embed_splice then loops over them)."""
    if len(audio_segments) < 2:
        return None
    b0, start, f0 = audio_segments[0]
    if f0.dim() != 2 or f0.dtype != torch.float32 or f0.device != h.device or not f0.is_contiguous():
        return None
    F, mm = f0.shape
    if F < 1 or start + 1 + F > S or not ops.gemm16_batched_bias_takes(F, hidden):
        return None
    base = f0.untyped_storage().data_ptr()
    for i, (b, st, f) in enumerate(audio_segments):
        if (b != b0 + i or st != start or f.shape != f0.shape or f.dtype != f0.dtype or f.device != f0.device or not f.is_contiguous()
                or f.untyped_storage().data_ptr() != base or f.storage_offset() != f0.storage_offset() + i * F * mm):
            return None
    nb = len(audio_segments)
    return b0, start, nb, F, f0.as_strided((nb * F, mm), (mm, 1))


def embed_splice(ids: torch.Tensor, table: torch.Tensor, h: torch.Tensor, audio_segments, proj_w, proj_b, split: bool) -> None:
    """h[b * S + t] = table[ids[b, t]], then the projected frames of every (batch index, position of <audio_start>, frames fp32 (F, mm))
    overwrite rows start + 1 .. start + F of their sequence (the splice of m2t/models/llamav2.py:141-222).  Shared with HipMptEngine."""
    S = ids.shape[1]
    ops.embed_gather(ids.reshape(-1).contiguous(), table, h)
    uni = _uniform_segments(audio_segments, h, S, table.shape[1])
    if uni is not None:
        # the clips' frames are one contiguous (nb * F, mm) matrix and the weight is shared: one split and one batched product whose
        # per-clip C stride is a whole sequence of h -- every row bit-equal to the per-segment loop below (same kernel, same m)
        assert proj_w is not None, "mm_projector weights not loaded"
        b0, start, nb, F, flat = uni
        a16, a16_lo = ops.split16(flat, torch.bfloat16, want_lo=split)
        ops.gemm16_batched_bias(a16, a16_lo, F * a16.stride(0), proj_w, proj_b, F, table.shape[1], h[b0 * S + start + 1:], h.stride(0),
                                S * h.stride(0), nb)
        return
    for (b, start, frames) in audio_segments:
        assert proj_w is not None, "mm_projector weights not loaded"
        F = frames.shape[0]
        a16, a16_lo = ops.split16(frames.to(device=h.device, dtype=torch.float32).contiguous(), torch.bfloat16, want_lo=split)
        r0 = b * S + start + 1
        ops.gemm16(a16, a16_lo, proj_w, proj_b, table.shape[1], ops.EPI_F32, c=h[r0: r0 + F])


class _Layer:
    __slots__ = ("wqkv", "wo", "wgu", "wdown", "ln1", "ln2", "wqkv_rope")


# What one prefill launch sequence works on: `nb` batch rows of the workspace (the whole batch, or one half per stream) and the KV-cache
# slot of the first of them.  The *_lo planes are None in the "bf16" flow.
_Rows = namedtuple("_Rows", "nb slot0 h qkv x16 x16_lo q q_lo att att_lo act act_lo")


class HipLlamaEngine:
    """precision: "split" (default) = fp32-class: every Linear input, q/k/v and the attention output are
    carried as bf16 hi+lo planes (16 significant bits) and every GEMM / attention product runs the extra
    MFMA passes -- logits then match the reference's fp32 CPU path (bf16-valued weights) to ~1e-5;
    "bf16" = the reference's GPU dtype flow (single bf16 rounding at those points), ~2x fewer MFMAs."""

    def __init__(self, dims: LlamaDims, device="cuda", max_batch: int = 8, max_seq: int = 512, precision: str = "split", frag_weights: bool = True):
        """frag_weights: keep a fragment-major twin of every Linear weight for the B-direct GEMM (inference; the
        training step updates the row-major weights in place and therefore builds its engine with False)."""
        self.frag_weights = frag_weights
        if precision not in ("split", "bf16"):
            raise ValueError(f"precision must be 'split' or 'bf16', got {precision!r}")
        self.precision = precision
        self.split = precision == "split"
        if dims.head_dim != 128:
            raise NotImplementedError(f"the HIP attention kernels are built for head_dim 128 (Llama-2); got {dims.head_dim}")
        if dims.intermediate_size % 32 or dims.hidden_size % 32 or dims.mm_hidden_size % 32:
            raise NotImplementedError("hidden / intermediate / mm_hidden sizes must be multiples of 32")
        self.dims = dims
        self.device = torch.device(device)
        self.max_batch = max_batch
        self.smax = ops.round_up(max_seq, 8)
        self.layers: List[Optional[_Layer]] = [None] * dims.num_hidden_layers
        self.embed = self.lm_head = self.norm = self.proj_w = self.proj_b = None
        # RoPE tables exactly as HF computes them (fp32, inv_freq = theta^(-2i/d), emb = cat(freqs, freqs))
        hd = dims.head_dim
        inv_freq = 1.0 / (dims.rope_theta ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
        freqs = torch.arange(self.smax, dtype=torch.float32)[:, None] * inv_freq[None, :]
        self.cos = freqs.cos().contiguous().to(self.device)
        self.sin = freqs.sin().contiguous().to(self.device)
        self._ws: Dict[str, torch.Tensor] = {}
        self._ws_key = None
        self.k_cache = self.vt_cache = self.k_cache_lo = self.vt_cache_lo = None
        self.cur_len = 0
        self.cur_batch = 0
        # The knobs of the launch sequences: what each does and its default.  How each was measured and why the opt-ins lost: DESIGN.md 7(g).
        # decode: o_proj / down_proj + the FOLLOWING RMSNorm in one launch ("last workgroup done" tail); bit-identical, slower: default off
        self.fuse_decode_norm = os.environ.get("LLARK_DECODE_FUSE_NORM", "0") == "1"
        # decode: RMSNorm INSIDE the consuming GEMM; bit-identical.  "auto" (default) = where the LDS-DMA streaming Linear takes it (B = 1,
        # weights >= 64 MB: q/k/v, gate/up, lm_head), "1" = every decode shape, "0" = never.  A property: also takes True / False.  The
        # per-k-step form of "1": B = 8 split 5.89 vs 6.04 ms per step, B = 8 bf16 5.26 vs 4.85, B = 1 split 492 vs 480 ms per 64 tokens
        self.fuse_decode_norm_a = os.environ.get("LLARK_DECODE_FUSE_NORM_A", "auto")
        # decode step as ONE hipGraph per batch size, position read from device memory; no gain on ROCm 7.2: default off
        self.decode_graph = os.environ.get("LLARK_DECODE_GRAPH", "0") == "1"
        # decode step as a recorded host launch list over static buffers (ops.LaunchList): removes the per-launch Python cost; default off
        self.decode_replay = os.environ.get("LLARK_DECODE_REPLAY", "0") == "1"
        # decode: RoPE + KV-cache append inside the attention launch (one launch per layer fewer); default on, "0" = two launches
        self.fuse_decode_rope = os.environ.get("LLARK_DECODE_FUSE_ROPE", "1") != "0"
        # batch-1 decode with o_proj on a side stream under the attention and gate/up under o_proj (_decode_layers_chained); default off
        self.decode_chain = os.environ.get("LLARK_DECODE_CHAIN", "0") == "1"
        self._chain = None
        # prefill: RoPE + head split + K / V^T cache writes in the q|k|v GEMM's epilogue.  "auto" (default) = wherever the two-launch path
        # runs the same whole-tile kernel, so results stay BIT-equal; "1" = every prefill of >= 32 positions; "0" = two launches.  Costs a
        # second fragment-major q|k|v weight per layer (3.2 GB at 7B), built lazily (_rope_weight)
        self.fuse_prefill_rope = os.environ.get("LLARK_PREFILL_FUSE_ROPE", "auto")
        if self.fuse_prefill_rope not in ("0", "1", "auto"):
            raise ValueError(f"LLARK_PREFILL_FUSE_ROPE must be 0, 1 or auto, got {self.fuse_prefill_rope!r}")
        # prefill of an even batch as TWO half-batches on two HIP streams (_prefill_two_streams); default 1 until measured
        self.prefill_streams = int(os.environ.get("LLARK_PREFILL_STREAMS", "1"))
        if self.prefill_streams not in (1, 2):
            raise ValueError(f"LLARK_PREFILL_STREAMS must be 1 or 2, got {self.prefill_streams}")
        self._side_streams = None
        self._resident_wgs = None
        self._rope_rows = None                                      # gather index of the epilogue's q|k|v row order (built on first use)
        self._dec: Dict[int, dict] = {}
        # ragged mode (init_slots / prefill_slots / decode_slots): every batch slot has its own cache length
        self._slot_ws = None
        self._clear_slots()

    # ---- weights -------------------------------------------------------------------------------
    def _bf16(self, t: torch.Tensor) -> torch.Tensor:
        return t.detach().to(device=self.device, dtype=torch.bfloat16).contiguous()

    def _f32(self, t: torch.Tensor) -> torch.Tensor:
        return t.detach().to(device=self.device, dtype=torch.float32).contiguous()

    def set_layer(self, i: int, q, k, v, o, gate, up, down, ln1, ln2) -> None:
        L = _Layer()
        L.wqkv = torch.cat((self._bf16(q), self._bf16(k), self._bf16(v)), dim=0).contiguous()
        L.wo = self._bf16(o)
        L.wgu = interleave_gate_up(self._bf16(gate), self._bf16(up))
        L.wdown = self._bf16(down)
        L.ln1, L.ln2 = self._f32(ln1), self._f32(ln2)
        self._dec.clear()                                     # captured graphs hold the old weight pointers
        old = self.layers[i]
        if old is not None:
            for t in (old.wqkv, old.wo, old.wgu, old.wdown):
                ops.detach_frag(t)
        if self.frag_weights:
            for t in (L.wqkv, L.wo, L.wgu, L.wdown):
                ops.attach_frag(t, t.shape[0])
        L.wqkv_rope = None                                    # built on the first prefill that takes the fused epilogue (_rope_weight)
        self.layers[i] = L

    def _rope_capable(self, L) -> bool:
        # only next to the fragment-major twin the two-launch path uses (LLARK_FRAG=0 switches both off: same kernel family either way)
        return (self.frag_weights and hasattr(L.wqkv, "_llark_frag") and self.fuse_prefill_rope != "0" and self.dims.num_attention_heads % 2 == 0
                and self.dims.hidden_size % 64 == 0)

    def _rope_weight(self, L):
        """The q|k|v weight in the fused epilogue's row order, fragment-major: + 3 H^2 x 2 bytes per layer (3.2 GB at 7B), so it is
        built LAZILY -- engines that only decode, prefill short prompts or train never pay for it."""
        if L.wqkv_rope is None and self._rope_capable(L):
            try:
                if self._rope_rows is None:
                    self._rope_rows = ops.rope_qkv_row_order(self.dims.num_attention_heads, self.dims.head_dim).to(self.device)
                L.wqkv_rope = ops.pack_weight16_frag(L.wqkv.index_select(0, self._rope_rows).contiguous(), L.wqkv.shape[0])
            except torch.cuda.OutOfMemoryError:
                # built inside the first qualifying prefill, i.e. after the KV cache and the activations were allocated: running out of
                # memory here must not fail the forward -- this engine keeps the two-launch path from now on
                self.fuse_prefill_rope = "0"
                for M in self.layers:
                    if M is not None:
                        M.wqkv_rope = None
                torch.cuda.empty_cache()
                return None
        return L.wqkv_rope

    def prepare_prefill(self) -> bool:
        """Build the fused-RoPE q|k|v twins of every layer NOW (+ 3 H^2 x 2 bytes per layer, 3.2 GB at 7B) instead of inside the first
        qualifying prefill: callers that time their first forward, or want an out-of-memory condition at load time rather than in the
        middle of inference, call this after loading the weights.  Returns False when this engine does not take the fused epilogue."""
        return all(L is not None and self._rope_weight(L) is not None for L in self.layers)

    def set_globals(self, embed, norm, lm_head, proj_w=None, proj_b=None) -> None:
        self._dec.clear()
        self.embed, self.norm, self.lm_head = self._bf16(embed), self._f32(norm), self._bf16(lm_head)
        if proj_w is not None:
            self.proj_w, self.proj_b = self._bf16(proj_w), self._f32(proj_b)
        if self.frag_weights:
            ops.attach_frag(self.lm_head, self.lm_head.shape[0])

    def state_dict_hf(self) -> Dict[str, torch.Tensor]:
        """Weights under the reference's state-dict names and layouts (inverse of :meth:`load_state_dict`): the fused
        q|k|v rows are split, gate/up rows de-interleaved.  Tensors are views / copies on the engine's device."""
        d = self.dims
        H, I = d.hidden_size, d.intermediate_size
        sd: Dict[str, torch.Tensor] = {}
        for i, L in enumerate(self.layers):
            p = f"model.layers.{i}"
            sd[f"{p}.self_attn.q_proj.weight"], sd[f"{p}.self_attn.k_proj.weight"], sd[f"{p}.self_attn.v_proj.weight"] = (
                L.wqkv[:H], L.wqkv[H: 2 * H], L.wqkv[2 * H:])
            sd[f"{p}.self_attn.o_proj.weight"] = L.wo
            gu = L.wgu.view(I // 32, 2, 32, H)
            sd[f"{p}.mlp.gate_proj.weight"] = gu[:, 0].reshape(I, H)
            sd[f"{p}.mlp.up_proj.weight"] = gu[:, 1].reshape(I, H)
            sd[f"{p}.mlp.down_proj.weight"] = L.wdown
            sd[f"{p}.input_layernorm.weight"] = L.ln1
            sd[f"{p}.post_attention_layernorm.weight"] = L.ln2
        sd["model.embed_tokens.weight"], sd["model.norm.weight"], sd["lm_head.weight"] = self.embed, self.norm, self.lm_head
        if self.proj_w is not None:
            sd["model.mm_projector.weight"], sd["model.mm_projector.bias"] = self.proj_w, self.proj_b
        return sd

    def drop_frag_weights(self) -> None:
        """Called by the training step: the row-major weights are about to be updated in place."""
        self.frag_weights = False
        for L in self.layers:
            if L is not None:
                for t in (L.wqkv, L.wo, L.wgu, L.wdown):
                    ops.detach_frag(t)
                L.wqkv_rope = None
        if self.lm_head is not None:
            ops.detach_frag(self.lm_head)

    def weights_changed_in_place(self) -> None:
        """The weights were overwritten in place (checkpoint.copy_weights_into_engine): every fragment-major copy attached to a
        layer weight or to lm_head is re-packed into its own buffer, so the captured decode steps in ``_dec`` stay valid (every
        buffer they read keeps its address) and are kept; the fused-RoPE q|k|v twins are dropped and rebuilt by the next prefill
        that takes them.  A trainer's engine (``frag_weights`` False) carries none of these: its trainer refreshes its own."""
        if not self.frag_weights:
            return
        for L in self.layers:
            if L is not None:
                for t in (L.wqkv, L.wo, L.wgu, L.wdown):
                    ops.refresh_frag(t)
                L.wqkv_rope = None
        if self.lm_head is not None:
            ops.refresh_frag(self.lm_head)

    def load_state_dict(self, sd) -> None:
        """HF / reference state-dict names (model.layers.N.self_attn.q_proj.weight, ..., model.mm_projector.*)."""
        d = self.dims
        for i in range(d.num_hidden_layers):
            p = f"model.layers.{i}"
            self.set_layer(i, sd[f"{p}.self_attn.q_proj.weight"], sd[f"{p}.self_attn.k_proj.weight"],
                           sd[f"{p}.self_attn.v_proj.weight"], sd[f"{p}.self_attn.o_proj.weight"],
                           sd[f"{p}.mlp.gate_proj.weight"], sd[f"{p}.mlp.up_proj.weight"], sd[f"{p}.mlp.down_proj.weight"],
                           sd[f"{p}.input_layernorm.weight"], sd[f"{p}.post_attention_layernorm.weight"])
        self.set_globals(sd["model.embed_tokens.weight"], sd["model.norm.weight"], sd["lm_head.weight"],
                         sd.get("model.mm_projector.weight"), sd.get("model.mm_projector.bias"))

    # ---- workspaces ----------------------------------------------------------------------------
    def _workspace(self, batch: int, s: int):
        key = (batch, s)
        if self._ws_key != key:
            self._ws, self._ws_key = self._alloc_workspace(batch, s), key
        return self._ws

    def _alloc_workspace(self, batch: int, s: int):
        d, dev = self.dims, self.device
        rows = batch * s
        H, I = d.hidden_size, d.intermediate_size
        ws = {
            "h": torch.empty((rows, H), dtype=torch.float32, device=dev),
            "x16": torch.empty((rows, H), dtype=torch.bfloat16, device=dev),
            "qkv": torch.empty((rows, 3 * H), dtype=torch.float32, device=dev),
            "q": torch.empty((batch, d.num_attention_heads, s, d.head_dim), dtype=torch.bfloat16, device=dev),
            "att": torch.empty((rows, H), dtype=torch.bfloat16, device=dev),
            "act": torch.empty((rows, I), dtype=torch.bfloat16, device=dev),
        }
        if self.split:
            for name in ("x16", "q", "att", "act"):
                ws[name + "_lo"] = torch.empty_like(ws[name])
        else:
            for name in ("x16", "q", "att", "act"):
                ws[name + "_lo"] = None
        return ws

    def set_precision(self, precision: str) -> None:
        """Switch between the "split" (fp32-class) and "bf16" activation flows.  The weights are the same bf16 values in both;
        activation planes, the KV cache and captured decode graphs are rebuilt on the next call."""
        if precision not in ("split", "bf16"):
            raise ValueError(f"precision must be 'split' or 'bf16', got {precision!r}")
        if precision == self.precision:
            return
        self.precision, self.split = precision, precision == "split"
        self._ws, self._ws_key = None, None
        self._dec.clear()
        self.k_cache = self.vt_cache = self.k_cache_lo = self.vt_cache_lo = None
        self._slot_ws = None
        self._clear_slots()

    def _ensure_cache(self, batch: int):
        d = self.dims
        if self.k_cache is None or self.k_cache.shape[1] < batch:
            self._dec.clear()                                 # captured graphs hold the old cache pointers
            shape_k = (d.num_hidden_layers, batch, d.num_attention_heads, self.smax, d.head_dim)
            shape_v = (d.num_hidden_layers, batch, d.num_attention_heads, d.head_dim, self.smax)
            self.k_cache = torch.zeros(shape_k, dtype=torch.bfloat16, device=self.device)
            self.vt_cache = torch.zeros(shape_v, dtype=torch.bfloat16, device=self.device)
            self.k_cache_lo = torch.zeros(shape_k, dtype=torch.bfloat16, device=self.device) if self.split else None
            self.vt_cache_lo = torch.zeros(shape_v, dtype=torch.bfloat16, device=self.device) if self.split else None

    def _prefill_rope_fused(self, batch: int, s: int) -> bool:
        """Does this prefill take the q|k|v product with RoPE in its epilogue?  "auto" = only where llark_gemm16_fragw would run the
        same whole 128x256 tiles (the library answers: llark_gemm16_fragw_whole_tiles), so results stay bit-equal."""
        if self.fuse_prefill_rope == "0" or s < 32 or batch * s < ops.FRAG_MIN_ROWS:
            return False
        if self.fuse_prefill_rope == "1":
            return True
        H = self.dims.hidden_size
        return ops.gemm16_fragw_whole_tiles(self.split, ops.EPI_F32, batch * s, 3 * H, H)

    # ---- forward: shared pieces ------------------------------------------------------------------
    def _kv_views(self, i: int, c0: int, c1: int):
        """kc, vc, kcl, vcl: the K / V^T cache of layer i for slots c0 .. c1 - 1 (the lo planes are None in the "bf16" flow)."""
        kc, vc = self.k_cache[i, c0:c1], self.vt_cache[i, c0:c1]
        kcl = self.k_cache_lo[i, c0:c1] if self.split else None
        vcl = self.vt_cache_lo[i, c0:c1] if self.split else None
        if not kc.is_contiguous():            # batch smaller than the allocated cache
            raise ops._lib.LlarkHipError("KV cache batch mismatch: call reset(batch) before prefill")
        return kc, vc, kcl, vcl

    def _epi_swiglu(self) -> int:
        return ops.EPI_SWIGLU_SPLIT if self.split else ops.EPI_SWIGLU16

    def _norm_gemm_takes(self, batch: int, n: int) -> bool:
        """Does the decode Linear [batch] x [n][H] run with the preceding RMSNorm inside its launch (fuse_decode_norm_a)?"""
        mode = self.fuse_decode_norm_a
        return mode == "1" or (mode == "auto" and ops.gemv_dma_rmsnorm_takes(batch, n, self.dims.hidden_size))

    def _head(self, ws, logits: torch.Tensor, normed: bool, may_fuse: bool) -> None:
        """Final norm + lm_head on the workspace rows.  normed: ws["x16"] already holds the normalised rows; may_fuse: the norm may
        run inside the streaming GEMM where that takes the shape (the graph / replay step never asks for it)."""
        d, h = self.dims, ws["h"]
        if may_fuse and not normed and self._norm_gemm_takes(h.shape[0], d.vocab_size):
            ops.gemm16_rmsnorm_a(h, self.norm, d.rms_norm_eps, self.lm_head, d.vocab_size, ops.EPI_F32, self.split, c=logits)
            return
        if not normed:
            ops.rmsnorm_bf16(h, self.norm, d.rms_norm_eps, ws["x16"], ws["x16_lo"])
        if self._mid_step(ws, h.shape[0]):
            ops.gemm16_mid(ws["x16"], ws["x16_lo"], self.lm_head, None, d.vocab_size, ops.EPI_F32, ws["mid"], c=logits)
            return
        ops.gemm16(ws["x16"], ws["x16_lo"], self.lm_head, None, d.vocab_size, ops.EPI_F32, c=logits)

    @staticmethod
    def _mid_step(ws, batch: int) -> bool:
        """Is this the ragged decode step with 17 .. 64 slots?  Its workspace (_slot_workspace) then carries the scratch of the mid-M
        weight-streaming GEMM (ops.gemm16_mid); every other workspace has none and keeps the launches it always had."""
        return ws.get("mid") is not None and 16 < batch <= 64

    def _head_rows(self, hl: torch.Tensor) -> torch.Tensor:
        """Final norm + lm_head on gathered rows hl fp32 [n][H] -> fp32 logits [n][V]."""
        d, n = self.dims, hl.shape[0]
        x16 = torch.empty((n, d.hidden_size), dtype=torch.bfloat16, device=self.device)
        x16_lo = torch.empty_like(x16) if self.split else None
        ops.rmsnorm_bf16(hl, self.norm, d.rms_norm_eps, x16, x16_lo)
        logits = torch.empty((n, d.vocab_size), dtype=torch.float32, device=self.device)
        ops.gemm16(x16, x16_lo, self.lm_head, None, d.vocab_size, ops.EPI_F32, c=logits)
        return logits

    def _layers_forward(self, ws, batch: int, s: int, pos0: int, num_layers: Optional[int] = None, pos_dev=None, hidden_sink=None,
                        slot0: int = 0, pos_rows=None) -> bool:
        """Runs the decoder layers on ws["h"]: the decode launch sequence for one token per sequence (s == 1, also at pos0 == 0), the
        prefill one otherwise.  Returns True when ws["x16"] already holds RMSNorm_final(h) (the fused decode path normalises inside
        the producing GEMM), False when the caller still has to apply the final norm.
        slot0: first KV-cache slot of these batch rows (ragged mode); pos_dev: int32 [1] device position of a graph-capturable
        decode step; pos_rows: int32 [batch] device positions of a ragged decode step, one per slot."""
        n_layers = self.dims.num_hidden_layers if num_layers is None else num_layers
        if slot0 < 0 or slot0 + batch > self.k_cache.shape[1]:
            raise ValueError(f"KV-cache slots {slot0} .. {slot0 + batch - 1} outside the {self.k_cache.shape[1]} allocated")
        if s == 1:
            return self._decode_layers(ws, batch, pos0, n_layers, pos_dev, hidden_sink, slot0, pos_rows)
        self._prefill_layers(ws, batch, s, pos0, n_layers, hidden_sink, slot0)
        return False

    # ---- forward: decode ---------------------------------------------------------------------------
    def _decode_layers(self, ws, batch: int, pos0: int, n_layers: int, pos_dev, hidden_sink, slot0: int, pos_rows, block=None) -> bool:
        """The decoder layers of a decode step.  Decided once, here: `fused` (o_proj / down_proj carry the FOLLOWING RMSNorm in their
        launch), `norm_a` (RMSNorm inside the consuming weight-streaming GEMM) and the attention form -- "rows" (ragged: each slot at its
        own position), "rope" (RoPE + cache append inside the attention launch), "dpos" (position in device memory, graph-capturable)
        or "plain" (rope_split_heads + attn_decode).  The ragged step with 17 .. 64 slots (`mid`) runs the unfused sequence on
        ops.gemm16_mid, the weight-streaming GEMM for that row count; every other case keeps ops.gemm16."""
        d = self.dims
        H, I, nh, hd, eps, sp = d.hidden_size, d.intermediate_size, d.num_attention_heads, d.head_dim, d.rms_norm_eps, self.split
        # block: (stride, blk) of a block step (decode_block) -- `batch` rows are n_slots * stride, slot b owns rows b*stride .. at
        # consecutive positions, the caches belong to the n_slots slots; the decisions are those of the plain step at n_slots rows
        n_cache = batch if block is None else batch // block[0]
        fused = batch <= 16 and n_layers > 0 and self.fuse_decode_norm and H <= 8192 and hidden_sink is None
        norm_a = batch <= 16 and not fused and H % 32 == 0 and self._norm_gemm_takes(n_cache, 3 * H)
        if fused:
            ops.rmsnorm_bf16(ws["h"], self.layers[0].ln1, eps, ws["x16"], ws["x16_lo"])
        if (self.decode_chain and batch == 1 and norm_a and self.fuse_decode_rope and pos_dev is None and hidden_sink is None
                and not fused and H <= 4096 and slot0 == 0 and pos_rows is None and not torch.cuda.is_current_stream_capturing()):
            self._decode_layers_chained(ws, pos0, n_layers)
            return False
        attn = "block" if block is not None else "rows" if pos_rows is not None else "rope" if self.fuse_decode_rope else "dpos" if pos_dev is not None else "plain"
        if attn == "rows" and self._groups is not None and pos_rows is self.slot_len and ws.get("attn_shared") is not None:
            attn = "shared"                                   # share_prefix with at least one group: the slots of a clip read their prefix once
        pos = pos_rows if attn in ("rows", "shared", "block") else pos_dev if pos_dev is not None else pos0
        mid = ws["mid"] if pos_rows is not None and self._mid_step(ws, batch) else None      # 17 .. 64 slots: rmsnorm_bf16 + gemm16_mid
        epi_gu, cos, sin = self._epi_swiglu(), self.cos, self.sin
        h, qkv, x16, x16l, q, ql = ws["h"], ws["qkv"], ws["x16"], ws["x16_lo"], ws["q"], ws["q_lo"]
        att, attl, act, actl = ws["att"], ws["att_lo"], ws["act"], ws["act_lo"]
        for i in range(n_layers):
            L = self.layers[i]
            if hidden_sink is not None:                       # HF output_hidden_states: the stream as it ENTERS every layer
                hidden_sink.append(h.view(batch, 1, H).clone())
            kc, vc, kcl, vcl = self._kv_views(i, slot0, slot0 + n_cache)
            if norm_a:
                ops.gemm16_rmsnorm_a(h, L.ln1, eps, L.wqkv, 3 * H, ops.EPI_F32, sp, c=qkv)
            else:
                if not fused:
                    ops.rmsnorm_bf16(h, L.ln1, eps, x16, x16l)
                if mid is not None:
                    ops.gemm16_mid(x16, x16l, L.wqkv, None, 3 * H, ops.EPI_F32, mid, c=qkv)
                else:
                    ops.gemm16(x16, x16l, L.wqkv, None, 3 * H, ops.EPI_F32, c=qkv)
            if attn == "block":
                ops.attn_decode_rope_block(qkv, n_cache, block[0], nh, hd, block[1], pos, cos, sin, kc, vc, att, kcl, vcl, attl)
            elif attn == "rows":
                ops.attn_decode_rope_rows(qkv, batch, nh, hd, pos, cos, sin, kc, vc, att, kcl, vcl, attl)
            elif attn == "shared":
                ops.attn_decode_rope_shared(qkv, batch, nh, hd, pos, cos, sin, kc, vc, att, self._groups, self._slot_shared, ws["attn_shared"],
                                            kcl, vcl, attl)
            elif attn == "rope":
                ops.attn_decode_rope(qkv, batch, nh, hd, pos, cos, sin, kc, vc, att, kcl, vcl, attl)
            elif attn == "dpos":
                ops.rope_split_heads_dpos(qkv, batch, nh, hd, pos, cos, sin, q, kc, vc, ql, kcl, vcl)
                ops.attn_decode_dpos(q, kc, vc, batch, nh, hd, pos, att, ql, kcl, vcl, attl)
            else:
                ops.rope_split_heads(qkv, batch, 1, nh, hd, pos, cos, sin, q, kc, vc, ql, kcl, vcl)
                ops.attn_decode(q, kc, vc, batch, nh, hd, pos + 1, att, ql, kcl, vcl, attl)
            if fused:
                ops.gemm16_resid_rmsnorm(att, attl, L.wo, h, L.ln2, eps, x16, x16l)
                ops.gemm16(x16, x16l, L.wgu, None, 2 * I, epi_gu, out_hi=act, out_lo=actl)
                nxt = self.layers[i + 1].ln1 if i + 1 < n_layers else self.norm
                ops.gemm16_resid_rmsnorm(act, actl, L.wdown, h, nxt, eps, x16, x16l)
                continue
            if mid is not None:
                ops.gemm16_mid(att, attl, L.wo, None, H, ops.EPI_RESID, mid, c=h, resid=h)
                ops.rmsnorm_bf16(h, L.ln2, eps, x16, x16l)
                ops.gemm16_mid(x16, x16l, L.wgu, None, 2 * I, epi_gu, mid, out_hi=act, out_lo=actl)
                ops.gemm16_mid(act, actl, L.wdown, None, H, ops.EPI_RESID, mid, c=h, resid=h)
                continue
            ops.gemm16(att, attl, L.wo, None, H, ops.EPI_RESID, c=h, resid=h)
            if norm_a:
                ops.gemm16_rmsnorm_a(h, L.ln2, eps, L.wgu, 2 * I, epi_gu, sp, out_hi=act, out_lo=actl)
            else:
                ops.rmsnorm_bf16(h, L.ln2, eps, x16, x16l)
                ops.gemm16(x16, x16l, L.wgu, None, 2 * I, epi_gu, out_hi=act, out_lo=actl)
            ops.gemm16(act, actl, L.wdown, None, H, ops.EPI_RESID, c=h, resid=h)
        return fused

    def _decode_layers_chained(self, ws, pos0: int, n_layers: int) -> None:
        """The decoder layers of a batch-1 decode step with two launches per layer overlapping their producers (round 6):

            main stream:  q|k|v (RMSNorm fused) -> attention [signals A_i] ------------> gate/up [fills its ring, waits O_i] -> down_proj
            side stream:            (after q|k|v)  o_proj [fills its ring, waits A_i, signals O_i]

        o_proj's 33.5 MB of weights start streaming into LDS while the attention launch -- a chain of memory latencies on 32 of 256 CUs, no
        weight traffic -- is running, and gate/up's while o_proj streams.  Both chained kernels use a 64 KiB ring so that two workgroups share a
        CU (98 / 144 registers: the only pairs of the layer that fit 4 waves per SIMD: DESIGN.md 7(d)).  Counters are monotonic device words.
        Same kernels, same arithmetic: results equal the unchained path."""
        d = self.dims
        H, I, nh, hd = d.hidden_size, d.intermediate_size, d.num_attention_heads, d.head_dim
        sp, epi_gu = self.split, self._epi_swiglu()
        if self._chain is None or self._chain["layers"] != n_layers:
            self._chain = {"layers": n_layers, "cnt": torch.zeros((2 * n_layers,), dtype=torch.int32, device=self.device), "epoch": 0,
                           "side": torch.cuda.Stream(device=self.device), "ev": torch.cuda.Event(), "blocks_o": ops.gemv16_dma_blocks(ops.EPI_RESID, H)}
        ch = self._chain
        ch["epoch"] += 1
        ep, cnt, side, ev = ch["epoch"], ch["cnt"], ch["side"], ch["ev"]
        main = torch.cuda.current_stream()
        h = ws["h"]
        for i in range(n_layers):
            L = self.layers[i]
            kc, vc, kcl, vcl = self._kv_views(i, 0, 1)
            a_done, o_done = cnt[2 * i: 2 * i + 1], cnt[2 * i + 1: 2 * i + 2]
            ops.gemm16_rmsnorm_a(h, L.ln1, d.rms_norm_eps, L.wqkv, 3 * H, ops.EPI_F32, sp, c=ws["qkv"])
            ev.record(main)
            side.wait_event(ev)                                  # o_proj becomes resident when q|k|v has finished, i.e. while the attention runs
            ops.attn_decode_rope_chain(ws["qkv"], 1, nh, hd, pos0, self.cos, self.sin, kc, vc, ws["att"], kcl, vcl, ws["att_lo"], a_done)
            with torch.cuda.stream(side):
                ops.gemv16_dma_chain(L.wo, H, ops.EPI_RESID, sp, a_hi=ws["att"], a_lo=ws["att_lo"], c=h, resid=h,
                                     wait=a_done, wait_target=ep * nh, signal=o_done)
            ops.gemv16_dma_chain(L.wgu, 2 * I, epi_gu, sp, x=h, norm_w=L.ln2, eps=d.rms_norm_eps,
                                 out_hi=ws["act"], out_lo=ws["act_lo"], wait=o_done, wait_target=ep * ch["blocks_o"])
            ops.gemm16(ws["act"], ws["act_lo"], L.wdown, None, H, ops.EPI_RESID, c=h, resid=h)
        main.wait_stream(side)                                   # (the data dependency is already met through O_i: this is for the allocator's sake)

    def _decode_body(self, st) -> None:
        """One decode step on static buffers: ids -> logits, new K/V written at *pos.  Never takes the norm-fused lm_head."""
        ws = st["ws"]
        ops.embed_gather(st["ids"].view(-1), self.embed, ws["h"])
        normed = self._layers_forward(ws, st["ids"].shape[0], 1, 0, None, pos_dev=st["pos"])
        self._head(ws, st["logits"], normed, may_fuse=False)

    # ---- forward: prefill --------------------------------------------------------------------------
    def _rows(self, ws, b0: int, b1: int, s: int, slot0: int):
        """Batch rows b0 .. b1 - 1 of the workspace (a full-range slice is the tensor itself to the kernels: same pointer, same shape);
        their KV-cache slots start at slot0 + b0."""
        r, b = slice(b0 * s, b1 * s), slice(b0, b1)

        def cut(name, sl):
            return ws[name][sl] if ws[name] is not None else None

        return _Rows(b1 - b0, slot0 + b0, ws["h"][r], ws["qkv"][r], ws["x16"][r], cut("x16_lo", r), ws["q"][b], cut("q_lo", b),
                     ws["att"][r], cut("att_lo", r), ws["act"][r], cut("act_lo", r))

    def _prefill_layer(self, i: int, v, s: int, pos0: int, rope_fused: bool) -> None:
        """Decoder layer i of a prefill on the rows `v`.  rope_fused: RoPE / head split / cache writes in the q|k|v GEMM's epilogue (no
        fp32 qkv tensor), else the q|k|v GEMM and rope_split_heads as two launches."""
        d, L = self.dims, self.layers[i]
        H, I, nh, hd, eps = d.hidden_size, d.intermediate_size, d.num_attention_heads, d.head_dim, d.rms_norm_eps
        kc, vc, kcl, vcl = self._kv_views(i, v.slot0, v.slot0 + v.nb)
        ops.rmsnorm_bf16(v.h, L.ln1, eps, v.x16, v.x16_lo)
        if rope_fused:
            ops.gemm16_fragw_rope_qkv(v.x16, v.x16_lo, L.wqkv_rope, H, v.nb, s, nh, pos0, self.cos, self.sin, v.q, kc, vc, v.q_lo, kcl, vcl)
        else:
            ops.gemm16(v.x16, v.x16_lo, L.wqkv, None, 3 * H, ops.EPI_F32, c=v.qkv)
            ops.rope_split_heads(v.qkv, v.nb, s, nh, hd, pos0, self.cos, self.sin, v.q, kc, vc, v.q_lo, kcl, vcl)
        ops.attn_prefill(v.q, kc, vc, v.nb, s, nh, hd, pos0, v.att, v.q_lo, kcl, vcl, v.att_lo)
        ops.gemm16(v.att, v.att_lo, L.wo, None, H, ops.EPI_RESID, c=v.h, resid=v.h)
        ops.rmsnorm_bf16(v.h, L.ln2, eps, v.x16, v.x16_lo)
        ops.gemm16(v.x16, v.x16_lo, L.wgu, None, 2 * I, self._epi_swiglu(), out_hi=v.act, out_lo=v.act_lo)
        ops.gemm16(v.act, v.act_lo, L.wdown, None, H, ops.EPI_RESID, c=v.h, resid=v.h)

    def _prefill_layers(self, ws, batch: int, s: int, pos0: int, n_layers: int, hidden_sink, slot0: int) -> None:
        """The decoder layers of a prefill (s > 1): one stream over the whole batch, or two half-batches on two streams."""
        rope_fused = self._prefill_rope_fused(batch, s)
        if rope_fused:
            rope_fused = all(self._rope_weight(self.layers[i]) is not None for i in range(n_layers))
        if (self.prefill_streams == 2 and rope_fused and batch >= 2 and batch % 2 == 0 and self._prefill_rope_fused(batch // 2, s)
                and hidden_sink is None and not torch.cuda.is_current_stream_capturing()):
            self._prefill_two_streams(ws, batch, s, pos0, n_layers, slot0)
            return
        v = self._rows(ws, 0, batch, s, slot0)
        for i in range(n_layers):
            if hidden_sink is not None:                       # HF output_hidden_states: the stream as it ENTERS every layer
                hidden_sink.append(v.h.view(batch, s, self.dims.hidden_size).clone())
            self._prefill_layer(i, v, s, pos0, rope_fused)

    def _prefill_two_streams(self, ws, batch: int, s: int, pos0: int, n_layers: int, slot0: int = 0) -> None:
        """The layer stack of a fused-RoPE prefill as two half-batches, each on its own stream, enqueued layer by layer in alternation.
        The side streams work on row slices of `ws`, tensors allocated on the CALLER's stream: safe only because the workspace is
        persistent (owned by the engine, never returned to the caching allocator while a forward is in flight) and both side streams
        are joined into the caller's stream before this returns."""
        if self._side_streams is None:
            self._side_streams = (torch.cuda.Stream(device=self.device), torch.cuda.Stream(device=self.device))
        cur = torch.cuda.current_stream()
        half = batch // 2
        parts = (self._rows(ws, 0, half, s, slot0), self._rows(ws, half, batch, s, slot0))
        for st in self._side_streams:
            st.wait_stream(cur)
        for i in range(n_layers):
            for st, v in zip(self._side_streams, parts):
                with torch.cuda.stream(st):
                    self._prefill_layer(i, v, s, pos0, True)
        for st in self._side_streams:
            cur.wait_stream(st)

    def _decode_step_graph(self, input_ids: torch.Tensor, pos0: int) -> torch.Tensor:
        """Greedy-decode step as ONE hipGraph replay (opt-in: `decode_graph` / LLARK_DECODE_GRAPH=1).  Bit-identical
        to the eager launches; measured on MI355X / ROCm 7.2 it does NOT shorten the step (7.41 vs 7.52 ms, B=8): the
        ~260 kernels of a step each keep their ~10 us dispatch + drain boundary inside the graph, so the lever for
        decode is fewer kernels (fusion), not graph replay.  First call per batch size runs eagerly on the static
        buffers (first-launch attribute calls happen outside capture), the second captures, later ones replay."""
        d = self.dims
        B = input_ids.shape[0]
        st = self._dec.get(B)
        if st is None:
            ws = dict(self._workspace(B, 1))                  # private copies: the graph owns these buffers
            ws = {k: (torch.empty_like(v) if v is not None else None) for k, v in ws.items()}
            st = {"ids": torch.zeros((B, 1), dtype=torch.int64, device=self.device),
                  "pos": torch.zeros((1,), dtype=torch.int32, device=self.device),
                  "logits": torch.empty((B, d.vocab_size), dtype=torch.float32, device=self.device),
                  "ws": ws, "graph": None, "calls": 0}
            self._dec[B] = st
        st["ids"].copy_(input_ids)
        st["pos"].fill_(pos0)
        if self.decode_replay and not self.decode_graph:
            if st.get("list") is None:
                with ops.LaunchList.record() as ll:
                    self._decode_body(st)
                st["list"] = ll
            else:
                st["list"].replay()
        elif st["graph"] is not None:
            st["graph"].replay()
        elif st["calls"] == 0:
            self._decode_body(st)
        else:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._decode_body(st)
            st["graph"] = g
            g.replay()
        st["calls"] += 1
        self.cur_len = pos0 + 1
        return st["logits"].clone().view(B, 1, d.vocab_size)

    @property
    def fuse_decode_norm_a(self) -> str:
        """"auto" | "1" | "0" (see __init__); assigning a bool means "1" / "0" (it was a bool before round 3)."""
        return self._fuse_decode_norm_a

    @fuse_decode_norm_a.setter
    def fuse_decode_norm_a(self, v) -> None:
        if isinstance(v, bool):
            v = "1" if v else "0"
        v = str(v).strip().lower()
        if v not in ("auto", "1", "0"):
            raise ValueError(f"fuse_decode_norm_a must be 'auto', '1', '0' or a bool, got {v!r}")
        self._fuse_decode_norm_a = v

    def reset(self, batch: int) -> None:
        if self.k_cache is not None and self.k_cache.shape[1] != batch:
            self.k_cache = self.vt_cache = self.k_cache_lo = self.vt_cache_lo = None
        self._ensure_cache(batch)
        self.cur_len, self.cur_batch = 0, batch
        self._clear_slots()

    def forward_tokens(self, input_ids: torch.Tensor, audio_segments: Sequence[Tuple[int, int, torch.Tensor]] = (),
                       pos0: int = 0, last_only: bool = False, num_layers: Optional[int] = None,
                       return_hidden: bool = False, hidden_sink: Optional[list] = None) -> torch.Tensor:
        """input_ids (B,S) int64 on device.  audio_segments: (batch index, position of <audio_start>,
        frames fp32 (F, mm) on device): projected frames overwrite rows start+1 .. start+F of the
        embedded sequence (the splice of m2t/models/llamav2.py:141-222).  Returns fp32 logits
        (B,S,V) (or (B,1,V) if last_only).  Positions pos0..pos0+S-1 of the KV cache are written."""
        d = self.dims
        assert self.embed is not None and all(L is not None for L in self.layers[: (num_layers or d.num_hidden_layers)]), \
            "weights not loaded"
        B, S = input_ids.shape
        if pos0 == 0:
            self.reset(B)
        assert B == self.cur_batch and pos0 == self.cur_len, "KV cache is out of sync with the requested positions"
        if pos0 + S > self.smax:
            raise ValueError(f"sequence of {pos0 + S} exceeds the engine's max_seq {self.smax}")
        if (S == 1 and pos0 > 0 and (self.decode_graph or self.decode_replay) and not audio_segments and num_layers is None
                and not return_hidden and hidden_sink is None and (self.decode_replay or not ops.kernel_timing_active())):
            return self._decode_step_graph(input_ids, pos0)
        ws = self._workspace(B, S)
        h = ws["h"]
        embed_splice(input_ids, self.embed, h, audio_segments, self.proj_w, self.proj_b, self.split)
        normed = self._layers_forward(ws, B, S, pos0, num_layers, hidden_sink=hidden_sink)
        self.cur_len = pos0 + S
        if hidden_sink is not None:
            # HF appends model.norm(h) last (LlamaModel.forward): here the kernel's output planes, hi (+ lo) -- 16 significant bits in the
            # "split" flow, the bf16 value in the "bf16" flow
            ops.rmsnorm_bf16(h, self.norm, d.rms_norm_eps, ws["x16"], ws["x16_lo"])
            nh_ = ws["x16"].float() + (ws["x16_lo"].float() if ws["x16_lo"] is not None else 0.0)
            hidden_sink.append(nh_.view(B, S, d.hidden_size))
            normed = True
        if return_hidden:
            return h.view(B, S, d.hidden_size)
        if last_only and S > 1:
            return self._head_rows(h.view(B, S, d.hidden_size)[:, -1].contiguous()).view(B, 1, d.vocab_size)
        logits = torch.empty((B * S, d.vocab_size), dtype=torch.float32, device=self.device)
        self._head(ws, logits, normed, may_fuse=S == 1 and B <= 16)
        return logits.view(B, S, d.vocab_size)

    # ---- ragged mode: batch slots with their own cache lengths ---------------------------------------------------------
    # Next to the uniform forward_tokens / cur_len mode (which it leaves untouched): slot b of the KV cache holds one sequence of
    # slot_len[b] tokens (-1 = idle).  prefill_slots fills slots with new prompts at position 0 while the other slots keep their
    # state, decode_slots runs one token for every slot at its own position, release_slots frees slots for a refill.  Up to 16
    # slots the decode GEMMs are the m <= 16 forms (skinny / streaming kernels, RMSNorm fused where they take it); 17 .. 64 slots run
    # rmsnorm_bf16 + ops.gemm16_mid (csrc/gemm_mid.hip: the same weights streamed once, activations shared through LDS, K split over
    # workgroups with its partial sums in the slot workspace).  Both are row-independent: a slot's logits do not depend on its
    # neighbours or on the slot count within one of the two ranges.  64 rows is what gemm16_mid takes, hence at most 64 slots.
    MAX_SLOTS = 64

    def _clear_slots(self) -> None:
        self.n_slots = 0
        self._block_ws = None                                   # init_block_decode: the block step's workspace, per slot count
        self.slot_len = self.slot_state = None                 # device int32 [n_slots]: positions, ops.ROW_* states
        self.slot_len_host: List[int] = []
        self.slot_state_host: List[int] = []
        # shared prefixes (fork_slots): lineage id of a slot (None: none), its leading positions bit-identical to the lineage's root,
        # forked slots that still wait for their suffix (slot -> n), and the group table of the decode step (share_prefix only)
        self.share_prefix = False
        self.slot_lineage: List[Optional[int]] = []
        self.slot_shared_host: List[int] = []
        self._forked: Dict[int, int] = {}
        self._lineages = 0
        self.group_list: List[Tuple[int, int, List[int]]] = []       # (source slot, shared length, member slots) as uploaded
        self._groups = self._slot_shared = None                      # device int32 [n_groups][ops.SHARED_GROUP_STRIDE], [n_slots]

    def init_slots(self, n_slots: int, share_prefix: bool = False) -> None:
        """Enter the ragged mode with `n_slots` idle slots (the KV cache is (re)sized to n_slots sequences).  share_prefix: the decode
        step reads the positions that the active slots of one lineage (fork_slots) have in common once per group
        (ops.attn_decode_rope_shared) instead of once per slot; off, every launch is the one it always was."""
        top = min(self.max_batch, self.MAX_SLOTS)
        if not 1 <= n_slots <= top:
            raise ValueError(f"n_slots must be in 1 .. {top} (max_batch {self.max_batch}, decode GEMMs m <= {self.MAX_SLOTS}), got {n_slots}")
        try:
            self.reset(n_slots)
        except torch.cuda.OutOfMemoryError as e:
            d = self.dims
            per_slot = d.num_hidden_layers * d.hidden_size * self.smax * 2 * 2 * (2 if self.split else 1)
            raise RuntimeError(f"init_slots({n_slots}): the KV cache does not fit: {per_slot / 2**30:.2f} GiB per slot x {n_slots} slots "
                               f"(max_seq {self.smax}, precision {self.precision!r}); use fewer slots or a smaller max_seq") from e
        self.n_slots, self._block_ws = n_slots, None
        self.slot_len = torch.full((n_slots,), -1, dtype=torch.int32, device=self.device)
        self.slot_state = torch.full((n_slots,), ops.ROW_IDLE, dtype=torch.int32, device=self.device)
        self.slot_len_host, self.slot_state_host = [-1] * n_slots, [ops.ROW_IDLE] * n_slots
        self.share_prefix = bool(share_prefix)
        self.slot_lineage, self.slot_shared_host = [None] * n_slots, [0] * n_slots
        if self.share_prefix:
            self._slot_shared = torch.zeros((n_slots,), dtype=torch.int32, device=self.device)

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
            self._drop_lineage(slots)

    # ---- shared prefixes ---------------------------------------------------------------------------------------------------
    # The examples of one clip start with the same tokens (conversation header + audio block).  fork_slots copies the K/V of those
    # positions from a slot that holds them into idle slots (ops.kv_copy_prefix: no prefill of the prefix), prefill_slots(past=...)
    # runs only the suffix through the layers, and with share_prefix the decode step reads the common positions once per group.
    # Untuned default: below this many common positions a group is not worth its extra launch and merge (no measurement moved it yet).
    MIN_SHARED = 64

    def _drop_lineage(self, slots: Sequence[int]) -> None:
        """Slots that were released or refilled from position 0 leave their lineage."""
        hit = False
        for b in slots:
            hit = hit or self.slot_lineage[b] is not None or b in self._forked
            self.slot_lineage[b], self.slot_shared_host[b] = None, 0
            self._forked.pop(b, None)
        if hit:
            self._rebuild_groups()

    def fork_slots(self, src: int, dsts: Sequence[int], n: int) -> None:
        """Copy positions [0, n) of the active slot `src` into the idle slots `dsts` (every layer and plane, one launch) and leave
        each of them "forked, awaiting suffix": slot_len = n on the host, still idle for the decode step until
        prefill_slots(..., past=[n]) has run its suffix.  src and dsts become one lineage (a new one if src had none); a slot's shared
        length is the number of its leading positions that are bit-identical to the lineage's root."""
        src, dsts = self._check_slots([src])[0], self._check_slots(dsts)
        if self.slot_state_host[src] != ops.ROW_ACTIVE or src in self._forked:
            raise ValueError(f"fork_slots: source slot {src} is not active")
        busy = [b for b in dsts if self.slot_len_host[b] >= 0 or b in self._forked]
        if busy or src in dsts:
            raise ValueError(f"fork_slots: destination slots {busy or [src]} are not idle")
        if not 1 <= n <= self.slot_len_host[src]:
            raise ValueError(f"fork_slots: n={n} outside 1 .. {self.slot_len_host[src]} (the source's length)")
        if not dsts:
            return
        ops.kv_copy_prefix(self.k_cache, self.vt_cache, src, dsts, n, self.k_cache_lo, self.vt_cache_lo)
        if self.slot_lineage[src] is None:                      # src is the root: everything it holds is the root's
            self.slot_lineage[src], self.slot_shared_host[src] = self._lineages, self.smax
            self._lineages += 1
        for b in dsts:
            self.slot_lineage[b], self.slot_shared_host[b] = self.slot_lineage[src], min(n, self.slot_shared_host[src])
            self._forked[b], self.slot_len_host[b] = n, n

    def clone_slots(self, src: int, dsts: Sequence[int]) -> None:
        """Copy the whole of the active slot `src` into the idle slots `dsts` (every layer and plane, one launch): they become active
        at the same length and join src's lineage (a new one if src had none), so with share_prefix the group attention reads what they
        have in common once.  The beams of one example start this way: the prompt is prefilled once."""
        src, dsts = self._check_slots([src])[0], self._check_slots(dsts)
        if self.slot_state_host[src] != ops.ROW_ACTIVE or src in self._forked:
            raise ValueError(f"clone_slots: source slot {src} is not active")
        busy = [b for b in dsts if self.slot_len_host[b] >= 0 or b in self._forked]
        if busy or src in dsts:
            raise ValueError(f"clone_slots: destination slots {busy or [src]} are not idle")
        if not dsts:
            return
        n = self.slot_len_host[src]
        ops.kv_copy_prefix(self.k_cache, self.vt_cache, src, dsts, n, self.k_cache_lo, self.vt_cache_lo)
        if self.slot_lineage[src] is None:
            self.slot_lineage[src], self.slot_shared_host[src] = self._lineages, self.smax
            self._lineages += 1
        for b in dsts:
            self.slot_lineage[b], self.slot_shared_host[b] = self.slot_lineage[src], min(n, self.slot_shared_host[src])
        self._set_slots(dsts, [n] * len(dsts), ops.ROW_ACTIVE)
        self._rebuild_groups()

    def _rebuild_groups(self) -> None:
        """The decode step's group table, from the host's view of the slots: the non-idle slots of one lineage (forked ones only once
        their suffix is in) form a group; its shared length is the smallest of its members', rounded down to a multiple of 8 (the
        per-slot V^T pass starts on a 16-byte chunk); its source is its lowest slot, so a released leader is simply no longer used.
        More than 16 members are cut into several groups; fewer than 2, or fewer than MIN_SHARED positions: no group."""
        if not self.share_prefix:
            return
        by_lineage: Dict[int, List[int]] = {}
        for b in range(self.n_slots):
            if self.slot_lineage[b] is not None and self.slot_len_host[b] >= 0 and b not in self._forked:
                by_lineage.setdefault(self.slot_lineage[b], []).append(b)
        groups: List[Tuple[int, int, List[int]]] = []
        for members in by_lineage.values():
            for c0 in range(0, len(members), ops.SHARED_GROUP_MEMBERS):
                chunk = members[c0:c0 + ops.SHARED_GROUP_MEMBERS]
                P = min(min(self.slot_shared_host[b], self.slot_len_host[b]) for b in chunk) // 8 * 8
                if len(chunk) >= 2 and P >= self.MIN_SHARED:
                    groups.append((chunk[0], P, chunk))
        if groups == self.group_list:
            return
        self.group_list = groups
        shared = [0] * self.n_slots
        tab = torch.zeros((max(1, len(groups)), ops.SHARED_GROUP_STRIDE), dtype=torch.int32)
        for g, (src, P, chunk) in enumerate(groups):
            tab[g, :3 + len(chunk)] = torch.tensor([src, P, len(chunk)] + chunk, dtype=torch.int32)
            for b in chunk:
                shared[b] = P
        self._groups = tab.to(self.device) if groups else None
        self._slot_shared.copy_(torch.tensor(shared, dtype=torch.int32))

    def prefill_slots(self, rows: Sequence[torch.Tensor], audio_segments: Sequence[Tuple[int, int, torch.Tensor]] = (),
                      slots: Optional[Sequence[int]] = None, past: Optional[Sequence[int]] = None) -> torch.Tensor:
        """Prefill new sequences into the given slots at position 0; the other slots keep their caches and positions.
        rows: 1-D int64 token tensors (one per new sequence); audio_segments: (index into rows, position of <audio_start>, frames
        fp32 (F, mm)) as in forward_tokens; slots: the slot of each row (default 0 .. len(rows) - 1).  A run of contiguous slots is
        prefilled as ONE right-padded batch: causal attention never lets a valid position see a pad, and the cache rows written for
        pad positions lie beyond the slot's length, where the decode step overwrites them before it reads them.
        Returns fp32 logits [len(rows), V] of each row's LAST valid token; sets slot_len = row length, state active.
        past: one start position per row.  A row with past > 0 holds only the SUFFIX tokens of a slot that fork_slots left at exactly
        that length: they run through the layers at positions past .. (the prefill-with-past path of forward_tokens) on top of the
        copied prefix; such a row must carry no audio segment.  Runs are then cut by contiguity and equal past."""
        d = self.dims
        assert self.embed is not None and all(L is not None for L in self.layers), "weights not loaded"
        slots = self._check_slots(range(len(rows)) if slots is None else slots)
        if len(slots) != len(rows):
            raise ValueError(f"{len(rows)} rows for {len(slots)} slots")
        rows = [r.reshape(-1).to(device=self.device, dtype=torch.int64) for r in rows]
        lens = [int(r.numel()) for r in rows]
        if past is not None:
            return self._prefill_slots_past(rows, lens, audio_segments, slots, [int(p) for p in past])
        if any(n < 1 or n > self.smax for n in lens):
            raise ValueError(f"row lengths {lens} must be in 1 .. max_seq {self.smax}")
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
            logits[torch.tensor(run, dtype=torch.long, device=self.device)] = self._prefill_run(ids, segs, slots[run[0]], last)
        self._set_slots(slots, lens, ops.ROW_ACTIVE)
        self._drop_lineage(slots)
        return logits

    def _prefill_slots_past(self, rows, lens: List[int], audio_segments, slots: List[int], past: List[int]) -> torch.Tensor:
        """prefill_slots with start positions: rows with past == 0 as ever, the others as suffixes of forked slots."""
        if len(past) != len(rows):
            raise ValueError(f"{len(past)} start positions for {len(rows)} rows")
        for r, (b, p, n) in enumerate(zip(slots, past, lens)):
            if p < 0 or n < 1 or p + n > self.smax:
                raise ValueError(f"row {r}: positions {p} .. {p + n - 1} outside 0 .. max_seq {self.smax} - 1")
            if p > 0 and self._forked.get(b) != p:
                raise ValueError(f"row {r}: slot {b} was not forked to length {p} (fork_slots first)")
            if p > 0 and any(rr == r for (rr, _, _) in audio_segments):
                raise ValueError(f"row {r}: a suffix (past {p}) must contain no audio tokens")
            if p == 0 and b in self._forked:
                raise ValueError(f"row {r}: slot {b} awaits the suffix of its fork at {self._forked[b]}")
        logits = torch.empty((len(rows), self.dims.vocab_size), dtype=torch.float32, device=self.device)
        order = sorted(range(len(rows)), key=lambda r: slots[r])
        runs: List[List[int]] = []
        for r in order:
            if runs and slots[r] == slots[runs[-1][-1]] + 1 and past[r] == past[runs[-1][-1]]:
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
            logits[torch.tensor(run, dtype=torch.long, device=self.device)] = self._prefill_run(ids, segs, slots[run[0]], last, past[run[0]])
        self._set_slots(slots, [p + n for p, n in zip(past, lens)], ops.ROW_ACTIVE)
        fresh = [b for b, p in zip(slots, past) if p == 0]
        for b, p in zip(slots, past):
            if p > 0:
                del self._forked[b]
        if fresh:
            self._drop_lineage(fresh)
        self._rebuild_groups()
        return logits

    def _prefill_run(self, ids: torch.Tensor, segs, slot0: int, last: torch.Tensor, pos0: int = 0) -> torch.Tensor:
        """forward_tokens(last_only=True) of a right-padded batch into cache slots slot0 .. at positions pos0 .., logits of the rows of
        h listed in `last`."""
        B, S = ids.shape
        ws = self._workspace(B, S)
        embed_splice(ids, self.embed, ws["h"], segs, self.proj_w, self.proj_b, self.split)
        self._layers_forward(ws, B, S, pos0, slot0=slot0)
        return self._head_rows(ws["h"].index_select(0, last))

    def _slot_workspace(self):
        """The decode step's own buffers: a refill prefill (other shapes) does not reallocate them."""
        n = self.n_slots
        if self._slot_ws is None or self._slot_ws["h"].shape[0] != n:
            ws = self._alloc_workspace(n, 1)
            ws["logits"] = torch.empty((n, self.dims.vocab_size), dtype=torch.float32, device=self.device)
            ws["next"] = torch.zeros((n,), dtype=torch.int64, device=self.device)
            if 16 < n <= self.MAX_SLOTS:                       # scratch of ops.gemm16_mid: the largest of the step's five products
                d = self.dims
                H, I = d.hidden_size, d.intermediate_size
                need = [ops.gemm16_mid_scratch_bytes(n, nn, w.shape[1], self.split, epi) for nn, w, epi in (
                    (3 * H, self.layers[0].wqkv, ops.EPI_F32), (H, self.layers[0].wo, ops.EPI_RESID),
                    (2 * I, self.layers[0].wgu, self._epi_swiglu()), (H, self.layers[0].wdown, ops.EPI_RESID),
                    (d.vocab_size, self.lm_head, ops.EPI_F32))]
                if min(need) == 0:
                    raise ops._lib.LlarkHipError(f"gemm16_mid does not take this model's decode shapes (H {H}, I {I}, {n} slots)")
                ws["mid"] = torch.empty((max(need) // 4,), dtype=torch.float32, device=self.device)
            self._slot_ws = ws
        if self.share_prefix and "attn_shared" not in self._slot_ws:   # partials of ops.attn_decode_rope_shared; word 0 = its status, zero
            need = ops.attn_decode_shared_scratch_bytes(n, self.dims.num_attention_heads)
            self._slot_ws["attn_shared"] = torch.zeros((need // 4,), dtype=torch.float32, device=self.device)
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

    def decode_slots(self, ids: torch.Tensor, eos: int = -1, pad: int = 0, out_col: Optional[torch.Tensor] = None,
                     sample=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """One decode step over all n_slots rows, each at its own position: embedding -> decoder layers (the uniform decode GEMMs up
        to 16 slots, ops.gemm16_mid for 17 .. 64; attention by ops.attn_decode_rope_rows over slot_len) -> final norm + lm_head -> advance_slots.  ids: int64 [n_slots] (the
        token of each slot at position slot_len; idle rows pass through the row-independent GEMMs harmlessly).  sample: optional
        callable logits -> int64 [n_slots] tokens (sampling); greedy otherwise.  Returns (next ids on the device, their host copy,
        the step's fp32 logits [n_slots, V] -- a buffer the next step overwrites)."""
        logits = self._slot_logits(ids)
        nxt, host = self.advance_slots(logits, eos, pad, out_col, None if sample is None else sample(logits))
        return nxt, host, logits

    def _slot_logits(self, ids: torch.Tensor) -> torch.Tensor:
        """The decode step up to the logits: embedding -> decoder layers -> final norm + lm_head, every slot at its own position."""
        n = self.n_slots
        if n == 0:
            raise RuntimeError("ragged mode is not active: call init_slots(n) first")
        full = [b for b in range(n) if self.slot_state_host[b] == ops.ROW_ACTIVE and self.slot_len_host[b] >= self.smax]
        if full:
            raise ValueError(f"slot(s) {full} reached the engine's max_seq {self.smax}")
        ids = ids.reshape(-1)
        assert ids.numel() == n and ids.dtype == torch.int64
        ws = self._slot_workspace()
        h, logits = ws["h"], ws["logits"]
        ops.embed_gather(ids.contiguous(), self.embed, h)
        normed = self._layers_forward(ws, n, 1, 0, pos_rows=self.slot_len)
        self._head(ws, logits, normed, may_fuse=True)
        return logits

    # ---- speculative greedy decoding: a decode step over a block of rows per slot -------------------------------------------------
    # Row 0 of slot b is the token the plain step would feed (at position slot_len[b]); rows 1 .. are drafted tokens at the following
    # positions.  One pass over the weights gives the greedy token after every row; ops.spec_verify_rows keeps the drafts that equal
    # them and emits one token more.  Rejected positions need no rollback: they lie beyond slot_len and are overwritten before they are
    # read.  llark_amd.m2t.speculate holds the loop.
    def init_block_decode(self, stride: int) -> None:
        """Allocate the block step's own workspace: n_slots * stride <= 16 rows (the row count the m <= 16 decode Linears take)."""
        n = self.n_slots
        if n == 0:
            raise RuntimeError("ragged mode is not active: call init_slots(n) first")
        if not 1 <= stride <= ops.SPEC_MAX_BLOCK or n * stride > 16:
            raise ValueError(f"block decode needs 1 <= stride <= {ops.SPEC_MAX_BLOCK} and n_slots * stride <= 16, got {n} slots x {stride}")
        dev, i32, i64 = self.device, torch.int32, torch.int64
        ws = self._alloc_workspace(n * stride, 1)
        ws.update(stride=stride, logits=torch.empty((n * stride, self.dims.vocab_size), dtype=torch.float32, device=dev),
                  ids=torch.zeros((n * stride,), dtype=i64, device=dev), blk=torch.zeros((n,), dtype=i32, device=dev),
                  budget=torch.zeros((n,), dtype=i32, device=dev), next=torch.zeros((n,), dtype=i64, device=dev),
                  step=ops.spec_step_buffer(n, dev), hist=torch.zeros((n, self.smax + 1), dtype=i64, device=dev),
                  hist_len=torch.zeros((n,), dtype=i32, device=dev))
        self._block_ws = ws

    def start_block_decode(self, histories: Sequence[torch.Tensor], budgets: Sequence[int]) -> None:
        """Every slot's history (prompt and the tokens emitted so far, the last of which the next step feeds) and the number of tokens
        it may still emit."""
        ws = self._block_ws
        if len(histories) != self.n_slots or len(budgets) != self.n_slots:
            raise ValueError(f"{self.n_slots} slots need as many histories and budgets")
        hist = torch.zeros(ws["hist"].shape, dtype=torch.int64)
        for b, r in enumerate(histories):
            r = r.reshape(-1).to("cpu", torch.int64)
            if not 1 <= r.numel() <= hist.shape[1]:
                raise ValueError(f"slot {b}: a history of {r.numel()} tokens (1 .. max_seq + 1)")
            hist[b, : r.numel()] = r
        ws["hist"].copy_(hist)
        ws["hist_len"].copy_(torch.tensor([int(r.numel()) for r in histories], dtype=torch.int32))
        ws["next"].copy_(torch.tensor([int(r.reshape(-1)[-1]) for r in histories], dtype=torch.int64))
        ws["budget"].copy_(torch.tensor([int(x) for x in budgets], dtype=torch.int32))

    def decode_block(self, eos: int = -1, pad: int = 0, k_max: int = 1, g_max: int = 2, drafts: Optional[torch.Tensor] = None,
                     n_drafts: Optional[torch.Tensor] = None) -> Tuple[List[List[int]], torch.Tensor, torch.Tensor]:
        """One block step over all slots: draft (prompt lookup over the device history with suffixes of g_max .. 1 tokens, or
        `drafts` int64 [n_slots][>= k_max] with `n_drafts` int32 [n_slots]) -> embedding -> the <= 16-row decode launch sequence with the
        block attention -> final norm + lm_head -> verify.  Returns (the tokens each slot emitted, host lists; the block's input ids
        [n_slots][stride] on the device; the fp32 logits [n_slots * stride][V], row b*stride + i being what token i of slot b was
        chosen from -- buffers the next step overwrites).  One device-to-host transfer."""
        ws, n = self._block_ws, self.n_slots
        stride = ws["stride"]
        if not 0 <= k_max < stride:
            raise ValueError(f"k_max must be in 0 .. stride - 1 = {stride - 1}, got {k_max}")
        ops.spec_draft_rows(ws["next"], self.slot_state, self.slot_len, ws["budget"], ws["ids"], ws["blk"], stride, k_max, self.smax,
                            **(dict(hist=ws["hist"], hist_len=ws["hist_len"], g_max=g_max) if drafts is None else
                               dict(drafts=drafts, n_drafts=n_drafts)), pad=max(pad, 0))
        ops.embed_gather(ws["ids"], self.embed, ws["h"])
        normed = self._decode_layers(ws, n * stride, 0, self.dims.num_hidden_layers, None, None, 0, self.slot_len, block=(stride, ws["blk"]))
        self._head(ws, ws["logits"], normed, may_fuse=False)
        out_tokens, n_out = ops.spec_step_views(ws["step"])
        ops.spec_verify_rows(ws["logits"], ws["ids"], ws["blk"], self.slot_state, self.slot_len, ws["budget"], out_tokens, n_out, ws["next"],
                             ws["hist"], ws["hist_len"], eos=eos, pad=pad)
        toks, cnt = ops.spec_step_views(ws["step"].cpu())
        emitted = []
        for b in range(n):
            k = int(cnt[b])
            emitted.append(toks[b, :k].tolist())
            if k:
                self.slot_len_host[b] += k
                if eos >= 0 and emitted[-1][-1] == eos:
                    self.slot_state_host[b] = ops.ROW_FINISHED
        return emitted, ws["ids"].view(n, stride), ws["logits"]

    def truncate_slots(self, slots: Sequence[int], lens: Sequence[int]) -> None:
        """Set slots back to shorter lengths, on the host and the device (after a host-side stop inside an accepted run): the positions
        beyond are overwritten before they are read."""
        slots = self._check_slots(slots)
        lens = [int(x) for x in lens]
        for b, x in zip(slots, lens):
            if not 0 <= x <= self.slot_len_host[b]:
                raise ValueError(f"slot {b}: cannot truncate length {self.slot_len_host[b]} to {x}")
        if slots:
            idx = torch.tensor(slots, dtype=torch.long, device=self.device)
            self.slot_len[idx] = torch.tensor(lens, dtype=torch.int32, device=self.device)
            for b, x in zip(slots, lens):
                self.slot_len_host[b] = x

    def beam_step(self, ids: Optional[torch.Tensor], beam, logits: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, List[bool]]:
        """One beam-search step over all n_slots rows (beam: llark_amd.m2t.beam.BeamSearch, which owns example e's slots e * B ..):
        the decode step up to the logits on `ids` (int64 [n_slots], the token of the beam now in each slot), then the three launches
        of the beam step -- ops.beam_topk_rows, ops.beam_advance, ops.kv_copy_slots -- instead of advance_slots.  ids None: the step on
        `logits` [n_slots, V] of the prompts' last tokens (replicated per beam): no forward, no position advances and, the slots being
        clones, no K/V move.  Returns (next ids on the device, the examples' done flags -- the step's one device-to-host transfer)."""
        first = ids is None
        if not first:
            logits = self._slot_logits(ids)
        B = beam.beams
        was_done = list(beam.done_host)
        kv = None if first else (self.k_cache, self.vt_cache, self.k_cache_lo, self.vt_cache_lo)
        if getattr(beam, "constraints", None) is not None or getattr(beam, "guide", None) is not None:
            nxt, done = beam.step(logits, self.slot_state, None if first else self.slot_len, kv, last=ids)
        else:
            nxt, done = beam.step(logits, self.slot_state, None if first else self.slot_len, kv)
        for e, (w, dn) in enumerate(zip(was_done, done)):
            for b in range(e * B, e * B + B):
                if not w and not first:
                    self.slot_len_host[b] += 1
                if dn:
                    self.slot_state_host[b] = ops.ROW_FINISHED
        return nxt, done
