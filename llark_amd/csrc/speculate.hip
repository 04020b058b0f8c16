// Device bookkeeping of a speculative greedy decode step (engine.decode_block): verify the block's drafts against the greedy token of
// every row, emit the accepted run, then fill the next block.  One 1024-thread workgroup per slot; the exact contract is in
// include/llark_hip.h (llark_spec_verify_rows, llark_spec_draft_rows).  Greedy verification is exact: the tokens emitted are those of the
// plain loop (llark_decode_advance_rows), whatever the drafts were.
#include "common.h"

namespace llark {

// llark_decode_advance_rows' order: first maximal index, a NaN counts as the maximum (torch.argmax).  A strict total order, so the
// reduction tree does not matter.
__device__ __forceinline__ bool spec_better(float v, int i, float bv, int bi) {
    const bool vn = v != v, bn = bv != bv;
    if (vn || bn) return vn && (!bn || i < bi);
    return v > bv || (v == bv && i < bi);
}

constexpr int SPEC_MAX = 8;                    // rows of a block, tokens emitted per step

__global__ __launch_bounds__(1024) void spec_verify_kernel(const float* __restrict__ logits, int ldl, int vocab, int stride,
                                                           const long long* __restrict__ ids, const int* __restrict__ blk, int* state,
                                                           int* pos_rows, int* budget, long long eos, long long pad,
                                                           long long* __restrict__ out_tokens, long long* __restrict__ n_out,
                                                           long long* __restrict__ next_ids, long long* hist, int* hist_len, int ld_hist) {
    __shared__ float sv[16];
    __shared__ int si[16];
    __shared__ int g[SPEC_MAX];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int nb = blk[b];
    nb = nb < stride ? nb : stride;
    const int st = state[b], bud = budget[b];
    __syncthreads();                               // every wave has read the slot's words before thread 0 may change them
    if (st != LLARK_ROW_ACTIVE || nb <= 0 || bud <= 0) {
        if (tid < SPEC_MAX) out_tokens[(size_t)b * SPEC_MAX + tid] = pad;
        if (tid == 0) n_out[b] = 0;
        return;
    }
    for (int i = 0; i < nb; ++i) {
        const float* row = logits + ((size_t)b * stride + i) * ldl;
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int j = tid; j < vocab; j += 1024) {
            const float v = row[j];
            if (spec_better(v, j, bv, bi)) bv = v, bi = j;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (spec_better(ov, oi, bv, bi)) bv = ov, bi = oi;
        }
        if (lane == 0) sv[wv] = bv, si[wv] = bi;
        __syncthreads();
        if (tid == 0) {
            bv = sv[0], bi = si[0];
            for (int w = 1; w < 16; ++w)
                if (spec_better(sv[w], si[w], bv, bi)) bv = sv[w], bi = si[w];
            g[i] = bi;
        }
        __syncthreads();
    }
    if (tid == 0) {
        int a = 0;                                 // accepted drafts: leading i with ids[i + 1] == g_i
        while (a < nb - 1 && ids[(size_t)b * stride + a + 1] == (long long)g[a]) ++a;
        int n = a + 1;                             // g_0 .. g_a, cut at the budget and after the first eos
        n = n < bud ? n : bud;
        bool fin = false;
        for (int i = 0; i < n; ++i)
            if (eos >= 0 && (long long)g[i] == eos) {
                n = i + 1;
                fin = true;
                break;
            }
        int hl = hist ? hist_len[b] : 0;
        for (int i = 0; i < SPEC_MAX; ++i) out_tokens[(size_t)b * SPEC_MAX + i] = i < n ? (long long)g[i] : pad;
        if (hist) {
            for (int i = 0; i < n; ++i)
                if (hl < ld_hist) hist[(size_t)b * ld_hist + hl++] = g[i];
            hist_len[b] = hl;
        }
        n_out[b] = n;
        next_ids[b] = g[n - 1];
        pos_rows[b] += n;
        budget[b] = bud - n;
        if (fin) state[b] = LLARK_ROW_FINISHED;
    }
}

__global__ __launch_bounds__(1024) void spec_draft_kernel(const long long* __restrict__ next_ids, const int* __restrict__ state,
                                                          const int* __restrict__ pos_rows, const int* __restrict__ budget,
                                                          const long long* __restrict__ hist, const int* __restrict__ hist_len, int ld_hist,
                                                          int stride, int k_max, int g_max, int smax, const long long* __restrict__ drafts,
                                                          const int* __restrict__ n_drafts, int ld_drafts, long long* __restrict__ ids,
                                                          int* __restrict__ blk, long long pad) {
    __shared__ int best;
    const int b = blockIdx.x, tid = threadIdx.x;
    long long* row = ids + (size_t)b * stride;
    const int pos = pos_rows[b], bud = budget[b];
    int cap = stride < bud ? stride : bud;        // blk <= budget and pos + blk <= smax
    cap = cap < smax - pos ? cap : smax - pos;
    if (state[b] != LLARK_ROW_ACTIVE || pos < 0 || cap <= 0) {
        if (tid < stride) row[tid] = pad;
        if (tid == 0) blk[b] = 0;
        return;
    }
    int nd = 0, from = 0;                          // drafts: src[from .. from + nd)
    const long long* src = nullptr;
    if (drafts) {
        src = drafts + (size_t)b * ld_drafts;
        nd = n_drafts[b];
        nd = nd < 0 ? 0 : (nd < ld_drafts ? nd : ld_drafts);
    } else {
        // prompt lookup: the longest suffix (g_max .. 1 tokens) of the history that occurs earlier, its most recent earlier occurrence
        // (one that ends before the history's last token, so at least one token follows it), the tokens that follow it
        const long long* hrow = hist + (size_t)b * ld_hist;
        int len = hist_len[b];
        len = len < 0 ? 0 : (len < ld_hist ? len : ld_hist);
        for (int g = g_max; g >= 1 && nd == 0; --g) {
            if (len < g + 1) continue;             // uniform per block
            if (tid == 0) best = -1;
            __syncthreads();
            int mine = -1;
            for (int s = tid; s <= len - g - 1; s += 1024) {
                bool eq = true;
                for (int e = 0; e < g; ++e) eq = eq && hrow[s + e] == hrow[len - g + e];
                if (eq) mine = s;                  // ascending: the last hit of this thread is its most recent
            }
            if (mine >= 0) atomicMax(&best, mine);
            __syncthreads();
            const int s = best;
            __syncthreads();                       // everyone has read `best` before the next length resets it
            if (s >= 0) {
                src = hrow;
                from = s + g;
                nd = len - from;
            }
        }
    }
    nd = nd < k_max ? nd : k_max;
    nd = nd < cap - 1 ? nd : cap - 1;
    if (tid < stride) row[tid] = tid == 0 ? next_ids[b] : (tid <= nd ? src[from + tid - 1] : pad);
    if (tid == 0) blk[b] = 1 + nd;
}

}  // namespace llark

using namespace llark;

extern "C" int llark_spec_verify_rows(const float* logits, int ldl, int vocab, int n_slots, int stride, const int64_t* ids, const int* blk,
                                      int* state, int* pos_rows, int* budget, int64_t eos, int64_t pad, int64_t* out_tokens, int64_t* n_out,
                                      int64_t* next_ids, int64_t* hist, int* hist_len, int ld_hist, llark_stream_t stream) {
    LLARK_REQUIRE(logits && ids && blk && state && pos_rows && budget && out_tokens && n_out && next_ids, "spec_verify_rows: null pointer");
    LLARK_REQUIRE((hist == nullptr) == (hist_len == nullptr) && (!hist || ld_hist > 0), "spec_verify_rows: hist, hist_len and ld_hist > 0 come together");
    LLARK_REQUIRE(n_slots > 0 && n_slots <= 65535 && stride >= 1 && stride <= SPEC_MAX && vocab > 0 && ldl >= vocab,
                  "spec_verify_rows: bad shape n_slots=%d stride=%d vocab=%d ldl=%d (stride 1 .. 8, ldl >= vocab)", n_slots, stride, vocab, ldl);
    spec_verify_kernel<<<n_slots, 1024, 0, (hipStream_t)stream>>>(logits, ldl, vocab, stride, (const long long*)ids, blk, state, pos_rows, budget,
                                                                  (long long)eos, (long long)pad, (long long*)out_tokens, (long long*)n_out,
                                                                  (long long*)next_ids, (long long*)hist, hist_len, ld_hist);
    return check_launch("spec_verify_rows");
}

extern "C" int llark_spec_draft_rows(const int64_t* next_ids, const int* state, const int* pos_rows, const int* budget, const int64_t* hist,
                                     const int* hist_len, int ld_hist, int n_slots, int stride, int k_max, int g_max, int smax,
                                     const int64_t* drafts, const int* n_drafts, int ld_drafts, int64_t* ids, int* blk, int64_t pad,
                                     llark_stream_t stream) {
    LLARK_REQUIRE(next_ids && state && pos_rows && budget && ids && blk, "spec_draft_rows: null pointer");
    LLARK_REQUIRE(drafts ? (n_drafts && ld_drafts > 0) : (hist && hist_len && ld_hist > 0),
                  "spec_draft_rows: give drafts + n_drafts + ld_drafts > 0, or hist + hist_len + ld_hist > 0");
    LLARK_REQUIRE(n_slots > 0 && n_slots <= 65535 && stride >= 1 && stride <= SPEC_MAX && k_max >= 0 && k_max < SPEC_MAX && smax > 0 &&
                      (drafts || (g_max >= 1 && g_max <= 64)),
                  "spec_draft_rows: bad shape n_slots=%d stride=%d k_max=%d g_max=%d smax=%d (stride 1 .. 8, k_max 0 .. 7, g_max 1 .. 64)", n_slots,
                  stride, k_max, g_max, smax);
    spec_draft_kernel<<<n_slots, 1024, 0, (hipStream_t)stream>>>((const long long*)next_ids, state, pos_rows, budget, (const long long*)hist, hist_len,
                                                                 ld_hist, stride, k_max, g_max, smax, (const long long*)drafts, n_drafts, ld_drafts,
                                                                 (long long*)ids, blk, (long long)pad);
    return check_launch("spec_draft_rows");
}
