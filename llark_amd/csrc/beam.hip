// Beam search on the device (llark_beam_topk_rows, llark_beam_advance, llark_kv_copy_slots): the step of HF 4.29.2's beam_search +
// BeamSearchScorer (one beam group) after the logits -- candidates per beam, the merge into the next beams and the finished-hypothesis
// heap, and the K/V move between the slots of beams that fork.  Contracts: include/llark_hip.h.
//
// llark_beam_topk_rows: one workgroup of 1024 threads per row.  Column ownership, the maximum and the sum of exponentials are those of
// csrc/logprob.hip -- thread tid owns the columns tid, tid + 1024, ...; per thread in column order, a butterfly over the lanes, the 16 wave
// sums in wave order -- so lp(t) = (l_t - M) - logf(S) has the bits llark_token_logprob_rows gives.  The first NPT columns of a thread
// stay in registers: a row of up to 1024 * NPT columns is read from memory once.  Selection: every column has the 64-bit key
// (order-preserving image of fp32(score + lp)) << 32 | ~token, unique in the row, whose descending order IS the tie rule (candidate
// descending, token ascending).  Each thread holds the largest key of its columns below the last winner; a round is one block maximum
// (one barrier), after which only the winner's owner rescans its columns.  2B rounds, trip counts fixed before the loop starts.
//
// llark_beam_advance: one wave per example; the merge of B sorted lists of 2B candidates and the hypothesis bookkeeping are a few
// hundred comparisons and run on lane 0, the other lanes stage the lists in LDS.  llark_kv_copy_slots: the 16-byte chunks of
// llark_kv_copy_prefix (csrc/attn_shared.hip) for a copy list in device memory.
//
// No workgroup waits for another; plain C++ and vector stores; the only atomic is the add on the nullable `fallbacks` counter.
#include "common.h"

namespace llark {

constexpr int BEAM_THREADS = 1024;
constexpr int BEAM_WAVES = BEAM_THREADS / 64;
constexpr int BEAM_MAX = 16;                                      // beams per example
constexpr int BEAM_HEAP_STRIDE = 8;                               // int32 words per heap entry (include/llark_hip.h)
constexpr int BEAM_META_STRIDE = 4;

struct BeamTopkArgs {
    const float* logits;
    int ldl, vocab, slots, k;
    const int* state;
    const int* slot_of_row;
    const float* score;
    float* cand_score;
    int* cand_token;
    float* cand_logprob;
    int* fallbacks;
    const unsigned* ban;                                          // BAN instantiation only: uint32 [slots][ld_ban]
    int ld_ban;
};

// order-preserving image of a non-NaN float: a < b  <=>  key(a) < key(b); -inf -> 0x007fffff, so 0 lies below every float
__device__ __forceinline__ unsigned beam_key(float x) {
    const unsigned b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ unsigned long long beam_comp(float cand, int token) {
    return ((unsigned long long)beam_key(cand) << 32) | (unsigned long long)(0xffffffffu - (unsigned)token);
}
__device__ __forceinline__ unsigned long long beam_max_u64(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

// BAN: a column whose bit of ban[slot] is set gets key 0 -- it is left out of the selection and still counts in M and S
template <int NPT, bool BAN = false>
__global__ __launch_bounds__(BEAM_THREADS) void beam_topk_rows_kernel(const BeamTopkArgs a) {
    __shared__ float smax[BEAM_WAVES];
    __shared__ int sbad[BEAM_WAVES];
    __shared__ float ssum[BEAM_WAVES];
    __shared__ unsigned long long sred[2][BEAM_WAVES];
    __shared__ unsigned long long swin[2 * BEAM_MAX];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int slot = a.slot_of_row ? a.slot_of_row[r] : r;
    if (slot < 0 || slot >= a.slots) return;                      // workgroup-uniform, like every return below
    if (a.state && a.state[slot] != LLARK_ROW_ACTIVE) return;
    const int vocab = a.vocab, K = a.k;
    const float* row = a.logits + (size_t)r * a.ldl;
    float* out_s = a.cand_score + (size_t)r * K;
    int* out_t = a.cand_token + (size_t)r * K;
    float* out_l = a.cand_logprob + (size_t)r * K;

    // ---- the row into registers; maximum and NaN flag (csrc/logprob.hip, pass 1) -----------------------------------------------------
    float v[NPT];
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
        const int j = tid + BEAM_THREADS * i;
        v[i] = j < vocab ? row[j] : -INFINITY;
    }
    float m = -INFINITY;
    int bad = 0;
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
        m = fmaxf(m, v[i]);
        bad |= v[i] != v[i] ? 1 : 0;
    }
    for (long long j = (long long)NPT * BEAM_THREADS + tid; j < vocab; j += BEAM_THREADS) {
        const float x = row[j];
        m = fmaxf(m, x);
        bad |= x != x ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        m = fmaxf(m, __shfl_xor(m, o, 64));
        bad |= __shfl_xor(bad, o, 64);
    }
    if (lane == 0) smax[wv] = m, sbad[wv] = bad;
    __syncthreads();
    float M = smax[0];
    int any_bad = sbad[0];
#pragma unroll
    for (int w = 1; w < BEAM_WAVES; ++w) M = fmaxf(M, smax[w]), any_bad |= sbad[w];
    if (any_bad || !(fabsf(M) < INFINITY)) {                      // a NaN in the row, or a maximum of +-inf: no candidates
        if (tid < K) out_s[tid] = -INFINITY, out_t[tid] = -1, out_l[tid] = -INFINITY;
        if (tid == 0 && a.fallbacks) atomicAdd(a.fallbacks, 1);
        return;
    }

    // ---- S = sum of expf(l - M) in the order of csrc/logprob.hip, pass 2 -------------------------------------------------------------
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < NPT; ++i) s += expf(v[i] - M);
    for (long long j = (long long)NPT * BEAM_THREADS + tid; j < vocab; j += BEAM_THREADS) s += expf(row[j] - M);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) ssum[wv] = s;
    __syncthreads();
    float S = ssum[0];
#pragma unroll
    for (int w = 1; w < BEAM_WAVES; ++w) S += ssum[w];
    const float logS = logf(S);
    const float score = a.score[slot];

    // ---- selection: K rounds of a block maximum over the keys below the last winner ---------------------------------------------------
    // + 0: -0 becomes +0, so the key order is the float order
#define BEAM_CAND(x) ((score + (((x) - M) - logS)) + 0.0f)
    const unsigned* banw = nullptr;
    if constexpr (BAN) banw = a.ban + (size_t)slot * a.ld_ban;
#define BEAM_KEY(x, j) (BAN && ((banw[(j) >> 5] >> ((j) & 31)) & 1u) ? 0ull : beam_comp(BEAM_CAND(x), (int)(j)))
    unsigned long long mine = 0ull;
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
        const int j = tid + BEAM_THREADS * i;
        if (j < vocab) mine = beam_max_u64(mine, BEAM_KEY(v[i], j));
    }
    for (long long j = (long long)NPT * BEAM_THREADS + tid; j < vocab; j += BEAM_THREADS)
        mine = beam_max_u64(mine, BEAM_KEY(row[j], j));
    int parity = 0;
#pragma unroll 1
    for (int k = 0; k < K; ++k) {
        unsigned long long w = mine;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) w = beam_max_u64(w, (unsigned long long)__shfl_xor((long long)w, o, 64));
        if (lane == 0) sred[parity][wv] = w;
        __syncthreads();
        w = sred[parity][0];
#pragma unroll
        for (int x = 1; x < BEAM_WAVES; ++x) w = beam_max_u64(w, sred[parity][x]);
        parity ^= 1;
        if (tid == 0) swin[k] = w;
        if (mine == w && w != 0ull) {                             // the owner (keys are unique): its largest key below the winner
            unsigned long long nxt = 0ull;
#pragma unroll
            for (int i = 0; i < NPT; ++i) {
                const int j = tid + BEAM_THREADS * i;
                const unsigned long long c = j < vocab ? BEAM_KEY(v[i], j) : 0ull;
                if (c < w) nxt = beam_max_u64(nxt, c);
            }
            for (long long j = (long long)NPT * BEAM_THREADS + tid; j < vocab; j += BEAM_THREADS) {
                const unsigned long long c = BEAM_KEY(row[j], j);
                if (c < w) nxt = beam_max_u64(nxt, c);
            }
            mine = nxt;
        }
    }
    __syncthreads();
    if (tid < K) {
        const unsigned long long w = swin[tid];
        if (w == 0ull) {                                          // fewer than K columns left (only under bans): never an index out of the row
            out_s[tid] = -INFINITY, out_t[tid] = -1, out_l[tid] = -INFINITY;
        } else {
            const int t = (int)(0xffffffffu - (unsigned)(w & 0xffffffffull));
            const float lp = (row[t] - M) - logS;
            out_s[tid] = score + lp;
            out_t[tid] = t;
            out_l[tid] = lp;
        }
    }
#undef BEAM_KEY
#undef BEAM_CAND
}

struct BeamAdvanceArgs {
    const float* cand_score;
    const int* cand_token;
    const float* cand_logprob;
    int beams, step;
    long long eos, pad;
    float length_penalty;
    int early_stopping;
    int open;                                                     // llark_beam_advance_open: an example goes on with fewer than B live beams
    float* score;
    int* rank_of_slot;
    int* state;
    int* pos_rows;
    int* cur_len;
    long long* next_ids;
    int* heap;
    int* heap_meta;
    int* done;
    int* trellis;
    int* pairs;
    int* pair_count;
};

// HF's BeamHypotheses.add on the packed heap of one example: entry = {score, sum, length, end step, end slot, order of arrival, logprob
// of the closing eos (NaN: none), 0}; meta = {count, worst score, arrivals, 0}
__device__ void beam_heap_add(int* heap, int* meta, int B, float sum, int length, float length_penalty, int end_step, int end_slot, float eos_lp) {
    const float sc = (float)((double)sum / pow((double)length, (double)length_penalty));
    int count = meta[0];
    const int arrivals = meta[2];
    meta[2] = arrivals + 1;
    int at = -1;
    if (count < B) {
        at = count++;
    } else if (sc > __int_as_float(meta[1])) {
        int worst = 0;                                            // the lowest score, the earliest arrival among equals
        for (int i = 1; i < B; ++i) {
            const float si = __int_as_float(heap[i * BEAM_HEAP_STRIDE]), sw = __int_as_float(heap[worst * BEAM_HEAP_STRIDE]);
            if (si < sw || (si == sw && heap[i * BEAM_HEAP_STRIDE + 5] < heap[worst * BEAM_HEAP_STRIDE + 5])) worst = i;
        }
        at = worst;
    }
    if (at < 0) return;
    int* e = heap + at * BEAM_HEAP_STRIDE;
    e[0] = __float_as_int(sc), e[1] = __float_as_int(sum), e[2] = length, e[3] = end_step, e[4] = end_slot, e[5] = arrivals;
    e[6] = __float_as_int(eos_lp), e[7] = 0;
    float w = __int_as_float(heap[0]);
    for (int i = 1; i < count; ++i) w = fminf(w, __int_as_float(heap[i * BEAM_HEAP_STRIDE]));
    meta[0] = count;
    meta[1] = __float_as_int(w);
}

__global__ __launch_bounds__(64) void beam_advance_kernel(const BeamAdvanceArgs a) {
    __shared__ float cs[BEAM_MAX][2 * BEAM_MAX];                  // [old rank][position in the beam's sorted list]
    __shared__ int ct[BEAM_MAX][2 * BEAM_MAX];
    __shared__ float cl[BEAM_MAX][2 * BEAM_MAX];
    __shared__ int slot_of_rank[BEAM_MAX];
    const int e = blockIdx.x, B = a.beams, K = 2 * B, base = e * B, lane = threadIdx.x;
    int* tr = a.trellis + ((size_t)a.step * gridDim.x * B + base) * 3;
    if (a.done[e]) {                                              // workgroup-uniform
        if (lane < B) {
            a.next_ids[base + lane] = a.pad;
            tr[lane * 3] = -1, tr[lane * 3 + 1] = -1, tr[lane * 3 + 2] = 0x7fc00000;
        }
        if (lane == 0) a.pair_count[e] = 0;
        return;
    }
    if (lane < BEAM_MAX) slot_of_rank[lane] = lane < B ? lane : 0;   // whatever rank_of_slot holds, every index below stays in range
    __syncthreads();
    if (lane < B) {
        const int rk = a.rank_of_slot[base + lane];
        if (rk >= 0 && rk < B) slot_of_rank[rk] = lane;
    }
    __syncthreads();
    for (int i = lane; i < B * K; i += 64) {
        const int rk = i / K, k = i % K, src = (base + slot_of_rank[rk]) * K + k;
        cs[rk][k] = a.cand_score[src], ct[rk][k] = a.cand_token[src], cl[rk][k] = a.cand_logprob[src];
    }
    __syncthreads();
    if (lane != 0) return;

    const int cur_len = a.cur_len[e];
    int* heap = a.heap + (size_t)e * B * BEAM_HEAP_STRIDE;
    int* meta = a.heap_meta + e * BEAM_META_STRIDE;
    int head[BEAM_MAX], parent[BEAM_MAX], tok[BEAM_MAX], first_child[BEAM_MAX];
    float nsc[BEAM_MAX], nlp[BEAM_MAX];
    for (int i = 0; i < B; ++i) head[i] = 0, first_child[i] = -1;
    int live = 0;
    float best0 = -INFINITY;
    for (int k = 0; k < K && live < B; ++k) {
        int rk = -1;                                              // candidate descending, then rank ascending; token order is the list's
        for (int i = 0; i < B; ++i)
            if (head[i] < K && (rk < 0 || cs[i][head[i]] > cs[rk][head[rk]])) rk = i;
        const int h = head[rk]++;
        const float c = cs[rk][h], lp = cl[rk][h];
        const int t = ct[rk][h];
        if (k == 0) best0 = c;
        if (t < 0) continue;                                      // a row without a distribution: never taken
        if (a.open && c == -INFINITY) continue;                   // open: the row of a slot that holds no beam
        if (a.eos >= 0 && t == a.eos) {
            if (k < B) beam_heap_add(heap, meta, B, c, cur_len, a.length_penalty, a.step, base + slot_of_rank[rk], lp);
            continue;
        }
        parent[live] = slot_of_rank[rk], tok[live] = t, nsc[live] = c, nlp[live] = lp;
        if (first_child[slot_of_rank[rk]] < 0) first_child[slot_of_rank[rk]] = live;
        ++live;
    }
    bool done = a.open ? live == 0 : live < B;                    // rows without candidates: the example cannot go on
    if (!done && meta[0] >= B) {
        const float cur = (float)((double)best0 / pow((double)cur_len, (double)a.length_penalty));
        done = a.early_stopping || __int_as_float(meta[1]) >= cur;
    }
    // the first child of a parent keeps the parent's slot; every further child takes, in rank order, the lowest slot whose old beam has
    // no child: a copy reads a slot nobody writes and writes a slot nobody reads
    int n_pairs = 0, free_slot = 0;
    for (int q = 0; q < live; ++q) {
        int slot = parent[q];
        if (first_child[slot] != q) {
            while (first_child[free_slot] >= 0) ++free_slot;
            slot = free_slot++;
            if (!done) {
                int* p = a.pairs + ((size_t)e * (B > 1 ? B - 1 : 1) + n_pairs) * 2;
                p[0] = base + parent[q], p[1] = base + slot;
                ++n_pairs;
            }
        }
        const int g = base + slot;
        a.score[g] = nsc[q];
        a.rank_of_slot[g] = q;
        a.next_ids[g] = done ? a.pad : (long long)tok[q];
        tr[slot * 3] = base + parent[q], tr[slot * 3 + 1] = tok[q], tr[slot * 3 + 2] = __float_as_int(nlp[q]);
    }
    for (int q = live; q < B; ++q) {                              // only when live < B: the slots left over hold nothing
        while (first_child[free_slot] >= 0) ++free_slot;
        const int slot = free_slot++, g = base + slot;
        a.score[g] = -INFINITY;
        a.rank_of_slot[g] = q;
        a.next_ids[g] = a.pad;
        tr[slot * 3] = -1, tr[slot * 3 + 1] = -1, tr[slot * 3 + 2] = 0x7fc00000;
    }
    a.pair_count[e] = n_pairs;
    a.cur_len[e] = cur_len + 1;
    for (int i = 0; i < B; ++i) {
        if (a.pos_rows) a.pos_rows[base + i] += 1;
        if (done) a.state[base + i] = LLARK_ROW_FINISHED;
    }
    if (done) a.done[e] = 1;
}

// blockIdx.z = entry of the copy list, blockIdx.y = layer * nh + head, blockIdx.x * 256 + thread = 16-byte chunk of the span: first the K
// rows [p0, n) (16 chunks each), then the chunks [p0 / 8, ceil(n / 8)) of the 128 V^T rows.  Every return is workgroup-uniform but the last.
__global__ __launch_bounds__(256) void kv_copy_slots_kernel(uint4* k, uint4* vt, uint4* k_lo, uint4* vt_lo, int slots, int nh, int smax,
                                                            const int* pairs, const int* count, int stride, const int* p0_rows,
                                                            const int* pos_rows, int max_span) {
    const int z = blockIdx.z;
    if (z % stride >= count[z / stride]) return;
    const int src = pairs[2 * z], dst = pairs[2 * z + 1];
    if (src < 0 || src >= slots || dst < 0 || dst >= slots || src == dst) return;
    const int p0 = p0_rows[dst], n = pos_rows[src];
    if (p0 < 0 || (p0 & 7) || n <= p0 || n > smax || n - p0 > max_span) return;
    const int layer = blockIdx.y / nh, head = blockIdx.y % nh;
    const int c0 = p0 >> 3, nch = ((n + 7) >> 3) - c0, kch = (n - p0) * 16, vch = 128 * nch;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= kch + vch) return;
    const size_t per_head = (size_t)smax * 16;                    // uint4 per (slot, head) of either cache
    const bool isv = i >= kch;
    const size_t off = isv ? (size_t)((i - kch) / nch) * (smax >> 3) + c0 + (i - kch) % nch : (size_t)p0 * 16 + i;
    uint4* hi = isv ? vt : k;
    uint4* lo = isv ? vt_lo : k_lo;
    const size_t so = (((size_t)layer * slots + src) * nh + head) * per_head + off;
    const size_t o = (((size_t)layer * slots + dst) * nh + head) * per_head + off;
    hi[o] = hi[so];
    if (lo) lo[o] = lo[so];
}

}  // namespace llark

using namespace llark;

extern "C" int llark_beam_topk_rows(const float* logits, int ldl, int vocab, int rows, int slots, const int* state, const int* slot_of_row,
                                    const float* score, int beams, float* cand_score, int* cand_token, float* cand_logprob, int* fallbacks,
                                    llark_stream_t stream) {
    LLARK_REQUIRE(logits && score && cand_score && cand_token && cand_logprob,
                  "beam_topk_rows: null pointer (logits, score, cand_score, cand_token, cand_logprob)");
    LLARK_REQUIRE(beams >= 1 && beams <= BEAM_MAX, "beam_topk_rows: beams=%d outside 1 .. %d", beams, BEAM_MAX);
    LLARK_REQUIRE(rows > 0 && slots > 0 && vocab >= 2 * beams && ldl >= vocab && (slot_of_row || rows <= slots),
                  "beam_topk_rows: bad shape rows=%d slots=%d vocab=%d (>= 2 beams = %d) ldl=%d", rows, slots, vocab, 2 * beams, ldl);
    BeamTopkArgs a;
    a.logits = logits, a.ldl = ldl, a.vocab = vocab, a.slots = slots, a.k = 2 * beams, a.state = state, a.slot_of_row = slot_of_row;
    a.score = score, a.cand_score = cand_score, a.cand_token = cand_token, a.cand_logprob = cand_logprob, a.fallbacks = fallbacks;
    a.ban = nullptr, a.ld_ban = 0;
    hipStream_t st = (hipStream_t)stream;
    if (vocab <= 4 * BEAM_THREADS) beam_topk_rows_kernel<4><<<rows, BEAM_THREADS, 0, st>>>(a);
    else if (vocab <= 32 * BEAM_THREADS) beam_topk_rows_kernel<32><<<rows, BEAM_THREADS, 0, st>>>(a);
    else beam_topk_rows_kernel<50><<<rows, BEAM_THREADS, 0, st>>>(a);
    return check_launch("beam_topk_rows");
}

extern "C" int llark_beam_topk_rows_banned(const float* logits, int ldl, int vocab, int rows, int slots, const int* state,
                                           const int* slot_of_row, const float* score, int beams, float* cand_score, int* cand_token,
                                           float* cand_logprob, int* fallbacks, const unsigned* ban, int ld_ban, llark_stream_t stream) {
    LLARK_REQUIRE(logits && score && cand_score && cand_token && cand_logprob && ban,
                  "beam_topk_rows_banned: null pointer (logits, score, cand_score, cand_token, cand_logprob, ban)");
    LLARK_REQUIRE(beams >= 1 && beams <= BEAM_MAX, "beam_topk_rows_banned: beams=%d outside 1 .. %d", beams, BEAM_MAX);
    LLARK_REQUIRE(rows > 0 && slots > 0 && vocab >= 2 * beams && ldl >= vocab && (slot_of_row || rows <= slots),
                  "beam_topk_rows_banned: bad shape rows=%d slots=%d vocab=%d (>= 2 beams = %d) ldl=%d", rows, slots, vocab, 2 * beams, ldl);
    LLARK_REQUIRE(ld_ban >= (vocab + 31) / 32, "beam_topk_rows_banned: ld_ban=%d below ceil(vocab / 32)=%d", ld_ban, (vocab + 31) / 32);
    BeamTopkArgs a;
    a.logits = logits, a.ldl = ldl, a.vocab = vocab, a.slots = slots, a.k = 2 * beams, a.state = state, a.slot_of_row = slot_of_row;
    a.score = score, a.cand_score = cand_score, a.cand_token = cand_token, a.cand_logprob = cand_logprob, a.fallbacks = fallbacks;
    a.ban = ban, a.ld_ban = ld_ban;
    hipStream_t st = (hipStream_t)stream;
    if (vocab <= 4 * BEAM_THREADS) beam_topk_rows_kernel<4, true><<<rows, BEAM_THREADS, 0, st>>>(a);
    else if (vocab <= 32 * BEAM_THREADS) beam_topk_rows_kernel<32, true><<<rows, BEAM_THREADS, 0, st>>>(a);
    else beam_topk_rows_kernel<50, true><<<rows, BEAM_THREADS, 0, st>>>(a);
    return check_launch("beam_topk_rows_banned");
}

static int beam_advance_launch(int open, const float* cand_score, const int* cand_token, const float* cand_logprob, int n_examples, int beams,
                               int step, int max_steps, int64_t eos, int64_t pad, float length_penalty, int early_stopping, float* score,
                               int* rank_of_slot, int* state, int* pos_rows, int* cur_len, int64_t* next_ids, int* heap, int* heap_meta,
                               int* done, int* trellis, int* pairs, int* pair_count, llark_stream_t stream) {
    LLARK_REQUIRE(cand_score && cand_token && cand_logprob && score && rank_of_slot && state && cur_len && next_ids && heap && heap_meta &&
                      done && trellis && pairs && pair_count,
                  "beam_advance: null pointer (only pos_rows may be null)");
    LLARK_REQUIRE(beams >= 1 && beams <= BEAM_MAX, "beam_advance: beams=%d outside 1 .. %d", beams, BEAM_MAX);
    LLARK_REQUIRE(n_examples >= 1 && n_examples <= 4096, "beam_advance: n_examples=%d outside 1 .. 4096", n_examples);
    LLARK_REQUIRE(step >= 0 && step < max_steps, "beam_advance: step=%d outside the trellis' %d rows", step, max_steps);
    LLARK_REQUIRE(length_penalty == length_penalty && fabsf(length_penalty) < INFINITY, "beam_advance: length_penalty must be finite");
    BeamAdvanceArgs a;
    a.cand_score = cand_score, a.cand_token = cand_token, a.cand_logprob = cand_logprob, a.beams = beams, a.step = step;
    a.eos = (long long)eos, a.pad = (long long)pad, a.length_penalty = length_penalty, a.early_stopping = early_stopping != 0;
    a.score = score, a.rank_of_slot = rank_of_slot, a.state = state, a.pos_rows = pos_rows, a.cur_len = cur_len;
    a.next_ids = (long long*)next_ids, a.heap = heap, a.heap_meta = heap_meta, a.done = done, a.trellis = trellis, a.pairs = pairs;
    a.pair_count = pair_count, a.open = open;
    beam_advance_kernel<<<n_examples, 64, 0, (hipStream_t)stream>>>(a);
    return check_launch("beam_advance");
}

extern "C" int llark_beam_advance(const float* cand_score, const int* cand_token, const float* cand_logprob, int n_examples, int beams,
                                  int step, int max_steps, int64_t eos, int64_t pad, float length_penalty, int early_stopping, float* score,
                                  int* rank_of_slot, int* state, int* pos_rows, int* cur_len, int64_t* next_ids, int* heap, int* heap_meta,
                                  int* done, int* trellis, int* pairs, int* pair_count, llark_stream_t stream) {
    return beam_advance_launch(0, cand_score, cand_token, cand_logprob, n_examples, beams, step, max_steps, eos, pad, length_penalty,
                               early_stopping, score, rank_of_slot, state, pos_rows, cur_len, next_ids, heap, heap_meta, done, trellis, pairs,
                               pair_count, stream);
}

extern "C" int llark_beam_advance_open(const float* cand_score, const int* cand_token, const float* cand_logprob, int n_examples, int beams,
                                       int step, int max_steps, int64_t eos, int64_t pad, float length_penalty, int early_stopping,
                                       float* score, int* rank_of_slot, int* state, int* pos_rows, int* cur_len, int64_t* next_ids, int* heap,
                                       int* heap_meta, int* done, int* trellis, int* pairs, int* pair_count, llark_stream_t stream) {
    return beam_advance_launch(1, cand_score, cand_token, cand_logprob, n_examples, beams, step, max_steps, eos, pad, length_penalty,
                               early_stopping, score, rank_of_slot, state, pos_rows, cur_len, next_ids, heap, heap_meta, done, trellis, pairs,
                               pair_count, stream);
}

extern "C" int llark_kv_copy_slots(void* k_cache, void* vt_cache, void* k_cache_lo, void* vt_cache_lo, int layers, int slots, int nh, int hd,
                                   int smax, const int* pairs, const int* count, int n_lists, int list_stride, const int* p0,
                                   const int* pos_rows, int max_span, llark_stream_t stream) {
    LLARK_REQUIRE(k_cache && vt_cache && pairs && count && p0 && pos_rows && (k_cache_lo == nullptr) == (vt_cache_lo == nullptr),
                  "kv_copy_slots: null pointer, or one lo plane only");
    LLARK_REQUIRE(layers > 0 && slots > 0 && nh > 0 && smax > 0 && (long)layers * nh <= 65535, "kv_copy_slots: bad shape layers=%d slots=%d nh=%d smax=%d",
                  layers, slots, nh, smax);
    LLARK_REQUIRE(hd == 128 && smax % 8 == 0, "kv_copy_slots: head_dim 128 and smax %% 8 == 0 required (hd=%d smax=%d)", hd, smax);
    LLARK_REQUIRE(n_lists >= 1 && list_stride >= 1 && (long)n_lists * list_stride <= 1024, "kv_copy_slots: %d lists of %d entries (1 .. 1024 in all)",
                  n_lists, list_stride);
    LLARK_REQUIRE(max_span >= 1 && max_span <= smax, "kv_copy_slots: max_span=%d outside 1 .. smax=%d", max_span, smax);
    const long chunks = (long)max_span * 16 + 128L * ((max_span + 7) / 8 + 1);
    kv_copy_slots_kernel<<<dim3(cdiv(chunks, 256), layers * nh, n_lists * list_stride), 256, 0, (hipStream_t)stream>>>(
        (uint4*)k_cache, (uint4*)vt_cache, (uint4*)k_cache_lo, (uint4*)vt_cache_lo, slots, nh, smax, pairs, count, list_stride, p0, pos_rows, max_span);
    return check_launch("kv_copy_slots");
}
