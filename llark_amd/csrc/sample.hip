// Token sampling on the device (llark_sample_rows, llark_seen_mark_rows): repetition penalty -> temperature -> top-k -> top-p -> draw,
// in the processor order of HF 4.29.2 (RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper,
// then multinomial), one workgroup of 1024 threads per row of fp32 logits.
//
// The row lives in registers.  Wave w (16 waves) owns the 64 * NPT consecutive tokens from w * 64 * NPT on; its chunk i (i < NPT) is
// the 64 consecutive tokens from there + 64 i, one per lane, so every load is a coalesced 256-byte wave load and token order is
// (wave, chunk, lane).  A thread holds NPT order-preserving uint32 keys of its post-temperature logits and the NPT exponentials
// exp(l - max); at NPT = 64 (vocab up to 65 536) both do not fit the 128 registers a thread of a 1024-thread workgroup may use, so the
// last E_LDS exponentials of each thread live in LDS (conflict-free: [i][tid]).
//
// Every loop has a trip count fixed before it starts: the selections are bisections over the uint32 key, exactly 32 steps each, and a
// NaN or an infinity never reaches them (such a row falls back to the greedy rule before the first bisection).  No workgroup waits for
// another, no atomics between workgroups except the `fallbacks` counter (a plain vector atomic add), only vector stores.
//
// Sums have a fixed order -- per thread in chunk order, a butterfly over the lanes (both partners of a step add the same two numbers,
// so all lanes agree), the 16 wave sums in wave order -- hence they are bit-reproducible and, fp32 addition being monotone in each
// operand, monotone in the set of tokens that take part: the top-p bisection is well defined.
//
// top-p keeps token i iff the mass of the tokens with a strictly larger logit is short of p * Z.  Tokens with EQUAL logits are kept or
// dropped together: tokens exactly tied at the boundary are all kept, where HF's sort keeps an arbitrary subset of them.
#include "common.h"

namespace llark {

constexpr int SAMPLE_THREADS = 1024;
constexpr int SAMPLE_WAVES = SAMPLE_THREADS / 64;

struct SampleArgs {
    const float* logits;
    int ldl, vocab, slots;
    const int* state;
    const int* slot_of_row;
    unsigned* seen;
    int ld_seen;
    int do_sample;
    float temperature;
    int top_k;
    float top_p, penalty;
    const float* u;
    unsigned seed_lo, seed_hi;
    int* draws;
    const long long* stream_id;
    long long* choice;
    int* kept;
    float* thresh;
    int* fallbacks;
};

// same rule as decode_advance_rows_kernel (llama.hip): first maximal index, a NaN counts as the maximum (torch.argmax)
__device__ __forceinline__ bool sample_argmax_better(float v, int i, float bv, int bi) {
    const bool vn = v != v, bn = bv != bv;
    if (vn || bn) return vn && (!bn || i < bi);
    return v > bv || (v == bv && i < bi);
}

// order-preserving image of a non-NaN float: a < b  <=>  key(a) < key(b); -inf -> 0x007fffff, so 0 lies below every float
__device__ __forceinline__ unsigned sample_key(float x) {
    const unsigned b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float sample_unkey(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// Philox4x32-10 (Salmon et al., SC'11), first output word
__device__ __forceinline__ unsigned philox4x32_10_word0(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

__device__ __forceinline__ float block_sum_f(float x, float (*buf)[SAMPLE_WAVES], int& parity) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    if ((threadIdx.x & 63) == 0) buf[parity][threadIdx.x >> 6] = x;
    __syncthreads();
    float s = buf[parity][0];
#pragma unroll
    for (int w = 1; w < SAMPLE_WAVES; ++w) s += buf[parity][w];
    parity ^= 1;
    return s;
}
__device__ __forceinline__ int block_sum_i(int x, int (*buf)[SAMPLE_WAVES], int& parity) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    if ((threadIdx.x & 63) == 0) buf[parity][threadIdx.x >> 6] = x;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int w = 0; w < SAMPLE_WAVES; ++w) s += buf[parity][w];
    parity ^= 1;
    return s;
}
__device__ __forceinline__ unsigned block_min_u(unsigned x, int (*buf)[SAMPLE_WAVES], int& parity) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = min(x, (unsigned)__shfl_xor((int)x, o, 64));
    if ((threadIdx.x & 63) == 0) buf[parity][threadIdx.x >> 6] = (int)x;
    __syncthreads();
    unsigned s = 0xffffffffu;
#pragma unroll
    for (int w = 0; w < SAMPLE_WAVES; ++w) s = min(s, (unsigned)buf[parity][w]);
    parity ^= 1;
    return s;
}
// inclusive scan over the 64 lanes, fixed order
__device__ __forceinline__ float wave_scan_incl(float x, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float t = __shfl_up(x, o, 64);
        if (lane >= o) x += t;
    }
    return x;
}

// The per-chunk loops are fully unrolled (register arrays need constant indices); left alone, the scheduler hoists every LDS read
// and every load of such a loop to its top and spills.  A scheduling fence every 8 chunks keeps at most 8 in flight.
#define SAMPLE_FENCE(i)                                          \
    do {                                                         \
        if (((i) & 7) == 7) __builtin_amdgcn_sched_barrier(0);   \
    } while (0)

template <int NPT, int E_LDS>
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_rows_kernel(const SampleArgs a) {
    constexpr int E_REG = NPT - E_LDS;
    extern __shared__ float e_lds[];                              // [E_LDS][1024]
    __shared__ float sf[2][SAMPLE_WAVES];
    __shared__ int si[2][SAMPLE_WAVES];
    __shared__ float sbv[SAMPLE_WAVES];
    __shared__ int sbi[SAMPLE_WAVES];
    __shared__ float swave[SAMPLE_WAVES];
    __shared__ int stok;
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int slot = a.slot_of_row ? a.slot_of_row[r] : r;
    if (slot < 0 || slot >= a.slots) return;                      // workgroup-uniform
    if (a.state && a.state[slot] != LLARK_ROW_ACTIVE) return;
    const int vocab = a.vocab;
    const float* row = a.logits + (size_t)r * a.ldl;
    unsigned* seen_row = a.seen ? a.seen + (size_t)slot * a.ld_seen : nullptr;
    const int j0 = wv * (64 * NPT) + lane;                        // token of chunk i: j0 + 64 i
    int parf = 0, pari = 0;

    // ---- load, repetition penalty, greedy token of the penalised row -------------------------------------------------------------
    float v[NPT];
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
        const int j = j0 + 64 * i;
        v[i] = j < vocab ? row[j] : -INFINITY;
    }
    if (a.penalty != 1.0f) {
        const float th = a.penalty;
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            const int j = j0 + 64 * i;
            if (j < vocab && ((seen_row[j >> 5] >> (j & 31)) & 1u)) v[i] = v[i] < 0.0f ? v[i] * th : v[i] / th;
            SAMPLE_FENCE(i);
        }
    }
    float bv = -INFINITY;
    int bi = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
        const int j = j0 + 64 * i;
        if (j < vocab && sample_argmax_better(v[i], j, bv, bi)) bv = v[i], bi = j;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (sample_argmax_better(ov, oi, bv, bi)) bv = ov, bi = oi;
    }
    if (lane == 0) sbv[wv] = bv, sbi[wv] = bi;
    __syncthreads();
    bv = sbv[0], bi = sbi[0];
#pragma unroll
    for (int w = 1; w < SAMPLE_WAVES; ++w)
        if (sample_argmax_better(sbv[w], sbi[w], bv, bi)) bv = sbv[w], bi = sbi[w];
    const int greedy = min(max(bi, 0), vocab - 1);                // vocab >= 1: token 0 is valid, so bi is already in range

    int tok = greedy;
    bool fell_back = false;
    int n_kept = 0;
    float th_out = __uint_as_float(0x7fc00000u);
    if (a.do_sample) {
        const float T = a.temperature;
        const float m = (bv / T) + 0.0f;                           // division is monotone: the maximum of l / T
        if (bv != bv || !(fabsf(m) < INFINITY)) {
            fell_back = true;                                      // NaN in the row, all -inf, or a +inf: the greedy rule
        } else {
            // ---- temperature, exponentials, keys ---------------------------------------------------------------------------------
            unsigned key[NPT];
            float e[E_REG > 0 ? E_REG : 1];
#pragma unroll
            for (int i = 0; i < NPT; ++i) {
                const int j = j0 + 64 * i;
                const float l = (v[i] / T) + 0.0f;                 // + 0: -0 becomes +0, the key order is the float order
                const float ex = expf(l - m);                       // beyond the vocabulary l = -inf: exactly 0
                key[i] = j < vocab ? sample_key(l) : 0u;
                if (i < E_REG) e[i] = ex;
                else e_lds[(i - E_REG) * SAMPLE_THREADS + tid] = ex;
                __builtin_amdgcn_sched_barrier(0);                 // one chunk at a time: l dies as its key is born
            }
#define E_AT(i) ((i) < E_REG ? e[(i) < E_REG ? (i) : 0] : e_lds[((i) - E_REG) * SAMPLE_THREADS + tid])
            unsigned x_keep = 1u;                                  // a token is kept iff key >= x_keep (0 = beyond the vocabulary)
            // ---- top-k: the largest x with count(key >= x) >= k, i.e. the key of the k-th largest logit; ties all kept ------------
            if (a.top_k > 0) {
                const int k = min(max(a.top_k, 1), vocab);
                unsigned y = 0u;
#pragma unroll 1
                for (int bit = 31; bit >= 0; --bit) {
                    const unsigned c = y | (1u << bit);
                    int cnt = 0;
#pragma unroll
                    for (int i = 0; i < NPT; ++i) cnt += key[i] >= c ? 1 : 0;
                    if (block_sum_i(cnt, si, pari) >= k) y = c;
                }
                x_keep = y;
            }
            // ---- top-p over the top-k set: the largest y with mass(key > y) >= p Z; kept iff key > y -------------------------------
            if (a.top_p < 1.0f) {
                float s = 0.0f;
#pragma unroll
                for (int i = 0; i < NPT; ++i) {
                    s += key[i] >= x_keep ? E_AT(i) : 0.0f;
                    SAMPLE_FENCE(i);
                }
                const float Z = block_sum_f(s, sf, parf);
                const float pz = a.top_p * Z;
                unsigned y = 0u;
#pragma unroll 1
                for (int bit = 31; bit >= 0; --bit) {
                    const unsigned c = y | (1u << bit);
                    float sa = 0.0f;
#pragma unroll
                    for (int i = 0; i < NPT; ++i) {
                        sa += (key[i] > c && key[i] >= x_keep) ? E_AT(i) : 0.0f;
                        SAMPLE_FENCE(i);
                    }
                    if (block_sum_f(sa, sf, parf) >= pz) y = c;
                }
                if (y != 0xffffffffu) x_keep = max(x_keep, y + 1u);
            }
            // ---- the kept set: its size and its smallest logit -------------------------------------------------------------------
            {
                int cnt = 0;
                unsigned mn = 0xffffffffu;
#pragma unroll
                for (int i = 0; i < NPT; ++i)
                    if (key[i] >= x_keep) ++cnt, mn = min(mn, key[i]);
                n_kept = block_sum_i(cnt, si, pari);
                th_out = sample_unkey(block_min_u(mn, si, pari));
            }
            // ---- draw: cumulative kept mass in token order = wave base + (sum of the wave's earlier chunks + scan inside the chunk) --
            float run = 0.0f;
#pragma unroll
            for (int i = 0; i < NPT; ++i) {
                const float sc = wave_scan_incl(key[i] >= x_keep ? E_AT(i) : 0.0f, lane);
                run += __shfl(sc, 63, 64);
                SAMPLE_FENCE(i);
            }
            if (lane == 0) swave[wv] = run;
            __syncthreads();
            float base = 0.0f, zk = 0.0f;
#pragma unroll
            for (int w = 0; w < SAMPLE_WAVES; ++w) {
                if (w == wv) base = zk;
                zk += swave[w];
            }
            if (!(zk > 0.0f && zk < INFINITY)) {
                fell_back = true;
            } else {
                float uu;
                if (a.u) {
                    uu = a.u[r];
                } else {
                    const unsigned long long sid = a.stream_id ? (unsigned long long)a.stream_id[slot] : (unsigned long long)slot;
                    const unsigned w0 = philox4x32_10_word0((unsigned)a.draws[slot], 0u, (unsigned)sid, (unsigned)(sid >> 32), a.seed_lo, a.seed_hi);
                    uu = (float)(w0 >> 8) * 0x1p-24f;
                }
                const float target = uu * zk;
                if (tid == 0) stok = greedy;                       // target >= zk (u >= 1): the maximum, which every kept set holds
                __syncthreads();
                // the first wave whose end exceeds the target holds the token; base <= target there
                if (base + run > target && !(base > target)) {
                    float part = 0.0f;
                    bool found = false;
#pragma unroll
                    for (int i = 0; i < NPT; ++i) {
                        const float sc = wave_scan_incl(key[i] >= x_keep ? E_AT(i) : 0.0f, lane);
                        const unsigned long long hit = __ballot(!found && base + (part + sc) > target);
                        if (hit != 0ull) {
                            if (lane == 0) stok = j0 + 64 * i + (int)__builtin_ctzll(hit);
                            found = true;
                        }
                        part += __shfl(sc, 63, 64);
                        SAMPLE_FENCE(i);
                    }
                }
                __syncthreads();
                tok = min(max(stok, 0), vocab - 1);
            }
#undef E_AT
        }
        if (fell_back) tok = greedy;
    }
    if (tid == 0) {
        a.choice[r] = tok;
        if (seen_row) seen_row[tok >> 5] |= 1u << (tok & 31);
        if (a.do_sample) {
            if (a.draws) a.draws[slot] += 1;
            if (a.kept) a.kept[r] = fell_back ? 0 : n_kept;
            if (a.thresh) a.thresh[r] = th_out;
            if (fell_back && a.fallbacks) atomicAdd(a.fallbacks, 1);
        }
    }
}

__global__ __launch_bounds__(256) void seen_mark_rows_kernel(const long long* __restrict__ ids, long long n_ids, const int* __restrict__ offs,
                                                             const int* __restrict__ lens, const int* __restrict__ slot_of_row, int slots,
                                                             int vocab, unsigned* seen, int ld_seen) {
    const int r = blockIdx.x;
    const int slot = slot_of_row ? slot_of_row[r] : r;
    const long long off = offs[r];
    const int len = lens[r];
    if (slot < 0 || slot >= slots || off < 0 || len <= 0 || off + len > n_ids) return;
    unsigned* row = seen + (size_t)slot * ld_seen;
    for (int t = threadIdx.x; t < len; t += 256) {
        const long long id = ids[off + t];
        if (id >= 0 && id < vocab) atomicOr(&row[id >> 5], 1u << (id & 31));
    }
}

}  // namespace llark

using namespace llark;

extern "C" int llark_sample_rows(const float* logits, int ldl, int vocab, int rows, int slots, const int* state, const int* slot_of_row,
                                 unsigned* seen, int ld_seen, int do_sample, float temperature, int top_k, float top_p,
                                 float repetition_penalty, const float* u, long long seed, int* draws, const int64_t* stream_id,
                                 int64_t* choice, int* kept, float* thresh, int* fallbacks, llark_stream_t stream) {
    LLARK_REQUIRE(logits && choice, "sample_rows: null pointer (logits, choice)");
    LLARK_REQUIRE(rows > 0 && slots > 0 && vocab > 0 && ldl >= vocab && (slot_of_row || rows <= slots),
                  "sample_rows: bad shape rows=%d slots=%d vocab=%d ldl=%d", rows, slots, vocab, ldl);
    LLARK_REQUIRE(repetition_penalty > 0.0f, "sample_rows: repetition_penalty must be > 0, got %g", (double)repetition_penalty);
    LLARK_REQUIRE(seen || repetition_penalty == 1.0f, "sample_rows: a repetition penalty needs the seen bitmap");
    LLARK_REQUIRE(!seen || ld_seen >= (vocab + 31) / 32, "sample_rows: ld_seen %d holds fewer than vocab %d bits", ld_seen, vocab);
    if (do_sample) {
        LLARK_REQUIRE(temperature > 0.0f && temperature < INFINITY, "sample_rows: temperature must be > 0, got %g", (double)temperature);
        LLARK_REQUIRE(top_p > 0.0f && top_p <= 1.0f, "sample_rows: top_p must be in (0, 1], got %g", (double)top_p);
        LLARK_REQUIRE(top_k >= 0, "sample_rows: top_k must be >= 0, got %d", top_k);
        LLARK_REQUIRE(u || draws, "sample_rows: sampling needs u or the draw counters");
    }
    if (vocab > 65536) {
        set_error("sample_rows: vocab %d above 65536", vocab);
        return LLARK_ERR_UNSUPPORTED;
    }
    SampleArgs a;
    a.logits = logits, a.ldl = ldl, a.vocab = vocab, a.slots = slots, a.state = state, a.slot_of_row = slot_of_row;
    a.seen = seen, a.ld_seen = ld_seen, a.do_sample = do_sample != 0, a.temperature = temperature, a.top_k = top_k, a.top_p = top_p;
    a.penalty = repetition_penalty, a.u = u, a.seed_lo = (unsigned)(unsigned long long)seed, a.seed_hi = (unsigned)((unsigned long long)seed >> 32);
    a.draws = draws, a.stream_id = (const long long*)stream_id, a.choice = (long long*)choice, a.kept = kept, a.thresh = thresh;
    a.fallbacks = fallbacks;
    hipStream_t st = (hipStream_t)stream;
    if (vocab <= 4096) {
        sample_rows_kernel<4, 0><<<rows, SAMPLE_THREADS, 0, st>>>(a);
    } else if (vocab <= 32768) {
        sample_rows_kernel<32, 0><<<rows, SAMPLE_THREADS, 0, st>>>(a);
    } else {
        constexpr int lds = 36 * SAMPLE_THREADS * (int)sizeof(float);
        static PerDeviceOnce once;
        if (once.first()) {
            (void)hipFuncSetAttribute((const void*)sample_rows_kernel<50, 36>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
            (void)hipFuncSetAttribute((const void*)sample_rows_kernel<64, 36>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        }
        if (vocab <= 50 * SAMPLE_THREADS) sample_rows_kernel<50, 36><<<rows, SAMPLE_THREADS, lds, st>>>(a);
        else sample_rows_kernel<64, 36><<<rows, SAMPLE_THREADS, lds, st>>>(a);
    }
    return check_launch("sample_rows");
}

extern "C" int llark_seen_mark_rows(const int64_t* ids, long long n_ids, const int* offs, const int* lens, const int* slot_of_row, int rows,
                                    int slots, int vocab, unsigned* seen, int ld_seen, llark_stream_t stream) {
    LLARK_REQUIRE(ids && offs && lens && seen, "seen_mark_rows: null pointer");
    LLARK_REQUIRE(rows > 0 && slots > 0 && vocab > 0 && n_ids >= 0 && ld_seen >= (vocab + 31) / 32 && (slot_of_row || rows <= slots),
                  "seen_mark_rows: bad shape rows=%d slots=%d vocab=%d ld_seen=%d", rows, slots, vocab, ld_seen);
    seen_mark_rows_kernel<<<rows, 256, 0, (hipStream_t)stream>>>((const long long*)ids, n_ids, offs, lens, slot_of_row, slots, vocab, seen,
                                                                  ld_seen);
    return check_launch("seen_mark_rows");
}
