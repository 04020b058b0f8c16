// Constrained decoding on the device (llark_constrain_rows): a row's token history plus the static lists become the set of tokens that
// are banned for the next choice -- HF 4.29.2's NoRepeatNGram, NoBadWords, MinLength and MinNewTokensLength processors -- in one launch
// per step, one workgroup of 1024 threads per row.  Contract: include/llark_hip.h.
//
// The history lives in device memory (hist / hist_len / prompt_len per slot) and is brought up to date by the same launch: a beam that
// forked takes its parent's row, then the token the row's logits were computed from is appended.  Every position below the old length L
// is READ from the parent's row (the slot's own row without a fork) and position L from the register that holds the appended token, so
// nothing a thread reads was written during this launch by anyone.  The bans are bits of an LDS bitmap (ceil(vocab / 32) words, vocab <=
// 65536) set with LDS atomicOr; the row is then streamed once: raw bits where the bit is clear, -inf where it is set.
//
// No workgroup waits for another; plain C++ and vector stores; no global atomics.
#include "common.h"

namespace llark {

constexpr int CONSTRAIN_THREADS = 1024;
constexpr int CONSTRAIN_WAVES = CONSTRAIN_THREADS / 64;
constexpr int CONSTRAIN_MAX_VOCAB = 65536;
constexpr int CONSTRAIN_MAX_NGRAM = 64;
constexpr int CONSTRAIN_MAX_WORDS = 4096;                         // words in the table
constexpr int CONSTRAIN_MAX_WORD_TOKENS = 1 << 20;                // tokens in the table, all words together

struct ConstrainArgs {
    const float* logits;
    int ldl, vocab, slots;
    const int* state;
    const int* slot_of_row;
    int* hist;
    int ld_hist;
    int* hist_len;
    const int* prompt_len;
    const int* parent;
    int parent_stride;
    const long long* last_token;
    int ngram;
    const int* bw_tokens;
    const int* bw_off;
    int n_words, bw_total;
    long long eos;
    int min_new, min_len;
    float* out;
    int ldo;
    unsigned* ban;
    int ld_ban;
    int* n_banned;
    int* status;
};

__global__ __launch_bounds__(CONSTRAIN_THREADS) void constrain_rows_kernel(const ConstrainArgs a) {
    __shared__ unsigned bm[CONSTRAIN_MAX_VOCAB / 32];
    __shared__ int tail[CONSTRAIN_MAX_NGRAM];
    __shared__ int scount[CONSTRAIN_WAVES];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int slot = a.slot_of_row ? a.slot_of_row[r] : r;
    if (slot < 0 || slot >= a.slots) return;                      // workgroup-uniform, like every return below
    if (a.state && a.state[slot] != LLARK_ROW_ACTIVE) return;
    const int vocab = a.vocab, words = (vocab + 31) >> 5, ld = a.ld_hist;

    // ---- history: fork, append --------------------------------------------------------------------------------------------------------
    int L = 0, L1 = 0, lastv = -1;                                // L: length before this launch, L1: after the append
    const int* hsrc = nullptr;                                    // positions [0, L)
    if (a.hist) {
        int* own = a.hist + (size_t)slot * ld;
        L = a.hist_len[slot];
        L = L < 0 ? 0 : (L > ld ? ld : L);
        int p = a.parent ? a.parent[(size_t)slot * a.parent_stride] : slot;
        if (p < 0 || p >= a.slots) p = slot;                      // an empty trellis entry: no fork
        hsrc = a.hist + (size_t)p * ld;
        if (p != slot)
            for (int i = tid; i < L; i += CONSTRAIN_THREADS) own[i] = hsrc[i];
        L1 = L;
        if (a.last_token) {
            const long long t = a.last_token[slot];
            lastv = (t < 0 || t > 0x7fffffffLL) ? -1 : (int)t;    // an id no vocabulary holds: compares, never indexes
            if (L < ld) {
                L1 = L + 1;
                if (tid == 0) own[L] = lastv;
            } else if (tid == 0 && a.status) {
                *a.status = *a.status | 1;                        // the row is full: nothing appended; every writer stores the same bit
            }
        }
        if (tid == 0) a.hist_len[slot] = L1;
    }
#define HIST_AT(i) ((i) < L ? hsrc[(i)] : lastv)

    // ---- bans -------------------------------------------------------------------------------------------------------------------------
    for (int w = tid; w < words; w += CONSTRAIN_THREADS) bm[w] = 0u;
    const int n = a.ngram;
    const bool scan = n > 0 && L1 + 1 >= n;
    if (scan && tid < n - 1) tail[tid] = HIST_AT(L1 - n + 1 + tid);
    __syncthreads();
    if (scan) {
        for (int i = tid; i <= L1 - n; i += CONSTRAIN_THREADS) {
            bool same = true;
            for (int j = 0; j < n - 1 && same; ++j) same = HIST_AT(i + j) == tail[j];
            if (same) {
                const int x = HIST_AT(i + n - 1);
                if (x >= 0 && x < vocab) atomicOr(&bm[x >> 5], 1u << (x & 31));
            }
        }
    }
    for (int w = tid; w < a.n_words; w += CONSTRAIN_THREADS) {
        const int o0 = a.bw_off[w], o1 = a.bw_off[w + 1], k = o1 - o0;
        if (o0 < 0 || k < 1 || o1 > a.bw_total || k - 1 > L1) continue;
        bool same = true;
        for (int j = 0; j < k - 1 && same; ++j) same = HIST_AT(L1 - k + 1 + j) == a.bw_tokens[o0 + j];
        if (same) {
            const int x = a.bw_tokens[o1 - 1];
            if (x >= 0 && x < vocab) atomicOr(&bm[x >> 5], 1u << (x & 31));
        }
    }
    if (tid == 0 && a.eos >= 0 && a.eos < vocab) {
        const int pl = a.prompt_len ? a.prompt_len[slot] : 0;
        if (L1 - pl < a.min_new || L1 < a.min_len) atomicOr(&bm[a.eos >> 5], 1u << (a.eos & 31));
    }
#undef HIST_AT
    __syncthreads();

    // ---- outputs ----------------------------------------------------------------------------------------------------------------------
    if (a.ban || a.n_banned) {
        int c = 0;
        unsigned* bo = a.ban ? a.ban + (size_t)slot * a.ld_ban : nullptr;
        for (int w = tid; w < words; w += CONSTRAIN_THREADS) {
            const unsigned b = bm[w];
            c += __popc(b);
            if (bo) bo[w] = b;
        }
        if (a.n_banned) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
            if (lane == 0) scount[wv] = c;
            __syncthreads();
            if (tid == 0) {
                int s = 0;
                for (int w = 0; w < CONSTRAIN_WAVES; ++w) s += scount[w];
                a.n_banned[r] = s;
            }
        }
    }
    if (a.out) {
        const unsigned NEG = 0xff800000u;                         // -inf
        const unsigned* src = (const unsigned*)(a.logits + (size_t)r * a.ldl);
        unsigned* dst = (unsigned*)(a.out + (size_t)r * a.ldo);
        const bool vec = ((((size_t)src) | ((size_t)dst)) & 15) == 0;     // workgroup-uniform
        int done = 0;
        if (vec) {
            const int quads = vocab >> 2;
            for (int q = tid; q < quads; q += CONSTRAIN_THREADS) {
                uint4 v = ((const uint4*)src)[q];
                const unsigned b = bm[q >> 3] >> ((q & 7) * 4);   // the four columns of a quad share a bitmap word
                if (b & 1u) v.x = NEG;
                if (b & 2u) v.y = NEG;
                if (b & 4u) v.z = NEG;
                if (b & 8u) v.w = NEG;
                ((uint4*)dst)[q] = v;
            }
            done = quads << 2;
        }
        for (int j = done + tid; j < vocab; j += CONSTRAIN_THREADS) dst[j] = ((bm[j >> 5] >> (j & 31)) & 1u) ? NEG : src[j];
    }
}

}  // namespace llark

using namespace llark;

extern "C" int llark_constrain_rows(const float* logits, int ldl, int vocab, int rows, int slots, const int* state, const int* slot_of_row,
                                    int* hist, int ld_hist, int* hist_len, const int* prompt_len, const int* parent, int parent_stride,
                                    const int64_t* last_token, int no_repeat_ngram, const int* bw_tokens, const int* bw_off, int n_words,
                                    int bw_total, int64_t eos, int min_new_tokens, int min_length, float* out, int ldo, unsigned* ban,
                                    int ld_ban, int* n_banned, int* status, llark_stream_t stream) {
    LLARK_REQUIRE(logits && (out || ban || n_banned), "constrain_rows: null pointer (logits; one of out, ban, n_banned)");
    LLARK_REQUIRE(rows > 0 && slots > 0 && vocab > 0 && ldl >= vocab && (slot_of_row || rows <= slots),
                  "constrain_rows: bad shape rows=%d slots=%d vocab=%d ldl=%d", rows, slots, vocab, ldl);
    LLARK_REQUIRE((hist == nullptr) == (hist_len == nullptr) && (!hist || ld_hist > 0),
                  "constrain_rows: hist and hist_len come together, with ld_hist > 0 (got ld_hist=%d)", ld_hist);
    LLARK_REQUIRE(hist || (!parent && !last_token && !prompt_len), "constrain_rows: parent / last_token / prompt_len without hist");
    LLARK_REQUIRE(!parent || parent_stride >= 1, "constrain_rows: parent_stride=%d must be >= 1", parent_stride);
    LLARK_REQUIRE(no_repeat_ngram >= 0 && no_repeat_ngram <= CONSTRAIN_MAX_NGRAM, "constrain_rows: no_repeat_ngram=%d outside 0 .. %d",
                  no_repeat_ngram, CONSTRAIN_MAX_NGRAM);
    LLARK_REQUIRE(no_repeat_ngram == 0 || hist, "constrain_rows: no_repeat_ngram=%d without hist", no_repeat_ngram);
    LLARK_REQUIRE(n_words >= 0 && n_words <= CONSTRAIN_MAX_WORDS && bw_total >= n_words && bw_total <= CONSTRAIN_MAX_WORD_TOKENS,
                  "constrain_rows: word table of %d words / %d tokens outside the caps (%d words, %d tokens, no empty word)", n_words,
                  bw_total, CONSTRAIN_MAX_WORDS, CONSTRAIN_MAX_WORD_TOKENS);
    LLARK_REQUIRE(n_words == 0 || (bw_tokens && bw_off), "constrain_rows: %d words without bw_tokens / bw_off", n_words);
    LLARK_REQUIRE(min_new_tokens >= 0 && min_length >= 0, "constrain_rows: min_new_tokens=%d / min_length=%d negative", min_new_tokens,
                  min_length);
    LLARK_REQUIRE(!out || ldo >= vocab, "constrain_rows: ldo=%d below vocab=%d", ldo, vocab);
    LLARK_REQUIRE(!ban || ld_ban >= (vocab + 31) / 32, "constrain_rows: ld_ban=%d below ceil(vocab / 32)=%d", ld_ban, (vocab + 31) / 32);
    if (vocab > CONSTRAIN_MAX_VOCAB) {
        set_error("constrain_rows: vocab %d above %d", vocab, CONSTRAIN_MAX_VOCAB);
        return LLARK_ERR_UNSUPPORTED;
    }
    ConstrainArgs a;
    a.logits = logits, a.ldl = ldl, a.vocab = vocab, a.slots = slots, a.state = state, a.slot_of_row = slot_of_row;
    a.hist = hist, a.ld_hist = ld_hist, a.hist_len = hist_len, a.prompt_len = prompt_len, a.parent = parent, a.parent_stride = parent_stride;
    a.last_token = (const long long*)last_token, a.ngram = no_repeat_ngram, a.bw_tokens = bw_tokens, a.bw_off = bw_off, a.n_words = n_words;
    a.bw_total = bw_total, a.eos = (long long)eos, a.min_new = min_new_tokens, a.min_len = min_length, a.out = out, a.ldo = ldo, a.ban = ban;
    a.ld_ban = ld_ban, a.n_banned = n_banned, a.status = status;
    constrain_rows_kernel<<<rows, CONSTRAIN_THREADS, 0, (hipStream_t)stream>>>(a);
    return check_launch("constrain_rows");
}
