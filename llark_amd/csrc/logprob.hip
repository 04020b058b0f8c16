// Token log-probabilities on the device (llark_token_logprob_rows): log-softmax of a row of fp32 logits at one chosen token, plus the
// token's rank, one workgroup of 1024 threads per row; the per-slot history (hist / count / total) is appended in the same launch.
//
// Thread tid owns the columns tid, tid + 1024, tid + 2048, ...: every load of a wave is 64 consecutive floats (256 bytes), and which
// thread owns which column depends on the column alone -- not on the row's address, so a row gives the same bits at any alignment.
// The first NPT columns of a thread stay in registers between the two passes (maximum / rank / NaN, then the sum of exponentials), so a
// row of up to 1024 * NPT columns is read from memory once; the columns beyond (vocab > 51 200) are read a second time in the sum pass.
//
// Sums have a fixed order: per thread in column order, a butterfly over the lanes (both partners of a step add the same two numbers, so
// all lanes agree), the 16 wave sums in wave order.  Longest path: ceil(vocab / 1024) + 6 + 15 additions.  Every exponential is
// expf(l - M) with the row's exact maximum M: nothing is rescaled.  No workgroup waits for another, no atomics, only vector stores.
#include "common.h"

namespace llark {

constexpr int LOGPROB_THREADS = 1024;
constexpr int LOGPROB_WAVES = LOGPROB_THREADS / 64;

struct LogprobArgs {
    const float* logits;
    int ldl, vocab, slots;
    const int* state;
    const int* slot_of_row;
    const long long* tokens;
    float* logprob;
    int* rank;
    float* hist;
    int ld_hist;
    int* count;
    float* total;
};

template <int NPT>
__global__ __launch_bounds__(LOGPROB_THREADS) void token_logprob_rows_kernel(const LogprobArgs a) {
    __shared__ float smax[LOGPROB_WAVES];
    __shared__ int sgt[LOGPROB_WAVES];
    __shared__ int sbad[LOGPROB_WAVES];
    __shared__ float ssum[LOGPROB_WAVES];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int slot = a.slot_of_row ? a.slot_of_row[r] : r;
    if (slot < 0 || slot >= a.slots) return;                      // workgroup-uniform, like every return below
    if (a.state && a.state[slot] != LLARK_ROW_ACTIVE) return;
    const int vocab = a.vocab;
    const long long t = a.tokens[r];
    if (t < 0 || t >= vocab) return;
    const float* row = a.logits + (size_t)r * a.ldl;
    const float lt = row[t];

    // ---- pass 1: the row into registers; maximum, rank of the target, NaN flag ------------------------------------------------------
    float v[NPT];
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
        const int j = tid + LOGPROB_THREADS * i;
        v[i] = j < vocab ? row[j] : -INFINITY;
    }
    float m = -INFINITY;
    int gt = 0, bad = 0;
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
        m = fmaxf(m, v[i]);                                        // a NaN operand is ignored here and caught by `bad`
        gt += v[i] > lt ? 1 : 0;
        bad |= v[i] != v[i] ? 1 : 0;
    }
    for (long long j = (long long)NPT * LOGPROB_THREADS + tid; j < vocab; j += LOGPROB_THREADS) {
        const float x = row[j];
        m = fmaxf(m, x);
        gt += x > lt ? 1 : 0;
        bad |= x != x ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        m = fmaxf(m, __shfl_xor(m, o, 64));
        gt += __shfl_xor(gt, o, 64);
        bad |= __shfl_xor(bad, o, 64);
    }
    if (lane == 0) smax[wv] = m, sgt[wv] = gt, sbad[wv] = bad;
    __syncthreads();
    float M = smax[0];
    int n_gt = sgt[0], any_bad = sbad[0];
#pragma unroll
    for (int w = 1; w < LOGPROB_WAVES; ++w) M = fmaxf(M, smax[w]), n_gt += sgt[w], any_bad |= sbad[w];

    float lp;
    int rk;
    if (any_bad || !(fabsf(M) < INFINITY)) {                       // a NaN in the row, or a maximum of +-inf: no distribution
        lp = __uint_as_float(0x7fc00000u);
        rk = -1;
    } else {
        // ---- pass 2: S = sum of expf(l - M); a -inf logit (and a column beyond the vocabulary) adds exactly 0 ------------------------
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < NPT; ++i) s += expf(v[i] - M);
        for (long long j = (long long)NPT * LOGPROB_THREADS + tid; j < vocab; j += LOGPROB_THREADS) s += expf(row[j] - M);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) ssum[wv] = s;
        __syncthreads();
        float S = ssum[0];
#pragma unroll
        for (int w = 1; w < LOGPROB_WAVES; ++w) S += ssum[w];
        lp = (lt - M) - logf(S);
        rk = n_gt;
    }
    if (tid == 0) {
        a.logprob[r] = lp;
        if (a.rank) a.rank[r] = rk;
        if (a.count) {
            const int c = a.count[slot];
            if (a.hist && c >= 0 && c < a.ld_hist) a.hist[(size_t)slot * a.ld_hist + c] = lp;
            a.count[slot] = c + 1;
        }
        if (a.total) a.total[slot] += lp;
    }
}

}  // namespace llark

using namespace llark;

extern "C" int llark_token_logprob_rows(const float* logits, int ldl, int vocab, int rows, int slots, const int* state,
                                        const int* slot_of_row, const int64_t* tokens, float* logprob, int* rank, float* hist, int ld_hist,
                                        int* count, float* total, llark_stream_t stream) {
    LLARK_REQUIRE(logits && tokens && logprob, "token_logprob_rows: null pointer (logits, tokens, logprob)");
    LLARK_REQUIRE(rows > 0 && slots > 0 && vocab > 0 && ldl >= vocab && (slot_of_row || rows <= slots),
                  "token_logprob_rows: bad shape rows=%d slots=%d vocab=%d ldl=%d", rows, slots, vocab, ldl);
    LLARK_REQUIRE(!hist || (count && ld_hist > 0), "token_logprob_rows: hist needs count and ld_hist > 0, got ld_hist=%d", ld_hist);
    LogprobArgs a;
    a.logits = logits, a.ldl = ldl, a.vocab = vocab, a.slots = slots, a.state = state, a.slot_of_row = slot_of_row;
    a.tokens = (const long long*)tokens, a.logprob = logprob, a.rank = rank, a.hist = hist, a.ld_hist = ld_hist, a.count = count;
    a.total = total;
    hipStream_t st = (hipStream_t)stream;
    if (vocab <= 4 * LOGPROB_THREADS) token_logprob_rows_kernel<4><<<rows, LOGPROB_THREADS, 0, st>>>(a);
    else if (vocab <= 32 * LOGPROB_THREADS) token_logprob_rows_kernel<32><<<rows, LOGPROB_THREADS, 0, st>>>(a);
    else token_logprob_rows_kernel<50><<<rows, LOGPROB_THREADS, 0, st>>>(a);
    return check_launch("token_logprob_rows");
}
