// LoRA adapters on a frozen base: the low-rank products and the operand refresh (include/llark_hip.h, "LoRA adapters").
// peft LoraLayer (m2t/train.py:85-92): y = W x + (alpha / r) B (A x).  T = x A^T and dT = dY (sB) contract a wide bf16 operand down
// to rp = 64 .. 256 columns; dB = s dY^T T and dA^T = x^T dT contract over the tokens into a [wide][rp] fp32 gradient.  All four
// read their wide operand once and do 64 .. 256 flops per byte of it: memory-bound, so the tiles are small (32 rows) and the
// contraction is split over the waves of a workgroup (and, for the token contraction, over workgroups) to put every CU to work.
// MFMA: v_mfma_f32_32x32x16_bf16 -- lane l (r = l & 31, h = l >> 5) holds A[row r][k = 8 h + j] and B[k = 8 h + j][col r], j = 0 .. 7;
// result col = l & 31, row = (reg & 3) + 8 (reg >> 2) + 4 h.
#include "common.h"

namespace llark {

typedef unsigned short u16x8_t __attribute__((ext_vector_type(8)));

constexpr int LORA_WAVES = 4;

__device__ __forceinline__ f32x16_t lora_mfma(bf16x8_t a, bf16x8_t b, f32x16_t c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// part[wave][row][col] <- the wave's two 32x32 accumulators (columns 0..31 and 32..63)
__device__ __forceinline__ void lora_spill(float (*part)[65], const f32x16_t& acc0, const f32x16_t& acc1, int lane) {
    const int col = lane & 31, h = lane >> 5;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int row = (reg & 3) + 8 * (reg >> 2) + 4 * h;
        part[row][col] = acc0[reg];
        part[row][col + 32] = acc1[reg];
    }
}

// ---- out[rows][64 per blockIdx.y] = x . m^T ------------------------------------------------------------------------------------
// grid (ceil(rows / 32), rp_total / 64).  A lane's MFMA fragment is 16 bytes of one of 32 rows, so one load instruction touches 32
// cache lines and uses 32 bytes of each: wave w therefore owns whole 64-wide k chunks (w, w + 4, ...: the 128 bytes of a line) and
// issues a chunk's four k steps back to back -- the three later ones find the line in L1 / in flight instead of fetching it again
// from L2 for another wave.  Two chunks (24 loads) are issued before the first MFMA.  Partials meet in LDS; 256 threads write the
// 32 x 64 bf16 tile, 16 bytes each.  With fewer tiles than CUs (rp_total = 64 at 4096 rows: 128) the host also splits k over
// gridDim.z workgroups per tile, whose fp32 sums meet in a second small launch (lora_down_finish_kernel).  (Staging both tiles through LDS with row-contiguous loads measured 3 x slower: DESIGN.md 6b.)
__global__ __launch_bounds__(256) void lora_down_kernel(const bf16_t* __restrict__ x, int lda, const bf16_t* __restrict__ m, int ldm,
                                                        int rows, int k, bf16_t* __restrict__ out, int ldo,
                                                        float* __restrict__ partial, int rp_total) {
    // ``partial`` != nullptr: blockIdx.z owns k columns [z k, (z + 1) k) and leaves its fp32 sums in partial[z][rows][rp_total]
    __shared__ float part[LORA_WAVES][32][65];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int row0 = blockIdx.x * 32, n0 = blockIdx.y * 64;
    const int xr = min(row0 + r, rows - 1);                       // rows past the end re-read the last one; they are never stored
    const size_t k0 = (size_t)blockIdx.z * k;
    const bf16_t* xp = x + (size_t)xr * lda + k0 + 8 * h;
    const bf16_t* m0 = m + (size_t)(n0 + r) * ldm + k0 + 8 * h;
    const bf16_t* m1 = m0 + (size_t)32 * ldm;
    f32x16_t acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc0[i] = acc1[i] = 0.0f;
    const int steps = k >> 4;
    bf16x8_t zero;
#pragma unroll
    for (int j = 0; j < 8; ++j) zero[j] = (bf16_t)0.0f;
    for (int c = wv; 4 * c < steps; c += 2 * LORA_WAVES) {         // chunks c and c + 4 of this wave
        bf16x8_t a[8], b0[8], b1[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int s = 4 * (c + (u >> 2) * LORA_WAVES) + (u & 3);
            const int ko = s << 4;
            const bool ok = s < steps;                              // a step past the end loads nothing and adds zeros
            a[u] = ok ? *(const bf16x8_t*)(xp + ko) : zero;
            b0[u] = ok ? *(const bf16x8_t*)(m0 + ko) : zero;
            b1[u] = ok ? *(const bf16x8_t*)(m1 + ko) : zero;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            acc0 = lora_mfma(a[u], b0[u], acc0);
            acc1 = lora_mfma(a[u], b1[u], acc1);
        }
    }
    lora_spill(part[wv], acc0, acc1, lane);
    __syncthreads();
    const int row = threadIdx.x >> 3, c8 = (threadIdx.x & 7) * 8;
    if (row0 + row < rows) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (part[0][row][c8 + j] + part[1][row][c8 + j]) + (part[2][row][c8 + j] + part[3][row][c8 + j]);
        if (partial != nullptr) {
            float* dst = partial + ((size_t)blockIdx.z * rows + row0 + row) * rp_total + n0 + c8;
            *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
            *(float4*)(dst + 4) = make_float4(v[4], v[5], v[6], v[7]);
        } else {
            bf16x8_t o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (bf16_t)v[j];
            *(bf16x8_t*)(out + (size_t)(row0 + row) * ldo + n0 + c8) = o;
        }
    }
}

// out <- bf16(sum over the k splits, fixed order): one thread per 8 output columns
__global__ __launch_bounds__(256) void lora_down_finish_kernel(const float* __restrict__ partial, int nsplit, int rows, int rp_total,
                                                               bf16_t* __restrict__ out, int ldo) {
    const long long i8 = (long long)blockIdx.x * 256 + threadIdx.x;
    const int per_row = rp_total >> 3;
    if (i8 >= (long long)rows * per_row) return;
    const int row = (int)(i8 / per_row), c8 = (int)(i8 % per_row) * 8;
    const size_t stride = (size_t)rows * rp_total;
    const float* p = partial + (size_t)row * rp_total + c8;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = p[j];
    for (int s = 1; s < nsplit; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += p[s * stride + j];
    bf16x8_t o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (bf16_t)v[j];
    *(bf16x8_t*)(out + (size_t)row * ldo + c8) = o;
}

// ---- partial[split][big][rp] = P^T . Q over the split's tokens --------------------------------------------------------------------
// grid (ceil(big / 64), nsplit, rp / 64): a 64 x 64 output tile per workgroup.  Both operands are token-major, the contraction index
// is their ROW, so a lane's eight k values are eight rows.  A lane reads them as 4-byte loads holding TWO adjacent columns (32 lanes =
// a whole 128-byte line of each token row): the low halves are the fragment of the even column, the high halves that of the odd
// one, and four MFMAs (even / odd P columns x even / odd Q columns) per 16 tokens cover the tile with 16 loads.
__device__ __forceinline__ void lora_load_pair(const unsigned short* __restrict__ p, size_t ld, int tok, int t1, bool valid, bf16x8_t& even,
                                               bf16x8_t& odd) {
    u16x8_t e, o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const unsigned v = (valid && tok + j < t1) ? *(const unsigned*)(p + (size_t)(tok + j) * ld) : 0u;
        e[j] = (unsigned short)(v & 0xffffu);
        o[j] = (unsigned short)(v >> 16);
    }
    even = __builtin_bit_cast(bf16x8_t, e);
    odd = __builtin_bit_cast(bf16x8_t, o);
}

__global__ __launch_bounds__(256) void lora_dw_partial_kernel(const unsigned short* __restrict__ p, int ldp, int p_blk,
                                                              const unsigned short* __restrict__ q, int ldq, int toks, int tps, int big,
                                                              int rp, float* __restrict__ partial) {
    __shared__ float part[LORA_WAVES][32][65];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int m0 = blockIdx.x * 64, sp = blockIdx.y, qc0 = blockIdx.z * 64;
    const int t0 = sp * tps, t1 = min(toks, t0 + tps);
    const int c0 = m0 + 2 * r;                                          // this lane's logical P columns c0, c0 + 1 (one 32-column block)
    const bool valid = c0 < big;                                        // big % 32 == 0: the last tile may be half empty
    const unsigned short* pp = p + (size_t)(c0 >> 5) * p_blk + (c0 & 31);
    const unsigned short* qq = q + qc0 + 2 * r;
    f32x16_t acc[2][2];                                                  // [P column parity][Q column parity]
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[0][0][i] = acc[0][1][i] = acc[1][0][i] = acc[1][1][i] = 0.0f;
    // two 16-token steps per round, all 32 loads issued before the first MFMA (a step past t1 loads nothing and adds zeros)
    for (int t = t0 + wv * 16; t < t1; t += 2 * LORA_WAVES * 16) {
        bf16x8_t a[2][2], b[2][2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int tok = t + u * LORA_WAVES * 16 + 8 * h;
            lora_load_pair(pp, (size_t)ldp, tok, t1, valid, a[u][0], a[u][1]);
            lora_load_pair(qq, (size_t)ldq, tok, t1, true, b[u][0], b[u][1]);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            acc[0][0] = lora_mfma(a[u][0], b[u][0], acc[0][0]);
            acc[0][1] = lora_mfma(a[u][0], b[u][1], acc[0][1]);
            acc[1][0] = lora_mfma(a[u][1], b[u][0], acc[1][0]);
            acc[1][1] = lora_mfma(a[u][1], b[u][1], acc[1][1]);
        }
    }
    // accumulator element (row i, lane column c) of acc[x][y] is output (m0 + 2 i + x, qc0 + 2 c + y): one P parity at a time through LDS
    const int row = threadIdx.x >> 3, c8 = (threadIdx.x & 7) * 8;
#pragma unroll
    for (int x = 0; x < 2; ++x) {
        if (x) __syncthreads();
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int i = (reg & 3) + 8 * (reg >> 2) + 4 * h;
            part[wv][i][2 * r] = acc[x][0][reg];
            part[wv][i][2 * r + 1] = acc[x][1][reg];
        }
        __syncthreads();
        const int m = m0 + 2 * row + x;
        if (m < big) {
            float* dst = partial + ((size_t)sp * big + m) * rp + qc0 + c8;
            float4 o[2];
            float* of = (float*)o;
#pragma unroll
            for (int j = 0; j < 8; ++j) of[j] = (part[0][row][c8 + j] + part[1][row][c8 + j]) + (part[2][row][c8 + j] + part[3][row][c8 + j]);
            *(float4*)dst = o[0];
            *(float4*)(dst + 4) = o[1];
        }
    }
}

// g (= | +=) scale * sum over the splits (fixed order), rank-padding columns zero; sumsq += sum of squares of what was stored
__global__ __launch_bounds__(256) void lora_dw_finish_kernel(const float* __restrict__ partial, int nsplit, long long n4, int rp, int r,
                                                             float scale, float* __restrict__ g, int accumulate, double* __restrict__ sumsq) {
    const long long i4 = (long long)blockIdx.x * 256 + threadIdx.x;
    double ss = 0.0;
    if (i4 < n4) {
        const long long stride = n4 * 4;
        float4 s = *(const float4*)(partial + i4 * 4);
        for (int k = 1; k < nsplit; ++k) {
            const float4 t = *(const float4*)(partial + k * stride + i4 * 4);
            s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
        }
        const int col = (int)((i4 * 4) % rp);
        float v[4] = {s.x * scale, s.y * scale, s.z * scale, s.w * scale};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (col + j >= r) v[j] = 0.0f;
        float4 o = make_float4(v[0], v[1], v[2], v[3]);
        if (accumulate) {
            const float4 old = *(const float4*)(g + i4 * 4);
            o.x += old.x; o.y += old.y; o.z += old.z; o.w += old.w;
        }
        *(float4*)(g + i4 * 4) = o;
        ss = ((double)o.x * o.x + (double)o.y * o.y) + ((double)o.z * o.z + (double)o.w * o.w);
    }
    if (sumsq != nullptr) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
        if ((threadIdx.x & 63) == 0 && ss != 0.0) atomicAdd(sumsq, ss);
    }
}

// ---- bf16 operand copies of one fp32 master -------------------------------------------------------------------------------------
// grid (rows / 32, rp / 32), 32 x 8 threads; the transposed copy goes through a padded LDS tile so both stores run along a row.
__global__ __launch_bounds__(256) void lora_refresh_kernel(const float* __restrict__ src, int rp, float scale, int blk,
                                                           bf16_t* __restrict__ dst, int ld_dst, bf16_t* __restrict__ dst_t, int ld_t) {
    __shared__ bf16_t tile[32][34];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int i0 = blockIdx.x * 32, j0 = blockIdx.y * 32;
    const size_t o0 = (size_t)blockIdx.x * blk;                      // row_of(i0): i0 is a multiple of 32
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
        const int i = ty + 8 * qd;
        const bf16_t v = (bf16_t)(src[(size_t)(i0 + i) * rp + j0 + tx] * scale);
        tile[i][tx] = v;
        if (dst != nullptr) dst[(o0 + i) * ld_dst + j0 + tx] = v;
    }
    __syncthreads();
    if (dst_t != nullptr) {
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
            const int j = ty + 8 * qd;
            dst_t[(size_t)(j0 + j) * ld_t + o0 + tx] = tile[tx][j];
        }
    }
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// k split of llark_lora_down: 4 or 2 workgroups per tile while that still fits one round of a 256-CU chip and every part keeps whole
// 64-wide chunks of the waves and at least 512 columns; 1 = no split
static inline int lora_down_split(int rows, int k, int rp_total) {
    const long tiles = (long)((rows + 31) / 32) * (rp_total / 64);
    for (int ns = 4; ns >= 2; ns >>= 1)
        if (tiles * ns <= 256 && k % (64 * ns) == 0 && k / ns >= 512) return ns;
    return 1;
}

// token split of llark_lora_dw: about four workgroups per CU of a 256-CU chip, whole 64-token rounds of the four waves
static inline void lora_dw_split(int toks, int big, int rp, int* nsplit, int* tps) {
    const long tiles = (long)((big + 63) / 64) * (rp / 64);
    long ns = (1024 + tiles - 1) / tiles;
    const long max_ns = (toks + 63) / 64;
    if (ns > max_ns) ns = max_ns;
    if (ns > 32) ns = 32;
    if (ns < 1) ns = 1;
    long t = (toks + ns - 1) / ns;
    t = (t + 63) / 64 * 64;
    *tps = (int)t;
    *nsplit = (int)((toks + t - 1) / t);
}

static inline bool lora_dw_takes(int toks, int big, int rp) {
    return toks > 0 && big > 0 && big % 32 == 0 && rp > 0 && rp % 64 == 0 && rp <= 256 && big / 64 < 65535;
}

}  // namespace llark

using namespace llark;

extern "C" long long llark_lora_down_scratch_bytes(int rows, int k, int rp_total) {
    if (rows <= 0 || k <= 0 || k % 16 || rp_total <= 0 || rp_total % 64 || rp_total > 1024) return 0;
    const int ns = lora_down_split(rows, k, rp_total);
    return ns > 1 ? (long long)ns * rows * rp_total * 4 : 0;
}

extern "C" int llark_lora_down(const void* x, int lda, const void* m, int ldm, int rows, int k, int rp_total, void* out, int ldo,
                               void* scratch, long long scratch_bytes, llark_stream_t stream) {
    LLARK_REQUIRE(x && m && out, "lora_down: null pointer");
    if (rows <= 0 || k <= 0 || k % 16 || rp_total <= 0 || rp_total % 64 || rp_total > 1024 || lda < k || ldm < k || ldo < rp_total ||
        lda % 8 || ldm % 8 || ldo % 8 || !aligned16(x) || !aligned16(m) || !aligned16(out)) {
        set_error("lora_down: unsupported shape rows=%d k=%d rp_total=%d lda=%d ldm=%d ldo=%d (or a pointer not 16-byte aligned)", rows, k,
                  rp_total, lda, ldm, ldo);
        return LLARK_ERR_UNSUPPORTED;
    }
    const int ns = lora_down_split(rows, k, rp_total);
    if (ns > 1 && scratch != nullptr && aligned16(scratch) && scratch_bytes >= (long long)ns * rows * rp_total * 4) {
        dim3 grid(cdiv(rows, 32), rp_total / 64, ns);
        lora_down_kernel<<<grid, 256, 0, (hipStream_t)stream>>>((const bf16_t*)x, lda, (const bf16_t*)m, ldm, rows, k / ns, (bf16_t*)out, ldo,
                                                                (float*)scratch, rp_total);
        const int rc = check_launch("lora_down (partial)");
        if (rc) return rc;
        const long long n8 = (long long)rows * (rp_total / 8);
        lora_down_finish_kernel<<<cdiv(n8, 256), 256, 0, (hipStream_t)stream>>>((const float*)scratch, ns, rows, rp_total, (bf16_t*)out, ldo);
        return check_launch("lora_down (finish)");
    }
    dim3 grid(cdiv(rows, 32), rp_total / 64);
    lora_down_kernel<<<grid, 256, 0, (hipStream_t)stream>>>((const bf16_t*)x, lda, (const bf16_t*)m, ldm, rows, k, (bf16_t*)out, ldo, nullptr,
                                                            rp_total);
    return check_launch("lora_down");
}

extern "C" long long llark_lora_dw_scratch_bytes(int toks, int big, int rp) {
    if (!lora_dw_takes(toks, big, rp)) return 0;
    int nsplit, tps;
    lora_dw_split(toks, big, rp, &nsplit, &tps);
    return (long long)nsplit * big * rp * 4;
}

extern "C" int llark_lora_dw(const void* p, int ldp, int p_blk, const void* q, int ldq, int toks, int big, int rp, int r, float scale,
                             float* g, int accumulate, double* sumsq, void* scratch, long long scratch_bytes, llark_stream_t stream) {
    LLARK_REQUIRE(p && q && g && scratch, "lora_dw: null pointer");
    if (!lora_dw_takes(toks, big, rp) || r <= 0 || r > rp || p_blk < 32 || p_blk % 32 || ldq < rp ||
        (long long)ldp < (long long)(big / 32 - 1) * p_blk + 32 || (ldp & 1) || (ldq & 1) || ((uintptr_t)p & 3) || ((uintptr_t)q & 3) ||
        !aligned16(g) || !aligned16(scratch) ||
        scratch_bytes < llark_lora_dw_scratch_bytes(toks, big, rp)) {
        set_error("lora_dw: unsupported shape toks=%d big=%d rp=%d r=%d ldp=%d p_blk=%d ldq=%d scratch=%lld", toks, big, rp, r, ldp, p_blk,
                  ldq, scratch_bytes);
        return LLARK_ERR_UNSUPPORTED;
    }
    int nsplit, tps;
    lora_dw_split(toks, big, rp, &nsplit, &tps);
    hipStream_t s = (hipStream_t)stream;
    dim3 grid(cdiv(big, 64), nsplit, rp / 64);
    lora_dw_partial_kernel<<<grid, 256, 0, s>>>((const unsigned short*)p, ldp, p_blk, (const unsigned short*)q, ldq, toks, tps, big, rp,
                                                (float*)scratch);
    int rc = check_launch("lora_dw (partial)");
    if (rc) return rc;
    const long long n4 = (long long)big * rp / 4;
    lora_dw_finish_kernel<<<cdiv(n4, 256), 256, 0, s>>>((const float*)scratch, nsplit, n4, rp, r, scale, g, accumulate, sumsq);
    return check_launch("lora_dw (finish)");
}

extern "C" int llark_lora_refresh(const float* src, int rows, int rp, float scale, int blk, void* dst, int ld_dst, void* dst_t, int ld_t,
                                  llark_stream_t stream) {
    LLARK_REQUIRE(src && (dst || dst_t), "lora_refresh: null pointer");
    if (rows <= 0 || rows % 32 || rp <= 0 || rp % 32 || blk < 32 || blk % 32 || (dst && ld_dst < rp) ||
        (dst_t && (long long)ld_t < (long long)(rows / 32 - 1) * blk + 32) || rp / 32 > 65535) {
        set_error("lora_refresh: unsupported shape rows=%d rp=%d blk=%d ld_dst=%d ld_t=%d", rows, rp, blk, ld_dst, ld_t);
        return LLARK_ERR_UNSUPPORTED;
    }
    dim3 grid(rows / 32, rp / 32);
    lora_refresh_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(src, rp, scale, blk, (bf16_t*)dst, ld_dst, (bf16_t*)dst_t, ld_t);
    return check_launch("lora_refresh");
}
