// Block decode attention for gfx950: several rows of one launch belong to the SAME slot at consecutive positions
// (llark_attn_decode_rope_bf16_block; the attention of a speculative decode step, engine.decode_block).
//
// Slot b owns rows b*stride .. b*stride + blk[b] - 1 of qkv / out; row i is the token at position pos_rows[b] + i.  Workgroup (head h,
// slot b) first rotates and appends the K / V of ALL its rows (rope_split_kernel's arithmetic and rounding, as the fused decode kernel of
// llama.hip does for its one row), then walks the cache ONCE: every K row and every V^T chunk is loaded once and used for each query of
// the block; query i sees keys 0 .. pos + i.
//
// Contract: row i's out planes and the cache rows written are BIT-equal to blk[b] successive llark_attn_decode_rope_bf16_rows launches.
// Per query the arithmetic below is attn_decode_body's, operation for operation, and that arithmetic is fixed by NT alone: the 16-lane
// shuffle tree of a score, lsum strided by NT then wave_sum then the ascending sum over waves, the PV chain in which chunk c belongs to
// part (c / 8) % (NT / 128) in ascending order followed by the xor tree, and the ragged-last-chunk rule of hi + lo planes.  What differs
// -- the trip counts, the clamped re-loads, the stale or newer columns a p = 0 multiplies -- never reaches a result.  No ALiBi.
#include "common.h"

namespace llark {

__device__ __forceinline__ void blk_store_split(bf16_t* __restrict__ hi, bf16_t* __restrict__ lo, size_t idx, float v) {   // llama.hip: store_split
    const bf16_t h = (bf16_t)v;
    hi[idx] = h;
    if (lo) lo[idx] = (bf16_t)(v - (float)h);
}

// QN: compiled query capacity (stride rounded up to 1, 2, 4, 8).  Queries live in LDS (sq, read as broadcasts inside the key loop) so
// that eight queries' running state -- lmax / acc / inv, 8 registers each -- stays far below the 128 registers of a 16-wave workgroup.
template <int NW, int UBT, int QN>
__global__ __launch_bounds__(NW * 64) void attn_block_kernel(const float* __restrict__ qkv, int stride, const int* __restrict__ blk,
                                                             const int* __restrict__ pos_rows, const float* __restrict__ cos_t,
                                                             const float* __restrict__ sin_t, bf16_t* kc, bf16_t* vtc, bf16_t* kc_lo,
                                                             bf16_t* vtc_lo, bf16_t* __restrict__ out, bf16_t* __restrict__ out_lo, int nh,
                                                             int smax, float scale) {
    constexpr int NT = NW * 64;
    constexpr int UB = UBT;
    constexpr int PARTS = NT / 128;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sp = (float*)smem;                                   // [stride][smax] scores / probabilities
    __shared__ __attribute__((aligned(16))) float sq[QN][128];
    __shared__ float red[QN][2 * NW];
    const int h = blockIdx.x, b = blockIdx.y, H = nh * 128;
    const size_t bh = (size_t)b * nh + h;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int pos = pos_rows[b];                                // uniform per block: the whole block leaves together
    int nq = blk[b];
    nq = nq < stride ? nq : stride;
    if (pos < 0 || pos >= smax) nq = 0;
    else nq = nq < smax - pos ? nq : smax - pos;                // rows at positions >= smax compute nothing
    nq = nq < 0 ? 0 : (nq < QN ? nq : QN);
    for (int e = tid; e < (stride - nq) * 128; e += NT)        // rows that compute nothing: zero output head
        blk_store_split(out, out_lo, ((size_t)b * stride + nq + (e >> 7)) * H + h * 128 + (e & 127), 0.0f);
    if (nq == 0) return;
    const bool split = kc_lo != nullptr;
    // ---- RoPE + cache append of every row of the block (attn_decode_kernel's fused front, once per row)
    for (int e = tid; e < nq * 256; e += NT) {
        const int i = e >> 8, r = e & 255, p = pos + i;
        const float* row = qkv + ((size_t)b * stride + i) * 3 * H + h * 128;
        if (r < 64) {
            const int d = r;
            const float c = cos_t[(size_t)p * 64 + d], sn = sin_t[(size_t)p * 64 + d];
            const float q1 = row[d], q2 = row[d + 64], k1 = row[H + d], k2 = row[H + d + 64];
            const float qa = __fadd_rn(__fmul_rn(q1, c), __fmul_rn(-q2, sn));
            const float qb = __fadd_rn(__fmul_rn(q2, c), __fmul_rn(q1, sn));
            const float ka = __fadd_rn(__fmul_rn(k1, c), __fmul_rn(-k2, sn));
            const float kb2 = __fadd_rn(__fmul_rn(k2, c), __fmul_rn(k1, sn));
            const bf16_t ha = (bf16_t)qa, hb = (bf16_t)qb;
            sq[i][d] = (float)ha + (split ? (float)(bf16_t)(qa - (float)ha) : 0.0f);
            sq[i][d + 64] = (float)hb + (split ? (float)(bf16_t)(qb - (float)hb) : 0.0f);
            const size_t ko = (bh * (size_t)smax + p) * 128;
            blk_store_split(kc, kc_lo, ko + d, ka);
            blk_store_split(kc, kc_lo, ko + d + 64, kb2);
        } else if (r >= 128) {
            const int d = r - 128;
            blk_store_split(vtc, vtc_lo, (bh * 128 + d) * (size_t)smax + p, row[2 * H + d]);
        }
    }
    __syncthreads();                                            // q (LDS) and the appended rows (global) are visible to the block
    const int total0 = pos + 1;                                 // keys visible to query 0; query i sees total0 + i
    const int totmax = total0 + nq - 1;                         // <= smax
    // ---- scores: 16 lanes per key, 4 keys per wave and iteration, the partial dot products meet in a shuffle tree
    const bf16_t* kb = kc + bh * (size_t)smax * 128;
    const bf16_t* kbl = kc_lo ? kc_lo + bh * (size_t)smax * 128 : nullptr;
    const int chunk = lane & 15, sub = lane >> 4;
    float lmax[QN];
#pragma unroll
    for (int i = 0; i < QN; ++i) lmax[i] = -INFINITY;
    constexpr int KSTEP = NW * 4;
    for (int jb = wv * 4 + sub; jb < totmax + KSTEP - 1; jb += KSTEP * UB) {
        bf16x8_t kv[UB], kl[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            int j = jb + KSTEP * u;
            j = j < totmax ? j : totmax - 1;
            kv[u] = *(const bf16x8_t*)(kb + (size_t)j * 128 + chunk * 8);
            if (kbl) kl[u] = *(const bf16x8_t*)(kbl + (size_t)j * 128 + chunk * 8);
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            const int j = jb + KSTEP * u;
            float kf[8];
            if (kbl) {
#pragma unroll
                for (int e = 0; e < 8; ++e) kf[e] = (float)kv[u][e] + (float)kl[u][e];
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) kf[e] = (float)kv[u][e];
            }
            // the queries are re-read from LDS for every key (two 16-byte broadcasts per query): an offset the compiler cannot see
            // through keeps it from hoisting QN * 8 query registers out of the key loop, which spilled at 16 waves
            int qoff = chunk * 8;
            asm volatile("" : "+v"(qoff));
#pragma unroll
            for (int i = 0; i < QN; ++i) {
                if (i < nq) {                                   // uniform per block
                    const float4 qa = *(const float4*)&sq[i][qoff], qb = *(const float4*)&sq[i][qoff + 4];
                    const float qv[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
                    float s = 0.0f;
#pragma unroll
                    for (int e = 0; e < 8; ++e) s = fmaf(qv[e], kf[e], s);
                    s += __shfl_xor(s, 1, 64);
                    s += __shfl_xor(s, 2, 64);
                    s += __shfl_xor(s, 4, 64);
                    s += __shfl_xor(s, 8, 64);
                    s *= scale;
                    if (j < total0 + i) {
                        if (chunk == 0) sp[(size_t)i * smax + j] = s;
                        lmax[i] = fmaxf(lmax[i], s);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);              // one query's loads and shuffles at a time: see QN above
            }
        }
    }
#pragma unroll
    for (int i = 0; i < QN; ++i) {
        const float m = wave_max(lmax[i]);
        if (lane == 0) red[i][wv] = m;
    }
    __syncthreads();
    float lsum[QN];
#pragma unroll
    for (int i = 0; i < QN; ++i) {
        lsum[i] = 0.0f;
        if (i < nq) {
            float mx = red[i][0];
#pragma unroll
            for (int w = 1; w < NW; ++w) mx = fmaxf(mx, red[i][w]);
            float* spi = sp + (size_t)i * smax;
            const int total = total0 + i, tpad = (total + 7) & ~7;
            float ls = 0.0f;
            for (int j = tid; j < tpad; j += NT) {
                float p = 0.0f;                                 // keys total..tpad-1 only pad the 8-key PV chunks
                if (j < total) {
                    p = expf(spi[j] - mx);
                    ls += p;
                }
                spi[j] = p;
            }
            lsum[i] = wave_sum(ls);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < QN; ++i)
        if (lane == 0) red[i][NW + wv] = lsum[i];
    __syncthreads();
    float acc[QN];
#pragma unroll
    for (int i = 0; i < QN; ++i) acc[i] = 0.0f;
    // ---- O_i[d] = sum_j p_ij V[j][d]: PARTS threads per d, each walking 16-B chunks of 8 keys; one load serves every query
    const int d = tid / PARTS, part = tid % PARTS;
    const bf16_t* vr = vtc + (bh * 128 + d) * (size_t)smax;
    const bf16_t* vrl = vtc_lo ? vtc_lo + (bh * 128 + d) * (size_t)smax : nullptr;
    const int tpadmax = (totmax + 7) & ~7;
    for (int cb = part * 8; cb < tpadmax; cb += 8 * PARTS * UB) {
        bf16x8_t vv[UB], vl[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            int c8 = cb + 8 * PARTS * u;
            c8 = c8 < tpadmax ? c8 : tpadmax - 8;
            vv[u] = *(const bf16x8_t*)(vr + c8);
            if (vrl) vl[u] = *(const bf16x8_t*)(vrl + c8);
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            const int c8 = cb + 8 * PARTS * u;
            float vf[8];
            if (vrl) {
#pragma unroll
                for (int e = 0; e < 8; ++e) vf[e] = (float)vv[u][e] + (float)vl[u][e];
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) vf[e] = (float)vv[u][e];
            }
#pragma unroll
            for (int i = 0; i < QN; ++i) {
                const int total = total0 + i, tpad = (total + 7) & ~7;
                if (i < nq && c8 < tpad) {
                    const float* spi = sp + (size_t)i * smax + c8;
                    const float4 pa = *(const float4*)spi, pb = *(const float4*)(spi + 4);
                    const float pv[8] = {pa.x, pa.y, pa.z, pa.w, pb.x, pb.y, pb.z, pb.w};
                    if (vrl && c8 + 8 > total) {
                        // the ragged last chunk of hi + lo planes: the sum of two stale planes need not be finite; those columns are
                        // left out instead of multiplied by p = 0 (attn_decode_body's rule, per query)
#pragma unroll
                        for (int e = 0; e < 8; ++e)
                            if (c8 + e < total) acc[i] = fmaf(pv[e], vf[e], acc[i]);
                    } else {
#pragma unroll
                        for (int e = 0; e < 8; ++e) acc[i] = fmaf(pv[e], vf[e], acc[i]);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < QN; ++i) {
        float a = acc[i];
#pragma unroll
        for (int o = 1; o < PARTS; o <<= 1) a += __shfl_xor(a, o, 64);
        // the normaliser is summed here, where it is used: summed before the PV loop, its QN * NW words stayed live across it and spilled
        float tot = 0.0f;
#pragma unroll
        for (int w = 0; w < NW; ++w) tot += red[i][NW + w];
        const float inv = 1.0f / tot;
        if (part == 0 && i < nq) blk_store_split(out, out_lo, ((size_t)b * stride + i) * H + h * 128 + d, a * inv);
        __builtin_amdgcn_sched_barrier(0);
    }
}

}  // namespace llark

using namespace llark;

extern "C" int llark_attn_decode_rope_bf16_block(const float* qkv, int n_slots, int stride, int nh, int hd, const int* blk, const int* pos_rows,
                                                 const float* cos_t, const float* sin_t, int max_pos, void* k_cache, void* vt_cache,
                                                 void* k_cache_lo, void* vt_cache_lo, int smax, void* out, void* out_lo, llark_stream_t stream) {
    const char* name = "attn_decode_rope_block";
    LLARK_REQUIRE(qkv && blk && pos_rows && cos_t && sin_t && k_cache && vt_cache && out, "%s: null pointer", name);
    LLARK_REQUIRE(hd == 128, "%s: head_dim must be 128 (Llama-2), got %d", name, hd);
    LLARK_REQUIRE((k_cache_lo == nullptr) == (vt_cache_lo == nullptr) && (k_cache_lo == nullptr) == (out_lo == nullptr),
                  "%s: give all lo planes (fp32-class mode) or none", name);
    LLARK_REQUIRE(n_slots > 0 && nh > 0 && stride >= 1 && stride <= 8 && smax > 0 && smax % 8 == 0 && smax <= max_pos && n_slots <= 65535,
                  "%s: bad shape n_slots=%d stride=%d nh=%d smax=%d max_pos=%d (stride 1 .. 8, smax %% 8 == 0, smax <= max_pos)", name, n_slots,
                  stride, nh, smax, max_pos);
    const size_t lds = (size_t)stride * smax * sizeof(float);
    if (lds > 128 * 1024) {
        set_error("%s: stride * smax = %d * %d scores do not fit the 128 KiB LDS score buffer", name, stride, smax);
        return LLARK_ERR_UNSUPPORTED;
    }
    const float scale = (float)(1.0 / sqrt((double)hd));
    auto run = [&](auto qn_c) {
        constexpr int QN = decltype(qn_c)::value;
        auto launch = [&](auto kern, int threads) {
            kern<<<dim3(nh, n_slots), threads, lds, (hipStream_t)stream>>>(qkv, stride, blk, pos_rows, cos_t, sin_t, (bf16_t*)k_cache, (bf16_t*)vt_cache,
                                                                           (bf16_t*)k_cache_lo, (bf16_t*)vt_cache_lo, (bf16_t*)out, (bf16_t*)out_lo, nh, smax,
                                                                           scale);
        };
        // the dynamic LDS limit is raised per device and instantiation, as attn_decode() does (not a stream op)
        static PerDeviceOnce once;
        const bool first = once.first();
        if (lds > 48 * 1024 && (first || (int)lds > once.slot())) {
            (void)hipFuncSetAttribute((const void*)attn_block_kernel<4, 8, QN>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            (void)hipFuncSetAttribute((const void*)attn_block_kernel<16, 4, QN>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            once.slot() = (int)lds;
        }
        if ((long)nh * n_slots < 256) launch(attn_block_kernel<16, 4, QN>, 1024);          // attn_decode()'s rule
        else launch(attn_block_kernel<4, 8, QN>, 256);
    };
    if (stride == 1) run(std::integral_constant<int, 1>{});
    else if (stride == 2) run(std::integral_constant<int, 2>{});
    else if (stride <= 4) run(std::integral_constant<int, 4>{});
    else run(std::integral_constant<int, 8>{});
    return check_launch(name);
}
