// Shared-prefix decode for the ragged slot mode: the slots of one clip hold the same K/V at their first P positions (conversation
// header + audio block), so a decode step reads those positions once per GROUP instead of once per slot.
//   llark_kv_copy_prefix                 positions [0, n) of one cache slot into other slots (a sibling's slot at its fork)
//   llark_attn_decode_rope_bf16_shared   llark_attn_decode_rope_bf16_rows plus a group table: two launches in stream order --
//       attn_group_kernel   per (head, group, key range): the members' rotated queries against keys [0, P) of the group's source slot,
//                           every K row and V^T chunk loaded once for all members; leaves per (member, head, key range) an unnormalised
//                           output, a running maximum and a sum (fp32) in the caller's scratch;
//       attn_slot_kernel    per (head, slot): RoPE + cache append + attention over keys [shared_len, total) exactly as the rows form,
//                           then the log-sum-exp merge with the slot's partials.  shared_len == 0: the rows form, bit for bit.
// No workgroup waits for another one: the launch boundary is the only synchronisation.
#include <math.h>
#include <type_traits>

#include "common.h"

using namespace llark;

namespace {

constexpr int GK_KEYS = 128;        // keys per round of the group pass: 16 key lanes-groups x GK_UB loads in flight = ONE round of memory latency
constexpr int GK_UB = 8;            // loads in flight per lane, in the K pass and in the V^T pass
constexpr int GK_MEMBERS = 16;      // members per group (the host cuts larger lineages)
constexpr int GK_SPLITS = 4;        // key ranges per group (grid.z): up to 4 rounds of one group run side by side
constexpr int GK_TAB = 3 + GK_MEMBERS;   // int32 per group: source slot, P, members, member slots
constexpr int PART_LD = 132;        // fp32 per partial: o[128], max, sum, 2 pad (16-byte rows)
constexpr int SCRATCH_HEAD = 64;    // bytes in front of the partials; word 0 = status of the last refused table (0: none)

enum { ST_OK = 0, ST_SHARED_LEN = 1, ST_GROUP_SIZE = 2, ST_MEMBER_POS = 3, ST_SOURCE = 4, ST_MEMBER = 5 };

__device__ __forceinline__ void store_split(bf16_t* __restrict__ hi, bf16_t* __restrict__ lo, size_t idx, float v) {
    const bf16_t h = (bf16_t)v;
    hi[idx] = h;
    if (lo) lo[idx] = (bf16_t)(v - (float)h);
}

// Key range z of a group whose shared length is P: rounds [r0, r1) of GK_KEYS keys; ns = ranges in use (<= GK_SPLITS).
__device__ __forceinline__ void split_rounds(int P, int z, int& r0, int& r1, int& ns) {
    const int rounds = (P + GK_KEYS - 1) / GK_KEYS;
    ns = rounds < GK_SPLITS ? rounds : GK_SPLITS;
    r0 = z * rounds / ns;
    r1 = (z + 1) * rounds / ns;
}

// One workgroup per (head, group, key range).  256 threads: K pass = 16 lanes per key, 16 keys per load slot, GK_UB slots = the round's
// 128 keys in flight at once; V^T pass = 2 threads per output dim, each GK_UB chunks of 8 keys.  LDS: queries 8 KiB + one round of
// scores 8 KiB, whatever P and the member count.
__global__ __launch_bounds__(256) void attn_group_kernel(const float* __restrict__ qkv, const bf16_t* __restrict__ kc, const bf16_t* __restrict__ vtc,
                                                         const bf16_t* __restrict__ kc_lo, const bf16_t* __restrict__ vtc_lo, int batch, int nh, int smax,
                                                         float scale, const int* __restrict__ pos_rows, const float* __restrict__ cos_t,
                                                         const float* __restrict__ sin_t, const int* __restrict__ groups,
                                                         const int* __restrict__ slot_shared, int* status, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float sq[GK_MEMBERS * 128];
    __shared__ __attribute__((aligned(16))) float sp[GK_MEMBERS * GK_KEYS];
    __shared__ float s_m[GK_MEMBERS], s_l[GK_MEMBERS], s_alpha[GK_MEMBERS];
    __shared__ int s_slot[GK_MEMBERS], s_pos[GK_MEMBERS];
    __shared__ int s_bad;
    const int h = blockIdx.x, z = blockIdx.z;
    const int* G = groups + (size_t)blockIdx.y * GK_TAB;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int src = G[0], P = G[1], cnt = G[2];
    // ---- the table is device data: check every index before it forms an address; a bad group is refused (status) and computes nothing
    int bad = ST_OK;
    if (cnt < 1 || cnt > GK_MEMBERS) bad = ST_GROUP_SIZE;
    else if (P <= 0 || (P & 7) != 0 || P > smax) bad = ST_SHARED_LEN;
    else if (src < 0 || src >= batch || pos_rows[src] < P) bad = ST_SOURCE;
    if (tid == 0) s_bad = bad;
    __syncthreads();
    if (bad == ST_OK && tid < cnt) {
        const int s = G[3 + tid];
        int mb = ST_OK, p = -1;
        if (s < 0 || s >= batch || slot_shared[s] != P) mb = ST_MEMBER;
        else {
            p = pos_rows[s];
            if (p < P || p >= smax) mb = ST_MEMBER_POS;
        }
        s_slot[tid] = s, s_pos[tid] = p;
        if (mb != ST_OK) s_bad = mb;                       // any one of the failing lanes' codes
    }
    __syncthreads();
    bad = s_bad;
    if (bad != ST_OK) {
        if (tid == 0 && h == 0 && z == 0) *status = bad;
        return;
    }
    int r0, r1, ns;
    split_rounds(P, z, r0, r1, ns);
    if (z >= ns) return;
    // ---- the members' rotated queries: the arithmetic and rounding of the fused decode kernel (attn_slot_kernel below)
    const int H = nh * 128;
    const bool split = kc_lo != nullptr;
    for (int i = tid; i < cnt * 64; i += 256) {
        const int m = i >> 6, d = i & 63;
        const float* row = qkv + (size_t)s_slot[m] * 3 * H + h * 128;
        const int pos = s_pos[m];
        const float c = cos_t[(size_t)pos * 64 + d], sn = sin_t[(size_t)pos * 64 + d];
        const float q1 = row[d], q2 = row[d + 64];
        const float qa = __fadd_rn(__fmul_rn(q1, c), __fmul_rn(-q2, sn));
        const float qb = __fadd_rn(__fmul_rn(q2, c), __fmul_rn(q1, sn));
        const bf16_t ha = (bf16_t)qa, hb = (bf16_t)qb;
        sq[m * 128 + d] = (float)ha + (split ? (float)(bf16_t)(qa - (float)ha) : 0.0f);
        sq[m * 128 + d + 64] = (float)hb + (split ? (float)(bf16_t)(qb - (float)hb) : 0.0f);
    }
    if (tid < GK_MEMBERS) s_m[tid] = -INFINITY, s_l[tid] = 0.0f;
    __syncthreads();
    const size_t sh = (size_t)src * nh + h;
    const bf16_t* kb = kc + sh * (size_t)smax * 128;
    const bf16_t* kbl = split ? kc_lo + sh * (size_t)smax * 128 : nullptr;
    const int chunk = lane & 15, kg = wv * 4 + (lane >> 4);     // 16 lanes per key; key group 0 .. 15
    const int d = tid >> 1, vpart = tid & 1;
    const bf16_t* vr = vtc + (sh * 128 + d) * (size_t)smax;
    const bf16_t* vrl = split ? vtc_lo + (sh * 128 + d) * (size_t)smax : nullptr;
    float acc[GK_MEMBERS];
#pragma unroll
    for (int m = 0; m < GK_MEMBERS; ++m) acc[m] = 0.0f;
    for (int r = r0; r < r1; ++r) {
        const int k0 = r * GK_KEYS;
        // ---- scores of the round: every K row loaded once, used by all members
        {
            bf16x8_t kv[GK_UB], kl[GK_UB];
#pragma unroll
            for (int u = 0; u < GK_UB; ++u) {
                int j = k0 + kg + 16 * u;
                j = j < P ? j : P - 1;
                kv[u] = *(const bf16x8_t*)(kb + (size_t)j * 128 + chunk * 8);
                if (kbl) kl[u] = *(const bf16x8_t*)(kbl + (size_t)j * 128 + chunk * 8);
            }
            float kf[GK_UB][8];
#pragma unroll
            for (int u = 0; u < GK_UB; ++u)
#pragma unroll
                for (int e = 0; e < 8; ++e) kf[u][e] = kbl ? (float)kv[u][e] + (float)kl[u][e] : (float)kv[u][e];
            for (int m = 0; m < cnt; ++m) {
                float qv[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) qv[e] = sq[m * 128 + chunk * 8 + e];
#pragma unroll
                for (int u = 0; u < GK_UB; ++u) {
                    const int jl = kg + 16 * u;
                    float s = 0.0f;
#pragma unroll
                    for (int e = 0; e < 8; ++e) s = fmaf(qv[e], kf[u][e], s);
                    s += __shfl_xor(s, 1, 64);
                    s += __shfl_xor(s, 2, 64);
                    s += __shfl_xor(s, 4, 64);
                    s += __shfl_xor(s, 8, 64);
                    s *= scale;
                    if (chunk == 0) sp[m * GK_KEYS + jl] = k0 + jl < P ? s : -INFINITY;
                }
            }
        }
        __syncthreads();
        // ---- running maximum and sum per member (wave w: members w, w + 4, ...); the scores become probabilities against the new maximum
        for (int m = wv; m < cnt; m += 4) {
            const float s0 = sp[m * GK_KEYS + lane], s1 = sp[m * GK_KEYS + 64 + lane];
            const float mold = s_m[m];
            const float mnew = fmaxf(mold, wave_max(fmaxf(s0, s1)));      // finite: key k0 < P is in the round
            const float p0 = expf(s0 - mnew), p1 = expf(s1 - mnew);       // exp(-inf) = 0 beyond P
            const float sum = wave_sum(p0 + p1);
            sp[m * GK_KEYS + lane] = p0;
            sp[m * GK_KEYS + 64 + lane] = p1;
            if (lane == 0) {
                const float alpha = expf(mold - mnew);                    // 0 in the first round (mold = -inf)
                s_m[m] = mnew, s_l[m] = s_l[m] * alpha + sum, s_alpha[m] = alpha;
            }
        }
        __syncthreads();
        // ---- O[m][d] = alpha O[m][d] + sum_j p[m][j] V[j][d]: every V^T chunk loaded once
        {
            bf16x8_t vv[GK_UB], vl[GK_UB];
#pragma unroll
            for (int u = 0; u < GK_UB; ++u) {
                int c8 = k0 + 8 * (vpart + 2 * u);
                c8 = c8 < P ? c8 : P - 8;                                  // clamped re-load, skipped below (P % 8 == 0: chunks are whole)
                vv[u] = *(const bf16x8_t*)(vr + c8);
                if (vrl) vl[u] = *(const bf16x8_t*)(vrl + c8);
            }
#pragma unroll
            for (int m = 0; m < GK_MEMBERS; ++m)
                if (m < cnt) acc[m] *= s_alpha[m];
#pragma unroll
            for (int u = 0; u < GK_UB; ++u) {
                const int cl = 8 * (vpart + 2 * u);
                if (k0 + cl < P) {
                    float vf[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) vf[e] = vrl ? (float)vv[u][e] + (float)vl[u][e] : (float)vv[u][e];
#pragma unroll
                    for (int m = 0; m < GK_MEMBERS; ++m) {
                        if (m < cnt) {
                            const f32x4_t pa = *(const f32x4_t*)(sp + m * GK_KEYS + cl), pb = *(const f32x4_t*)(sp + m * GK_KEYS + cl + 4);
                            float a = acc[m];
#pragma unroll
                            for (int e = 0; e < 4; ++e) a = fmaf(pa[e], vf[e], a);
#pragma unroll
                            for (int e = 0; e < 4; ++e) a = fmaf(pb[e], vf[4 + e], a);
                            acc[m] = a;
                        }
                    }
                }
            }
        }
        __syncthreads();                                                   // the next round overwrites sp
    }
#pragma unroll
    for (int m = 0; m < GK_MEMBERS; ++m) {
        if (m < cnt) {
            const float a = acc[m] + __shfl_xor(acc[m], 1, 64);
            float* dst = part + (((size_t)s_slot[m] * nh + h) * GK_SPLITS + z) * PART_LD;
            if (vpart == 0) dst[d] = a;
            if (tid == 0) dst[128] = s_m[m], dst[129] = s_l[m];
        }
    }
}

// The per-slot pass: attn_decode_kernel<NW, UBT, ROWS = true> of llama.hip in its fused form (same waves, loads in flight, loop order,
// reductions and roundings) over keys [p0, total), p0 = slot_shared[slot], followed by the merge with the group pass's partials.
template <int NW, int UBT>
__global__ __launch_bounds__(NW * 64) void attn_slot_kernel(bf16_t* kc, bf16_t* vtc, bf16_t* kc_lo, bf16_t* vtc_lo,
                                                              bf16_t* __restrict__ out, bf16_t* __restrict__ out_lo, int nh, int smax, float scale,
                                                              const int* __restrict__ pos_rows, const float* __restrict__ qkv,
                                                              const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                                              const int* __restrict__ slot_shared, int* status, const float* __restrict__ part) {
    constexpr int NT = NW * 64;
    constexpr int UB = UBT;
    constexpr int PARTS = NT / 128;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int p = pos_rows[blockIdx.y];
    if (p < 0 || p >= smax) {
        if (threadIdx.x < 128) store_split(out, out_lo, (size_t)blockIdx.y * (nh * 128) + blockIdx.x * 128 + threadIdx.x, 0.0f);
        return;
    }
    const int total = p + 1;
    int p0 = slot_shared[blockIdx.y];
    if (p0 < 0 || (p0 & 7) != 0 || p0 > p) {                  // refused: the slot walks its whole cache
        if (threadIdx.x == 0 && blockIdx.x == 0) *status = p0 > p ? ST_MEMBER_POS : ST_SHARED_LEN;
        p0 = 0;
    }
    float* sp = (float*)smem;                    // [total] scores / probabilities (entries below p0 unused)
    __shared__ float sq[128];
    __shared__ float red[2 * NW];
    const int h = blockIdx.x, b = blockIdx.y;
    const size_t bh = (size_t)b * nh + h;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    {
        const int pos = total - 1, H = nh * 128;
        const float* row = qkv + (size_t)b * 3 * H + h * 128;
        const bool split = kc_lo != nullptr;
        if (tid < 64) {
            const int d = tid;
            const float c = cos_t[(size_t)pos * 64 + d], sn = sin_t[(size_t)pos * 64 + d];
            const float q1 = row[d], q2 = row[d + 64], k1 = row[H + d], k2 = row[H + d + 64];
            const float qa = __fadd_rn(__fmul_rn(q1, c), __fmul_rn(-q2, sn));
            const float qb = __fadd_rn(__fmul_rn(q2, c), __fmul_rn(q1, sn));
            const float ka = __fadd_rn(__fmul_rn(k1, c), __fmul_rn(-k2, sn));
            const float kb2 = __fadd_rn(__fmul_rn(k2, c), __fmul_rn(k1, sn));
            const bf16_t ha = (bf16_t)qa, hb = (bf16_t)qb;
            sq[d] = (float)ha + (split ? (float)(bf16_t)(qa - (float)ha) : 0.0f);
            sq[d + 64] = (float)hb + (split ? (float)(bf16_t)(qb - (float)hb) : 0.0f);
            const size_t ko = (bh * (size_t)smax + pos) * 128;
            store_split(kc, kc_lo, ko + d, ka);
            store_split(kc, kc_lo, ko + d + 64, kb2);
        } else if (tid >= 128 && tid < 256) {
            const int d = tid - 128;
            store_split(vtc, vtc_lo, (bh * 128 + d) * (size_t)smax + pos, row[2 * H + d]);
        }
    }
    __syncthreads();
    const bf16_t* kb = kc + bh * (size_t)smax * 128;
    const bf16_t* kbl = kc_lo ? kc_lo + bh * (size_t)smax * 128 : nullptr;
    const int chunk = lane & 15, sub = lane >> 4;
    float qv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) qv[e] = sq[chunk * 8 + e];
    float lmax = -INFINITY;
    constexpr int KSTEP = NW * 4;
    for (int jb = p0 + wv * 4 + sub; jb < total + KSTEP - 1; jb += KSTEP * UB) {
        bf16x8_t kv[UB], kl[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            int j = jb + KSTEP * u;
            j = j < total ? j : total - 1;
            kv[u] = *(const bf16x8_t*)(kb + (size_t)j * 128 + chunk * 8);
            if (kbl) kl[u] = *(const bf16x8_t*)(kbl + (size_t)j * 128 + chunk * 8);
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            const int j = jb + KSTEP * u;
            float s = 0.0f;
            if (kbl) {
#pragma unroll
                for (int e = 0; e < 8; ++e) s = fmaf(qv[e], (float)kv[u][e] + (float)kl[u][e], s);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) s = fmaf(qv[e], (float)kv[u][e], s);
            }
            s += __shfl_xor(s, 1, 64);
            s += __shfl_xor(s, 2, 64);
            s += __shfl_xor(s, 4, 64);
            s += __shfl_xor(s, 8, 64);
            s *= scale;
            if (j < total) {
                if (chunk == 0) sp[j] = s;
                lmax = fmaxf(lmax, s);
            }
        }
    }
    lmax = wave_max(lmax);
    if (lane == 0) red[wv] = lmax;
    __syncthreads();
    float mx = red[0];
#pragma unroll
    for (int i = 1; i < NW; ++i) mx = fmaxf(mx, red[i]);
    float lsum = 0.0f;
    const int tpad = (total + 7) & ~7;
    for (int j = p0 + tid; j < tpad; j += NT) {
        float pr = 0.0f;
        if (j < total) {
            pr = expf(sp[j] - mx);
            lsum += pr;
        }
        sp[j] = pr;
    }
    lsum = wave_sum(lsum);
    __syncthreads();
    if (lane == 0) red[NW + wv] = lsum;
    __syncthreads();
    float tot = 0.0f;
#pragma unroll
    for (int i = 0; i < NW; ++i) tot += red[NW + i];
    const int d = tid / PARTS, vpart = tid % PARTS;
    const bf16_t* vr = vtc + (bh * 128 + d) * (size_t)smax;
    const bf16_t* vrl = vtc_lo ? vtc_lo + (bh * 128 + d) * (size_t)smax : nullptr;
    float acc = 0.0f;
    for (int cb = p0 + vpart * 8; cb < tpad; cb += 8 * PARTS * UB) {
        bf16x8_t vv[UB], vl[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            int c8 = cb + 8 * PARTS * u;
            c8 = c8 < tpad ? c8 : tpad - 8;
            vv[u] = *(const bf16x8_t*)(vr + c8);
            if (vrl) vl[u] = *(const bf16x8_t*)(vrl + c8);
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            const int c8 = cb + 8 * PARTS * u;
            if (c8 < tpad) {
                if (vrl && c8 + 8 > total) {
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        if (c8 + e < total) acc = fmaf(sp[c8 + e], (float)vv[u][e] + (float)vl[u][e], acc);
                } else if (vrl) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc = fmaf(sp[c8 + e], (float)vv[u][e] + (float)vl[u][e], acc);
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc = fmaf(sp[c8 + e], (float)vv[u][e], acc);
                }
            }
        }
    }
#pragma unroll
    for (int o = 1; o < PARTS; o <<= 1) acc += __shfl_xor(acc, o, 64);
    if (vpart != 0) return;
    const size_t oi = (size_t)b * (nh * 128) + h * 128 + d;
    if (p0 == 0) {                                             // in no group: the rows form's own last step
        const float inv = 1.0f / tot;
        store_split(out, out_lo, oi, acc * inv);
        return;
    }
    // ---- merge with the shared positions' partials: M = max of the maxima, every part scaled by exp(its max - M)
    int r0, r1, ns;
    split_rounds(p0, 0, r0, r1, ns);
    const float* pp = part + (bh * GK_SPLITS) * PART_LD;
    float M = mx;
    for (int s = 0; s < ns; ++s) M = fmaxf(M, pp[s * PART_LD + 128]);
    const float w0 = expf(mx - M);
    float L = tot * w0, O = acc * w0;
    for (int s = 0; s < ns; ++s) {
        const float w = expf(pp[s * PART_LD + 128] - M);
        L = fmaf(pp[s * PART_LD + 129], w, L);
        O = fmaf(pp[s * PART_LD + d], w, O);
    }
    store_split(out, out_lo, oi, O * (1.0f / L));
}

constexpr int COPY_MAX_DST = 64;
struct CopyDst {
    int n;
    int slot[COPY_MAX_DST];
};

// Positions [0, n) of slot `src` into the slots of `dst`, all layers, every plane given, in 16-byte chunks read once and stored once per
// destination.  blockIdx.y = layer * nh + head.  K: n rows of 256 B, contiguous; V^T: 128 rows, ceil(n / 8) chunks each.
__global__ __launch_bounds__(256) void kv_copy_prefix_kernel(uint4* k, uint4* vt, uint4* k_lo, uint4* vt_lo, int slots, int nh, int smax, int n, int src,
                                                             CopyDst dst) {
    const int layer = blockIdx.y / nh, head = blockIdx.y % nh;
    const int nch = (n + 7) >> 3, kch = n * 16, vch = 128 * nch;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= kch + vch) return;
    const size_t per_head = (size_t)smax * 16;                // uint4 per (slot, head) of either cache
    const bool isv = i >= kch;
    const size_t off = isv ? (size_t)((i - kch) / nch) * (smax >> 3) + (i - kch) % nch : (size_t)i;
    uint4* hi = isv ? vt : k;
    uint4* lo = isv ? vt_lo : k_lo;
    const size_t so = (((size_t)layer * slots + src) * nh + head) * per_head + off;
    const uint4 a = hi[so];
    uint4 bl = a;
    if (lo) bl = lo[so];
    for (int t = 0; t < dst.n; ++t) {
        const size_t o = (((size_t)layer * slots + dst.slot[t]) * nh + head) * per_head + off;
        hi[o] = a;
        if (lo) lo[o] = bl;
    }
}

}  // namespace

#define LLARK_REFUSE(cond, ...)                  \
    do {                                         \
        if (!(cond)) {                           \
            llark::set_error(__VA_ARGS__);       \
            return LLARK_ERR_UNSUPPORTED;        \
        }                                        \
    } while (0)

extern "C" int llark_kv_copy_prefix(void* k_cache, void* vt_cache, void* k_cache_lo, void* vt_cache_lo, int layers, int slots, int nh, int hd,
                                    int smax, int src, const int* dst, int n_dst, int n, llark_stream_t stream) {
    LLARK_REQUIRE(k_cache && vt_cache && dst && (k_cache_lo == nullptr) == (vt_cache_lo == nullptr), "kv_copy_prefix: null pointer, or one lo plane only");
    LLARK_REQUIRE(layers > 0 && slots > 0 && nh > 0 && smax > 0 && (long)layers * nh <= 65535, "kv_copy_prefix: bad shape layers=%d slots=%d nh=%d smax=%d",
                  layers, slots, nh, smax);
    LLARK_REFUSE(hd == 128 && smax % 8 == 0, "kv_copy_prefix: head_dim 128 and smax %% 8 == 0 required (hd=%d smax=%d)", hd, smax);
    LLARK_REFUSE(n >= 1 && n <= smax, "kv_copy_prefix: n=%d outside 1 .. smax=%d", n, smax);
    LLARK_REFUSE(n_dst >= 1 && n_dst <= COPY_MAX_DST, "kv_copy_prefix: %d destinations (1 .. %d)", n_dst, COPY_MAX_DST);
    LLARK_REQUIRE(src >= 0 && src < slots, "kv_copy_prefix: src=%d outside the %d slots", src, slots);
    CopyDst d;
    d.n = n_dst;
    for (int i = 0; i < n_dst; ++i) {
        LLARK_REQUIRE(dst[i] >= 0 && dst[i] < slots, "kv_copy_prefix: dst[%d]=%d outside the %d slots", i, dst[i], slots);
        LLARK_REFUSE(dst[i] != src, "kv_copy_prefix: src slot %d is among the destinations", src);
        for (int j = 0; j < i; ++j) LLARK_REFUSE(dst[j] != dst[i], "kv_copy_prefix: slot %d twice among the destinations", dst[i]);
        d.slot[i] = dst[i];
    }
    const long chunks = (long)n * 16 + 128L * ((n + 7) / 8);
    kv_copy_prefix_kernel<<<dim3(cdiv(chunks, 256), layers * nh), 256, 0, (hipStream_t)stream>>>((uint4*)k_cache, (uint4*)vt_cache, (uint4*)k_cache_lo,
                                                                                                  (uint4*)vt_cache_lo, slots, nh, smax, n, src, d);
    return check_launch("kv_copy_prefix");
}

extern "C" long long llark_attn_decode_shared_scratch_bytes(int batch, int nh) {
    if (batch <= 0 || nh <= 0) return 0;
    return SCRATCH_HEAD + (long long)batch * nh * GK_SPLITS * PART_LD * (long long)sizeof(float);
}

extern "C" int llark_attn_decode_rope_bf16_shared(const float* qkv, int batch, int nh, int hd, const int* pos_rows, const float* cos_t,
                                                  const float* sin_t, int max_pos, void* k_cache, void* vt_cache, void* k_cache_lo,
                                                  void* vt_cache_lo, int smax, void* out, void* out_lo, const int* groups, int n_groups,
                                                  const int* slot_shared, void* scratch, long long scratch_bytes, llark_stream_t stream) {
    const char* name = "attn_decode_rope_shared";
    LLARK_REQUIRE(qkv && pos_rows && cos_t && sin_t && k_cache && vt_cache && out && slot_shared && scratch && (groups || n_groups == 0),
                  "%s: null pointer", name);
    LLARK_REFUSE(hd == 128, "%s: head_dim must be 128 (Llama-2), got %d", name, hd);
    LLARK_REQUIRE((k_cache_lo == nullptr) == (vt_cache_lo == nullptr) && (k_cache_lo == nullptr) == (out_lo == nullptr),
                  "%s: give all lo planes (fp32-class mode) or none", name);
    LLARK_REQUIRE(batch > 0 && nh > 0 && smax > 0 && smax % 8 == 0 && smax <= max_pos && batch <= 65535,
                  "%s: bad shape batch=%d nh=%d smax=%d max_pos=%d", name, batch, nh, smax, max_pos);
    LLARK_REFUSE(n_groups >= 0 && n_groups <= batch, "%s: %d groups for %d slots", name, n_groups, batch);
    LLARK_REQUIRE(((uintptr_t)scratch & 15) == 0 && scratch_bytes >= llark_attn_decode_shared_scratch_bytes(batch, nh),
                  "%s: scratch must be 16-byte aligned and hold llark_attn_decode_shared_scratch_bytes = %lld bytes (got %lld)", name,
                  llark_attn_decode_shared_scratch_bytes(batch, nh), scratch_bytes);
    const size_t lds = (size_t)smax * sizeof(float);
    LLARK_REFUSE(lds <= 128 * 1024, "%s: context too long for the LDS score buffer (smax=%d)", name, smax);
    const float scale = (float)(1.0 / sqrt((double)hd));
    int* status = (int*)scratch;
    float* part = (float*)((char*)scratch + SCRATCH_HEAD);
    hipStream_t st = (hipStream_t)stream;
    if (n_groups > 0)
        attn_group_kernel<<<dim3(nh, n_groups, GK_SPLITS), 256, 0, st>>>(qkv, (const bf16_t*)k_cache, (const bf16_t*)vt_cache, (const bf16_t*)k_cache_lo,
                                                                         (const bf16_t*)vt_cache_lo, batch, nh, smax, scale, pos_rows, cos_t, sin_t, groups,
                                                                         slot_shared, status, part);
    static PerDeviceOnce once;
    const bool first = once.first();
    if (lds > 48 * 1024 && (first || (int)lds > once.slot())) {
        (void)hipFuncSetAttribute((const void*)attn_slot_kernel<4, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        (void)hipFuncSetAttribute((const void*)attn_slot_kernel<16, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        once.slot() = (int)lds;
    }
    auto launch = [&](auto kern, int threads) {
        kern<<<dim3(nh, batch), threads, lds, st>>>((bf16_t*)k_cache, (bf16_t*)vt_cache, (bf16_t*)k_cache_lo, (bf16_t*)vt_cache_lo, (bf16_t*)out,
                                                    (bf16_t*)out_lo, nh, smax, scale, pos_rows, qkv, cos_t, sin_t, slot_shared, status, part);
    };
    if ((long)nh * batch < 256) launch(attn_slot_kernel<16, 4>, 1024);       // the wave counts of the rows form
    else launch(attn_slot_kernel<4, 8>, 256);
    return check_launch(name);
}
