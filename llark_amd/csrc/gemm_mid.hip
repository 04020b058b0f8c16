// Mid-M GEMM for the ragged decode step with 17 .. 64 slots (include/llark_hip.h, llark_gemm16_mid): HBM-bound weight streaming with
// the activation rows shared through LDS.
//   c[m][n] = (a_hi [+ a_lo]) . wt^T, wt row-major bf16 [n][ldw] -- the tensors the M <= 16 skinny kernel (gemm.hip) reads.
// Workgroup = WAVES waves owning BN = 32 WAVES weight rows (128 in the bf16 flow, 256 in the split flow) x one K slice; wave w owns 32 of
// them (two 16-row MFMA tiles) against all <= 64 activation rows (four 16-row tiles): 8 accumulator tiles.  The weights are not shared
// between waves and go HBM -> VGPR, one 128-k round ahead; the activation chunk ([<= 64 rows][128 k] per plane) is shared by every
// wave, so it is staged through LDS in full lines -- 16 consecutive lanes fetch the 256 bytes of one row -- and read back as MFMA
// fragments with ds_read_b128 from rows padded to 272 bytes (conflict-free).  Activation bytes out of L2 per workgroup are
// m planes / BN of its weight bytes: 1/2 at m = 64 in both flows.
// v_mfma_f32_16x16x32_bf16 with the WEIGHTS as the first operand: lane (c = lane & 15, g = lane >> 4) ends up with
// C[m = 16 mt + c][n = tile row 0 + 4 g + r], r = 0 .. 3 -- four consecutive columns of one output row.  Inside a 64-k chunk lane
// group g contributes k = 16 g .. 16 g + 15 (two MFMAs of 8) for BOTH operands, so a lane's weight load is 32 contiguous bytes and four
// lanes cover a whole 128-byte line; the contraction does not care about the order of k.
// K split: (n / BN) x splits workgroups, about 0.5 .. 1 x 256; the split count depends on (n, kp, flow) only, never on m, and every
// output row is a function of its own activation row alone, so row r's bits do not depend on m or on the other rows.  splits > 1:
// fp32 partials [split][m][npad] in caller-owned scratch, summed in a fixed order by a second launch that applies the epilogue
// (the llark_lora_down form: no atomics, no waiting).
#include "common.h"
#include "gemm_core.h"

namespace llark {

constexpr int MID_BK = 128;                  // k per round (one barrier pair)
constexpr int MID_ROWB = 2 * MID_BK + 16;    // LDS bytes per activation row: 68 dwords, lane c starts at bank 4 c
constexpr int MID_MAX_SPLITS = 8;

struct MidParams {
    const bf16_t* ahi;
    const bf16_t* alo;
    const bf16_t* wt;
    const float* bias;
    float* c;
    const float* resid;
    bf16_t* ohi;
    bf16_t* olo;
    float* scratch;
    int lda, ldw, ldc, ldr, ldo, m, n, kp, npad;
};

__device__ __forceinline__ f32x4_t mid_mfma(uint4 w, bf16x8_t a, f32x4_t acc) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, w), a, acc, 0, 0, 0);
}

// the epilogue of one output row's four consecutive values v (gate) / u (up, SwiGLU only) at output column oc
template <int EPI>
__device__ __forceinline__ void mid_store(const MidParams& p, int row, int oc, const float (&v)[4], const float (&u)[4]) {
    const int nout = IS_SWIGLU(EPI) ? (p.n >> 1) : p.n;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = oc + j;
        if (col >= nout) continue;
        if (EPI == EPI_F32) {
            p.c[(size_t)row * p.ldc + col] = v[j] + (p.bias ? p.bias[col] : 0.0f);
        } else if (EPI == EPI_RESID) {
            p.c[(size_t)row * p.ldc + col] = p.resid[(size_t)row * p.ldr + col] + (v[j] + (p.bias ? p.bias[col] : 0.0f));
        } else {
            const float a = silu(v[j]) * u[j];
            const bf16_t hi = (bf16_t)a;
            p.ohi[(size_t)row * p.ldo + col] = hi;
            if (EPI == EPI_SWIGLU_SPLIT) p.olo[(size_t)row * p.ldo + col] = (bf16_t)(a - (float)hi);
        }
    }
}

template <int WAVES, bool SPLIT, int EPI>
__global__ __launch_bounds__(WAVES * 64) void gemm_mid_kernel(const MidParams p) {
    constexpr int T = WAVES * 64, BN = WAVES * 32, PLANES = SPLIT ? 2 : 1;
    constexpr int PIECES = PLANES * 64 * 16 / T;                 // 16-byte pieces of a round's activation chunk per thread
    static_assert(PIECES * T == PLANES * 64 * 16 && PIECES == 4, "4 waves per plane");
    __shared__ __attribute__((aligned(16))) unsigned char lds[PLANES * 64 * MID_ROWB];
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int mtiles = (p.m + 15) >> 4;
    // the wave's two weight-row tiles.  plain: rows n0 + 32 w + 16 t.  SwiGLU: gate rows 64 q + 16 h .., up rows 64 q + 32 + 16 h ..
    int wrow[2], ocol0;
    if (IS_SWIGLU(EPI)) {
        const int q = blockIdx.x * (BN / 64) + (w >> 1), h = w & 1;
        wrow[0] = 64 * q + 16 * h;
        wrow[1] = wrow[0] + 32;
        ocol0 = 32 * q + 16 * h;
    } else {
        wrow[0] = blockIdx.x * BN + 32 * w;
        wrow[1] = wrow[0] + 16;
        ocol0 = wrow[0];
    }
    // this workgroup's K slice: whole rounds, the last one possibly short (kp % 32 == 0)
    const int rounds = (p.kp + MID_BK - 1) / MID_BK;
    const int S = gridDim.y, s = blockIdx.y;
    const int kb = (int)((long)s * rounds / S) * MID_BK;
    const int ke = min(p.kp, (int)((long)(s + 1) * rounds / S) * MID_BK);
    const bf16_t* wp[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int r = min(wrow[t] + c, p.n - 1);                  // rows past the end re-read the last one; they are never stored
        wp[t] = p.wt + (size_t)r * p.ldw + 16 * g;
    }
    // Two-level accumulation.  One long fp32 MFMA chain over K = 4096 rounds once per instruction at the magnitude of the running sum:
    // measured 4e-6 absolute on sums of magnitude 3, which SwiGLU multiplies by a partner of magnitude ~10 -- more than its hi / lo
    // output planes resolve.  So the hi-plane products of ONE 128-k round go through a short fresh fp32 chain (racc: 4 adds at a
    // small magnitude) that is then added to a double accumulator; the lo-plane products (2^-9 of the hi ones) keep an fp32 chain
    // of their own, whose roundings are far below everything else.  One rounding to fp32 at the end.
    double accd[4][2][4];
    f32x4_t accl[4][2];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            accl[mt][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < 4; ++r) accd[mt][t][r] = 0.0;
        }
    // this thread's four 16-byte pieces of a round's activation chunk: piece idx = (plane * 64 + row) * 16 + piece of the row
    const bf16_t* asrc[PIECES];
    bool alive[PIECES];
#pragma unroll
    for (int j = 0; j < PIECES; ++j) {
        const int idx = threadIdx.x + j * T;
        const int plane = idx >> 10, row = (idx >> 4) & 63;
        alive[j] = row < p.m;                                     // rows >= m load nothing and stage zeros
        asrc[j] = ((SPLIT && plane) ? p.alo : p.ahi) + (size_t)(alive[j] ? row : 0) * p.lda + (idx & 15) * 8;
    }
    uint4 ar0, ar1, ar2, ar3, wc[2][2][2], wn[2][2][2];
    // software pipeline with one load site: iteration k0 stages and multiplies round k0 while round k0 + MID_BK is in flight
    for (int k0 = kb - MID_BK; k0 < ke; k0 += MID_BK) {
        const bool cur = k0 >= kb;
        if (cur) {
            if (k0 != kb) __syncthreads();                        // every wave is done reading the previous round's chunk
            const int i0 = threadIdx.x;
            *(uint4*)(lds + ((i0 + 0 * T) >> 4) * MID_ROWB + (i0 & 15) * 16) = ar0;
            *(uint4*)(lds + ((i0 + 1 * T) >> 4) * MID_ROWB + (i0 & 15) * 16) = ar1;
            *(uint4*)(lds + ((i0 + 2 * T) >> 4) * MID_ROWB + (i0 & 15) * 16) = ar2;
            *(uint4*)(lds + ((i0 + 3 * T) >> 4) * MID_ROWB + (i0 & 15) * 16) = ar3;
            __syncthreads();
        }
        const int kn = k0 + MID_BK;
        if (kn < ke) {                                            // k >= ke (a short last round) loads nothing: zeros
            const int ka = kn + (threadIdx.x & 15) * 8;
            ar0 = ar1 = ar2 = ar3 = make_uint4(0, 0, 0, 0);
            if (ka < ke) {
                if (alive[0]) ar0 = *(const uint4*)(asrc[0] + kn);
                if (alive[1]) ar1 = *(const uint4*)(asrc[1] + kn);
                if (alive[2]) ar2 = *(const uint4*)(asrc[2] + kn);
                if (alive[3]) ar3 = *(const uint4*)(asrc[3] + kn);
            }
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const int k = kn + 64 * q;
                    wn[t][q][0] = wn[t][q][1] = make_uint4(0, 0, 0, 0);
                    if (k + 16 * g < ke) {
                        wn[t][q][0] = *(const uint4*)(wp[t] + k);
                        wn[t][q][1] = *(const uint4*)(wp[t] + k + 8);
                    }
                }
        }
        if (cur) {
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                if (mt < mtiles) {
                    f32x4_t racc[2] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const unsigned char* ap = lds + (mt * 16 + c) * MID_ROWB + q * 128 + g * 32;
                        const bf16x8_t a0 = *(const bf16x8_t*)ap, a1 = *(const bf16x8_t*)(ap + 16);
#pragma unroll
                        for (int t = 0; t < 2; ++t) {
                            racc[t] = mid_mfma(wc[t][q][0], a0, racc[t]);
                            racc[t] = mid_mfma(wc[t][q][1], a1, racc[t]);
                        }
                        if (SPLIT) {
                            const bf16x8_t l0 = *(const bf16x8_t*)(ap + 64 * MID_ROWB), l1 = *(const bf16x8_t*)(ap + 64 * MID_ROWB + 16);
#pragma unroll
                            for (int t = 0; t < 2; ++t) {
                                accl[mt][t] = mid_mfma(wc[t][q][0], l0, accl[mt][t]);
                                accl[mt][t] = mid_mfma(wc[t][q][1], l1, accl[mt][t]);
                            }
                        }
                    }
#pragma unroll
                    for (int t = 0; t < 2; ++t)
#pragma unroll
                        for (int r = 0; r < 4; ++r) accd[mt][t][r] += (double)racc[t][r];
                }
            }
        }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                wc[t][q][0] = wn[t][q][0];
                wc[t][q][1] = wn[t][q][1];
            }
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const int row = mt * 16 + c;
        if (mt >= mtiles || row >= p.m) continue;
        f32x4_t acc[2];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[t][r] = (float)(SPLIT ? accd[mt][t][r] + (double)accl[mt][t][r] : accd[mt][t][r]);
        if (S > 1) {                                              // partial sums of this K slice, every column of the padded row
            float* part = p.scratch + ((size_t)s * p.m + row) * p.npad;
#pragma unroll
            for (int t = 0; t < 2; ++t) *(f32x4_t*)(part + wrow[t] + 4 * g) = acc[t];
        } else if (IS_SWIGLU(EPI)) {
            const float v[4] = {acc[0][0], acc[0][1], acc[0][2], acc[0][3]};
            const float u[4] = {acc[1][0], acc[1][1], acc[1][2], acc[1][3]};
            mid_store<EPI>(p, row, ocol0 + 4 * g, v, u);
        } else {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const float v[4] = {acc[t][0], acc[t][1], acc[t][2], acc[t][3]};
                mid_store<EPI>(p, row, ocol0 + 16 * t + 4 * g, v, v);
            }
        }
    }
}

// out <- epilogue(sum over the K splits, fixed order): one thread per four output columns of one row
template <int EPI>
__global__ __launch_bounds__(256) void gemm_mid_finish_kernel(const MidParams p, int nsplit) {
    const int nout = IS_SWIGLU(EPI) ? (p.n >> 1) : p.n;
    const int per_row = (nout + 3) >> 2;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)p.m * per_row) return;
    const int row = (int)(i / per_row), oc = (int)(i % per_row) * 4;
    const int pcol = IS_SWIGLU(EPI) ? 64 * (oc >> 5) + (oc & 31) : oc;          // gate columns of [gate 32 | up 32]
    const size_t stride = (size_t)p.m * p.npad;
    const float* src = p.scratch + (size_t)row * p.npad + pcol;
    f32x4_t sv = *(const f32x4_t*)src, su = sv;
    if (IS_SWIGLU(EPI)) su = *(const f32x4_t*)(src + 32);
    for (int s = 1; s < nsplit; ++s) {
        sv += *(const f32x4_t*)(src + s * stride);
        if (IS_SWIGLU(EPI)) su += *(const f32x4_t*)(src + s * stride + 32);
    }
    const float v[4] = {sv[0], sv[1], sv[2], sv[3]};
    const float u[4] = {su[0], su[1], su[2], su[3]};
    mid_store<EPI>(p, row, oc, v, u);
}

static inline int mid_bn(int split) { return split ? 256 : 128; }

// K splits: fill about 0.5 .. 1 x 256 CUs, at least two rounds per slice.  A function of (n, kp, flow) only -- never of m.
static inline int mid_splits(int n, int kp, int split) {
    const int colblocks = cdiv(n, mid_bn(split)), rounds = cdiv(kp, MID_BK);
    int s = 256 / colblocks;
    if (s > MID_MAX_SPLITS) s = MID_MAX_SPLITS;
    if (s > rounds / 2) s = rounds / 2;
    return s < 1 ? 1 : s;
}

static inline bool mid_epilogue_ok(int e) { return e == EPI_F32 || e == EPI_RESID || e == EPI_SWIGLU16 || e == EPI_SWIGLU_SPLIT; }

static inline bool mid_shape_ok(int m, int n, int kp, int epilogue) {
    return m >= 17 && m <= 64 && n > 0 && kp > 0 && kp % 32 == 0 && mid_epilogue_ok(epilogue) && (!IS_SWIGLU(epilogue) || n % 64 == 0);
}

template <bool SPLIT, int EPI>
static int launch_mid(const MidParams& p, int splits, hipStream_t s) {
    constexpr int WAVES = SPLIT ? 8 : 4;
    dim3 grid(p.npad / (WAVES * 32), splits);
    gemm_mid_kernel<WAVES, SPLIT, EPI><<<grid, WAVES * 64, 0, s>>>(p);
    int rc = check_launch("gemm16_mid");
    if (rc || splits == 1) return rc;
    const long long items = (long long)p.m * (((IS_SWIGLU(EPI) ? p.n / 2 : p.n) + 3) / 4);
    gemm_mid_finish_kernel<EPI><<<cdiv(items, 256), 256, 0, s>>>(p, splits);
    return check_launch("gemm16_mid (finish)");
}

}  // namespace llark

using namespace llark;

extern "C" long long llark_gemm16_mid_scratch_bytes(int m, int n, int kp, int split, int epilogue) {
    if (!mid_shape_ok(m, n, kp, epilogue)) return 0;
    const int bn = mid_bn(split);
    return (long long)mid_splits(n, kp, split) * m * ((long long)cdiv(n, bn) * bn) * 4;
}

extern "C" int llark_gemm16_mid(int dtype, int split, int epilogue, const void* a_hi, const void* a_lo, int lda, const void* wt, int ldw,
                                const float* bias, int m, int n, int kp, float* c, int ldc, const float* resid, int ldr, void* out_hi,
                                void* out_lo, int ldo, void* scratch, long long scratch_bytes, llark_stream_t stream) {
    if (dtype != LLARK_BF16) {
        set_error("gemm16_mid: dtype=%d: only LLARK_BF16 is compiled", dtype);
        return LLARK_ERR_UNSUPPORTED;
    }
    LLARK_REQUIRE(mid_epilogue_ok(epilogue), "gemm16_mid: epilogue=%d is not F32, RESID, SWIGLU16 or SWIGLU_SPLIT", epilogue);
    if (m < 17 || m > 64) {
        set_error("gemm16_mid: m=%d outside 17 .. 64 (llark_gemm16 takes the other row counts)", m);
        return LLARK_ERR_UNSUPPORTED;
    }
    LLARK_REQUIRE(n > 0, "gemm16_mid: n=%d must be positive", n);
    LLARK_REQUIRE(kp > 0 && kp % 32 == 0, "gemm16_mid: kp=%d must be a positive multiple of 32 (zero-pad K)", kp);
    LLARK_REQUIRE(a_hi != nullptr, "gemm16_mid: a_hi is null");
    LLARK_REQUIRE(wt != nullptr, "gemm16_mid: wt is null");
    LLARK_REQUIRE(!split || a_lo != nullptr, "gemm16_mid: a_lo is null in the split flow");
    LLARK_REQUIRE(lda % 8 == 0 && lda >= kp, "gemm16_mid: lda=%d must be >= kp and a multiple of 8", lda);
    LLARK_REQUIRE(ldw % 8 == 0 && ldw >= kp, "gemm16_mid: ldw=%d must be >= kp and a multiple of 8", ldw);
    LLARK_REQUIRE(((uintptr_t)a_hi & 15) == 0 && ((uintptr_t)wt & 15) == 0 && ((uintptr_t)a_lo & 15) == 0,
                  "gemm16_mid: a_hi / a_lo / wt must be 16-byte aligned");
    if (IS_SWIGLU(epilogue)) {
        LLARK_REQUIRE(n % 64 == 0, "gemm16_mid: n=%d must be a multiple of 64 for a SwiGLU epilogue", n);
        LLARK_REQUIRE(out_hi != nullptr && ldo >= n / 2, "gemm16_mid: out_hi is null or ldo=%d < n / 2", ldo);
        LLARK_REQUIRE(epilogue != EPI_SWIGLU_SPLIT || out_lo != nullptr, "gemm16_mid: out_lo is null for SWIGLU_SPLIT");
    } else {
        LLARK_REQUIRE(c != nullptr && ldc >= n, "gemm16_mid: c is null or ldc=%d < n", ldc);
        if (epilogue == EPI_RESID) LLARK_REQUIRE(resid != nullptr && ldr >= n, "gemm16_mid: resid is null or ldr=%d < n", ldr);
    }
    const long long need = llark_gemm16_mid_scratch_bytes(m, n, kp, split, epilogue);
    LLARK_REQUIRE(scratch != nullptr && ((uintptr_t)scratch & 15) == 0, "gemm16_mid: scratch is null or not 16-byte aligned");
    LLARK_REQUIRE(scratch_bytes >= need, "gemm16_mid: scratch_bytes=%lld, llark_gemm16_mid_scratch_bytes asks for %lld", scratch_bytes, need);
    MidParams p = {};
    p.ahi = (const bf16_t*)a_hi; p.alo = split ? (const bf16_t*)a_lo : nullptr; p.wt = (const bf16_t*)wt; p.bias = bias;
    p.c = c; p.resid = resid; p.ohi = (bf16_t*)out_hi; p.olo = (bf16_t*)out_lo; p.scratch = (float*)scratch;
    p.lda = lda; p.ldw = ldw; p.ldc = ldc; p.ldr = ldr; p.ldo = ldo; p.m = m; p.n = n; p.kp = kp;
    const int bn = mid_bn(split);
    p.npad = cdiv(n, bn) * bn;
    const int splits = mid_splits(n, kp, split);
    hipStream_t s = (hipStream_t)stream;
#define MID(E)                                                                                  \
    case E:                                                                                     \
        return split ? launch_mid<true, E>(p, splits, s) : launch_mid<false, E>(p, splits, s);
    switch (epilogue) {
        MID(EPI_F32)
        MID(EPI_RESID)
        MID(EPI_SWIGLU16)
        MID(EPI_SWIGLU_SPLIT)
    }
#undef MID
    return LLARK_ERR_INVALID;
}
