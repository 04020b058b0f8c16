/* llark_hip.h -- C ABI of libllark_hip.so: the MI355X (gfx950) implementation of LLark's
 * audio-encoder -> LLM hot path.
 *
 * The reference (spotify-research/llark) has NO native/FFI boundary: its hot path is Python calling
 * third-party CUDA libraries.  This header is therefore the boundary a
 * maintainer of the reference would bind (via ctypes) underneath the
 * reference's own Python module interfaces.  Each entry point names the reference call site it
 * replaces.  Conventions:
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless stated otherwise;
 *   - every function returns LLARK_OK (0) or a negative error code, never throws, and enqueues its
 *     work on `stream` (a hipStream_t passed as void*);
 *   - compute entry points never allocate and keep no hidden device state: the only functions that
 *     allocate are the two object constructors llark_workspace_create (1 KiB of device counters the
 *     persistent GEMM kernels synchronise through) and llark_vqvae_plan_create (a host-side launch
 *     list); both objects are owned, passed in and destroyed by the caller;
 *   - llark_last_error() returns a thread-local human-readable message for the last failure;
 *   - re-entrant per stream: a workspace serves ONE stream at a time (launches that share it are
 *     ordered on that stream); create one per (device, stream).  The remaining process-level state is
 *     immutable once set: per-kernel "dynamic LDS size raised" flags and occupancy figures of the code
 *     object, the CU count of each device ordinal.  Scratch memory a kernel needs beyond the workspace is
 *     passed in by the caller (llark_gemm16_fragw_sk);
 *   - the library reads NO environment variables: every choice it makes is a function of its arguments (tile variants,
 *     K-splitting, kernel forms); the only getenv in the sources is LLARK_LO8_PROF_BUF inside `#ifdef LLARK_LO8_PROF`,
 *     a cycle-counter build (scripts/build_lo8_prof.sh) that is never shipped.  The knobs of the Python host layer
 *     (LLARK_PRIOR_PRECISION, LLARK_LLM_PRECISION, LLARK_HIP_LIB, ...) are listed in INTEGRATION.md.
 */
#ifndef LLARK_HIP_H
#define LLARK_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* llark_stream_t; /* hipStream_t */

enum {
    LLARK_OK = 0,
    LLARK_ERR_INVALID = -1,     /* bad argument (shape, null pointer, alignment) */
    LLARK_ERR_UNSUPPORTED = -2, /* shape outside what is compiled */
    LLARK_ERR_LAUNCH = -3       /* HIP launch / runtime error */
};

enum { LLARK_F16 = 0, LLARK_BF16 = 1 };

/* epilogues of llark_gemm16 */
enum {
    LLARK_EPI_F32 = 0,         /* C = acc + bias                              (fp32 out)        */
    LLARK_EPI_RESID = 1,       /* C = R + (acc + bias)                        (fp32, C may alias R) */
    LLARK_EPI_QGELU_SPLIT = 2, /* g = x*sigmoid(1.702x), x = acc+bias -> hi/lo 16-bit planes     */
    LLARK_EPI_OUT16 = 3,       /* out = 16-bit(acc + bias)                                       */
    LLARK_EPI_SWIGLU16 = 4,    /* out = 16-bit(silu(gate) * up), W rows interleaved [32 gate|32 up] */
    LLARK_EPI_SPLIT16 = 5,     /* acc + bias -> hi/lo 16-bit planes                              */
    LLARK_EPI_SWIGLU_SPLIT = 6, /* silu(gate)*up -> hi/lo 16-bit planes (fp32-class Llama mode)       */
    LLARK_EPI_QGELU_SPLIT8 = 7 /* llark_gemm16_lo8 only: g -> fp16 hi plane + e4m3 low plane          */
};

/* Caller-owned workspace of the persistent GEMM kernels (per-XCD chunk counters; see the conventions
 * above).  create() binds to the CURRENT device; returns NULL on failure (llark_last_error()). */
typedef struct llark_workspace* llark_workspace_t;
llark_workspace_t llark_workspace_create(void);
int llark_workspace_destroy(llark_workspace_t ws);

int llark_version(void);
const char* llark_last_error(void);
/* device properties probe: returns CU count (>0) or a negative error; arch_name receives e.g. "gfx950". */
int llark_device_info(int device, char* arch_name, int arch_name_len);

/* ---------------------------------------------------------------------------------------------
 * Audio front end: the sample-rate conversion inside `lr.load(fpath, sr=44100)` at jukebox/main.py:31 (librosa 0.7.2
 * -- the version openai/jukebox @ 08efbbc pins, docker/jukebox-embed.dockerfile:56 -- resamples with resampy's
 * "kaiser_best" band-limited sinc interpolation).  HOST entry point on HOST pointers, no stream, no device work:
 * x [n_in] -> y [n_out] at ratio = sr_new / sr_orig; win / dwin [nwin] = right half of the interpolation window with
 * num_table samples per zero crossing (scaled by ratio when ratio < 1) and its forward difference.
 * ------------------------------------------------------------------------------------------- */
int llark_resample_sinc_host(const float* x, int64_t n_in, double ratio, const double* win, const double* dwin, int nwin,
                             int num_table, float* y, int64_t n_out);

/* FLAC streams (the other container libsndfile -- `lr.load` at jukebox/main.py:31, `sf.read` at m2t/gcs_utils.py:123 -- reads without
 * further dependencies), decoded from memory on the HOST.  info: STREAMINFO fields (total_samples 0 = not recorded).  decode:
 * interleaved int32 [frames][channels] into out (NULL = count only), at most cap_frames frames; every frame's CRC-8 / CRC-16 is
 * checked and, with verify_md5, the MD5 signature of the decoded samples against STREAMINFO's (a FLAC stream certifies its decode). */
int llark_flac_info_host(const uint8_t* data, int64_t n, int* sample_rate, int* channels, int* bits_per_sample, int64_t* total_samples);
int llark_flac_decode_host(const uint8_t* data, int64_t n, int32_t* out, int64_t cap_frames, int64_t* decoded_frames, int verify_md5);

/* ---------------------------------------------------------------------------------------------
 * Jukebox VQ-VAE level-2 encoder: replaces `vqvae.encode(...)` at jukebox/main.py:61
 * (upstream openai/jukebox vqvae/encdec.py EncoderConvBlock, resnet.py ResConv1DBlock,
 * bottleneck.py BottleneckBlock.encode).  Activations: fp32 [n][C][T] (torch NCT).
 * ------------------------------------------------------------------------------------------- */
/* w[cout][cin][k] (torch Conv1d.weight) -> wp[k][cin][cout] (kernel layout). */
int llark_pack_conv_weight(const float* w, float* wp, int cout, int cin, int k, llark_stream_t stream);
/* nn.Conv1d forward; built shapes: (cin in {1,32,64}, cout 32, k4 s2) and (cin 32, cout 64, k3 s1). */
int llark_conv1d_f32(const float* x, int n, int cin, int tin, const float* wp, const float* bias, int cout, int k,
                     int stride, int pad, int dil, float* y, int tout, llark_stream_t stream);
/* ResConv1DBlock: y = x + conv1x1(relu(conv3(relu(x), dilation))); c must be 32. */
int llark_resblock_f32(const float* x, int n, int c, int t, const float* w1p, const float* b1, const float* w2p,
                       const float* b2, int dil, float* y, llark_stream_t stream);
/* kk[j] = sum_c k[j][c]^2 */
int llark_codebook_norms_f32(const float* k, int bins, int emb, float* kk, llark_stream_t stream);
/* BottleneckBlock.quantise: codes[n][t] = argmin_j |x[n][:,t] - k[j]|^2 (first minimum); min_dist optional. */
int llark_codebook_argmin(const float* x, int n, int emb, int t, const float* k, const float* kk, int bins,
                          int64_t* codes, float* min_dist, llark_stream_t stream);
/* The whole level-2 encode of jukebox/main.py:61 (`vqvae.encode(x)` -> zs[-1]) as ONE call: a plan lists the layers
 * (device pointers to llark_pack_conv_weight outputs and biases stay owned by the caller), llark_vqvae_encode runs
 * conv / residual blocks through two ping-pong buffers and finishes with the codebook search. */
void* llark_vqvae_plan_create(void);
void llark_vqvae_plan_destroy(void* plan);
int llark_vqvae_plan_add_conv(void* plan, const float* wp, const float* bias, int cin, int cout, int k, int stride, int pad);
int llark_vqvae_plan_add_resblock(void* plan, const float* w1p, const float* b1, const float* w2p, const float* b2, int width, int dil);
int llark_vqvae_encode(void* plan, const float* audio, int n, int t, float* buf0, float* buf1, long long buf_elems,
                       const float* codebook, const float* kk, int bins, int64_t* codes, int* t_out, llark_stream_t stream);
/* Fused stage of the level encoder on the 16-bit matrix cores (csrc/vqvae_fused.hip): one `down_t` step of upstream
 * EncoderConvBlock -- Conv1d(cin -> 32, k = 4, stride 2, pad 1), `depth` ResConv1DBlocks (dilations dil[0 .. depth), a HOST array),
 * optionally the block's output Conv1d(32 -> 64, k = 3, pad 1) -- in ONE launch, activations resident in LDS / registers, every
 * product as three fp16 MFMA passes over hi / lo splits of BOTH operands (fp32-class; the cin = 1 convolution stays an exact fp32
 * fmaf chain).  Replaces the same call site as llark_vqvae_encode (jukebox/main.py:61 -> VQVAE.encode); VQ codes equal the fp32
 * path's on every fixture, activations agree to ~1e-6 relative instead of bit for bit (the exact per-layer kernels stay).
 *   input : cin == 1: audio fp32 [n][tin];  cin == 32 / 64: planes in_hi / in_lo fp16 [n][tin][cin] (= a previous stage's output)
 *   weights: w0_f32 (cin == 1) = llark_pack_conv_weight layout [4][1][32]; every other weight operand = the hi / lo outputs of
 *            llark_vqvae_pack_frag16: w0 (32, cin, 4), wr = depth x [conv3 (32, 32, 3) | 1x1 (32, 32, 1) with perm1x1 = 1] concatenated
 *            (8 k-steps of 1 KiB per block and plane), wo (64, 32, 3) or NULL;  b0 [32], br [depth][2][32] (b1, b2), bo [64]
 *   output: planes out_hi / out_lo [n][tin/2][C] and / or out_f32 [n][C][tin/2], C = 64 with the output conv else 32.
 *   wexp  : HOST array of 2 + 2 depth ints: the exp2 each weight tensor was packed with (strided conv; dilated conv, 1x1 per block;
 *           output conv; 0 where a tensor is not fragment-packed).
 * tin even; 1 <= depth <= 4; sum(dil) (+1 with the output conv) <= 48 (the window's halo) and each dilation <= 32 (the zero guard
 * rows a tap may reach beyond the window; LLARK_ERR_UNSUPPORTED above that). */
int llark_vqvae_stage_f16x2(const float* audio, const void* in_hi, const void* in_lo, int n, int cin, int tin, const float* w0_f32,
                            const void* w0_hi, const void* w0_lo, const float* b0, const void* wr_hi, const void* wr_lo,
                            const float* br, int depth, const int* dil, const void* wo_hi, const void* wo_lo, const float* bo,
                            const int* wexp, void* out_hi, void* out_lo, float* out_f32, llark_stream_t stream);
/* Conv1d.weight fp32 [cout][cin][k] (cout % 32 == 0, cin % 16 == 0) -> MFMA A fragments of w 2^exp2, fp16 hi / lo planes of
 * (cout / 32) * (k * cin / 16) * 512 elements each; perm1x1 != 0 (k == 1, cin == 32): channels in accumulator-register order.
 * exp2: choose max|w| 2^exp2 in [2^13, 2^14] so that the low plane is a normal fp16 (unscaled it is subnormal and the pair carries
 * ~19 bits instead of 22). */
int llark_vqvae_pack_frag16(const float* w, int cout, int cin, int k, int perm1x1, int exp2, void* hi, void* lo, llark_stream_t stream);

/* Near-tie certificate for the fused encoder (round 4; same call site: jukebox/main.py:61 -> VQVAE.encode -> bottleneck.encode).
 * llark_codebook_argmin plus: every token whose best / second-best distance gap is below  |x| (tie_a sqrt(d_best) + tie_b |x|)  is
 * appended to flag_list (ids n_index * t + token, at most `cap`; *flag_count -- zeroed by this call -- keeps counting past cap so the
 * caller can detect an overflow).  An encoder-output error e moves the gap by <= 2 |e| |k_a - k_b| <= 4 |e| sqrt(d): tie_a = 4 |e| / |x|;
 * the fp32 rounding of the distance chains moves it by a few ulp of |x|^2: tie_b = c * 2^-23. */
int llark_codebook_argmin_tie(const float* x, int n, int emb, int t, const float* k, const float* kk, int bins, int64_t* codes,
                              float tie_a, float tie_b, int* flag_count, int* flag_list, int cap, llark_stream_t stream);
/* Exact fix-up of the flagged tokens: for flag_list[0 .. count) (count read back by the caller) gathers a window of `win_tokens`
 * tokens of audio around each token (start clamp(tok - halo_tokens, 0, t_tok - win_tokens): a window edge on a clip edge is the
 * clip edge), runs the plan's exact per-layer kernels on the `count` windows and overwrites codes[] of the flagged tokens with the
 * argmin of the exact value -- bit-equal to llark_vqvae_encode on the whole clip when halo_tokens covers the receptive field.
 * win [count][win_tokens * raw_to_tokens] fp32, col [count] int, buf0 / buf1 (>= count * 32 * win_tokens * raw_to_tokens / 2 floats
 * each): caller-owned scratch.  count <= 0 is a no-op. */
int llark_vqvae_fix_near_ties(void* plan, const float* audio, int n, int t_samples, int raw_to_tokens, const int* flag_list, int count,
                              int halo_tokens, int win_tokens, float* win, int* col, float* buf0, float* buf1, long long buf_elems,
                              const float* codebook, const float* kk, int bins, int64_t* codes, llark_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Jukebox top prior, only_encode: replaces `top_prior.prior.forward(...)` at jukebox/main.py:108
 * and the pooling at jukebox/main.py:113-167.
 * ------------------------------------------------------------------------------------------- */
int llark_prior_embed(const int64_t* z, int n, int t, int width, int bins, const float* x_emb, const float* pos_emb,
                      const float* x_cond, const float* y_cond, float* h, llark_stream_t stream);
/* The head of a forward in one pass: llark_prior_embed + llark_layernorm_split_f16 (gamma, beta: block 0's ln_0) + -- pred != NULL --
 * llark_ln_row_pred, every output (h, the planes, pred [n*t][2]) bit-equal to that sequence.  width % 8 == 0, width <= 8192, ldo % 8 == 0. */
int llark_prior_head(const int64_t* z, int n, int t, int width, int bins, const float* x_emb, const float* pos_emb,
                     const float* x_cond, const float* y_cond, const float* gamma, const float* beta, float eps, float* h,
                     void* out_hi, void* out_lo, int ldo, float* pred, llark_stream_t stream);
/* LayerNorm(width, eps) in fp32 -> fp16 hi/lo planes [rows][ldo].  width % 4 == 0, width <= 8192.
 * Precision of an fp16 hi/lo pair, here and wherever this header speaks of "22 bits" or "fp32-class": hi = fp16(x), lo = fp16(x - hi) is
 * within 2^-22 |x| of x only while lo is a NORMAL fp16, |x - hi| >= 2^-14, which |x| >= 2^-3 guarantees.  Below that lo is subnormal with
 * a spacing of 2^-24 and the pair carries an ABSOLUTE error of up to 2^-25 whatever |x| is:  |x - hi - lo| <= 2^-22 |x| + 2^-25.
 * (|x| > 65504 overflows the hi plane.)  Producers that must keep 22 bits on small values scale by a power of two first: llark_gemm16_ln_p. */
int llark_layernorm_split_f16(const float* x, int ldx, int rows, int width, const float* gamma, const float* beta,
                              float eps, void* out_hi, void* out_lo, int ldo, llark_stream_t stream);
/* FactoredAttention core (pattern 1 block, 2 transpose-block, 3 previous-block) on qkv [n*t][ldq] -> fp16 hi/lo planes [n*t][ldo].
 * q, k, v, the probabilities and the output are each carried as an fp16 hi/lo pair (three MFMA passes per product, lo.lo dropped), with
 * the precision stated above: softmax probabilities are almost always below 2^-3, so next to the relative 2^-22 terms every output
 * element carries a floor of  2^-25 (2 + sum_visible |v_jd|) + 2 B 2^-25 / sqrt(hd) max_j sum_d (|q_d| + |k_jd|),  B = sum_j p_j |v_jd|
 * (tests/prior_kernel_ref.py derives and measures it).  head_dim = n_state / heads even and <= 160, block_ctx = t / blocks <= 64,
 * blocks <= 64 or == 128, ldq >= 3 n_state and ldo >= n_state both even; LLARK_ERR_* before anything is launched otherwise. */
int llark_prior_attn(const float* qkv, int ldq, int n, int t, int n_state, int heads, int blocks, int pattern,
                     void* out_hi, void* out_lo, int ldo, llark_stream_t stream);
/* The same two producers in "lo8" mode (see llark_gemm16_lo8): fp16 hi plane [rows][ldo] + E4M3 low plane
 * [rows][ldo8] = fp8(sat((y - hi) * 2^sa)) in MFMA slot order; ldo8 in bytes, a multiple of 64 covering the width. */
int llark_layernorm_split_lo8(const float* x, int ldx, int rows, int width, const float* gamma, const float* beta,
                              float eps, void* out_hi, int ldo, void* out_lo8, int ldo8, int sa, llark_stream_t stream);
int llark_prior_attn_lo8(const float* qkv, int ldq, int n, int t, int n_state, int heads, int blocks, int pattern,
                         void* out_hi, int ldo, void* out_lo8, int ldo8, int sa, llark_stream_t stream);
/* AvgPool1d(frame_len, stride=frame_len, ceil_mode=False) over time: h [n][t][width] -> out [n][frames][width] */
int llark_pool_window(const float* h, int n, int t, int width, int frame_len, float* out, int frames,
                      llark_stream_t stream);
/* llark_pool_window moved in front of the last block's second MLP product (pooling is linear over rows): one pass over the fp32
 * stream h [n][t][width] and the fp16 planes g_hi / g_lo [n*t][ldg] (gwidth valid columns) writes pool_h [n*frames][width] -- bit-equal
 * to llark_pool_window -- and pg_hi / pg_lo [n*frames][ldg]: the window mean of float(hi) + float(lo), summed in fp32 in row order and
 * split again like the GEMM epilogues; columns [gwidth, ldg) are written as zeros.  Windows never cross a clip; rows past
 * frames * frame_len are not read.  width % 4 == 0, ldg % 8 == 0, pointers 16-byte aligned. */
int llark_pool_window_tail(const float* h, const void* g_hi, const void* g_lo, int n, int t, int width, int gwidth, int ldg,
                           int frame_len, int frames, float* pool_h, void* pg_hi, void* pg_lo, llark_stream_t stream);
/* acts[:len].mean(0): lens is a device int[n] (NULL -> t) */
int llark_pool_mean(const float* h, int n, int t, int width, const int* lens, float* out, llark_stream_t stream);
int llark_zero_pad16(void* plane, int rows, int ld, int from, llark_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * 16-bit MFMA GEMM with fp32 accumulation: replaces upstream Conv1D.forward (`addmm`) of the prior
 * (split hi/lo fp16 activations, fp32-class accuracy) and nn.Linear of Llama / mm_projector
 * (m2t/models/llamav2.py:79,133,312).  C[m,n] = (a_hi [+ a_lo])[m,k] . wt[n,k]^T (+ bias).
 * ------------------------------------------------------------------------------------------- */
int llark_gemm16(int dtype, int split, int epilogue, const void* a_hi, const void* a_lo, int lda, const void* wt,
                 int ldw, const float* bias, int m, int n, int kp, float* c, int ldc, const float* resid, int ldr,
                 void* out_hi, void* out_lo, int ldo, llark_stream_t stream);
/* Same with an explicit tile variant (tuning knob: 0, 1, 2, 11, 12, 20 = persistent 12; -1 = library default). All
 * variants compute the same product; kp must be a multiple of 64 for the BK=64 variants (11, 12, 20). */
int llark_gemm16_ex(int variant, int dtype, int split, int epilogue, const void* a_hi, const void* a_lo, int lda,
                    const void* wt, int ldw, const float* bias, int m, int n, int kp, float* c, int ldc, const float* resid,
                    int ldr, void* out_hi, void* out_lo, int ldo, llark_stream_t stream);
/* llark_gemm16_ex plus a workspace: only with one are the persistent, chunk-synchronous variants (20 = 128x256x64,
 * 30 = the 256x256x64 LDS-DMA ring of csrc/gemm256.hip, 31 = the 256x256x64 tile with phases over N and resident A
 * fragments of csrc/gemm256n.hip -- the default for the prior's M = clips x 8192 split-fp16 products) chosen or honoured;
 * without, such requests run variant 12.  All variants produce bit-identical results. */
int llark_gemm16_ws(int variant, int dtype, int split, int epilogue, const void* a_hi, const void* a_lo, int lda,
                    const void* wt, int ldw, const float* bias, int m, int n, int kp, float* c, int ldc, const float* resid,
                    int ldr, void* out_hi, void* out_lo, int ldo, llark_workspace_t ws, llark_stream_t stream);

/* LayerNorm folded into the epilogues of the products around it (round 4; replaces the F.layer_norm + Conv1D pairs of upstream
 * transformer.py ResAttnBlock -- `attn(ln_0(x))`, `mlp(ln_1(x + a))` -- reached from jukebox/main.py:108).  One entry point, two roles:
 *   producer (ln_part != NULL, LLARK_EPI_RESID): c = resid + a.wt^T + bias as llark_gemm16_ws, plus out_hi / out_lo [m][ldo] = hi / lo of
 *            c * ln_vec[n] (ln_vec = gamma of the LayerNorm that follows) and ln_part [m][2 * ceil(n / 256)][2] = (sum, sum of squares) of c
 *            per 128-column slice; llark_ln_stats_finalize reduces them, in slice order, to ln_stat [m][2] = (mean, 1 / sqrt(var + eps));
 *   consumer (ln_stat != NULL, LLARK_EPI_F32 or LLARK_EPI_QGELU_SPLIT): a_hi / a_lo = those planes;
 *            out = rstd_m * (acc - mean_m * ln_vec[n]) + bias[n]  with ln_vec[n] = sum_k gamma_k wt[n][k], bias[n] = sum_k beta_k wt[n][k] + b[n]
 *            (both precomputed by the caller): == Conv1D(layer_norm(x)) without the LayerNorm kernel's read and write of x.
 * Split operands only; shapes the 256x256 tile does not take (llark_gemm16_ln_takes() == 0) return LLARK_ERR_UNSUPPORTED before anything
 * is launched.  Partial sums are written, never accumulated atomically: results are run-to-run bit-equal. */
int llark_gemm16_ln_takes(int m, int n, int kp);
int llark_gemm16_ln(int dtype, int epilogue, const void* a_hi, const void* a_lo, int lda, const void* wt, int ldw, const float* bias, int m,
                    int n, int kp, float* c, int ldc, const float* resid, int ldr, void* out_hi, void* out_lo, int ldo,
                    const float* ln_stat, const float* ln_vec, float* ln_part, llark_workspace_t ws, llark_stream_t stream);
int llark_ln_stats_finalize(const float* part, int rows, int nparts, int width, float eps, float* stat, llark_stream_t stream);
/* Round 5: the producer role with PREDICTED row statistics.  ln_pred [m][2] = (shift_m, scale_m), scale a power of two: out_hi / out_lo then
 * hold hi / lo of ((c - shift_m) scale_m) ln_vec[n] -- values of order one, so that rows whose level is far from their spread (|mean| >> std)
 * or whose spread is far from one (std ~ 1e-3: the fp16 lo plane would sit in its subnormals; std ~ 1e3: the hi plane would overflow) keep the
 * planes' 22 bits (an fp16 hi/lo pair has them for |x| >= 2^-3 only: see llark_layernorm_split_f16) -- and ln_part the sums of
 * (c - shift_m) and of its square.  llark_ln_stats_finalize_p reduces them to the pair the
 * UNCHANGED consumer role applies, ln_stat = ((mean - shift) scale, rstd / scale), and replaces ln_pred by the prediction for the next
 * LayerNorm of the same rows, (mean, nearest power of two of rstd).  llark_ln_row_pred makes the first prediction of a forward from the rows
 * of x themselves.  ln_pred = NULL: llark_gemm16_ln.  Same call sites (upstream ResAttnBlock ln_0 / ln_1 around the Conv1D products). */
int llark_gemm16_ln_p(int dtype, int epilogue, const void* a_hi, const void* a_lo, int lda, const void* wt, int ldw, const float* bias, int m,
                      int n, int kp, float* c, int ldc, const float* resid, int ldr, void* out_hi, void* out_lo, int ldo,
                      const float* ln_stat, const float* ln_vec, float* ln_part, const float* ln_pred, llark_workspace_t ws, llark_stream_t stream);
int llark_ln_stats_finalize_p(const float* part, int rows, int nparts, int width, float eps, float* stat, float* pred, llark_stream_t stream);
/* The producer role on 128x256 tiles, two workgroups to a CU, weights fragment-major (llark_pack_weight16_frag): one workgroup's epilogue
 * (residual loads, fp32 + plane stores) runs under the other's K loop, which the persistent 256x256 tile (one workgroup per CU) cannot do.
 * For the product with the short K loop -- upstream ResAttnBlock's attention-output Conv1D c_proj, K = n_state = 1200, reached from
 * jukebox/main.py:108 -- where that serial epilogue was 40 % of the launch.  Same arithmetic as llark_gemm16_ln_p's producer role (ln_pred may be
 * NULL); ln_part is [m][ceil(n / 64)][2] (64-column slices: pass nparts = ceil(n / 64) to llark_ln_stats_finalize[_p]).  kp % 64 == 0,
 * kp >= 192, n % 4 == 0; LLARK_ERR_UNSUPPORTED otherwise, before anything is launched. */
int llark_gemm16_lnp_fragw(int dtype, const void* a_hi, const void* a_lo, int lda, const void* wfrag, const float* bias, int m, int n, int kp,
                           float* c, int ldc, const float* resid, int ldr, void* out_hi, void* out_lo, int ldo, const float* ln_vec,
                           float* ln_part, const float* ln_pred, llark_stream_t stream);
int llark_ln_row_pred(const float* x, int ldx, int rows, int width, float eps, float* pred, llark_stream_t stream);
/* "lo8" form of the prior's split GEMM (csrc/gemm256_lo8n.hip; OPT-IN reduced precision, the default is the two-pass fp16
 * form behind llark_gemm16_ws): same call site, upstream Conv1D.forward reached from
 * jukebox/main.py:108 with fp16=False.  The activation is a_hi = fp16(a) plus an E4M3 low plane
 * a_lo8[m][lda8] = fp8(sat((a - a_hi) * 2^sa)) whose 64-element k blocks are stored in MFMA slot order
 * (byte 32*(k/8 % 2) + 8*(k/16 % 4) + k % 8 of the block holds element k); the fp8 weight plane w8 = fp8(wt * 2^sw), same
 * slot order, is packed once by llark_pack_weight_lo8 (choose sw with max|W| * 2^sw <= 448; required).  C = a_hi.W^T + 2^-(sa+sw) a_lo8.W8^T (+ bias):
 * one v_mfma_scale_f32_32x32x64_f8f6f4 replaces the four fp16 MFMAs of the second pass.  Accuracy: the activation
 * carries 15-16 significant bits instead of 22 (measured end to end in tests/test_fulldepth_gpu.py: 36-layer embedding
 * max-abs-err 5.1e-4 against 5.4e-5 for the two-pass form -- above the 1e-4 of BASELINE configs[1], hence opt-in).
 * Operands are addressed with 32-bit byte offsets: m * lda * 2 and m * lda8 must stay below 2^31 (LLARK_ERR_UNSUPPORTED
 * otherwise; split the rows over several calls -- rows are independent).
 * epilogue: LLARK_EPI_F32, LLARK_EPI_RESID, LLARK_EPI_QGELU_SPLIT8 (out_hi fp16 [m][ldo] + out_lo8 [m][ldo8], same format).
 * kp % 64 == 0, kp >= 128; lda8 / ldo8 in bytes, multiples of 64. */
int llark_gemm16_lo8(int epilogue, const void* a_hi, const void* a_lo8, int lda, int lda8, const void* wt, int ldw,
                     const void* w8, int ldw8, const float* bias, int m, int n, int kp, int sa, int sw, float* c, int ldc, const float* resid, int ldr,
                     void* out_hi, void* out_lo8, int ldo, int ldo8, llark_workspace_t ws, llark_stream_t stream);
/* wt fp16 [n][ldw] -> out e4m3 [n][ldo] = fp8(sat(wt * 2^sw)) in MFMA slot order: the w8 operand of llark_gemm16_lo8. */
int llark_pack_weight_lo8(const void* wt, int ldw, int n, int kp, int sw, void* out, int ldo, llark_stream_t stream);
/* Fragment-major weights for the "B-direct" GEMM: wt [n][ldw] (16-bit, K-contiguous, kp % 64 == 0) -> dst of
 * ceil(n/32)*32 * kp elements laid out as 1-KiB chunks [row tile][k16 step][lane 0..63][8 elements] = one MFMA
 * B fragment per chunk (rows >= n are zero).  llark_gemm16_fragw computes the same product as llark_gemm16 but
 * streams these chunks L2 -> VGPR (the weight never goes through LDS); variant: -1 library choice,
 * 0 = 128x256 tiles, 1 = 128x128 tiles (no SwiGLU epilogues).   variant 2 (round 5, csrc/gemm_bda.hip; hi + lo bf16 operands, kp >= 192): the same 128x256 tiles
 * with A staged by LDS-DMA and the A fragments read one sub-step ahead -- results bit-identical to variant 0. */
int llark_pack_weight16_frag(const void* wt, int ldw, int n, int kp, void* dst, llark_stream_t stream);
int llark_gemm16_fragw(int variant, int dtype, int split, int epilogue, const void* a_hi, const void* a_lo, int lda,
                       const void* wfrag, const float* bias, int m, int n, int kp, float* c, int ldc, const float* resid,
                       int ldr, void* out_hi, void* out_lo, int ldo, llark_stream_t stream);
/* 1 when llark_gemm16_fragw_sk's library choice (variant -1, a scratch given) runs the product as whole 128x256 tiles of the per-tile
 * kernel -- no K cut, not the 128x128 tiles: the case in which llark_gemm16_fragw_rope_qkv (always whole 128x256 tiles) is BIT-equal to
 * llark_gemm16_fragw_sk + llark_rope_split_heads.  Shape rule only (no launch); callers ask it instead of restating the rule. */
int llark_gemm16_fragw_whole_tiles(int split, int epilogue, int m, int n, int kp);
/* The Llama q|k|v product of a PREFILL with RoPE, the head split, the K-cache append and the transposed V-cache append in its
 * epilogue: one launch instead of llark_gemm16_fragw (fp32 qkv) + llark_rope_split_heads (m2t/models/llamav2.py:224-234 -> HF
 * LlamaAttention q_proj / k_proj / v_proj, apply_rotary_pos_emb, cache update).  bf16 only; head_dim 128, nh even, s >= 32.
 * a_hi / a_lo [batch * s][lda]: RMSNorm output planes (a_lo NULL = plain bf16 mode: the three *_lo outputs must be NULL too).
 * wfrag: llark_pack_weight16_frag of the [3 * nh * 128][kp] q|k|v weight with the q and k rows of every head reordered to
 * [0..31 | 64..95 | 32..63 | 96..127] (v rows natural), so that a rotation pair (d, d + 64) shares a lane and register.
 * Outputs as llark_rope_split_heads writes them; bit-equal to the two-launch path wherever that runs whole 128x256 tiles. */
int llark_gemm16_fragw_rope_qkv(const void* a_hi, const void* a_lo, int lda, const void* wfrag, int kp, int batch, int s, int nh, int hd,
                                int pos0, const float* cos_t, const float* sin_t, int max_pos, void* q, void* k_cache, void* vt_cache,
                                void* q_lo, void* k_cache_lo, void* vt_cache_lo, int smax, llark_stream_t stream);
/* llark_gemm16_fragw with the K range of a tile cut over several workgroups, for products whose tile count is not a whole
 * number of rounds of the resident workgroups (Llama prefill at M = 2968: 384 / 1152 / 2064 tiles of 128x256 against 512
 * resident workgroups; one clip, M = 371: 48 .. 258 tiles -- m2t/models/llamav2.py:224-234 -> the q/k/v, o, gate/up, down
 * projections of HF LlamaDecoderLayer).  variant -1: where the measured rule says it pays (gemm.hip, gemm16_fragw_impl), the
 * library's choice cuts EVERY tile into the same 2 or 4 K ranges (one workgroup each; the last range finishes the tile and
 * adds the others' fp32 partial tiles from `scratch` in order: deterministic, no atomics on data, no assumption about how
 * many workgroups are resident); variant 0 instead cuts the ragged remainder of the tile order into equal runs over exactly
 * the resident workgroups (stream-K; needs an otherwise idle device).  Same product and epilogues as llark_gemm16_fragw (QGELU_SPLIT
 * excepted, which runs the per-tile kernel), equal up to the fp32 summation order over K.
 * scratch: caller-owned device memory, >= llark_gemm16_sk_scratch_bytes() bytes (the function returns that size for the
 * CURRENT device, -1 on error), 16-byte aligned, ZEROED once after allocation; launches sharing it must be ordered on one
 * stream.  The hand-off flags occupy the LAST 64 KiB of [scratch, scratch + scratch_bytes) whatever the shape of a launch (the
 * fp32 partial tiles grow from the front and are checked never to reach them), so pass the same (scratch, scratch_bytes)
 * pair on every call that shares a scratch.  scratch == NULL, or a problem too small to cut -> exactly llark_gemm16_fragw. */
long long llark_gemm16_sk_scratch_bytes(void);
int llark_gemm16_fragw_sk(int variant, int dtype, int split, int epilogue, const void* a_hi, const void* a_lo, int lda,
                          const void* wfrag, const float* bias, int m, int n, int kp, float* c, int ldc, const float* resid,
                          int ldr, void* out_hi, void* out_lo, int ldo, void* scratch, long long scratch_bytes,
                          llark_stream_t stream);
/* Decode step (m <= 16 rows, bf16): h[m][n] += a . wt^T and then RMSNorm(h; norm_w, eps) -> bf16 planes x_hi (/x_lo),
 * in one launch (the last workgroup to finish normalises the complete rows; bit-identical to llark_gemm16 +
 * llark_rmsnorm_bf16).  Replaces o_proj / down_proj + the next LlamaRMSNorm of the cached decode path
 * (m2t/models/llamav2.py:224-234 -> HF LlamaDecoderLayer). */
int llark_gemm16_resid_rmsnorm(int dtype, int split, const void* a_hi, const void* a_lo, int lda, const void* wt, int ldw,
                               int m, int n, int kp, float* h, int ldh, const float* norm_w, float eps, void* x_hi,
                               void* x_lo, int ldx, llark_stream_t stream);
/* Decode step (m <= 16 rows, bf16): RMSNorm(x; norm_w, eps) . wt^T with the norm fused INTO the consuming weight-streaming
 * GEMM (every workgroup re-derives the row scales; bit-identical to llark_rmsnorm_bf16 + llark_gemm16).  epilogue: F32 or
 * SwiGLU(16/split).  Replaces LlamaRMSNorm + q/k/v, gate/up and lm_head projections of the cached decode path. */
int llark_gemm16_rmsnorm_a(int dtype, int split, int epilogue, const float* x, int ldx, const float* norm_w, float eps,
                           const void* wt, int ldw, const float* bias, int m, int n, int kp, float* c, int ldc, void* out_hi,
                           void* out_lo, int ldo, llark_stream_t stream);
/* Batched form (grid.y = batch): per-batch element strides for A, wt, c and the 16-bit outputs (no bias / residual).
 * Used by the attention backward of the training step (one product per (sequence, head)). */
int llark_gemm16_batched(int dtype, int split, int epilogue, const void* a_hi, const void* a_lo, int lda, long long stride_a,
                         const void* wt, int ldw, long long stride_w, int m, int n, int kp, float* c, int ldc,
                         long long stride_c, void* out_hi, void* out_lo, int ldo, long long stride_o, int batch,
                         llark_stream_t stream);
/* The same with a bias [n] shared by every batch element and a per-element residual (epilogue F32: c = A . wt^T + bias; RESID: + resid).
 * Every element is bit-equal to its own llark_gemm16_ws call with the same m: elements of m <= 16 rows are launched one by one on the
 * weight-streaming kernel, larger ones share one launch of the tile kernel; shapes of the persistent tiles are refused. */
int llark_gemm16_batched_bias(int dtype, int split, int epilogue, const void* a_hi, const void* a_lo, int lda, long long stride_a,
                              const void* wt, int ldw, long long stride_w, const float* bias, int m, int n, int kp, float* c, int ldc,
                              long long stride_c, const float* resid, int ldr, long long stride_r, void* out_hi, void* out_lo, int ldo,
                              long long stride_o, int batch, llark_stream_t stream);
/* w[k][n] (upstream Conv1D.w, 16-bit) -> wt[n][ldw] with zero K padding; also serves row-major copies
 * (transpose=0: w is already [n][k], e.g. nn.Linear.weight). src_dtype/dst_dtype: LLARK_F16/BF16 or
 * 2 for fp32 source. */
int llark_pack_weight16(const void* w, int src_dtype, int transpose, int k, int n, void* wt, int dst_dtype, int ldw,
                        llark_stream_t stream);
/* fp32 [rows][ld_in] -> 16-bit hi/lo planes [rows][ldo] (lo may be NULL); pads [width, ldo) with zeros. */
int llark_split16(int dtype, const float* x, int ldx, int rows, int width, void* out_hi, void* out_lo, int ldo,
                  llark_stream_t stream);


/* ---------------------------------------------------------------------------------------------
 * Llama-2 decoder: what WrappedLlamav2Model.forward delegates to HF LlamaModel.forward
 * (m2t/models/llamav2.py:224-234) plus the embed_tokens gather (m2t/models/llamav2.py:124).
 * Residual stream fp32 [rows][hidden]; Linear inputs / q / k / v / probabilities bf16.
 * ------------------------------------------------------------------------------------------- */
/* nn.Embedding gather: out[row] = table[ids[row]] (table_dtype LLARK_F16 / LLARK_BF16 / 2 = fp32).  llark_embed_gather clamps ids
 * to [0, vocab): a negative id reads row 0, an id >= vocab reads row vocab - 1 (torch raises there). */
int llark_embed_gather(const int64_t* ids, int rows, const void* table, int table_dtype, int vocab, int width,
                       float* out, int ldo, llark_stream_t stream);
/* LlamaRMSNorm -> bf16 (out_lo optional second plane with the rounding residual). */
int llark_rmsnorm_bf16(const float* x, int ldx, int rows, int width, const float* w, float eps, void* out_hi,
                       void* out_lo, int ldo, llark_stream_t stream);
/* apply_rotary_pos_emb (half-split) + split heads + KV-cache write.  qkv fp32 [batch*s][3*nh*hd];
 * q bf16 [batch][nh][s][hd]; k_cache bf16 [batch][nh][smax][hd]; vt_cache bf16 [batch][nh][hd][smax]
 * (V transposed); rows/columns pos0..pos0+s-1 are written; cos/sin fp32 [max_pos][hd/2]. */
/* q_lo / k_cache_lo / vt_cache_lo: optional second planes holding the bf16 rounding residual (all three or
 * none): the "fp32-class" mode in which q, k, v keep 16 significant bits. */
int llark_rope_split_heads(const float* qkv, int batch, int s, int nh, int hd, int pos0, const float* cos_t,
                           const float* sin_t, int max_pos, void* q, void* k_cache, void* vt_cache, void* q_lo,
                           void* k_cache_lo, void* vt_cache_lo, int smax, llark_stream_t stream);
/* smax % 8 == 0 for every attention entry point, prefill and decode, fused or not (LLARK_ERR_INVALID otherwise, before any launch):
 * the kernels read V^T rows in 16-byte chunks of 8 keys.  Cache positions [total, round_up(total, 8)) are read by the decode forms
 * and must hold finite values in every plane (stale rows of an earlier sequence are fine, NaN / Inf are not): they are multiplied by
 * a zero probability (bf16 planes) or left out of the sum (hi + lo planes).  Positions >= round_up(total, 8) are never read. */
/* causal attention over the cache: query i sees keys j <= past + i. out bf16 [batch*s][nh*hd]. */
int llark_attn_prefill_bf16(const void* q, const void* k_cache, const void* vt_cache, const void* q_lo,
                            const void* k_cache_lo, const void* vt_cache_lo, int batch, int s, int nh, int hd, int past,
                            int smax, void* out, void* out_lo, llark_stream_t stream);
/* single-token attention over `total` cached keys. q bf16 [batch][nh][hd]; out bf16 [batch][nh*hd]. */
int llark_attn_decode_bf16(const void* q, const void* k_cache, const void* vt_cache, const void* q_lo,
                           const void* k_cache_lo, const void* vt_cache_lo, int batch, int nh, int hd, int total, int smax,
                           void* out, void* out_lo, llark_stream_t stream);
/* Same two kernels with ALiBi (MPT, m2t/llava/model/mpt/attention.py:build_alibi_bias + :58): alibi_slopes fp32 [nh]
 * (nullptr = none); slope_h * (key - (keys_visible - 1)) is added to the scaled scores before the softmax. */
int llark_attn_prefill_bf16_alibi(const void* q, const void* k_cache, const void* vt_cache, const void* q_lo,
                                  const void* k_cache_lo, const void* vt_cache_lo, int batch, int s, int nh, int hd, int past,
                                  int smax, void* out, void* out_lo, const float* alibi_slopes, llark_stream_t stream);
int llark_attn_decode_bf16_alibi(const void* q, const void* k_cache, const void* vt_cache, const void* q_lo,
                                 const void* k_cache_lo, const void* vt_cache_lo, int batch, int nh, int hd, int total, int smax,
                                 void* out, void* out_lo, const float* alibi_slopes, llark_stream_t stream);

/* Decode-step Linear: c[m][n] = sum_k a[m][k] wt[n][k] (+ bias[n]) for m <= 4 activation rows, bf16 operands (a = hi plane + optional
 * lo plane for the fp32-class mode), fp32 accumulate -- the weight-streaming form of llark_gemm16 (csrc/gemv_dma.hip: weights global ->
 * LDS by LDS-DMA, 96 KiB in flight per CU, no barrier in the K loop).  Replaces nn.Linear under LlamaModel.forward with one new token
 * (m2t/infer.py:146 -> model.generate; transformers==4.29.2 modeling_llama.py).  epilogue: LLARK_EPI_F32, LLARK_EPI_RESID (resid may
 * alias c), LLARK_EPI_SWIGLU16 / LLARK_EPI_SWIGLU_SPLIT (wt rows interleaved [gate 32 | up 32], out [m][n / 2]).  kp % 8 == 0,
 * kp <= 12288, lda / ldw % 8 == 0; other shapes return LLARK_ERR_UNSUPPORTED (use llark_gemm16). */
int llark_gemv16_dma(int split, int epilogue, const void* a_hi, const void* a_lo, int lda, const void* wt, int ldw, const float* bias,
                     int m, int n, int kp, float* c, int ldc, const float* resid, int ldr, void* out_hi, void* out_lo, int ldo,
                     llark_stream_t stream);
/* ... with LlamaRMSNorm fused in front (decode: input_layernorm -> q/k/v_proj, post_attention_layernorm -> gate/up_proj, norm ->
 * lm_head; modeling_llama.py LlamaRMSNorm): a = bf16 hi (+ lo when split) of norm_w * (x * rstd), x fp32 [m][ldx].  Bit-identical to
 * llark_rmsnorm_bf16 followed by llark_gemv16_dma.  m == 1, kp <= 4096; epilogue LLARK_EPI_F32 or SwiGLU. */
int llark_gemv16_dma_rmsnorm(int split, int epilogue, const float* x, int ldx, const float* norm_w, float eps, const void* wt, int ldw,
                             const float* bias, int m, int n, int kp, float* c, int ldc, void* out_hi, void* out_lo, int ldo,
                             llark_stream_t stream);

/* Decode-step Linear for 17 <= m <= 64 activation rows (the ragged decode step with more than 16 slots; csrc/gemm_mid.hip):
 * c[m][n] = sum_k (a_hi [+ a_lo])[m][k] wt[n][k] (+ bias[n]), bf16 operands, fp32 accumulate; wt is the row-major [n][ldw] tensor
 * llark_gemm16 reads.  Every weight byte is read from HBM once per launch; a workgroup owns 128 (bf16 flow) or 256 (split flow) output
 * columns and shares its activation chunk through LDS; K is cut over workgroups so that a 256-CU chip is filled, fp32 partial sums
 * meet in `scratch` and a second launch adds them in a fixed order -- no atomics, nothing waits.  Output row r is bit-identical
 * whatever m is, whatever the other rows hold and from launch to launch.
 * epilogue: LLARK_EPI_F32, LLARK_EPI_RESID (resid may alias c), LLARK_EPI_SWIGLU16 / LLARK_EPI_SWIGLU_SPLIT (wt rows interleaved
 * [gate 32 | up 32], n % 64 == 0, out [m][n / 2]).  kp % 32 == 0; lda, ldw >= kp and % 8 == 0; a_hi / a_lo / wt / scratch 16-byte
 * aligned; ldc, ldr, ldo free.  Rows >= m and columns >= n are never stored.  dtype: LLARK_BF16 (LLARK_F16 and m outside 17 .. 64
 * return LLARK_ERR_UNSUPPORTED); every rule is checked before any launch and llark_last_error names the argument.
 * scratch: caller-owned, at least llark_gemm16_mid_scratch_bytes(...) bytes = splits x m x (n rounded up to the column tile) x 4, where
 * splits (1 .. 8) depends on n, kp and split only; 0 = the shape or epilogue is refused. */
long long llark_gemm16_mid_scratch_bytes(int m, int n, int kp, int split, int epilogue);
int llark_gemm16_mid(int dtype, int split, int epilogue, const void* a_hi, const void* a_lo, int lda, const void* wt, int ldw,
                     const float* bias, int m, int n, int kp, float* c, int ldc, const float* resid, int ldr, void* out_hi, void* out_lo,
                     int ldo, void* scratch, long long scratch_bytes, llark_stream_t stream);

/* Backward products of nn.Linear without transposed copies of their operands (csrc/gemm_tn.hip; torch autograd of the Linear
 * layers under WrappedLlamav2ForCausalLM.forward + loss.backward(), m2t/models/llamav2.py:259-337, m2t/train.py:53-277):
 *   c[m][n] (= | +=) sum_k A(m, k) W(n, k), 16-bit operands, fp32 accumulate / output.
 * trans_a == 0: a is [m][lda], k contiguous; trans_a != 0: a is [kp][lda], row = k and column = m (e.g. dY for dW = dY^T X).
 * trans_b == 0: wt is [n][ldw], k contiguous; trans_b != 0: wt is [kp][ldw], row = k and column = n (e.g. W itself for dX = dY W).
 * kp % 64 == 0 and every one of the kp contraction rows / columns is read (pad with zeros); lda, ldw % 8 == 0; a transposed
 * operand's free size % 8 == 0.  epilogue: LLARK_EPI_F32 or LLARK_EPI_RESID (resid may alias c). */
int llark_gemm16_t(int dtype, int epilogue, int trans_a, int trans_b, const void* a, int lda, const void* wt, int ldw, int m, int n,
                   int kp, float* c, int ldc, const float* resid, int ldr, llark_stream_t stream);
/* ... and *sumsq (a double in device memory) += the sum of squares of every value written to c: the dW product of the last
 * micro-batch leaves its share of the squared gradient norm behind (HF Trainer's clip_grad_norm_; llark_adamw_clip consumes it). */
int llark_gemm16_t_sumsq(int dtype, int epilogue, int trans_a, int trans_b, const void* a, int lda, const void* wt, int ldw, int m, int n,
                         int kp, float* c, int ldc, const float* resid, int ldr, double* sumsq, llark_stream_t stream);

/* llark_gemm16_t / llark_gemm16_t_sumsq (sumsq nullable) with an explicit tile / pipeline variant, for benchmarks and A/B tests:
 * -1 = library choice, 0 = one LDS stage per workgroup, 1 = 128x256x32 tiles with two stages, 2 = 128x256x64 two stages, 3 = 256x256x64
 * two stages (8 waves).  Results are bit-identical across variants. */
int llark_gemm16_t_ex(int variant, int dtype, int epilogue, int trans_a, int trans_b, const void* a, int lda, const void* wt, int ldw, int m,
                      int n, int kp, float* c, int ldc, const float* resid, int ldr, double* sumsq, llark_stream_t stream);

/* Training pair (csrc/llama.hip, csrc/attn_bwd.hip): what torch autograd does for LlamaAttention's eager path
 * (transformers==4.29.2 modeling_llama.py) under WrappedLlamav2ForCausalLM.forward + loss.backward()
 * (m2t/models/llamav2.py:259-337, m2t/train.py:53-277), without ever writing an S x S matrix.
 * Forward: bf16 operands, no past keys; also writes lse fp32 [batch*nh][s], the log-sum-exp of each query's scaled masked scores. */
int llark_attn_prefill_bf16_lse(const void* q, const void* k_cache, const void* vt_cache, int batch, int s, int nh, int hd,
                                int smax, void* out, float* lse, const float* alibi_slopes, llark_stream_t stream);
/* Backward: q, dO, v_rm bf16 [batch*nh][s][128] (row-major); k_cache bf16 [batch*nh][smax][128]; o bf16 [batch*s][nh*128] = the
 * forward's out; lse from the forward; dsum fp32 [batch*nh][s] scratch.  Outputs dq, dk, dv fp32 [batch*nh][s][128] (before the RoPE
 * backward / head merge).  No transposed copies of any operand are needed (transposing LDS reads inside).
 * alibi_slopes (both calls): nullptr (Llama) or fp32 [nh] (MPT-1B trainer), the bias of llark_attn_prefill_bf16_alibi.
 * The contract (tests/test_attn_bwd_kernels_gpu.py holds every output element to it): o and lse are used AS GIVEN, nothing of the
 * forward is recomputed -- P_ij = exp(q_i.k_j / sqrt(hd) + slope_h (j - (s - 1)) - lse_i) for j <= i, else 0; D_i = sum_d dO_id o_id;
 * dS = P (dO V^T - D); dv = P^T dO, dq = dS K / sqrt(hd), dk = dS^T Q / sqrt(hd), with P and dS each rounded to bf16 once.  dsum is an
 * OUTPUT: it holds D = rowsum(dO * o) afterwards.  K-cache rows >= s are never read (nor any row >= s of q, v_rm, dO, lse).  dq, dk and
 * dv must be 16-byte aligned (they are written as 4 floats per store).  No input is written; no atomics: launches are bit-reproducible. */
int llark_attn_backward_bf16(const void* q, const void* k_cache, const void* v_rm, const void* dO, const void* o, const float* lse,
                             float* dsum, int batch, int s, int nh, int hd, int smax, float* dq, float* dk, float* dv,
                             const float* alibi_slopes, llark_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * MPT backbone (m2t/models/mpt.py over m2t/llava/model/mpt/{blocks,attention,norm}.py): the row-wise / element-wise
 * pieces that differ from Llama.  LayerNorm (norm.py; beta may be NULL for no_bias models) to bf16 hi (+ lo) planes
 * for the next GEMM, or fp32 -> fp32 (qk_ln over the q / k column blocks of the fused qkv, attention.py:330-333);
 * clip_qkv (attention.py:325-326); exact erf GELU between up_proj and down_proj (blocks.py:15,19) to bf16 planes.
 * ------------------------------------------------------------------------------------------- */
int llark_layernorm_bf16(const float* x, int ldx, int rows, int width, const float* gamma, const float* beta, float eps,
                         void* out_hi, void* out_lo, int ldo, llark_stream_t stream);
int llark_layernorm_f32(const float* x, int ldx, int rows, int width, const float* gamma, const float* beta, float eps,
                        float* y, int ldy, llark_stream_t stream);
int llark_clamp_f32(float* x, long long n, float limit, llark_stream_t stream);
/* backward of that clamp in the MPT training step: dy (bf16 [n], in place) keeps its value where |x| <= limit (x = the qkv
 * BEFORE the clamp) and becomes 0 elsewhere -- torch.clamp's gradient under loss.backward() (m2t/train.py:53-277). */
int llark_clamp_bwd_bf16(const float* x, long long n, float limit, void* dy, llark_stream_t stream);
int llark_scale_f32(float* x, long long n, float a, llark_stream_t stream);   /* logits *= logit_scale */
int llark_gelu_split_bf16(const float* x, int ldx, int rows, int width, void* out_hi, void* out_lo, int ldo,
                          llark_stream_t stream);
/* Backward pieces of the MPT training step: LayerNorm (dx [+= if accumulate], dgamma / dbeta accumulated with atomics),
 * exact GELU (fp32 copy optional, bf16 copy for the GEMMs), causal softmax rows with the ALiBi bias (probabilities of the
 * materialised attention backward; slopes fp32 [nh], row b of the batch belongs to head b % nh). */
int llark_layernorm_bwd(const float* x, int ldx, const float* gamma, const float* dy, int ldy, int rows, int width, float eps,
                        float* dx, int lddx, float* dgamma, float* dbeta, int accumulate, llark_stream_t stream);
int llark_gelu_bwd(const float* up, const float* dact, long long n, float* dup32, void* dup16, llark_stream_t stream);
int llark_causal_softmax_rows_alibi(const float* scores, int batch, int s, float scale, const float* slopes, int nh, void* p_out,
                                    int ldp, llark_stream_t stream);
/* ---------------------------------------------------------------------------------------------
 * CLAP HTSAT-base audio encoder (scripts/clap/clap_embeddings.py:63-107 -> laion_clap
 * CLAP_Module(enable_fusion=False, amodel="HTSAT-base").model.get_audio_embedding): the pieces that are not GEMM /
 * LayerNorm / GELU.  patchify: log-mel x [batch][frames][mel] -> BatchNorm over mel bins ((x - mean) * scale + bias),
 * 4-tap bicubic stretch of the time axis (tap_idx / tap_w [spec * spec / mel][4], host built), time-chunk fold to a
 * spec x spec image, patch x patch im2col -> bf16 planes [batch * (spec/patch)^2][ldo] (k = kh * patch + kw).
 * window_attn: Swin attention over 8x8 windows of a [batch][H][W] token map, qkv fp32 rows [q | k | v] of 3C in token
 * order; cyclic shift, relative-position bias (table [(2*8-1)^2][heads]) and the shifted-window mask (-100) are applied
 * in-kernel; context written to bf16 planes at the same token rows.  patch_merge: 2x2 neighbourhood gather to 4C-wide
 * rows (quadrant order (0,0),(1,0),(0,1),(1,1)).  mean_rows: per-clip mean over L token rows.  l2_normalize_rows in place
 * (x / max(||x||, eps)).
 * ------------------------------------------------------------------------------------------- */
/* waveform [batch][n] (48 kHz) -> log-mel dB [batch][n/480 + 1][64]: STFT n_fft 1024 / hop 480 / center-reflect with `window`
 * [1024], radix-2 FFT with `twiddle` [512] (cos, -sin) pairs of exp(-2 pi i k / 1024), power, mel filters melw [64][513]
 * (non-zero over bins [mel_lo, mel_hi)), 10 log10(max(x, 1e-10)).  quantize_int16 != 0 applies laion_clap's
 * int16_to_float32(float32_to_int16(x)) round trip (clap_embeddings.py:139) to each sample as it is read. */
int llark_clap_logmel(const float* wav, int batch, int n, int quantize_int16, const float* window, const float* twiddle,
                      const float* melw, const int* mel_lo, const int* mel_hi, float* out, llark_stream_t stream);
int llark_clap_patchify(const float* x, int batch, int frames, int mel, const float* bn_mean, const float* bn_scale,
                        const float* bn_bias, const int* tap_idx, const float* tap_w, int spec, int patch, void* out_hi,
                        void* out_lo, int ldo, llark_stream_t stream);
int llark_clap_window_attn(const float* qkv, int ldq, int batch, int H, int W, int C, int heads, int window, int shift,
                           const float* bias_table, void* out_hi, void* out_lo, void* out_hi_dup, int ldo, llark_stream_t stream);
/* fp32-class linears over fp32 checkpoint weights W = W_hi + W_lo as ONE launch: the producer writes the activation as a
 * K-concatenated [hi | lo | hi] operand (out_hi_dup = second copy of the hi plane, same row stride) and the product runs
 * non-split against [W_hi | W_hi | W_lo].  layernorm_bf16_dup / window_attn (above) / gemm16_act are the producers;
 * gemm16_act is a GEMM whose epilogue is acc + bias -> optional exact (erf) GELU (act = 2) -> 16-bit planes
 * (epilogue LLARK_EPI_SPLIT16 or LLARK_EPI_OUT16), i.e. fc1 + GELU of a transformer MLP without the fp32 round trip. */
int llark_layernorm_bf16_dup(const float* x, int ldx, int rows, int width, const float* gamma, const float* beta, float eps,
                             void* out_hi, void* out_lo, void* out_hi_dup, int ldo, llark_stream_t stream);
int llark_gemm16_act(int variant, int dtype, int split, int epilogue, const void* a_hi, const void* a_lo, int lda, const void* wt,
                     int ldw, const float* bias, int m, int n, int kp, void* out_hi, void* out_lo, void* out_hi_dup, int ldo,
                     int act, llark_stream_t stream);
int llark_clap_patch_merge(const float* x, int ldx, int batch, int H, int W, int C, float* out, int ldo, llark_stream_t stream);
int llark_mean_rows_f32(const float* x, int ldx, int batch, int L, int C, float* out, int ldo, llark_stream_t stream);
int llark_relu_split_bf16(const float* x, int ldx, int rows, int width, void* out_hi, void* out_lo, int ldo, llark_stream_t stream);
int llark_l2_normalize_rows(float* x, int ldx, int rows, int width, float eps, llark_stream_t stream);

/* Decode step, fused: RoPE of the new token (qkv fp32 [batch][3 * nh * 128]) + append to the KV caches + attention over the
 * cache, one launch (m2t/models/llamav2.py:339-365 decode loop; replaces rope_split_heads + attn_decode).  Position = pos,
 * or *pos_dev when pos_dev != NULL.  lo planes: all or none.  alibi_slopes may be NULL. */
int llark_attn_decode_rope_bf16(const float* qkv, int batch, int nh, int hd, int pos, const int* pos_dev, const float* cos_t,
                                const float* sin_t, int max_pos, void* k_cache, void* vt_cache, void* k_cache_lo, void* vt_cache_lo,
                                int smax, void* out, void* out_lo, const float* alibi_slopes, llark_stream_t stream);
/* Ragged decode over batch slots (every sequence its own cache length; in-flight slot refill):
 *   llark_attn_decode_rope_bf16_rows: llark_attn_decode_rope_bf16 with the position of sequence b read from pos_rows[b]
 *     (int32 [batch], device): block (h, b) rotates q / k with cos / sin[pos_rows[b]], appends k and v at row pos_rows[b] of slot
 *     b and walks keys 0 .. pos_rows[b].  pos_rows[b] < 0 marks an idle slot: nothing is written to its caches, its output head
 *     is zero (a position >= smax is treated the same way).  Caches k [batch][nh][smax][128], v^T [batch][nh][128][smax];
 *     out bf16 [batch][nh * 128]; dynamic LDS holds smax scores; smax <= max_pos (rows of cos_t / sin_t [max_pos][64]).
 *   llark_decode_advance_rows: the bookkeeping after the logits of such a step, one launch.  logits fp32 [batch][ldl];
 *     state int32 [batch] of LLARK_ROW_*; for every ACTIVE row: token = choice[b] when choice != NULL, else the first maximal
 *     index of logits[b][0 .. vocab) (torch.argmax); next_ids[b] = token (int64), out_col[b * ld_out] = token (out_col may be
 *     NULL); state[b] = LLARK_ROW_FINISHED when token == eos (eos >= 0); pos_rows[b] += 1 (pos_rows may be NULL: no advance).
 *     IDLE and FINISHED rows get `pad` in next_ids / out_col and keep their position. */
#define LLARK_ROW_IDLE 0
#define LLARK_ROW_ACTIVE 1
#define LLARK_ROW_FINISHED 2
int llark_attn_decode_rope_bf16_rows(const float* qkv, int batch, int nh, int hd, const int* pos_rows, const float* cos_t,
                                     const float* sin_t, int max_pos, void* k_cache, void* vt_cache, void* k_cache_lo, void* vt_cache_lo,
                                     int smax, void* out, void* out_lo, const float* alibi_slopes, llark_stream_t stream);
int llark_decode_advance_rows(const float* logits, int ldl, int vocab, int batch, const int64_t* choice, int* pos_rows, int* state,
                              int64_t* next_ids, int64_t* out_col, int ld_out, int64_t eos, int64_t pad, llark_stream_t stream);
/* Speculative greedy decoding: a decode step that verifies a block of drafted tokens per slot (csrc/attn_block.hip, csrc/speculate.hip).
 *   llark_attn_decode_rope_bf16_block: llark_attn_decode_rope_bf16_rows for rows that belong to the SAME slot at consecutive positions.
 *     qkv fp32 [n_slots * stride][3 * nh * 128], stride 1 .. 8 rows per slot; blk int32 [n_slots] (0 .. stride; larger counts as stride)
 *     and pos_rows int32 [n_slots] on the device.  Slot b owns rows b*stride .. b*stride + blk[b] - 1; row i is the token at position
 *     pos_rows[b] + i.  Workgroup (head, slot) rotates and appends the K / V of all its rows first (rope_split's arithmetic and rounding),
 *     then walks the cache once; query i sees keys 0 .. pos_rows[b] + i.  out (+ out_lo) bf16 [n_slots * stride][nh * 128].
 *     A slot with blk == 0 or pos < 0 writes nothing to the caches; a row at a position >= smax writes nothing; the output heads of such
 *     rows and of rows >= blk[b] are zero.  No ALiBi.  Contract: the out planes of row i and the cache rows written are BIT-equal to
 *     what blk[b] successive llark_attn_decode_rope_bf16_rows launches with batch = n_slots produce (row i in launch i, slots whose
 *     block is shorter idle).  16 waves per workgroup while nh * n_slots < 256, 4 otherwise, as llark_attn_decode_rope_bf16_rows.
 *     Dynamic LDS holds stride * smax scores: above 128 KiB LLARK_ERR_UNSUPPORTED, before any launch.  LLARK_ERR_INVALID before any
 *     launch: a null pointer, one lo plane only, hd != 128, stride outside 1 .. 8, smax % 8 != 0, smax > max_pos.
 *   llark_spec_verify_rows: the bookkeeping after the logits of a block step, one launch, one workgroup per slot.  logits fp32
 *     [n_slots * stride][ldl], ids int64 [n_slots * stride] (the block's input tokens), blk / state / pos_rows / budget int32 [n_slots]
 *     (budget: tokens the slot may still emit).  For a slot that is LLARK_ROW_ACTIVE with blk > 0 and budget > 0:
 *       g_i = first maximal index of logits row i over [0, vocab), a NaN counting as the maximum (llark_decode_advance_rows' rules);
 *       a = number of leading i in 0 .. blk-2 with ids[i + 1] == g_i; the emitted tokens are g_0 .. g_a, cut at `budget` and after the
 *       first eos (eos >= 0); n = their count (>= 1).
 *     It writes out_tokens[b][0 .. 8) (int64, the emitted tokens, then pad), n_out[b] = n (int64, so that out_tokens and n_out can be
 *     two views of one buffer and leave in one transfer), next_ids[b] = the last emitted token, pos_rows[b] += n, budget[b] -= n,
 *     state[b] = LLARK_ROW_FINISHED when the run ended on eos, and appends the emitted tokens to hist[b][hist_len[b] ..] (int64
 *     [n_slots][ld_hist], hist_len int32 [n_slots]; tokens beyond ld_hist are dropped; hist and hist_len may both be NULL).
 *     Every other slot: out_tokens[b] = pad, n_out[b] = 0, nothing else is touched.
 *   llark_spec_draft_rows: fills the next block, one launch.  A slot that is not ACTIVE, has pos_rows < 0, budget <= 0 or pos_rows >=
 *     smax gets blk = 0 and pad ids.  Otherwise ids[b*stride] = next_ids[b], followed by n_draft drafted tokens and pad, and blk[b] =
 *     1 + n_draft with n_draft <= k_max, blk <= stride, blk <= budget and pos_rows + blk <= smax.  The drafts are
 *       drafts != NULL: drafts[b][0 .. n_drafts[b]) of the caller's int64 [n_slots][ld_drafts];
 *       drafts == NULL (prompt lookup): for g = g_max down to 1, the first g for which the last g tokens of the slot's history occur
 *       at an earlier start s <= hist_len - g - 1; of these the largest s; the tokens hist[s + g .. hist_len) that follow it (the
 *       continuation may run into the suffix itself).  No match, or a history shorter than g + 1 for every g: n_draft = 0, a plain step.
 *     LLARK_ERR_INVALID before any launch: a null pointer, neither drafts nor hist, stride outside 1 .. 8, k_max outside 0 .. 7, g_max
 *     outside 1 .. 64. */
int llark_attn_decode_rope_bf16_block(const float* qkv, int n_slots, int stride, int nh, int hd, const int* blk, const int* pos_rows,
                                      const float* cos_t, const float* sin_t, int max_pos, void* k_cache, void* vt_cache, void* k_cache_lo,
                                      void* vt_cache_lo, int smax, void* out, void* out_lo, llark_stream_t stream);
int llark_spec_verify_rows(const float* logits, int ldl, int vocab, int n_slots, int stride, const int64_t* ids, const int* blk, int* state,
                           int* pos_rows, int* budget, int64_t eos, int64_t pad, int64_t* out_tokens, int64_t* n_out, int64_t* next_ids,
                           int64_t* hist, int* hist_len, int ld_hist, llark_stream_t stream);
int llark_spec_draft_rows(const int64_t* next_ids, const int* state, const int* pos_rows, const int* budget, const int64_t* hist,
                          const int* hist_len, int ld_hist, int n_slots, int stride, int k_max, int g_max, int smax, const int64_t* drafts,
                          const int* n_drafts, int ld_drafts, int64_t* ids, int* blk, int64_t pad, llark_stream_t stream);
/* Token sampling on the device (csrc/sample.hip): the producer of llark_decode_advance_rows' `choice`.
 *   llark_sample_rows: one workgroup per row r of logits fp32 [rows][ldl] (columns >= vocab are never read).  slot = slot_of_row[r]
 *     (int32 [rows], NULL: slot = r; rows map to DISTINCT slots); a row whose slot is outside [0, slots) or, when state != NULL (int32
 *     [slots] of LLARK_ROW_*), not LLARK_ROW_ACTIVE is skipped: nothing of it is read or written.  Otherwise, in fp32 and in the
 *     processor order of HF 4.29.2:
 *       1. repetition penalty (1 = off): a token t whose bit (t & 31) of word seen[slot][t >> 5] is set: l < 0 ? l * penalty : l / penalty
 *          (seen uint32 [slots][ld_seen], ld_seen >= ceil(vocab / 32));
 *       do_sample == 0: choice[r] = first maximal index of the penalised row (a NaN counts as the maximum), its seen bit is set (seen
 *          != NULL), nothing else is written;
 *       2. l / temperature;  3. top_k (0 = off, else clamped to 1 .. vocab): keep l >= the k-th largest value, ties at the threshold
 *          all kept;  4. top_p (1 = off): with e_i = exp(l_i - max) over the kept set and Z their sum, keep token i iff the sum of
 *          the e_j with l_j > l_i is < top_p * Z -- tokens with equal logits stay or go together, so tokens exactly tied at the
 *          boundary are all kept;  5. the token is the smallest index whose inclusive cumulative kept mass, in token order, exceeds
 *          x * Z_kept.  x = u[r] (u fp32 [rows] in [0, 1)) when u != NULL, else (w >> 8) * 2^-24 with w the first word of
 *          Philox4x32-10 under key (seed lo32, seed hi32) and counter (draws[slot], 0, stream_id[slot] lo32, hi32); stream_id int64
 *          [slots], NULL: the slot index.
 *       Then choice[r] = token (always in [0, vocab)), its seen bit is set (seen != NULL), draws[slot] += 1 (draws != NULL), kept[r] =
 *       size of the final kept set and thresh[r] = its smallest post-temperature logit (both nullable).  A row that holds a NaN, whose
 *       maximum is +-inf or whose kept mass is not a positive finite number takes the greedy token of the penalised row instead, gets
 *       kept[r] = 0, and adds 1 to *fallbacks (nullable).  Sums have a fixed order: results are bit-reproducible.
 *     LLARK_ERR_INVALID before any launch: a null logits / choice, rows, slots or vocab <= 0, ldl < vocab, rows > slots without
 *     slot_of_row, repetition_penalty <= 0, a penalty != 1 without seen, ld_seen too small, and when sampling temperature <= 0, top_p
 *     outside (0, 1], top_k < 0, u and draws both NULL.  LLARK_ERR_UNSUPPORTED: vocab > 65536.
 *   llark_seen_mark_rows: sets, in seen[slot_of_row[r]] (NULL: slot r), the bits of ids[offs[r] .. offs[r] + lens[r]) for r < rows (ids
 *     int64 [n_ids]; offs, lens int32 [rows]).  Ids outside [0, vocab), rows with a slot outside [0, slots) or a range outside [0, n_ids)
 *     are ignored.  Clearing a slot is a memset of its row by the caller. */
int llark_sample_rows(const float* logits, int ldl, int vocab, int rows, int slots, const int* state, const int* slot_of_row,
                      unsigned* seen, int ld_seen, int do_sample, float temperature, int top_k, float top_p, float repetition_penalty,
                      const float* u, long long seed, int* draws, const int64_t* stream_id, int64_t* choice, int* kept, float* thresh,
                      int* fallbacks, llark_stream_t stream);
int llark_seen_mark_rows(const int64_t* ids, long long n_ids, const int* offs, const int* lens, const int* slot_of_row, int rows,
                         int slots, int vocab, unsigned* seen, int ld_seen, llark_stream_t stream);
/* Token log-probabilities on the device (csrc/logprob.hip): what the model's own distribution -- log-softmax of the RAW logits, before any
 * repetition penalty, temperature, top-k or top-p -- gives the token tokens[r], for the rows of a decode step, a prefill or a scored text.
 *   llark_token_logprob_rows: one workgroup per row r of logits fp32 [rows][ldl] (columns >= vocab are never read).  slot = slot_of_row[r]
 *     (int32 [rows], NULL: slot = r; rows map to DISTINCT slots).  A row is skipped -- nothing of it is read, nothing is written for it --
 *     when its slot is outside [0, slots), when state != NULL (int32 [slots] of LLARK_ROW_*) and the slot is not LLARK_ROW_ACTIVE, or when
 *     tokens[r] (int64 [rows]) is outside [0, vocab): a negative token is the caller's "no target here" mark.  Otherwise, with t =
 *     tokens[r], M = max_i l_i and S = sum_i expf(l_i - M) over i < vocab, all in fp32:
 *       logprob[r] = (l_t - M) - logf(S);  rank[r] (nullable) = the number of i with l_i > l_t, exact; 0: t is a greedy token.
 *       A -inf logit adds 0 to S; a target whose logit is -inf gets -inf.  A row that holds a NaN, or whose maximum is +-inf, gets
 *       logprob[r] = NaN and rank[r] = -1.
 *     Per-slot history (hist fp32 [slots][ld_hist], count int32 [slots], total fp32 [slots]; each nullable, hist needs count): when
 *       count[slot] < ld_hist, hist[slot][count[slot]] = logprob[r]; then total[slot] += logprob[r] and count[slot] += 1.  The caller
 *       zeroes count and total when a slot starts a new sequence, and reads a finished sequence's history in one transfer.
 *     S is summed in a fixed order (thread tid takes the columns tid, tid + 1024, ... in order; a butterfly over the 64 lanes; the 16
 *       wave sums in wave order: at most ceil(vocab / 1024) + 21 additions on a path): logprob[r] is bit-reproducible and depends on
 *       the row's vocab floats and on t alone, not on r, the slot, rows, ldl or the row's alignment.  Any vocab; a row of up to 51 200
 *       columns is read from memory once.
 *     LLARK_ERR_INVALID before any launch: a null logits / tokens / logprob, rows, slots or vocab <= 0, ldl < vocab, rows > slots without
 *     slot_of_row, hist without count, ld_hist <= 0 with hist. */
int llark_token_logprob_rows(const float* logits, int ldl, int vocab, int rows, int slots, const int* state, const int* slot_of_row,
                             const int64_t* tokens, float* logprob, int* rank, float* hist, int ld_hist, int* count, float* total,
                             llark_stream_t stream);
/* Beam search on the device (csrc/beam.hip): the step of HF 4.29.2's beam_search + BeamSearchScorer with one beam group, after the logits.
 * Example e of n_examples owns the `beams` (B, 1 .. 16) consecutive slots e * B .. e * B + B - 1; a beam's RANK (its place in HF's order) and
 * its SLOT are different things: rank_of_slot int32 [slots].
 *   llark_beam_topk_rows: one workgroup per row r of logits fp32 [rows][ldl]; slot_of_row, state and the skip rules are those of
 *     llark_token_logprob_rows (a skipped row: nothing read, nothing written).  With lp(t) = (l_t - M) - logf(S) -- M, S and therefore lp
 *     bit-equal to llark_token_logprob_rows for that row and token (same column ownership, same summation order) -- and cand(t) =
 *     fp32(score[slot] + lp(t)) (score fp32 [slots]), the 2B largest candidates of the row, ordered by cand descending, then t ascending:
 *       cand_score fp32 [rows][2B], cand_token int32 [rows][2B], cand_logprob fp32 [rows][2B] (= lp of that token).
 *     A row that holds a NaN, or whose maximum is +-inf: all 2B entries are (-inf, -1, -inf) and *fallbacks (nullable) += 1.  Any vocab; a
 *     row of up to 51 200 columns is read from memory once.  Bit-reproducible: depends on the row's floats and the score alone.
 *     LLARK_ERR_INVALID before any launch: a null logits / score / cand_*, beams outside 1 .. 16, vocab < 2B, ldl < vocab, rows or slots
 *     <= 0, rows > slots without slot_of_row.
 *   llark_beam_advance: one workgroup per example, from the B * 2B candidates of its slots (cand_* indexed [slot][2B]: row = slot); a merge
 *     of sorted lists, no second pass over the vocabulary.  An example with done[e] != 0 only gets next_ids = pad, an empty trellis row
 *     (-1, -1, NaN) and pair_count[e] = 0.  Otherwise, with cur_len[e] the length, prompt included, before the new token:
 *       the top 2B of the example's candidates are walked in the order cand descending, rank ascending, token ascending; k = place in
 *       that order.  token == eos (eos >= 0): k >= B skipped, k < B a hypothesis (sum = cand, length = cur_len, end step = step, end slot =
 *       the beam's global slot: its tokens are that beam's, without the eos).  A token of -1 is never taken.  Anything else becomes the live
 *       beam of the next free rank; the walk ends with the B-th.
 *       Adding a hypothesis: score = fp32(sum / length^length_penalty) (the quotient in double); kept when the heap holds fewer than B or
 *       score > worst, replacing the lowest score (the earliest arrival among equals).
 *       done[e] |= heap full and (early_stopping or worst >= fp32(cand of k = 0 / cur_len^length_penalty)); also when fewer than B live
 *       beams were found.  A done example's slots become LLARK_ROW_FINISHED and emit pad, from this step on.
 *       Slots: the first accepted child of a parent stays in the parent's slot; every further child takes, in rank order, the lowest slot
 *       whose old beam has no child this step, and (src = parent's slot, dst = that slot) is appended to the example's copy list: every
 *       copy reads a slot that is not written this step and writes a slot that nobody reads.
 *     Written: score, rank_of_slot, next_ids int64 [slots] (token of the beam now in that slot), state, pos_rows[slot] += 1 for the B slots
 *       (pos_rows nullable: the step on the prefill logits advances nothing), cur_len[e] += 1, done[e],
 *       trellis int32 [max_steps][slots][3]: row `step`, entry of a slot = (parent's global slot, token, bits of the token's fp32 lp); rows are
 *         never rewritten, a hypothesis' tokens are found by walking parents from (end step - 1, end slot);
 *       heap int32 [n_examples][B][8] = {score f32, sum f32, length, end step, end slot, order of arrival, lp of the closing eos f32, 0},
 *       heap_meta int32 [n_examples][4] = {count, worst score f32 (caller: 1e9 while empty), arrivals, 0};
 *       pairs int32 [n_examples][max(B - 1, 1)][2] = (src, dst) global slots, pair_count int32 [n_examples].
 *     LLARK_ERR_INVALID before any launch: a null pointer other than pos_rows, beams outside 1 .. 16, n_examples outside 1 .. 4096, step
 *     outside [0, max_steps), a length_penalty that is not finite.
 *   llark_kv_copy_slots: for entry i < count[l] of list l of a copy table in DEVICE memory (pairs int32 [n_lists][list_stride][2], count int32
 *     [n_lists]; one list with its count is n_lists = 1): positions [p0[dst], pos_rows[src]) of cache slot src into slot dst, every layer,
 *     the lo planes too when given (both or none).  p0 int32 [slots] holds multiples of 8; layout, 16-byte chunks and the rule for V^T rows
 *     (positions up to round_up(pos_rows[src], 8) - 1 of dst are overwritten, nothing else) are those of llark_kv_copy_prefix.  The grid is
 *     sized from max_span, the caller's upper bound on pos_rows[src] - p0[dst].  Nothing is copied for an entry at or past its count, with a
 *     slot outside [0, slots), with src == dst, with a p0 that is negative or no multiple of 8, an empty span, pos_rows[src] > smax or a
 *     span above max_span.  LLARK_ERR_INVALID before any launch: a null pointer or one lo plane only, hd != 128, smax % 8 != 0, layers *
 *     nh > 65535, n_lists * list_stride outside 1 .. 1024, max_span outside 1 .. smax.
 *   No workgroup waits for another; the only atomic is the add on *fallbacks. */
int llark_beam_topk_rows(const float* logits, int ldl, int vocab, int rows, int slots, const int* state, const int* slot_of_row,
                         const float* score, int beams, float* cand_score, int* cand_token, float* cand_logprob, int* fallbacks,
                         llark_stream_t stream);
int llark_beam_advance(const float* cand_score, const int* cand_token, const float* cand_logprob, int n_examples, int beams, int step,
                       int max_steps, int64_t eos, int64_t pad, float length_penalty, int early_stopping, float* score, int* rank_of_slot,
                       int* state, int* pos_rows, int* cur_len, int64_t* next_ids, int* heap, int* heap_meta, int* done, int* trellis,
                       int* pairs, int* pair_count, llark_stream_t stream);
int llark_kv_copy_slots(void* k_cache, void* vt_cache, void* k_cache_lo, void* vt_cache_lo, int layers, int slots, int nh, int hd, int smax,
                        const int* pairs, const int* count, int n_lists, int list_stride, const int* p0, const int* pos_rows, int max_span,
                        llark_stream_t stream);
/* llark_beam_advance_open: llark_beam_advance for a search inside a closed set (llark_guide_rows), where an example soon has fewer
 * continuations than beams.  Two differences: a candidate whose cand_score is -inf is never taken (the row of a slot that holds no
 * beam: its score is -inf, as the left-over slots of llark_beam_advance are written), and an example with fewer than B live beams goes
 * on -- done[e] is set when NO live beam was found, or by the heap rule.  The left-over slots stay LLARK_ROW_ACTIVE, are fed pad, and
 * take a beam again when a later step forks into them (their K/V span is copied whole, from p0).  Everything else as llark_beam_advance. */
int llark_beam_advance_open(const float* cand_score, const int* cand_token, const float* cand_logprob, int n_examples, int beams, int step,
                            int max_steps, int64_t eos, int64_t pad, float length_penalty, int early_stopping, float* score,
                            int* rank_of_slot, int* state, int* pos_rows, int* cur_len, int64_t* next_ids, int* heap, int* heap_meta,
                            int* done, int* trellis, int* pairs, int* pair_count, llark_stream_t stream);
/* Constrained decoding on the device (csrc/constrain.hip): the tokens that HF 4.29.2's NoRepeatNGram, NoBadWords, MinLength and
 * MinNewTokensLength processors ban for a row's next choice, from the row's token history, which lives in device memory.
 *   llark_constrain_rows: one workgroup of 1024 threads per row r of logits fp32 [rows][ldl]; slot_of_row, state and the skip rules are
 *     those of llark_token_logprob_rows (a skipped row: nothing read, nothing written, its history untouched).  Per-slot state: hist int32
 *     [slots][ld_hist], hist_len int32 [slots], prompt_len int32 [slots] (nullable: 0).  hist == NULL (then hist_len, prompt_len, parent and
 *     last_token are NULL too): every row has the empty history.  In order, with L = hist_len[slot] clamped to [0, ld_hist]:
 *       1. fork: parent (nullable) is int32 with an element stride -- entry of a slot at parent[slot * parent_stride], so column 0 of a
 *          trellis row of llark_beam_advance can be passed as it lies.  p = that entry; p outside [0, slots) counts as p = slot.  When p !=
 *          slot, hist[p][0 .. L) is copied into hist[slot]: the slot's OWN length, since the beams of an example advance together and
 *          hist_len[p] is being written by another workgroup.  Race-free in place by the slot rule of llark_beam_advance: a slot that is
 *          read keeps its own beam this step, and the only write to its row is at position L.
 *       2. append: last_token int64 [slots] (nullable: a prefill row, whose history is its prompt) holds the token this row's logits were
 *          computed from: hist[slot][L] = it, hist_len[slot] = L + 1.  When L == ld_hist nothing is appended and bit 0 of *status
 *          (nullable) is set; nothing is ever written outside the row.  An id outside int32 is stored as -1.
 *       3. bans, over the history h[0 .. L') after the append:
 *          no_repeat_ngram = n (0: off), when L' + 1 >= n: x is banned if some i in [0, L' - n] has h[i .. i+n-1) == h[L'-n+1 .. L') and
 *            x == h[i+n-1]; n = 1 bans every token of the history;
 *          bad words: a flat table bw_tokens int32 [bw_total] with bw_off int32 [n_words + 1] (word w = bw_tokens[bw_off[w] .. bw_off[w+1]),
 *            k tokens), when k - 1 <= L': x = w[k-1] is banned if h[L'-k+1 .. L') == w[0 .. k-1) (4.29.2's _tokens_match); a word whose
 *            offsets are not 0 <= bw_off[w] < bw_off[w+1] <= bw_total is ignored;
 *          eos (>= 0) is banned while L' - prompt_len[slot] < min_new_tokens or L' < min_length.
 *          A history or table token outside [0, vocab) takes part in comparisons and never bans anything.
 *       4. outputs, each nullable but not all three: out fp32 [rows][ldo] = the row's raw bits, -inf at banned columns (columns >= vocab
 *          are not written); ban uint32 [slots][ld_ban], row of the SLOT: bit (t & 31) of word t >> 5, words [0, ceil(vocab / 32));
 *          n_banned int32 [rows].
 *     Caps: vocab <= 65536 (LLARK_ERR_UNSUPPORTED above, as llark_sample_rows), no_repeat_ngram <= 64, n_words <= 4096, bw_total <= 2^20.
 *     LLARK_ERR_INVALID before any launch: a null logits, all of out / ban / n_banned null, rows, slots or vocab <= 0, ldl < vocab, rows >
 *     slots without slot_of_row, hist without hist_len or the reverse, ld_hist <= 0 with hist, parent / last_token / prompt_len without
 *     hist, parent_stride < 1, no_repeat_ngram outside 0 .. 64 or > 0 without hist, a word table above the caps, with bw_total < n_words
 *     or without its pointers, a negative min_new_tokens / min_length, ldo < vocab, ld_ban < ceil(vocab / 32).
 *     No workgroup waits for another; no global atomics (the bitmap is built in LDS).
 *   llark_beam_topk_rows_banned: llark_beam_topk_rows with ban uint32 [slots][ld_ban] as llark_constrain_rows writes it: a banned column
 *     is left out of the selection only -- it still counts in M and S, so cand_logprob stays bit-equal to llark_token_logprob_rows.  A row
 *     with fewer than 2B columns left fills the rest with (-inf, -1, -inf).  LLARK_ERR_INVALID additionally: a null ban, ld_ban too small. */
int llark_constrain_rows(const float* logits, int ldl, int vocab, int rows, int slots, const int* state, const int* slot_of_row, int* hist,
                         int ld_hist, int* hist_len, const int* prompt_len, const int* parent, int parent_stride, const int64_t* last_token,
                         int no_repeat_ngram, const int* bw_tokens, const int* bw_off, int n_words, int bw_total, int64_t eos,
                         int min_new_tokens, int min_length, float* out, int ldo, unsigned* ban, int ld_ban, int* n_banned, int* status,
                         llark_stream_t stream);
int llark_beam_topk_rows_banned(const float* logits, int ldl, int vocab, int rows, int slots, const int* state, const int* slot_of_row,
                                const float* score, int beams, float* cand_score, int* cand_token, float* cand_logprob, int* fallbacks,
                                const unsigned* ban, int ld_ban, llark_stream_t stream);
/* Guided choice on the device (csrc/guide.hip): a row may only continue inside a closed set of token sequences -- HF 4.29.2's
 * PrefixConstrainedLogitsProcessor with the set given as data, a prefix tree in device memory, instead of a host callback.
 *   llark_guide_rows: one workgroup of 1024 threads per row r of logits fp32 [rows][ldl]; slot_of_row, state and the skip rules are those
 *     of llark_token_logprob_rows (a skipped row: nothing read, nothing written, its node untouched in BOTH buffers).
 *     Table (CSR, read only): child_off int32 [n_nodes + 1]; child_tok int32 [n_edges], ascending and distinct within a node; child_node
 *       int32 [n_edges]; terminal int32 [n_nodes] (non-zero: a whole sequence ends here).  The roots of all sets of a call are nodes of
 *       the one table.  Per-slot state: node_in int32 [slots] is only read, node_out int32 [slots] only written (two buffers; the caller
 *       swaps them after the launch): under beams a slot reads its parent's node while the parent's own workgroup advances it.  Node
 *       values: >= 0 a node of the table, -1 unconstrained, -2 closed (only eos is allowed); anything else counts as -2.
 *     In order:
 *       1. parent (nullable) is int32 with an element stride, as in llark_constrain_rows -- a trellis column can be passed as it lies.
 *          p = parent[slot * parent_stride]; p outside [0, slots) counts as p = slot.  n = node_in[p].
 *       2. advance: last_token int64 [slots] (nullable: a prefill row) holds the token this row's logits were computed from.  When it
 *          is given and n >= 0: n' = the child of n under that token; without such a child n' = -2, and bit 1 of *status (nullable) is
 *          set unless the token is eos and terminal[n] is set.  With n < 0 or a prefill row n' = n.  Then node_out[slot] = n'.
 *       3. allowed: the tokens of the children of n'; eos when terminal[n'] is set or n' == -2; everything when n' == -1.  A child token
 *          outside [0, vocab) allows nothing.  A fan-out above 1024 is strided over the threads.
 *       4. outputs, each nullable but not all three: out fp32 [rows][ldo] = the row's raw bits (NaN and -inf included) at allowed
 *          columns, -inf elsewhere; out == logits with ldo == ldl is in place; columns >= vocab are not written.  ban uint32
 *          [slots][ld_ban], row of the SLOT, in the layout of llark_constrain_rows (bit set: NOT allowed; bits of columns >= vocab stay
 *          clear): stored, or with ban_accumulate != 0 OR-ed into what is there, so that it composes with that kernel's bitmap for
 *          llark_beam_topk_rows_banned.  n_open int32 [rows]: the allowed columns whose logit is neither -inf nor NaN; when it is 0,
 *          bit 2 of *status is set.
 *     Caps: vocab <= 65536 (LLARK_ERR_UNSUPPORTED above, as llark_sample_rows), n_nodes in 1 .. 2^20, n_edges <= 2^20.
 *     LLARK_ERR_INVALID before any launch: a null logits / child_off / terminal / node_in / node_out, edges without child_tok /
 *     child_node, all of out / ban / n_open null, rows, slots or vocab <= 0, ldl < vocab, rows > slots without slot_of_row, a table
 *     above the caps, node_in == node_out, parent_stride < 1, eos outside [0, vocab), ldo < vocab (in place: ldo != ldl), ld_ban <
 *     ceil(vocab / 32).
 *     No workgroup waits for another; the allowed set is built in LDS; the only global atomic is the OR on *status. */
int llark_guide_rows(const float* logits, int ldl, int vocab, int rows, int slots, const int* state, const int* slot_of_row,
                     const int* child_off, const int* child_tok, const int* child_node, const int* terminal, int n_nodes, int n_edges,
                     const int* node_in, int* node_out, const int* parent, int parent_stride, const int64_t* last_token, int64_t eos,
                     float* out, int ldo, unsigned* ban, int ld_ban, int ban_accumulate, int* n_open, int* status,
                     llark_stream_t stream);
/* MPT ragged decode step, the whole attention front in one launch (m2t/llava/model/mpt/attention.py: qkv.clamp_ -> q_ln / k_ln ->
 * head split -> attention with the ALiBi bias; replaces llark_clamp_f32 + 2 x llark_layernorm_f32 + llark_attn_decode_rope_bf16_rows
 * with identity tables).  qkv fp32 [batch][ldq], laid out q | k | v with nh*128 columns each, is READ ONLY.  Workgroup (h, b) reads
 * p = pos_rows[b]; p < 0 or p >= smax: idle slot, nothing is written to its caches and its output head is zero.  Otherwise, for its own
 * 128 columns of q, k and v: (1) clamp to +-clip_qkv (clip_qkv <= 0: no clamp; v too; a NaN is kept); (2) when q_ln_w != NULL the
 * LayerNorm of q_ln / k_ln over the WHOLE nh*128-wide clamped q row, respectively k row (fp32 statistics, two-pass mean / variance,
 * recomputed per workgroup; q_ln_w and k_ln_w come together, q_ln_b / k_ln_b are nullable on their own); (3) rounding to the bf16
 * plane(s) as llark_rope_split_heads does (lo planes: all or none); (4) k appended at row p of slot b's K cache, v at column p of its
 * V^T cache; (5) attention over keys 0 .. p with alibi_slopes[h] * (j - p) added to the scaled scores.  Caches k [batch][nh][smax][128],
 * v^T [batch][nh][128][smax]; out bf16 [batch][nh * 128]; dynamic LDS holds smax scores.  hd == 128, smax % 8 == 0, nh*128 <= 8192,
 * alibi_slopes != NULL, ldq >= 3*nh*128, ldq % 4 == 0, qkv 16-byte aligned; anything else: LLARK_ERR_UNSUPPORTED / LLARK_ERR_INVALID
 * before any launch.  No atomics, no waiting between workgroups. */
int llark_mpt_attn_decode_rows(const float* qkv, int ldq, int batch, int nh, int hd, const int* pos_rows, float clip_qkv,
                               const float* q_ln_w, const float* q_ln_b, const float* k_ln_w, const float* k_ln_b, float ln_eps,
                               void* k_cache, void* vt_cache, void* k_cache_lo, void* vt_cache_lo, int smax, void* out, void* out_lo,
                               const float* alibi_slopes, llark_stream_t stream);
/* Shared prompt prefix in the ragged slot mode (csrc/attn_shared.hip).  Under the contract of infer_from_webdataset.py every
 * (question, answer) pair of a sample is its own example and all of them start with the same audio block: the slots of one clip hold
 * the same K/V at their first positions.
 *   llark_kv_copy_prefix (engine.fork_slots: a sibling's slot receives the prefix instead of prefilling it): positions [0, n) of cache
 *     slot `src` into each of the n_dst slots of `dst` (a HOST array), all layers, the lo planes too when given (both or none).  Whole
 *     caches: k [layers][slots][nh][smax][128], v^T [layers][slots][nh][128][smax].  V^T rows move in 16-byte chunks, so positions
 *     n .. round_up(n, 8) - 1 of a destination are overwritten too (dead until the decode step appends there, like pad positions);
 *     nothing at or beyond round_up(n, 8) is written.  LLARK_ERR_UNSUPPORTED: n outside 1 .. smax, src among dst, a slot twice in dst,
 *     more than 64 destinations, hd != 128, smax % 8 != 0.
 *   llark_attn_decode_rope_bf16_shared (engine.decode_slots with share_prefix): llark_attn_decode_rope_bf16_rows -- same arguments,
 *     same caches, same outputs, no ALiBi -- plus a group table in DEVICE memory:
 *       groups int32 [n_groups][19] = {source slot, P, members m (1 .. 16), member slot 0 .. m - 1, unused};
 *       slot_shared int32 [batch]: P of the slot's group, 0 = in no group.
 *     Keys [0, P) of a member are read from the source slot's cache, once for the whole group (they must be bit-identical to the
 *     member's own; P % 8 == 0, P <= the position of every member and of the source); keys [P, pos] from the member's own cache.  A
 *     slot with slot_shared == 0 gets exactly the bits of llark_attn_decode_rope_bf16_rows, output and caches.  Two launches in stream
 *     order (group pass, per-slot pass + merge); no workgroup waits for another.  scratch: caller-owned, 16-byte aligned, at least
 *     llark_attn_decode_shared_scratch_bytes(batch, nh) bytes = 64 + batch * nh * 4 key ranges * 132 floats, zeroed once by the caller;
 *     its first int32 is a status word: the table lives on the device, so the KERNEL refuses a bad one -- it stores a nonzero code
 *     there (1: P not a positive multiple of 8 or > smax, 2: members outside 1 .. 16, 3: P greater than a member's position, or that
 *     member idle or at smax, 4: source slot inactive or shorter than P, 5: member slot out of range or slot_shared[member] != P),
 *     the group pass of that group computes nothing and the outputs of its members are undefined.  The word is sticky: the caller
 *     reads and clears it (ops.attn_decode_shared_status).  LLARK_ERR_UNSUPPORTED from the host: hd != 128, n_groups > batch,
 *     smax > 32768. */
int llark_kv_copy_prefix(void* k_cache, void* vt_cache, void* k_cache_lo, void* vt_cache_lo, int layers, int slots, int nh, int hd,
                         int smax, int src, const int* dst, int n_dst, int n, llark_stream_t stream);
long long llark_attn_decode_shared_scratch_bytes(int batch, int nh);
int llark_attn_decode_rope_bf16_shared(const float* qkv, int batch, int nh, int hd, const int* pos_rows, const float* cos_t,
                                       const float* sin_t, int max_pos, void* k_cache, void* vt_cache, void* k_cache_lo,
                                       void* vt_cache_lo, int smax, void* out, void* out_lo, const int* groups, int n_groups,
                                       const int* slot_shared, void* scratch, long long scratch_bytes, llark_stream_t stream);
/* Decode-step forms with the sequence position in DEVICE memory (*pos_dev = tokens already cached = position of the
 * new token; s = 1): lets ONE captured hipGraph of the whole decode step serve every generated token of
 * m2t/models/llamav2.py:339-365 / m2t/infer.py:137-148. */
int llark_rope_split_heads_dpos(const float* qkv, int batch, int nh, int hd, const int* pos_dev, const float* cos_t,
                                const float* sin_t, void* q, void* k_cache, void* vt_cache, void* q_lo, void* k_cache_lo,
                                void* vt_cache_lo, int smax, llark_stream_t stream);
int llark_attn_decode_bf16_dpos(const void* q, const void* k_cache, const void* vt_cache, const void* q_lo,
                                const void* k_cache_lo, const void* vt_cache_lo, int batch, int nh, int hd,
                                const int* pos_dev, int smax, void* out, void* out_lo, llark_stream_t stream);
/* CrossEntropyLoss on shifted logits (m2t/models/llamav2.py:316-325). logits fp32 [batch*s][ldl]; labels
 * int64 [batch][s]; row_loss scratch float[batch*s]; loss_out float[2] = {mean loss, counted rows}.  A target outside
 * [0, vocab) is treated like ignore_index: its row is not counted and gets a zero gradient (torch raises there). */
int llark_cross_entropy_shifted(const float* logits, int ldl, int batch, int s, int vocab, const int64_t* labels,
                                int64_t ignore_index, float* row_loss, float* loss_out, llark_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Training step of the LLM half: backward / optimizer pieces around the GEMMs (m2t/train.py:53-277 -> HF Trainer:
 * WrappedLlamav2ForCausalLM.forward(labels), loss.backward(), AdamW; scripts/training/train_llark.sh:20-49).
 * ------------------------------------------------------------------------------------------- */
/* dst[b][c][r] = src[b][r][c] (16-bit), dst columns [rows, ld_dst) zero-filled. */
int llark_transpose16(const void* src, int ld_src, int rows, int cols, void* dst, int ld_dst, int batch,
                      long long stride_src, long long stride_dst, llark_stream_t stream);
/* x [batch*s][nh*hd] (16-bit) -> y [batch][nh][s][hd] */
int llark_split_heads16(const void* x, int batch, int s, int nh, int hd, void* y, llark_stream_t stream);
/* P[b][i][j] = softmax_j(scale*scores[b][i][j]), j <= i (bf16, pitch ldp, zero elsewhere). scores fp32 [batch][s][s]. */
int llark_causal_softmax_rows(const float* scores, int batch, int s, float scale, void* p_out, int ldp, llark_stream_t stream);
/* softmax backward: dS = P o (dP - rowsum(P o dP)) * scale  (bf16, pitch ldp) */
int llark_attn_ds(const void* p, const float* dp, int batch, int s, float scale, void* ds_out, int ldp, llark_stream_t stream);
/* RoPE backward + merge heads: dq/dk/dv fp32 [batch][nh][s][hd] -> dqkv bf16 [batch*s][3*nh*hd] */
int llark_rope_merge_bwd(const float* dq, const float* dk, const float* dv, const float* cos_t, const float* sin_t, int batch,
                         int s, int nh, int hd, int pos0, void* dqkv, llark_stream_t stream);
/* LlamaRMSNorm backward: dx (=|+=) ..., dw += ... (fp32 atomics) */
int llark_rmsnorm_bwd(const float* x, const float* w, const float* dy, int rows, int width, float eps, float* dx, int accumulate,
                      float* dw, llark_stream_t stream);
/* ... that also writes the final dx as bf16 [rows][ld16] (ld16 >= width, a multiple of 4): the A operand of the products that follow in the
 * training step, without a llark_split16 pass over the fp32 tensor (same rounding as its hi plane). */
int llark_rmsnorm_bwd_out16(const float* x, const float* w, const float* dy, int rows, int width, float eps, float* dx, int accumulate,
                            float* dw, void* dx16, int ld16, llark_stream_t stream);
/* SwiGLU on the interleaved [32 gate | 32 up] layout: gu fp32 [rows][2*inter] */
int llark_swiglu_fwd(const float* gu, int rows, int inter, void* act, llark_stream_t stream);
int llark_swiglu_bwd(const float* gu, const float* dact, int rows, int inter, void* dgu, llark_stream_t stream);
/* out (one double in device memory) (= | +=) sum_i x[i]^2 over n contiguous fp32 values: the squared global gradient norm behind HF
 * Trainer's clip_grad_norm_ (transformers TrainingArguments.max_grad_norm = 1.0, not overridden by scripts/training/train_llark.sh;
 * reached from m2t/train.py:53-277 -> trainer.train()).  accumulate == 0 zeroes `out` on the stream first; != 0 adds to it, so the
 * norm can be collected slice by slice while the backward is still running. */
int llark_sumsq_f32(const float* x, long long n, double* out, int accumulate, llark_stream_t stream);
/* d(mean shifted CE)/dlogits * loss_scale as bf16 [batch*s][ldd]; row_loss / loss_cnt come from llark_cross_entropy_shifted */
int llark_cross_entropy_bwd(const float* logits, int ldl, int batch, int s, int vocab, const int64_t* labels,
                            const float* row_loss, const float* loss_cnt, float loss_scale, void* dlogits, int ldd,
                            llark_stream_t stream);
int llark_colsum_f32(const float* x, int ld, int rows, int cols, float* out, llark_stream_t stream);
int llark_gather_rows_f32(const float* src, int ld_src, const int64_t* idx, int n, int cols, float* dst, int ld_dst,
                          llark_stream_t stream);
int llark_scatter_add_rows_f32(const float* src, int ld_src, const int64_t* idx, int n, int cols, float* dst, int ld_dst,
                               llark_stream_t stream);
/* torch.optim.AdamW step on bf16 (param_dtype 1) or fp32 (2) parameters with fp32 gradients (scaled by grad_scale) and moments */
int llark_adamw(int param_dtype, void* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                float eps, float weight_decay, int step, float grad_scale, llark_stream_t stream);
/* the same step with HF Trainer's clip_grad_norm_ (TrainingArguments.max_grad_norm) applied on the device: grad_sumsq = the squared norm
 * of the whole unscaled gradient (llark_sumsq_f32, device memory); gradients are multiplied by
 * grad_scale * min(1, max_grad_norm / (sqrt(*grad_sumsq) * grad_scale + 1e-6)) -- no host read between backward and update. */
int llark_adamw_clip(int param_dtype, void* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                     float eps, float weight_decay, int step, float grad_scale, const double* grad_sumsq, float max_grad_norm,
                     llark_stream_t stream);
/* Decode-step launches that overlap across their boundaries (round 6; model.generate -> LlamaModel.forward with ONE new token,
 * m2t/infer.py:146, m2t/models/llamav2.py:339-365): a chained consumer is launched on ANOTHER stream while its producer still runs; it fills
 * its LDS ring with weights (64 KiB per workgroup: it fits a CU next to the producer's workgroup), waits until the producer's monotonic
 * arrival counter *wait has reached wait_target before it reads activations / the residual, and adds 1 per workgroup to *signal when its own
 * outputs are written and released.  Counters are caller-owned device words (zeroed once); a producer launch advances its counter by its
 * grid size: llark_gemv16_dma_blocks(epilogue, n) for the Linears, nh * batch for the attention.  The spin is bounded (a lost producer gives
 * wrong data, never a hung GPU).  Results equal the unchained entry points (llark_gemv16_dma, llark_gemv16_dma_rmsnorm,
 * llark_attn_decode_rope_bf16).  llark_gemv16_dma_chain: x != NULL selects the RMSNorm-fused form; m == 1, kp <= 4096. */
int llark_gemv16_dma_blocks(int epilogue, int n);
int llark_gemv16_dma_chain(int split, int epilogue, const void* a_hi, const void* a_lo, int lda, const float* x, int ldx, const float* norm_w,
                           float eps, const void* wt, int ldw, const float* bias, int m, int n, int kp, float* c, int ldc, const float* resid,
                           int ldr, void* out_hi, void* out_lo, int ldo, const unsigned* wait, unsigned wait_target, unsigned* signal,
                           llark_stream_t stream);
int llark_attn_decode_rope_bf16_chain(const float* qkv, int batch, int nh, int hd, int pos, const int* pos_dev, const float* cos_t,
                                      const float* sin_t, int max_pos, void* k_cache, void* vt_cache, void* k_cache_lo, void* vt_cache_lo,
                                      int smax, void* out, void* out_lo, const float* alibi_slopes, unsigned* done, llark_stream_t stream);
/* Layout glue of the Llama training step folded into the kernels around it (round 6; torch autograd of LlamaAttention.forward under
 * WrappedLlamav2ForCausalLM.forward + loss.backward(), m2t/models/llamav2.py:259-337, m2t/train.py:53-277):
 *   llark_gemm16_fragw_rope_qkv_train: llark_gemm16_fragw_rope_qkv in the plain bf16 mode that ALSO writes V row-major,
 *     v_rm [batch][nh][s][128] (the attention backward's operand; no llark_transpose16 of the V^T cache);
 *   llark_attn_backward_bf16_fused: llark_attn_backward_bf16 that reads dO TOKEN-major ([batch*s][ld_do], head h at column 128 h: what the
 *     o_proj dX product leaves; no llark_split_heads16) and writes d(q | k | v) of the fused projection as bf16 dqkv [batch*s][3 nh 128] with
 *     the RoPE backward applied to the q and k parts (bit-equal to llark_rope_merge_bwd over the fp32 outputs of llark_attn_backward_bf16).
 *     As there: o and lse are used as given, K-cache rows >= s are never read, dsum is an output holding rowsum(dO * o).  Of dO only the
 *     columns [0, nh 128) of a row are read; dO must be 16-byte and dqkv 8-byte aligned, ld_do % 8 == 0; pos0 + s <= max_pos. */
int llark_gemm16_fragw_rope_qkv_train(const void* a, int lda, const void* wfrag, int kp, int batch, int s, int nh, int hd, int pos0,
                                      const float* cos_t, const float* sin_t, int max_pos, void* q, void* k_cache, void* vt_cache, int smax,
                                      void* v_rm, llark_stream_t stream);
int llark_attn_backward_bf16_fused(const void* q, const void* k_cache, const void* v_rm, const void* dO, int ld_do, const void* o,
                                   const float* lse, float* dsum, int batch, int s, int nh, int hd, int smax, const float* cos_t,
                                   const float* sin_t, int pos0, int max_pos, void* dqkv, llark_stream_t stream);
/* Variable-length (packed) forms of the training pair and its fused backward (csrc/llama.hip, csrc/attn_bwd.hip): a whole optimizer step of
 * ragged sequences as ONE row stream with no padded sequence.  Layouts are those of the uniform calls with batch = 1 and s = s_total:
 * q, v_rm, head-major dO [nh][s_total][128]; k_cache [nh][smax][128]; vt_cache [nh][128][smax]; out, o, token-major dO, dqkv [s_total][..];
 * lse, dsum [nh][s_total].  seqs: DEVICE int32 [nseq][2] = (off_b, len_b): query i of sequence b is row off_b + i and sees keys
 * off_b .. off_b + i, nothing else.  Llama only (no ALiBi), hd == 128.
 *   Table contract: off_b % 8 == 0 (the forward reads V^T in 16-byte chunks of 8 keys, the rule behind smax % 8 == 0); len_b >= 1;
 *   off_b + len_b <= s_total <= smax; ranges disjoint; max_len >= every len_b.  Rows that lie in no sequence are neither read nor written,
 *   in any tensor.  The workgroups of an entry that breaks a rule return without touching memory: no table content can produce an access
 *   outside rows [0, s_total).  (Overlapping ranges stay in bounds; their rows then hold either sequence's result.)
 *   Scalars are checked before any launch (LLARK_ERR_INVALID): null pointer, hd != 128, 0 < max_len <= s_total <= smax, smax % 8 == 0,
 *   max_len <= max_pos.  Results are bit-equal, sequence by sequence, to the uniform entry point called with batch = 1, s = len_b on that
 *   sequence's rows; the fused backward's RoPE uses the position INSIDE the sequence (row off_b + i -> cos_t[i]).  No atomics. */
int llark_attn_prefill_bf16_lse_varlen(const void* q, const void* k_cache, const void* vt_cache, const int* seqs, int nseq, int max_len,
                                       int s_total, int nh, int hd, int smax, void* out, float* lse, llark_stream_t stream);
int llark_attn_backward_bf16_varlen(const void* q, const void* k_cache, const void* v_rm, const void* dO, const void* o, const float* lse,
                                    float* dsum, const int* seqs, int nseq, int max_len, int s_total, int nh, int hd, int smax, float* dq,
                                    float* dk, float* dv, llark_stream_t stream);
int llark_attn_backward_bf16_fused_varlen(const void* q, const void* k_cache, const void* v_rm, const void* dO, int ld_do, const void* o,
                                          const float* lse, float* dsum, const int* seqs, int nseq, int max_len, int s_total, int nh, int hd,
                                          int smax, const float* cos_t, const float* sin_t, int max_pos, void* dqkv, llark_stream_t stream);
/* The variable-length training pair with ALiBi (MPT): the same contract as llark_attn_prefill_bf16_lse_varlen / llark_attn_backward_bf16_varlen
 * plus alibi_slopes fp32 [nh] (null: LLARK_ERR_INVALID).  The bias of sequence b is slope_h * (i - (len_b - 1)) with i the key's position
 * INSIDE the sequence, so out, lse, dsum, dq, dk, dv are bit-equal, sequence by sequence, to llark_attn_prefill_bf16_lse /
 * llark_attn_backward_bf16 called with the same slopes at batch = 1, s = len_b (below the uniform call's 128-query-block threshold). */
int llark_attn_prefill_bf16_lse_varlen_alibi(const void* q, const void* k_cache, const void* vt_cache, const int* seqs, int nseq, int max_len,
                                             int s_total, int nh, int hd, int smax, void* out, float* lse, const float* alibi_slopes,
                                             llark_stream_t stream);
int llark_attn_backward_bf16_varlen_alibi(const void* q, const void* k_cache, const void* v_rm, const void* dO, const void* o, const float* lse,
                                          float* dsum, const int* seqs, int nseq, int max_len, int s_total, int nh, int hd, int smax, float* dq,
                                          float* dk, float* dv, const float* alibi_slopes, llark_stream_t stream);
/* dW = dY^T . X without transposed copies of dY (csrc/gemm_bda.hip, round 6; torch autograd of nn.Linear: grad_weight = grad_output^T .
 * input, under WrappedLlamav2ForCausalLM.forward + loss.backward(), m2t/models/llamav2.py:259-337, m2t/train.py:53-277):
 *   llark_pack_frag_t16: src [kp][ld] 16-bit (row = contraction index: the token; column = feature) -> dst = the fragment-major copy of
 *     src^T ([n][kp]; the layout of llark_pack_weight16_frag), kp % 64 == 0, n % 8 == 0; dst holds round_up(n, 32) * kp elements;
 *   llark_gemm16_ta_fragw: c[m][n] (= | +=) sum_k a[k][m] . B(n, k) with a [kp][lda] bf16 contraction-major (dY as it stands) and wfrag =
 *     B fragment-major (llark_pack_frag_t16 of X).  epilogue LLARK_EPI_F32 / LLARK_EPI_RESID (resid may alias c); sumsq (nullable) += sum of
 *     squares of every stored value (as llark_gemm16_t_sumsq).  m % 8 == 0, kp >= 192; LLARK_ERR_UNSUPPORTED otherwise. */
int llark_pack_frag_t16(const void* src, int ld, int kp, int n, void* dst, llark_stream_t stream);
int llark_gemm16_ta_fragw(int epilogue, const void* a, int lda, const void* wfrag, int m, int n, int kp, float* c, int ldc,
                          const float* resid, int ldr, double* sumsq, llark_stream_t stream);
/* The same product on the 16x16x32 MFMA shape (csrc/gemm_bda16.hip, round 6): per joule that instruction does more, and the training
 * GEMMs run against the power limit.  llark_pack_frag_t16x16 = llark_pack_frag_t16 in 16-row chunks (chunk (feature / 16, token / 32), lane
 * l = the 8 tokens 32 q + 8 (l / 16) .. of feature 16 R + l % 16; same extent); llark_gemm16_ta_fragw16 = llark_gemm16_ta_fragw over it.
 * Additionally kp % 128 == 0, kp >= 256, n / ldc / ldr multiples of 4, c / resid 16-byte aligned: LLARK_ERR_UNSUPPORTED otherwise (the
 * caller keeps llark_gemm16_ta_fragw).  32 products per MFMA: agrees with llark_gemm16_ta_fragw to fp32 rounding, not bit for bit. */
int llark_pack_frag_t16x16(const void* src, int ld, int kp, int n, void* dst, llark_stream_t stream);
int llark_gemm16_ta_fragw16(int epilogue, const void* a, int lda, const void* wfrag, int m, int n, int kp, float* c, int ldc,
                            const float* resid, int ldr, double* sumsq, llark_stream_t stream);
/* The two SwiGLU products of the training step with the element-wise pass in their epilogues (csrc/gemm_bda.hip; HF LlamaMLP.forward and
 * its autograd under WrappedLlamav2ForCausalLM.forward + loss.backward(), m2t/models/llamav2.py:224-234,259-337, m2t/train.py:53-277).
 * Plain bf16 operands, fragment-major weights (llark_pack_weight16_frag / llark_adamw_twins).  gu16 [m][ldg >= 2 I] = the gate | up
 * pre-activations as bf16, interleaved like the fused gate/up weight rows ([32 gate | 32 up] per 64 columns).
 *   mode 0: a = x [m][kp], wfrag = gate|up twin (n = 2 I): out = act [m][ldo >= I] = silu(gate) * up; gu16 is WRITTEN.
 *   mode 1: a = d(h) [m][kp], wfrag = down_proj^T twin (n = I): out = d(gate | up) [m][ldo >= 2 I]; gu16 is READ.
 * LLARK_ERR_UNSUPPORTED when the DMA loop does not take the shape (kp < 192, operand beyond 2 GiB). */
int llark_gemm16_fragw_swiglu_train(int mode, const void* a, int lda, const void* wfrag, int m, int n, int kp, void* out, int ldo,
                                    void* gu16, int ldg, llark_stream_t stream);
/* The bf16 step of llark_adamw / llark_adamw_clip (grad_sumsq nullable = no clipping) on a weight MATRIX p [n][k] that also writes the
 * fragment-major operand twins of the UPDATED weight (what the reference reaches through HF Trainer's optimizer.step(), m2t/train.py:255-260,
 * followed by the next micro-batch's nn.Linear forward / backward, m2t/models/llamav2.py:259-337): wfrag (nullable) =
 * llark_pack_weight16_frag(p), the B operand of the forward product -- rows below rope_rows (the q and k parts of a fused q|k|v weight)
 * in llark_gemm16_fragw_rope_qkv's head-permuted order; wtfrag (nullable) = llark_pack_weight16_frag of p^T ([k][n]), the B operand
 * of dX = dY . W.  n % 32 == 0, k % 128 == 0, wtfrag needs n % 64 == 0, rope_rows % 128 == 0, every pointer 16-byte aligned.
 * Parameters and moments are bit-equal to llark_adamw / llark_adamw_clip. */
int llark_adamw_twins(void* p, const float* g, float* m, float* v, int n, int k, float lr, float beta1, float beta2, float eps,
                      float weight_decay, int step, float grad_scale, const double* grad_sumsq, float max_grad_norm, void* wfrag,
                      int rope_rows, void* wtfrag, llark_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * LoRA adapters on a frozen base (csrc/lora.hip; peft LoraLayer as configured by m2t/train.py:85-92: y = W x + (alpha / r) B (A x)).
 * The low-rank products read one wide bf16 operand once for a 64-wide result: they are memory-bound and get kernels of their own
 * (32-row tiles, the contraction split over the four waves of a workgroup) instead of 16 workgroups of the tiled GEMMs.
 * Every entry point returns LLARK_ERR_UNSUPPORTED for a shape it does not take, before anything is launched.
 * ------------------------------------------------------------------------------------------- */
/* out[rows][ldo] (bf16, columns 0 .. rp_total - 1 of the pointer given: the caller may point into the tail of a wider buffer) =
 * x[rows][lda] . m[rp_total][ldm]^T, bf16 operands, fp32 accumulation over k.  k % 16 == 0, rp_total % 64 == 0, rp_total <= 1024,
 * lda / ldm / ldo % 8 == 0, every pointer 16-byte aligned, operands below 2^31 elements. */
int llark_lora_down(const void* x, int lda, const void* m, int ldm, int rows, int k, int rp_total, void* out, int ldo,
                    void* scratch, long long scratch_bytes, llark_stream_t stream);
/* Bytes of scratch with which llark_lora_down splits the contraction over 2 or 4 workgroups per tile, when its (rows / 32) x
 * (rp_total / 64) tiles alone would leave most of a 256-CU chip idle (0: the shape is not split).  fp32 partial sums, joined in a fixed
 * order by a second small launch.  ``scratch`` NULL or smaller: one workgroup per tile, same result up to the fp32 summation order. */
long long llark_lora_down_scratch_bytes(int rows, int k, int rp_total);
/* Bytes of scratch llark_lora_dw needs for a shape (0 for a shape it does not take). */
long long llark_lora_dw_scratch_bytes(int toks, int big, int rp);
/* g[big][rp] fp32 (= | += when accumulate) scale * P^T . Q, contraction over the toks rows: P bf16 [toks][ldp] whose logical column
 * i is the physical column (i / 32) * p_blk + i % 32 of the pointer given (p_blk = 32: a plain column window; 64: one half of the
 * interleaved gate | up columns), Q bf16 [toks][ldq] (rp columns).  Columns r .. rp - 1 of g (the rank padding) take no gradient: they
 * are written as zero (kept when accumulate).  sumsq (nullable, a double in device memory) += the sum of squares of every value
 * stored to g (as llark_gemm16_t_sumsq).  Token-split partial sums go through `scratch` and a second small launch in a fixed order:
 * no atomics on g, no waits between workgroups, results do not vary from run to run.
 * big % 32 == 0, rp % 64 == 0, rp <= 256, 0 < r <= rp, p_blk % 32 == 0, p and q 4-byte aligned with even ldp / ldq (two adjacent
 * columns are read as one word), g 16-byte aligned, scratch 16-byte aligned and of at least
 * llark_lora_dw_scratch_bytes(toks, big, rp) bytes. */
int llark_lora_dw(const void* p, int ldp, int p_blk, const void* q, int ldq, int toks, int big, int rp, int r, float scale,
                  float* g, int accumulate, double* sumsq, void* scratch, long long scratch_bytes, llark_stream_t stream);
/* bf16 operand copies of one fp32 adapter master src[rows][rp] (the A^T [K][rp] or B [N][rp] factor), times `scale`:
 *   dst   [row_of(i)][ld_dst], columns 0 .. rp - 1 of the pointer given = scale * src[i][:]          (nullable)
 *   dst_t [j][ld_t], column row_of(i) of the pointer given              = scale * src[i][j]          (nullable)
 * with row_of(i) = (i / 32) * blk + i % 32 (blk = 32: identity; 64: the interleaved gate | up rows).  Only these elements are
 * written: the rest of the stacked / block-diagonal operands (other adapters, zero blocks) is neither read nor written.
 * rows % 32 == 0, rp % 32 == 0, blk % 32 == 0. */
int llark_lora_refresh(const float* src, int rows, int rp, float scale, int blk, void* dst, int ld_dst, void* dst_t, int ld_t,
                       llark_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LLARK_HIP_H */
