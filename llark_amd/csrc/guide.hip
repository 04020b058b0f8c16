// Guided choice on the device (llark_guide_rows): a row may only continue inside a closed set of token sequences -- HF 4.29.2's
// PrefixConstrainedLogitsProcessor with the set given as data: a prefix tree in device memory (CSR: child_off / child_tok / child_node /
// terminal) and one node per slot that this launch advances.  One workgroup of 1024 threads per row.  Contract: include/llark_hip.h.
//
// The per-slot node is double-buffered (node_in is only read, node_out only written; the host swaps them): under beams a slot reads its
// PARENT's node while the parent's own workgroup advances it, and two buffers make that race-free without any slot rule.  The allowed set
// is a bitmap in LDS (ceil(vocab / 32) words, vocab <= 65536) whose bits are set with LDS atomicOr, children strided over the threads;
// the row is then streamed once: raw bits where the bit is set, -inf where it is clear.  Every index read from the table or the state
// is range-checked before it is used: whatever they hold, no address outside the arrays is formed.
//
// No workgroup waits for another; plain C++ and vector stores; the only global atomic is the OR on *status.
#include "common.h"

namespace llark {

constexpr int GUIDE_THREADS = 1024;
constexpr int GUIDE_WAVES = GUIDE_THREADS / 64;
constexpr int GUIDE_MAX_VOCAB = 65536;
constexpr int GUIDE_MAX_NODES = 1 << 20;
constexpr int GUIDE_MAX_EDGES = 1 << 20;
constexpr int GUIDE_FREE = -1;                                    // node values: an unconstrained slot
constexpr int GUIDE_CLOSED = -2;                                  // only eos is allowed

struct GuideArgs {
    const float* logits;
    int ldl, vocab, slots;
    const int* state;
    const int* slot_of_row;
    const int* child_off;
    const int* child_tok;
    const int* child_node;
    const int* terminal;
    int n_nodes, n_edges;
    const int* node_in;
    int* node_out;
    const int* parent;
    int parent_stride;
    const long long* last_token;
    int eos;
    float* out;
    int ldo;
    unsigned* ban;
    int ld_ban, ban_accumulate;
    int* n_open;
    int* status;
};

__device__ __forceinline__ bool guide_open(unsigned bits) {       // neither -inf nor a NaN
    return bits != 0xff800000u && (bits & 0x7fffffffu) <= 0x7f800000u;
}

__global__ __launch_bounds__(GUIDE_THREADS) void guide_rows_kernel(const GuideArgs a) {
    __shared__ unsigned bm[GUIDE_MAX_VOCAB / 32];                 // bit set: the column is ALLOWED
    __shared__ int scount[GUIDE_WAVES];
    __shared__ int snext;
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int slot = a.slot_of_row ? a.slot_of_row[r] : r;
    if (slot < 0 || slot >= a.slots) return;                      // workgroup-uniform, like every branch around a barrier below
    if (a.state && a.state[slot] != LLARK_ROW_ACTIVE) return;
    const int vocab = a.vocab, words = (vocab + 31) >> 5;

    // ---- parent, advance ----------------------------------------------------------------------------------------------------------------
    int p = a.parent ? a.parent[(size_t)slot * a.parent_stride] : slot;
    if (p < 0 || p >= a.slots) p = slot;                          // an empty trellis entry: the slot's own node
    int n = a.node_in[p];
    if (n < GUIDE_CLOSED || n >= a.n_nodes) n = GUIDE_CLOSED;     // a value no table holds: closed, never an index
    int n1 = n;
    if (a.last_token && n >= 0) {
        const long long t = a.last_token[slot];
        int c0 = a.child_off[n], c1 = a.child_off[n + 1];
        if (c0 < 0 || c1 > a.n_edges || c1 < c0) c0 = c1 = 0;
        if (tid == 0) snext = GUIDE_CLOSED;
        __syncthreads();
        for (int e = c0 + tid; e < c1; e += GUIDE_THREADS)
            if ((long long)a.child_tok[e] == t) snext = a.child_node[e];      // tokens are distinct within a node: one writer at most
        __syncthreads();
        n1 = snext;
        if (n1 < 0 || n1 >= a.n_nodes) {
            if (tid == 0 && a.status && !(n1 == GUIDE_CLOSED && t == (long long)a.eos && a.terminal[n] != 0)) atomicOr(a.status, 2);
            n1 = GUIDE_CLOSED;
        }
    }
    if (tid == 0) a.node_out[slot] = n1;

    // ---- the allowed set ----------------------------------------------------------------------------------------------------------------
    const unsigned fill = n1 == GUIDE_FREE ? 0xffffffffu : 0u;
    for (int w = tid; w < words; w += GUIDE_THREADS) bm[w] = fill;
    __syncthreads();
    if (n1 >= 0) {
        int c0 = a.child_off[n1], c1 = a.child_off[n1 + 1];
        if (c0 < 0 || c1 > a.n_edges || c1 < c0) c0 = c1 = 0;
        for (int e = c0 + tid; e < c1; e += GUIDE_THREADS) {
            const int x = a.child_tok[e];
            if (x >= 0 && x < vocab) atomicOr(&bm[x >> 5], 1u << (x & 31));
        }
    }
    if (tid == 0 && (n1 == GUIDE_CLOSED || (n1 >= 0 && a.terminal[n1] != 0))) atomicOr(&bm[a.eos >> 5], 1u << (a.eos & 31));
    __syncthreads();

    // ---- outputs ------------------------------------------------------------------------------------------------------------------------
    if (a.ban) {
        unsigned* bo = a.ban + (size_t)slot * a.ld_ban;
        const unsigned tail = (vocab & 31) ? (1u << (vocab & 31)) - 1u : 0xffffffffu;      // columns >= vocab are never banned
        for (int w = tid; w < words; w += GUIDE_THREADS) {
            const unsigned b = ~bm[w] & (w == words - 1 ? tail : 0xffffffffu);
            bo[w] = a.ban_accumulate ? (bo[w] | b) : b;
        }
    }
    const unsigned* src = (const unsigned*)(a.logits + (size_t)r * a.ldl);
    int c = 0;
    if (a.out) {
        const unsigned NEG = 0xff800000u;                         // -inf
        unsigned* dst = (unsigned*)(a.out + (size_t)r * a.ldo);
        const bool vec = ((((size_t)src) | ((size_t)dst)) & 15) == 0;     // workgroup-uniform
        int done = 0;
        if (vec) {
            const int quads = vocab >> 2;
            for (int q = tid; q < quads; q += GUIDE_THREADS) {
                uint4 v = ((const uint4*)src)[q];
                const unsigned b = bm[q >> 3] >> ((q & 7) * 4);   // the four columns of a quad share a bitmap word
                if (b & 1u) c += guide_open(v.x); else v.x = NEG;
                if (b & 2u) c += guide_open(v.y); else v.y = NEG;
                if (b & 4u) c += guide_open(v.z); else v.z = NEG;
                if (b & 8u) c += guide_open(v.w); else v.w = NEG;
                ((uint4*)dst)[q] = v;
            }
            done = quads << 2;
        }
        for (int j = done + tid; j < vocab; j += GUIDE_THREADS) {
            const unsigned v = src[j];
            const bool ok = (bm[j >> 5] >> (j & 31)) & 1u;
            c += ok && guide_open(v);
            dst[j] = ok ? v : NEG;
        }
    } else if (a.n_open) {
        for (int j = tid; j < vocab; j += GUIDE_THREADS)
            if ((bm[j >> 5] >> (j & 31)) & 1u) c += guide_open(src[j]);
    }
    if (a.n_open) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if (lane == 0) scount[wv] = c;
        __syncthreads();
        if (tid == 0) {
            int s = 0;
            for (int w = 0; w < GUIDE_WAVES; ++w) s += scount[w];
            a.n_open[r] = s;
            if (s == 0 && a.status) atomicOr(a.status, 4);
        }
    }
}

}  // namespace llark

using namespace llark;

extern "C" int llark_guide_rows(const float* logits, int ldl, int vocab, int rows, int slots, const int* state, const int* slot_of_row,
                                const int* child_off, const int* child_tok, const int* child_node, const int* terminal, int n_nodes,
                                int n_edges, const int* node_in, int* node_out, const int* parent, int parent_stride,
                                const int64_t* last_token, int64_t eos, float* out, int ldo, unsigned* ban, int ld_ban, int ban_accumulate,
                                int* n_open, int* status, llark_stream_t stream) {
    LLARK_REQUIRE(logits && (out || ban || n_open), "guide_rows: null pointer (logits; one of out, ban, n_open)");
    LLARK_REQUIRE(child_off && terminal && node_in && node_out, "guide_rows: null pointer (child_off, terminal, node_in, node_out)");
    LLARK_REQUIRE(rows > 0 && slots > 0 && vocab > 0 && ldl >= vocab && (slot_of_row || rows <= slots),
                  "guide_rows: bad shape rows=%d slots=%d vocab=%d ldl=%d", rows, slots, vocab, ldl);
    LLARK_REQUIRE(n_nodes >= 1 && n_nodes <= GUIDE_MAX_NODES && n_edges >= 0 && n_edges <= GUIDE_MAX_EDGES,
                  "guide_rows: table of %d nodes / %d edges outside the caps (1 .. %d nodes, 0 .. %d edges)", n_nodes, n_edges,
                  GUIDE_MAX_NODES, GUIDE_MAX_EDGES);
    LLARK_REQUIRE(n_edges == 0 || (child_tok && child_node), "guide_rows: %d edges without child_tok / child_node", n_edges);
    LLARK_REQUIRE(node_in != (const int*)node_out, "guide_rows: node_in and node_out must be two buffers");
    LLARK_REQUIRE(!parent || parent_stride >= 1, "guide_rows: parent_stride=%d must be >= 1", parent_stride);
    LLARK_REQUIRE(eos >= 0 && eos < vocab, "guide_rows: eos=%lld outside [0, vocab=%d)", (long long)eos, vocab);
    LLARK_REQUIRE(!out || ldo >= vocab, "guide_rows: ldo=%d below vocab=%d", ldo, vocab);
    LLARK_REQUIRE(!out || (const float*)out != logits || ldo == ldl, "guide_rows: in place needs ldo=%d equal to ldl=%d", ldo, ldl);
    LLARK_REQUIRE(!ban || ld_ban >= (vocab + 31) / 32, "guide_rows: ld_ban=%d below ceil(vocab / 32)=%d", ld_ban, (vocab + 31) / 32);
    if (vocab > GUIDE_MAX_VOCAB) {
        set_error("guide_rows: vocab %d above %d", vocab, GUIDE_MAX_VOCAB);
        return LLARK_ERR_UNSUPPORTED;
    }
    GuideArgs a;
    a.logits = logits, a.ldl = ldl, a.vocab = vocab, a.slots = slots, a.state = state, a.slot_of_row = slot_of_row;
    a.child_off = child_off, a.child_tok = child_tok, a.child_node = child_node, a.terminal = terminal, a.n_nodes = n_nodes;
    a.n_edges = n_edges, a.node_in = node_in, a.node_out = node_out, a.parent = parent, a.parent_stride = parent_stride;
    a.last_token = (const long long*)last_token, a.eos = (int)eos, a.out = out, a.ldo = ldo, a.ban = ban, a.ld_ban = ld_ban;
    a.ban_accumulate = ban_accumulate, a.n_open = n_open, a.status = status;
    guide_rows_kernel<<<rows, GUIDE_THREADS, 0, (hipStream_t)stream>>>(a);
    return check_launch("guide_rows");
}
