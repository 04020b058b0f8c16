"""Numpy restatement of ``llark_sample_rows`` (csrc/sample.hip; contract in include/llark_hip.h) for the sampling tests.

fp32 for the steps whose result the kernel must reproduce exactly (repetition penalty, temperature, top-k), float64 from the
softmax on, Philox4x32-10 in Python integers.  Also the shared input family of the kernel tests and the tolerance of the
kernel's fp32 sums."""
import numpy as np

# ---- Philox4x32-10 -------------------------------------------------------------------------------------------------------
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    c0, c1, c2, c3 = (int(c) & MASK for c in ctr)
    k0, k1 = (int(k) & MASK for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def philox_uniform(seed: int, stream_id: int, draw: int) -> float:
    """The kernel's u for (seed, stream id, draw number): (word0 >> 8) * 2^-24, exact in fp32."""
    seed &= (1 << 64) - 1
    stream_id &= (1 << 64) - 1
    w = philox4x32_10((draw, 0, stream_id & MASK, stream_id >> 32), (seed & MASK, seed >> 32))[0]
    return (w >> 8) * 2.0 ** -24


# ---- tolerance -----------------------------------------------------------------------------------------------------------
# The kernel's cumulative mass of a token is a chain of fp32 additions: 6 steps of the scan inside a 64-token chunk, at most 64
# chunk sums per wave, 16 wave sums; every partial sum is <= Z, so each addition errs by at most 2^-24 Z: 6 + 64 + 16 = 86.  The
# bisection's sums have the same depth (64 per thread, 6 butterfly steps, 16 waves).  The exponentials: expf is accurate to 1 ulp and
# its argument l - m is rounded to fp32, an error of 2^-24 |l - m| / 2 in the exponent; summed with the weights e_i that is
# 2^-25 * sum e_i (m - l_i) = 2^-25 Z (H - ln(Z)) <= 2^-25 Z ln(V) with H the entropy: at most 0.5 * ln(65536) < 6 units, plus 2 for
# expf itself and the rounding of u * Z / p * Z.  86 + 6 + 2 = 94, rounded up to 96.
C_TOL = 96.0


def tol_of(z: float) -> float:
    return C_TOL * 2.0 ** -24 * z


# ---- the processors ------------------------------------------------------------------------------------------------------
def penalise(row: np.ndarray, seen: np.ndarray, theta: float) -> np.ndarray:
    row = np.asarray(row, dtype=np.float32)
    if theta == 1.0:
        return row.copy()
    th = np.float32(theta)
    with np.errstate(all="ignore"):
        pen = np.where(row < 0, row * th, row / th).astype(np.float32)
    return np.where(seen, pen, row).astype(np.float32)


def greedy_token(row: np.ndarray) -> int:
    """torch.argmax: first maximal index, a NaN counts as the maximum."""
    nan = np.isnan(row)
    return int(np.argmax(nan)) if nan.any() else int(np.argmax(row))


def mass_above(l: np.ndarray, e: np.ndarray, members: np.ndarray) -> np.ndarray:
    """For every token, the float64 sum of e_j over members j with l_j > l_i."""
    idx = np.flatnonzero(members)
    order = idx[np.argsort(-l[idx].astype(np.float64), kind="stable")]
    ls, es = l[order], e[order]
    csum = np.concatenate(([0.0], np.cumsum(es)))
    first = np.searchsorted(-ls.astype(np.float64), -l.astype(np.float64), side="left")      # members strictly above l_i
    return csum[first]


def process(row, seen, temperature=1.0, top_k=0, top_p=1.0, theta=1.0):
    """Steps 1-4 for one row.  Returns a dict: l (post-temperature fp32), in_k (top-k members), e (float64 exp(l - max), 0 outside
    in_k), Z, above (mass strictly above each token), keep (final kept set), thresh, kept; or {"fallback": greedy token}."""
    pen = penalise(row, seen, theta)
    V = pen.size
    with np.errstate(all="ignore"):
        l = (pen / np.float32(temperature)).astype(np.float32) + np.float32(0.0)
    m = l.max() if not np.isnan(l).any() else np.float32("nan")
    if np.isnan(m) or np.isinf(m):
        return {"fallback": greedy_token(pen)}
    in_k = np.ones(V, dtype=bool)
    if top_k > 0:
        k = min(max(int(top_k), 1), V)
        kth = np.partition(l, V - k)[V - k]
        in_k = l >= kth
    e = np.where(in_k, np.exp(l.astype(np.float64) - np.float64(m)), 0.0)
    Z = float(e.sum())
    above = mass_above(l, e, in_k)
    keep = in_k.copy()
    if top_p < 1.0:
        keep &= above < float(np.float32(top_p)) * Z
    return {"l": l, "in_k": in_k, "e": e, "Z": Z, "above": above, "keep": keep, "thresh": np.float32(l[keep].min()), "kept": int(keep.sum()),
            "greedy": greedy_token(pen)}


def draw(l, e, keep, u: float):
    """Step 5 over a given kept set: (token, acceptable tokens under the tolerance, Z_kept, tol)."""
    ek = np.where(keep, e, 0.0)
    cum = np.cumsum(ek)
    zk = float(cum[-1])
    target = float(np.float32(u)) * zk
    tol = tol_of(zk)
    tok = int(np.searchsorted(cum, target, side="right"))
    tok = min(tok, int(np.flatnonzero(keep)[-1]))
    lo = np.concatenate(([0.0], cum[:-1]))
    ok = np.flatnonzero((ek > 0) & (lo - tol <= target) & (target < cum + tol))
    return tok, ok, zk, tol


# ---- the input family of the kernel tests --------------------------------------------------------------------------------
PARAM_SETS = {
    "T0.8": dict(temperature=0.8),
    "k50": dict(top_k=50),
    "p0.9": dict(top_p=0.9),
    "T0.7_k200_p0.95_th1.3": dict(temperature=0.7, top_k=200, top_p=0.95, theta=1.3),
}
VOCABS = (1, 63, 1025, 32003, 50435)


def make_case(vocab: int, rows: int, seed: int = 0):
    """3 * randn logits with five tokens raised by 6 .. 10; 300 random tokens plus two of the raised ones marked seen; u in [0, 1)."""
    rng = np.random.default_rng(1000 * seed + vocab)
    logits = (3.0 * rng.standard_normal((rows, vocab))).astype(np.float32)
    seen = np.zeros((rows, vocab), dtype=bool)
    n_up = min(5, vocab)
    for r in range(rows):
        up = rng.choice(vocab, size=n_up, replace=False)
        logits[r, up] += rng.uniform(6.0, 10.0, size=n_up).astype(np.float32)
        seen[r, rng.choice(vocab, size=min(300, vocab), replace=False)] = True
        seen[r, up[:2]] = True
    u = (rng.integers(0, 1 << 24, size=rows).astype(np.float64) * 2.0 ** -24).astype(np.float32)
    return logits, seen, u


def pack_seen(seen: np.ndarray) -> np.ndarray:
    """bool [rows][vocab] -> the kernel's bitmap, int32 [rows][ceil(vocab / 32)] (bit t & 31 of word t >> 5)."""
    rows, vocab = seen.shape
    words = (vocab + 31) // 32
    padded = np.zeros((rows, words * 32), dtype=np.uint64)
    padded[:, :vocab] = seen
    w = (padded.reshape(rows, words, 32) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
    return w.view(np.int32)


def ambiguous_rows(logits, seen, u, **params) -> int:
    """Rows of a case in which the reference itself admits more than one token under the tolerance."""
    n = 0
    for r in range(logits.shape[0]):
        ref = process(logits[r], seen[r], **params)
        if "fallback" in ref:
            continue
        n += draw(ref["l"], ref["e"], ref["keep"], float(u[r]))[1].size > 1
    return n

