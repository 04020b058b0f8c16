"""Plain Python / numpy restatement of guided choice (csrc/guide.hip; contract in include/llark_hip.h: llark_guide_rows), for the guide
tests: HF 4.29.2's PrefixConstrainedLogitsProcessor with the set given as data -- a prefix tree in CSR form and one node per slot.

Node values: >= 0 a node of the table, FREE (-1) an unconstrained slot, CLOSED (-2) only eos is allowed.  Status bits: OFF_SET (2) a slot
was handed a token outside its set, EMPTY (4) a row had no allowed column with a logit that is neither -inf nor NaN."""
import numpy as np

FREE, CLOSED = -1, -2
OFF_SET, EMPTY = 2, 4


def build_table(sets):
    """All choice sets of a call as ONE prefix tree: (child_off [nodes + 1], child_tok [edges], child_node [edges], terminal [nodes],
    roots [sets]); a node's children ascend by token; duplicate sequences collapse.  Nodes are numbered in order of first visit, the
    sets in order, each set's sequences sorted."""
    kids, term, roots = [], [], []
    for s in sets:
        roots.append(len(kids))
        kids.append({}), term.append(0)
        for q in sorted({tuple(int(t) for t in q) for q in s}):
            n = roots[-1]
            for t in q:
                if t not in kids[n]:
                    kids[n][t] = len(kids)
                    kids.append({}), term.append(0)
                n = kids[n][t]
            term[n] = 1
    off, tok, node = [0], [], []
    for k in kids:
        for t in sorted(k):
            tok.append(t), node.append(k[t])
        off.append(len(tok))
    i32 = np.int32
    return np.array(off, i32), np.array(tok, i32), np.array(node, i32), np.array(term, i32), roots


def step(table, n, token, eos):
    """(n', status bits) of a slot at node ``n`` that is handed ``token``."""
    off, tok, node, term, _ = table
    if n < CLOSED or n >= len(term):
        n = CLOSED
    if n < 0:
        return n, 0
    for e in range(off[n], off[n + 1]):
        if int(tok[e]) == int(token):
            return int(node[e]), 0
    return CLOSED, 0 if (int(token) == eos and term[n]) else OFF_SET


def allowed(table, n, eos, vocab):
    """bool [vocab]: the columns a slot at node ``n`` may choose."""
    off, tok, _, term, _ = table
    ok = np.zeros(vocab, dtype=bool)
    if n == FREE:
        ok[:] = True
        return ok
    if n >= 0:
        for e in range(off[n], off[n + 1]):
            if 0 <= tok[e] < vocab:
                ok[tok[e]] = True
    if n == CLOSED or (n >= 0 and term[n]):
        ok[eos] = True
    return ok


def is_open(row):
    """bool per column: the logit is neither -inf nor NaN."""
    row = np.asarray(row, dtype=np.float32)
    return ~(np.isnan(row) | np.isneginf(row))


def bitmap_of(ok):
    """The ban bitmap (bit set: NOT allowed) of one row as uint32 words; bits of columns >= vocab stay clear."""
    vocab = len(ok)
    bits = np.zeros(((vocab + 31) // 32) * 32, dtype=np.uint8)
    bits[:vocab] = ~ok
    return np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view(np.uint32).reshape(-1).copy()


def guide_rows(logits, table, node_in, eos, vocab=None, state=None, slot_of_row=None, parent=None, last=None, out=None, ban=None,
               ban_accumulate=False, want_open=False, status=0):
    """One launch.  ``logits`` fp32 [rows, >= vocab]; ``node_in`` int [slots]; ``state`` (1: active) / ``slot_of_row`` / ``parent`` /
    ``last`` as the kernel takes them; ``out`` (fp32 [rows, >= vocab]) and ``ban`` (uint32 [slots, words]) are the buffers' contents
    BEFORE the launch (None: that output is not asked for).  Returns dict(out, ban, node_out, n_open, status): node_out holds None
    where the launch writes nothing, n_open likewise."""
    logits = np.asarray(logits, dtype=np.float32)
    rows = logits.shape[0]
    vocab = logits.shape[1] if vocab is None else vocab
    slots = len(node_in)
    res_out = None if out is None else np.array(out, dtype=np.float32, copy=True)
    res_ban = None if ban is None else np.array(ban, dtype=np.uint32, copy=True)
    node_out, n_open = [None] * slots, [None] * rows
    for r in range(rows):
        slot = r if slot_of_row is None else int(slot_of_row[r])
        if slot < 0 or slot >= slots or (state is not None and int(state[slot]) != 1):
            continue
        p = slot if parent is None else int(parent[slot])
        if p < 0 or p >= slots:
            p = slot
        n = int(node_in[p])
        if n < CLOSED or n >= len(table[3]):
            n = CLOSED
        if last is not None:
            n, bits = step(table, n, int(last[slot]), eos)
            status |= bits
        node_out[slot] = n
        ok = allowed(table, n, eos, vocab)
        if res_out is not None:
            res_out[r, :vocab] = np.where(ok, logits[r, :vocab], np.float32(-np.inf))
        if res_ban is not None:
            w = bitmap_of(ok)
            res_ban[slot, :len(w)] = (res_ban[slot, :len(w)] | w) if ban_accumulate else w
        if want_open:
            n_open[r] = int((ok & is_open(logits[r, :vocab])).sum())
            if n_open[r] == 0:
                status |= EMPTY
    return dict(out=res_out, ban=res_ban, node_out=node_out, n_open=n_open, status=status)


class RowGuide:
    """One row of a host generation loop: ``mask(row)`` is the row with -inf outside the allowed set, ``push(token)`` the step."""

    def __init__(self, choice_set, eos):
        self.table = None if choice_set is None else build_table([choice_set])
        self.node = FREE if choice_set is None else 0
        self.eos, self.status = eos, 0

    def allowed(self, vocab):
        return np.ones(vocab, dtype=bool) if self.table is None else allowed(self.table, self.node, self.eos, vocab)

    def mask(self, row):
        row = np.asarray(row, dtype=np.float32)
        return np.where(self.allowed(len(row)), row, np.float32(-np.inf))

    def push(self, token):
        if self.table is not None:
            self.node, bits = step(self.table, self.node, token, self.eos)
            self.status |= bits


def prefix_allowed_tokens_fn(sets_of_row, prompt_len, eos):
    """HF's callback derived from the same sets, straight from the rule: after the generated tokens g, x is allowed iff some sequence
    starts with g + [x]; eos iff g is a whole sequence."""
    def fn(batch_id, sent):
        g = [int(t) for t in sent[prompt_len:]]
        s = sets_of_row[batch_id]
        out = {q[len(g)] for q in s if len(q) > len(g) and list(q[:len(g)]) == g}
        if any(list(q) == g for q in s):
            out.add(eos)
        return sorted(out)
    return fn
