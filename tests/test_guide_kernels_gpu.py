"""GPU: llark_guide_rows (csrc/guide.hip) against tests/guide_ref.py.

Everything the kernel writes is integers or copied bits, so every comparison is exact: the bits of the processed rows, the bitmap's
words, the new nodes, the counts of open columns and the status word.  Rows that the launch skips, and every buffer word outside what
it may write, keep a sentinel."""
import functools

import numpy as np
import pytest
import torch

import guide_ref as GR
from llark_amd import _lib, ops

pytestmark = pytest.mark.gpu

I32, I64, F32 = torch.int32, torch.int64, torch.float32
SENT = -777.25
NODE_SENT = -99


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _rows(vocab, rows):
    from logprob_ref import make_rows
    x = make_rows(vocab, rows, 5)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _sets(vocab, eos):
    """The choice sets of every kernel test: fan-outs 1, 2, 1 024 and 1 025 (where the vocabulary has room), children at column 0 and
    vocab - 1, a sequence that is a prefix of another, eos as a non-final member, eos the last column."""
    wide = [t for t in range(vocab) if t != eos]
    s = [
        [[0], [vocab - 1], [5, 6, 7]],                                          # children at both edges; fan-out 3, then 1
        [[3, 1], [3, 2]],                                                       # fan-out 1 at the root, 2 below
        [[4], [4, 8], [4, 8, 9]],                                               # a whole sequence that is a prefix of two more
        [[2, eos, 10], [11]],                                                   # eos inside a sequence
    ]
    if vocab > 2000:
        s.append([[t] for t in wide[:1024]])                                    # fan-out 1 024: one child per thread
        s.append([[12, t] for t in wide[-1025:]])                               # fan-out 1 025 below the root: the stride's second turn
    return s


def _dev(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype).cuda()


def _table_dev(table):
    return tuple(_dev(t, I32) for t in table[:4])


def _walk(table, root, seq, eos):
    n = root
    for t in seq:
        n, b = GR.step(table, n, t, eos)
        assert b == 0
    return n


def _case(vocab, slots, seed):
    """Per slot a node (roots, inner nodes, terminals, FREE, CLOSED, cycled) and a last token (a child, a token outside the set, eos)."""
    eos = vocab - 1 if seed % 2 else 13
    sets = _sets(vocab, eos)
    table = GR.build_table(sets)
    rng = np.random.default_rng(seed)
    nodes, last = [], []
    for s in range(slots):
        kind = s % 8
        k = (s // 8) % len(sets)
        root = table[4][k]
        q = sorted(sets[k])[s % len(sets[k])] if len(sets[k]) < 100 else sets[k][int(rng.integers(0, len(sets[k])))]
        if kind == 0:
            n, t = root, q[0]                                                    # a step from the root
        elif kind == 1:
            n, t = _walk(table, root, q[:-1], eos), q[-1]                        # the step onto a terminal
        elif kind == 2:
            n, t = _walk(table, root, q, eos), eos                               # eos at a terminal: CLOSED, no bit
        elif kind == 3:
            n, t = root, 14                                                      # a token outside the set: CLOSED and OFF_SET
        elif kind == 4:
            n, t = GR.FREE, int(rng.integers(0, vocab))
        elif kind == 5:
            n, t = GR.CLOSED, eos
        elif kind == 6:
            n, t = root, eos                                                     # eos where no sequence ends: OFF_SET
        else:
            n, t = _walk(table, root, q[:1], eos), (q[1] if len(q) > 1 else eos)
        nodes.append(int(n)), last.append(int(t))
    return eos, table, nodes, last


@pytest.mark.parametrize("rows", [1, 3, 64])
@pytest.mark.parametrize("vocab", [33, 32003, 50435])
def test_guide_rows_against_the_reference(vocab, rows):
    """Rows in a permuted slot order with inactive and out-of-range slots among them; all three outputs at once, decode step (last)."""
    slots = rows + 2
    eos, table, nodes, last = _case(vocab, slots, vocab + rows)
    rng = np.random.default_rng(rows)
    perm = rng.permutation(slots)[:rows].astype(np.int32)
    state = np.ones(slots, dtype=np.int32)
    if rows > 1:
        state[perm[1]] = 2                                                       # finished: skipped
        perm[rows - 1] = slots + 3                                               # no slot: skipped
    logits = np.array(_rows(vocab, rows), copy=True)
    ldl = logits.shape[1]
    logits[0, 0], logits[0, vocab - 1] = np.nan, -np.inf                         # kept where allowed
    words = (vocab + 31) // 32
    ban0 = rng.integers(0, 2 ** 32, size=(slots, words + 1), dtype=np.uint64).astype(np.uint32)
    ref = GR.guide_rows(logits, table, nodes, eos, vocab=vocab, state=state, slot_of_row=perm, last=last,
                        out=np.full((rows, vocab + 3), SENT, np.float32), ban=ban0, ban_accumulate=True, want_open=True)
    dev = torch.from_numpy(logits).cuda()
    out = torch.full((rows, vocab + 3), SENT, dtype=F32, device="cuda")
    ban = torch.from_numpy(ban0.view(np.int32)).cuda()
    node_in, node_out = _dev(nodes, I32), torch.full((slots,), NODE_SENT, dtype=I32, device="cuda")
    n_open = torch.full((rows,), -5, dtype=I32, device="cuda")
    status = torch.zeros((1,), dtype=I32, device="cuda")
    ops.guide_rows(dev, *_table_dev(table), node_in, node_out, eos=eos, vocab=vocab, state=_dev(state, I32), slot_of_row=_dev(perm, I32),
                   last_token=_dev(last, I64), out=out, ban=ban, ban_accumulate=True, n_open=n_open, status=status)
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(ref["out"]))
    assert np.array_equal(ban.cpu().numpy().view(np.uint32), ref["ban"])
    assert node_out.cpu().tolist() == [NODE_SENT if n is None else n for n in ref["node_out"]]
    assert n_open.cpu().tolist() == [-5 if n is None else n for n in ref["n_open"]]
    assert int(status.item()) == ref["status"]
    assert node_in.cpu().tolist() == nodes and np.array_equal(bits(dev.cpu().numpy()), bits(logits))      # read only
    assert ldl >= vocab


def test_every_case_of_the_state_machine_occurs():
    """The generator above does produce what the list of cases names (on the widest shape)."""
    eos, table, nodes, last = _case(50435, 66, 50435 + 64)
    ref = GR.guide_rows(np.zeros((66, 50435), np.float32), table, nodes, eos, last=last, want_open=True)
    new = ref["node_out"]
    assert ref["status"] == GR.OFF_SET
    assert GR.CLOSED in new and GR.FREE in new and any(n >= 0 and table[3][n] for n in new) and any(n >= 0 and not table[3][n] for n in new)
    fan = [int(table[0][n + 1] - table[0][n]) for n in range(len(table[3]))]
    assert {1, 2, 1024, 1025} <= set(fan)


@pytest.mark.parametrize("vocab", [33, 32003])
def test_prefill_rows_in_place_and_single_outputs(vocab):
    """No last token (prefill rows: the node stays), no state, no slot table; out == logits in place; each output alone."""
    eos, table, _, _ = _case(vocab, 3, 7)
    nodes = [table[4][0], GR.FREE, table[4][2]]
    if vocab > 2000:                                                                                # the allowed set itself 1 024 and 1 025 wide
        nodes += [table[4][4], _walk(table, table[4][5], [12], eos)]
        assert [int(table[0][n + 1] - table[0][n]) for n in nodes[3:]] == [1024, 1025]
    rows = len(nodes)
    logits = np.array(_rows(vocab, rows), copy=True)
    ref = GR.guide_rows(logits, table, nodes, eos, vocab=vocab, out=logits, ban=np.zeros((rows, (vocab + 31) // 32), np.uint32), want_open=True)
    tab = _table_dev(table)
    node_in = _dev(nodes, I32)

    def fresh():
        return torch.full((rows,), NODE_SENT, dtype=I32, device="cuda")
    dev = torch.from_numpy(logits).cuda()
    node_out = fresh()
    ops.guide_rows(dev, *tab, node_in, node_out, eos=eos, vocab=vocab, out=dev)                     # in place
    assert np.array_equal(bits(dev.cpu().numpy()), bits(ref["out"])) and node_out.cpu().tolist() == nodes
    assert np.array_equal(bits(dev.cpu().numpy()[1]), bits(logits[1]))                              # the unconstrained row: bit-equal
    dev = torch.from_numpy(logits).cuda()
    ban = torch.full((rows, (vocab + 31) // 32), -1, dtype=I32, device="cuda")
    ops.guide_rows(dev, *tab, node_in, fresh(), eos=eos, vocab=vocab, ban=ban)                      # stored, not OR-ed
    assert np.array_equal(ban.cpu().numpy().view(np.uint32), ref["ban"])
    n_open = torch.zeros((rows,), dtype=I32, device="cuda")
    status = torch.zeros((1,), dtype=I32, device="cuda")
    ops.guide_rows(dev, *tab, node_in, fresh(), eos=eos, vocab=vocab, n_open=n_open, status=status)
    assert n_open.cpu().tolist() == ref["n_open"] and int(status.item()) == 0
    assert np.array_equal(bits(dev.cpu().numpy()), bits(logits))


def test_all_banned_row_sets_the_empty_bit_and_nan_inf_stay():
    vocab, eos = 32003, 32002                                                                       # eos in the last column
    table = GR.build_table(_sets(vocab, eos))
    root = table[4][0]                                                                              # allows 0, 5, vocab - 1
    logits = np.array(_rows(vocab, 3), copy=True)
    logits[0, [0, 5, vocab - 1]] = -np.inf                                                          # others banned them all
    logits[1, 0], logits[1, 5] = np.nan, -np.inf                                                    # one open column left: vocab - 1
    nodes = [root, root, GR.CLOSED]
    ref = GR.guide_rows(logits, table, nodes, eos, out=np.zeros_like(logits), want_open=True)
    assert ref["n_open"] == [0, 1, 1] and ref["status"] == GR.EMPTY
    dev = torch.from_numpy(logits).cuda()
    out = torch.zeros_like(dev)
    n_open = torch.full((3,), -1, dtype=I32, device="cuda")
    status = torch.zeros((1,), dtype=I32, device="cuda")
    ops.guide_rows(dev, *_table_dev(table), _dev(nodes, I32), torch.zeros((3,), dtype=I32, device="cuda"), eos=eos, out=out, n_open=n_open,
                   status=status)
    assert np.array_equal(bits(out.cpu().numpy()), bits(ref["out"]))
    assert n_open.cpu().tolist() == [0, 1, 1] and int(status.item()) == GR.EMPTY
    got = out.cpu().numpy()
    assert np.isnan(got[1, 0]) and np.isneginf(got[1, 5]) and got[1, vocab - 1] == logits[1, vocab - 1]
    assert np.flatnonzero(~np.isneginf(got[2])).tolist() == [eos]


def test_parent_route_survives_a_parent_that_is_replaced_in_the_same_launch():
    """Beams: slot 0 and slot 2 continue slot 1's beam while slot 1 takes slot 3's and slot 3 steps on -- every workgroup reads node_in,
    none reads what the launch writes.  The parents lie in column 0 of a trellis row (stride 3); a -1 entry means the slot's own."""
    vocab, eos = 32003, 13
    sets = [[[1, 2, 3], [1, 2, 4], [1, 5], [6, 7]]]
    table = GR.build_table(sets)
    n1, n12, n6 = _walk(table, 0, [1], eos), _walk(table, 0, [1, 2], eos), _walk(table, 0, [6], eos)
    nodes = [0, n12, n1, n6, n1]
    parent = [1, 3, 1, 3, -1]
    last = [3, 7, 4, 7, 5]
    ref = GR.guide_rows(np.zeros((5, vocab), np.float32), table, nodes, eos, parent=parent, last=last, ban=np.zeros((5, 1001), np.uint32))
    assert ref["node_out"] == [_walk(table, 0, [1, 2, 3], eos), _walk(table, 0, [6, 7], eos), _walk(table, 0, [1, 2, 4], eos),
                               _walk(table, 0, [6, 7], eos), _walk(table, 0, [1, 5], eos)] and ref["status"] == 0
    trellis = torch.full((5, 3), 77, dtype=I32, device="cuda")
    trellis[:, 0] = _dev(parent, I32)
    ban = torch.zeros((5, 1001), dtype=I32, device="cuda")
    node_out = torch.full((5,), NODE_SENT, dtype=I32, device="cuda")
    status = torch.zeros((1,), dtype=I32, device="cuda")
    for _ in range(3):                                                                              # the same launch, the same answer
        ops.guide_rows(torch.zeros((5, vocab), dtype=F32, device="cuda"), *_table_dev(table), _dev(nodes, I32), node_out, eos=eos,
                       parent=trellis[:, 0], last_token=_dev(last, I64), ban=ban, status=status)
        assert node_out.cpu().tolist() == ref["node_out"]
    assert np.array_equal(ban.cpu().numpy().view(np.uint32), ref["ban"]) and int(status.item()) == 0


def test_refusals():
    x = torch.zeros((1, 65537), dtype=F32, device="cuda")
    one = torch.zeros((2,), dtype=I32, device="cuda")
    a, b = torch.zeros((1,), dtype=I32, device="cuda"), torch.zeros((1,), dtype=I32, device="cuda")
    with pytest.raises(_lib.LlarkHipError, match="above 65536"):
        ops.guide_rows(x, one, one[:0], one[:0], one[:1], a, b, eos=0, out=torch.zeros_like(x))
    x = x[:, :64].contiguous()
    out = torch.zeros_like(x)
    L = _lib.lib()

    def call(**kw):
        args = dict(logits=x.data_ptr(), ldl=64, vocab=64, rows=1, slots=1, state=None, slot_of_row=None, child_off=one.data_ptr(),
                    child_tok=None, child_node=None, terminal=one.data_ptr(), n_nodes=1, n_edges=0, node_in=a.data_ptr(),
                    node_out=b.data_ptr(), parent=None, parent_stride=1, last_token=None, eos=3, out=out.data_ptr(), ldo=64, ban=None,
                    ld_ban=0, ban_accumulate=0, n_open=None, status=None)
        args.update(kw)
        return L.llark_guide_rows(*args.values(), None)
    assert call() == 0
    for bad, word in ((dict(logits=None), "null"), (dict(out=None), "null"), (dict(child_off=None), "null"), (dict(terminal=None), "null"),
                      (dict(node_in=None), "null"), (dict(node_out=None), "null"), (dict(ldl=63), "ldl"), (dict(rows=2), "rows"),
                      (dict(parent=a.data_ptr(), parent_stride=0), "parent_stride"), (dict(eos=-1), "eos"), (dict(eos=64), "eos"),
                      (dict(ldo=63), "ldo"), (dict(ban=out.data_ptr(), ld_ban=1), "ld_ban"), (dict(node_out=a.data_ptr()), "two buffers"),
                      (dict(n_nodes=0), "caps"), (dict(n_nodes=(1 << 20) + 1), "caps"), (dict(n_edges=(1 << 20) + 1), "caps"),
                      (dict(n_edges=1), "child_tok"), (dict(out=x.data_ptr(), ldo=65), "in place")):
        assert call(**bad) == -1, bad
        assert word in L.llark_last_error().decode(), (bad, L.llark_last_error().decode())
    torch.cuda.synchronize()
