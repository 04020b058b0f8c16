"""tests/guide_ref.py against the installed transformers' PrefixConstrainedLogitsProcessor (seeded cases, exact agreement, none skipped),
against hand-written expected sets, and llark_amd.m2t.guide.ChoiceSets.table against the restatement's table."""
import numpy as np
import pytest
import torch

import guide_ref as GR

N_CASES = 2400


def _random_sets(rng, vocab, eos, kind):
    """One choice set of the given kind; every kind is a shape the kernel's rules treat differently."""
    def seq(n):
        return [int(t) for t in rng.integers(0, vocab, size=n)]
    if kind == "random":
        s = [seq(int(rng.integers(1, 5))) for _ in range(int(rng.integers(1, 7)))]
    elif kind == "prefix":                                        # one sequence is a proper prefix of another
        a = seq(int(rng.integers(1, 4)))
        s = [a, a + seq(int(rng.integers(1, 3)))] + [seq(int(rng.integers(1, 4))) for _ in range(int(rng.integers(0, 3)))]
    elif kind == "single":                                        # single-token sequences only
        s = [[int(t)] for t in rng.integers(0, vocab, size=int(rng.integers(1, 6)))]
    elif kind == "shared":                                        # a shared first token
        t = int(rng.integers(0, vocab))
        s = [[t] + seq(int(rng.integers(1, 4))) for _ in range(int(rng.integers(2, 5)))]
    elif kind == "edges":                                         # token 0 and vocab - 1
        s = [[0], [vocab - 1], [0, vocab - 1], [vocab - 1, 0, int(rng.integers(0, vocab))]]
    elif kind == "eos_inside":                                    # eos as a non-final member
        s = [[int(rng.integers(0, vocab)), eos, int(rng.integers(0, vocab))], seq(2), [eos, int(rng.integers(0, vocab))]]
    else:
        raise AssertionError(kind)
    if rng.integers(0, 4) == 0:
        s.append(list(s[0]))                                      # a duplicate collapses
    return s


KINDS = ("random", "prefix", "single", "shared", "edges", "eos_inside")


def test_agrees_with_transformers_prefix_constrained_processor():
    from transformers import PrefixConstrainedLogitsProcessor

    rng = np.random.default_rng(0)
    done = 0
    for case in range(N_CASES):
        vocab = int(rng.choice([5, 33, 64, 97]))
        eos = int(rng.integers(0, vocab))
        rows = int(rng.integers(1, 4))
        prompt_len = int(rng.integers(0, 4))
        sets = [_random_sets(rng, vocab, eos, KINDS[(case + r) % len(KINDS)]) for r in range(rows)]
        table = GR.build_table(sets)
        # every row sits after a random valid prefix g of one of its sequences (the whole sequence included), reached by stepping
        gens, nodes, status = [], [], 0
        for r in range(rows):
            q = sets[r][int(rng.integers(0, len(sets[r])))]
            g = list(q[:int(rng.integers(0, len(q) + 1))])
            n = table[4][r]
            for t in g:
                n, bits = GR.step(table, n, t, eos)
                status |= bits
            assert n >= 0 and status == 0
            gens.append(g), nodes.append(n)
        width = max(len(g) for g in gens)
        if any(len(g) != width for g in gens):                    # HF sees one tensor: rows of one case share the generated length
            keep = [r for r in range(rows) if len(gens[r]) == width]
            sets, gens, nodes = [sets[r] for r in keep], [gens[r] for r in keep], [nodes[r] for r in keep]
            table_rows = keep
        else:
            table_rows = list(range(rows))
        rows = len(gens)
        logits = rng.standard_normal((rows, vocab)).astype(np.float32)
        got = GR.guide_rows(logits, table, nodes, eos, out=np.zeros_like(logits), want_open=True)
        prompt = rng.integers(0, vocab, size=(rows, prompt_len))
        ids = torch.from_numpy(np.concatenate([prompt, np.array(gens, dtype=np.int64).reshape(rows, width)], axis=1))
        proc = PrefixConstrainedLogitsProcessor(GR.prefix_allowed_tokens_fn(sets, prompt_len, eos), num_beams=1)
        want = proc(ids, torch.from_numpy(logits.copy())).numpy()
        assert np.array_equal(got["out"], want), (case, sets, gens)
        assert got["n_open"] == [int(np.isfinite(w).sum()) for w in want] and got["status"] == 0
        assert got["node_out"] == nodes and len(table_rows) == rows
        done += 1
    assert done == N_CASES >= 2000


def test_table_layout_and_the_packaged_builder():
    from llark_amd.m2t.guide import ChoiceSets

    sets = [[[5, 6], [5], [7, 1, 2], [5, 6]], [[3]]]
    off, tok, node, term, roots = GR.build_table(sets)
    assert roots == [0, 6] and node.tolist() == [1, 3, 2, 4, 5, 7]
    assert off.tolist() == [0, 2, 3, 3, 4, 5, 5, 6, 6] and tok.tolist() == [5, 7, 6, 1, 2, 3]
    for s, root in zip(sets, roots):
        for q in s:
            n = root
            for t in q:
                n, bits = GR.step((off, tok, node, term, roots), n, t, 9)
                assert bits == 0 and n >= 0
            assert term[n] == 1
    assert int(term.sum()) == 4                                   # [5], [5, 6], [7, 1, 2], [3]: the duplicate collapsed
    mine = ChoiceSets(sets).table(10)
    for a, b in zip(mine[:4], (off, tok, node, term)):
        assert a.dtype == torch.int32 and a.tolist() == b.tolist()
    assert mine[4] == roots


def test_step_allowed_and_status_bits_by_hand():
    eos, vocab = 4, 8
    table = GR.build_table([[[1, 2], [1], [3, eos, 5]]])
    root = table[4][0]
    assert np.flatnonzero(GR.allowed(table, root, eos, vocab)).tolist() == [1, 3]
    n1, b = GR.step(table, root, 1, eos)
    assert b == 0 and np.flatnonzero(GR.allowed(table, n1, eos, vocab)).tolist() == [2, eos]      # [1] is whole and a prefix of [1, 2]
    n2, b = GR.step(table, n1, 2, eos)
    assert b == 0 and np.flatnonzero(GR.allowed(table, n2, eos, vocab)).tolist() == [eos]
    assert GR.step(table, n2, eos, eos) == (GR.CLOSED, 0)                                         # eos at a terminal: closed, no bit
    assert GR.step(table, n1, 7, eos) == (GR.CLOSED, GR.OFF_SET)                                  # a token outside the set
    assert GR.step(table, root, eos, eos) == (GR.CLOSED, GR.OFF_SET)                              # eos where no sequence ends
    n3, b = GR.step(table, root, 3, eos)
    n4, b4 = GR.step(table, n3, eos, eos)                                                         # eos as a non-final member: a child
    assert (b, b4) == (0, 0) and np.flatnonzero(GR.allowed(table, n4, eos, vocab)).tolist() == [5]
    assert GR.step(table, GR.CLOSED, 1, eos) == (GR.CLOSED, 0) and GR.step(table, GR.FREE, 1, eos) == (GR.FREE, 0)
    assert np.flatnonzero(GR.allowed(table, GR.CLOSED, eos, vocab)).tolist() == [eos] and GR.allowed(table, GR.FREE, eos, vocab).all()


def test_outputs_preserve_bits_count_open_columns_and_flag_empty_rows():
    eos, vocab = 2, 40
    table = GR.build_table([[[0], [39], [33, 1]]])
    logits = np.zeros((3, vocab), dtype=np.float32)
    logits[0, 0], logits[0, 39], logits[0, 33] = np.nan, -np.inf, 1.5
    logits[1, [0, 39, 33]] = -np.inf                              # every allowed column banned by somebody else
    ban0 = np.full((3, 2), 0x80000001, dtype=np.uint32)
    got = GR.guide_rows(logits, table, [0, 0, GR.FREE], eos, out=np.ones_like(logits), ban=ban0, ban_accumulate=True, want_open=True)
    assert np.isnan(got["out"][0, 0]) and np.isneginf(got["out"][0, 39]) and got["out"][0, 33] == 1.5
    assert np.isneginf(np.delete(got["out"][0], [0, 33, 39])).all()
    assert got["n_open"] == [1, 0, vocab] and got["status"] == GR.EMPTY
    assert np.array_equal(got["out"][2], logits[2])               # an unconstrained row passes through
    w = GR.bitmap_of(GR.allowed(table, 0, eos, vocab))
    assert w.tolist() == [0xfffffffe, 0x7d] and got["ban"][0].tolist() == [0xffffffff, 0x8000007d]
    assert got["ban"][2].tolist() == [0x80000001, 0x80000001]
    stored = GR.guide_rows(logits, table, [0, 0, GR.FREE], eos, ban=ban0)
    assert stored["ban"][0].tolist() == w.tolist() and stored["ban"][2].tolist() == [0, 0]


def test_parent_route_reads_the_old_nodes_only():
    """Slot 0 continues slot 1's beam while slot 1 itself steps on: both read node_in, nobody reads what this launch writes."""
    eos = 9
    table = GR.build_table([[[1, 2, 3], [1, 4]]])
    n1, _ = GR.step(table, 0, 1, eos)
    got = GR.guide_rows(np.zeros((2, 10), np.float32), table, [0, n1], eos, parent=[1, 1], last=[4, 2], out=np.zeros((2, 10), np.float32))
    assert got["node_out"] == [GR.step(table, n1, 4, eos)[0], GR.step(table, n1, 2, eos)[0]] and got["status"] == 0


@pytest.mark.parametrize("bad", [-3, 10 ** 6])
def test_a_node_no_table_holds_counts_as_closed(bad):
    table = GR.build_table([[[1]]])
    got = GR.guide_rows(np.zeros((1, 4), np.float32), table, [bad], 3, out=np.zeros((1, 4), np.float32))
    assert got["node_out"] == [GR.CLOSED] and np.flatnonzero(~np.isneginf(got["out"][0])).tolist() == [3]
