"""GPU: llark_beam_advance_open (csrc/beam.hip), the beam step of a search inside a closed set, step by step against the reference
step of tests/beam_ref.py with the two rules that differ: a candidate whose score is -inf is never taken, and an example goes on
while ANY beam lives.  The candidates come from the device (``ops.beam_topk_rows`` under the guide's bitmap), as in
tests/test_beam_kernels_gpu.py, so that the comparison is of the advance step alone and exact."""
import numpy as np
import pytest
import torch

import beam_ref as R
import test_beam_kernels_gpu as BK
from llark_amd import ops
from llark_amd.m2t.beam import BeamSearch
from llark_amd.m2t.guide import ChoiceSets, DeviceGuide

pytestmark = pytest.mark.gpu

I32, I64 = torch.int32, torch.int64
EOS = 7
# the root has two children, one of them a leaf; [20, 21] then fans out six ways.  Beams start at (0, -1e9, ...): the first step fills
# every slot with 10s and 20s, the second leaves the slots of the 10s over (a leaf only offers the eos), the third forks [20, 21] into them
SET = [[10]] + [[20, 21, t] for t in range(22, 28)] + [[20, 21, 22, 30], [20, 21, 23, 31, 32]]


class OpenBeamRef(R.BeamRef):
    """beam_ref.BeamRef.step with the open rules."""

    def step(self, logits=None, cands=None, advance: bool = True):
        B, K, n = self.B, 2 * self.B, self.N * self.B
        cs, ct, cl = self.candidates(logits) if cands is None else cands
        parent_row, token_row, lp_row = np.full(n, -1), np.full(n, -1), np.full(n, np.nan)
        next_ids, all_pairs = np.full(n, self.pad, dtype=np.int64), []
        for e in range(self.N):
            base = e * B
            if self.done[e]:
                all_pairs.append([])
                continue
            slot_of_rank = np.zeros(B, dtype=np.int64)
            slot_of_rank[self.rank_of_slot[base:base + B]] = np.arange(B)
            merged = sorted(((-np.float64(np.float32(cs[base + slot_of_rank[r], k])), r, int(ct[base + slot_of_rank[r], k]), k)
                             for r in range(B) for k in range(K)), key=lambda x: (x[0], x[1], x[3]))[:K]
            live, cur = [], self.cur_len[e]
            for place, (negc, r, t, k) in enumerate(merged):
                slot = int(slot_of_rank[r])
                c, lp = np.float32(-negc), cl[base + slot, k]
                if t < 0 or np.isneginf(c):                        # open: the row of a slot that holds no beam
                    continue
                if self.eos >= 0 and t == self.eos:
                    if place < B:
                        self.add(e, c, cur, self.steps, base + slot, lp)
                    continue
                live.append((slot, t, c, lp))
                if len(live) == B:
                    break
            done = len(live) == 0                                  # open: the example goes on while any beam lives
            if not done and len(self.heaps[e]) >= B:
                done = self.early_stopping or self.worst(e) >= R.hyp_score(-merged[0][0], cur, self.length_penalty)
            has_child, first = [False] * B, []
            for (p, _, _, _) in live:
                first.append(not has_child[p])
                has_child[p] = True
            free = [s for s in range(B) if not has_child[s]]
            pairs = []
            for q, (p, t, c, lp) in enumerate(live):
                slot = p if first[q] else free.pop(0)
                if slot != p and not done:
                    pairs.append((base + p, base + slot))
                g = base + slot
                self.score[g], self.rank_of_slot[g] = c, q
                next_ids[g] = self.pad if done else t
                parent_row[g], token_row[g], lp_row[g] = base + p, t, lp
            for q in range(len(live), B):
                g = base + free.pop(0)
                self.score[g], self.rank_of_slot[g] = -np.inf, q
            all_pairs.append(pairs)
            self.cur_len[e] = cur + 1
            if done:
                self.done[e] = True
                self.state[base:base + B] = R.ROW_FINISHED
        self.trellis.append((parent_row, token_row, lp_row))
        self.steps += 1
        return next_ids, all_pairs


@pytest.mark.parametrize("n_ex", [1, 3])
@pytest.mark.parametrize("beams", [2, 4, 8])
def test_open_advance_follows_the_reference_step_by_step(beams, n_ex):
    """After the second step fewer beams live than there are slots, the third step's forks take the left-over slots again (with their
    K/V pair), closed members fill the heap, and the example ends when no beam lives -- or, with as many hypotheses as beams, by the
    heap rule."""
    vocab, steps = 64, 8
    rng = np.random.default_rng(97 * beams + n_ex)
    tab = torch.from_numpy((2.5 * rng.standard_normal((vocab, vocab))).astype(np.float32)).cuda()
    slots = n_ex * beams
    lens = [5 + 3 * e for e in range(n_ex)]
    bs = BeamSearch(n_ex, beams, vocab, steps, "cuda", eos=EOS, pad=0, length_penalty=0.0)
    bs.admit(lens)
    bs.guide = DeviceGuide(ChoiceSets([SET]), slots, vocab, "cuda", EOS)
    bs.guide.admit(range(slots), [0] * slots)
    ref = OpenBeamRef(lens, beams, EOS, 0, 0.0, False)
    state = torch.full((slots,), ops.ROW_ACTIVE, dtype=I32, device="cuda")
    pos = torch.tensor(np.repeat(lens, beams), dtype=I32, device="cuda")
    last = torch.tensor(np.repeat([(11 * e + 3) % vocab for e in range(n_ex)], beams), dtype=I64, device="cuda")
    offs = torch.tensor(np.repeat([5 * e for e in range(n_ex)], beams), dtype=I64, device="cuda")
    partial = retaken = 0
    for step in range(steps):
        logits = tab[(last + offs) % vocab].contiguous()
        BK._load_ref(ref, bs, state)
        was_done = list(ref.done)
        empty_before = np.isneginf(ref.score)
        pos_before = pos.clone()
        nxt, done = bs.step(logits, state, pos if step else None, last=last if step else None)
        cs = bs.cand_score.cpu().numpy()
        want_next, want_pairs = ref.step(cands=(cs, bs.cand_token.cpu().numpy().astype(np.int64), bs.cand_logprob.cpu().numpy().astype(np.float64)))
        BK._same_state(ref, bs, state, step)
        assert nxt.cpu().tolist() == want_next.tolist() and done == ref.done
        adv = np.repeat([0 if (w or step == 0) else 1 for w in was_done], beams)
        assert (pos.cpu().numpy() - pos_before.cpu().numpy()).tolist() == adv.tolist()
        cnt, pairs = bs.pair_count.cpu().tolist(), bs.pairs.cpu().numpy()
        parent = ref.trellis[-1][0]
        for e in range(n_ex):
            got = [tuple(int(x) for x in pairs[e, i]) for i in range(cnt[e])]
            assert got == want_pairs[e], f"step {step} example {e}: pairs {got} vs {want_pairs[e]}"
            sl = slice(e * beams, (e + 1) * beams)
            if not was_done[e]:
                assert not any(empty_before[p] for p in parent[sl] if p >= 0), f"step {step}: a slot without a beam became a parent"
                live = int((parent[sl] >= 0).sum())
                partial += 0 < live < beams and not ref.done[e]
                for s in range(e * beams, (e + 1) * beams):       # a left-over slot that takes a beam again does so by a copy of its parent
                    if empty_before[s] and parent[s] >= 0:
                        retaken += 1
                        assert (int(parent[s]), s) in got
        last = nxt.clone()
        if all(done):
            break
    assert all(ref.done), "the search did not end within the set's longest member"
    if beams >= 4:
        assert partial > 0, "no step had fewer live beams than slots: the open rule was not exercised"
        assert retaken > 0, "no left-over slot took a beam again"
    got, want = bs.hypotheses(1), ref.finalize(1)
    for e in range(n_ex):
        g, w = got[e][0], want[e][0]
        assert g["tokens"] == w["tokens"] and g["tokens"] in SET and g["eos"] and np.float32(g["sum"]) == np.float32(w["sum"])
        assert [np.float32(x) for x in g["logprobs"]] == [np.float32(x) for x in w["logprobs"]]
    assert int(bs.fallbacks.item()) == 0
