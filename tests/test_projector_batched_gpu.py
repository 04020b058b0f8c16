"""GPU: the mm_projector splice over a batch of clips.  Equal-length views of one contiguous tensor, in consecutive batch rows at the
same start, go through ONE split and ONE batched product (llark_gemm16_batched_bias, a clip's C stride = a whole sequence of h);
everything else keeps the per-segment loop.  Each clip's rows are computed by the same kernel at the same m either way, so the hidden
state is bit-equal."""
import pytest
import torch

pytestmark = pytest.mark.gpu

H, MM, VOCAB = 256, 96, 128


def _setup(B, S, F, seed):
    gen = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, VOCAB, (B, S), generator=gen).cuda()
    table = (torch.randn(VOCAB, H, generator=gen) * 0.1).bfloat16().cuda()
    proj_w = (torch.randn(H, MM, generator=gen) * 0.1).bfloat16().cuda()
    proj_b = (torch.randn(H, generator=gen) * 0.1).cuda()
    emb = torch.randn(B, F, MM, generator=gen).cuda()
    return ids, table, proj_w, proj_b, emb


def _splice(ids, table, proj_w, proj_b, segs, split, monkeypatch):
    """embed_splice into a fresh h; returns (h, number of batched products, number of per-segment products)."""
    from llark_amd import ops
    from llark_amd.m2t import engine as EN
    B, S = ids.shape
    h = torch.full((B * S, H), float("nan"), device="cuda")
    calls = {"batched": 0, "loop": 0}
    real_b, real_g = ops.gemm16_batched_bias, ops.gemm16

    def spy_b(*a, **k):
        calls["batched"] += 1
        return real_b(*a, **k)

    def spy_g(*a, **k):
        calls["loop"] += 1
        return real_g(*a, **k)

    monkeypatch.setattr(ops, "gemm16_batched_bias", spy_b)
    monkeypatch.setattr(ops, "gemm16", spy_g)
    EN.embed_splice(ids, table, h, segs, proj_w, proj_b, split)
    monkeypatch.setattr(ops, "gemm16_batched_bias", real_b)
    monkeypatch.setattr(ops, "gemm16", real_g)
    return h, calls["batched"], calls["loop"]


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("F,S", [(5, 12), (40, 48)])           # m <= 16: the weight-streaming kernel per clip; above: the tile kernel's batch dimension
def test_uniform_segments_take_the_batched_path_bit_equal(F, S, split, monkeypatch):
    B, start = 3, 2
    ids, table, proj_w, proj_b, emb = _setup(B, S, F, seed=F)
    h_b, nb, nl = _splice(ids, table, proj_w, proj_b, [(b, start, emb[b]) for b in range(B)], split, monkeypatch)
    assert (nb, nl) == (1, 0), "uniform segments did not take the batched path"
    # the same frames as separate tensors: not views of one tensor, so the loop
    h_l, nb, nl = _splice(ids, table, proj_w, proj_b, [(b, start, emb[b].clone()) for b in range(B)], split, monkeypatch)
    assert (nb, nl) == (0, B)
    assert torch.isfinite(h_b).all() and torch.equal(h_b, h_l), "the batched splice differs from the per-segment loop"
    gathered = table.float()[ids.reshape(-1)]
    rows = torch.zeros(B * S, dtype=torch.bool, device="cuda")
    for b in range(B):
        rows[b * S + start + 1: b * S + start + 1 + F] = True
    assert torch.equal(h_b[~rows], gathered[~rows]), "rows outside the audio positions changed"
    want = emb.reshape(B * F, MM).bfloat16().double() @ proj_w.double().t() + proj_b.double()
    if not split:
        assert float((h_b[rows].double() - want).abs().max()) <= 1e-5 * float(want.abs().max())      # fp32 accumulation of exact bf16 products


def test_other_segment_layouts_take_the_loop(monkeypatch):
    B, S, F = 3, 16, 5
    ids, table, proj_w, proj_b, emb = _setup(B, S, F, seed=1)
    uniform = [(b, 2, emb[b]) for b in range(B)]
    cases = {"ragged starts": [(0, 2, emb[0]), (1, 3, emb[1]), (2, 2, emb[2])],
             "batch rows out of order": [uniform[1], uniform[0], uniform[2]],
             "a gap in the batch rows": [(0, 2, emb[0]), (2, 2, emb[1])],
             "one segment": uniform[:1],
             "views that skip a clip": [(0, 2, emb[0]), (1, 2, emb[2])]}
    for what, segs in cases.items():
        h, nb, nl = _splice(ids, table, proj_w, proj_b, segs, True, monkeypatch)
        assert (nb, nl) == (0, len(segs)), what
        h_ref, _, _ = _splice(ids, table, proj_w, proj_b, [(b, st, f.clone()) for b, st, f in segs], True, monkeypatch)
        assert torch.equal(h, h_ref), what
