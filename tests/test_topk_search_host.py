"""Host side of the fused top-K search: EmbANN.topk on CPU tensors is the first k columns of EmbANN._ann, and the C ABI declares the
three entry points of csrc/search.hip."""
import pytest
import torch


def _int_emb(rows, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-3, 4, (rows, D), generator=g).float()


@pytest.mark.parametrize("k", [1, 5, 10])
def test_embann_topk_cpu_equals_ann_truncated(k):
    from simseg.tasks.clip.hooks.utils import EmbANN, IndexedEmbInfo
    M, N, D = 37, 211, 64
    # integer-valued embeddings: every score is an exact small integer, ties are plentiful; right ids repeat (5 rows per id)
    left = IndexedEmbInfo("image", torch.arange(M), _int_emb(M, D, 1))
    right = IndexedEmbInfo("text", torch.arange(N) // 5, _int_emb(N, D, 2))
    sim = left.emb_mat @ right.emb_mat.T
    assert (sim.sort(dim=1).values.diff(dim=1) == 0).any(), "the case is meant to have tied scores"
    ann = EmbANN()
    want_sorted, want_matched = ann._ann(left, right)
    got_sorted, got_matched = ann.topk(left, right, k)
    assert got_sorted.shape == (M, k) and got_matched.shape == (M, k)
    assert torch.equal(got_sorted, want_sorted[:, :k])
    assert torch.equal(got_matched, want_matched[:, :k])
    assert got_matched.dtype == torch.bool and got_matched.any()


def test_header_declares_search_entry_points():
    from simseg_amd.lib import parse_header
    protos = parse_header()
    for name in ("simseg_topk_search_workspace_bytes", "simseg_topk_search", "simseg_topk_merge"):
        assert name in protos, name
    args = [n for _, n in protos["simseg_topk_search"][1]]
    assert args[:3] == ["q", "g", "dtype"] and "index_offset" in args and args[-1] == "stream"
    assert [n for _, n in protos["simseg_topk_merge"][1]][-3:] == ["M", "K", "stream"]
