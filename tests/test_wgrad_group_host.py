"""ops.wgrad_group_plan: the slice count of a grouped split-K weight-gradient launch (plain arithmetic, no GPU)."""
from simseg_amd import ops

BLOCK = (36, 36, 9, 27)          # fc2, fc1, proj, qkv of ViT-B / BERT-base in 256x256 tiles


def test_block_shapes():
    assert ops.wgrad_group_plan(BLOCK, 1576) == 7         # ViT-B, 512 x 197 rows: 756 blocks = 2.95 rounds of 256
    assert ops.wgrad_group_plan(BLOCK, 340) == 7          # the packed text tower (~21.8 k rows)
    assert ops.wgrad_group_plan(BLOCK, 20) == 1


def test_slices_stay_sixteen_k_tiles_deep_and_fall_back_to_one():
    prev = None
    for nk in range(400, 0, -1):
        sk = ops.wgrad_group_plan(BLOCK, nk)
        assert sk == 1 or nk // sk >= 16, (nk, sk)
        if nk < 32:
            assert sk == 1, (nk, sk)
        if prev is not None and prev == 1 and nk < 64:
            assert sk == 1, (nk, sk)                      # once at 1 on the way down, it stays there
        prev = sk


def test_fewer_cus_never_more_rounds_than_needed():
    assert ops.wgrad_group_plan((1, 3, 4, 4), 112) == 7   # 12 tiles x 7 = 84 blocks: one round
    assert ops.wgrad_group_plan((1,), 16) == 1
    assert ops.wgrad_group_plan((64, 64, 64, 64), 1576) == 1      # a full round of tiles already: nothing to gain from slicing
