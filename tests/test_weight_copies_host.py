"""The staleness rules of the towers' derived weight copies (simseg_amd.towers.DerivedCopies) as pure host logic: CPU parameters, a "copy"
that is `w.detach().to(torch.bfloat16)` or a plain object.  What the copies hold and that every tower path reads the right one is the
subject of tests/test_gpu_weight_copies.py.  No GPU."""
import gc

import pytest
import torch

BF16, F16 = torch.bfloat16, torch.float16


@pytest.fixture
def towers():
    from simseg_amd import towers
    towers.invalidate_weight_cache()
    yield towers
    towers.invalidate_weight_cache()


def _lin(seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.Parameter(torch.randn(4, 4, generator=g)), torch.nn.Parameter(torch.randn(4, generator=g))


def _fill(copies, w, b):
    """One entry of every kind the towers make from a Linear's weight (and bias)."""
    made = {"w16": w.detach().to(BF16), "split": object(), "qscaled": (object(), object())}
    copies.put("w16", (w,), BF16, made["w16"])
    copies.put("split", (w,), None, made["split"])
    copies.put("qscaled", (w, b), BF16, made["qscaled"])
    return made


def test_hit_is_the_same_object_and_the_tag_counts(towers):
    c = towers.DerivedCopies()
    w, _ = _lin()
    assert c.get("w16", (w,), BF16) is None
    w16 = w.detach().to(BF16)
    assert c.put("w16", (w,), BF16, w16) is w16
    assert c.get("w16", (w,), BF16) is w16 and c.get("w16", (w,), BF16) is w16
    assert c.get("w16", (w,), F16) is None                      # another tag: a miss
    assert c.get("split", (w,)) is None                         # another kind
    assert c.count("w16") == 1 and c.count("split") == 0
    other, _ = _lin(1)
    assert c.get("w16", (other,), BF16) is None


def test_writes_torch_can_see_are_misses(towers):
    c = towers.DerivedCopies()
    w, _ = _lin()
    c.put("w16", (w,), BF16, w.detach().to(BF16))
    with torch.no_grad():
        w.mul_(2.0)                                             # `_version` moves
    assert c.get("w16", (w,), BF16) is None
    c.put("w16", (w,), BF16, w.detach().to(BF16))
    assert c.get("w16", (w,), BF16) is not None
    w.data = w.data.clone()                                     # the storage moves, `_version` does not
    assert c.get("w16", (w,), BF16) is None


def test_write_through_data_needs_invalidate(towers):
    """p.data carries a version counter of its own: the documented reason invalidate_weight_cache() exists."""
    w, _ = _lin()
    stale = towers.COPIES.put("w16", (w,), BF16, w.detach().to(BF16))
    v0 = w._version
    w.data.mul_(2.0)
    assert w._version == v0
    assert towers.COPIES.get("w16", (w,), BF16) is stale        # still a hit, with the old values
    towers.invalidate_weight_cache()
    assert towers.COPIES.get("w16", (w,), BF16) is None and towers.COPIES.count("w16") == 0


def test_rewriting_the_bias_drops_only_what_was_made_from_it(towers):
    w, b = _lin()
    made = _fill(towers.COPIES, w, b)
    towers.weights_rewritten(b, b.detach().to(BF16))
    assert towers.COPIES.get("qscaled", (w, b), BF16) is None and towers.COPIES.count("qscaled") == 0
    assert towers.COPIES.get("w16", (w,), BF16) is made["w16"]
    assert towers.COPIES.get("split", (w,)) is made["split"]


def test_rewriting_the_weight_drops_every_kind_and_installs_the_copy(towers):
    w, b = _lin()
    k, v = _lin(1)[0], _lin(2)[0]
    _fill(towers.COPIES, w, b)
    towers.COPIES.put("cat", (w, k, v), BF16, ([object()] * 3, object()))
    kept = towers.COPIES.put("w16", (k,), BF16, k.detach().to(BF16))
    p16 = w.detach().to(F16)
    towers.weights_rewritten(w, p16)                            # (through raw pointers: neither `_version` nor `data_ptr()` moved)
    assert towers.COPIES.get("w16", (w,), F16) is p16 and towers.COPIES.get("w16", (w,), BF16) is None
    assert towers.COPIES.get("split", (w,)) is None and towers.COPIES.get("qscaled", (w, b), BF16) is None
    assert towers.COPIES.get("cat", (w, k, v), BF16) is None
    assert [towers.COPIES.count(kind) for kind in ("w16", "split", "qscaled", "cat")] == [2, 0, 0, 0]      # released, not left to a lookup
    assert towers.COPIES.get("w16", (k,), BF16) is kept


def test_a_plain_tensor_source_is_never_stored(towers):
    c = towers.DerivedCopies()
    w, b = _lin()
    view = w.detach().reshape(2, 8)                             # (the reshaped patch-embedding weight: a view, made anew every forward)
    x = object()
    assert c.put("w16", (view,), BF16, x) is x and c.get("w16", (view,), BF16) is None
    assert c.put("qscaled", (w, b.detach()), BF16, x) is x and c.get("qscaled", (w, b.detach()), BF16) is None
    assert c.count("w16") == 0 and c.count("qscaled") == 0 and not c._of


def test_dead_parameters_are_swept_with_their_index_keys(towers, monkeypatch):
    monkeypatch.setattr(towers.DerivedCopies, "SWEEP", 8)
    c = towers.DerivedCopies()
    owners = [torch.nn.Linear(4, 4) for _ in range(5)]
    for lin in owners:                                          # 10 entries > SWEEP, all live: nothing to sweep
        c.put("w16", (lin.weight,), BF16, object())
        c.put("qscaled", (lin.weight, lin.bias), BF16, object())
    assert c.count("w16") == 5 and c.count("qscaled") == 5 and len(c._of) == 10
    dead = {id(p) for lin in owners[:4] for p in lin.parameters()}
    last = owners[4]
    w, b = _lin()                                               # (made while the others live: their ids are not handed out again here)
    del owners, lin
    gc.collect()
    c.put("qscaled", (w, b), BF16, object())                   # a store past the bound
    assert c.count("w16") == 1 and c.count("qscaled") == 2
    assert not dead & {i for key in c._ent for i in key[1:]}
    assert set(c._of) == {id(last.weight), id(last.bias), id(w), id(b)}
