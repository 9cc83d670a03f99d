"""Host side of the tensor table that AdamW and LARS share (simseg_amd.optim.TensorTable): the chunk lists, the (lr, weight_decay) table
word and the single handoff to the towers' weight caches.  No GPU."""
import os
import re
import struct

import numpy as np
import pytest

from conftest import REPO


def test_chunk_lists():
    from simseg_amd.optim import CHUNK, chunk_lists
    tid, coff, first = chunk_lists([1, 0, CHUNK, CHUNK + 1, 2 * CHUNK], CHUNK)
    assert (tid.dtype, coff.dtype, first.dtype) == (np.int32, np.int64, np.int32)
    assert tid.tolist() == [0, 2, 3, 3, 4, 4]
    assert coff.tolist() == [0, 0, 0, CHUNK, 0, CHUNK]
    assert first.tolist() == [0, 1, 1, 2, 4, 6]
    assert first[1] == first[2]                       # the tensor without elements owns no chunk
    assert first[-1] == len(tid)


@pytest.mark.parametrize("lr, wd", [(0.0, 0.0), (1e-4, 1e-3), (0.5, 0.0), (1e-45, 3.0), (-0.0, 1e-40), (123.25, 2.0 ** -126)])
def test_lr_wd_word(lr, wd):
    """Two float32 in one little-endian 8-byte word, lr first: what the kernels read as `float lr; float wd;`."""
    from simseg_amd.optim import pack_lr_wd
    words = pack_lr_wd([lr, 7.0], [wd, 9.0])
    assert words.dtype == np.int64 and words.shape == (2,)
    assert int(words[0]) == struct.unpack("<q", struct.pack("<ff", lr, wd))[0]
    assert int(words[1]) == struct.unpack("<q", struct.pack("<ff", 7.0, 9.0))[0]


def test_one_handoff_to_the_weight_caches():
    from simseg_amd import towers
    assert callable(towers.weights_rewritten) and "_version" in towers.weights_rewritten.__doc__ and "data_ptr" in towers.weights_rewritten.__doc__
    src = open(os.path.join(REPO, "simseg_amd", "optim.py")).read()
    assert not re.search(r"\b(drop_split_copy|drop_qscaled_copy|register_w16)\b", src)
    assert len(re.findall(r"\bweights_rewritten\(", src)) == 2            # AdamW.step and LARS.step
