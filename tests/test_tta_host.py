"""Host side of the multi-scale / flip test-time augmentation (segpost.tta_sizes, the integer nearest index, the tool's flag checks, the
C ABI of simseg_slide_extract_flip / simseg_slide_stitch_multi).  No GPU."""
import argparse
import ctypes
import importlib.util
import os
from fractions import Fraction

import numpy as np
import pytest

from conftest import REPO

import _tta_ref as TR


def test_tta_sizes_rounding():
    from simseg_amd import segpost
    sizes = [(40, 56), (19, 45), (75, 50), (1, 3)]
    got = segpost.tta_sizes(sizes, [0.5, 1.0, 1.5, 0.75, 0.01])
    # 0.5 * odd rounds half up (floor(x + 0.5)): 19 -> 10, 45 -> 23, 75 -> 38; 1 -> 1 (0.5 + 0.5), 3 -> 2
    assert got[0] == [(20, 28), (10, 23), (38, 25), (1, 2)]
    assert got[1] == [tuple(s) for s in sizes]
    assert got[2] == [(60, 84), (29, 68), (113, 75), (2, 5)]          # 28.5 -> 29, 67.5 -> 68, 112.5 -> 113, 1.5 -> 2, 4.5 -> 5
    assert got[3] == [(30, 42), (14, 34), (56, 38), (1, 2)]           # 14.25 -> 14, 33.75 -> 34, 56.25 -> 56, 37.5 -> 38, 0.75 -> 1, 2.25 -> 2
    assert got[4] == [(1, 1)] * 4                                     # the floor at 1
    for s, per in zip([0.5, 1.0, 1.5, 0.75, 0.01], got):
        assert per == [TR.pass_size(H, W, s) for H, W in sizes]
    with pytest.raises(ValueError):
        segpost.tta_sizes(sizes, [0.0])
    with pytest.raises(ValueError):
        segpost.tta_sizes(sizes, [float("nan")])


@pytest.mark.parametrize("L,Lp", [(40, 1), (40, 40), (40, 60), (19, 10), (19, 29), (75, 38), (7, 100), (512, 384), (513, 641), (1, 5)])
def test_nearest_index_against_float64(L, Lp):
    """The integer formula == floor((i + 0.5) * Lp / L) clamped to Lp - 1, the pixel-centre nearest index.  The float64 evaluation is
    checked against exact rationals too: (2i + 1) Lp / (2L) is never within rounding of an integer unless it is one."""
    from simseg_amd import segpost
    for i in range(L):
        got = segpost.tta_nearest_index(i, L, Lp)
        exact = min(int(Fraction((2 * i + 1) * Lp, 2 * L).__floor__()), Lp - 1)
        f64 = min(int(np.floor((np.float64(i) + 0.5) * np.float64(Lp) / np.float64(L))), Lp - 1)
        assert got == exact == f64, (i, L, Lp, got, exact, f64)
        assert 0 <= got < Lp
    idx = TR.nearest_index(L, Lp)
    assert idx.tolist() == [segpost.tta_nearest_index(i, L, Lp) for i in range(L)]
    assert (np.diff(idx) >= 0).all()                                   # monotone: a tile's sample rectangle is spanned by its corners
    if Lp == L:
        assert idx.tolist() == list(range(L))
    if Lp == 1:
        assert not idx.any()


def _tool():
    spec = importlib.util.spec_from_file_location("seg_eval_device_tool", os.path.join(REPO, "tools", "seg_eval_device.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _ns(**kw):
    base = dict(scales="", flip=False, slide="", device_preproc=False)
    base.update(kw)
    return argparse.Namespace(**base)


def test_tool_flag_errors():
    tool = _tool()
    assert tool.tta_options(_ns()) == (None, False)
    assert tool.tta_options(_ns(slide="96,48")) == (None, False)
    assert tool.tta_options(_ns(scales="0.75,1.0,1.25", flip=True, slide="512,256", device_preproc=True)) == ([0.75, 1.0, 1.25], True)
    assert tool.tta_options(_ns(flip=True, slide="512,256", device_preproc=True)) == ([1.0], True)
    with pytest.raises(SystemExit, match="1.0"):
        tool.tta_options(_ns(scales="0.75,1.25", slide="512,256", device_preproc=True))
    with pytest.raises(SystemExit, match="--slide"):
        tool.tta_options(_ns(flip=True, device_preproc=True))
    with pytest.raises(SystemExit, match="--device-preproc"):
        tool.tta_options(_ns(scales="0.5,1.0", slide="512,256"))
    with pytest.raises(SystemExit, match="numbers"):
        tool.tta_options(_ns(scales="1.0,big", slide="512,256", device_preproc=True))
    with pytest.raises(SystemExit, match="positive"):
        tool.tta_options(_ns(scales="1.0,-2", slide="512,256", device_preproc=True))
    with pytest.raises(SystemExit, match="at most 16"):
        tool.tta_options(_ns(scales=",".join(str(1.0 + 0.1 * i) for i in range(9)), flip=True, slide="512,256", device_preproc=True))


def test_tool_parses_the_new_flags(monkeypatch):
    tool = _tool()
    monkeypatch.setattr("sys.argv", ["seg_eval_device.py", "--cfg", "x.yaml", "--slide", "32,16", "--device-preproc", "--scales", "0.5,1.0,1.5", "--flip"])
    args, rest = tool.parse_args()
    assert args.scales == "0.5,1.0,1.5" and args.flip and rest == []
    monkeypatch.setattr("sys.argv", ["seg_eval_device.py", "--cfg", "x.yaml"])
    args, _ = tool.parse_args()
    assert args.scales == "" and args.flip is False


def test_header_declares_and_library_exports_the_entries():
    from simseg_amd import lib
    protos = lib.parse_header()
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in ("simseg_slide_extract_flip", "simseg_slide_stitch_multi", "simseg_slide_stitch_multi_workspace_bytes"):
        assert name in protos, f"{name} is not declared in include/simseg_hip.h"
        assert hasattr(so, name), f"{name} is declared but not exported"
    assert len(protos["simseg_slide_extract_flip"][1]) == len(protos["simseg_slide_extract"][1]) + 1
    assert [n for _, n in protos["simseg_slide_stitch_multi"][1]][:3] == ["pass_tab", "P", "img_tab"]
    l = lib.load()
    assert l.simseg_slide_stitch_multi_workspace_bytes(2, 5, 100, 130) == l.simseg_slide_stitch_workspace_bytes(2, 5, 100, 130) > 0
    # argument validation happens before any device work: the cap on the number of passes is refused without a GPU
    args = [None, 17, None, None, None, None, None, None, 1, 5, 2, 7, 32, 40, 56, 40 * 56, None]
    assert l.simseg_slide_stitch_multi(*args) != 0
    assert b"17 passes" in l.simseg_last_error() and b"<= 16" in l.simseg_last_error()
    args[1] = 0
    assert l.simseg_slide_stitch_multi(*args) != 0
    args[1] = 16
    assert l.simseg_slide_stitch_multi(*args) != 0 and b"null pointer" in l.simseg_last_error()


def test_reference_masks_stay_clear_of_the_threshold():
    """The seeded inputs of tests/test_gpu_tta.py, through the NumPy reference alone: pixels whose reference prob lies within 1e-5 of 0.5
    (where a device rounding may flip the mask) number at most 0.1 % of all mask pixels."""
    case = TR.fusion_case()
    assert any(len(o[b]) == 1 for o in case["offs"] for b in range(len(TR.SIZES)))                      # a pass with a single window
    assert any(h < TR.WIN and w < TR.WIN for per in case["sizes"] for h, w in per)                      # an image smaller than one window
    near = total = 0
    for b in range(len(TR.SIZES)):
        for k in range(TR.K):
            if case["cand"][b][k] < 0:
                continue
            prob = case["ref"][(b, k)][0]
            near += int((np.abs(prob - 0.5) < 1e-5).sum())
            total += prob.size
    assert total > 0 and near <= 1e-3 * total, (near, total)
