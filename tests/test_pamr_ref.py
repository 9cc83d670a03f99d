"""The float64 statements of PAMR (tests/_pamr_ref.py) against each other and against the properties of the definition, and the
argument checks of ops.pamr, the `refiner` keyword and the evaluation tool's flags as far as they run without a device."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import _pamr_ref as P
from conftest import REPO

SIZES = [(64, 64), (16, 16), (40, 56), (17, 50)]


@pytest.mark.parametrize("H,W", SIZES)
def test_two_formulations_agree(H, W):
    rgb, maps = P.scene(H, W, 2, seed=H * 100 + W)
    w0, w1 = P.weights_np(rgb), P.weights_torch(rgb).numpy()
    assert np.abs(w0 - w1).max() <= 1e-12
    assert np.abs(w0.sum(0) - 1.0).max() <= 1e-12                   # the weights of a pixel sum to one
    a, b = P.pamr_np(rgb, maps), P.pamr_torch(rgb, maps)
    print(f"{H}x{W}: the two float64 formulations differ by {np.abs(a - b).max():.2e}")
    assert np.abs(a - b).max() <= 1e-12
    for dil in [(1,), (3, 64)]:
        assert np.abs(P.pamr_np(rgb, maps, dil, 3) - P.pamr_torch(rgb, maps, dil, 3)).max() <= 1e-12


def test_flat_image_gives_uniform_weights():
    rgb = np.full((20, 33, 3), 77, np.uint8)
    w = P.weights_np(rgb)
    assert w.shape == (48, 20, 33) and (w == 1.0 / 48.0).all()       # exactly: exp(0) = 1, 48 ones, one division
    assert np.abs(P.weights_torch(rgb).numpy() - 1.0 / 48.0).max() <= 1e-15


def test_constant_map_is_a_fixed_point_and_zero_iterations_return_the_input():
    rgb, maps = P.scene(40, 56, 2, seed=5)
    const = np.full((1, 40, 56), 0.3)
    assert np.abs(P.pamr_np(rgb, const) - 0.3).max() <= 1e-12
    assert np.abs(P.pamr_torch(rgb, const) - 0.3).max() <= 1e-12
    assert np.array_equal(P.pamr_np(rgb, maps, iters=0), maps.astype(np.float64))
    assert np.array_equal(P.pamr_torch(rgb, maps, iters=0), maps.astype(np.float64))
    out = P.pamr_np(rgb, maps)
    assert out.min() >= maps.min() - 1e-12 and out.max() <= maps.max() + 1e-12        # a convex combination


def test_ops_pamr_checks_its_arguments_before_it_needs_a_device():
    from simseg_amd import ops
    rgb, prob = torch.zeros(2, 32, 32, 3, dtype=torch.uint8), torch.zeros(2, 3, 32, 32)
    with pytest.raises(TypeError):
        ops.pamr(rgb.float(), prob)
    with pytest.raises(TypeError):
        ops.pamr(rgb, prob.double())
    with pytest.raises(TypeError):
        ops.pamr(rgb[0], prob)                                       # a single image with a batch of maps
    for bad in [(), (0,), (65,), (1,) * 9, (1.5,), 3]:
        with pytest.raises(ValueError):
            ops.pamr(rgb, prob, dilations=bad)
    for bad in [-1, 65, 2.5]:
        with pytest.raises(ValueError):
            ops.pamr(rgb, prob, iters=bad)
    with pytest.raises(ValueError):
        ops.pamr(rgb, torch.zeros(2, 9, 32, 32))                     # K = 9
    with pytest.raises(ValueError):
        ops.pamr(rgb, prob, scale=0)
    with pytest.raises(ValueError):
        ops.pamr(rgb, prob, scale=2)                                 # 64 x 64 maps for 32 x 32 images
    with pytest.raises(ValueError):
        ops.pamr(rgb, prob, cand_idx=torch.zeros(2, 3, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.pamr(rgb, prob, cand_idx=torch.zeros(2, 5, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pamr(rgb, prob)                                          # everything fits: now it wants the device
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pamr(rgb[0], prob[0], cand_idx=torch.zeros(3, dtype=torch.int32), scale=1)
    assert ops.pamr_check([1, 2, 4], 0) == (1, 2, 4)


def test_refiner_keyword():
    from simseg_amd import segpost
    assert segpost.parse_refiner(None) is None and segpost.parse_refiner("crf") is None
    assert segpost.parse_refiner(None, crf=False) is None and segpost.parse_refiner("crf", crf=False) is None
    assert segpost.parse_refiner("pamr") == ("pamr", {})
    assert segpost.parse_refiner(("pamr", {"iters": 3, "dilations": (1, 2)})) == ("pamr", {"iters": 3, "dilations": (1, 2)})
    assert segpost.PAMR_PARAMS == dict(dilations=(1, 2, 4, 8, 12, 24), iters=10)
    for bad in ["densecrf", ("pamr",), ("pamr", 3), ("crf", {}), 5, ("pamr", {"sigma": 1}), ("pamr", {"iters": 65}), ("pamr", {"dilations": (0,)})]:
        with pytest.raises(ValueError):
            segpost.parse_refiner(bad)
    with pytest.raises(ValueError, match="crf=False"):
        segpost.parse_refiner("pamr", crf=False)
    # every entry point refuses before it touches the model
    x, text = torch.zeros(1, 3, 32, 32), torch.zeros(4, 512)
    for fn, args in [(segpost.encode_batch, (None, x, text, 10)), (segpost.encode_batch_sliding, (None, x, text, 10)),
                     (segpost.encode_images_sliding, (None, [x[0]], text, 10)), (segpost.encode_images_multiscale, (None, [], text, 10)),
                     (segpost.eval_batch, (None, x, torch.zeros(1, 32, 32, dtype=torch.uint8), text, 10)),
                     (segpost.evaluate_sharded, (None, [], text, 10))]:
        with pytest.raises(ValueError, match="crf=False"):
            fn(*args, crf=False, refiner="pamr")
        with pytest.raises(ValueError, match="refiner"):
            fn(*args, refiner="bilateral")
    with pytest.raises(ValueError, match="refine hook"):
        segpost.encode_batch(None, x, text, 10, refine=lambda *a: None, refiner="pamr")


def test_eval_tool_flags(monkeypatch):
    spec = importlib.util.spec_from_file_location("seg_eval_device_flags", os.path.join(REPO, "tools", "seg_eval_device.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)

    def parse(*argv):
        monkeypatch.setattr(sys, "argv", ["seg_eval_device.py", "--cfg", "x.yaml", *argv])
        return tool.parse_args()[0]

    assert parse().refine == "crf" and parse().refiner is None
    assert parse("--refine", "pamr").refiner == ("pamr", {})
    assert parse("--refine", "pamr", "--pamr-iters", "4", "--pamr-dilations", "1,3,9").refiner == ("pamr", {"iters": 4, "dilations": (1, 3, 9)})
    for bad in [("--refine", "pamr", "--no-crf"), ("--refine", "pamr", "--host-crf"), ("--refine", "bilateral"), ("--pamr-iters", "3"),
                ("--refine", "pamr", "--pamr-iters", "65"), ("--refine", "pamr", "--pamr-dilations", "1,x"),
                ("--refine", "pamr", "--pamr-dilations", "0")]:
        with pytest.raises(SystemExit):
            parse(*bad)
