"""The derived weight copies the 16-bit and split-fp32 towers cache per parameter (simseg_amd/towers.py DerivedCopies: the kinds "w16",
"cat", "split", "qscaled"; its staleness rules alone, without a GPU: tests/test_weight_copies_host.py) against a
FRESH module: a new module of the same class and config, loaded with the model's state_dict, has no cache entry that could match, so after
every way a weight can be written the model under test must evaluate bit for bit as that module does (same input, same compute mode, same
switches).  Bit-identity is the bar: every copy is an exact function of the fp32 masters (the optimizer kernel rounds as torch does), the
evaluations are forward-only and ops.gemm defaults to splitk=1 - and each comparison first checks that two runs of the fresh module agree
bit for bit.

Routes: W16 (the 16-bit copies every 16-bit GEMM reads, bf16 and fp16), CAT (BERT's concatenated q / k / v copy, bf16 evaluation without this
package's optimizer keeping the copies adjacent), W3 (the split-bf16x3 copies of exact-mode evaluation), WQS (the folded q-scaled qkv copy of
16-bit evaluation at T >= 512).  Writes: (a) simseg_amd.optim.AdamW.step() without a scaler, (b) under a GradScaler, taken, (c) under a
GradScaler, skipped, as the first step of a new launch plan (new optimizer, after opt.load_state_dict, after set_param_streams, after the
parameters' storage moved), (d) torch-side in-place writes, (e) model.load_state_dict, (f) a write through p.data followed by
towers.invalidate_weight_cache().  Gradients are synthetic: the subject is the copy, not the backward."""
import copy
import os

import pytest
import torch

from conftest import REPO, tt

pytestmark = pytest.mark.gpu

BF16, F16 = torch.bfloat16, torch.float16
LR = 1e-3
TINY = ["transforms.input_size=96", "model.image_encoder.tag=vit_test_patch16", "model.image_encoder.embedding_dim=128",
        "model.image_encoder.pretrained=False", "model.text_encoder.tag=bert-test", "model.text_encoder.embedding_dim=128",
        "model.text_encoder.pretrained=False"]
SCALERS = ["torch", "simseg_amd"]


def _clip(golden):
    """The tiny CLIPModel of tests/test_gpu_model.py (_build), golden weights."""
    from simseg.core.config import update_cfg
    from simseg.models import PIPELINE
    from simseg.tasks.clip.config import task_cfg_init_fn, update_clip_config
    from simseg.utils import build_from_cfg
    cfg = update_cfg(task_cfg_init_fn, os.path.join(REPO, "configs/clip/simseg.vit-s.yaml"), TINY, update_clip_config)
    model = build_from_cfg(cfg.model.name, cfg, PIPELINE)
    g = golden("clip_glue")
    missing, unexpected = model.load_state_dict({k[3:]: tt(g[k]) for k in g.files if k.startswith("sd.")}, strict=False)
    assert not unexpected and all("position_ids" in m for m in missing)
    return model.cuda().eval()


def _biased(m, seed):
    """Non-zero biases (the modules initialise them to zero; a write that scales a zero bias would change nothing)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("bias"):
                p.add_(torch.randn(p.shape, generator=g) * 0.02)
    return m


class Route:
    """One cached copy and a way to force its path.  make() builds the model under test, fresh(m) the reference module, run(m) evaluates and
    asserts that the route's path ran, wb(m) is the weight and bias whose copy the route caches."""

    def __init__(self, name, monkeypatch, golden):
        from simseg_amd import towers
        self.name, self.golden = name, golden
        self.adt = {"w16_bf16": BF16, "w16_fp16": F16, "cat": BF16, "w3": torch.float32, "wqs_bf16": BF16, "wqs_fp16": F16}[name]
        self.half = self.adt if self.adt != torch.float32 else F16          # the optimizer's copies: the route's type, else the reference's AMP type
        monkeypatch.setenv("SIMSEG_AMD_COMPUTE", {BF16: "bf16", F16: "fp16", torch.float32: "fp32"}[self.adt])
        monkeypatch.setattr(towers, "_QSCALED", True)
        if name == "w3":
            monkeypatch.setattr(towers, "_SPLIT_FP32", "1")
        if name.startswith("wqs"):
            self.qs_calls = [0]
            orig = towers._wt_qscaled

            def counting(*a, **k):
                self.qs_calls[0] += 1
                return orig(*a, **k)
            monkeypatch.setattr(towers, "_wt_qscaled", counting)
        g = torch.Generator().manual_seed(11)
        if name.startswith("w16"):
            gl = golden("clip_train_ws1")
            self.inp = {"image": tt(gl["r0.image"]).cuda(), "input_ids": tt(gl["r0.input_ids"]).cuda(),
                        "attention_mask": tt(gl["r0.attention_mask"]).cuda()}
        elif name == "cat":
            from oracle.simseg_ref import synthetic_text
            ids, mask = synthetic_text(4, 25, 1000, seed=1)
            self.inp = (ids.cuda(), mask.cuda())
        elif name == "w3":
            self.inp = torch.randn(64, 3, 64, 64, generator=g).cuda()              # 64 x 17 token rows: the split GEMMs take them
        else:
            self.inp = torch.randn(2, 3, 368, 368, generator=g).cuda()             # T = 23 * 23 + 1 = 530 >= ops.ATTN_QSCALED_MIN_T

    def _new(self):
        from simseg_amd.nn import Bert, ViT
        if self.name.startswith("w16"):
            return _clip(self.golden)
        if self.name == "cat":
            return _biased(Bert("bert-test"), 5).cuda().eval()
        return _biased(ViT("vit_test_patch16", 64 if self.name == "w3" else 368), 5).cuda().eval()

    def make(self):
        return self._new()

    def fresh(self, m):
        f = self._new()
        f.load_state_dict(m.state_dict())
        return f

    def params(self, m):
        """Parameter order of the optimizer.  CAT: reversed, so the optimizer's copies of query / key / value are NOT back to back and the
        evaluation keeps concatenating them (towers._wt_stacked) instead of reading them in place."""
        ps = list(m.parameters())
        return ps[::-1] if self.name == "cat" else ps

    def wb(self, m):
        if self.name.startswith("w16"):
            lin = m.image_encoder.model.model.blocks[0].attn.qkv
        elif self.name == "cat":
            lin = m.encoder.layer[0].attention.self.query
        elif self.name == "w3":
            lin = m.blocks[0].mlp.fc1
        else:
            lin = m.blocks[0].attn.qkv
        return lin.weight, lin.bias

    def run(self, m, opt=None):
        """Evaluate; assert the route's cached copy was used (and, W16, that it is the copy `opt` - when given - handed to the towers)."""
        from simseg_amd import towers
        w, b = self.wb(m)
        n_split, n_qs = towers.SPLIT_CALLS[0], getattr(self, "qs_calls", [0])[0]
        with torch.no_grad():
            if self.name.startswith("w16"):
                out = torch.cat([o.float().reshape(-1) for o in m(self.inp, embeddings="all")])
            elif self.name == "cat":
                out = m(*self.inp).last_hidden_state.float().reshape(-1)
            else:
                out = m(self.inp).float().reshape(-1)
        torch.cuda.synchronize()
        if self.name.startswith("w16"):
            w16 = towers.COPIES.get("w16", (w,), self.adt)              # (a hit: made from this parameter at its current version, in the route's dtype)
            assert w16 is not None and w16.dtype == self.adt
            if opt is not None and opt.half_dtype == self.adt:
                assert w16 is opt.state[w]["p16"]                                 # the towers read the optimizer's copy
        elif self.name == "cat":
            lay = m.encoder.layer[0].attention.self
            qkv = (lay.query.weight, lay.key.weight, lay.value.weight)
            parts, _ = towers.COPIES.get("cat", qkv, self.adt)
            assert all(p16 is not None and p16 is towers.COPIES.get("w16", (p,), self.adt) for p16, p in zip(parts, qkv))
        elif self.name == "w3":
            assert towers.SPLIT_CALLS[0] > n_split
            assert towers.COPIES.get("split", (w,)) is not None                   # (made from this parameter at its current version)
        else:
            assert self.qs_calls[0] == n_qs + len(m.blocks)                        # one folded projection per block
            assert towers.COPIES.get("qscaled", (w, b), self.adt) is not None     # (made from this weight and this bias as they are now)
        return out

    def compare(self, m, opt=None):
        """Evaluate the model under test and a fresh module of its weights; bit-identical (after checking the fresh route is deterministic)."""
        from simseg_amd import towers
        out = self.run(m, opt)
        f = self.fresh(m)
        n_wqs = towers.COPIES.count("qscaled")
        r1 = self.run(f)
        if self.name.startswith("wqs"):
            assert towers.COPIES.count("qscaled") > n_wqs                                      # the fresh module made its own folded copies
        r2 = self.run(f)
        assert torch.equal(r1, r2), "the fresh module's route is not deterministic"
        assert torch.isfinite(out).all(), f"{self.name}: non-finite output"
        diff = float((out - r1).abs().max())
        assert torch.equal(out, r1), f"{self.name}: the model under test differs from a fresh module of its weights by {diff:.3e}"
        if self.name.startswith("wqs"):
            self.anchor(f, r1)
        return out

    def anchor(self, f, got):
        """The comparator itself against the fp32 oracle (relative L2, the tolerances of tests/test_gpu_fullsize.py for this path)."""
        from oracle import simseg_ref as R
        ref = R.RefViT("vit_test_patch16", 368)
        ref.load_state_dict({k: v.cpu() for k, v in f.state_dict().items()})
        with torch.no_grad():
            want = ref.eval()(self.inp.cpu()).reshape(-1)
        rel = float((got.cpu() - want).norm() / want.norm())
        print(f"{self.name}: fresh module vs fp32 oracle, relative L2 {rel:.2e}")
        assert rel < (2e-2 if self.adt == BF16 else 4e-3), rel


@pytest.fixture(params=["w16_bf16", "w16_fp16", "cat", "w3", "wqs_bf16", "wqs_fp16"])
def route(request, monkeypatch, golden):
    return Route(request.param, monkeypatch, golden)


@pytest.fixture(params=["w16_fp16", "wqs_fp16"])
def amp_route(request, monkeypatch, golden):
    return Route(request.param, monkeypatch, golden)


def _grads(params, seed, scale=1.0, inf=False):
    g = torch.Generator().manual_seed(seed)
    for p in params:
        p.grad = (torch.randn(p.shape, generator=g) * scale).cuda()
    if inf:
        params[len(params) // 2].grad.view(-1)[0] = float("inf")


def _masters(m):
    return {n: p.detach().clone() for n, p in m.named_parameters()}


def _same_masters(m, before):
    return all(torch.equal(before[n], p.detach()) for n, p in m.named_parameters())


def _check_copies(opt):
    """The direct invariant after every optimizer call, taken or skipped: each 16-bit copy equals its master rounded."""
    torch.cuda.synchronize()
    for grp in opt.param_groups:
        for p in grp["params"]:
            assert torch.equal(opt.state[p]["p16"], p.detach().to(opt.half_dtype)), (tuple(p.shape), "16-bit copy != master")


def _poison(params, dtype):
    """NaN-filled memory, freed just before the step, so that a newly allocated, unwritten copy buffer holds NaNs or other stale bytes
    rather than bytes that happen to match (such as an earlier model's copies of the same weights).  The cache is emptied first; one block
    covers what a plan allocates (its fp32 moments m and v, then the copy buffer; above 10 MB, so a segment of its own), and a copy buffer
    under 1 MB, which comes from the small-block pool, gets a NaN block of its own byte size there."""
    n = sum(p.numel() for p in params)
    copy_bytes = n * torch.empty((), dtype=dtype).element_size()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    nan = [torch.full((max(8 * n + copy_bytes + (1 << 16), 12 << 20) * n // copy_bytes,), float("nan"), device="cuda", dtype=dtype)]
    if copy_bytes <= 1 << 20:
        nan.append(torch.full((n,), float("nan"), device="cuda", dtype=dtype))
    torch.cuda.synchronize()
    del nan


def _scaler(kind, init_scale):
    from simseg_amd.optim import GradScaler
    s = (torch.amp.GradScaler if kind == "torch" else GradScaler)("cuda", init_scale=init_scale, growth_interval=1000)
    s.scale(torch.zeros((), device="cuda"))              # (lazy init of the scale tensor)
    return s


def _plain_step(opt, params, seed):
    _grads(params, seed)
    opt.step()
    _check_copies(opt)


def _skipped_step(route, m, opt, params, kind):
    """(c) cell: caches filled, a GradScaler step that overflows as the first step of a new plan; masters and output unchanged, output
    equal to a fresh module's."""
    before_out = route.run(m)
    before = _masters(m)
    n0 = opt.steps_taken()
    sc = _scaler(kind, 2.0 ** 40)
    old = list(opt._plans.values())                       # (kept alive: a new plan cannot reuse their buffers)
    _grads(params, 21, scale=2.0 ** 40, inf=True)
    _poison(params, opt.half_dtype)                       # (last allocation before the step)
    sc.step(opt)
    sc.update()
    assert sc.get_scale() == 2.0 ** 39 and opt.steps_taken() == n0
    assert opt._plans and all(all(p is not o for o in old) for p in opt._plans.values())      # it was the first step of a new plan
    _check_copies(opt)
    assert _same_masters(m, before)
    out = route.compare(m, opt)
    assert torch.equal(out, before_out), "a skipped step changed the output"


# ---- (a) plain optimizer steps ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", ["bf16", "fp16"])
def test_plain_step(route, half):
    from simseg_amd.optim import AdamW
    m = route.make()
    params = route.params(m)
    opt = AdamW(params, lr=LR, half_dtype=BF16 if half == "bf16" else F16)
    before = route.run(m)
    _plain_step(opt, params, 1)
    after = route.compare(m, opt)
    assert not torch.equal(after, before), "the step was not seen"
    _plain_step(opt, params, 2)                           # a second step on the same plan
    assert not torch.equal(route.compare(m, opt), after)


# ---- (b) a taken step under a GradScaler ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", SCALERS)
def test_taken_scaled_step(amp_route, kind):
    from simseg_amd.optim import AdamW
    route = amp_route
    m = route.make()
    params = route.params(m)
    opt = AdamW(params, lr=LR, half_dtype=route.half)
    _plain_step(opt, params, 1)
    before = route.run(m, opt)
    sc = _scaler(kind, 1024.0)
    _grads(params, 3, scale=1024.0)
    sc.step(opt)
    sc.update()
    assert opt.steps_taken() == 2
    _check_copies(opt)
    assert not torch.equal(route.compare(m, opt), before), "the step was not seen"


# ---- (c) a skipped step as the first step of a new plan ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", SCALERS)
def test_skipped_first_step_new_optimizer(route, kind):
    from simseg_amd.optim import AdamW
    m = route.make()
    params = route.params(m)
    opt = AdamW(params, lr=LR, half_dtype=route.half)
    _skipped_step(route, m, opt, params, kind)
    _plain_step(opt, params, 4)                           # and the plan's next (taken) step is seen
    route.compare(m, opt)


@pytest.mark.parametrize("kind", SCALERS)
def test_skipped_first_step_after_optimizer_load(amp_route, kind):
    from simseg_amd.optim import AdamW
    route = amp_route
    m = route.make()
    params = route.params(m)
    opt = AdamW(params, lr=LR, half_dtype=route.half)
    _plain_step(opt, params, 1)
    ck_model, ck_opt = copy.deepcopy(m.state_dict()), copy.deepcopy(opt.state_dict())
    _plain_step(opt, params, 2)                           # the weights move on past the checkpoint
    moved = route.run(m, opt)
    m.load_state_dict(ck_model)
    opt.load_state_dict(ck_opt)
    assert not torch.equal(route.run(m), moved)
    _skipped_step(route, m, opt, params, kind)


@pytest.mark.parametrize("kind", SCALERS)
def test_skipped_first_step_after_set_param_streams(amp_route, kind):
    from simseg_amd.optim import AdamW
    route = amp_route
    m = route.make()
    params = route.params(m)
    opt = AdamW(params, lr=LR, half_dtype=route.half)
    _plain_step(opt, params, 1)
    side = torch.cuda.Stream()
    opt.set_param_streams({p: side for p in params})
    _skipped_step(route, m, opt, params, kind)


@pytest.mark.parametrize("kind", SCALERS)
def test_skipped_first_step_after_storage_move(amp_route, kind):
    from simseg_amd.optim import AdamW
    route = amp_route
    m = route.make()
    params = route.params(m)
    opt = AdamW(params, lr=LR, half_dtype=route.half)
    _plain_step(opt, params, 1)
    ptrs = [p.data_ptr() for p in params]
    keep = [p.data for p in params]                       # (the old storage stays allocated across the move: new addresses)
    m.cpu().cuda()
    del keep
    assert all(p.data_ptr() != a for p, a in zip(params, ptrs))
    _skipped_step(route, m, opt, params, kind)            # the step sees the moved storage and builds a new plan (optim.py _prepare)


# ---- (d) torch-side in-place writes ---------------------------------------------------------------------------------------------------
def test_inplace_writes(route):
    m = route.make()
    w, b = route.wb(m)
    g = torch.Generator().manual_seed(7)
    out = route.run(m)
    for t, op in ((w, "mul_"), (w, "copy_"), (b, "copy_"), (b, "mul_")):
        with torch.no_grad():
            if op == "mul_":
                t.mul_(1.5)
            else:
                t.copy_(t + (torch.randn(t.shape, generator=g) * 0.02).cuda())
        new = route.compare(m)
        assert not torch.equal(new, out), f"{op} on {tuple(t.shape)} was not seen"
        out = new


# ---- (e) model.load_state_dict ------------------------------------------------------------------------------------------------------
def test_model_load_state_dict(amp_route):
    from simseg_amd.optim import AdamW
    route = amp_route
    m = route.make()
    params = route.params(m)
    opt = AdamW(params, lr=LR, half_dtype=route.half)
    _plain_step(opt, params, 1)                           # the caches hold the optimizer's copies
    before = route.run(m, opt)
    g = torch.Generator().manual_seed(8)
    sd = {k: (v + (torch.randn(v.shape, generator=g) * 0.01).to(v.device) if v.is_floating_point() else v) for k, v in m.state_dict().items()}
    m.load_state_dict(sd)
    assert not torch.equal(route.compare(m), before), "load_state_dict was not seen"


# ---- (f) a write torch cannot see, then invalidate_weight_cache() ------------------------------------------------------------------------
def test_data_write_then_invalidate(route):
    from simseg_amd import towers
    m = route.make()
    w, b = route.wb(m)
    out = route.run(m)
    for t in (w, b):
        v0 = t._version
        t.data.mul_(1.5)                                  # (p.data has a version counter of its own: the parameter's does not move)
        assert t._version == v0
        towers.invalidate_weight_cache()
        new = route.compare(m)
        assert not torch.equal(new, out), f"the write to {tuple(t.shape)} was not seen"
        out = new
