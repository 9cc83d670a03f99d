"""Fused global-norm gradient clipping (AdamW.clip_grad_norm_ / grad_norm, GradScaler.clip_grad_norm_, Trainer with cfg.optim.grad_clip)
against float64 expectations computed from the same gradients.

One optimizer holds the smallest tensors at which each path of the norm pass (CHUNK = 65536 elements per block) can go wrong: 1 element;
3 (scalar tail only); 65536 (exactly one chunk); 65537 (a chunk plus a one-element chunk); 200003 (several chunks, odd tail); a gradient
that is the view buf[1:65540] of a larger buffer (4 bytes off 16-byte alignment: the unaligned branch); two parameters in a second bucket
(another eps: the partials of two buckets are combined); one parameter without a gradient.  Gradients are N(0,1) times a per-tensor scale
in {1e-3, 1, 30}.

Tolerances, derived and not measured: the fp32 sum inside a 65536-element chunk is a tree of depth <= 64 + 2 + 6 + 2 additions of
non-negative terms, in practice (log2 65536 + 4) * 2^-24 = 1.2e-6 relative, and the finish is in double: the norm is held to 1e-5
(margin ~8x).  The moments after one step from zero are (1 - beta) times one or two fp32 products of the gradient and the coefficient:
a few 2^-24 on top of the coefficient's own error (that of the norm) and of 1 - beta formed in fp32 (2.4e-7 for 0.9, 1.5e-6 for 0.98):
1e-5 for exp_avg, 2e-5 for exp_avg_sq, element by element."""
import math
import os

import pytest
import torch

from conftest import REPO, tt

pytestmark = pytest.mark.gpu

CHUNK = 65536
MAIN = [(1, 1.0), (3, 30.0), (CHUNK, 1e-3), (CHUNK + 1, 1.0), (200003, 30.0), (CHUNK + 3, 1e-3)]      # the last one gets the unaligned view
SECOND = [(70001, 1.0), (5, 30.0)]                                                                    # second bucket (another eps)
BETAS, LR = (0.9, 0.98), 1e-3


@pytest.fixture(scope="module")
def data():
    """Parameter values and gradients, drawn once (CPU generator), and the float64 reference norms; read-only for every test."""
    gen = torch.Generator().manual_seed(1234)
    ps = [torch.randn(n, generator=gen) * 0.05 for n, _ in MAIN + SECOND]
    gs = [torch.randn(n, generator=gen) * s for n, s in MAIN + SECOND]
    ps, gs = [p.cuda() for p in ps], [g.cuda() for g in gs]
    flat = torch.cat([g.double() for g in gs])
    return dict(p=ps, g=gs, norm2=float(torch.linalg.vector_norm(flat)), norminf=torch.cat(gs).abs().max())


def _make(data, half_dtype=torch.bfloat16, mult=1.0):
    """-> (optimizer, parameters with a gradient).  A fresh optimizer over clones of the shared values; gradients = shared * mult."""
    from simseg_amd.optim import AdamW
    params = [torch.nn.Parameter(p.clone()) for p in data["p"]]
    for k, (p, g) in enumerate(zip(params, data["g"])):
        if k == len(MAIN) - 1:
            buf = torch.zeros(g.numel() + 8, device="cuda")
            buf[1:1 + g.numel()] = g * mult
            p.grad = buf[1:1 + g.numel()]
            assert p.grad.data_ptr() % 16 == 4 and p.grad.is_contiguous()
        else:
            p.grad = g * mult
    idle = torch.nn.Parameter(torch.ones(7, device="cuda"))                 # grad is None: does not count, is not updated
    nm = len(MAIN)
    opt = AdamW([{"params": params[:nm] + [idle]}, {"params": params[nm:], "eps": 1e-5}], lr=LR, betas=BETAS, eps=1e-6, weight_decay=1e-2,
                half_dtype=half_dtype)
    return opt, params


def _moments(opt, params):
    """exp_avg / exp_avg_sq from the state dict, in parameter order (the idle parameter, index len(MAIN), has no state)."""
    st = opt.state_dict()["state"]
    idx = [i for i in range(len(params) + 1) if i != len(MAIN)]
    assert sorted(st) == idx
    return [st[i]["exp_avg"] for i in idx], [st[i]["exp_avg_sq"] for i in idx]


def _check_moments(opt, params, data, c, tag):
    m, v = _moments(opt, params)
    worst = [0.0, 0.0]
    for k, g in enumerate(data["g"]):
        cg = c * g.double()
        for j, (got, want, tol) in enumerate(((m[k], (1 - BETAS[0]) * cg, 1e-5), (v[k], (1 - BETAS[1]) * cg * cg, 2e-5))):
            rel = ((got.double().view(-1) - want).abs() / want.abs().clamp_min(1e-300)).max().item()
            worst[j] = max(worst[j], rel)
            assert rel <= tol, (tag, k, j, rel)
    print(f"{tag}: worst relative error exp_avg {worst[0]:.2e}, exp_avg_sq {worst[1]:.2e}")


def _rel(a, b):
    return abs(float(a) - b) / abs(b)


def test_norm_parity_and_determinism(data):
    opt, _ = _make(data)
    n2 = opt.grad_norm()
    assert n2.dim() == 0 and n2.dtype == torch.float32 and n2.is_cuda
    first = n2.clone()
    print(f"2-norm {float(n2):.8e} vs float64 {data['norm2']:.8e}: relative error {_rel(n2, data['norm2']):.2e}")
    assert _rel(n2, data["norm2"]) <= 1e-5
    assert torch.equal(opt.grad_norm().clone().view(torch.int32), first.view(torch.int32))            # bit-reproducible
    ninf = opt.grad_norm(math.inf).clone()
    assert torch.equal(ninf, data["norminf"])                                                        # bit-exact
    assert torch.equal(opt.grad_norm(float("inf")), ninf)
    # the clipping call returns the same number, and the same number twice
    a = opt.clip_grad_norm_(1.0).clone()
    b = opt.clip_grad_norm_(1.0).clone()
    assert torch.equal(a.view(torch.int32), first.view(torch.int32)) and torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(opt.clip_grad_norm_(1.0, norm_type=math.inf), data["norminf"])
    want = min(1.0, 1.0 / (float(data["norminf"]) + 1e-6))
    assert _rel(opt.clip_coef(), want) <= 1e-6
    with pytest.raises(NotImplementedError):
        opt.clip_grad_norm_(1.0, norm_type=1.0)


def test_clip_that_bites_moments_follow_the_clipped_gradients(data):
    opt, params = _make(data)
    max_norm = 0.1 * data["norm2"]
    c = max_norm / (data["norm2"] + 1e-6)
    before = [p.grad.clone() for p in params]
    norm = opt.clip_grad_norm_(max_norm)
    assert _rel(norm, data["norm2"]) <= 1e-5 and _rel(opt.clip_coef(), c) <= 1e-5
    opt.step()
    assert all(torch.equal(p.grad, g) for p, g in zip(params, before))          # p.grad itself stays unclipped
    _check_moments(opt, params, data, c, "clip bites")


def _same_state(o1, p1, o2, p2):
    for a, b in zip(p1, p2):
        assert torch.equal(a.detach(), b.detach())
        for k in ("m", "v", "p16"):
            assert torch.equal(o1.state[a][k], o2.state[b][k]), k


def test_clip_that_does_not_bite_is_the_unclipped_step_bit_for_bit(data):
    o1, p1 = _make(data)
    o2, p2 = _make(data)
    o1.clip_grad_norm_(10.0 * data["norm2"])
    assert float(o1.clip_coef()) == 1.0
    o1.step(); o2.step()
    _same_state(o1, p1, o2, p2)


def test_step_disarms_the_clip(data):
    from simseg_amd.optim import AdamW
    o1, p1 = _make(data)
    o1.clip_grad_norm_(0.1 * data["norm2"])
    o1.step()
    # a twin that starts from the state after the clipped step (values, moments, step counter) ...
    o2, p2 = _make(data)
    with torch.no_grad():
        for a, b in zip(p1, p2):
            b.copy_(a)
    o2.load_state_dict(o1.state_dict())
    assert isinstance(o2, AdamW) and o2.steps_taken() == 1
    # ... takes a plain step; the first optimizer takes a second step without a new clip call
    o1.step(); o2.step()
    _same_state(o1, p1, o2, p2)


@pytest.mark.parametrize("own_scaler", [True, False])
def test_amp_unscale_then_clip_then_update(data, own_scaler):
    from simseg_amd.optim import GradScaler, live_scale
    S = 2.0 ** 16
    opt, params = _make(data, half_dtype=torch.float16, mult=S)
    scaler = GradScaler("cuda", init_scale=S) if own_scaler else torch.amp.GradScaler("cuda", init_scale=S)
    scaler.scale(torch.zeros((), device="cuda"))                                # (lazy init of the scale tensor)
    max_norm = 0.1 * data["norm2"]
    c = max_norm / (data["norm2"] + 1e-6)
    norm = scaler.clip_grad_norm_(opt, max_norm) if own_scaler else opt.clip_grad_norm_(max_norm, loss_scale=live_scale(scaler))
    assert _rel(norm, data["norm2"]) <= 1e-5                                    # the UNSCALED norm
    scaler.step(opt)
    scaler.update()
    assert opt.steps_taken() == 1 and scaler.get_scale() == S
    assert opt.state[params[0]]["p16"].dtype == torch.float16
    _check_moments(opt, params, data, c, "fp16 AMP, clip bites")


def test_amp_nan_in_a_gradient_skips_the_step(data):
    from simseg_amd.optim import GradScaler
    S = 2.0 ** 16
    opt, params = _make(data, half_dtype=torch.float16, mult=S)
    params[4].grad[123457] = float("nan")
    scaler = GradScaler("cuda", init_scale=S)
    scaler.scale(torch.zeros((), device="cuda"))
    before = [p.detach().clone() for p in params]
    norm = scaler.clip_grad_norm_(opt, 0.1 * data["norm2"]).clone()
    assert not math.isfinite(float(norm))
    assert math.isnan(float(opt.grad_norm(math.inf)))                           # a maximum built on fmaxf would have dropped it
    scaler.step(opt)
    scaler.update()
    assert scaler.get_scale() == S / 2 and opt.steps_taken() == 0
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, params))
    with pytest.raises(RuntimeError, match="non-finite"):
        opt.clip_grad_norm_(1.0, error_if_nonfinite=True)


def test_materialize_scales_the_gradients_in_place(data):
    opt, params = _make(data)
    max_norm = 0.1 * data["norm2"]
    opt.clip_grad_norm_(max_norm, materialize=True)
    c_dev = float(opt.clip_coef())
    assert _rel(c_dev, max_norm / (data["norm2"] + 1e-6)) <= 1e-5
    for p, g in zip(params, data["g"]):
        want = c_dev * g.double()
        ulp = torch.ldexp(torch.ones_like(want), torch.frexp(want)[1] - 24)     # spacing of fp32 numbers at |want| (2^(e-24), frexp exponent e)
        assert ((p.grad.double() - want).abs() <= ulp).all()
    # the gradients are clipped already: the step that follows multiplies nothing in (moments = those of the materialised gradients)
    opt.step()
    _check_moments(opt, params, data, c_dev, "materialize")


# ---- Trainer ---------------------------------------------------------------------------------------------------------------
TINY = ["transforms.input_size=96", "model.image_encoder.tag=vit_test_patch16", "model.image_encoder.embedding_dim=128",
        "model.image_encoder.pretrained=False", "model.text_encoder.tag=bert-test", "model.text_encoder.embedding_dim=128",
        "model.text_encoder.pretrained=False", "epoch=1", "optim.lr.init=1e-3", "dist.fp16=True"]


def _build(golden, tmp_path, grad_clip):
    """The tiny model of the model tests; cfg.optim.grad_clip comes from a YAML (a dict-valued leaf: YAML replaces it wholesale)."""
    import yaml
    from simseg.core.config import update_cfg
    from simseg.models import PIPELINE
    from simseg.tasks.clip.config import task_cfg_init_fn, update_clip_config
    from simseg.utils import build_from_cfg
    with open(os.path.join(REPO, "configs/clip/simseg.vit-s.yaml")) as f:
        y = yaml.load(f, Loader=yaml.FullLoader)
    y.setdefault("optim", {})["grad_clip"] = dict(grad_clip)
    path = tmp_path / "clip.yaml"
    with open(path, "w") as f:
        yaml.safe_dump(y, f)
    cfg = update_cfg(task_cfg_init_fn, str(path), TINY, update_clip_config)
    model = build_from_cfg(cfg.model.name, cfg, PIPELINE)
    g = golden("clip_glue")
    model.load_state_dict({k[3:]: tt(g[k]) for k in g.files if k.startswith("sd.")}, strict=False)
    return model.cuda().eval()                      # (eval: no dropout, so that two runs see the same gradients)


class _Coef64:
    """torch.nn.utils.clip_grad_norm_ (2-norm) with the coefficient computed in float64 - the norm accumulated and the division done in
    double - instead of float32; the same in-place scaling of the same gradients."""

    def __call__(self, parameters, max_norm, **_):
        grads = [p.grad for p in parameters]
        total = torch.linalg.vector_norm(torch.cat([g.double().view(-1) for g in grads]))
        coef = torch.clamp(max_norm / (total + 1e-6), max=1.0)
        for g in grads:
            g.mul_(coef)
        return total.float()


@pytest.mark.parametrize("amp", ["bf16", "fp16"])
def test_trainer_fused_route_matches_the_torch_route(golden, tmp_path, monkeypatch, amp):
    from simseg_amd import trainer as T
    g = golden("clip_train_ws1")
    batch = {"image": tt(g["r0.image"]).cuda(), "input_ids": tt(g["r0.input_ids"]).cuda(), "attention_mask": tt(g["r0.attention_mask"]).cuda()}
    fp16 = amp == "fp16"
    S = 2.0 ** 16

    def trainer(grad_clip):
        m = _build(golden, tmp_path, grad_clip)
        tr = T.Trainer(m, m.cfg, steps_per_epoch=40, amp_dtype=amp)
        assert tr.scaler.is_enabled() == fp16
        if fp16:
            tr.scaler = T.GradScaler("cuda", init_scale=S)
        return m, tr

    # dry run: the gradient norm of this batch, without a step (under fp16 AMP the gradients carry the loss scale)
    m, tr = trainer({})
    with torch.autocast("cuda", dtype=tr.amp_dtype):
        loss = sum(m(batch)[0].values())
    tr.scaler.scale(loss).backward()
    dry = float(tr.optimizer.grad_norm()) / (S if fp16 else 1.0)
    assert math.isfinite(dry) and dry > 0
    out = tr.train_step(batch)
    assert "grad_norm" not in out                                               # grad_clip empty: the step is as it was
    max_norm = 0.5 * dry
    c = max_norm / (dry + 1e-6)

    def run(fused, clip_fn=None):
        monkeypatch.setattr(T, "FUSED_CLIP", fused)
        if clip_fn is not None:
            monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", clip_fn)
        m, tr = trainer({"max_norm": max_norm})
        out = tr.train_step(batch)
        monkeypatch.undo()
        assert tr.optimizer.steps_taken() == 1
        return m, tr, out

    m_f, tr_f, out_f = run(True)
    m_t, tr_t, out_t = run(False)
    m_64, _, _ = run(False, _Coef64())
    for out in (out_f, out_t):
        assert out["grad_norm"].is_cuda and out["grad_norm"].dim() == 0
        assert math.isfinite(float(out["grad_norm"])) and abs(float(out["grad_norm"]) - dry) <= 1e-3 * dry      # both routes: the UNSCALED norm
    # the two routes differ in the rounding of one scalar (the coefficient): allow 4x what rounding it in float32 instead of float64 does
    noise = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(m_t.parameters(), m_64.parameters()))
    diff = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(m_f.parameters(), m_t.parameters()))
    print(f"{amp}: max |parameter difference| fused vs torch route {diff:.3e}; torch route float32 vs float64 coefficient {noise:.3e} (bound 4x)")
    assert diff <= 4 * noise
    # the update is the clipped one in the reference's order (unscale, clip): |exp_avg| = (1 - beta1) c |g|.  (Clipping the SCALED
    # gradients, as the trainer once did, makes it ~2^-16 of that under fp16 AMP.)
    b1 = float(tr_f.optimizer.param_groups[0]["betas"][0])
    for tr in (tr_f, tr_t):
        got = math.sqrt(sum(float(st["m"].double().pow(2).sum()) for st in tr.optimizer.state.values() if "m" in st))
        assert abs(got - (1 - b1) * c * dry) <= 1e-3 * (1 - b1) * c * dry, (amp, got, (1 - b1) * c * dry)
