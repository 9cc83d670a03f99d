"""Host-side contract of the linear-probe task: its config against the golden captured from the reference, the pipeline's state-dict
surface, the LARS constructor / checkpoints, the C ABI's new symbols, the lr schedule of the shipped recipe, and the float64 restatement
of the LARS law against the reference's own fp32 result.  CPU only."""
import json
import os

import numpy as np
import pytest
import torch

from _lars_ref import LARS_TOL, golden_cases, rel_dev, trajectory64
from conftest import GOLD, REPO

YAML = os.path.join(REPO, "configs/linear_prob/imagenet.yaml")
NEW = ["simseg_ce_rows", "simseg_lars_norm_partials", "simseg_lars_finish", "simseg_lars_multi_step"]
TINY = ["transforms.input_size=96", "model.image_encoder.tag=vit_test_patch16", "model.image_encoder.embedding_dim=128",
        "model.classifier.num_classes=10"]


def _cfg(argv=()):
    from simseg.core.config import update_cfg
    from simseg.tasks.linear_prob.config import task_cfg_init_fn, update_clip_config
    return update_cfg(task_cfg_init_fn, YAML, list(argv), update_clip_config)


def _plain(d):
    return {k: _plain(v) if isinstance(v, dict) else (list(v) if isinstance(v, tuple) else v) for k, v in d.items()}


GOLDEN_CFG = json.load(open(os.path.join(GOLD, "linear_prob_config.json")))


@pytest.mark.parametrize("case", [k for k in GOLDEN_CFG if k != "errors"])
def test_config_matches_the_reference(case):
    want = GOLDEN_CFG[case]
    assert _plain(_cfg(want["argv"])) == want["cfg"]


def test_unknown_key_still_raises():
    assert GOLDEN_CFG["errors"] == {"unknown_key": "ValueError"}
    with pytest.raises(ValueError, match="Undefined attribute"):
        _cfg(["model.nope=1"])
    import yaml
    doc = yaml.safe_load(open(YAML))
    doc["model"]["nope"] = 1
    import tempfile
    with tempfile.NamedTemporaryFile("w", suffix=".yaml") as f:
        yaml.safe_dump(doc, f)
        f.flush()
        from simseg.core.config import update_cfg
        from simseg.tasks.linear_prob.config import task_cfg_init_fn, update_clip_config
        with pytest.raises(KeyError, match="Non-existent config key: model.nope"):
            update_cfg(task_cfg_init_fn, f.name, [], update_clip_config)


def test_pipeline_builds_on_the_cpu_with_the_documented_keys():
    from simseg.models import PIPELINE
    from simseg.utils import build_from_cfg
    cfg = _cfg(TINY)
    assert cfg.optim.name == "LARS" and cfg.model.name == "linear_prob"
    model = build_from_cfg(cfg.model.name, cfg, PIPELINE)
    keys = list(model.state_dict())
    assert "classifier.weight" in keys and "classifier.bias" in keys
    rest = [k for k in keys if not k.startswith("classifier.")]
    assert rest and all(k.startswith("image_encoder.model.model.") for k in rest)
    assert model.classifier.weight.shape == (10, 128)
    # the same image tower and key layout as the clip pipeline: a SimSeg checkpoint's image_encoder.* entries load
    g = np.load(os.path.join(GOLD, "clip_glue.npz"))
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd.image_encoder.")}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and sorted(missing) == ["classifier.bias", "classifier.weight"]
    # trainable: False -> nothing of the encoder asks for a gradient, and train() leaves it in eval mode
    assert not any(p.requires_grad for p in model.image_encoder.parameters())
    assert all(p.requires_grad for p in model.classifier.parameters())
    model.train()
    assert model.training and not model.image_encoder.training
    import simseg.models.pipelines.linear_prob as LP
    assert "no loss scaling" in " ".join(LP.__doc__.split())


def test_lars_constructor_errors():
    from simseg.core.optimizer import LARS
    p = [torch.nn.Parameter(torch.zeros(3))]
    for kw, msg in [(dict(lr=-1.0), "Invalid learning rate"), (dict(lr=0.1, momentum=-0.5), "Invalid momentum value"),
                    (dict(lr=0.1, weight_decay=-1e-4), "Invalid weight_decay value"), (dict(lr=0.1, eta=-1e-3), "Invalid LARS coefficient value"),
                    (dict(lr=0.1, nesterov=True), "Nesterov momentum requires a momentum and zero dampening"),
                    (dict(lr=0.1, nesterov=True, momentum=0.9, dampening=0.1), "Nesterov momentum requires")]:
        with pytest.raises(ValueError, match=msg):
            LARS(p, **kw)
    opt = LARS(p, lr=0.1)
    assert opt.defaults == dict(lr=0.1, momentum=0, dampening=0, weight_decay=0, nesterov=False, eta=0.001) and opt.eps == 1e-8


class _TorchLARS(torch.optim.Optimizer):
    """Torch-side restatement of the law (same defaults, group keys and state key), for checkpoint exchange."""

    def __init__(self, params, lr, momentum=0, weight_decay=0, dampening=0, eta=0.001, nesterov=False, eps=1e-8):
        self.eps = eps
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, eta=eta))

    @torch.no_grad()
    def step(self):
        for g in self.param_groups:
            for p in g["params"]:
                if p.grad is None:
                    continue
                local = 1.0
                if not g.get("lars_exclude", False):
                    wn, gn = p.norm().item(), p.grad.norm().item()
                    if wn != 0 and gn != 0:
                        local = g["eta"] * wn / (gn + g["weight_decay"] * wn + self.eps)
                d = (p.grad + g["weight_decay"] * p) * (local * g["lr"])
                if g["momentum"] != 0:
                    st = self.state[p]
                    if "momentum_buffer" not in st:
                        st["momentum_buffer"] = d.clone()
                    else:
                        st["momentum_buffer"].mul_(g["momentum"]).add_(d, alpha=1 - g["dampening"])
                    d = d + g["momentum"] * st["momentum_buffer"] if g["nesterov"] else st["momentum_buffer"]
                p.sub_(d)


def test_lars_state_dicts_round_trip_and_load_into_a_torch_restatement():
    from simseg.core.optimizer import LARS
    gen = torch.Generator().manual_seed(3)
    ps = [torch.nn.Parameter(torch.randn(4, 5, generator=gen)), torch.nn.Parameter(torch.randn(5, generator=gen))]
    groups = lambda q: [dict(params=[q[0]]), dict(params=[q[1]], lars_exclude=True, lr=0.01)]      # noqa: E731
    ref = _TorchLARS(groups(ps), lr=0.5, momentum=0.9, weight_decay=1e-4)
    for _ in range(2):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=gen)
        ref.step()
    sd = ref.state_dict()
    ours = LARS(groups(ps), lr=0.1)
    ours.load_state_dict(sd)                                     # torch -> ours
    back = ours.state_dict()                                     # ours -> the layout torch loads
    assert set(back) == {"state", "param_groups"} and set(back["state"]) == {0, 1}
    for i in (0, 1):
        assert set(back["state"][i]) == {"momentum_buffer"}
        assert torch.equal(back["state"][i]["momentum_buffer"], sd["state"][i]["momentum_buffer"])
    assert back["param_groups"] == sd["param_groups"] and back["param_groups"][1]["lars_exclude"] is True
    again = _TorchLARS(groups(ps), lr=0.1)
    again.load_state_dict(back)
    assert torch.equal(again.state[ps[0]]["momentum_buffer"], ref.state[ps[0]]["momentum_buffer"])
    assert again.param_groups[0]["momentum"] == 0.9 and again.param_groups[0]["lr"] == 0.5
    # before the first step there is no momentum buffer, as in the reference
    assert LARS(groups(ps), lr=0.1, momentum=0.9).state_dict()["state"] == {}


def test_header_declares_the_new_symbols():
    from simseg_amd import lib
    decl = lib.parse_header()
    for name in NEW:
        assert name in decl, name
    assert [n for _, n in decl["simseg_ce_rows"][1]] == ["logits", "dt", "labels", "loss_rows", "ranks", "dlogits", "out3", "B", "C", "gscale",
                                                         "write_grad", "stream"]
    tables = ["table", "sizes", "chunk_tid", "chunk_off", "sizes_host", "chunk_tid_host", "chunk_off_host", "n_tensors", "n_chunks", "chunk"]
    assert [n for _, n in decl["simseg_lars_norm_partials"][1]] == tables + ["partials", "stream"]
    assert [n for _, n in decl["simseg_lars_multi_step"][1]] == tables + ["local_lr", "momentum", "dampening", "nesterov", "stream"]
    assert [n for _, n in decl["simseg_lars_finish"][1]] == ["table", "tensor_first", "tensor_first_host", "partials", "n_tensors", "n_chunks",
                                                             "eta", "eps", "local_lr", "stream"]
    from simseg_amd import ops, probe
    assert callable(ops.ce_rows) and callable(ops.lars_norm_partials) and callable(ops.lars_finish) and callable(ops.lars_multi_step)
    assert "no loss scaling" in " ".join(probe.__doc__.split())


def test_lr_schedule_of_the_shipped_recipe():
    from simseg_amd.probe import LinearProbeTrainer
    from simseg_amd.trainer import lr_multiplier
    cfg = _cfg()
    steps_per_epoch = 78                                          # 1 281 167 images at batch 16384
    total = steps_per_epoch * cfg.epoch
    warm = int(total * cfg.optim.lr.warmup_proportion)
    assert (cfg.optim.lr.init, cfg.optim.lr.name, cfg.epoch, warm) == (6.4, "cosine_schedule_with_warmup", 90, 779)
    sched = dict(name=cfg.optim.lr.name, num_warmup_steps=warm, num_training_steps=total, **dict(cfg.optim.lr.param))
    lr = lambda s: cfg.optim.lr.init * lr_multiplier(step=s, **sched)      # noqa: E731
    assert lr(0) == 0.0
    assert lr(warm) == 6.4
    assert lr(warm - 1) == pytest.approx(6.4 * (warm - 1) / warm, rel=1e-12)
    last = total - 1
    want = 6.4 * 0.5 * (1.0 + np.cos(np.pi * (last - warm) / (total - warm)))
    assert lr(last) == pytest.approx(want, rel=1e-9) and 0 < lr(last) < 1e-5
    # the trainer derives the same schedule from the config (no device needed to build it around a CPU parameter)
    model = torch.nn.Linear(4, 3)
    t = LinearProbeTrainer.__new__(LinearProbeTrainer)
    t.model, t.cfg = model, cfg
    t.optimizer = torch.optim.SGD(model.parameters(), lr=cfg.optim.lr.init)
    t.base_lrs = [cfg.optim.lr.init]
    t.sched = sched
    assert t.set_lrs(warm) == [6.4] and t.optimizer.param_groups[0]["lr"] == 6.4


def test_float64_restatement_reproduces_the_golden():
    """The golden trajectories are the reference's fp32 arithmetic; the restatement runs in float64 from the same inputs.  Largest
    relative deviation (max |a - b| / max |b| per tensor; parameters and momentum buffers after each of three steps, every case):
    1.986e-07, so the gate is 4 x that = 7.944e-07 (_lars_ref.LARS_TOL).  The reference alone passes its own gate."""
    cases = golden_cases(np.load(os.path.join(GOLD, "linear_prob_head.npz")))
    assert set(cases) == {"m9", "m9_wd_nesterov", "m9_wd_damp_exclude"}
    worst = 0.0
    for name, c in cases.items():
        ps, bufs, lls = trajectory64(c["kws"], c["p0"], c["g"])
        assert len(ps) == 3
        for s in range(3):
            for i in range(len(c["kws"])):
                worst = max(worst, rel_dev(c["p"][s][i], ps[s][i]), rel_dev(c["buf"][s][i], bufs[s][i]))
            assert all(l == 1.0 for l, kw in zip(lls[s], c["kws"]) if kw["exclude"])
    print(f"largest relative deviation of the reference's fp32 LARS from the float64 restatement: {worst:.4e}; gate {LARS_TOL:.4e}")
    assert worst <= LARS_TOL                                     # the reference passes its own gate
    assert abs(LARS_TOL - 4 * worst) <= 1e-3 * LARS_TOL          # and the fixed constant is 4 x what is measured here
