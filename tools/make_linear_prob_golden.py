"""Capture the linear-probe fixtures by running the REFERENCE itself on the CPU (imported at run time the way oracle/make_golden.py does
it; its stub helpers are imported from there).  TEST INFRASTRUCTURE - runs only where the reference checkout is present, never imported
by the product, and nothing of the reference's program text is written: the fixtures hold settings and recorded numbers only.

    python tools/make_linear_prob_golden.py

  tests/golden/linear_prob_config.json   update_cfg(task_cfg_init_fn, configs/linear_prob/imagenet.yaml, argv, update_clip_config) of the
                                         reference: plain and with two sets of argv overrides, plus the error an unknown key raises
  tests/golden/linear_prob_head.npz      small tensors through the reference's nn.CrossEntropyLoss + accuracy(topk=(1, 5)) (loss, logit
                                         gradient, accuracies) and through three LARS.step()s per case (parameters and momentum buffers
                                         after every step): momentum 0.9; weight decay 0 and 1e-4; Nesterov off and on; dampening 0.1;
                                         one lars_exclude group
"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
from oracle.make_golden import GOLD, REF, _import_reference, _np  # noqa: E402

CONFIG_CASES = {
    "plain": [],
    "argv-batch": ["data.batch_size=4096", "optim.lr.init=1.6"],
    "argv-model": ["model.classifier.num_classes=100", "model.image_encoder.tag=vit_small_patch16_224_in21k"],
}

# name -> (optimizer keywords, [(group keywords, [tensor shapes])])
LARS_CASES = {
    "m9": (dict(lr=0.5, momentum=0.9, weight_decay=0.0), [({}, [(12, 40), (12,)])]),
    "m9_wd_nesterov": (dict(lr=0.5, momentum=0.9, weight_decay=1e-4, nesterov=True), [({}, [(12, 40), (1000,)])]),
    "m9_wd_damp_exclude": (dict(lr=0.25, momentum=0.9, weight_decay=1e-4, dampening=0.1, eta=0.002),
                           [({}, [(12, 40)]), (dict(lars_exclude=True, lr=0.01), [(12,), (65,)])]),
}
STEPS = 3


def gold_config():
    from simseg.core.config import update_cfg
    from simseg.tasks.linear_prob.config import task_cfg_init_fn, update_clip_config
    import simseg.core.config as rc

    def plain(d):
        return {k: plain(v) if isinstance(v, dict) else (list(v) if isinstance(v, tuple) else v) for k, v in d.items()}

    yaml_path = os.path.join(REF, "configs/linear_prob/imagenet.yaml")
    out = {}
    for name, argv in CONFIG_CASES.items():
        rc.cfg.set_this_dict_immutable(False)
        out[name] = dict(argv=argv, cfg=plain(update_cfg(task_cfg_init_fn, yaml_path, argv, update_clip_config)))
    errs = {}
    for name, argv in {"unknown_key": ["model.nope=1"]}.items():
        rc.cfg.set_this_dict_immutable(False)
        try:
            update_cfg(task_cfg_init_fn, yaml_path, argv, update_clip_config)
            errs[name] = None
        except Exception as e:   # noqa: BLE001
            errs[name] = type(e).__name__
    out["errors"] = errs
    os.makedirs(GOLD, exist_ok=True)
    with open(os.path.join(GOLD, "linear_prob_config.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote linear_prob_config.json", errs)


def gold_head():
    from simseg.core.optimizer.lars import LARS
    from simseg.tasks.linear_prob.hooks.utils import accuracy
    out = {}
    g = torch.Generator().manual_seed(17)
    for tag, (B, C) in {"ce_a": (8, 10), "ce_b": (5, 37)}.items():
        logits = (torch.randn(B, C, generator=g) * 3.0).requires_grad_(True)
        labels = torch.randint(0, C, (B,), generator=g)
        labels[0], labels[1] = 0, C - 1
        loss = torch.nn.CrossEntropyLoss(reduction="mean")(logits, labels)
        loss.backward()
        acc1, acc5 = accuracy(logits, labels, topk=(1, 5))
        out.update({f"{tag}.logits": _np(logits), f"{tag}.labels": _np(labels), f"{tag}.loss": _np(loss), f"{tag}.dlogits": _np(logits.grad),
                    f"{tag}.acc1": _np(acc1), f"{tag}.acc5": _np(acc5)})
    meta = {}
    for name, (kw, groups) in LARS_CASES.items():
        params, pg = [], []
        for gkw, shapes in groups:
            ps = [torch.nn.Parameter(torch.randn(*s, generator=g) * 0.3) for s in shapes]
            params += ps
            pg.append(dict(params=ps, **gkw))
        opt = LARS(pg, **kw)
        for i, p in enumerate(params):
            out[f"{name}.p0.{i}"] = _np(p).copy()
        for s in range(1, STEPS + 1):
            for i, p in enumerate(params):
                p.grad = torch.randn(p.shape, generator=g) * 0.05
                out[f"{name}.g{s}.{i}"] = _np(p.grad).copy()
            opt.step()
            for i, p in enumerate(params):
                out[f"{name}.p{s}.{i}"] = _np(p).copy()
                out[f"{name}.buf{s}.{i}"] = _np(opt.state[p]["momentum_buffer"]).copy()
        meta[name] = dict(kw=kw, eps=opt.eps, groups=[dict(kw=gkw, shapes=[list(s) for s in shapes]) for gkw, shapes in groups])
    out["lars_meta"] = np.array(json.dumps(meta, sort_keys=True))
    os.makedirs(GOLD, exist_ok=True)
    path = os.path.join(GOLD, "linear_prob_head.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    torch.set_num_threads(4)
    _import_reference()
    gold_config()
    gold_head()
