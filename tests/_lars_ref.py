"""Float64 numpy restatement of the LARS law (DESIGN.md "Linear probe") shared by the CPU and GPU linear-probe tests, the deviation
measure both use, and the tolerance fixed from the reference's own fp32 result.  Not a test module."""
import json

import numpy as np

# 4 x the largest relative deviation (rel_dev below) of the reference's own fp32 LARS trajectories in tests/golden/linear_prob_head.npz
# (parameters and momentum buffers after each of three steps, every case) from the float64 restatement on the same inputs:
# measured 1.986e-07 (tests/test_linear_probe_host.py::test_float64_restatement_reproduces_the_golden prints it and checks this constant).
LARS_TOL = 4 * 1.986e-07


def rel_dev(got, want64):
    """max |got - want| / max |want| over one array (normwise: an element near zero does not blow the measure up)."""
    want64 = np.asarray(want64, dtype=np.float64)
    scale = np.abs(want64).max()
    err = np.abs(np.asarray(got, dtype=np.float64) - want64).max()
    return float(err / scale) if scale > 0 else float(err)


def lars_step64(p, g, buf, *, lr, momentum=0.0, weight_decay=0.0, dampening=0.0, eta=0.001, nesterov=False, eps=1e-8, exclude=False):
    """One LARS step of one tensor in float64: (p, g, buf or None) -> (p, buf or None, local_lr)."""
    p, g = np.asarray(p, dtype=np.float64), np.asarray(g, dtype=np.float64)
    local = 1.0
    if not exclude:
        wn, gn = float(np.sqrt((p * p).sum())), float(np.sqrt((g * g).sum()))
        if wn != 0 and gn != 0:
            local = eta * wn / (gn + weight_decay * wn + eps)
    d = (g + weight_decay * p) * (local * lr)
    if momentum != 0:
        buf = d.copy() if buf is None else momentum * np.asarray(buf, dtype=np.float64) + (1 - dampening) * d
        d = d + momentum * buf if nesterov else buf
    return p - d, buf, local


def golden_cases(npz):
    """tests/golden/linear_prob_head.npz -> {case: (per-tensor keyword dicts for lars_step64, p0 list, [g lists per step], [p lists], [buf lists])}."""
    meta = json.loads(str(npz["lars_meta"]))
    out = {}
    for name, m in meta.items():
        kws = []
        for grp in m["groups"]:
            for _ in grp["shapes"]:
                kw = dict(m["kw"])
                kw.update({k: v for k, v in grp["kw"].items() if k != "lars_exclude"})
                kw["exclude"] = bool(grp["kw"].get("lars_exclude", False))
                kw["eps"] = m["eps"]
                kws.append(kw)
        n = len(kws)
        steps = 1
        while f"{name}.g{steps + 1}.0" in npz.files:
            steps += 1
        out[name] = dict(meta=m, kws=kws, p0=[npz[f"{name}.p0.{i}"] for i in range(n)],
                         g=[[npz[f"{name}.g{s}.{i}"] for i in range(n)] for s in range(1, steps + 1)],
                         p=[[npz[f"{name}.p{s}.{i}"] for i in range(n)] for s in range(1, steps + 1)],
                         buf=[[npz[f"{name}.buf{s}.{i}"] for i in range(n)] for s in range(1, steps + 1)])
    return out


def trajectory64(kws, p0, grads):
    """The float64 trajectory of a case: ([p lists per step], [buf lists per step], [local lr lists per step])."""
    p = [np.asarray(a, dtype=np.float64) for a in p0]
    buf = [None] * len(p)
    ps, bufs, lls = [], [], []
    for gs in grads:
        ll = []
        for i, g in enumerate(gs):
            p[i], buf[i], l = lars_step64(p[i], g, buf[i], **kws[i])
            ll.append(l)
        ps.append([a.copy() for a in p])
        bufs.append([None if b is None else b.copy() for b in buf])
        lls.append(ll)
    return ps, bufs, lls
