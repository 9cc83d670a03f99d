"""Float64 statement of the SigLIP row kernel, written from the formulas of include/simseg_hip.h (simseg_siglip_rows) in closed form - no
autograd, no code shared with the device path -, the torch statement of the loss the tests differentiate, and the (T, b) settings the
host and the GPU tests share.  siglip_eval takes a dtype and a device: in float64 on the CPU it is the reference, in fp32 on the device
the yardstick of tests/test_gpu_loss_head.py.  The similarity blocks and embeddings are the tables of tests/_contrastive_ref.py."""
import numpy as np
import torch
import torch.nn.functional as F

from _contrastive_ref import SHAPES, acc32, sim_blocks

T_LO, T_HI = float(np.float32(0.001)), 0.5          # the kernel's clamp constants are fp32 numbers: 0.001f is not 1e-3
# (T, b): the paper's init (t = 10, b = -10); a sharp trained state; clamped above; clamped below
SETTINGS = [(0.1, -10.0), (0.02, -10.0), (0.7, -3.0), (5e-4, 0.0)]
ROW_SHAPES = SHAPES + [(1, 1, 0)]


def blocks(family, N1, N2, target0):
    """[2, N1, N2] of the shared tables; (1, 1, 0) - one pair, the positive - is not in them.  Its values are small enough that at
    T = 1e-3 (the lower clamp) exp(-|z|) stays a normal fp32 number: dLoss/db of the lone pair is then not 0 under any setting."""
    if (N1, N2) == (1, 1):
        return torch.tensor([[[-0.0625]], [[-0.03125]]]) if family == "random" else torch.tensor([[[0.0625]], [[0.03125]]])
    return sim_blocks(family, N1, N2, target0)


def _scalars(T, b, dtype, device):
    T = torch.as_tensor(T, dtype=torch.float32).to(device=device, dtype=dtype).reshape(())          # fp32 values: what the kernel reads
    b = torch.as_tensor(b, dtype=torch.float32).to(device=device, dtype=dtype).reshape(())
    return T, b


def siglip_eval(s, T, b, target0, dtype=torch.float64, device="cpu"):
    """One [N1, N2] block.  T: the temperature before the clamp, b: the bias.  -> dict(rows, total, ds, dt, db, acc)"""
    s = s.to(device=device, dtype=dtype)
    N1, N2 = s.shape
    T, b = _scalars(T, b, dtype, device)
    temp = torch.clamp(T, T_LO, T_HI)
    inv_t = 1 / temp
    z = s * inv_t + b
    pos = torch.arange(N2, device=device)[None, :] == (target0 + torch.arange(N1, device=device))[:, None]
    y = torch.where(pos, torch.ones_like(z), -torch.ones_like(z))
    x = -y * z
    e = torch.exp(-x.abs())
    lij = torch.clamp(x, min=0) + torch.log1p(e)
    rows = lij.sum(1)
    sig = torch.where(x >= 0, 1 / (1 + e), e / (1 + e))
    dz = -y * sig / N1
    inside = T_LO <= float(T) <= T_HI                             # the kernel's test on the fp32 temperature
    dt = -(dz * s).sum() / (temp * temp) if inside else torch.zeros((), device=device, dtype=dtype)
    return {"rows": rows, "total": rows.sum() / N1, "ds": dz * inv_t, "dt": dt, "db": dz.sum(), "acc": acc32(s, target0)}


def siglip_torch(s, T, b, target0):
    """The loss as one writes it in torch, in s's dtype on s's device (autograd flows to whatever requires it):
    -F.logsigmoid(y * (s / clamp(T) + b)).sum() / N1."""
    N1, N2 = s.shape
    pos = torch.arange(N2, device=s.device)[None, :] == (target0 + torch.arange(N1, device=s.device))[:, None]
    y = torch.where(pos, 1.0, -1.0).to(s.dtype)
    return -F.logsigmoid(y * (s / torch.clamp(T, T_LO, T_HI) + b)).sum() / N1
