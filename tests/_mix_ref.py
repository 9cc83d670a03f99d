"""float64 / exact restatements shared by tests/test_mixup_host.py and tests/test_gpu_mixup.py.  Nothing here imports simseg_amd: these
are the statements the package's own host statements (simseg_amd.mixup.mix_ref, soft_target_ref) and its kernels are checked against."""
import numpy as np
import torch

INT_MAX = 2 ** 31 - 1


def dense_target64(a, b, lam, eps, C):
    """timm's mixup_target in float64: y1 * lam + y2 * (1 - lam), with y1 / y2 the one-hot rows of a / b at on = 1 - eps + eps / C and
    off = eps / C.  a, b: int64 [B] (valid labels), lam: [B]."""
    a, b = torch.as_tensor(a).long(), torch.as_tensor(b).long()
    lam = torch.as_tensor(np.asarray(lam, dtype=np.float64))[:, None]
    off = eps / C
    on = 1.0 - eps + off
    y1 = torch.full((a.shape[0], C), off, dtype=torch.float64).scatter_(1, a[:, None], on)
    y2 = torch.full((a.shape[0], C), off, dtype=torch.float64).scatter_(1, b[:, None], on)
    return y1 * lam + y2 * (1.0 - lam)


def soft_ce64(x64, t64):
    """-> (loss rows, d(mean loss)/dx) of -sum_c t_c log softmax(x)_c in float64."""
    logp = torch.log_softmax(x64, dim=1)
    return -(t64 * logp).sum(1), (torch.softmax(x64, dim=1) - t64) / x64.shape[0]


def ranks64(x64, y):
    """How many classes rank ahead of the label's: strictly larger, or equal with a smaller class id."""
    xy = x64.gather(1, y[:, None])
    cols = torch.arange(x64.shape[1])[None, :]
    return ((x64 > xy) | ((x64 == xy) & (cols < y[:, None]))).sum(1)


def mix_exact(x, table):
    """The law of the mix in numpy, element by element in IEEE arithmetic, from the ORIGINAL values: x fp32 numpy [B, C, H, W] (16-bit
    batches are passed widened, the caller rounds the result once), table int32 [B, 8] -> fp32 numpy.  kind 1 is
    fl32(fl32(lam * x_i) + fl32(om * x_j)) - numpy float32 scalars multiply and add with one rounding each."""
    x = np.asarray(x, dtype=np.float32)
    out = x.copy()
    B = x.shape[0]
    fl = np.ascontiguousarray(table[:, 5:7]).view(np.float32)
    for i in range(B):
        j = B - 1 - i
        kind, yl, yh, xl, xh = (int(v) for v in table[i, :5])
        if kind == 1:
            out[i] = (fl[i, 0] * x[i]).astype(np.float32) + (fl[i, 1] * x[j]).astype(np.float32)
        elif kind == 2:
            out[i, :, yl:yh, xl:xh] = x[j, :, yl:yh, xl:xh]
    return out
