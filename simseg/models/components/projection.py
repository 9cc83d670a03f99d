import torch.nn as nn

from simseg_amd.nn import compute_dtype
from simseg_amd.towers import LinearFn, MlpHeadFn

__all__ = ["SimpleProjection", "ComplexProjection", "MlpProjection"]


class SimpleProjection(nn.Module):
    """Per-token Linear(D -> projection_dim, bias=False): simseg/models/components/projection.py:29-46."""

    def __init__(self, cfg, embedding_dim, projection_dim, trainable=True):
        super().__init__()
        self.projection_dim = projection_dim
        self.linear = nn.Linear(embedding_dim, projection_dim, bias=False)
        nn.init.trunc_normal_(self.linear.weight, std=0.02)
        if not trainable:
            for p in self.linear.parameters():
                p.requires_grad = False

    def forward(self, x):
        return LinearFn.apply(x, self.linear.weight, None, compute_dtype())


class ComplexProjection(nn.Module):
    def __init__(self, *a, **kw):
        super().__init__()
        raise NotImplementedError("projection.name='complex' is not used by any shipped config and cannot be built by the "
                                  "reference either (its ctor rejects the `trainable` kwarg CLIPModel passes, clip.py:28-33)")


class MlpProjection(nn.Module):
    """Linear(D -> hidden, bias) -> erf-GELU -> Linear(hidden -> out, bias=False): the projection head of the image self-supervision branch
    (CLIPModel.enable_ssl; SimCLR's / SLIP's MLP head without its batch norms), one autograd node (simseg_amd.towers.MlpHeadFn)."""

    def __init__(self, embedding_dim, hidden_dim, out_dim):
        super().__init__()
        self.fc1 = nn.Linear(embedding_dim, hidden_dim, bias=True)
        self.fc2 = nn.Linear(hidden_dim, out_dim, bias=False)
        nn.init.trunc_normal_(self.fc1.weight, std=0.02)
        nn.init.zeros_(self.fc1.bias)
        nn.init.trunc_normal_(self.fc2.weight, std=0.02)

    def forward(self, x):
        return MlpHeadFn.apply(x, self.fc1.weight, self.fc1.bias, self.fc2.weight, compute_dtype())
