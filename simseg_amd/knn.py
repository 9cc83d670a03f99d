"""Weighted k-nearest-neighbour evaluation of a frozen encoder (DESIGN.md "k-NN evaluation"): the protocol DINO, iBOT and MoCo v3 report
beside the linear probe.  A bank of L2-normalised training features with their labels, one fused top-K search of the query features over
it (retrieval.search: no M x N matrix) at K = max(ks), and the temperature-weighted class vote for every k from one launch
(ops.knn_vote).  No training, no parameters.

Not covered: a bank sharded over ranks (every rank would hold the whole bank), k above ops.TOPK_MAX = 128, and config keys - the
evaluator takes keyword arguments."""
import torch

from . import ops
from .retrieval import search

F32, BF16 = torch.float32, torch.bfloat16


def normalize_rows(x):
    """[B, D] fp32 / bf16 / fp16 on the device -> fp32 rows x / max(||x||, 1e-12), through the row kernels (row_rnorm, scale_rows)."""
    if x.dim() != 2:
        raise ValueError(f"knn: features are [B, D] matrices, got shape {tuple(x.shape)}")
    ops.require_gpu(x)
    x = x.detach().contiguous()
    if x.dtype in ops.HALF_TYPES:
        x = ops.cast(x, F32)
    elif x.dtype != F32:
        raise TypeError(f"knn: fp32, bf16 or fp16 features, got {x.dtype}")
    return ops.scale_rows(x, ops.row_rnorm(x, eps=1e-12))


class FeatureBank:
    """Unit-norm gallery rows [N, dim] in `dtype` (fp32, or bf16 at half the memory) kept as the chunks they arrived in, each with the
    offset of its first row, and their labels as one int32 vector."""

    def __init__(self, dim, dtype=F32):
        if dim < 8 or dim % 8:
            raise ValueError(f"FeatureBank: dim = {dim}; the search takes D % 8 == 0 (topk_search's rule)")
        if dtype not in (F32, BF16):
            raise TypeError(f"FeatureBank: torch.float32 or torch.bfloat16 rows, got {dtype}")
        self.dim, self.dtype = int(dim), dtype
        self._chunks, self._offsets, self._labels, self._n = [], [], [], 0
        self._all_labels = None

    def __len__(self):
        return self._n

    def add(self, features, labels):
        """features [B, dim] (any floating dtype of the encoder), labels [B] of any integer dtype: normalises the rows and appends them as
        one chunk."""
        if features.dim() != 2 or features.shape[1] != self.dim:
            raise ValueError(f"FeatureBank.add: features are [B, {self.dim}], got shape {tuple(features.shape)}")
        lab = ops._labels_i32("FeatureBank.add: labels", labels, features.device)
        if lab.numel() != features.shape[0]:
            raise ValueError(f"FeatureBank.add: {lab.numel()} labels for {features.shape[0]} rows")
        if features.shape[0] == 0:
            return
        rows = normalize_rows(features)
        if self.dtype == BF16:
            rows = ops.cast(rows, BF16)
        self._chunks.append(rows)
        self._offsets.append(self._n)
        self._labels.append(lab)
        self._n += rows.shape[0]
        self._all_labels = None

    def chunks(self):
        """(chunk [n_i, dim], offset) pairs in the form retrieval.search takes: chunk row j is bank row offset + j."""
        return zip(self._chunks, self._offsets)

    @property
    def labels(self):
        """int32 [N], resident: row i of the bank has class labels[i]."""
        if not self._n:
            raise ValueError("FeatureBank: the bank is empty")
        if self._all_labels is None:
            self._all_labels = self._labels[0] if len(self._labels) == 1 else torch.cat(self._labels)
            self._labels = [self._all_labels]
        return self._all_labels


def knn_predict(queries, bank, ks=(10, 20, 100), temperature=0.07, compute_dtype=None, query_label=None, counts=None):
    """queries [M, D] raw features -> (pred [len(ks), M, 5], vote [len(ks), M, 5], counts) as ops.knn_vote returns them: one search at
    K = max(ks) over the bank's chunks serves every k.  compute_dtype: the search's operand type, None = the bank's."""
    ks = ops.check_knn_ks(ks)                     # max(ks) > TOPK_MAX is refused here, before any device work
    if len(bank) == 0:
        raise ValueError("knn_predict: the bank is empty")
    if queries.dim() != 2 or queries.shape[1] != bank.dim:
        raise ValueError(f"knn_predict: queries are [M, {bank.dim}], got shape {tuple(queries.shape)}")
    q = normalize_rows(queries)
    score, index = search(q, bank.chunks(), ks[-1], compute_dtype=compute_dtype or bank.dtype)
    return ops.knn_vote(score, index, bank.labels, ks, temperature, query_label=query_label, counts=counts)


class KNNEvaluator:
    """fit() fills a FeatureBank from the frozen model's features, evaluate() scores held-out batches against it.  Batches are
    {"image", "label"} dicts, as LinearProbeTrainer.evaluate takes them.  The feature is the [cls] row of model.forward_image_feature
    (`[:, 0]` when every token comes back), computed in eval() mode under torch.no_grad() and the model's own autocast;
    feature_fn(image) -> [B, D] replaces it (e.g. a CLIPModel's pooled embedding)."""

    def __init__(self, model, ks=(10, 20, 100), temperature=0.07, bank_dtype=F32, feature_fn=None):
        self.model, self.ks, self.temperature = model, ops.check_knn_ks(ks), float(temperature)
        self.bank_dtype, self.feature_fn = bank_dtype, feature_fn
        self.bank = None

    @torch.no_grad()
    def features(self, image):
        """[B, D] features of a batch of images; the model is left in the mode it was in."""
        was_training = self.model.training
        self.model.eval()
        try:
            if self.feature_fn is not None:
                return self.feature_fn(image)
            f = self.model.forward_image_feature(image)
            return f[:, 0] if f.dim() == 3 else f
        finally:
            self.model.train(was_training)

    def fit(self, batches):
        """Replaces the bank with the features of `batches`; -> the bank."""
        self.bank = None
        for batch in batches:
            f = self.features(batch["image"])
            if self.bank is None:
                self.bank = FeatureBank(f.shape[1], self.bank_dtype)
            self.bank.add(f, batch["label"])
        if self.bank is None:
            raise ValueError("KNNEvaluator.fit: no batches")
        return self.bank

    def evaluate(self, batches):
        """-> {k: {"top1": percent, "top5": percent}}.  The hit counts accumulate on the device; they are read back once, at the end."""
        if self.bank is None:
            raise ValueError("KNNEvaluator.evaluate: fit() a bank first")
        counts = None
        for batch in batches:
            counts = knn_predict(self.features(batch["image"]), self.bank, self.ks, self.temperature, query_label=batch["label"], counts=counts)[2]
        if counts is None:
            return {k: {"top1": float("nan"), "top5": float("nan")} for k in self.ks}
        rows = counts.tolist()                    # the one host read
        return {k: {"top1": 100.0 * h1 / n, "top5": 100.0 * h5 / n} for k, (n, h1, h5) in zip(self.ks, rows)}
