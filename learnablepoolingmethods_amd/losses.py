"""Losses (reference: losses.py:21-96).

HingeLoss and SoftmaxLoss carry a torch formulation for any device and any label dtype (the CPU path and the drop-in surface); fp32
predictions with bool / uint8 labels on the GPU go to ops.label_loss (csrc/label_loss.hip: one launch each way over the predictions,
the labels read as bytes) when FLAGS.label_loss_fused is on.  ``by_name`` is train.py:576's
``find_class_by_name(FLAGS.label_loss, [losses])()``."""
import torch

from .flags import FLAGS


class BaseLoss(object):
    def calculate_loss(self, unused_predictions, unused_labels, **unused_params):
        raise NotImplementedError()


class CrossEntropyLoss(BaseLoss):
    """losses.py:41-51: epsilon = 10e-6, sum over classes, mean over the batch."""

    def calculate_loss(self, predictions, labels, **unused_params):
        epsilon = 10e-6
        float_labels = labels.to(predictions.dtype)
        cross_entropy_loss = float_labels * torch.log(predictions + epsilon) + \
            (1 - float_labels) * torch.log(1 - predictions + epsilon)
        return (-cross_entropy_loss).sum(dim=1).mean()


def _fused(predictions, labels) -> bool:
    return bool(FLAGS.label_loss_fused and predictions.is_cuda and labels.is_cuda and predictions.dtype == torch.float32
                and labels.dtype in (torch.bool, torch.uint8) and predictions.dim() == 2 and predictions.shape == labels.shape
                and predictions.numel() > 0)


class HingeLoss(BaseLoss):
    """losses.py:54-69: s = 2 y - 1, sum over classes of max(0, b - s p), mean over the batch.  tf.maximum(zeros, .) hands the gradient
    of a tie (b - s p == 0) to its first argument, the zeros: torch.where(m > 0, m, 0), not clamp_min (which gives a tie gradient 1)."""

    def calculate_loss(self, predictions, labels, b=1.0, **unused_params):
        if _fused(predictions, labels):
            from . import ops
            return ops.label_loss(predictions, labels, "hinge", b=b)
        float_labels = labels.to(predictions.dtype)
        sign_labels = 2 * float_labels - 1
        margin = b - sign_labels * predictions
        hinge_loss = torch.where(margin > 0, margin, torch.zeros_like(margin))
        return hinge_loss.sum(dim=1).mean()


class SoftmaxLoss(BaseLoss):
    """losses.py:72-96: epsilon = 10e-8, labels L1-normalised per row (row sum at least epsilon), minus their dot product with
    log softmax(p), mean over the batch.  log_softmax takes the row maximum out, so a row without labels is 0 * (finite): exactly 0 in
    the loss and in the gradient."""

    def calculate_loss(self, predictions, labels, **unused_params):
        if _fused(predictions, labels):
            from . import ops
            return ops.label_loss(predictions, labels, "softmax")
        epsilon = 10e-8
        float_labels = labels.to(predictions.dtype)
        label_rowsum = float_labels.sum(dim=1, keepdim=True).clamp_min(epsilon)
        norm_float_labels = float_labels / label_rowsum
        softmax_loss = -(norm_float_labels * torch.log_softmax(predictions, dim=1)).sum(dim=1)
        return softmax_loss.mean()


_BY_NAME = {c.__name__: c for c in (CrossEntropyLoss, HingeLoss, SoftmaxLoss)}


def by_name(name):
    """An instance of the loss class called ``name`` (train.py:576); an unknown name raises and lists the classes."""
    if name not in _BY_NAME:
        raise ValueError(f"unknown label_loss {name!r}; the losses are {', '.join(sorted(_BY_NAME))}")
    return _BY_NAME[name]()
