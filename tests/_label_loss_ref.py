"""HingeLoss and SoftmaxLoss restated in fp64 from the reference's lines (losses.py:54-69, :72-96), with the gradients TensorFlow's
registered gradient functions give -- never from the op or the classes under test.

Each function -> (loss, dloss/dpredictions), fp64 on the CPU, the gradient scaled by ``upstream``.

Hinge, losses.py:63-69:
    float_labels = cast(labels);  sign_labels = 2 * float_labels - all_ones
    hinge_loss = maximum(all_zeros, b * all_ones - sign_labels * predictions)
    return reduce_mean(reduce_sum(hinge_loss, 1))
  tf.maximum(x, y)'s gradient (math_grad._MaximumMinimumGrad with xmask = x >= y) sends the upstream gradient to x where x >= y and to y
  elsewhere: with x = all_zeros, y = the margin, the margin receives it where 0 < margin STRICTLY; a tie goes to the zeros.

Softmax, losses.py:86-96:
    label_rowsum = maximum(reduce_sum(float_labels, 1, keep_dims=True), epsilon), epsilon = 10e-8
    norm_float_labels = float_labels / label_rowsum
    softmax_loss = -reduce_sum(norm_float_labels * log(softmax(predictions)), 1);  return reduce_mean(softmax_loss)
  d/dp_j of -sum_k n_k log softmax(p)_k = softmax(p)_j * sum_k n_k - n_j (sum_k n_k is 1 for a labelled row and 0 for a row without
  labels).  In fp64 softmax(p) stays positive over every input range the tests use, so log never sees a zero."""
import torch


def hinge(predictions, labels, b=1.0, upstream=1.0):
    p = predictions.detach().double().cpu()
    float_labels = labels.detach().cpu().to(torch.float64)
    all_zeros, all_ones = torch.zeros_like(float_labels), torch.ones_like(float_labels)
    sign_labels = 2 * float_labels - all_ones
    margin = b * all_ones - sign_labels * p
    hinge_loss = torch.maximum(all_zeros, margin)
    loss = hinge_loss.sum(dim=1).mean()
    to_margin = ~(all_zeros >= margin)                                  # _MaximumMinimumGrad: xmask = (x >= y) keeps it at x
    grad = torch.where(to_margin, -sign_labels, all_zeros) * (upstream / p.shape[0])
    return loss, grad


def softmax(predictions, labels, upstream=1.0):
    epsilon = 10e-8
    p = predictions.detach().double().cpu()
    float_labels = labels.detach().cpu().to(torch.float64)
    label_rowsum = torch.clamp(float_labels.sum(dim=1, keepdim=True), min=epsilon)
    norm_float_labels = float_labels / label_rowsum
    softmax_outputs = torch.softmax(p, dim=1)
    softmax_loss = -(norm_float_labels * torch.log(softmax_outputs)).sum(dim=1)
    loss = softmax_loss.mean()
    grad = (softmax_outputs * norm_float_labels.sum(dim=1, keepdim=True) - norm_float_labels) * (upstream / p.shape[0])
    return loss, grad


BY_NAME = {"HingeLoss": hinge, "SoftmaxLoss": softmax}
