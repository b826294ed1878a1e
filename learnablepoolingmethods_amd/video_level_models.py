"""MoeModel (reference: video_level_models.py:48-158), FishMoeModel3 (:367-438), MoeModel2 (:441-541), JuhanMoeModel (:544-622),
FourLayerBatchNeuralModel (:625-684), ClassLearningThreeNnModel (:687-714) and ClassLearningFourNnModel (:717-749) --
host-side PyTorch per the north-star; the glue of the class filter behind MoeModel2 / JuhanMoeModel is ops.class_filter on the GPU,
the row-wise glue of FishMoeModel3 (LayerNorm, softmax) ops.class_rows."""
from __future__ import annotations

import math

import torch

from . import FLAGS, models
from . import variables as vs


def _linear(x, W, b=None):
    """x W (+ b); on the GPU through ops.linear_direct (the weight gradient may go straight into the trainer's gradient arena)."""
    if x.is_cuda and x.dtype == torch.float32 and W.dtype == torch.float32 and x.dim() == 2:
        from . import ops
        return ops.linear_direct(x, W, b)
    return torch.addmm(b, x, W) if b is not None else x.matmul(W)


class MoeModel(models.BaseModel):
    """A softmax over a mixture of logistic models (with L2 regularization)."""

    def create_model(self, model_input, vocab_size, is_training=True, num_mixtures=None, l2_penalty=1e-8,
                     labels=None, fused_cross_entropy=False, **unused_params):
        """labels + fused_cross_entropy (the trainer sets it when its loss is CrossEntropyLoss): the mixture tail and the
        loss run as one fused kernel pair and the result carries "loss" (train.py:291-294 takes it from there)."""
        num_mixtures = num_mixtures or FLAGS.moe_num_mixtures
        low_rank_gating = FLAGS.moe_low_rank_gating                    # :77
        l2_penalty = FLAGS.moe_l2                                     # :78 (the kwarg is ignored, App. C15)
        gating_probabilities = FLAGS.moe_prob_gating                   # :79
        gating_input = FLAGS.moe_prob_gating_input                     # :80
        H = model_input.shape[1]
        dev = model_input.device
        store = vs.default_store()
        if low_rank_gating == -1:
            with vs.variable_scope("gates"):                           # slim.fully_connected, no bias :86-93
                wg = vs.get_variable("weights", [H, vocab_size * (num_mixtures + 1)], vs.glorot_uniform_initializer(), device=dev)
            store.add_l2_regularizer(wg, l2_penalty)                   # slim.l2_regularizer :91
            gate_activations = _linear(model_input, wg)
        else:                                                          # two bias-free layers through a low_rank_gating bottleneck :94-108
            with vs.variable_scope("gates1"):
                wg1 = vs.get_variable("weights", [H, low_rank_gating], vs.glorot_uniform_initializer(), device=dev)
            with vs.variable_scope("gates2"):
                wg2 = vs.get_variable("weights", [low_rank_gating, vocab_size * (num_mixtures + 1)], vs.glorot_uniform_initializer(), device=dev)
            store.add_l2_regularizer(wg1, l2_penalty)                  # :99
            store.add_l2_regularizer(wg2, l2_penalty)                  # :106
            gate_activations = model_input.matmul(wg1).matmul(wg2)
        with vs.variable_scope("experts"):                             # :109-114
            we = vs.get_variable("weights", [H, vocab_size * num_mixtures], vs.glorot_uniform_initializer(), device=dev)
            be = vs.get_variable("biases", [vocab_size * num_mixtures], vs.zeros_initializer(), device=dev)
        store.add_l2_regularizer(we, l2_penalty)                       # :113
        expert_activations = _linear(model_input, we, be)
        fuse_loss = fused_cross_entropy and not gating_probabilities   # (probability gating changes the predictions behind the mixture)
        if model_input.is_cuda and num_mixtures <= 8 and (labels is None or fused_cross_entropy):
            from . import ops
            probabilities, loss = ops.moe_cross_entropy(gate_activations, expert_activations,
                                                        labels if fuse_loss else None, num_mixtures)   # :116-126 (+ losses.py:41-51)
            if not gating_probabilities:
                return {"predictions": probabilities, "loss": loss} if loss is not None else {"predictions": probabilities}
        else:
            gating_distribution = torch.softmax(gate_activations.reshape(-1, num_mixtures + 1), dim=-1)   # :116-118
            expert_distribution = torch.sigmoid(expert_activations.reshape(-1, num_mixtures))             # :119-121
            probabilities = (gating_distribution[:, :num_mixtures] * expert_distribution).sum(dim=1)      # :123-124
            probabilities = probabilities.reshape(-1, vocab_size)                                         # :125-126
        if gating_probabilities:                                       # :128-156
            from . import layers
            rows = vocab_size if gating_input == "prob" else H
            gating_weights = vs.get_variable("gating_prob_weights", [rows, vocab_size],
                                             vs.random_normal_initializer(1 / math.sqrt(vocab_size)), device=dev)   # :130-140
            gates = (probabilities if gating_input == "prob" else model_input).matmul(gating_weights)
            if FLAGS.gating_remove_diag:                               # :144-147 (tf.matrix_diag_part: the main diagonal)
                if rows != vocab_size:
                    raise ValueError("gating_remove_diag with moe_prob_gating_input != 'prob': the diagonal of a "
                                     f"[{rows}, {vocab_size}] matrix does not broadcast against the probabilities (as in the reference)")
                gates = gates - torch.diagonal(gating_weights) * probabilities
            gates = layers.batch_norm(gates, is_training, "gating_prob_bn")                                # :149-154
            probabilities = probabilities * torch.sigmoid(gates)                                           # :156-158
        return {"predictions": probabilities}                                                             # :158


CLASS_FILTER_KEEP_PROB = 0.8       # tf.nn.dropout(., 0.8): the second argument is the KEEP probability (:526, :598, :607)
CLASS_FILTER_NUM_MIXTURES = 3      # num_mixtures = 3, whatever the argument says (:469, :570)


def _mixture_of_experts(model_input, vocab_size, num_mixtures, l2_penalty, low_rank_gating=-1):
    """The MoE mixture MoeModel2 and JuhanMoeModel start with (video_level_models.py:475-516, :572-596): bias-free gates (optionally
    through a low_rank_gating bottleneck), experts with a bias, every weight under slim.l2_regularizer(l2_penalty) -> probabilities
    [B, vocab_size].  On the GPU the softmax / sigmoid / sum tail is ops.moe_cross_entropy without labels."""
    H = model_input.shape[1]
    dev = model_input.device
    store = vs.default_store()
    if low_rank_gating == -1:
        with vs.variable_scope("gates"):
            wg = vs.get_variable("weights", [H, vocab_size * (num_mixtures + 1)], vs.glorot_uniform_initializer(), device=dev)
        store.add_l2_regularizer(wg, l2_penalty)
        gate_activations = _linear(model_input, wg)
    else:
        with vs.variable_scope("gates1"):
            wg1 = vs.get_variable("weights", [H, low_rank_gating], vs.glorot_uniform_initializer(), device=dev)
        with vs.variable_scope("gates2"):
            wg2 = vs.get_variable("weights", [low_rank_gating, vocab_size * (num_mixtures + 1)], vs.glorot_uniform_initializer(), device=dev)
        store.add_l2_regularizer(wg1, l2_penalty)
        store.add_l2_regularizer(wg2, l2_penalty)
        gate_activations = model_input.matmul(wg1).matmul(wg2)
    with vs.variable_scope("experts"):
        we = vs.get_variable("weights", [H, vocab_size * num_mixtures], vs.glorot_uniform_initializer(), device=dev)
        be = vs.get_variable("biases", [vocab_size * num_mixtures], vs.zeros_initializer(), device=dev)
    store.add_l2_regularizer(we, l2_penalty)
    expert_activations = _linear(model_input, we, be)
    if model_input.is_cuda and model_input.dtype == torch.float32:
        from . import ops
        return ops.moe_cross_entropy(gate_activations, expert_activations, None, num_mixtures)[0]
    gating_distribution = torch.softmax(gate_activations.reshape(-1, num_mixtures + 1), dim=-1)
    expert_distribution = torch.sigmoid(expert_activations.reshape(-1, num_mixtures))
    return (gating_distribution[:, :num_mixtures] * expert_distribution).sum(dim=1).reshape(-1, vocab_size)


def _keep_mask(masks, key, shape, device):
    """The KEEP mask [B, C] (uint8, 1 = kept) of one tf.nn.dropout: the one handed in under ``key``, or a draw of ops.dropout_keep_mask
    (allocated as a multiple of 16 elements, the size its kernel takes, and cut to [B, C])."""
    keep = masks.get(key)
    if keep is not None:
        if tuple(keep.shape) != tuple(shape):
            raise ValueError(f"dropout_masks[{key!r}] must be {list(shape)}, got {list(keep.shape)}")
        return keep.to(device=device).ne(0).to(torch.uint8).contiguous()
    from . import ops
    n = shape[0] * shape[1]
    return ops.dropout_keep_mask(((n + 15) // 16 * 16,), CLASS_FILTER_KEEP_PROB, device)[:n].view(*shape)


def _filter_stage(a, bias, residual, act, batch_norm, is_training, keep):
    """One stage of the class filter behind its GEMM ``a``: dropout(BN(act(a + bias + residual))), act "relu" | "leaky_relu" (alpha 0.2,
    tf.nn.leaky_relu's default) | "sigmoid", BN a tf.layers.batch_normalization with the next automatic name.  FLAGS.class_filter_fused
    on the GPU: one ops.class_filter launch each way; otherwise the torch formulation (the CPU path; same variables, same results)."""
    from . import layers
    bn = layers.tf_layers_bn_variables(a.shape[1], a.device) if batch_norm else None
    keep = keep if is_training else None
    if FLAGS.class_filter_fused and a.is_cuda:
        from . import ops
        if ops.class_filter_ok(a, bias, residual, act, bn, is_training, keep, CLASS_FILTER_KEEP_PROB):
            return ops.class_filter(a, bias, residual, act=act, bn=bn, is_training=is_training, keep=keep,
                                    keep_prob=CLASS_FILTER_KEEP_PROB, decay=layers.TF_LAYERS_BN_MOMENTUM, alpha=0.2)
    return _filter_stage_torch(a, bias, residual, act, bn, is_training, keep)


def _filter_stage_torch(a, bias, residual, act, bn, is_training, keep):
    """_filter_stage's torch formulation on given batch-norm variables (gamma, beta, moving_mean, moving_variance) or None."""
    from . import layers
    pre = a if bias is None else a + bias
    if residual is not None:
        pre = pre + residual
    u = {"relu": torch.relu, "leaky_relu": lambda t: torch.nn.functional.leaky_relu(t, 0.2), "sigmoid": torch.sigmoid}[act](pre)
    if bn is not None:
        u = layers.tf_layers_bn_apply(u, is_training, *bn)
    if keep is not None:
        u = u * keep.to(u.dtype) / CLASS_FILTER_KEEP_PROB
    return u


def _class_filter(probabilities, vocab_size, is_training, act, masks):
    """The class filter over the vocabulary (video_level_models.py:518-539, :600-620): v-filter1 (V -> 2V, bias, act, batch norm, dropout
    in training), v-filter2 (2V -> V, no bias), p + filter2 -> act -> batch norm, v-final_output (V -> V, bias, sigmoid).  The variables
    carry tf.layers' names: v-filter1/{kernel,bias}, batch_normalization/..., v-filter2/kernel, batch_normalization_1/...,
    v-final_output/{kernel,bias}."""
    from . import layers
    dev = probabilities.device
    B = probabilities.shape[0]
    w1, b1 = layers.dense_variables("v-filter1", vocab_size, vocab_size * 2, True, dev)
    keep1 = _keep_mask(masks, "filter1", (B, vocab_size * 2), dev) if is_training else None
    filter1 = _filter_stage(_linear(probabilities, w1), b1, None, act, True, is_training, keep1)              # :518-526 / :600-607
    w2, _ = layers.dense_variables("v-filter2", vocab_size * 2, vocab_size, False, dev)
    p = _filter_stage(_linear(filter1, w2), None, probabilities, act, True, is_training, None)                # :528-536 / :609-617
    w3, b3 = layers.dense_variables("v-final_output", vocab_size, vocab_size, True, dev)
    return _filter_stage(_linear(p, w3), b3, None, "sigmoid", False, is_training, None)                       # :538-539 / :619-620


class MoeModel2(models.BaseModel):
    """The MoE mixture with three experts, then the class filter with relu (video_level_models.py:441-541).  num_mixtures is 3 whatever
    the argument says (:469), the penalty is FLAGS.moe_l2 (:471; the argument is ignored), moe_low_rank_gating is honoured as in MoeModel,
    moe_prob_gating and moe_prob_gating_input are read and used nowhere (:472-473).  ``dropout_masks`` {"filter1"}: the KEEP mask
    [B, 2 vocab_size] (non-zero = kept) in place of the random draw.  ``labels`` / ``fused_cross_entropy`` (the trainer's) are ignored:
    the loss is taken of the filter's output."""

    def create_model(self, model_input, vocab_size, is_training=True, num_mixtures=None, l2_penalty=1e-8, dropout_masks=None,
                     labels=None, fused_cross_entropy=False, **unused_params):
        probabilities = _mixture_of_experts(model_input, vocab_size, CLASS_FILTER_NUM_MIXTURES, FLAGS.moe_l2, FLAGS.moe_low_rank_gating)
        return {"predictions": _class_filter(probabilities, vocab_size, is_training, "relu", dropout_masks or {})}


class JuhanMoeModel(models.BaseModel):
    """The MoE mixture with three experts, dropout of the probabilities in training (keep 0.8; the residual takes the dropped tensor),
    then the class filter with leaky_relu (alpha 0.2) (video_level_models.py:544-622).  Reads no flag: the penalty is the ``l2_penalty``
    argument.  ``dropout_masks`` {"probabilities": [B, vocab_size], "filter1": [B, 2 vocab_size]}: KEEP masks in place of the random
    draws.  ``labels`` / ``fused_cross_entropy`` are ignored."""

    def create_model(self, model_input, vocab_size, is_training=True, num_mixtures=None, l2_penalty=1e-8, dropout_masks=None,
                     labels=None, fused_cross_entropy=False, **unused_params):
        masks = dropout_masks or {}
        probabilities = _mixture_of_experts(model_input, vocab_size, CLASS_FILTER_NUM_MIXTURES, l2_penalty)
        if is_training:                                                                                      # :597-598
            keep = _keep_mask(masks, "probabilities", tuple(probabilities.shape), probabilities.device)
            probabilities = probabilities * keep.to(probabilities.dtype) / CLASS_FILTER_KEEP_PROB
        return {"predictions": _class_filter(probabilities, vocab_size, is_training, "leaky_relu", masks)}


def _batch_normalization(x, is_training):
    """tf.layers.batch_normalization(x, training=is_training) over [B, V] with the next automatic name.  FLAGS.class_filter_fused on the
    GPU: ops.class_filter with act "leaky_relu" and alpha = 1.0 -- t > 0 ? t : 1.0 t, exactly the identity both ways;
    otherwise layers.tf_layers_bn_apply (the CPU path; same variables, same results)."""
    from . import layers
    bn = layers.tf_layers_bn_variables(x.shape[1], x.device)
    if FLAGS.class_filter_fused and x.is_cuda:
        from . import ops
        if ops.class_filter_ok(x, None, None, "leaky_relu", bn, is_training):
            return ops.class_filter(x, act="leaky_relu", bn=bn, is_training=is_training, decay=layers.TF_LAYERS_BN_MOMENTUM, alpha=1.0)
    return layers.tf_layers_bn_apply(x, is_training, *bn)


class FishMoeModel3(models.BaseModel):
    """The MoE mixture, then a residual block over the vocabulary and a softmax (video_level_models.py:367-438): batch norm, dense
    (V -> V filter_size, bias) + relu + batch norm, dense_1 (-> V, bias), p0 + r1 -> LayerNorm -> batch norm, dense_2 (V -> V, bias) +
    softmax.  num_mixtures is the argument or FLAGS.moe_num_mixtures (:396), the penalty is FLAGS.moe_l2 (:397; the argument is
    ignored), there is no low-rank gating.  tf.layers.dropout(r_activation0, 0.9) (:430) is given no ``training=``, so it is the
    identity in TF1, also in training: no mask is drawn (a ``dropout_masks`` argument is accepted and read nowhere).
    The variables carry tf.layers' and slim's automatic names.  ``labels`` / ``fused_cross_entropy`` (the trainer's) are ignored: the
    loss is taken of the softmax output.  On the GPU the two row stages are one ops.class_rows each with FLAGS.class_rows_fused (off
    by default: flags.py says what was measured), the three batch norms one ops.class_filter each (FLAGS.class_filter_fused)."""

    def create_model(self, model_input, vocab_size, is_training=True, num_mixtures=None, l2_penalty=1e-6, filter_size=2,
                     labels=None, fused_cross_entropy=False, **unused_params):
        from . import layers
        dev = model_input.device
        store = vs.default_store()
        num_mixtures = num_mixtures or FLAGS.moe_num_mixtures                                                # :396
        probabilities0 = _mixture_of_experts(model_input, vocab_size, num_mixtures, FLAGS.moe_l2)            # :397-424
        probabilities0 = _batch_normalization(probabilities0, is_training)                                   # :425
        w0, b0 = layers.dense_variables(store.unique_layer_name("dense"), vocab_size, vocab_size * filter_size, True, dev)
        r_activation0 = _filter_stage(_linear(probabilities0, w0), b0, None, "relu", True, is_training, None)   # :427-428 (:430: a no-op)
        w1, b1 = layers.dense_variables(store.unique_layer_name("dense"), vocab_size * filter_size, vocab_size, True, dev)
        ln = layers.layer_norm_variables("LayerNorm", vocab_size, dev)
        probabilities1 = layers.class_rows(_linear(r_activation0, w1), b1, probabilities0, norm="layer_norm", ln=ln)   # :431-434
        probabilities1 = _batch_normalization(probabilities1, is_training)                                   # :435
        w2, b2 = layers.dense_variables(store.unique_layer_name("dense"), vocab_size, vocab_size, True, dev)
        return {"predictions": layers.class_rows(_linear(probabilities1, w2), b2, norm="softmax")}           # :436-438


class FourLayerBatchNeuralModel(models.BaseModel):
    """Four bias-free layers of width vocab_size (video_level_models.py:625-684): relu BEFORE batch norm on the first three
    (``fc{1,2,3}_weights``, ``fc{1,2,3}_activation_bn``), then ``fc4_weights`` with ``fc4_bias`` (initialised to 0.01) and a sigmoid.
    Every weight is xavier; ``l2_penalty`` is accepted and read nowhere, as written (no regulariser is attached)."""

    def create_model(self, model_input, vocab_size, is_training=True, l2_penalty=1e-7, **unused_params):
        from . import layers
        dev = model_input.device
        h = model_input
        for i in (1, 2, 3):                                                             # :632-670
            w = vs.get_variable(f"fc{i}_weights", [h.shape[1], vocab_size], vs.glorot_uniform_initializer(), device=dev)
            vs.summary(f"fc{i}_weights", w)
            h = layers.batch_norm(torch.relu(h.matmul(w)), is_training, f"fc{i}_activation_bn")
        fc4_weights = vs.get_variable("fc4_weights", [vocab_size, vocab_size], vs.glorot_uniform_initializer(), device=dev)   # :672-675
        fc4_bias = vs.get_variable("fc4_bias", [vocab_size], lambda shape, d, gen: torch.full(shape, 0.01, device=d), device=dev)
        vs.summary("fc4_bias", fc4_bias)
        return {"predictions": torch.sigmoid(h.matmul(fc4_weights) + fc4_bias)}          # :680-684


def _class_learning_fc(x, scope, biases, vocab_size, l2_penalty):
    """slim.fully_connected of the ClassLearning*NnModel classifiers: width vocab_size, l2-regularised weights, a bias (0.1) or none."""
    dev = x.device
    with vs.variable_scope(scope):
        w = vs.get_variable("weights", [x.shape[1], vocab_size], vs.glorot_uniform_initializer(), device=dev)
        b = vs.get_variable("biases", [vocab_size], lambda shape, d, gen: torch.full(shape, 0.1, device=d), device=dev) if biases else None
    vs.default_store().add_l2_regularizer(w, l2_penalty)                          # slim.l2_regularizer :697,704,711 / :727-746
    y = x.matmul(w)
    return y + b if biases else y


class ClassLearningThreeNnModel(models.BaseModel):
    """Three fully connected layers of width vocab_size (video_level_models.py:687-714): bias-free + layer_norm + leaky_relu(0.2)
    (+ dropout, keep probability 0.5, in training) twice, then sigmoid with a bias initialised to 0.1.  Variable names are slim's:
    fully_connected[_1|_2]/weights, fully_connected_2/biases, LayerNorm[_1]/{beta,gamma}.  ``dropout_masks`` {"fc1", "fc2"}: KEEP
    masks [B, vocab_size] (non-zero = kept) in place of the random draw (App. C10: the default is faithful, parity tests hand masks in)."""

    KEEP_PROB = 0.5

    def create_model(self, model_input, vocab_size, is_training=True, l2_penalty=1e-8, ortho_reg=0, dropout_masks=None,
                     **unused_params):
        from . import layers
        dev = model_input.device
        masks = dropout_masks or {}

        def fully_connected(x, scope, biases):
            return _class_learning_fc(x, scope, biases, vocab_size, l2_penalty)

        def dropout(x, key):
            if not is_training:
                return x
            keep = masks.get(key)
            if keep is None:
                keep = torch.rand(x.shape, device=dev) < self.KEEP_PROB
            return x * keep.to(device=dev).ne(0).to(x.dtype) / self.KEEP_PROB          # tf.nn.dropout(keep_prob=0.5) :700,707

        fc1 = fully_connected(model_input, "fully_connected", False)                   # :695-697
        fc1 = torch.nn.functional.leaky_relu(layers.layer_norm(fc1, "LayerNorm"), 0.2)  # :698
        fc1 = dropout(fc1, "fc1")
        fc2 = fully_connected(fc1, "fully_connected_1", False)                          # :702-704
        fc2 = torch.nn.functional.leaky_relu(layers.layer_norm(fc2, "LayerNorm_1"), 0.2)  # :705
        fc2 = dropout(fc2, "fc2")
        fc3 = torch.sigmoid(fully_connected(fc2, "fully_connected_2", True))            # :709-711
        return {"predictions": fc3, "regularization_loss": ortho_reg}


class ClassLearningFourNnModel(models.BaseModel):
    """Four fully connected layers of width vocab_size (video_level_models.py:717-749): bias-free + layer_norm + leaky_relu(0.2) three
    times -- NO dropout: the reference's dropout lines are commented out (:729-730, :736-737) -- then sigmoid with a bias initialised
    to 0.1.  Variable names are slim's: fully_connected[_1|_2|_3]/weights, fully_connected_3/biases, LayerNorm[_1|_2]/{beta,gamma}."""

    def create_model(self, model_input, vocab_size, is_training=True, l2_penalty=1e-8, ortho_reg=0, **unused_params):
        from . import layers
        h = model_input
        for i in range(3):                                                              # :725-742
            suffix = f"_{i}" if i else ""
            h = _class_learning_fc(h, "fully_connected" + suffix, False, vocab_size, l2_penalty)
            h = torch.nn.functional.leaky_relu(layers.layer_norm(h, "LayerNorm" + suffix), 0.2)
        fc4 = torch.sigmoid(_class_learning_fc(h, "fully_connected_3", True, vocab_size, l2_penalty))   # :744-746
        return {"predictions": fc4, "regularization_loss": ortho_reg}
