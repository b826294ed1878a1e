"""NetVladOrthoReg and NetVladAttenCluster (reference: video_pooling_modules.py:1499-1586, 1589-1663) and the triangulation
embeddings (TriangulationEmbedding :376-428, WeightedTriangulationEmbedding :1395-1459, TriangulationTemporalEmbedding :1462-1497)."""
from __future__ import annotations

import math

from . import layers, module_utils, modules, ops, transformer_utils
from . import variables as vs


class NetVladOrthoReg(modules.BaseModule):
    """NetVLAD from WILLOW's model with orthogonal regularisation (video_pooling_modules.py:1499-1586): the pooling is
    NetVLAD's (same K1/K2/K3 kernels) with a 2-D ``cluster_weights2`` [D, K] and scope-id-suffixed variable names; the
    penalty ``det_reg * sum |W2n^T W2n - I|`` is collected as a regularisation loss."""

    def __init__(self, feature_size, max_frames, cluster_size, batch_norm, is_training, det_reg=None, scope_id=None):
        self.feature_size = feature_size
        self.max_frames = max_frames
        self.is_training = is_training
        self.batch_norm = batch_norm
        self.cluster_size = int(cluster_size)
        self.det_reg = det_reg
        self.scope_id = scope_id

    def forward(self, inputs, **unused_params):
        D, K, dev = self.feature_size, self.cluster_size, inputs.device
        sid = "" if self.scope_id is None else str(self.scope_id)
        std = 1 / math.sqrt(D)
        cluster_weights = vs.get_variable("cluster_weights" + sid, [D, K], vs.random_normal_initializer(std), device=dev)
        bn = bias = None
        if self.batch_norm:
            bn = layers.bn_variables("cluster_bn", K, dev)
        else:
            bias = vs.get_variable("cluster_biases" + sid, [K], vs.random_normal_initializer(std), device=dev)
        cluster_weights2 = vs.get_variable("cluster_weights2", [D, K], vs.random_normal_initializer(std), device=dev)
        if self.det_reg is not None:
            reg = module_utils.orthogonal_regularizer(self.det_reg, self.scope_id)(cluster_weights2)
            if reg is not None:
                vs.default_store().add_regularization_loss(reg)
        return ops.netvlad(inputs, cluster_weights, cluster_weights2.reshape(1, D, K), self.max_frames, bn=bn, bias=bias,
                           is_training=self.is_training)


class NetVladAttenCluster(modules.BaseModule):
    """NetVLAD whose cluster similarities come from a frame-level transformer encoder."""

    def __init__(self, feature_size, max_frames, cluster_size, batch_norm, is_training, scope_id=None):
        self.feature_size = feature_size
        self.max_frames = max_frames
        self.is_training = is_training
        self.batch_norm = batch_norm
        self.cluster_size = int(cluster_size)
        self.scope_id = scope_id
        self.encoder_hidden_size = feature_size
        self.num_heads = feature_size // 16               # :1613
        self.dropout_ratio = 0.1
        self.filter_size = 4 * self.encoder_hidden_size   # :1615

    def forward(self, inputs, dropout_mask=None, dropout_rate=None, lazy=False, **unused_params):
        """inputs [(B*max_frames), F] -> [B, F*K] (f-major), L2-normalised (lazy: the lazily normalised form, ops.vlad_aggregate)."""
        reshaped_input = inputs.reshape(-1, self.max_frames, self.feature_size)          # :1623
        with vs.variable_scope("cluster_attention"):
            encoder_block = transformer_utils.TransformerEncoderMod(
                feature_size=self.feature_size, hidden_size=self.encoder_hidden_size, num_heads=self.num_heads,
                attention_dropout=self.dropout_ratio, ff_filter_size=self.filter_size, ff_relu_dropout=0.1,
                is_train=self.is_training, scope_id="encode", final_size=self.cluster_size)
            # (the frames are read twice, by the encoder and by the aggregation below: their two gradients meet inside the encoder's
            # backward instead of in an add pass of autograd's -- ops.GradJoin)
            join = ops.GradJoin() if (self.is_training and inputs.is_cuda) else None
            cluster_similarities = encoder_block.forward(reshaped_input, dropout_mask=dropout_mask,
                                                         dropout_rate=dropout_rate, grad_join=join)          # [B,S,K] :1638
        cluster_centres = vs.get_variable("cluster_centers", [self.feature_size, self.cluster_size],
                                          vs.random_normal_initializer(1 / math.sqrt(self.feature_size)),
                                          device=inputs.device)                                # :1641-1643
        # sum_n sims * (x - c), intra-L2, flatten, L2 (:1646-1658; App. C6/C7) -- HIP kernel K2
        return ops.vlad_aggregate(cluster_similarities, inputs, cluster_centres, self.max_frames, lazy=lazy, grad_join=join)


def _anchor_weights(feature_size, anchor_size, scope_id, device):
    """``anchor_weights{scope_id}`` [D, K], N(0, 1 / K) (:401-405, :1423-1426)."""
    sid = "" if scope_id is None else str(scope_id)
    return vs.get_variable("anchor_weights" + sid, [feature_size, anchor_size],
                           vs.random_normal_initializer(1 / math.sqrt(anchor_size)), device=device)


def _anchor_residuals(inputs, anchor_weights):
    """tile / subtract / reshape / l2_normalize(2) of :414-424 without the tile: [M, D], [D, K] -> [M, K, D], every (row, anchor)
    block l2-normalised.  Anchor k is the k-th block of the flattened row (element k * D + d), the reference's transpose + reshape."""
    return layers.l2_normalize(inputs.unsqueeze(1) - anchor_weights.t().unsqueeze(0), 2)


class TriangulationEmbedding(modules.BaseModule):
    """Triangulation embedding of every frame (:376-428): the unit vectors from each L2-normalised anchor column to the frame.
    This forward MATERIALISES [(B*T), D*K] -- the drop-in surface and the small-shape path; ops.triangulation_pool(scale=1) pools the
    same embedding (and its temporal differences) without it."""

    def __init__(self, feature_size, max_frames, anchor_size, batch_norm, is_training, scope_id=None):
        self.feature_size = feature_size
        self.max_frames = max_frames
        self.batch_norm = batch_norm
        self.anchor_size = int(anchor_size)
        self.is_training = is_training
        self.scope_id = scope_id

    def variables(self, device):
        """The L2-normalised anchors [D, K] (:401-410) without a forward: what the fused path needs."""
        anchor_weights = _anchor_weights(self.feature_size, self.anchor_size, self.scope_id, device)
        vs.summary("anchor_weights" + ("" if self.scope_id is None else str(self.scope_id)), anchor_weights)
        return layers.l2_normalize(anchor_weights, 0)                                              # :410

    def forward(self, inputs, **unused_params):
        """inputs [(B*max_frames), D] -> [(B*max_frames), D*K]."""
        anchor_weights = self.variables(inputs.device)
        t_emb = _anchor_residuals(inputs, anchor_weights)                                          # :413-424
        return t_emb.reshape(-1, self.feature_size * self.anchor_size)


class TriangulationCnnModule(modules.BaseModule):
    """:1345-1392: a 1x1 convolution per anchor over every frame of a triangulation embedding -- ``cnn_weights`` [K, F, D],
    N(0, 1 / (F D)); no bias, no activation.  MATERIALISES [B, T, K*F] from a [(B*T), K*D] input: the drop-in surface and the CPU path;
    the map is linear, so ops.triangulation_cnn_pool applies it to the pooled means instead."""

    def __init__(self, feature_size, max_frames, num_filters, anchor_size, batch_norm, is_training, scope_id=None):
        self.feature_size = feature_size
        self.max_frames = max_frames
        self.batch_norm = batch_norm
        self.num_filters = int(num_filters)
        self.anchor_size = int(anchor_size)
        self.is_training = is_training
        self.scope_id = scope_id

    def variables(self, device):
        """``cnn_weights`` [K, F, D] without a forward: what the fused path needs."""
        return vs.get_variable("cnn_weights", [self.anchor_size, self.num_filters, self.feature_size],
                               vs.random_normal_initializer(1 / math.sqrt(self.num_filters * self.feature_size)), device=device)

    def forward(self, inputs, **unused_params):
        """inputs [(B*max_frames), D*K] (any leading shape with that many elements) -> [B, max_frames, K*F] (element k * F + j)."""
        cnn_weights = self.variables(inputs.device).transpose(1, 2)                                 # :1383 -> [K, D, F]
        reshaped_inputs = inputs.reshape(-1, self.anchor_size, self.feature_size).transpose(0, 1)   # :1386-1387 -> [K, B*T, D]
        output = reshaped_inputs.matmul(cnn_weights).transpose(0, 1)                                # :1388-1389 -> [B*T, K, F]
        return output.reshape(-1, self.max_frames, self.anchor_size * self.num_filters)


class WeightedTriangulationEmbedding(modules.BaseModule):
    """:1395-1459: the anchors enter as they are, and the whole row of K blocks is l2-normalised once more -- every block has unit
    norm, so that is a division by sqrt(K) (ops.triangulation_pool(scale=1/sqrt(K)); SURVEY App. C19 for the one case where it is
    not).  Returns ([B, T, D*K], det_reg); det_reg is identically 0 as written (``identity = tf.identity(det_reg)``, App. C18)."""

    def __init__(self, feature_size, max_frames, anchor_size, batch_norm, is_training, scope_id=None):
        self.feature_size = feature_size
        self.max_frames = max_frames
        self.batch_norm = batch_norm
        self.anchor_size = int(anchor_size)
        self.is_training = is_training
        self.det_reg = True
        self.det_reg_lambda = 1e-5
        self.scope_id = scope_id

    def variables(self, device):
        """(anchor_weights, det_reg) without a forward: what the fused path needs."""
        anchor_weights = _anchor_weights(self.feature_size, self.anchor_size, self.scope_id, device)
        vs.summary("anchor_weights" + ("" if self.scope_id is None else str(self.scope_id)), anchor_weights)
        det_reg = anchor_weights.new_zeros(()) if self.det_reg else None                           # :1431-1439: |A - identity(A)| = 0
        return anchor_weights, det_reg

    def forward(self, inputs, **unused_params):
        """inputs [(B*max_frames), D] -> ([B, max_frames, D*K], det_reg)."""
        anchor_weights, det_reg = self.variables(inputs.device)
        t_emb = _anchor_residuals(inputs, anchor_weights)                                          # :1442-1453
        t_emb = layers.l2_normalize(t_emb.reshape(-1, self.feature_size * self.anchor_size), 1)    # :1454-1455
        return t_emb.reshape(-1, self.max_frames, self.feature_size * self.anchor_size), det_reg


class TriangulationTemporalEmbedding(modules.BaseModule):
    """:1462-1497: the l2-normalised (per anchor block) difference of consecutive frames' embeddings.  The reference rolls the frame
    axis by one and deletes frame 0 afterwards: exactly the differences t = 1 .. T-1."""

    def __init__(self, feature_size, max_frames, anchor_size, batch_norm, is_training, scope_id=None):
        self.feature_size = feature_size
        self.max_frames = max_frames
        self.batch_norm = batch_norm
        self.anchor_size = int(anchor_size)
        self.is_training = is_training
        self.scope_id = scope_id

    def forward(self, inputs, **unused_params):
        """inputs [B, max_frames, D*K] (or [(B*max_frames), D*K]) -> [B, max_frames - 1, D*K]."""
        x = inputs.reshape(-1, self.max_frames, self.anchor_size, self.feature_size)
        temp_info = layers.l2_normalize(x[:, 1:] - x[:, :-1], 3)                                   # :1485-1490, frame 0 dropped (:1494-1496)
        return temp_info.reshape(-1, self.max_frames - 1, self.feature_size * self.anchor_size)
