"""NetVladOrthoReg and NetVladAttenCluster (reference: video_pooling_modules.py:1499-1586, 1589-1663) and the triangulation
embeddings (TriangulationEmbedding :376-428, WeightedTriangulationEmbedding :1395-1459, TriangulationTemporalEmbedding :1462-1497,
TriangulationV5Module :142-373, TriangulationCnnIndirectAttentionModule :431-631, TriangulationNsCnnIndirectAttentionModule :1108-1342,
TriangulationMagnitudeNsCnnIndirectAttentionModule :634-888, TriangulationMagnitudeNsCnnNetVladModule :891-1105,
TriangulationV6Module :39-138)."""
from __future__ import annotations

import math

import torch

from . import layers, loupe_modules, module_utils, modules, ops, transformer_utils
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


class TriangulationV5Module(modules.BaseModule):
    """:142-373 (JuhanTestModelV5's module): the triangulation embedding of every frame against the anchors AS THEY ARE (xavier, not
    normalised) and its "temporal" part -- ``tf.manip.roll(spatial, shift=1, axis=1)`` of the 2-D [(B*T), K*D] tensor rolls the FEATURE
    axis (:216): g[t,k,d] = e[t,k,d] - e[t,k,d-1] with e[t,k,-1] = e[t,(k-1) mod K, D-1], frame 0 dropped -- a 1x1
    convolution per anchor over each (``spatial_cnn_weights``, ``temporal_cnn_weights`` [K, F, D]), the two tf.norm columns appended, the
    mean and reduce_var over the frames, and per stream batch norm, two hidden layers with batch norm and relu, then the fusion layer.
    ``self_attention``, ``add_relu`` and ``scope_id``'s absence aside, the arguments are the reference's; ``self_attention`` and
    ``add_relu`` are stored and read nowhere (C30).  ``forward`` MATERIALISES [(B*T), K*D] twice: the drop-in surface and the CPU path;
    ``variables`` + ops.triangulation_cnn_moments + ``head`` is the fused one."""

    def __init__(self, feature_size, max_frames, anchor_size, self_attention, hidden_layer_size, kernel_size, output_dim, add_relu,
                 batch_norm, is_training, scope_id=None):
        self.feature_size = feature_size
        self.max_frames = max_frames
        self.anchor_size = int(anchor_size)
        self.self_attention = self_attention
        self.hidden_layer_size = int(hidden_layer_size)
        self.kernel_size = int(kernel_size)
        self.output_dim = int(output_dim)
        self.add_relu = add_relu
        self.batch_norm = batch_norm
        self.is_training = is_training
        self.scope_id = scope_id

    def variables(self, device):
        """(anchor_weights [D, K], spatial_cnn_weights, temporal_cnn_weights [K, F, D]) without a forward, created in the reference's
        order (:190-193, :238-247): what the fused path needs."""
        sid = "" if self.scope_id is None else str(self.scope_id)
        D, K, F = self.feature_size, self.anchor_size, self.kernel_size
        anchor_weights = vs.get_variable("anchor_weights" + sid, [D, K], vs.glorot_uniform_initializer(), device=device)
        vs.summary("anchor_weights" + sid, anchor_weights)
        spatial_cnn_weights = vs.get_variable("spatial_cnn_weights" + sid, [K, F, D], vs.glorot_uniform_initializer(), device=device)
        temporal_cnn_weights = vs.get_variable("temporal_cnn_weights" + sid, [K, F, D], vs.glorot_uniform_initializer(), device=device)
        return anchor_weights, spatial_cnn_weights, temporal_cnn_weights

    def pool(self, inputs):
        """inputs [(B*max_frames), D] -> (spatial_pool, temporal_pool), each [B, 2 (K*F + K)] (:198-276)."""
        D, K, F, T = self.feature_size, self.anchor_size, self.kernel_size, self.max_frames
        anchor_weights, spatial_cnn_weights, temporal_cnn_weights = self.variables(inputs.device)
        spatial = inputs.unsqueeze(1) - anchor_weights.t().unsqueeze(0)                                # :198-205 -> [M, K, D]
        spatial_norm = torch.linalg.vector_norm(spatial, dim=2)                                        # :206
        spatial = layers.l2_normalize(spatial, 2).reshape(-1, K * D)                                   # :208-209
        temporal = spatial - torch.roll(spatial, shifts=1, dims=1)                                     # :216-217: the feature axis (C29)
        temporal = temporal.reshape(-1, T, K * D)[:, 1:].reshape(-1, K, D)                             # :218-223
        temporal_norm = torch.linalg.vector_norm(temporal, dim=2)                                      # :224
        temporal = layers.l2_normalize(temporal, 2)                                                    # :225
        spatial = spatial.reshape(-1, K, D)
        spatial_output = spatial.transpose(0, 1).matmul(spatial_cnn_weights.transpose(1, 2)).transpose(0, 1)      # :249-258 -> [M, K, F]
        temporal_output = temporal.transpose(0, 1).matmul(temporal_cnn_weights.transpose(1, 2)).transpose(0, 1)
        spatial_output = torch.cat([spatial_output.reshape(-1, T, K * F), spatial_norm.reshape(-1, T, K)], 2)      # :261-267
        temporal_output = torch.cat([temporal_output.reshape(-1, T - 1, K * F), temporal_norm.reshape(-1, T - 1, K)], 2)
        spatial_pool = torch.cat([spatial_output.mean(dim=1), module_utils.reduce_var(spatial_output, 1)], 1)      # :269-276
        temporal_pool = torch.cat([temporal_output.mean(dim=1), module_utils.reduce_var(temporal_output, 1)], 1)
        return spatial_pool, temporal_pool

    def head(self, spatial_pool, temporal_pool):
        """The two pools -> [B, output_dim] (:278-373)."""
        dev, H = spatial_pool.device, self.hidden_layer_size

        def bn(x, scope):
            return layers.batch_norm(x, self.is_training, scope) if self.batch_norm else x

        def weights(name, rows, units):
            return vs.get_variable(name, [rows, units], vs.glorot_uniform_initializer(), device=dev)
        spatial_pool, temporal_pool = bn(spatial_pool, "spatial_pool_bn"), bn(temporal_pool, "temporal_pool_bn")            # :278-290
        spatial_weights = weights("spatial_hidden", spatial_pool.shape[1], H)                                            # :292-300
        temporal_weights = weights("temporal_hidden", temporal_pool.shape[1], H)
        spatial_activation, temporal_activation = spatial_pool.matmul(spatial_weights), temporal_pool.matmul(temporal_weights)
        spatial_activation = torch.relu(bn(spatial_activation, "spatial_activation_bn"))                                 # :305-321
        temporal_activation = torch.relu(bn(temporal_activation, "temporal_activation_bn"))
        spatial_weights2, temporal_weights2 = weights("spatial_hidden2", H, H), weights("temporal_hidden2", H, H)         # :323-329
        spatial_activation, temporal_activation = spatial_activation.matmul(spatial_weights2), temporal_activation.matmul(temporal_weights2)
        spatial_activation = torch.relu(bn(spatial_activation, "spatial_pool2_bn"))                                      # :334-349
        temporal_activation = torch.relu(bn(temporal_activation, "temporal_pool2_bn"))
        spatial_temporal_concat = torch.cat([spatial_activation, temporal_activation], 1)                                 # :354
        sp_weights = weights("spa_temp_fusion", spatial_temporal_concat.shape[1], self.output_dim)                        # :356-360
        return torch.relu(bn(spatial_temporal_concat.matmul(sp_weights), "st_fuse_activation_bn"))                        # :362-370

    def forward(self, inputs, **unused_params):
        """inputs [(B*max_frames), D] -> [B, output_dim]."""
        return self.head(*self.pool(inputs))


class TriangulationCnnIndirectAttentionModule(modules.BaseModule):
    """:431-631 (JuhanTestModelV1's module): the triangulation embedding of every frame against the anchors AS THEY ARE
    (random_normal(1 / sqrt(K)), not normalised), its difference with itself rolled by one along the FEATURE axis (:506; SURVEY App. C29;
    frame 0 dropped, not normalised again: C34), a batch norm over all K*D features of each (``spatial_bn`` over the B*T rows,
    ``temporal_bn`` over the B*(T-1) rows: C35), soft-attention weights from the relu'd Gram matrix of the normalised rows, the weighted
    mean divided by the frame count once more (C32) and the UNWEIGHTED reduce_var (C33) over the frames; then per stream a hidden layer,
    batch norm and relu, and the fusion layer.  ``pool`` MATERIALISES [(B*T), K*D] several times: the drop-in surface and the CPU path;
    ``variables`` + ops.triangulation_bn_moments + ``head`` is the fused one (``fused_pool``)."""

    def __init__(self, feature_size, max_frames, anchor_size, self_attention, hidden_layer_size, output_dim, add_relu, batch_norm,
                 is_training, scope_id=None):
        self.feature_size = feature_size
        self.max_frames = max_frames
        self.anchor_size = int(anchor_size)
        self.self_attention = self_attention
        self.hidden_layer_size = int(hidden_layer_size)
        self.output_dim = int(output_dim)
        self.add_relu = add_relu
        self.batch_norm = batch_norm
        self.is_training = is_training
        self.scope_id = scope_id

    def variables(self, device):
        """anchor_weights [D, K] without a forward (:476-482): what the fused path needs."""
        sid = "" if self.scope_id is None else str(self.scope_id)
        anchor_weights = vs.get_variable("anchor_weights" + sid, [self.feature_size, self.anchor_size],
                                         vs.random_normal_initializer(1 / math.sqrt(self.anchor_size)), device=device)
        vs.summary("anchor_weights" + sid, anchor_weights)
        return anchor_weights

    def pool(self, inputs):
        """inputs [(B*max_frames), D] -> (spatial_pool, temporal_pool), each [B, 2 K*D] (:476-571)."""
        D, K, T = self.feature_size, self.anchor_size, self.max_frames
        anchor_weights = self.variables(inputs.device)
        spatial = inputs.unsqueeze(1) - anchor_weights.t().unsqueeze(0)                                # :485-494 -> [M, K, D]
        spatial = layers.l2_normalize(spatial, 2).reshape(-1, K * D)                                   # :496-497
        temporal = spatial - torch.roll(spatial, shifts=1, dims=1)                                     # :506-507: the feature axis (C29)
        temporal = temporal.reshape(-1, T, K * D)[:, 1:].reshape(-1, K * D)                            # :508-513
        if self.batch_norm:                                                                            # :517-530
            spatial = layers.batch_norm(spatial, self.is_training, "spatial_bn")
            temporal = layers.batch_norm(temporal, self.is_training, "temporal_bn")
        pools = []
        for v in (spatial.reshape(-1, T, K * D), temporal.reshape(-1, T - 1, K * D)):                  # :533-571
            if self.self_attention:
                weight = torch.softmax(torch.relu(v.matmul(v.transpose(1, 2))).sum(dim=2), dim=1)      # :539-554
                mean = (v * weight.unsqueeze(2)).mean(dim=1)                                           # :561-562 (C32)
            else:
                mean = v.mean(dim=1)
            pools.append(torch.cat([mean, module_utils.reduce_var(v, 1)], 1))                          # :567-571 (C33)
        return pools[0], pools[1]

    def fused_pool(self, inputs):
        """``pool`` through ops.triangulation_bn_moments: the same variables in the same order, the moving averages updated from the op's
        batch statistics by layers.batch_norm's rank-2 rule (the unbiased estimate into the moving variance)."""
        T, J = self.max_frames, self.feature_size * self.anchor_size
        anchor_weights = self.variables(inputs.device)
        if not self.batch_norm:
            spatial_pool, temporal_pool, _ = ops.triangulation_bn_moments(inputs, anchor_weights, None, None, None, None, T,
                                                                          self_attention=self.self_attention, batch_norm=False)
            return spatial_pool, temporal_pool
        gamma_s, beta_s, mm_s, mv_s = layers.bn_variables("spatial_bn", J, inputs.device)
        gamma_t, beta_t, mm_t, mv_t = layers.bn_variables("temporal_bn", J, inputs.device)
        stats = None if self.is_training else (mm_s, mv_s, mm_t, mv_t)
        spatial_pool, temporal_pool, batch_stats = ops.triangulation_bn_moments(inputs, anchor_weights, gamma_s, beta_s, gamma_t, beta_t, T,
                                                                                self_attention=self.self_attention, stats=stats)
        if self.is_training:
            B = inputs.shape[0] // T
            with torch.no_grad():
                for mm, mv, mean, var, n in ((mm_s, mv_s, batch_stats[0], batch_stats[1], B * T),
                                             (mm_t, mv_t, batch_stats[2], batch_stats[3], B * (T - 1))):
                    mm.mul_(layers.BN_DECAY).add_(mean, alpha=1 - layers.BN_DECAY)
                    mv.mul_(layers.BN_DECAY).add_(var * (n / max(n - 1, 1)), alpha=1 - layers.BN_DECAY)
        return spatial_pool, temporal_pool

    def head(self, spatial_pool, temporal_pool):
        """The two pools -> [B, output_dim] (:573-631)."""
        dev, H = spatial_pool.device, self.hidden_layer_size

        def bn(x, scope):
            return layers.batch_norm(x, self.is_training, scope) if self.batch_norm else x

        def act(x):
            return torch.relu(x) if self.add_relu else x

        def weights(name, rows, units):
            return vs.get_variable(name, [rows, units], vs.random_normal_initializer(1 / math.sqrt(H)), device=dev)
        spatial_weights = weights("spatial_hidden", spatial_pool.shape[1], H)                                            # :573-583
        temporal_weights = weights("temporal_hidden", temporal_pool.shape[1], H)
        spatial_activation, temporal_activation = spatial_pool.matmul(spatial_weights), temporal_pool.matmul(temporal_weights)
        spatial_activation = act(bn(spatial_activation, "spatial_activation_bn"))                                        # :588-605
        temporal_activation = act(bn(temporal_activation, "temporal_activation_bn"))
        spatial_temporal_concat = torch.cat([spatial_activation, temporal_activation], 1)                                 # :610
        sp_weights = weights("spa_temp_fusion", spatial_temporal_concat.shape[1], self.output_dim)                        # :612-616
        return act(bn(spatial_temporal_concat.matmul(sp_weights), "activation_bn"))                                       # :617-628

    def forward(self, inputs, **unused_params):
        """inputs [(B*max_frames), D] -> [B, output_dim]."""
        return self.head(*self.pool(inputs))


class TriangulationNsCnnIndirectAttentionModule(modules.BaseModule):
    """:1108-1342 (JuhanTestModelV2's module): the triangulation embedding of every frame against the anchors AS THEY ARE
    (tf.orthogonal_initializer, not normalised), its difference with itself rolled by one along the FEATURE axis (:1185; SURVEY App. C29;
    frame 0 dropped, not normalised again: C34), a 1x1 convolution per anchor over each (``spatial_cnn_weights``, ``temporal_cnn_weights``
    [K, F, D], not shared between anchors), soft-attention weights over the frames of a clip from the relu'd Gram matrix of the [T, K*D]
    rows (C39: as written the Gram is taken per frame and the model raises), the weighted mean of the convolutions' results divided by the
    frame count once more (C32) and their UNWEIGHTED reduce_var (C33); then per stream a batch norm, a hidden layer, batch norm and an
    optional relu, and the fusion layer.  ``pool`` MATERIALISES [(B*T), K*D] several times: the drop-in surface and the CPU path;
    ``variables`` + ops.triangulation_cnn_attention_moments + ``head`` is the fused one (``fused_pool``)."""

    def __init__(self, feature_size, max_frames, anchor_size, self_attention, hidden_layer_size, kernel_size, output_dim, add_relu,
                 batch_norm, is_training, scope_id=None):
        self.feature_size = feature_size
        self.max_frames = max_frames
        self.anchor_size = int(anchor_size)
        self.self_attention = self_attention
        self.hidden_layer_size = int(hidden_layer_size)
        self.kernel_size = int(kernel_size)
        self.output_dim = int(output_dim)
        self.add_relu = add_relu
        self.batch_norm = batch_norm
        self.is_training = is_training
        self.scope_id = scope_id

    def variables(self, device):
        """(anchor_weights [D, K], spatial_cnn_weights, temporal_cnn_weights [K, F, D]) without a forward, created in the reference's
        order (:1156-1161, :1222-1235): what the fused path needs."""
        sid = "" if self.scope_id is None else str(self.scope_id)
        D, K, F = self.feature_size, self.anchor_size, self.kernel_size
        anchor_weights = vs.get_variable("anchor_weights" + sid, [D, K], vs.orthogonal_initializer(), device=device)
        vs.summary("anchor_weights" + sid, anchor_weights)
        init = vs.random_normal_initializer(1 / math.sqrt(F * D))
        spatial_cnn_weights = vs.get_variable("spatial_cnn_weights" + sid, [K, F, D], init, device=device)
        temporal_cnn_weights = vs.get_variable("temporal_cnn_weights" + sid, [K, F, D], init, device=device)
        return anchor_weights, spatial_cnn_weights, temporal_cnn_weights

    def pool(self, inputs):
        """inputs [(B*max_frames), D] -> (spatial_pool, temporal_pool), each [B, 2 K*F] (:1156-1268)."""
        D, K, F, T = self.feature_size, self.anchor_size, self.kernel_size, self.max_frames
        anchor_weights, spatial_cnn_weights, temporal_cnn_weights = self.variables(inputs.device)
        spatial = inputs.unsqueeze(1) - anchor_weights.t().unsqueeze(0)                                # :1164-1173 -> [M, K, D]
        spatial = layers.l2_normalize(spatial, 2).reshape(-1, K * D)                                   # :1175-1176
        temporal = spatial - torch.roll(spatial, shifts=1, dims=1)                                     # :1185-1186: the feature axis (C29)
        temporal = temporal.reshape(-1, T, K * D)[:, 1:].reshape(-1, K * D)                            # :1187-1192
        pools = []
        for v, cnn, Tz in ((spatial, spatial_cnn_weights, T), (temporal, temporal_cnn_weights, T - 1)):
            out = v.reshape(-1, K, D).transpose(0, 1).matmul(cnn.transpose(1, 2)).transpose(0, 1).reshape(-1, Tz, K * F)   # :1237-1254
            if self.self_attention:
                v = v.reshape(-1, Tz, K * D)                                                           # (C39: the frames of a clip)
                weight = torch.softmax(torch.relu(v.matmul(v.transpose(1, 2))).sum(dim=2), dim=1)      # :1201-1216
                mean = (out * weight.unsqueeze(2)).mean(dim=1)                                         # :1258-1259 (C32)
            else:
                mean = out.mean(dim=1)                                                                 # :1261-1262
            pools.append(torch.cat([mean, module_utils.reduce_var(out, 1)], 1))                        # :1264-1268 (C33)
        return pools[0], pools[1]

    def fused_pool(self, inputs):
        """``pool`` through ops.triangulation_cnn_attention_moments: the same variables in the same order."""
        anchor_weights, spatial_cnn_weights, temporal_cnn_weights = self.variables(inputs.device)
        return ops.triangulation_cnn_attention_moments(inputs, anchor_weights, spatial_cnn_weights, temporal_cnn_weights, self.max_frames,
                                                       self_attention=bool(self.self_attention))

    def head(self, spatial_pool, temporal_pool):
        """The two pools -> [B, output_dim] (:1270-1342)."""
        dev, H = spatial_pool.device, self.hidden_layer_size

        def bn(x, scope):
            return layers.batch_norm(x, self.is_training, scope) if self.batch_norm else x

        def act(x):
            return torch.relu(x) if self.add_relu else x

        def weights(name, rows, units, fan):
            return vs.get_variable(name, [rows, units], vs.random_normal_initializer(1 / math.sqrt(fan)), device=dev)
        spatial_pool, temporal_pool = bn(spatial_pool, "spatial_pool_bn"), bn(temporal_pool, "temporal_pool_bn")            # :1270-1282
        spatial_weights = weights("spatial_hidden", spatial_pool.shape[1], H, H)                                         # :1284-1294
        temporal_weights = weights("temporal_hidden", temporal_pool.shape[1], H, H)
        spatial_activation, temporal_activation = spatial_pool.matmul(spatial_weights), temporal_pool.matmul(temporal_weights)
        spatial_activation = act(bn(spatial_activation, "spatial_activation_bn"))                                        # :1299-1316
        temporal_activation = act(bn(temporal_activation, "temporal_activation_bn"))
        spatial_temporal_concat = torch.cat([spatial_activation, temporal_activation], 1)                                 # :1321
        sp_weights = weights("spa_temp_fusion", spatial_temporal_concat.shape[1], self.output_dim, self.output_dim)       # :1323-1328
        return act(bn(spatial_temporal_concat.matmul(sp_weights), "activation_bn"))                                       # :1330-1339

    def forward(self, inputs, **unused_params):
        """inputs [(B*max_frames), D] -> [B, output_dim]."""
        return self.head(*self.pool(inputs))


class TriangulationMagnitudeNsCnnIndirectAttentionModule(TriangulationNsCnnIndirectAttentionModule):
    """:634-888 (JuhanTestModelV3's module), "non-sharing CNN / magnitude preserving": TriangulationNsCnnIndirectAttentionModule with the
    rolled difference normalised again per anchor (:732; C34 does not hold here), the attention Gram of the temporal stream taken of
    those normalised rows (C39's resolution: over the frames of a clip), a relu on both convolutions' results before they are pooled
    (:793-794) and, with ``add_norm``, the two tf.norm columns |x - a_k| and |g_k| appended to them (:799-801), so the weighted mean
    (C32) and the unweighted reduce_var (C33) are of [relu(conv) | norm], K*F + K columns.  The variables and the head are the sibling's,
    the two ``*_hidden`` matrices with 2 (K*F + K) rows.  ``pool`` MATERIALISES [(B*T), K*D] several times: the drop-in surface and the
    CPU path; ``variables`` + ops.triangulation_magnitude_moments + ``head`` is the fused one (``fused_pool``)."""

    def __init__(self, feature_size, max_frames, anchor_size, self_attention, hidden_layer_size, kernel_size, output_dim, add_relu,
                 add_norm, batch_norm, is_training, scope_id=None):
        super().__init__(feature_size, max_frames, anchor_size, self_attention, hidden_layer_size, kernel_size, output_dim, add_relu,
                         batch_norm, is_training, scope_id)
        self.add_norm = add_norm

    def _features(self, inputs, add_norm):
        """inputs [(B*max_frames), D] -> per stream (out [B, T', K*F + K] = [relu(conv) | norm] (K*F columns without ``add_norm``), the
        normalised embedding [(B*T'), K*D]); T' = T and T - 1 (:684-801).  Shared with TriangulationMagnitudeNsCnnNetVladModule.frames."""
        D, K, F, T = self.feature_size, self.anchor_size, self.kernel_size, self.max_frames
        anchor_weights, spatial_cnn_weights, temporal_cnn_weights = self.variables(inputs.device)
        spatial = inputs.unsqueeze(1) - anchor_weights.t().unsqueeze(0)                                # :692-701 -> [M, K, D]
        spatial_norm = torch.linalg.vector_norm(spatial, dim=2)                                        # :702
        spatial = layers.l2_normalize(spatial, 2).reshape(-1, K * D)                                   # :706-707
        temporal = spatial - torch.roll(spatial, shifts=1, dims=1)                                     # :718-719: the feature axis (C29)
        temporal = temporal.reshape(-1, T, K * D)[:, 1:].reshape(-1, K, D)                             # :720-725
        temporal_norm = torch.linalg.vector_norm(temporal, dim=2)                                      # :726
        temporal = layers.l2_normalize(temporal, 2).reshape(-1, K * D)                                 # :732
        streams = []
        for v, norm, cnn, Tz in ((spatial, spatial_norm, spatial_cnn_weights, T), (temporal, temporal_norm, temporal_cnn_weights, T - 1)):
            out = v.reshape(-1, K, D).transpose(0, 1).matmul(cnn.transpose(1, 2)).transpose(0, 1).reshape(-1, Tz, K * F)   # :777-791
            out = torch.relu(out)                                                                      # :793-794
            if add_norm:
                out = torch.cat([out, norm.reshape(-1, Tz, K)], 2)                                     # :799-801
            streams.append((out, v))
        return streams

    def pool(self, inputs):
        """inputs [(B*max_frames), D] -> (spatial_pool, temporal_pool), each [B, 2 (K*F + K)] (2 K*F without ``add_norm``; :684-814)."""
        K, D, T = self.anchor_size, self.feature_size, self.max_frames
        pools = []
        for (out, v), Tz in zip(self._features(inputs, self.add_norm), (T, T - 1)):
            if self.self_attention:
                v = v.reshape(-1, Tz, K * D)                                                           # (C39: the frames of a clip)
                weight = torch.softmax(torch.relu(v.matmul(v.transpose(1, 2))).sum(dim=2), dim=1)      # :741-756
                mean = (out * weight.unsqueeze(2)).mean(dim=1)                                         # :804-805 (C32)
            else:
                mean = out.mean(dim=1)                                                                 # :807-808
            pools.append(torch.cat([mean, module_utils.reduce_var(out, 1)], 1))                        # :810-814 (C33)
        return pools[0], pools[1]

    def fused_pool(self, inputs):
        """``pool`` through ops.triangulation_magnitude_moments: the same variables in the same order."""
        anchor_weights, spatial_cnn_weights, temporal_cnn_weights = self.variables(inputs.device)
        return ops.triangulation_magnitude_moments(inputs, anchor_weights, spatial_cnn_weights, temporal_cnn_weights, self.max_frames,
                                                   self_attention=bool(self.self_attention), add_norm=bool(self.add_norm))


class TriangulationMagnitudeNsCnnNetVladModule(TriangulationMagnitudeNsCnnIndirectAttentionModule):
    """:891-1105 (JuhanTestModelV4's module): the sibling's front end -- the twice-normalised embedding, the rectified per-anchor
    convolutions and the two norm columns -- handed PER FRAME to a ``loupe_modules.NetVLAD`` per stream (scopes ``spatial_vlad`` and
    ``temporal_vlad``, max_samples T and T - 1, ``cluster_size`` clusters: 256 as written, :1043) in place of the moments and the hidden
    layers; then the sibling's batch norms, optional relu and fusion layer.  As written ``self_attention`` and ``add_norm`` are taken and
    never read: there is no Gram, and the norm columns are always appended.  ``frames`` MATERIALISES [(B*T), K*D] several
    times: the drop-in surface and the CPU path; ``fused_frames`` (ops.triangulation_magnitude_frames) + ``head`` is the fused one."""

    def __init__(self, feature_size, max_frames, anchor_size, self_attention, hidden_layer_size, kernel_size, output_dim, add_relu,
                 add_norm, batch_norm, is_training, scope_id=None, cluster_size=256):
        super().__init__(feature_size, max_frames, anchor_size, self_attention, hidden_layer_size, kernel_size, output_dim, add_relu,
                         add_norm, batch_norm, is_training, scope_id)
        self.cluster_size = int(cluster_size)

    def frames(self, inputs):
        """inputs [(B*max_frames), D] -> (spatial_output [(B*T), K*F + K], temporal_output [(B*(T-1)), K*F + K]) (:938-1039)."""
        W = self.anchor_size * self.kernel_size + self.anchor_size
        (out_s, _), (out_t, _) = self._features(inputs, True)
        return out_s.reshape(-1, W), out_t.reshape(-1, W)

    def fused_frames(self, inputs):
        """``frames`` through ops.triangulation_magnitude_frames: the same variables in the same order.  The rows come zero-padded to the
        width loupe_modules.NetVLAD hands to ops.netvlad (loupe_modules.padded_size), when it will."""
        anchor_weights, spatial_cnn_weights, temporal_cnn_weights = self.variables(inputs.device)
        W, T = self.anchor_size * self.kernel_size + self.anchor_size, self.max_frames
        pad = all(loupe_modules.fused_ok(Tz, W, self.cluster_size) for Tz in (T, T - 1))
        return ops.triangulation_magnitude_frames(inputs, anchor_weights, spatial_cnn_weights, temporal_cnn_weights, T,
                                                  pad_to=loupe_modules.padded_size(W, self.cluster_size) if pad else 1)

    def pool(self, inputs):
        raise NotImplementedError("TriangulationMagnitudeNsCnnNetVladModule pools with NetVLAD: frames / fused_frames + head")

    fused_pool = pool

    def head(self, spatial_output, temporal_output):
        """The two streams' per-frame rows -> [B, output_dim] (:1040-1105)."""
        dev, T = spatial_output.device, self.max_frames
        W = self.anchor_size * self.kernel_size + self.anchor_size

        def bn(x, scope):
            return layers.batch_norm(x, self.is_training, scope) if self.batch_norm else x

        def act(x):
            return torch.relu(x) if self.add_relu else x
        spatial_vlad, temporal_vlad = (loupe_modules.NetVLAD(feature_size=W, max_samples=Tz, cluster_size=self.cluster_size,
                                                             output_dim=self.hidden_layer_size, gating=False,
                                                             add_batch_norm=self.batch_norm, is_training=self.is_training)
                                       for Tz in (T, T - 1))                                                              # :1041-1055
        with vs.variable_scope("spatial_vlad"):
            spatial_agg = spatial_vlad.forward(spatial_output)                                                           # :1056-1057
        with vs.variable_scope("temporal_vlad"):
            temporal_agg = temporal_vlad.forward(temporal_output)                                                        # :1059-1060
        spatial_agg = act(bn(spatial_agg, "spatial_activation_bn"))                                                      # :1062-1079
        temporal_agg = act(bn(temporal_agg, "temporal_activation_bn"))
        spatial_temporal_concat = torch.cat([spatial_agg, temporal_agg], 1)                                              # :1084
        sp_weights = vs.get_variable("spa_temp_fusion", [spatial_temporal_concat.shape[1], self.output_dim],
                                     vs.random_normal_initializer(1 / math.sqrt(self.output_dim)), device=dev)           # :1086-1091
        return act(bn(spatial_temporal_concat.matmul(sp_weights), "activation_bn"))                                      # :1093-1102

    def forward(self, inputs, **unused_params):
        """inputs [(B*max_frames), D] -> [B, output_dim]."""
        return self.head(*self.frames(inputs))


class TriangulationV6Module(modules.BaseModule):
    """:39-138 (JuhanTestModelV6's module): the triangulation embedding of every frame against the anchors AS THEY ARE (xavier, not
    normalised), normalised once more over the whole flattened [K*D] row (:106: e / sqrt(K) unless a norm was clamped), a batch norm over
    all K*D features (``spatial_bn``), then attention_modules.OneFcAttention(K*D, max_frames, cluster_size, do_shift=True): a softmax
    over the FRAMES of (1 / sqrt(K*D)) v W, the C weighted sums of the frames, ``alpha`` * . + ``beta``, an l2 normalisation of each
    cluster's row and 1 / sqrt(C); then one matrix ``hidden_weight`` [C*K*D, output_dim], batch norm (``spatial_pool2_bn``) and relu.
    ``self_attention``, ``hidden_layer_size``, ``kernel_size`` and ``add_relu`` are stored and read nowhere, as written.
    ``pool`` MATERIALISES [(B*T), K*D] five times: the drop-in surface, the CPU path and the unfused GPU path; it creates OneFcAttention's
    three variables itself under the reference's names (attention_modules.OneFcAttention's K2 route is GPU-only, limited in width, and
    gives nan at alpha == 0: C49).  ``fused_pool`` is ops.triangulation_onefc_pool with the same variables in the same order."""

    def __init__(self, feature_size, max_frames, anchor_size, self_attention, hidden_layer_size, kernel_size, output_dim, cluster_size,
                 add_relu, batch_norm, is_training, scope_id=None):
        self.feature_size = feature_size
        self.max_frames = max_frames
        self.anchor_size = int(anchor_size)
        self.self_attention = self_attention
        self.hidden_layer_size = hidden_layer_size
        self.kernel_size = kernel_size
        self.output_dim = int(output_dim)
        self.add_relu = add_relu
        self.cluster_size = int(cluster_size)
        self.batch_norm = batch_norm
        self.is_training = is_training
        self.scope_id = scope_id

    def variables(self, device):
        """anchor_weights [D, K] without a forward (:86-91)."""
        sid = "" if self.scope_id is None else str(self.scope_id)
        anchor_weights = vs.get_variable("anchor_weights" + sid, [self.feature_size, self.anchor_size], vs.glorot_uniform_initializer(),
                                         device=device)
        vs.summary("anchor_weights" + sid, anchor_weights)
        return anchor_weights

    def attention_variables(self, device):
        """OneFcAttention's (one_fc_attention_weight [K*D, C], alpha [1] = 1, beta [1] = 0.01), in its order (attention_modules.py:30-54)."""
        J = self.feature_size * self.anchor_size
        weight = vs.get_variable("one_fc_attention_weight", [J, self.cluster_size], vs.glorot_uniform_initializer(), device=device)
        alpha = vs.get_variable("alpha", [1], lambda shape, d, gen: torch.full(shape, 1.0, device=d), device=device)
        beta = vs.get_variable("beta", [1], lambda shape, d, gen: torch.full(shape, 0.01, device=d), device=device)
        return weight, alpha, beta

    def pool(self, inputs):
        """inputs [(B*max_frames), D] -> [B, C * K*D] cluster-major (:86-119)."""
        D, K, C, T = self.feature_size, self.anchor_size, self.cluster_size, self.max_frames
        J = K * D
        anchor_weights = self.variables(inputs.device)
        spatial = inputs.unsqueeze(1) - anchor_weights.t().unsqueeze(0)                                # :94-101 -> [M, K, D]
        spatial = layers.l2_normalize(spatial, 2).reshape(-1, J)                                       # :104-105
        spatial = layers.l2_normalize(spatial, 1)                                                      # :106
        if self.batch_norm:
            spatial = layers.batch_norm(spatial, self.is_training, "spatial_bn")                       # :108-114
        weight, alpha, beta = self.attention_variables(inputs.device)
        attention = spatial.matmul(weight).reshape(-1, T, C) * (1 / math.sqrt(J))                      # attention_modules.py:34-36
        attention = torch.softmax(attention, dim=1)                                                    # :37: over the frames
        activation = attention.transpose(1, 2).matmul(spatial.reshape(-1, T, J)).reshape(-1, J)        # :39-44
        activation = layers.l2_normalize(alpha * activation + beta, 1) * (1 / math.sqrt(C))            # :56-59
        return activation.reshape(-1, C * J)                                                           # :61

    def fused_pool(self, inputs):
        """``pool`` through ops.triangulation_onefc_pool: the same variables in the same order, the moving averages updated from the op's
        batch statistics by layers.batch_norm's rank-2 rule (the unbiased estimate into the moving variance)."""
        T, J = self.max_frames, self.feature_size * self.anchor_size
        anchor_weights = self.variables(inputs.device)
        gamma = beta_bn = stats = mm = mv = None
        if self.batch_norm:
            gamma, beta_bn, mm, mv = layers.bn_variables("spatial_bn", J, inputs.device)
            stats = None if self.is_training else (mm, mv)
        weight, alpha, beta = self.attention_variables(inputs.device)
        pooled, batch_stats = ops.triangulation_onefc_pool(inputs, anchor_weights, gamma, beta_bn, weight, alpha, beta, T,
                                                           batch_norm=bool(self.batch_norm), stats=stats)
        if self.batch_norm and self.is_training:
            n = inputs.shape[0]
            with torch.no_grad():
                mm.mul_(layers.BN_DECAY).add_(batch_stats[0], alpha=1 - layers.BN_DECAY)
                mv.mul_(layers.BN_DECAY).add_(batch_stats[1] * (n / max(n - 1, 1)), alpha=1 - layers.BN_DECAY)
        return pooled

    def head(self, pooled):
        """[B, C * K*D] -> [B, output_dim] (:121-136)."""
        hidden_weight = vs.get_variable("hidden_weight", [pooled.shape[1], self.output_dim], vs.glorot_uniform_initializer(),
                                        device=pooled.device)
        spatial_activation = pooled.matmul(hidden_weight)
        if self.batch_norm:
            spatial_activation = layers.batch_norm(spatial_activation, self.is_training, "spatial_pool2_bn")
        return torch.relu(spatial_activation)

    def forward(self, inputs, **unused_params):
        """inputs [(B*max_frames), D] -> [B, output_dim]."""
        return self.head(self.pool(inputs))
