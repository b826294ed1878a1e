"""NetVLAD prototypes behind the reference's model-registry API
(reference: frame_level_models.py:2193-2513 NetVladV1 / NetVladV2, :2765-2877 NetVLAD / LightVLAD) and the triangulation-embedding
family's RegularizedTriangulationModel (:1148-1307), SoftAttentionTriangulationModel (:965-1145), TriangulationCnnClusterModel
(:757-939), JuhanTestModelV5 (:491-606), JuhanTestModelV1 (:59-154), JuhanTestModelV2 (:158-268), JuhanTestModelV3 (:302-378), JuhanTestModelV4 (:411-487), JuhanTestModelV6 (:638-733) and the recurrent TriangulationRelationalModel (:1511-1630).

Same names, ``create_model`` signature, variable names and output contract as the reference; the hot
ops (frame sampling + input_bn, soft-assignment GEMM, fused softmax/residual aggregation/normalise,
attention cores) run as hand-written gfx950 kernels through ops.py.  Defect resolutions follow
SURVEY.md App. C (C1 scope_id ignored, C5 tokens = clusters, C8 K // 4, C9 rgb-only input skips audio).
"""
from __future__ import annotations

import contextlib
import math
import os

import torch

from . import FLAGS, aggregation_modules, layers, model_utils, models, ops, transformer_utils, video_level_models, video_pooling_modules
from . import variables as vs
from ._capi import LpmError


class NetVLAD():
    """frame_level_models.py:2765-2824.  forward(reshaped_input [(B*max_frames), D]) -> [B, D*K] (d-major)."""

    residual = True

    def __init__(self, feature_size, max_frames, cluster_size, add_batch_norm, is_training, scope_id=None):
        self.feature_size = feature_size
        self.max_frames = max_frames
        self.is_training = is_training
        self.add_batch_norm = add_batch_norm
        self.cluster_size = int(cluster_size)

    def forward(self, reshaped_input, kmajor=False, input_affine=None, storage="f32", lazy=False, out_slot=None):
        """input_affine: (gamma, beta) slices of input_bn when reshaped_input is its (gradient-free) output, see ops.netvlad.
        lazy: hand the k-major descriptor over lazily normalised (ops.netvlad) -- for a consumer that applies the row scale."""
        D, K, dev = self.feature_size, self.cluster_size, reshaped_input.device
        std = 1 / math.sqrt(D)
        cluster_weights = vs.get_variable("cluster_weights", [D, K], vs.random_normal_initializer(std), device=dev)   # :2775
        bn = bias = None
        if self.add_batch_norm:
            bn = layers.bn_variables("cluster_bn", K, dev)                                                          # :2783-2789
        else:
            bias = vs.get_variable("cluster_biases", [K], vs.random_normal_initializer(std), device=dev)            # :2790-2796
        cluster_weights2 = None
        if self.residual:
            cluster_weights2 = vs.get_variable("cluster_weights2", [1, D, K], vs.random_normal_initializer(std),
                                               device=dev)                                                           # :2805-2808
        # matmul -> cluster_bn -> softmax -> a^T x - sum(a) W2 -> l2norm(D) -> flatten -> l2norm  (:2781-2822)
        return ops.netvlad(reshaped_input, cluster_weights, cluster_weights2, self.max_frames, bn=bn, bias=bias,
                           is_training=self.is_training, kmajor=kmajor, input_affine=input_affine, storage=storage, lazy=lazy,
                           out_slot=out_slot)


class LightVLAD(NetVLAD):
    """frame_level_models.py:2827-2877: NetVLAD without the centre-residual term."""
    residual = False


def _project_gate_classify(vlad, vocab_size, cluster_size, hidden1_size, add_batch_norm, relu, gating, remove_diag,
                           is_training, **unused_params):
    """Shared tail of NetVladV1 / NetVladV2: hidden projection, context gating, MoE
    (frame_level_models.py:2309-2377 == :2445-2513)."""
    # vlad = (video, audio | None): the video stream's descriptor LAZILY normalised (ops.vlad_aggregate(lazy=True)) and the concat left to
    # the projection, which reads both blocks where they are (ops.projection_parts)
    parts = vlad if isinstance(vlad, tuple) else None
    dev = parts[0].device if parts else vlad.device
    vlad_dim = sum(p.shape[1] for p in parts if p is not None) if parts else vlad.shape[1]
    hidden1_weights = vs.get_variable("hidden1_weights", [vlad_dim, hidden1_size],
                                      vs.random_normal_initializer(1 / math.sqrt(cluster_size)), device=dev)   # :2315-2317
    if parts and ops.projection_parts_ok(getattr(parts[0], "_lpm_raw", parts[0]), ops.row_scale_of(parts[0]),
                                         getattr(parts[0], "_lpm_scale_ks", 0), parts[1], hidden1_weights):
        activation = ops.projection_parts(parts[0], parts[1], hidden1_weights)                                 # :2309 / :2445 + :2319
    else:
        if parts:
            vlad = ops.materialise(parts[0])
            vlad = torch.cat([vlad, parts[1]], 1) if parts[1] is not None else vlad
        activation = ops.projection(vlad, hidden1_weights) if vlad.is_cuda else vlad.matmul(hidden1_weights)  # :2319
    small = is_training and ops.bn_small_ok(activation)         # clip-level tensors: batch norm + what follows it in one launch each way
    if add_batch_norm and relu and small:
        activation = ops.bn_small(activation, *layers.bn_variables("hidden1_bn", hidden1_size, dev), act=1)    # :2321-2327 + relu6 :2337
    elif add_batch_norm and relu:
        activation = layers.batch_norm(activation, is_training, "hidden1_bn")                                  # :2321-2327
    else:
        hidden1_biases = vs.get_variable("hidden1_biases", [hidden1_size], vs.random_normal_initializer(0.01), device=dev)
        activation = activation + hidden1_biases                                                               # :2329-2334
    if relu and not (add_batch_norm and small):
        activation = torch.clamp(activation, 0.0, 6.0)                                                         # relu6 :2337
    if gating:
        gating_weights = vs.get_variable("gating_weights_2", [hidden1_size, hidden1_size],
                                         vs.random_normal_initializer(1 / math.sqrt(hidden1_size)), device=dev)  # :2343-2346
        gates = activation.matmul(gating_weights)
        if remove_diag:
            gates = gates - torch.diagonal(gating_weights) * activation                                        # :2349-2352
        if not add_batch_norm:
            raise NotImplementedError("context gating without batch norm is broken in the reference (App. C12)")
        if small:
            activation = ops.bn_small(gates, *layers.bn_variables("gating_bn", hidden1_size, dev), act=2, mul=activation)   # :2354-2368
        else:
            gates = layers.batch_norm(gates, is_training, "gating_bn")                                         # :2354-2360
            activation = activation * torch.sigmoid(gates)                                                     # :2367-2368
    vs.summary("activation", activation)
    aggregated_model = getattr(video_level_models, "MoeModel")
    return aggregated_model().create_model(model_input=activation, vocab_size=vocab_size, is_training=is_training,
                                           **unused_params)


class _GammaWatch:
    """The closed-form input_bn gradients divide by gamma (ops._NetVLAD.backward): fine while |gamma| is O(1), inaccurate once an
    element comes within rounding of zero.  This watch keeps min |gamma| under observation WITHOUT stalling the step: a tiny
    reduction + a 4-byte copy into pinned memory every ``EVERY`` calls, read back once its event has completed; below
    ``FLOOR`` the model falls back, for good, to the explicit input-gradient path (same result, ~0.19 ms/step more)."""
    EVERY, FLOOR = 8, 0.2

    def __init__(self):
        self.disabled, self.count, self.pending, self.host = False, 0, None, None

    def ok(self, gamma):
        if self.disabled:
            return False
        if self.count == 0:                                    # first use (fresh or restored weights): decide synchronously, once
            self._decide(float(gamma.detach().abs().min()))
        elif self.pending is not None and self.pending.query():
            self.pending = None
            self._decide(float(self.host))
        if not self.disabled and self.pending is None and self.count % self.EVERY == 0 and self.count > 0:
            if self.host is None:
                self.host = torch.empty((), dtype=torch.float32).pin_memory()
            self.host.copy_(gamma.detach().abs().min(), non_blocking=True)
            self.pending = torch.cuda.Event()
            self.pending.record()
        self.count += 1
        return not self.disabled

    def _decide(self, min_abs_gamma):
        if not (min_abs_gamma >= self.FLOOR):                  # also catches NaN
            import warnings
            self.disabled = True
            warnings.warn(f"input_bn: min |gamma| = {min_abs_gamma:.3g} < {self.FLOOR}: the closed-form gamma / beta gradients are "
                          "switched off, the input gradient is formed explicitly from now on")


def _sample_and_normalise(model_input, num_frames, iterations, add_batch_norm, is_training, storage="f32", quantised_training=False):
    """SampleUniformFrames + reshape + input_bn (frame_level_models.py:2248-2271), one fused kernel pair.  quantised_training: uint8
    frames (the reader's batch) are accepted in training mode too (ops.frame_sample_bn)."""
    bn = layers.bn_variables("input_bn", model_input.shape[2], model_input.device) if add_batch_norm else (None,) * 4
    # bf16 storage: the fp32 matrix itself is only filled in when summaries are being collected (nothing else reads it)
    return ops.frame_sample_bn(model_input, num_frames.reshape(-1), iterations, *bn, is_training=is_training, storage=storage,
                               materialize=storage == "f32" or vs.default_store().summaries is not None,
                               quantised_training=quantised_training)


def _gather_and_normalise(model_input, num_frames, iterations, frame_uniform, bn_scopes, is_training, quantised_training):
    """The triangulation models' input stage from the reader's uint8 batch on the GPU: SampleRandomFrames' index table
    (model_utils.random_frame_index) + ops.frame_gather_bn_split -> (video [B*S, 1024], audio [B*S, F - 1024]), contiguous.  bn_scopes:
    ("input_bn",) one batch norm over [F]; ("video_bn", "audio_bn") one per stream -- their variables concatenated for the kernels, which
    treat every column alone, and the moving statistics bn_fold updated copied back into each scope; (): no batch norm."""
    if not model_input.is_cuda:
        raise LpmError("uint8 (quantised) frames reach this model on the GPU only: on the CPU normalise them first (train.normalize_input)")
    dev, feature_size = model_input.device, model_input.shape[2]
    nf = num_frames.reshape(-1).to(dev)
    frame_index = model_utils.random_frame_index(nf, iterations, uniform=frame_uniform)
    widths = (feature_size,) if len(bn_scopes) == 1 else (1024, feature_size - 1024)
    parts = [layers.bn_variables(scope, width, dev) for scope, width in zip(bn_scopes, widths)]
    if len(parts) == 2:
        bn = [torch.cat(pair) for pair in zip(*parts)]                    # gamma, beta, moving_mean, moving_variance over [F]
    else:
        bn = list(parts[0]) if parts else [None] * 4
    video, audio = ops.frame_gather_bn_split(model_input, nf, frame_index, *bn, is_training, 1024, quantised_training)
    if len(parts) == 2 and is_training:
        with torch.no_grad():
            for (_, _, mm, mv), cols in zip(parts, (slice(0, 1024), slice(1024, None))):
                mm.copy_(bn[2][cols])
                mv.copy_(bn[3][cols])
    return video, audio


def _random_frames(model_input, num_frames, iterations, frame_uniform):
    """-> (quantised, frames, max_frames, feature_size): SampleRandomFrames of fp32 frames; a uint8 batch stays as it is for
    _gather_and_normalise, which samples where it reads."""
    if model_input.dtype == torch.uint8:
        return True, model_input, iterations, model_input.shape[2]
    model_input = model_utils.SampleRandomFrames(model_input, num_frames.reshape(-1, 1), iterations, uniform=frame_uniform)
    return False, model_input, model_input.shape[1], model_input.shape[2]


def _stream_features(quantised, model_input, num_frames, iterations, frame_uniform, add_batch_norm, is_training, quantised_training):
    """-> [video [B*S, 1024], audio [B*S, F - 1024]] behind the scopes video_bn / audio_bn (add_batch_norm): column slices of the sampled
    fp32 frames through layers.batch_norm, or (a uint8 batch) two contiguous matrices from _gather_and_normalise."""
    if quantised:
        scopes = ("video_bn", "audio_bn") if add_batch_norm else ()
        return list(_gather_and_normalise(model_input, num_frames, iterations, frame_uniform, scopes, is_training, quantised_training))
    reshaped_input = model_input.reshape(-1, model_input.shape[2])
    features = []
    for name, cols in (("video", slice(0, 1024)), ("audio", slice(1024, None))):
        x = reshaped_input[:, cols]
        features.append(layers.batch_norm(x, is_training, name + "_bn") if add_batch_norm else x)
    return features


class NetVladV1(models.BaseModel):
    """Paper prototype 1: NetVLAD -> cluster-level transformer encoders -> context gating -> MoE
    (frame_level_models.py:2222-2377)."""

    def create_model(self, model_input, vocab_size, num_frames, iterations=None, add_batch_norm=None,
                     sample_random_frames=None, cluster_size=None, hidden_size=None, is_training=True, encoder=None,
                     quantised_training=False, **unused_params):
        iterations = iterations or FLAGS.iterations
        add_batch_norm = add_batch_norm or FLAGS.netvlad_add_batch_norm
        cluster_size = cluster_size or FLAGS.netvlad_cluster_size
        hidden1_size = hidden_size or FLAGS.netvlad_hidden_size
        relu, gating, remove_diag = FLAGS.netvlad_relu, FLAGS.gating, FLAGS.gating_remove_diag
        encoder = FLAGS.netvlad_encoder if encoder is None else encoder
        storage = FLAGS.netvlad_storage
        if storage == "bf16" and (encoder or not add_batch_norm or not model_input.is_cuda):
            raise ValueError("netvlad_storage='bf16' is the gated-NetVLAD configuration: netvlad_encoder off, batch norm on, on the GPU")

        max_frames, feature_size = iterations, model_input.shape[2]
        has_audio = feature_size > 1024                                      # App. C9
        shortcut = False
        if (FLAGS.input_bn_grad_shortcut and add_batch_norm and is_training and model_input.is_cuda and torch.is_grad_enabled()
                and ops.netvlad_input_shortcut_ok(max_frames, 1024, cluster_size)
                and (not has_audio or ops.netvlad_input_shortcut_ok(max_frames, 128, cluster_size // 4))):
            # the frames need no gradient of their own, only input_bn's gamma / beta do: the pooling ops take those as inputs and
            # return their gradients in closed form (ops._NetVLAD.backward); the [B*S, 1152] input gradient is never formed
            g_in, b_in, _, _ = layers.bn_variables("input_bn", feature_size, model_input.device)
            watch = getattr(g_in, "_lpm_gamma_watch", None)
            if watch is None:
                watch = g_in._lpm_gamma_watch = _GammaWatch()
            shortcut = watch.ok(g_in)
        if storage == "bf16" and is_training and torch.is_grad_enabled() and not shortcut:
            # bf16 storage writes the frames as operand tiles only and has no input-gradient path: once the closed-form input_bn
            # gradients are off (min |gamma| below the watch's floor, or the flag), this step runs with fp32 storage -- same model,
            # same variables, the explicit gradient path -- instead of reaching the pooling op with unmaterialised frames
            if not getattr(NetVladV1, "_warned_bf16_fallback", False):
                import warnings
                NetVladV1._warned_bf16_fallback = True
                warnings.warn("netvlad_storage='bf16': the closed-form input_bn gradients are unavailable; training steps fall "
                              "back to fp32 storage (explicit input-gradient path)")
            storage = "f32"

        reshaped_input = _sample_and_normalise(model_input, num_frames, iterations, add_batch_norm, is_training, storage, quantised_training)
        if storage == "f32" or vs.default_store().summaries is not None:
            vs.summary("input_bn", reshaped_input)

        video_NetVLAD = NetVLAD(1024, max_frames, cluster_size, add_batch_norm, is_training, "netvlad_rgb_scope")
        audio_NetVLAD = NetVLAD(128, max_frames, cluster_size // 4, add_batch_norm, is_training, "netvlad_audio_scope")
        aff_v = aff_a = None
        if shortcut:
            with torch.no_grad():
                rgb, audio = reshaped_input[:, 0:1024], reshaped_input[:, 1024:]
            if g_in.is_cuda and g_in.dim() == 1 and g_in.shape[0] > 1024:
                (gv, ga), (bv, ba) = ops.split_vector(g_in, 1024), ops.split_vector(b_in, 1024)
                aff_v, aff_a = (gv, bv), (ga, ba)
            else:
                aff_v, aff_a = (g_in[0:1024], b_in[0:1024]), (g_in[1024:], b_in[1024:])
        if aff_v is not None:
            pass
        elif has_audio and reshaped_input.is_cuda:
            rgb, audio = ops.split_columns(reshaped_input, 1024)      # the two slices, sharing one gradient buffer
        else:
            rgb, audio = reshaped_input[:, 0:1024], reshaped_input[:, 1024:]
        # the audio branch is ~100 small, latency-bound launches per step: it runs on a second stream beside the video branch
        # (variables are still created in the reference's order: video_VLAD, audio_VLAD, video_attention, audio_attention)
        use_side = has_audio and reshaped_input.is_cuda and FLAGS.audio_side_stream
        side = ops.side_stream(audio, reshaped_input) if use_side else contextlib.nullcontext()
        # The video descriptor goes to its cluster encoder LAZILY NORMALISED when that encoder will run as block Functions (they apply
        # the per-cluster scale where they read the rows): the pooling then writes the [B, K, D] tensor once and has no finalize pass.
        video_encoder_block = None
        if encoder:
            video_encoder_block = transformer_utils.TransformerEncoder(
                feature_size=1024, hidden_size=1024, num_heads=64, attention_dropout=0.1, ff_filter_size=4 * 1024,
                ff_relu_dropout=0.1, is_train=is_training, scope_id="encode1")
        batch = model_input.shape[0]
        lazy_v = bool(encoder and FLAGS.netvlad_lazy_descriptor and storage == "f32" and reshaped_input.is_cuda
                      and (aff_v is not None or not torch.is_grad_enabled())
                      and video_encoder_block.fused_shape(batch, cluster_size, True) and ops.netvlad_lazy_ok(max_frames, 1024, cluster_size))
        slots = None
        # bf16 storage without the cluster encoders (BASELINE configs[4]): the video descriptor LAZILY normalised -- the bf16 sums as the
        # aggregation kernel wrote them + one scale per (clip, cluster), applied by the projection where it reads them (no finalize pass:
        # that pass read the sums and wrote the fp32 descriptor, 0.4 GB per step at bs 128), the audio descriptor in an fp32 buffer of its own
        lazy5 = bool(storage == "bf16" and not encoder and has_audio and FLAGS.netvlad_lazy_descriptor and FLAGS.descriptor_slots
                     and aff_v is not None and batch <= 128 and hidden1_size % 512 == 0 and cluster_size % 32 == 0)
        if lazy5:
            slots = ops.DescriptorSlots(batch, [(1, 128 * (cluster_size // 4))], reshaped_input)
        elif (storage == "bf16" and not encoder and has_audio and FLAGS.descriptor_slots and aff_v is not None):
            # bf16 storage without the cluster encoders (BASELINE configs[4]): the projection behind the pooling computes in fp32, so the
            # two normalised descriptors leave their finalize passes as fp32 straight into ONE [B, 1024 K + 128 K/4] buffer -- no bf16
            # copy of the descriptor, no concat, no casts of it or of its gradient
            slots = ops.DescriptorSlots(batch, [(1, 1024 * cluster_size), (1, 128 * (cluster_size // 4))], reshaped_input)
        with vs.variable_scope("video_VLAD"):
            vlad_video = video_NetVLAD.forward(rgb, kmajor=encoder, input_affine=aff_v, storage=storage, lazy=lazy_v or lazy5,
                                               out_slot=slots.slots[0] if slots and not lazy5 else None)  # :2273-2274
            if vs.default_store().summaries is not None:
                # [B, K, D] (the App. C5 token view) when the encoders follow, else [B, D*K]
                vs.summary("vlad_video", ops.materialise(vlad_video))
        if has_audio:
            with side, vs.variable_scope("audio_VLAD"):
                vlad_audio = audio_NetVLAD.forward(audio, kmajor=encoder, input_affine=aff_a, storage=storage,
                                                   out_slot=(slots.slots[0 if lazy5 else 1] if slots else None))   # :2276-2277
                vs.summary("vlad_audio", vlad_audio)

        if encoder:
            # tokens = clusters (App. C5): the pooling kernel already wrote the [B, K, D] view
            if has_audio:
                with vs.variable_scope("audio_attention"):
                    audio_encoder_block = transformer_utils.TransformerEncoder(
                        feature_size=128, hidden_size=128, num_heads=16, attention_dropout=0.1, ff_filter_size=4 * 128,
                        ff_relu_dropout=0.1, is_train=is_training, scope_id="encode2")
                if FLAGS.descriptor_slots and video_encoder_block.fused(vlad_video) and audio_encoder_block.fused(vlad_audio):
                    # both encoders write their result straight into one [B, 1024 K + 128 K/4] buffer: the concat below and
                    # the slicing of its gradient cost nothing
                    slots = ops.DescriptorSlots(vlad_video.shape[0], [(cluster_size, 1024), (cluster_size // 4, 128)], vlad_video)
            with vs.variable_scope("video_attention"):
                vlad_video = video_encoder_block.forward(vlad_video, out_slot=slots.slots[0] if slots else None)   # :2282-2292
            if has_audio:
                with side, vs.variable_scope("audio_attention"):
                    vlad_audio = audio_encoder_block.forward(vlad_audio, out_slot=slots.slots[1] if slots else None)  # :2294-2304
            if slots is None:
                vlad_video = vlad_video.reshape(-1, 1024 * cluster_size)
                if has_audio:
                    vlad_audio = vlad_audio.reshape(-1, 128 * (cluster_size // 4))
        if use_side:
            side.join(vlad_audio)

        if lazy5:
            if vs.default_store().summaries is not None:
                vs.summary("vlad", torch.cat([ops.materialise(vlad_video), vlad_audio.reshape(batch, -1)], 1))
            return _project_gate_classify((vlad_video, vlad_audio.reshape(batch, -1)), vocab_size, cluster_size, hidden1_size,
                                          add_batch_norm, relu, gating, remove_diag, is_training, **unused_params)   # :2309 inside the projection
        if slots is not None:
            vlad = slots.join(vlad_video, vlad_audio)                                          # :2309, in place
        else:
            vlad = torch.cat([vlad_video, vlad_audio], 1) if has_audio else vlad_video         # :2309
        vs.summary("vlad", vlad)
        if vlad.dtype != torch.float32:      # bf16 storage: the projection and everything behind it compute in fp32
            vlad = vlad.float()
        return _project_gate_classify(vlad, vocab_size, cluster_size, hidden1_size, add_batch_norm, relu, gating,
                                      remove_diag, is_training, **unused_params)


class WillowModelReg(models.BaseModel):
    """WILLOW model with orthogonal regularisation (frame_level_models.py:2516-2635): random frame
    sampling, input_bn, NetVladOrthoReg on both streams, then the shared projection / context gating / MoE tail."""

    def create_model(self, model_input, vocab_size, num_frames, iterations=None, add_batch_norm=None,
                     sample_random_frames=None, cluster_size=None, hidden_size=None, is_training=True,
                     frame_uniform=None, **unused_params):
        iterations = iterations or FLAGS.iterations
        add_batch_norm = add_batch_norm or FLAGS.netvlad_add_batch_norm
        random_frames = sample_random_frames or FLAGS.sample_random_frames
        cluster_size = cluster_size or FLAGS.netvlad_cluster_size
        hidden1_size = hidden_size or FLAGS.netvlad_hidden_size
        relu, gating, remove_diag = FLAGS.netvlad_relu, FLAGS.gating, FLAGS.gating_remove_diag
        sampler = model_utils.SampleRandomFrames if random_frames else model_utils.SampleRandomSequence
        model_input = sampler(model_input, num_frames.reshape(-1, 1), iterations, uniform=frame_uniform)      # :2539-2544
        max_frames, feature_size = model_input.shape[1], model_input.shape[2]
        reshaped_input = model_input.reshape(-1, feature_size)
        video_NetVLAD = video_pooling_modules.NetVladOrthoReg(1024, max_frames, cluster_size, add_batch_norm, is_training,
                                                              FLAGS.rgb_det_reg, "netvlad_rgb_scope")
        audio_NetVLAD = video_pooling_modules.NetVladOrthoReg(128, max_frames, cluster_size // 4, add_batch_norm, is_training,
                                                              FLAGS.audio_det_reg, "netvlad_audio_scope")
        if add_batch_norm:
            reshaped_input = layers.batch_norm(reshaped_input, is_training, "input_bn")                       # :2558-2564
        has_audio = feature_size > 1024                                                                       # App. C9
        with vs.variable_scope("video_VLAD"):
            vlad = video_NetVLAD.forward(reshaped_input[:, 0:1024])
        if has_audio:
            with vs.variable_scope("audio_VLAD"):
                vlad = torch.cat([vlad, audio_NetVLAD.forward(reshaped_input[:, 1024:])], 1)
        return _project_gate_classify(vlad, vocab_size, cluster_size, hidden1_size, add_batch_norm, relu, gating,
                                      remove_diag, is_training, **unused_params)


class RegularizedTriangulationModel(models.BaseModel):
    """Weighted triangulation embedding of both streams, its temporal differences, max-mean pooling of both, five projections with
    batch norms and the three-layer classifier (frame_level_models.py:1148-1307).  Defect resolutions: SURVEY App. C17-C21.

    On the GPU with FLAGS.triangulation_fused each stream is ONE ops.triangulation_pool call: the embedding [B, T, D*K] and the temporal
    embedding (79 MB per clip each at the defaults T = 300, K = 64, D = 1024) are never written; otherwise the materialising modules of
    video_pooling_modules / aggregation_modules compose the same graph.  The variables and the results are the same either way.
    ``frame_uniform`` [B, iterations] replaces the random draw of SampleRandomFrames, ``dropout_masks`` {"fc1", "fc2"} the classifier's."""

    def create_model(self, model_input, vocab_size, num_frames, iterations=None, add_batch_norm=None, sample_random_frames=None,
                     hidden_size=None, is_training=True, frame_uniform=None, video_anchor_size=None, audio_anchor_size=None,
                     quantised_training=False, **unused_params):
        iterations = iterations or FLAGS.iterations
        video_anchor_size = int(video_anchor_size or FLAGS.wtm_video_anchor_size)                             # :1160
        audio_anchor_size = int(audio_anchor_size or FLAGS.wtm_audio_anchor_size)                             # :1161
        quantised, model_input, max_frames, feature_size = _random_frames(model_input, num_frames, iterations, frame_uniform)  # :1163-1165
        if feature_size <= 1024:
            raise ValueError("RegularizedTriangulationModel slices a 1024-wide video and a 128-wide audio stream out of its input "
                             f"(frame_level_models.py:1202,1210); got {feature_size} features")
        dev = model_input.device
        # add_batch_norm is accepted and unused, as written: the modules store it and never read it (:1176-1192)
        streams = (("video_t_emb", 1024, video_anchor_size, slice(0, 1024)), ("audio_t_emb", feature_size - 1024, audio_anchor_size, slice(1024, None)))
        d_modules = [video_pooling_modules.WeightedTriangulationEmbedding(D, max_frames, K, add_batch_norm, is_training) for _, D, K, _ in streams]
        mean_max_pool = aggregation_modules.MaxMeanPoolingModule(l2_normalize=False)                          # :1183
        t_modules = [video_pooling_modules.TriangulationTemporalEmbedding(D, max_frames, K, add_batch_norm, is_training) for _, D, K, _ in streams]
        if quantised:       # the reader's uint8 batch: sampled, dequantised, normalised and batch-normalised by the frame-prep kernels
            stream_inputs = _gather_and_normalise(model_input, num_frames, iterations, frame_uniform, ("input_bn",), is_training, quantised_training)
        else:
            reshaped_input = layers.batch_norm(model_input.reshape(-1, feature_size), is_training, "input_bn")   # :1194-1199
            stream_inputs = [reshaped_input[:, cols] for *_, cols in streams]
        fused = bool(FLAGS.triangulation_fused and dev.type == "cuda" and max_frames >= 2)
        agg_d, agg_t, orthogonal_reg = [], [], 0.0
        for (scope, D, K, _), x, d_module, t_module in zip(streams, stream_inputs, d_modules, t_modules):
            with vs.variable_scope(scope):                                                                    # :1201-1215
                if fused:
                    anchors, ortho = d_module.variables(dev)
                    max_d, mean_d, max_t, mean_t = ops.triangulation_pool(x.contiguous(), anchors, max_frames, scale=1 / math.sqrt(K))
                    agg_d.append(torch.cat([max_d, mean_d], 1))
                    agg_t.append(torch.cat([max_t, mean_t], 1))
                else:
                    emb_d, ortho = d_module.forward(x)
                    emb_t = t_module.forward(emb_d)
                    agg_d.append(mean_max_pool.forward(emb_d))
                    agg_t.append(mean_max_pool.forward(emb_t))
            orthogonal_reg = orthogonal_reg + ortho                                                           # :1217
        (agg_video_d, agg_audio_d), (agg_video_t, agg_audio_t) = agg_d, agg_t

        def project(x, name, units, regularised=False):
            w = vs.get_variable(name, [x.shape[1], units], vs.random_normal_initializer(1 / math.sqrt(units)), device=dev)
            if regularised:                                          # layers.l1_l2_regularizer(1e-5) = (scale_l1 = 1e-5, scale_l2 = 1.0): App. B
                store = vs.default_store()
                if FLAGS.wtm_projection_l1:
                    store.add_regularization_loss(FLAGS.wtm_projection_l1 * w.abs().sum())
                if FLAGS.wtm_projection_l2:
                    store.add_l2_regularizer(w, FLAGS.wtm_projection_l2)
            return x.matmul(w)

        video_projection_activation = layers.batch_norm(project(agg_video_d, "video_projection", 1024), is_training,
                                                        "video_projection_bn")                               # :1219-1231
        # :1239 multiplies the integer agg_audio_d_dim; the intent is agg_audio_d (App. C17)
        audio_projection_activation = layers.batch_norm(project(agg_audio_d, "audio_projection", 128), is_training,
                                                        "audio_projection_bn")                               # :1233-1245
        dis_projection_activation = torch.cat([video_projection_activation, audio_projection_activation], 1)  # :1247
        agg_temp = torch.cat([agg_video_t, agg_audio_t], 1)                                                   # :1251
        temp_projection_activation = layers.batch_norm(project(agg_temp, "temp_projection_1", 1152), is_training,
                                                       "temp_projection_bn")                                 # :1253-1263
        dis_activation = layers.batch_norm(project(dis_projection_activation, "dis_projection_2", 2048, regularised=True), is_training,
                                           "dis_activation_bn")                                              # :1266-1279
        temp_activation = layers.batch_norm(project(temp_projection_activation, "temp_projection_2", 2048, regularised=True), is_training,
                                            "temp_activation_bn")                                            # :1282-1294
        activation = torch.cat([dis_activation, temp_activation], 1)                                          # :1297
        aggregated_model = getattr(video_level_models, "ClassLearningThreeNnModel")
        return aggregated_model().create_model(model_input=activation, vocab_size=vocab_size, is_training=is_training,
                                               ortho_reg=orthogonal_reg, **unused_params)                    # :1299-1307


class SoftAttentionTriangulationModel(models.BaseModel):
    """Triangulation embedding of both streams, its temporal differences, soft-attention mean and max pooling of all four, six
    projections with batch norms and the four-layer classifier (frame_level_models.py:965-1145).  As written: SURVEY App. C22-C25.

    On the GPU with FLAGS.soft_attention_fused each stream is ONE ops.triangulation_attention_pool call: the embedding [B, T, D*K] and
    the temporal embedding (33.5 MB per clip each at the defaults T = 64, K = 128, D = 1024) are never written; otherwise the
    materialising modules of video_pooling_modules / aggregation_modules compose the same graph.  The variables and the results are
    the same either way.  ``frame_uniform`` [B, iterations] replaces the random draw of SampleRandomFrames; ``video_anchor_size``,
    ``audio_anchor_size``, ``video_bottleneck`` and ``audio_bottleneck`` override the flags (the reference reads the flags only)."""

    def create_model(self, model_input, vocab_size, num_frames, iterations=None, add_batch_norm=None, sample_random_frames=None,
                     hidden_size=None, is_training=True, frame_uniform=None, video_anchor_size=None, audio_anchor_size=None,
                     video_bottleneck=None, audio_bottleneck=None, quantised_training=False, **unused_params):
        iterations = iterations or FLAGS.sftm_iterations                                                      # :976
        add_batch_norm = add_batch_norm or FLAGS.sftm_add_batch_norm                                          # :977 (False cannot switch it off: C23)
        video_anchor_size = int(video_anchor_size or FLAGS.sftm_video_anchor_size)                            # :978-981
        audio_anchor_size = int(audio_anchor_size or FLAGS.sftm_audio_anchor_size)
        video_bottleneck = int(video_bottleneck or FLAGS.sftm_video_bottleneck)
        audio_bottleneck = int(audio_bottleneck or FLAGS.sftm_audio_bottleneck)
        # sample_random_frames and hidden_size are accepted and read nowhere, as written (C24)
        quantised, model_input, max_frames, feature_size = _random_frames(model_input, num_frames, iterations, frame_uniform)  # :983-984
        if feature_size <= 1024:
            raise ValueError("SoftAttentionTriangulationModel slices a 1024-wide video and a 128-wide audio stream out of its input "
                             f"(frame_level_models.py:991-992); got {feature_size} features")
        dev = model_input.device
        streams = (("video", 1024, video_anchor_size, video_bottleneck, slice(0, 1024)),
                   ("audio", feature_size - 1024, audio_anchor_size, audio_bottleneck, slice(1024, None)))
        features = _stream_features(quantised, model_input, num_frames, iterations, frame_uniform, add_batch_norm, is_training,
                                    quantised_training)                                                       # :991-1006
        d_modules = [video_pooling_modules.TriangulationEmbedding(D, max_frames, K, add_batch_norm, is_training) for _, D, K, _, _ in streams]
        cluster_pool = aggregation_modules.IndirectClusterMaxMeanPoolModule(l2_normalize=False)               # :1019
        t_modules = [video_pooling_modules.TriangulationTemporalEmbedding(D, max_frames, K, add_batch_norm, is_training) for _, D, K, _, _ in streams]
        fused = bool(FLAGS.soft_attention_fused and dev.type == "cuda" and max_frames >= 2)
        agg = {}
        for (name, D, K, _, _), x, d_module, t_module in zip(streams, features, d_modules, t_modules):
            with vs.variable_scope(name + "_triangulation_embedding"):                                        # :1031-1051
                if fused:
                    mean_d, max_d, mean_t, max_t = ops.triangulation_attention_pool(x.contiguous(), d_module.variables(dev), max_frames)
                    agg[name + "_d"] = torch.cat([mean_d, max_d], 1)
                    agg[name + "_t"] = torch.cat([mean_t, max_t], 1)
                else:
                    emb_d = d_module.forward(x)
                    emb_t = t_module.forward(emb_d)                                                           # (the frame differences: C22)
                    agg[name + "_d"] = cluster_pool.forward(emb_d.reshape(-1, max_frames, D * K))
                    agg[name + "_t"] = cluster_pool.forward(emb_t)

        def project(x, name, units):
            w = vs.get_variable(name, [x.shape[1], units], vs.random_normal_initializer(1 / math.sqrt(units)), device=dev)
            return x.matmul(w)

        def bn(x, scope):
            return layers.batch_norm(x, is_training, scope) if add_batch_norm else x

        # the four projection variables are created before any of their batch norms (:1054-1071, then :1078-1102)
        acts = {f"{name}_{kind}": project(agg[f"{name}_{kind}"], f"{name}_{kind}_projection", units)
                for name, _, _, units, _ in streams for kind in ("d", "t")}
        acts = {key: bn(a, key + "_activation_bn") for key, a in acts.items()}
        fused_streams = []
        for name, _, _, units, _ in streams:                                                                  # :1105-1120
            fused_streams.append(project(torch.cat([acts[name + "_d"], acts[name + "_t"]], 1), name + "_projection", units))
        activation = torch.cat([bn(a, name + "_activation_bn") for a, (name, *_) in zip(fused_streams, streams)], 1)   # :1122-1137
        aggregated_model = getattr(video_level_models, "ClassLearningFourNnModel")
        return aggregated_model().create_model(model_input=activation, vocab_size=vocab_size, is_training=is_training,
                                               **unused_params)                                              # :1139-1145


class TriangulationCnnClusterModel(models.BaseModel):
    """Triangulation embedding of both streams and its temporal differences, a per-anchor 1x1 convolution over each, soft-attention
    mean pooling of the first and mean pooling of the second, one hidden layer per stream and the four-layer classifier
    (frame_level_models.py:757-939).  As written: SURVEY App. C26-C28 (and C22, C23, C25).

    On the GPU with FLAGS.triangulation_cnn_fused each stream is ONE ops.triangulation_cnn_pool call: the convolution has no bias and
    no activation, so it commutes with both poolings and runs on the pooled means -- neither the embeddings [B, T, D*K] (105 MB per
    clip at the defaults T = 200, K = 128, D = 1024) nor the convolutions' [B, T, K*F] results are written; otherwise the
    materialising modules of video_pooling_modules / aggregation_modules compose the reference's graph.  The variables and the results
    are the same either way.  ``frame_uniform`` [B, iterations] replaces the random draw of SampleRandomFrames; ``video_anchor_size``,
    ``audio_anchor_size``, ``video_kernel_size``, ``audio_kernel_size``, ``video_hidden`` and ``audio_hidden`` override the flags (the
    reference reads the flags only)."""

    def create_model(self, model_input, vocab_size, num_frames, iterations=None, add_batch_norm=None, sample_random_frames=None,
                     hidden_size=None, is_training=True, frame_uniform=None, video_anchor_size=None, audio_anchor_size=None,
                     video_kernel_size=None, audio_kernel_size=None, video_hidden=None, audio_hidden=None, quantised_training=False,
                     **unused_params):
        iterations = iterations or FLAGS.tccm_iterations                                                      # :768
        add_batch_norm = add_batch_norm or FLAGS.tccm_add_batch_norm                                          # :769 (C23)
        video_anchor_size = int(video_anchor_size or FLAGS.tccm_video_anchor_size)                            # :770-775
        audio_anchor_size = int(audio_anchor_size or FLAGS.tccm_audio_anchor_size)
        video_kernel_size = int(video_kernel_size or FLAGS.tccm_video_kernel_size)
        audio_kernel_size = int(audio_kernel_size or FLAGS.tccm_audio_kernel_size)
        video_hidden = int(video_hidden or FLAGS.tccm_video_hidden)
        audio_hidden = int(audio_hidden or FLAGS.tccm_audio_hidden)
        # sample_random_frames and hidden_size are accepted and read nowhere, as written (C26)
        quantised, model_input, max_frames, feature_size = _random_frames(model_input, num_frames, iterations, frame_uniform)  # :777-778
        if feature_size <= 1024:
            raise ValueError("TriangulationCnnClusterModel slices a 1024-wide video and a 128-wide audio stream out of its input "
                             f"(frame_level_models.py:785-786); got {feature_size} features")
        dev = model_input.device
        streams = (("video", 1024, video_anchor_size, video_kernel_size, video_hidden, slice(0, 1024)),
                   ("audio", feature_size - 1024, audio_anchor_size, audio_kernel_size, audio_hidden, slice(1024, None)))
        features = _stream_features(quantised, model_input, num_frames, iterations, frame_uniform, add_batch_norm, is_training,
                                    quantised_training)                                                       # :785-800
        d_modules = [video_pooling_modules.TriangulationEmbedding(D, max_frames, K, add_batch_norm, is_training) for _, D, K, _, _, _ in streams]
        cnn_modules = [(video_pooling_modules.TriangulationCnnModule(D, max_frames, F, K, add_batch_norm, is_training, name + "_d"),
                        video_pooling_modules.TriangulationCnnModule(D, max_frames - 1, F, K, add_batch_norm, is_training, name + "_t"))
                       for name, D, K, F, _, _ in streams]                                                    # :813-843 (max_frames - 1: C28)
        ic_mean_pool = aggregation_modules.IndirectClusterMeanPoolModule(l2_normalize=False)                  # :845
        mean_std_pool = aggregation_modules.MeanStdPoolModule(l2_normalize=False)                             # :846 (the mean only: C27)
        t_modules = [video_pooling_modules.TriangulationTemporalEmbedding(D, max_frames, K, add_batch_norm, is_training) for _, D, K, _, _, _ in streams]
        fused = bool(FLAGS.triangulation_cnn_fused and dev.type == "cuda" and max_frames >= 2)
        agg = []
        for (name, D, K, _, _, _), x, d_module, (d_cnn, t_cnn), t_module in zip(streams, features, d_modules, cnn_modules, t_modules):
            with vs.variable_scope(name + "_triangulation_embedding"):                                        # :859-915
                if fused:
                    anchors = d_module.variables(dev)
                    with vs.variable_scope(name + "_d"):
                        cnn_d = d_cnn.variables(dev)
                    with vs.variable_scope(name + "_t"):
                        cnn_t = t_cnn.variables(dev)
                    agg_d, agg_t = ops.triangulation_cnn_pool(x.contiguous(), anchors, cnn_d, cnn_t, max_frames)
                else:
                    emb_d = d_module.forward(x)
                    with vs.variable_scope(name + "_d"):
                        emb_d_cnn = d_cnn.forward(emb_d)
                    agg_d = ic_mean_pool.forward(emb_d.reshape(-1, max_frames, D * K), emb_d_cnn)             # (weights from e, pooling over the convolution)
                    emb_t = t_module.forward(emb_d)                                                           # (the frame differences: C22)
                    with vs.variable_scope(name + "_t"):
                        emb_t_cnn = t_cnn.forward(emb_t.reshape(-1, D * K))
                    agg_t = mean_std_pool.forward(emb_t_cnn)
                a = torch.cat([agg_d, agg_t], 1)
                agg.append(layers.batch_norm(a, is_training, f"agg_{name}_bn") if add_batch_norm else a)
        acts = []
        for (name, _, _, _, units, _), a in zip(streams, agg):                                                # :917-929
            w = vs.get_variable(name + "_hidden", [a.shape[1], units], vs.random_normal_initializer(1 / math.sqrt(units)), device=dev)
            acts.append(a.matmul(w))
        activation = torch.cat(acts, 1)                                                                       # :931
        aggregated_model = getattr(video_level_models, "ClassLearningFourNnModel")
        return aggregated_model().create_model(model_input=activation, vocab_size=vocab_size, is_training=is_training,
                                               **unused_params)                                              # :933-939


class JuhanTestModelV5(models.BaseModel):
    """Batch norm of both streams, one TriangulationV5Module per stream (the per-anchor convolutions of the triangulation embedding and
    of its rolled differences over EVERY frame, the mean and variance over the frames, two hidden layers and a fusion layer) and the
    four-layer batch-norm classifier (frame_level_models.py:491-606).  As written: SURVEY App. C29-C31 (and C23, C24).

    On the GPU with FLAGS.triangulation_v5_fused each stream's pooling is ONE ops.triangulation_cnn_moments call: neither embedding
    [B, T, D*K] (31 MB per clip at the defaults T = 30, K = 256, D = 1024) is written; otherwise TriangulationV5Module.forward
    materialises them.  The variables and the results are the same either way.  ``frame_uniform`` [B, iterations] replaces the random
    draw of SampleRandomFrames; ``video_anchor_size``, ``audio_anchor_size``, ``video_kernel_size``, ``audio_kernel_size``,
    ``video_hidden``, ``audio_hidden``, ``video_output_dim`` and ``audio_output_dim`` override the flags (the reference reads the flags
    only)."""

    def create_model(self, model_input, vocab_size, num_frames, iterations=None, add_batch_norm=None, sample_random_frames=None,
                     hidden_size=None, is_training=True, frame_uniform=None, video_anchor_size=None, audio_anchor_size=None,
                     video_kernel_size=None, audio_kernel_size=None, video_hidden=None, audio_hidden=None, video_output_dim=None,
                     audio_output_dim=None, quantised_training=False, **unused_params):
        iterations = iterations or FLAGS.jtmv5_iteration                                                      # :526
        add_batch_norm = add_batch_norm or FLAGS.jtmv5_add_batch_norm                                         # :527 (C23)
        video_anchor_size = int(video_anchor_size or FLAGS.jtmv5_video_anchor_size)                           # :528-535
        audio_anchor_size = int(audio_anchor_size or FLAGS.jtmv5_audio_anchor_size)
        video_kernel_size = int(video_kernel_size or FLAGS.jtmv5_video_kernel_size)
        audio_kernel_size = int(audio_kernel_size or FLAGS.jtmv5_audio_kernel_size)
        video_hidden = int(video_hidden or FLAGS.jtmv5_video_hidden)
        audio_hidden = int(audio_hidden or FLAGS.jtmv5_audio_hidden)
        video_output_dim = int(video_output_dim or FLAGS.jtmv5_video_output_dim)
        audio_output_dim = int(audio_output_dim or FLAGS.jtmv5_audio_output_dim)
        # sample_random_frames and hidden_size are accepted and read nowhere, as written (C30)
        quantised, model_input, max_frames, feature_size = _random_frames(model_input, num_frames, iterations, frame_uniform)  # :537-538
        if feature_size <= 1024:
            raise ValueError("JuhanTestModelV5 slices a 1024-wide video and a 128-wide audio stream out of its input "
                             f"(frame_level_models.py:546-547); got {feature_size} features")
        dev = model_input.device
        streams = (("video", 1024, video_anchor_size, video_kernel_size, video_hidden, video_output_dim, slice(0, 1024)),
                   ("audio", feature_size - 1024, audio_anchor_size, audio_kernel_size, audio_hidden, audio_output_dim, slice(1024, None)))
        features = _stream_features(quantised, model_input, num_frames, iterations, frame_uniform, add_batch_norm, is_training,
                                    quantised_training)                                                       # :546-562
        v5_modules = [video_pooling_modules.TriangulationV5Module(
            feature_size=D, max_frames=max_frames, anchor_size=K, kernel_size=F, self_attention=False, hidden_layer_size=H, output_dim=O,
            add_relu=True, batch_norm=add_batch_norm, is_training=is_training, scope_id=None) for _, D, K, F, H, O, _ in streams]   # :564-588
        fused = bool(FLAGS.triangulation_v5_fused and dev.type == "cuda" and max_frames >= 2)
        acts = []
        for (name, *_), x, module in zip(streams, features, v5_modules):
            with vs.variable_scope(name + "_triangulation_embedding"):                                        # :590-596
                if fused:
                    anchors, cnn_s, cnn_t = module.variables(dev)
                    acts.append(module.head(*ops.triangulation_cnn_moments(x.contiguous(), anchors, cnn_s, cnn_t, max_frames)))
                else:
                    acts.append(module.forward(x))
        activation = torch.cat(acts, 1)                                                                       # :598
        aggregated_model = getattr(video_level_models, "FourLayerBatchNeuralModel")
        return aggregated_model().create_model(model_input=activation, vocab_size=vocab_size, is_training=is_training,
                                               **unused_params)                                              # :600-606


def weight_fits(nbytes: int, limit: int) -> bool:
    """Whether a weight of ``nbytes`` bytes can be held at all by a device with ``limit`` bytes of memory."""
    return int(nbytes) <= int(limit)


def device_memory_bytes(device) -> int:
    """The total memory of the device a model is built on: the GPU's, or the host's for the CPU."""
    device = torch.device(device)
    if device.type == "cuda":
        return int(torch.cuda.get_device_properties(device).total_memory)
    return int(os.sysconf("SC_PHYS_PAGES")) * int(os.sysconf("SC_PAGE_SIZE"))


def check_v6_hidden_weight(stream, feature_size, anchor_size, cluster_size, output_dim, limit, is_training=False):
    """JuhanTestModelV6's size check, before any variable of ``stream`` is created: hidden_weight [C * K * D, O] in fp32 against ``limit``
    bytes -- in training together with its gradient, which every step holds beside it (an MI355X reports 309 GB: the 275 GB of the video
    defaults alone would pass, and no step could run).  -> the weight's size in bytes; ValueError naming the stream, the size and the three
    flags that reduce it."""
    nbytes = 4 * int(feature_size) * int(anchor_size) * int(cluster_size) * int(output_dim)
    if not weight_fits(nbytes * (2 if is_training else 1), limit):
        raise ValueError(
            f"JuhanTestModelV6: the {stream} stream's hidden_weight [{cluster_size} * {anchor_size} * {feature_size}, {output_dim}] takes "
            f"{nbytes / 1e9:.1f} GB ({nbytes} bytes) in fp32{' and as much again for its gradient' if is_training else ''}, more than the device's "
            f"{limit / 1e9:.1f} GB: reduce "
            f"jtmv6_{stream}_anchor_size ({anchor_size}), jtmv6_{stream}_cluster_size ({cluster_size}) or jtmv6_{stream}_output_dim "
            f"({output_dim}), or pass the keyword overrides of the same names")
    return nbytes


class JuhanTestModelV6(models.BaseModel):
    """Batch norm of both streams, one TriangulationV6Module per stream (the twice-normalised triangulation embedding, a batch norm over
    all K*D features, OneFcAttention's C attention-weighted sums over the frames, shifted and normalised, one matrix to the stream's
    output, batch norm and relu) and the four-layer batch-norm classifier (frame_level_models.py:638-733).  As written: SURVEY App.
    C48-C50 (and C23).

    Each stream's hidden_weight is [C * K * D, O]; at the flags' defaults the video stream's takes 275 GB, so its size is checked against
    the device's memory before any of the stream's variables is created (``memory_limit`` replaces the device's).  On the GPU with
    FLAGS.triangulation_v6_fused each stream's pooling goes through ops.triangulation_onefc_pool: no [(B*T), K*D] tensor is written;
    otherwise TriangulationV6Module.pool materialises five.  The variables and the results are the same either way.  ``frame_uniform``
    [B, iterations] replaces the random draw of SampleRandomFrames; ``video_anchor_size``, ``audio_anchor_size``,
    ``video_cluster_size``, ``audio_cluster_size``, ``video_output_dim`` and ``audio_output_dim`` override the flags (the reference reads
    the flags only)."""

    def create_model(self, model_input, vocab_size, num_frames, iterations=None, add_batch_norm=None, sample_random_frames=None,
                     hidden_size=None, is_training=True, frame_uniform=None, video_anchor_size=None, audio_anchor_size=None,
                     video_cluster_size=None, audio_cluster_size=None, video_output_dim=None, audio_output_dim=None,
                     quantised_training=False, memory_limit=None, **unused_params):
        iterations = iterations or FLAGS.jtmv6_iteration                                                      # :649
        add_batch_norm = add_batch_norm or FLAGS.jtmv6_add_batch_norm                                         # :650 (C23)
        video_anchor_size = int(video_anchor_size or FLAGS.jtmv6_video_anchor_size)                           # :651-660
        audio_anchor_size = int(audio_anchor_size or FLAGS.jtmv6_audio_anchor_size)
        video_cluster_size = int(video_cluster_size or FLAGS.jtmv6_video_cluster_size)
        audio_cluster_size = int(audio_cluster_size or FLAGS.jtmv6_audio_cluster_size)
        video_output_dim = int(video_output_dim or FLAGS.jtmv6_video_output_dim)
        audio_output_dim = int(audio_output_dim or FLAGS.jtmv6_audio_output_dim)
        # the kernel sizes and the hidden sizes go to the modules and are read nowhere; sample_random_frames and hidden_size are accepted
        # and read nowhere, as written (C48)
        quantised, model_input, max_frames, feature_size = _random_frames(model_input, num_frames, iterations, frame_uniform)  # :662-663
        if feature_size <= 1024:
            raise ValueError("JuhanTestModelV6 slices a 1024-wide video and a 128-wide audio stream out of its input "
                             f"(frame_level_models.py:671-672); got {feature_size} features")
        dev = model_input.device
        streams = (("video", 1024, video_anchor_size, FLAGS.jtmv6_video_kernel_size, FLAGS.jtmv6_video_hidden, video_cluster_size,
                    video_output_dim),
                   ("audio", feature_size - 1024, audio_anchor_size, FLAGS.jtmv6_audio_kernel_size, FLAGS.jtmv6_audio_hidden,
                    audio_cluster_size, audio_output_dim))
        limit = device_memory_bytes(dev) if memory_limit is None else int(memory_limit)
        for name, D, K, _, _, C, O in streams:                                                                # (before any variable)
            check_v6_hidden_weight(name, D, K, C, O, limit, is_training)
        features = _stream_features(quantised, model_input, num_frames, iterations, frame_uniform, add_batch_norm, is_training,
                                    quantised_training)                                                       # :671-687
        v6_modules = [video_pooling_modules.TriangulationV6Module(
            feature_size=D, max_frames=max_frames, anchor_size=K, kernel_size=F, self_attention=False, cluster_size=C, hidden_layer_size=H,
            output_dim=O, add_relu=True, batch_norm=add_batch_norm, is_training=is_training, scope_id=None)
            for _, D, K, F, H, C, O in streams]                                                               # :689-715
        fused = bool(FLAGS.triangulation_v6_fused and dev.type == "cuda")
        acts = []
        for (name, *_), x, module in zip(streams, features, v6_modules):
            with vs.variable_scope(name + "_triangulation_embedding"):                                        # :717-723
                acts.append(module.head(module.fused_pool(x.contiguous())) if fused else module.forward(x))
        activation = torch.cat(acts, 1)                                                                       # :725
        aggregated_model = getattr(video_level_models, "FourLayerBatchNeuralModel")
        return aggregated_model().create_model(model_input=activation, vocab_size=vocab_size, is_training=is_training,
                                               **unused_params)                                              # :727-733


class JuhanTestModelV1(models.BaseModel):
    """One TriangulationCnnIndirectAttentionModule per stream (the triangulation embedding and its rolled differences, each batch-normed
    over all K*D features, soft-attention weights from the relu'd Gram, the weighted mean and the variance over the frames, a hidden layer
    and a fusion layer) and the class-learning four-layer classifier (frame_level_models.py:59-154).  No input batch norm.  As written:
    SURVEY App. C29, C32-C35 (and C23).

    On the GPU with FLAGS.triangulation_v1_fused each stream's pooling goes through ops.triangulation_bn_moments: no [(B*T), K*D] tensor
    (126 MB at the video defaults B = 16, T = 30, K = 64, D = 1024) is written; otherwise TriangulationCnnIndirectAttentionModule.pool
    materialises them.  The variables and the results are the same either way.  ``frame_uniform`` [B, iterations] replaces the random
    draw of SampleRandomFrames; ``video_anchor_size``, ``audio_anchor_size``, ``video_hidden``, ``audio_hidden``, ``video_output_dim``
    and ``audio_output_dim`` override the flags (the reference reads the flags only)."""

    def create_model(self, model_input, vocab_size, num_frames, iterations=None, add_batch_norm=None, sample_random_frames=None,
                     hidden_size=None, is_training=True, frame_uniform=None, video_anchor_size=None, audio_anchor_size=None,
                     video_hidden=None, audio_hidden=None, video_output_dim=None, audio_output_dim=None, quantised_training=False,
                     **unused_params):
        iterations = iterations or FLAGS.jtmv1_iteration                                                      # :94
        add_batch_norm = add_batch_norm or FLAGS.jtmv1_add_batch_norm                                         # :95 (C23)
        video_anchor_size = int(video_anchor_size or FLAGS.jtmv1_video_anchor_size)                           # :96-101
        audio_anchor_size = int(audio_anchor_size or FLAGS.jtmv1_audio_anchor_size)
        video_hidden = int(video_hidden or FLAGS.jtmv1_video_hidden)
        audio_hidden = int(audio_hidden or FLAGS.jtmv1_audio_hidden)
        video_output_dim = int(video_output_dim or FLAGS.jtmv1_video_output_dim)
        audio_output_dim = int(audio_output_dim or FLAGS.jtmv1_audio_output_dim)
        use_attention, use_relu = FLAGS.jtmv1_use_attention, FLAGS.jtmv1_use_relu                             # :102-103
        # sample_random_frames and hidden_size are accepted and read nowhere, as written
        quantised, model_input, max_frames, feature_size = _random_frames(model_input, num_frames, iterations, frame_uniform)  # :105-106
        if feature_size <= 1024:
            raise ValueError("JuhanTestModelV1 slices a 1024-wide video and a 128-wide audio stream out of its input "
                             f"(frame_level_models.py:137-141); got {feature_size} features")
        streams = (("video", 1024, video_anchor_size, video_hidden, video_output_dim, slice(0, 1024)),
                   ("audio", feature_size - 1024, audio_anchor_size, audio_hidden, audio_output_dim, slice(1024, None)))
        features = _stream_features(quantised, model_input, num_frames, iterations, frame_uniform, False, is_training,
                                    quantised_training)                                                       # (no input batch norm)
        v1_modules = [video_pooling_modules.TriangulationCnnIndirectAttentionModule(
            feature_size=D, max_frames=max_frames, anchor_size=K, self_attention=use_attention, hidden_layer_size=H, output_dim=O,
            add_relu=use_relu, batch_norm=add_batch_norm, is_training=is_training, scope_id=None) for _, D, K, H, O, _ in streams]   # :113-135
        fused = bool(FLAGS.triangulation_v1_fused and model_input.is_cuda and max_frames >= 2)
        acts = []
        for (name, *_), x, module in zip(streams, features, v1_modules):
            with vs.variable_scope(name + "_triangulation_embedding"):                                        # :137-143
                acts.append(module.head(*module.fused_pool(x.contiguous())) if fused else module.forward(x))
        activation = torch.cat(acts, 1)                                                                       # :145
        aggregated_model = getattr(video_level_models, "ClassLearningFourNnModel")
        return aggregated_model().create_model(model_input=activation, vocab_size=vocab_size, is_training=is_training,
                                               **unused_params)                                              # :147-154


class JuhanTestModelV2(models.BaseModel):
    """One TriangulationNsCnnIndirectAttentionModule per stream (the triangulation embedding against orthogonally initialised anchors and
    its rolled differences, a convolution per anchor over each, soft-attention weights over the frames from the relu'd Gram of the
    embedding, the weighted mean and the variance of the convolutions' results, a hidden layer and a fusion layer), a batch norm of the
    joined streams and the class-learning four-layer classifier (frame_level_models.py:158-268).  No input batch norm.  As written:
    SURVEY App. C29, C32-C34, C39 (and C23).

    On the GPU with FLAGS.triangulation_v2_fused each stream's pooling goes through ops.triangulation_cnn_attention_moments: no
    [(B*T), K*D] tensor (419 MB at the video defaults B = 16, T = 200, K = 32, D = 1024) is written; otherwise
    TriangulationNsCnnIndirectAttentionModule.pool materialises them.  The variables and the results are the same either way.
    ``frame_uniform`` [B, iterations] replaces the random draw of SampleRandomFrames; ``video_anchor_size``, ``audio_anchor_size``,
    ``video_kernel_size``, ``audio_kernel_size``, ``video_hidden``, ``audio_hidden``, ``video_output_dim`` and ``audio_output_dim``
    override the flags (the reference reads the flags only)."""

    def create_model(self, model_input, vocab_size, num_frames, iterations=None, add_batch_norm=None, sample_random_frames=None,
                     hidden_size=None, is_training=True, frame_uniform=None, video_anchor_size=None, audio_anchor_size=None,
                     video_kernel_size=None, audio_kernel_size=None, video_hidden=None, audio_hidden=None, video_output_dim=None,
                     audio_output_dim=None, quantised_training=False, **unused_params):
        iterations = iterations or FLAGS.jtmv2_iteration                                                      # :197
        add_batch_norm = add_batch_norm or FLAGS.jtmv2_add_batch_norm                                         # :198 (C23)
        video_anchor_size = int(video_anchor_size or FLAGS.jtmv2_video_anchor_size)                           # :199-206
        audio_anchor_size = int(audio_anchor_size or FLAGS.jtmv2_audio_anchor_size)
        video_hidden = int(video_hidden or FLAGS.jtmv2_video_hidden)
        audio_hidden = int(audio_hidden or FLAGS.jtmv2_audio_hidden)
        video_kernel_size = int(video_kernel_size or FLAGS.jtmv2_video_kernel_size)
        audio_kernel_size = int(audio_kernel_size or FLAGS.jtmv2_audio_kernel_size)
        video_output_dim = int(video_output_dim or FLAGS.jtmv2_video_output_dim)
        audio_output_dim = int(audio_output_dim or FLAGS.jtmv2_audio_output_dim)
        use_attention, use_relu = FLAGS.jtmv2_use_attention, FLAGS.jtmv2_use_relu                             # :207-208
        # sample_random_frames and hidden_size are accepted and read nowhere, as written
        quantised, model_input, max_frames, feature_size = _random_frames(model_input, num_frames, iterations, frame_uniform)  # :210-216
        if feature_size <= 1024:
            raise ValueError("JuhanTestModelV2 slices a 1024-wide video and a 128-wide audio stream out of its input "
                             f"(frame_level_models.py:245-249); got {feature_size} features")
        streams = (("video", 1024, video_anchor_size, video_kernel_size, video_hidden, video_output_dim, slice(0, 1024)),
                   ("audio", feature_size - 1024, audio_anchor_size, audio_kernel_size, audio_hidden, audio_output_dim, slice(1024, None)))
        features = _stream_features(quantised, model_input, num_frames, iterations, frame_uniform, False, is_training,
                                    quantised_training)                                                       # (no input batch norm)
        v2_modules = [video_pooling_modules.TriangulationNsCnnIndirectAttentionModule(
            feature_size=D, max_frames=max_frames, anchor_size=K, self_attention=use_attention, hidden_layer_size=H, kernel_size=F,
            output_dim=O, add_relu=use_relu, batch_norm=add_batch_norm, is_training=is_training, scope_id=None)
            for _, D, K, F, H, O, _ in streams]                                                               # :218-242
        fused = bool(FLAGS.triangulation_v2_fused and model_input.is_cuda and max_frames >= 2)
        acts = []
        for (name, *_), x, module in zip(streams, features, v2_modules):
            with vs.variable_scope(name + "_triangulation_embedding"):                                        # :244-250
                acts.append(module.head(*module.fused_pool(x.contiguous())) if fused else module.forward(x))
        activation = torch.cat(acts, 1)                                                                       # :252
        if add_batch_norm:
            activation = layers.batch_norm(activation, is_training, "final_activation_bn")                    # :254-260
        aggregated_model = getattr(video_level_models, "ClassLearningFourNnModel")
        return aggregated_model().create_model(model_input=activation, vocab_size=vocab_size, is_training=is_training,
                                               **unused_params)                                              # :262-268


class JuhanTestModelV3(models.BaseModel):
    """One TriangulationMagnitudeNsCnnIndirectAttentionModule per stream (JuhanTestModelV2's pooling with the rolled differences
    normalised again, both convolutions rectified and the two norm columns appended: "magnitude preserving"), the two streams joined
    WITHOUT a batch norm, and the classifier FLAGS.jtmv3_video_level_model names (frame_level_models.py:302-378).  No input batch norm.
    As written: SURVEY App. C29, C32, C33, C39, C42-C44 (and C23).

    On the GPU with FLAGS.triangulation_v3_fused each stream's pooling goes through ops.triangulation_magnitude_moments: no
    [(B*T), K*D] tensor (419 MB at the video defaults B = 16, T = 200, K = 32, D = 1024) is written; otherwise the module's ``pool``
    materialises them.  The variables and the results are the same either way.  ``frame_uniform`` [B, iterations] replaces the random draw
    of SampleRandomFrames; ``video_anchor_size``, ``audio_anchor_size``, ``video_kernel_size``, ``audio_kernel_size``, ``video_hidden``,
    ``audio_hidden``, ``video_output_dim`` and ``audio_output_dim`` override the flags (the reference reads the flags only)."""

    def create_model(self, model_input, vocab_size, num_frames, iterations=None, add_batch_norm=None, sample_random_frames=None,
                     hidden_size=None, is_training=True, frame_uniform=None, video_anchor_size=None, audio_anchor_size=None,
                     video_kernel_size=None, audio_kernel_size=None, video_hidden=None, audio_hidden=None, video_output_dim=None,
                     audio_output_dim=None, quantised_training=False, **unused_params):
        iterations = iterations or FLAGS.jtmv3_iteration                                                      # :313
        add_batch_norm = add_batch_norm or FLAGS.jtmv3_add_batch_norm                                         # :314 (C23)
        video_anchor_size = int(video_anchor_size or FLAGS.jtmv3_video_anchor_size)                           # :315-322
        audio_anchor_size = int(audio_anchor_size or FLAGS.jtmv3_audio_anchor_size)
        video_hidden = int(video_hidden or FLAGS.jtmv3_video_hidden)
        audio_hidden = int(audio_hidden or FLAGS.jtmv3_audio_hidden)
        video_kernel_size = int(video_kernel_size or FLAGS.jtmv3_video_kernel_size)
        audio_kernel_size = int(audio_kernel_size or FLAGS.jtmv3_audio_kernel_size)
        video_output_dim = int(video_output_dim or FLAGS.jtmv3_video_output_dim)
        audio_output_dim = int(audio_output_dim or FLAGS.jtmv3_audio_output_dim)
        use_attention, use_relu = FLAGS.jtmv3_use_attention, FLAGS.jtmv3_use_relu                             # :323-324
        aggregated_model = getattr(video_level_models, FLAGS.jtmv3_video_level_model)                         # :325, :372-373 (raises)
        # sample_random_frames and hidden_size are accepted and read nowhere, as written
        quantised, model_input, max_frames, feature_size = _random_frames(model_input, num_frames, iterations, frame_uniform)  # :327-333
        if feature_size <= 1024:
            raise ValueError("JuhanTestModelV3 slices a 1024-wide video and a 128-wide audio stream out of its input "
                             f"(frame_level_models.py:363-368); got {feature_size} features")
        streams = (("video", 1024, video_anchor_size, video_kernel_size, video_hidden, video_output_dim),
                   ("audio", feature_size - 1024, audio_anchor_size, audio_kernel_size, audio_hidden, audio_output_dim))
        features = _stream_features(quantised, model_input, num_frames, iterations, frame_uniform, False, is_training,
                                    quantised_training)                                                       # (no input batch norm)
        v3_modules = [video_pooling_modules.TriangulationMagnitudeNsCnnIndirectAttentionModule(
            feature_size=D, max_frames=max_frames, anchor_size=K, self_attention=use_attention, hidden_layer_size=H, kernel_size=F,
            output_dim=O, add_relu=use_relu, add_norm=True, batch_norm=add_batch_norm, is_training=is_training, scope_id=None)
            for _, D, K, F, H, O in streams]                                                                  # :335-361
        fused = bool(FLAGS.triangulation_v3_fused and model_input.is_cuda and max_frames >= 2)
        acts = []
        for (name, *_), x, module in zip(streams, features, v3_modules):
            with vs.variable_scope(name + "_triangulation_embedding"):                                        # :363-369
                acts.append(module.head(*module.fused_pool(x.contiguous())) if fused else module.forward(x))
        activation = torch.cat(acts, 1)                                                                       # :371 (no batch norm behind it)
        return aggregated_model().create_model(model_input=activation, vocab_size=vocab_size, is_training=is_training,
                                               **unused_params)                                              # :374-378


class JuhanTestModelV4(models.BaseModel):
    """One TriangulationMagnitudeNsCnnNetVladModule per stream (JuhanTestModelV3's front end -- the twice-normalised embedding, the
    rectified per-anchor convolutions, the two norm columns -- handed per frame to a loupe_modules.NetVLAD per stream and a projection
    onto ``*_hidden`` in place of V3's moments), the two streams joined WITHOUT a batch norm, and the classifier
    FLAGS.jtmv3_video_level_model names: line :434 reads V3's flag, not jtmv4_video_level_model (frame_level_models.py:411-487).  No input
    batch norm.  As written / resolved: SURVEY App. C29, C45-C47 (and C23).

    On the GPU with FLAGS.triangulation_v4_fused each stream's per-frame features come from ops.triangulation_magnitude_frames: no
    [(B*T), K*D] tensor (419 MB at the video defaults B = 16, T = 200, K = 32, D = 1024) is written; otherwise the module's ``frames``
    materialises them.  The variables and the results are the same either way.  At the defaults the two video ``hidden1_weights`` are
    [256 * 2080, 2048], 4.4 GB each in fp32; NetVladV1's factored / early update routes of its hidden1_weights are NOT extended to them.
    ``frame_uniform`` [B, iterations] replaces the random draw of SampleRandomFrames; ``video_anchor_size``, ``audio_anchor_size``,
    ``video_kernel_size``, ``audio_kernel_size``, ``video_hidden``, ``audio_hidden``, ``video_output_dim``, ``audio_output_dim`` and
    ``cluster_size`` override the flags (the reference reads the flags only, and writes 256 clusters into the module)."""

    def create_model(self, model_input, vocab_size, num_frames, iterations=None, add_batch_norm=None, sample_random_frames=None,
                     hidden_size=None, is_training=True, frame_uniform=None, video_anchor_size=None, audio_anchor_size=None,
                     video_kernel_size=None, audio_kernel_size=None, video_hidden=None, audio_hidden=None, video_output_dim=None,
                     audio_output_dim=None, cluster_size=None, quantised_training=False, **unused_params):
        iterations = iterations or FLAGS.jtmv4_iteration                                                      # :422
        add_batch_norm = add_batch_norm or FLAGS.jtmv4_add_batch_norm                                         # :423 (C23)
        video_anchor_size = int(video_anchor_size or FLAGS.jtmv4_video_anchor_size)                           # :424-431
        audio_anchor_size = int(audio_anchor_size or FLAGS.jtmv4_audio_anchor_size)
        video_hidden = int(video_hidden or FLAGS.jtmv4_video_hidden)
        audio_hidden = int(audio_hidden or FLAGS.jtmv4_audio_hidden)
        video_kernel_size = int(video_kernel_size or FLAGS.jtmv4_video_kernel_size)
        audio_kernel_size = int(audio_kernel_size or FLAGS.jtmv4_audio_kernel_size)
        video_output_dim = int(video_output_dim or FLAGS.jtmv4_video_output_dim)
        audio_output_dim = int(audio_output_dim or FLAGS.jtmv4_audio_output_dim)
        cluster_size = int(cluster_size or FLAGS.jtmv4_cluster_size)
        use_attention, use_relu = FLAGS.jtmv4_use_attention, FLAGS.jtmv4_use_relu                             # :432-433
        aggregated_model = getattr(video_level_models, FLAGS.jtmv3_video_level_model)                         # :434 (C47), :481-482 (raises)
        # sample_random_frames and hidden_size are accepted and read nowhere, as written
        quantised, model_input, max_frames, feature_size = _random_frames(model_input, num_frames, iterations, frame_uniform)  # :436-442
        if feature_size <= 1024:
            raise ValueError("JuhanTestModelV4 slices a 1024-wide video and a 128-wide audio stream out of its input "
                             f"(frame_level_models.py:472-477); got {feature_size} features")
        streams = (("video", 1024, video_anchor_size, video_kernel_size, video_hidden, video_output_dim),
                   ("audio", feature_size - 1024, audio_anchor_size, audio_kernel_size, audio_hidden, audio_output_dim))
        features = _stream_features(quantised, model_input, num_frames, iterations, frame_uniform, False, is_training,
                                    quantised_training)                                                       # (no input batch norm)
        v4_modules = [video_pooling_modules.TriangulationMagnitudeNsCnnNetVladModule(
            feature_size=D, max_frames=max_frames, anchor_size=K, self_attention=use_attention, hidden_layer_size=H, kernel_size=F,
            output_dim=O, add_relu=use_relu, add_norm=True, batch_norm=add_batch_norm, is_training=is_training, scope_id=None,
            cluster_size=cluster_size) for _, D, K, F, H, O in streams]                                       # :444-470
        fused = bool(FLAGS.triangulation_v4_fused and model_input.is_cuda and max_frames >= 2)
        acts = []
        for (name, *_), x, module in zip(streams, features, v4_modules):
            with vs.variable_scope(name + "_triangulation_embedding"):                                        # :472-478
                acts.append(module.head(*module.fused_frames(x.contiguous())) if fused else module.forward(x))
        activation = torch.cat(acts, 1)                                                                       # :480 (no batch norm behind it)
        return aggregated_model().create_model(model_input=activation, vocab_size=vocab_size, is_training=is_training,
                                               **unused_params)                                              # :483-487


class TriangulationRelationalModel(models.BaseModel):
    """The reference's recurrent model (frame_level_models.py:1511-1630): input batch norm, per stream the triangulation embedding of
    every sampled frame MATERIALISED as [B, T, D*K] -- the LSTM reads it -- and a one-layer LstmLastHiddenModule of hidden size D*K over it
    with the raw ``num_frames`` as sequence lengths (up to 300 against 30 sampled frames: a length above T means T), the two last hidden
    states concatenated, two hidden layers of width 2048 (``lstm_hidden_1`` / ``lstm_hidden_2``: batch norm, leaky_relu(0.2), dropout with
    keep probability 0.5 in training) and the mixture-of-experts classifier.

    The model does not run as written; the resolutions:
      * ``t_emb, det_reg = TriangulationEmbedding.forward(...)`` (:1570, :1576) unpacks a single tensor: the tensor is taken and
        det_reg = 0, the model's own ``else`` branch (:1583-1584);
      * ``getattr(video_level_models, "WillowMoeModel")`` (:1622) names a class that exists nowhere: MoeModel it is, WILLOW's
        mixture of experts with probability gating; det_reg goes into its ``**unused_params``;
      * ``add_batch_norm = add_batch_norm or FLAGS.batch_norm`` (:1524): False cannot switch it off (C23), kept.
    Frames are sampled (SampleRandomFrames) only when ``sample_random_frames`` or FLAGS.sample_random_frames is set, as written; there is
    no sampling otherwise and T is the input's max_frames.

    On the GPU with FLAGS.lstm_fused each stream's LSTM is ONE ops.lstm_layer call (csrc/lstm.hip); otherwise rnn_modules runs the
    per-step torch formulation.  The variables and the results are the same either way.  ``frame_uniform`` [B, iterations] replaces the
    random draw of SampleRandomFrames, ``dropout_masks`` {"hidden_1", "hidden_2"} (KEEP masks [B, 2048], non-zero = kept) the two
    dropout draws; ``video_anchor_size`` and ``audio_anchor_size`` override the flags (the reference reads the flags only).  fp32 frames
    only: a uint8 batch is dequantised before it gets here (train.normalize_input)."""

    HIDDEN = 2048
    KEEP_PROB = 0.5

    def create_model(self, model_input, vocab_size, num_frames, iterations=None, add_batch_norm=None, sample_random_frames=None,
                     hidden_size=None, is_training=True, frame_uniform=None, video_anchor_size=None, audio_anchor_size=None,
                     dropout_masks=None, **unused_params):
        from . import rnn_modules
        iterations = iterations or FLAGS.iterations                                                           # :1522
        random_frames = sample_random_frames or FLAGS.sample_random_frames                                    # :1523
        add_batch_norm = add_batch_norm or FLAGS.batch_norm                                                   # :1524 (C23)
        video_anchor_size = int(video_anchor_size or FLAGS.video_triangulation_anchor_size_v1)                # :1525
        audio_anchor_size = int(audio_anchor_size or FLAGS.audio_triangulation_anchor_size_v1)                # :1526
        if model_input.dtype == torch.uint8:
            raise LpmError("TriangulationRelationalModel reads fp32 frames: dequantise a uint8 batch first (train.normalize_input)")
        if random_frames:                                                                                     # :1528-1531
            model_input = model_utils.SampleRandomFrames(model_input, num_frames.reshape(-1, 1), iterations, uniform=frame_uniform)
        max_frames, feature_size = model_input.shape[1], model_input.shape[2]                                 # :1534-1535
        if feature_size <= 1024:
            raise ValueError("TriangulationRelationalModel slices a 1024-wide video and a 128-wide audio stream out of its input "
                             f"(frame_level_models.py:1570,1576); got {feature_size} features")
        dev = model_input.device
        masks = dropout_masks or {}
        reshaped_input = model_input.reshape(-1, feature_size)                                                # :1537
        streams = (("video_t_emb", 1024, video_anchor_size, slice(0, 1024)),
                   ("audio_t_emb", feature_size - 1024, audio_anchor_size, slice(1024, None)))
        t_embs = [video_pooling_modules.TriangulationEmbedding(D, max_frames, K, add_batch_norm, is_training) for _, D, K, _ in streams]
        lstms = [rnn_modules.LstmLastHiddenModule(lstm_size=D * K, lstm_layers=1, output_dim=D * K, num_frames=num_frames.reshape(-1),
                                                  scope_id=None) for _, D, K, _ in streams]                   # :1550-1559
        if add_batch_norm:
            reshaped_input = layers.batch_norm(reshaped_input, is_training, "input_bn")                       # :1561-1567
        lstm_outputs = []
        for (scope, D, K, cols), t_emb, lstm in zip(streams, t_embs, lstms):
            with vs.variable_scope(scope):                                                                    # :1569-1579
                emb = t_emb.forward(reshaped_input[:, cols]).reshape(-1, max_frames, D * K)                   # (a single tensor: C36)
                lstm_outputs.append(lstm.forward(emb))
        det_reg = 0                                                                                           # :1581-1584 (C36)
        activation = torch.cat(lstm_outputs, 1)                                                               # :1586

        def hidden(x, name, bn_scope, key):
            w = vs.get_variable(name, [x.shape[1], self.HIDDEN], vs.random_normal_initializer(1 / math.sqrt(self.HIDDEN)), device=dev)
            x = x.matmul(w)
            if add_batch_norm:
                x = layers.batch_norm(x, is_training, bn_scope)
            x = torch.nn.functional.leaky_relu(x, 0.2)
            if is_training:                                          # tf.nn.dropout(keep_prob=0.5) :1604, :1620
                keep = masks.get(key)
                if keep is None:
                    keep = torch.rand(x.shape, device=dev) < self.KEEP_PROB
                x = x * keep.to(device=dev).ne(0).to(x.dtype) / self.KEEP_PROB
            return x

        activation = hidden(activation, "lstm_hidden_1", "activation_1_bn", "hidden_1")                       # :1590-1604
        activation = hidden(activation, "lstm_hidden_2", "activation_2_bn", "hidden_2")                       # :1606-1620
        aggregated_model = getattr(video_level_models, "MoeModel")                                            # :1622 (C37)
        return aggregated_model().create_model(model_input=activation, vocab_size=vocab_size, is_training=is_training,
                                               det_reg=det_reg, **unused_params)                             # :1625-1630


class NetVladV2(models.BaseModel):
    """Paper prototype 2: attention-based cluster similarities (frame_level_models.py:2383-2513)."""

    def create_model(self, model_input, vocab_size, num_frames, iterations=None, add_batch_norm=None,
                     sample_random_frames=None, cluster_size=None, hidden_size=None, is_training=True,
                     dropout_masks=None, dropout_rate=None, quantised_training=False, **unused_params):
        iterations = iterations or FLAGS.iterations
        add_batch_norm = add_batch_norm or FLAGS.netvlad_add_batch_norm
        cluster_size = cluster_size or FLAGS.netvlad_cluster_size
        hidden1_size = hidden_size or FLAGS.netvlad_hidden_size
        relu, gating, remove_diag = FLAGS.netvlad_relu, FLAGS.gating, FLAGS.gating_remove_diag
        dm = dropout_masks or {}

        max_frames, feature_size = iterations, model_input.shape[2]
        has_audio = feature_size > 1024
        split = None
        if (has_audio and add_batch_norm and vs.default_store().summaries is None and ops.frame_sample_bn_split_ok(model_input, 1024, is_training, quantised_training)):
            # the two streams' blocks of the sampled, batch-normalised frames as two contiguous matrices straight from the frame-prep
            # kernel (ops.frame_sample_bn_split): same values, same variables; no column slices, copies or gradient concatenation
            bn = layers.bn_variables("input_bn", feature_size, model_input.device)
            split = ops.frame_sample_bn_split(model_input, num_frames.reshape(-1), iterations, *bn, is_training, 1024, quantised_training)
            reshaped_input = None
        else:
            reshaped_input = _sample_and_normalise(model_input, num_frames, iterations, add_batch_norm, is_training,
                                                   quantised_training=quantised_training)
            vs.summary("input_bn", reshaped_input)

        video_NetVLAD = video_pooling_modules.NetVladAttenCluster(1024, max_frames, cluster_size, add_batch_norm,
                                                                  is_training, "netvlad_rgb_scope")
        audio_NetVLAD = video_pooling_modules.NetVladAttenCluster(128, max_frames, cluster_size // 4, add_batch_norm,
                                                                  is_training, "netvlad_audio_scope")
        if split is not None:
            rgb, audio = split
        elif has_audio and reshaped_input.is_cuda:
            # one contiguous copy per stream (the encoder and the aggregation both want whole rows); their gradients come back as ONE
            # concatenation instead of two zero-filled [M, 1152] buffers, two slice copies and an add
            # (the copies do not carry the views' shared-gradient slot -- ops._SplitColumns.backward then concatenates the two
            # gradients, which is the point here; the slot mechanism itself serves NetVladV1, whose pooling ops write into it)
            rgb, audio = ops.split_columns(reshaped_input, 1024)
            rgb, audio = rgb.contiguous(), audio.contiguous()
        else:
            rgb, audio = reshaped_input[:, 0:1024], reshaped_input[:, 1024:]
        # (NetVladV1 runs its audio stream on a second HIP stream; here that was measured SLOWER -- 10.95 vs 10.84 ms per step at cfg-3,
        # tools/ab_flags.py: this model's audio stream attends over 300 frames, its launches are long enough to fill the chip by themselves)
        # The video descriptor leaves its pooling LAZILY NORMALISED where the projection can take it that way: the un-normalised sums,
        # written once by the aggregation kernel, + one scale per (clip, cluster) -- no finalize pass, and no tf.concat either (the
        # projection reads the two streams' blocks where they are)
        lazy_v = bool(FLAGS.netvlad_lazy_descriptor and model_input.is_cuda and model_input.shape[0] <= 128 and hidden1_size % 512 == 0
                      and ops.vlad_aggregate_lazy_ok(max_frames, 1024, cluster_size))
        with vs.variable_scope("video_VLAD"):
            vlad_video = video_NetVLAD.forward(rgb, dropout_mask=dm.get("video"), dropout_rate=dropout_rate, lazy=lazy_v)   # :2437-2438
            if vs.default_store().summaries is not None:
                vs.summary("vlad_video", ops.materialise(vlad_video))
        vlad_audio = None
        if has_audio:
            with vs.variable_scope("audio_VLAD"):
                vlad_audio = audio_NetVLAD.forward(audio, dropout_mask=dm.get("audio"), dropout_rate=dropout_rate)  # :2440-2441
                vs.summary("vlad_audio", vlad_audio)
        if lazy_v:
            if vs.default_store().summaries is not None:
                vm = ops.materialise(vlad_video)
                vs.summary("vlad", torch.cat([vm, vlad_audio], 1) if has_audio else vm)
            vlad = (vlad_video, vlad_audio)                                                     # :2445 inside the projection
        else:
            vlad = torch.cat([vlad_video, vlad_audio], 1) if has_audio else vlad_video          # :2445
            vs.summary("vlad", vlad)
        return _project_gate_classify(vlad, vocab_size, cluster_size, hidden1_size, add_batch_norm, relu, gating,
                                      remove_diag, is_training, **unused_params)
