"""Flag registry with the reference's names and defaults (absl/tf.flags in the reference:
frame_level_models.py:35,2197-2216; video_level_models.py:26-45; train.py:44-112)."""
from __future__ import annotations


class _Flags:
    def __init__(self):
        self.__dict__["_defaults"] = {}

    def define(self, name, default, help=""):  # noqa: A002
        self._defaults[name] = default
        self.__dict__[name] = default

    def reset(self):
        for k, v in self._defaults.items():
            self.__dict__[k] = v

    def __setattr__(self, k, v):
        if k not in self._defaults:
            raise AttributeError(f"unknown flag {k!r}")
        self.__dict__[k] = v


FLAGS = _Flags()
# frame_level_models.py
FLAGS.define("iterations", 30, "Number of frames per batch (frame_level_models.py:35)")
FLAGS.define("sample_random_frames", True, "unused by NetVladV1/V2 (uniform sampling, :2255)")
FLAGS.define("netvlad_add_batch_norm", True, ":2197")
FLAGS.define("netvlad_cluster_size", 256, ":2199")
FLAGS.define("netvlad_hidden_size", 1024, ":2201")
FLAGS.define("netvlad_relu", False, ":2203")
FLAGS.define("gating", True, ":2205")
FLAGS.define("gating_remove_diag", False, ":2207")
FLAGS.define("netvlad_encoder", True, "build extension: False = gated NetVLAD without the cluster encoders (BASELINE cfg-5)")
FLAGS.define("sample_random_frames", True, "frame_level_models.py:40: random frames (True) or a random contiguous sequence")
FLAGS.define("rgb_det_reg", 1e-4, "frame_level_models.py:2213: orthogonality penalty on the rgb cluster centres (WillowModelReg)")
FLAGS.define("audio_det_reg", 1e-4, "frame_level_models.py:2209: orthogonality penalty on the audio cluster centres")
FLAGS.define("netvlad_storage", "f32", "build extension: 'bf16' = the frames, logits / assignment and pooled descriptor of the NetVLAD "
             "streams live in HBM as bf16 with fp32 accumulation (BASELINE configs[4], 'Gated NetVLAD K=512 + MoE-4 ... bf16'); needs "
             "netvlad_encoder off, batch norm on, cluster_size a multiple of 512")
FLAGS.define("netvlad_lazy_descriptor", True, "build extension: NetVladV1's video pooling hands its cluster encoder the un-normalised "
             "residual sums [B, K, D] plus one scale per (clip, cluster); the encoder's block Functions apply the scale where they read "
             "the rows -- the pooled tensor is written once, there is no finalize pass and no transpose in the pooling backward.  "
             "NetVladV2 and the model without cluster encoders (bf16 storage) hand the same form, d-major, to the hidden projection "
             "(ops.projection_parts: the scale applied where the operand is read, no concat)")
FLAGS.define("fused_encoder_blocks", True, "build extension: run the V1 cluster encoder as two block Functions whose backward "
             "folds the gradient sums of shared tensors into GEMM accumulation / the layer-norm kernel (no add passes)")
FLAGS.define("descriptor_slots", True, "build extension: both encoders write their pooled descriptor into one shared buffer "
             "(no concat copy forward, no slice copies backward); needs fused_encoder_blocks")
FLAGS.define("mha_gradient_image", True, "build extension: inside the encoder block Functions the attention kernels write their "
             "result and the q/k/v gradients directly as the split-bf16 operand images of the projection GEMMs (no fp32 copies, no "
             "split passes)")
FLAGS.define("ln_gradient_image", True, "build extension: the FFN block's inner layer-norm backward writes the ReLU-masked "
             "gradient directly as the split-bf16 operand image of the FFN backward GEMMs")
FLAGS.define("input_bn_grad_shortcut", True, "build extension: NetVladV1 training forms input_bn's gamma / beta gradients in closed "
             "form from quantities the pooling backward already has; the [B*S, 1152] input gradient is never computed")
FLAGS.define("ln_pair_forward", True, "build extension: the two layer norms at the end of the V1 encoder share a residual and run "
             "as one three-pass kernel sequence (the first one's output is never stored)")
FLAGS.define("audio_side_stream", True, "build extension: run the audio stream (NetVLAD + encoder, ~100 latency-bound small "
             "launches per step) on a second HIP stream next to the video stream")
FLAGS.define("dense_precision", "bf16x3", "build extension: encoder dense GEMMs as split-bf16 ('bf16x3', ~4e-6) or 'f32'")
FLAGS.define("dense_arithmetic", "fp16x2", "build extension, the encoders' dense GEMMs of NetVladV1 and NetVladV2 (q|k|v, output transform, "
             "both feed-forward layers and every input / weight gradient of them): 'fp16x2' = fp16 (hi, lo) operand planes with per-tensor "
             "power-of-two scales the trainer measures at one step and applies two steps later (ops.OperandScales; the first two steps of a "
             "run stay on split-bf16) -- forward products keep three terms (~1e-6), input gradients two (the weight rounded once to fp16: "
             "1.4e-4 per GEMM), weight gradients one (both operands rounded once: 2e-4, not carried further down the backward) -- against "
             "split-bf16's three terms everywhere; 'bf16x3' = split-bf16 throughout (rounds 1-4)")
FLAGS.define("wtm_video_anchor_size", 64, "RegularizedTriangulationModel (frame_level_models.py:1160): anchors of the video stream")
FLAGS.define("wtm_audio_anchor_size", 64, "RegularizedTriangulationModel (frame_level_models.py:1161): anchors of the audio stream")
FLAGS.define("triangulation_fused", True, "build extension: on the GPU each stream of RegularizedTriangulationModel is ONE ops.triangulation_pool "
             "call (csrc/triangulation_pool.hip: the four pooled vectors without any [B, T, K*D] tensor); False: the materialising modules of "
             "video_pooling_modules / aggregation_modules compose it (the CPU path; same variables, same results)")
FLAGS.define("sftm_iterations", 64, "SoftAttentionTriangulationModel (frame_level_models.py:945): sampled frames per clip")
FLAGS.define("sftm_add_batch_norm", True, "SoftAttentionTriangulationModel (:947): batch norm on the streams and after every projection")
FLAGS.define("sftm_video_anchor_size", 128, "SoftAttentionTriangulationModel (:951): anchors of the video stream")
FLAGS.define("sftm_audio_anchor_size", 16, "SoftAttentionTriangulationModel (:953): anchors of the audio stream")
FLAGS.define("sftm_video_bottleneck", 100, "SoftAttentionTriangulationModel (:955): width of the video stream's projections")
FLAGS.define("sftm_audio_bottleneck", 16, "SoftAttentionTriangulationModel (:957): width of the audio stream's projections")
FLAGS.define("soft_attention_fused", True, "build extension: on the GPU each stream of SoftAttentionTriangulationModel is ONE "
             "ops.triangulation_attention_pool call (csrc/triangulation_attention.hip: the Grams, the softmax weights and the four pooled "
             "vectors without any [B, T, K*D] tensor); False: the materialising modules of video_pooling_modules / aggregation_modules "
             "compose it (the CPU path; same variables, same results)")
FLAGS.define("tccm_iterations", 200, "TriangulationCnnClusterModel (frame_level_models.py:737): sampled frames per clip")
FLAGS.define("tccm_add_batch_norm", True, "TriangulationCnnClusterModel (:739): batch norm on the streams and on each stream's pooled vector")
FLAGS.define("tccm_video_anchor_size", 128, "TriangulationCnnClusterModel (:743): anchors of the video stream")
FLAGS.define("tccm_audio_anchor_size", 32, "TriangulationCnnClusterModel (:745): anchors of the audio stream")
FLAGS.define("tccm_video_kernel_size", 128, "TriangulationCnnClusterModel (:747): filters per anchor of the video stream's two convolutions")
FLAGS.define("tccm_audio_kernel_size", 128, "TriangulationCnnClusterModel (:749): filters per anchor of the audio stream's two convolutions")
FLAGS.define("tccm_video_hidden", 2048, "TriangulationCnnClusterModel (:751): width of the video stream's hidden layer")
FLAGS.define("tccm_audio_hidden", 256, "TriangulationCnnClusterModel (:753): width of the audio stream's hidden layer")
FLAGS.define("triangulation_cnn_fused", True, "build extension: on the GPU each stream of TriangulationCnnClusterModel is ONE "
             "ops.triangulation_cnn_pool call (csrc/triangulation_mean.hip: the Gram, the softmax weights and the two pooled means without "
             "any [B, T, K*D] tensor, then the per-anchor convolution on the pooled means); False: the materialising modules of "
             "video_pooling_modules / aggregation_modules compose it (the CPU path; same variables, same results)")
FLAGS.define("jtmv5_iteration", 30, "JuhanTestModelV5 (frame_level_models.py:491): sampled frames per clip")
FLAGS.define("jtmv5_add_batch_norm", True, "JuhanTestModelV5 (:493): batch norm on the streams and inside each stream's module")
FLAGS.define("jtmv5_video_anchor_size", 256, "JuhanTestModelV5 (:497): anchors of the video stream")
FLAGS.define("jtmv5_audio_anchor_size", 32, "JuhanTestModelV5 (:499): anchors of the audio stream")
FLAGS.define("jtmv5_video_kernel_size", 512, "JuhanTestModelV5 (:501): filters per anchor of the video stream's two convolutions")
FLAGS.define("jtmv5_audio_kernel_size", 64, "JuhanTestModelV5 (:503): filters per anchor of the audio stream's two convolutions")
FLAGS.define("jtmv5_video_hidden", 2048, "JuhanTestModelV5 (:505): width of the video stream's two hidden layers")
FLAGS.define("jtmv5_video_output_dim", 4096, "JuhanTestModelV5 (:507): width of the video stream's fused output")
FLAGS.define("jtmv5_audio_hidden", 256, "JuhanTestModelV5 (:509): width of the audio stream's two hidden layers")
FLAGS.define("jtmv5_audio_output_dim", 512, "JuhanTestModelV5 (:511): width of the audio stream's fused output")
FLAGS.define("triangulation_v5_fused", True, "build extension: on the GPU each stream of JuhanTestModelV5 is ONE ops.triangulation_cnn_moments "
             "call (csrc/triangulation_moments.hip: the per-anchor convolutions of the embedding and of its rolled differences over every "
             "frame, and the mean and variance over the frames, without any [B, T, K*D] tensor); False: TriangulationV5Module.forward "
             "materialises it (the CPU path; same variables, same results)")
FLAGS.define("jtmv1_iteration", 30, "JuhanTestModelV1 (frame_level_models.py:59): sampled frames per clip")
FLAGS.define("jtmv1_add_batch_norm", True, "JuhanTestModelV1 (:61): batch norm inside each stream's module")
FLAGS.define("jtmv1_sample_random_frames", True, "JuhanTestModelV1 (:63): defined and read nowhere, as written")
FLAGS.define("jtmv1_video_anchor_size", 64, "JuhanTestModelV1 (:65): anchors of the video stream")
FLAGS.define("jtmv1_audio_anchor_size", 16, "JuhanTestModelV1 (:67): anchors of the audio stream")
FLAGS.define("jtmv1_video_hidden", 1024, "JuhanTestModelV1 (:69): width of the video stream's hidden layer")
FLAGS.define("jtmv1_video_output_dim", 2048, "JuhanTestModelV1 (:71): width of the video stream's fused output")
FLAGS.define("jtmv1_audio_hidden", 128, "JuhanTestModelV1 (:73): width of the audio stream's hidden layer")
FLAGS.define("jtmv1_audio_output_dim", 256, "JuhanTestModelV1 (:75): width of the audio stream's fused output")
FLAGS.define("jtmv1_use_attention", True, "JuhanTestModelV1 (:77): the soft-attention weights on the pooled means")
FLAGS.define("jtmv1_use_relu", True, "JuhanTestModelV1 (:79): relu behind the hidden and the fusion layer")
FLAGS.define("triangulation_v1_fused", False, "build extension: on the GPU each stream of JuhanTestModelV1 pools through "
             "ops.triangulation_bn_moments (csrc/triangulation_bn_moments.hip: the batch-norm statistics, the Grams, the softmax weights and "
             "the mean and variance over the frames without any [B, T, K*D] tensor); False: TriangulationCnnIndirectAttentionModule.pool "
             "materialises it (the CPU path; same variables, same results).  Off until tools/bench_triangulation_v1.py has shown the fused "
             "path not slower at both model-default shapes (profiles/bench_triangulation_v1.json)")
FLAGS.define("jtmv2_iteration", 200, "JuhanTestModelV2 (frame_level_models.py:158): sampled frames per clip")
FLAGS.define("jtmv2_add_batch_norm", True, "JuhanTestModelV2 (:160): batch norm inside each stream's module and on the joined streams")
FLAGS.define("jtmv2_sample_random_frames", True, "JuhanTestModelV2 (:162): defined and read nowhere, as written")
FLAGS.define("jtmv2_video_anchor_size", 32, "JuhanTestModelV2 (:164): anchors of the video stream")
FLAGS.define("jtmv2_audio_anchor_size", 8, "JuhanTestModelV2 (:166): anchors of the audio stream")
FLAGS.define("jtmv2_video_kernel_size", 64, "JuhanTestModelV2 (:168): filters per anchor of the video stream's two convolutions")
FLAGS.define("jtmv2_audio_kernel_size", 16, "JuhanTestModelV2 (:170): filters per anchor of the audio stream's two convolutions")
FLAGS.define("jtmv2_video_hidden", 2048, "JuhanTestModelV2 (:172): width of the video stream's hidden layer")
FLAGS.define("jtmv2_video_output_dim", 2048, "JuhanTestModelV2 (:174): width of the video stream's fused output")
FLAGS.define("jtmv2_audio_hidden", 256, "JuhanTestModelV2 (:176): width of the audio stream's hidden layer")
FLAGS.define("jtmv2_audio_output_dim", 256, "JuhanTestModelV2 (:178): width of the audio stream's fused output")
FLAGS.define("jtmv2_use_attention", True, "JuhanTestModelV2 (:180): the soft-attention weights on the pooled means")
FLAGS.define("jtmv2_use_relu", False, "JuhanTestModelV2 (:182): relu behind the hidden and the fusion layer")
FLAGS.define("triangulation_v2_fused", False, "build extension: on the GPU each stream of JuhanTestModelV2 pools through "
             "ops.triangulation_cnn_attention_moments (the norms, the Grams, the softmax weights, the per-anchor convolutions of the embedding "
             "and of its rolled differences and their weighted mean and variance over the frames, without any [B, T, K*D] tensor); False: "
             "TriangulationNsCnnIndirectAttentionModule.pool materialises it (the CPU path; same variables, same results).  Off: "
             "tools/bench_triangulation_v2.py measured forward + backward of one stream at 37.3 ms fused against 11.6 ms at (B, T, D, K, F) = "
             "(16, 200, 1024, 32, 64) and 3.44 against 1.51 ms at (16, 200, 128, 8, 16) (with 148 against 2594 MiB and 19 against 125 MiB "
             "allocated), and the default is on only if the fused path is not slower at both (profiles/bench_triangulation_v2.json)")
FLAGS.define("jtmv3_iteration", 200, "JuhanTestModelV3 (frame_level_models.py:272): sampled frames per clip")
FLAGS.define("jtmv3_add_batch_norm", True, "JuhanTestModelV3 (:274): batch norm inside each stream's module")
FLAGS.define("jtmv3_sample_random_frames", True, "JuhanTestModelV3 (:276): defined and read nowhere, as written")
FLAGS.define("jtmv3_video_anchor_size", 32, "JuhanTestModelV3 (:278): anchors of the video stream")
FLAGS.define("jtmv3_audio_anchor_size", 8, "JuhanTestModelV3 (:280): anchors of the audio stream")
FLAGS.define("jtmv3_video_kernel_size", 64, "JuhanTestModelV3 (:282): filters per anchor of the video stream's two convolutions")
FLAGS.define("jtmv3_audio_kernel_size", 16, "JuhanTestModelV3 (:284): filters per anchor of the audio stream's two convolutions")
FLAGS.define("jtmv3_video_hidden", 2048, "JuhanTestModelV3 (:286): width of the video stream's hidden layer")
FLAGS.define("jtmv3_video_output_dim", 2048, "JuhanTestModelV3 (:288): width of the video stream's fused output")
FLAGS.define("jtmv3_audio_hidden", 256, "JuhanTestModelV3 (:290): width of the audio stream's hidden layer")
FLAGS.define("jtmv3_audio_output_dim", 256, "JuhanTestModelV3 (:292): width of the audio stream's fused output")
FLAGS.define("jtmv3_use_attention", True, "JuhanTestModelV3 (:294): the soft-attention weights on the pooled means")
FLAGS.define("jtmv3_use_relu", False, "JuhanTestModelV3 (:296): relu behind the hidden and the fusion layer")
FLAGS.define("jtmv3_video_level_model", "ClassLearningFourNnModel", "JuhanTestModelV3 (:298): the classifier, a class of video_level_models "
             "taken by name")
FLAGS.define("triangulation_v3_fused", False, "build extension: on the GPU each stream of JuhanTestModelV3 pools through "
             "ops.triangulation_magnitude_moments (both norms, the Grams of the embedding and of its normalised rolled differences, the softmax "
             "weights, the rectified per-anchor convolutions and the weighted mean and variance over the frames of [relu(conv) | norm], without "
             "any [B, T, K*D] tensor); False: TriangulationMagnitudeNsCnnIndirectAttentionModule.pool materialises it (the CPU path; same "
             "variables, same results).  Off: tools/bench_triangulation_v3.py measured forward + backward of one stream at 44.7 ms fused against "
             "14.7 ms at (B, T, D, K, F) = (16, 200, 1024, 32, 64) and 4.08 against 1.79 ms at (16, 200, 128, 8, 16) (with 149 against 3048 MiB "
             "and 19 against 125 MiB allocated), and the default is on only if the fused path is not slower at both "
             "(profiles/bench_triangulation_v3.json)")
FLAGS.define("jtmv4_iteration", 200, "JuhanTestModelV4 (frame_level_models.py:381): sampled frames per clip")
FLAGS.define("jtmv4_add_batch_norm", True, "JuhanTestModelV4 (:383): batch norm inside each stream's module")
FLAGS.define("jtmv4_sample_random_frames", True, "JuhanTestModelV4 (:385): defined and read nowhere, as written")
FLAGS.define("jtmv4_video_anchor_size", 32, "JuhanTestModelV4 (:387): anchors of the video stream")
FLAGS.define("jtmv4_audio_anchor_size", 8, "JuhanTestModelV4 (:389): anchors of the audio stream")
FLAGS.define("jtmv4_video_kernel_size", 64, "JuhanTestModelV4 (:391): filters per anchor of the video stream's two convolutions")
FLAGS.define("jtmv4_audio_kernel_size", 16, "JuhanTestModelV4 (:393): filters per anchor of the audio stream's two convolutions")
FLAGS.define("jtmv4_video_hidden", 2048, "JuhanTestModelV4 (:395): output width of the video stream's two NetVLADs")
FLAGS.define("jtmv4_video_output_dim", 2048, "JuhanTestModelV4 (:397): width of the video stream's fused output")
FLAGS.define("jtmv4_audio_hidden", 256, "JuhanTestModelV4 (:399): output width of the audio stream's two NetVLADs")
FLAGS.define("jtmv4_audio_output_dim", 256, "JuhanTestModelV4 (:401): width of the audio stream's fused output")
FLAGS.define("jtmv4_use_attention", True, "JuhanTestModelV4 (:403): handed to the module as self_attention, which never reads it (App. C46)")
FLAGS.define("jtmv4_use_relu", False, "JuhanTestModelV4 (:405): relu behind the NetVLADs' batch norms and the fusion layer")
FLAGS.define("jtmv4_video_level_model", "ClassLearningFourNnModel", "JuhanTestModelV4 (:407): defined and read nowhere, as written: the "
             "classifier is taken from jtmv3_video_level_model (:434, App. C47)")
FLAGS.define("jtmv4_cluster_size", 256, "build extension: clusters of each of JuhanTestModelV4's four NetVLADs (the reference writes 256 into "
             "the module, video_pooling_modules.py:1043)")
FLAGS.define("triangulation_v4_fused", False, "build extension: on the GPU each stream of JuhanTestModelV4 takes its per-frame features from "
             "ops.triangulation_magnitude_frames (both norms, the rectified per-anchor convolutions and the norm columns written as the rows "
             "the two NetVLADs read, without any [B, T, K*D] tensor); False: TriangulationMagnitudeNsCnnNetVladModule.frames materialises "
             "them (the CPU path; same variables, same results).  Off: tools/bench_triangulation_v4.py measured forward + backward of one stream's "
             "features at 13.8 ms fused against 8.3 ms at (B, T, D, K, F) = (16, 200, 1024, 32, 64) and 1.55 against 0.89 ms at "
             "(16, 200, 128, 8, 16) (with 192 against 2637 MiB and 18 against 132 MiB allocated; the whole module 20.1 against 14.3 ms and "
             "3.18 against 2.54 ms), and the default is on only if the fused path is not slower at both "
             "(profiles/bench_triangulation_v4.json)")
FLAGS.define("jtmv6_iteration", 30, "JuhanTestModelV6 (frame_level_models.py:610): sampled frames per clip")
FLAGS.define("jtmv6_add_batch_norm", True, "JuhanTestModelV6 (:612): batch norm on the streams and inside each stream's module")
FLAGS.define("jtmv6_sample_random_frames", True, "JuhanTestModelV6 (:614): read nowhere, as written: the frames are always sampled at random")
FLAGS.define("jtmv6_video_anchor_size", 256, "JuhanTestModelV6 (:616): anchors of the video stream")
FLAGS.define("jtmv6_audio_anchor_size", 32, "JuhanTestModelV6 (:618): anchors of the audio stream")
FLAGS.define("jtmv6_video_kernel_size", 512, "JuhanTestModelV6 (:620): handed to the video module, read nowhere, as written")
FLAGS.define("jtmv6_audio_kernel_size", 64, "JuhanTestModelV6 (:622): handed to the audio module, read nowhere, as written")
FLAGS.define("jtmv6_video_hidden", 2048, "JuhanTestModelV6 (:624): handed to the video module, read nowhere, as written")
FLAGS.define("jtmv6_video_output_dim", 4096, "JuhanTestModelV6 (:626): width of the video stream's output")
FLAGS.define("jtmv6_audio_hidden", 256, "JuhanTestModelV6 (:628): handed to the audio module, read nowhere, as written")
FLAGS.define("jtmv6_audio_output_dim", 512, "JuhanTestModelV6 (:630): width of the audio stream's output")
FLAGS.define("jtmv6_video_cluster_size", 64, "JuhanTestModelV6 (:632): attention clusters of the video stream.  With the defaults the video "
             "stream's hidden_weight is [64 * 256 * 1024, 4096], 275 GB: the model refuses it before any variable is created")
FLAGS.define("jtmv6_audio_cluster_size", 8, "JuhanTestModelV6 (:634): attention clusters of the audio stream")
FLAGS.define("triangulation_v6_fused", True, "build extension: on the GPU each stream of JuhanTestModelV6 pools through "
             "ops.triangulation_onefc_pool (csrc/triangulation_onefc.hip: both normalisations, the folded batch norm, the logits, the "
             "cluster sums and the shifted row norms straight from the frames, without any [B*T, K*D] tensor); False: "
             "TriangulationV6Module.pool materialises them (the CPU path; same variables, same results).  On: tools/bench_triangulation_v6.py "
             "measured forward + backward of one stream's pooling at 0.82 ms fused against 0.91 ms at (B, T, D, K, C) = (16, 30, 128, 32, 8), "
             "0.88 against 1.02 ms at (16, 30, 1024, 16, 8) and 1.47 against 2.99 ms at (80, 30, 1024, 16, 8) (with 11 against 201 MiB, 41 "
             "against 194 MiB and 202 against 971 MiB allocated), and the default is on only if the fused path is not slower at all three "
             "(profiles/bench_triangulation_v6.json, DESIGN.md section 34)")
FLAGS.define("batch_norm", True, "TriangulationRelationalModel (frame_level_models.py:1503): True iff add batch normalization")
FLAGS.define("audio_triangulation_anchor_size_v1", 4, "TriangulationRelationalModel (:1505): anchors of the audio stream")
FLAGS.define("video_triangulation_anchor_size_v1", 16, "TriangulationRelationalModel (:1507): anchors of the video stream")
FLAGS.define("lstm_fused", True, "build extension: on the GPU every layer of rnn_modules' LSTM stacks whose hidden size is a multiple of 128 "
             "is ONE ops.lstm_layer call (csrc/lstm.hip: a kernel per time step each way -- the recurrent product on exact-fp32 MFMAs with "
             "the gate arithmetic, the length mask and the state update in its epilogue -- between three large GEMMs outside the time "
             "loop); False: rnn_modules._lstm_layer_host runs the layer as a per-step torch formulation (the CPU path; same variables, "
             "same results).  On: tools/bench_lstm.py measured forward + backward of one layer at 0.93 ms fused against 10.6 ms per step at "
             "(B, T, In, H) = (16, 30, 512, 512) and 82.3 against 175.3 ms at (16, 30, 16384, 16384), and the default is on only if the "
             "fused route is not slower at both shapes (profiles/bench_lstm.json, DESIGN.md section 27)")
FLAGS.define("class_filter_fused", True, "build extension: on the GPU the three glue stages of the class filter behind MoeModel2 / "
             "JuhanMoeModel (bias, relu / leaky_relu / sigmoid, tf.layers.batch_normalization over the batch, the dropout mask, the "
             "residual add) are ONE ops.class_filter launch each way per stage (csrc/class_filter.hip) between the three library GEMMs; "
             "False: the torch formulation (the CPU path; same variables, same results).  On: tools/bench_class_filter.py measured forward "
             "+ backward of the three stages together at 0.29 ms fused against 0.63 ms at (B, V) = (128, 3862) and 0.49 against 0.94 ms at "
             "(1024, 3862) -- the bias + sigmoid stage alone is SLOWER fused, 0.055 against 0.038 ms and 0.065 against 0.050 ms -- and one "
             "Trainer.step of MoeModel2 / JuhanMoeModel at 2.17 / 2.29 ms against 2.47 / 2.57 ms and 6.19 / 6.28 against 6.62 / 6.71 ms; the "
             "default is on only if the fused route is faster at both shapes (profiles/bench_class_filter.json, DESIGN.md section 36)")
FLAGS.define("class_rows_fused", False, "build extension: on the GPU the row-wise glue over [B, V] class scores -- FishMoeModel3's "
             "bias + residual + LayerNorm and bias + softmax, the clipped gates (relu6, -relu6(-t)) + residual (+ softmax) of "
             "attention_modules' PGateModule / PnGateModule / NpGateModule -- is ONE ops.class_rows launch forward and one or two "
             "backward per stage (csrc/class_rows.hip) behind its library GEMM; False: the torch formulation (the CPU path; same "
             "variables, same results).  Off: tools/bench_class_rows.py measured forward + backward of FishMoeModel3's two row stages together at 0.165 ms fused against 0.225 ms at (B, V) = (1024, 3862) but 0.196 against 0.181 ms at (128, 3862), where both routes are bound by the host and an autograd node written in Python costs more than torch's own; the PN gate's two stages 0.099 against 0.113 ms and 0.100 against 0.100 ms; one Trainer.step of FishMoeModel3 5.90 against 5.96 ms and 2.13 against 2.12 ms; the default is on only if the fused route is faster at both shapes "
             "(profiles/bench_class_rows.json, DESIGN.md section 37)")
FLAGS.define("wtm_projection_l1", 1e-5, "layers.l1_l2_regularizer(1e-5) on dis_projection_2 / temp_projection_2 (frame_level_models.py:1272,1287): "
             "tf.contrib's first positional argument is scale_l1")
FLAGS.define("wtm_projection_l2", 1.0, "... and its scale_l2 keeps the default 1.0: the penalty is l1 * sum |w| + l2 * sum(w^2) / 2 (SURVEY App. B)")
# video_level_models.py
FLAGS.define("moe_num_mixtures", 2, "video_level_models.py:27")
FLAGS.define("moe_l2", 1e-8, ":35")
FLAGS.define("moe_low_rank_gating", -1, ":38")
FLAGS.define("moe_prob_gating", False, ":41")
FLAGS.define("moe_prob_gating_input", "prob", ":44")
# train.py
FLAGS.define("batch_size", 1024, "train.py:78")
FLAGS.define("label_loss", "CrossEntropyLoss", "train.py:80: the class of losses the run optimises (CrossEntropyLoss, HingeLoss, SoftmaxLoss)")
FLAGS.define("label_loss_fused", False, "build extension: HingeLoss / SoftmaxLoss of fp32 predictions and bool / uint8 labels on the GPU run as "
             "ops.label_loss (csrc/label_loss.hip: one row-reduction launch plus the batch mean forward, one element-wise launch backward, "
             "the labels read as bytes); False: the classes' torch formulation (the CPU path; same results).  Off: "
             "tools/bench_label_loss.py measured the fused route 1.4 x faster for the softmax kind and 1.5-5 % slower for the hinge kind at "
             "(1024, 3862) and (80, 3862), and the default is on only if it is not slower for both kinds at both shapes "
             "(profiles/bench_label_loss.json, DESIGN.md section 23)")
FLAGS.define("regularization_penalty", 1.0, ":83")
FLAGS.define("base_learning_rate", 0.01, ":86")
FLAGS.define("learning_rate_decay", 0.95, ":88")
FLAGS.define("learning_rate_decay_examples", 4000000, ":91")
FLAGS.define("clip_gradient_norm", 1.0, ":108")
FLAGS.define("optimizer", "AdamOptimizer", "train.py:106: the class of tf.train that applies the gradients (optimizers.SUPPORTED: AdamOptimizer, "
             "GradientDescentOptimizer, MomentumOptimizer, AdagradOptimizer, RMSPropOptimizer, AdadeltaOptimizer), built from the learning rate "
             "alone as train.py:252 does.  Any rule but Adam updates every variable, hidden1_weights included, through "
             "lpm_multi_tensor_clip_update: the factored, early, sharded routes of that variable are Adam's")
FLAGS.define("optimizer_momentum", None, "build extension: MomentumOptimizer's momentum.  tf.train.MomentumOptimizer has no default for it -- the "
             "reference's optimizer_class(learning_rate) raises -- so --optimizer MomentumOptimizer is refused without this flag")
FLAGS.define("hidden1_factored_update", True, "build extension: the GPU trainer consumes hidden1_weights' gradient as the product "
             "descriptors^T . d(activation) it is (lpm_factored_clip_adam): the gradient is never written, the towers all-gather its "
             "two skinny factors instead of all-reducing it.  False: the generic path (gradient written into the arena)")
FLAGS.define("hidden1_compute_copy", True, "build extension, netvlad_storage='bf16' with the factored update: hidden1_weights keeps a bf16 "
             "compute copy beside its fp32 master (SURVEY section 7); the Adam epilogue writes it, the projection's forward and input-gradient "
             "passes read it (2 bytes per weight instead of 4, one bf16 MFMA per product).  False: both stream the fp32 weight (A/B).")
FLAGS.define("hidden1_early_update", True, "build extension, one tower with the factored update: clip + Adam of hidden1_weights run inside backward, "
             "right behind the projection's input gradient (the clip is per variable, utils.py:181-188: it needs only this variable's "
             "gradient factors), where the main queue would otherwise idle while the host enqueues the audio encoder's backward")
FLAGS.define("hidden1_update_stream", "auto", "build extension, with hidden1_early_update: the update pass of hidden1_weights (HBM-bound: 24-26 bytes "
             "per weight) runs on a HIP stream of its own behind the projection's input gradient, UNDER the rest of backward; the step joins it "
             "before it returns.  Measured, alternating on one box: cfg-5 (the gated model: the rest of backward is K3's latency-bound "
             "kernels) 5.495 -> 5.351 ms; cfg-2 (the rest is the encoders' power-limited GEMMs, which the extra HBM traffic slows) 6.64 -> "
             "6.70 ms.  'auto': on for netvlad_storage='bf16' (the configuration whose update pass is half the step), off otherwise; "
             "True / False force it")
FLAGS.define("hidden1_fold_input_gradient", False, "build extension, one tower with hidden1_early_update and the bf16 compute copy: the projection's "
             "INPUT gradient dx = dy W^T is formed inside hidden1_weights' update pass, from the weights that pass streams anyway "
             "(lpm_factored_clip_adam_copy_dx: VERDICT r3-r5), instead of by lpm_proj_dx_w16 from 2 more bytes per weight; the update then runs "
             "on the main stream (the rest of backward waits for dx) whatever hidden1_update_stream says.  Built and measured in round 6, NOT the "
             "default: the pass saves 60-165 us of the two kernels' 2.8 ms box to box and gives up the update stream's overlap with the rest of "
             "backward (~0.14 ms) -- cfg-5 5.431 -> 5.339 ms on one box, 5.275 -> 5.33 ms on another (profiles/r06_update_pass_fold.md).  "
             "LPM_FOLD_DX=0/1 overrides")
FLAGS.define("fold_l2_into_update", True, "build extension, one tower on the GPU: the analytic gradient of the MoE weights' L2 penalties "
             "(coefficient * w) is added inside the clip + Adam passes (lpm_multi_tensor_clip_adam_l2) instead of by an add pass over the "
             "gradient arena in front of them.  False: the add pass (A/B; towers > 1 always add before the all-reduce)")
FLAGS.define("direct_weight_gradients", True, "build extension: single-GPU training writes the encoders' dense-kernel gradients straight "
             "into the gradient arena from their producers (ops._dw_x3) instead of through autograd's .grad + a gather copy")
FLAGS.define("hidden1_factored_max_towers", 4, "build extension: ... up to this many towers.  Both passes of the factored update multiply "
             "over ALL towers' clips (R = 80 N at cfg-2: 0.72 ms at N = 1, 0.94 / 1.2 / 1.73 ms at N = 2 / 4 / 8 measured with "
             "tools/time_factored.py) where the generic route costs 0.88 ms of kernels plus a 554 MB all-reduce under the backward")
FLAGS.define("hidden1_sharded_update", True, "build extension (data parallel, route C of DESIGN.md section 6): beyond hidden1_factored_max_towers "
             "towers hidden1_weights' gradient is reduce-scattered instead of all-reduced, every rank clips (one-float all-reduce of "
             "the shard norms) and Adam-updates its 1/N shard, and the updated shards are all-gathered under the next forward (waited "
             "for where the projection reads the variable).  False: route A (bucket all-reduce + full update on every rank)")
FLAGS.define("hidden1_sharded_min_towers", 0, "build extension: 0 = the sharded route starts right above hidden1_factored_max_towers; "
             "N > 0 = from N towers on, taking precedence over the factored route (tests, A/B on a real node)")
FLAGS.define("library_gemm_selection", True, "build extension: the fp32 library GEMMs the host code leaves to PyTorch (MoE head, context gating, the "
             "small-batch projections) run on the hipBLASLt / rocBLAS solutions recorded per shape in _tunable/gfx950_fp32_gemm.csv (PyTorch's "
             "TunableOp with tuning OFF: a recorded shape takes its recorded solution, any other shape the library's default).  The MoE-4 head of "
             "BASELINE configs[4] is 159 + 87 us forward on the default choices and 47 + 39 us on the recorded ones; the file is ignored (with a "
             "warning from PyTorch) where its ROCm / hipBLASLt / rocBLAS / device validators do not match")
FLAGS.define("train_quantised_frames", True, "build extension: Trainer.build / step / calibrate_operand_scales hand the reader's uint8 frames on "
             "the GPU straight to the frame-prep kernels of NetVladV1 / NetVladV2 (lpm_frame_inv_norm_q8, lpm_frame_stats_q8, the *_q8 apply "
             "forms, lpm_frame_bn_bwd*_q8) instead of first writing the dequantised, L2-normalised fp32 frames of all max_frames "
             "(ops.dequantize_l2_normalize) -- the same results bit for bit.  False: the fp32 detour (A/B).  fp32 input, the CPU and other "
             "models are not affected")
FLAGS.define("csv_rows_fused", True, "build extension: inference.write_csv formats the rows of the CSV with ops.format_pairs (csrc/csv_rows.hip: "
             "every \"%i %g\" pair of a batch as text on the device, exact for every float) and joins ids and rows in native host code "
             "(lpm_csv_join_rows), batch n's copy and join under batch n + 1's forward; False: the rows go through format_top_k_lines, "
             "Python's own formatting (the same bytes).  On: tools/bench_inference.py measured write_csv against write_top_k end to end on an "
             "MI355X at 31.5 k against 24.7 k rows/s for NetVladV1 at the cfg-2 sizes (B = 80) and 1.73 M against 0.235 M rows/s for MoeModel on "
             "[1024, 1152] features, and the default is on only if it is not slower at both shapes (profiles/bench_inference.json, DESIGN.md "
             "section 24)")
FLAGS.define("eval_stats_fused", True, "build extension: evaluation.DeviceEvaluationMetrics.accumulate is two launches, lpm_eval_rows and "
             "lpm_eval_batch_stats (csrc/eval_batch_stats.hip: the batch's Hit@1 / PERR / loss means into one fp64 [4] slot, the loss sum and the "
             "per-class label counts, the labels read once as 16-byte loads); False: the means and the label counts are about ten small torch "
             "launches behind lpm_eval_rows (the same values; the fp64 sums in torch's order).  On: tools/bench_eval_stats.py measured accumulate on an MI355X at 50.7 against 122.5 us per batch at (80, 3862), 50.1 "
             "against 115.9 us at (128, 3862) and 60.4 against 129.5 us at (1024, 3862), and the default is on only if the fused route is not "
             "slower at all three shapes (profiles/bench_eval_stats.json, DESIGN.md section 25)")
FLAGS.define("gather_frames_fused", False, "build extension: the reader's uint8 frames on the GPU go unnormalised to the five triangulation "
             "models as well (RegularizedTriangulationModel, SoftAttentionTriangulationModel, TriangulationCnnClusterModel, JuhanTestModelV5, "
             "JuhanTestModelV1), which draw SampleRandomFrames' index table and gather, dequantise, L2-normalise and batch-normalise the "
             "sampled frames only (ops.frame_gather_bn_split: the *_idx frame-prep kernels).  False: these models take the normalise-everything "
             "route (ops.dequantize_l2_normalize over all max_frames, then the fp32 path).  fp32 input and the CPU are not affected.  Off by "
             "default until tools/bench_frame_gather.py has shown the new route not slower at every model shape on an MI355X: it has not run "
             "yet (profiles/bench_frame_gather.json)")
