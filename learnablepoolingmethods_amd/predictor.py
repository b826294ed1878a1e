"""Frozen forward-only predictor (reference: eval.py:143-150, inference.py:135 and export_model.py:40-107, which all build the model
with ``is_training=False``; the exported model returns ``video_id``, ``class_indexes`` and ``predictions``, the top 20 classes per
video).

A ``Predictor`` holds a snapshot of a model's weights and batch-norm moving statistics in a variable store of its own -- no Adam
slots, no gradient arena, nothing a running ``Trainer`` writes -- and runs the eval-mode forward of the registry model on it.  The
reader's quantised uint8 frames go straight into the frame-prep kernels for NetVladV1 / NetVladV2 (ops.frame_sample_bn: the
dequantisation and per-frame L2 normalisation happen for the sampled frames only) and for the five triangulation models
(ops.frame_gather_bn_split, FLAGS.gather_frames_fused); other models, and fp32 frames, are normalised
first exactly as ``Trainer.predict`` does it.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import FLAGS, ops
from . import variables as vs
from ._capi import LpmError
from .optimizers import SLOT_KEYS
from .train import check_input_rank, normalize_input

# models whose frame-prep op reads uint8 frames in eval mode (ops.frame_sample_bn / frame_sample_bn_split)
FUSED_Q8_MODELS = ("NetVladV1", "NetVladV2")
# models that gather SampleRandomFrames' frames from the uint8 batch themselves (ops.frame_gather_bn_split), FLAGS.gather_frames_fused
GATHER_Q8_MODELS = ("RegularizedTriangulationModel", "SoftAttentionTriangulationModel", "TriangulationCnnClusterModel", "JuhanTestModelV5",
                    "JuhanTestModelV1")
# likewise, added after the five above (whose tuple the frame-gather tests pin by value)
GATHER_Q8_LATER_MODELS = ("JuhanTestModelV2", "JuhanTestModelV3", "JuhanTestModelV4", "JuhanTestModelV6")


def takes_quantised_frames(model, frames) -> bool:
    """Whether a uint8 batch goes to this model unnormalised: on the GPU, and either a NetVLAD model (uniform sampling) or -- with
    FLAGS.gather_frames_fused, at a feature size the q8 kernels accept -- one of the triangulation models (random sampling)."""
    name = type(model).__name__
    if not (frames.dtype == torch.uint8 and frames.is_cuda and frames.dim() == 3):
        return False
    if name in FUSED_Q8_MODELS:
        return True
    return bool(name in GATHER_Q8_MODELS + GATHER_Q8_LATER_MODELS and FLAGS.gather_frames_fused and frames.shape[2] % 4 == 0 and frames.shape[2] <= 2048)
# checkpoint entries that are not variables (train.Trainer.state_dict)
_NOT_VARIABLES = ("global_step", "bn_statistics_synced", "hidden1_adam_shard")
_H1 = "tower/hidden1_weights"


def _is_statistic(name: str) -> bool:
    return name.endswith("/moving_mean") or name.endswith("/moving_variance")


class Predictor:
    """Eval-mode forward of a frozen snapshot.  Build it with ``from_trainer`` or ``from_checkpoint``."""

    def __init__(self, model, vocab_size: int, variables: Dict[str, torch.Tensor], device, model_kwargs=None,
                 compute_copy: Optional[torch.Tensor] = None):
        """variables: name -> tensor (the ``tower/...`` names of Trainer.store), copied onto ``device``.  compute_copy: the bf16 copy
        of hidden1_weights the eval forward reads (netvlad_storage='bf16'); built from the weight at its first use when it is None."""
        self.model = model
        self.vocab_size = int(vocab_size)
        self.device = torch.device(device)
        self.model_kwargs = dict(model_kwargs or {})
        self.store = vs.VariableStore(device=self.device)
        self.store.analytic_l2 = self.device.type == "cuda"       # (as the trainer's store: the forward records no penalty tensors)
        with torch.no_grad():
            for n, v in variables.items():
                t = torch.as_tensor(v).detach().to(device=self.device, dtype=torch.float32, copy=True).contiguous()
                trainable = not _is_statistic(n)
                t.requires_grad_(trainable)
                self.store.vars[n] = t
                self.store.trainable[n] = trainable
        self.store.frozen = True              # a variable the forward asks for and the snapshot lacks raises instead of being initialised
        self.w16 = None
        if self._wants_compute_copy():
            W = self.store.vars[_H1]
            self.w16 = ops.ComputeCopy(W)
            if compute_copy is not None:
                self.w16.buf.copy_(compute_copy)
                self.w16.version, self.w16.stale = self.w16._versions(W), False
            W._lpm_w16 = self.w16

    def _wants_compute_copy(self) -> bool:
        # the condition under which train.Trainer.build attaches hidden1_weights' bf16 compute copy on one GPU
        W = self.store.vars.get(_H1)
        return bool(self.device.type == "cuda" and W is not None and FLAGS.hidden1_factored_update and FLAGS.netvlad_storage == "bf16"
                    and FLAGS.hidden1_compute_copy and W.dim() == 2 and W.shape[1] % 32 == 0)

    # -- construction -----------------------------------------------------------------------------------------------------------
    @classmethod
    def from_trainer(cls, trainer) -> "Predictor":
        """Snapshot of a built trainer's variables and moving statistics, on its device (after hidden1_weights' update of the last
        step, which may run on a stream of its own, has finished: as Trainer.predict)."""
        if trainer.arena is None:
            raise RuntimeError("Predictor.from_trainer needs a built trainer: run build() or one step first")
        trainer.wait_pending()
        cc = None
        with torch.no_grad():
            variables = {n: v.detach() for n, v in trainer.store.vars.items()}
            if trainer.w16 is not None:
                cc = trainer._w16_current()       # the copy the trainer's own eval forward would read (None: stale, rebuilt from the master)
            return cls(trainer.model, trainer.vocab_size, variables, trainer.device, trainer.model_kwargs, compute_copy=cc)

    @classmethod
    def from_checkpoint(cls, path: str, model, vocab_size: int = 3862, model_kwargs=None, device="cuda") -> "Predictor":
        """From a file written by Trainer.save: its variables and moving statistics (the optimiser's slots -- Adam's, or those of the
        ``--optimizer`` the file names -- and the step count are dropped)."""
        state = torch.load(path, map_location="cpu")
        slots = tuple("/" + k for k in SLOT_KEYS.get(state.get("optimizer", "AdamOptimizer"), SLOT_KEYS["AdamOptimizer"]))
        variables = {n: v for n, v in state.items() if n not in _NOT_VARIABLES and torch.is_tensor(v) and not (slots and n.endswith(slots))}
        if not variables:
            raise ValueError(f"{path}: no variables in this checkpoint")
        return cls(model, vocab_size, variables, device, model_kwargs)

    # -- inference ---------------------------------------------------------------------------------------------------------------
    def _check_inputs(self, frames, num_frames):
        ok = torch.is_tensor(frames) and ((frames.dim() == 3 and frames.dtype in (torch.uint8, torch.float32))
                                          or (frames.dim() == 2 and frames.dtype == torch.float32))
        if not ok:
            raise LpmError("Predictor: the input must be frames, a uint8 (quantised) or float32 [batch, max_frames, feature] tensor, or "
                           "video-level features, a float32 [batch, feature] tensor")
        check_input_rank(self.model, frames)
        if not torch.is_tensor(num_frames) or num_frames.dim() != 1 or num_frames.shape[0] != frames.shape[0]:
            raise LpmError("Predictor: num_frames must be a [batch] tensor")
        if num_frames.dtype.is_floating_point or num_frames.dtype == torch.bool:
            raise LpmError("Predictor: num_frames must hold integers")

    def _check_k(self, k):
        k = int(k)
        if not (1 <= k <= ops.TOPK_MAX_K and k <= self.vocab_size):
            raise LpmError(f"Predictor.top_k: need 1 <= k <= min({ops.TOPK_MAX_K}, vocab_size={self.vocab_size}), got {k}")
        return k

    # (torch.no_grad, as Trainer.predict, rather than inference_mode: the frame-prep tile cache and the compute copy identify their
    # tensors by version counter, which inference tensors do not carry)
    @torch.no_grad()
    def predict(self, frames, num_frames) -> torch.Tensor:
        """-> predictions [B, vocab_size]: the eval-mode forward (is_training=False, moving statistics, no operand scales).  ``frames``:
        [B, max_frames, F] frames, or the video-level reader's float32 [B, F] features in front of a model of video_level_models."""
        self._check_inputs(frames, num_frames)
        frames = frames.to(self.device)
        nf = num_frames.to(self.device)
        if not takes_quantised_frames(self.model, frames):
            frames = normalize_input(frames, nf)
        with vs.use_store(self.store):
            with vs.variable_scope("tower"):
                result = self.model.create_model(frames, num_frames=nf, vocab_size=self.vocab_size, labels=None,
                                                 fused_cross_entropy=False, **{**self.model_kwargs, "is_training": False})
            self.store.pop_regularization_losses()
            self.store.pop_l2_regularizers()
        return result["predictions"]

    @torch.no_grad()
    def top_k(self, frames, num_frames, k: int = 20):
        """-> (class_indexes int32 [B, k], predictions fp32 [B, k]): export_model.py's outputs, the k best classes per video in
        descending score order (ties: ascending class index), from lpm_topk_rows."""
        self._check_inputs(frames, num_frames)
        k = self._check_k(k)
        return ops.topk_rows(self.predict(frames, num_frames), k)
