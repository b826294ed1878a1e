"""The training run loop (reference: train.py:446-497, the loop of ``Trainer.run``; :546-575, ``get_meta_filename`` / resume; :160-184,
the input pipeline; :44-112, the flags) around ``train.Trainer.step``:

    files -> readers.YT8MFrameFeatureReader.training_batches (shuffled device batches) -> Trainer.step -> log line / checkpoint / summaries

(``--frame_features false``: readers.YT8MAggregatedFeatureReader, the video-level files, in front of a model of video_level_models.)

``run`` steps until ``max_steps <= global_step`` or the batches end.  On steps with ``global_step % log_every == 0`` it computes
Hit@1, PERR and GAP of the step's predictions against its labels (``evaluation.batch_metrics``: lpm_eval_rows + the pooled top-20
average precision on the device, eval_util on the CPU), copies them and the loss to the host ONCE and logs the reference's line byte
for byte.  With ``train_dir`` it saves ``model.ckpt-<step>.pt`` (``Trainer.save`` under a temporary name, then ``os.replace``) at the first logged step, at every logged step at
which ``export_model_steps`` steps have passed since the last save (the reference takes this decision at its logged steps too), and on
exit; on entry the newest ``model.ckpt-*.pt`` there is restored -- after ``Trainer.build`` on the first batch -- unless
``start_new_model``, which removes the old ``model.ckpt-*.pt`` files instead (the reference deletes the whole directory).  The input
stream restarts on resume, as the reference's does.

With a ``summary_writer`` (summaries.SummaryWriter) every logged step also writes, at ``global_step``, the reference's scalars --
``model/Training_Hit@1``, ``model/Training_Perr``, ``model/Training_GAP``, ``global_step/Examples/Second`` (train.py:470-480), ``label_loss``
and ``learning_rate`` (train.py:250, 326) -- from the numbers the log line was formatted from: no further device read.  At the first logged
step, and at every logged step at which ``histogram_steps`` steps have passed since the last histogram write (the checkpoint cadence's rule),
it writes a histogram of every variable (``SummaryWriter.add_variables``: one HIP pass over the parameter arena) and of the raw input
(``model/input_raw``); their results come to the host in one asynchronous copy.  ``summary_activations=True`` adds the activation
histograms the models record with ``vs.summary`` (``store.summaries``): only the forward of a histogram step collects them, and because
collecting makes the models take their materialising paths that step's arithmetic path changes -- the default set does not change one bit
of the training result.

Deviations from the reference, on purpose:
  * the steps between two logged ones log nothing and read nothing back from the device.  The reference prints "training step N | Loss
    ... Examples/sec ..." for every step, which takes the loss to the host -- a synchronisation per step that the GPU trainer's
    asynchronous step does not otherwise have;
  * Examples/sec is therefore measured over the interval since the previous logged step (the reference: one ``sess.run``);
  * the log line is emitted with or without ``train_dir`` (the reference's chief logs metrics only when it has one);
  * checkpoints are ``torch.save`` files of ``Trainer.state_dict``; there is no SavedModel export;
  * summaries: ``reg_loss`` is not written -- on the GPU the L2 penalties enter as gradients and their value is never formed; the
    histograms cover ALL variables, not only ``slim.get_model_variables()``; they follow a step cadence, not the Supervisor's 120 s.
Multi-tower loops are out of scope: a trainer with ``num_towers > 1`` is refused.
"""
from __future__ import annotations

import argparse
import glob
import json
import logging
import os
import re
import time
from typing import Callable, Dict, Iterable, List, Optional

import torch

from . import FLAGS, evaluation
from .model_flags import MODEL_FLAGS_FILE

_CKPT = re.compile(r"^model\.ckpt-(\d+)\.pt$")


def checkpoint_path(train_dir: str, step: int) -> str:
    return os.path.join(train_dir, f"model.ckpt-{int(step)}.pt")


def checkpoints(train_dir: str) -> List[str]:
    """The ``model.ckpt-<step>.pt`` files of train_dir, oldest step first."""
    if not train_dir or not os.path.isdir(train_dir):
        return []
    found = sorted((int(m.group(1)), n) for n in os.listdir(train_dir) for m in [_CKPT.match(n)] if m)
    return [os.path.join(train_dir, n) for _, n in found]


def latest_checkpoint(train_dir: str) -> Optional[str]:
    """tf.train.latest_checkpoint for this module's files: the one with the highest step, or None."""
    found = checkpoints(train_dir)
    return found[-1] if found else None


def format_log_line(global_step, loss, examples_per_second, hit_at_one, perr, gap) -> str:
    """train.py:468-472, byte for byte."""
    return ("training step " + str(global_step) + " | Loss: " + ("%.2f" % loss) + " Examples/sec: " + ("%.2f" % examples_per_second)
            + " | Hit@1: " + ("%.2f" % hit_at_one) + " PERR: " + ("%.2f" % perr) + " GAP: " + ("%.2f" % gap))


def run(trainer, batches: Iterable, max_steps: Optional[int] = None, log_every: int = 10, train_dir: Optional[str] = None,
        export_model_steps: int = 1000, start_new_model: bool = False, log: Callable[[str], None] = logging.info,
        on_step: Optional[Callable] = None, summary_writer=None, histogram_steps: int = 1000,
        summary_activations: bool = False) -> Dict[str, object]:
    """Train ``trainer`` over ``batches`` of (ids, frames, labels, num_frames) -- see the module docstring.  ``on_step(step_result,
    batch)`` is called after every step with ``Trainer.step``'s dict and the batch.  -> {global_step, steps, num_examples, seconds,
    examples_per_second, last_loss, checkpoints}: the steps and examples of THIS call, the paths it wrote, the last step's loss (None
    when no step ran).  ``summary_writer`` / ``histogram_steps`` / ``summary_activations``: the module docstring; the writer is flushed on
    exit and stays open (its owner closes it)."""
    if trainer.num_towers > 1:
        raise ValueError(f"training.run drives one tower; this trainer has num_towers = {trainer.num_towers} "
                         "(multi-tower run loops are out of scope)")
    if int(log_every) < 1 or int(export_model_steps) < 1 or int(histogram_steps) < 1:
        raise ValueError("training.run: log_every, export_model_steps and histogram_steps must be at least 1")
    written: List[str] = []
    last_export = 0                       # train.py's last_model_export_step
    last_histograms = 0                   # the same rule for the histogram writes

    def save(step):
        nonlocal last_export
        path = checkpoint_path(train_dir, step)
        # written under a name _CKPT does not match, then renamed: a polling evaluation.run never opens half a file.  model.ckpt-<step>.tmp,
        # not ...pt.tmp: torch.save names the records inside the file after the file's name up to its last dot, so this keeps the bytes
        tmp = path[:-len(".pt")] + ".tmp"
        trainer.save(tmp)
        os.replace(tmp, path)
        written.append(path)
        last_export = step

    resume = None
    if train_dir:
        os.makedirs(train_dir, exist_ok=True)
        if start_new_model:
            for path in checkpoints(train_dir):
                os.remove(path)
        else:
            resume = latest_checkpoint(train_dir)
    steps = examples = 0
    interval_examples = 0
    last = None
    t0 = interval_start = time.perf_counter()
    first = True
    for batch in batches:
        _, frames, labels, num_frames = batch
        if first:
            first = False
            if resume is not None:
                trainer.build(frames.to(trainer.device), num_frames.to(trainer.device), labels.to(trainer.device))
                trainer.restore(resume)
                log(f"restored {resume}: global_step {trainer.global_step}")
        if max_steps is not None and max_steps <= trainer.global_step:
            break
        # a histogram step is known before it runs: the logged step after which histogram_steps steps have passed
        upcoming = trainer.global_step + 1
        histograms = (summary_writer is not None and upcoming % log_every == 0
                      and (last_histograms == 0 or upcoming - last_histograms >= histogram_steps))
        collect = histograms and summary_activations and getattr(trainer, "store", None) is not None
        if collect:
            trainer.store.summaries = {}
        try:
            last = trainer.step(frames, num_frames, labels)
        finally:
            activations = trainer.store.summaries if collect else None
            if collect:
                trainer.store.summaries = None
        step = trainer.global_step
        n = int(labels.shape[0])
        steps, examples, interval_examples = steps + 1, examples + n, interval_examples + n
        if step % log_every == 0:
            p = last["predictions"]
            m = evaluation.batch_metrics(p, labels.to(p.device))
            loss, hit, perr, gap = torch.cat([last["loss"].detach().to(torch.float64).reshape(1), m.to(p.device)]).tolist()   # the one host copy
            now = time.perf_counter()
            rate = interval_examples / max(now - interval_start, 1e-12)
            log(format_log_line(step, loss, rate, hit, perr, gap))
            interval_start, interval_examples = now, 0
            if summary_writer is not None:
                scalars = {"model/Training_Hit@1": hit, "model/Training_Perr": perr, "model/Training_GAP": gap,
                           "global_step/Examples/Second": rate, "label_loss": loss}                    # train.py:470-480, :326
                if "learning_rate" in last:
                    scalars["learning_rate"] = float(last["learning_rate"])                             # train.py:250
                summary_writer.add_scalars(scalars, step)
                if histograms and step == upcoming:
                    summary_writer.add_variables(trainer, step)
                    summary_writer.add_input(frames, num_frames, step)
                    for name, t in (activations or {}).items():
                        summary_writer.add_histogram(name, t, step)
                    summary_writer.commit()          # one asynchronous copy; encoded when it has arrived
                    last_histograms = step
            if train_dir and (last_export == 0 or step - last_export >= export_model_steps):
                save(step)
        if on_step is not None:
            on_step(last, batch)
        if max_steps is not None and max_steps <= step:
            break
    if train_dir and trainer.arena is not None and steps and last_export != trainer.global_step:
        save(trainer.global_step)
    last_loss = float(last["loss"]) if last is not None else None        # (waits for the last step)
    if summary_writer is not None:
        summary_writer.flush()
    seconds = time.perf_counter() - t0
    return {"global_step": trainer.global_step, "steps": steps, "num_examples": examples, "seconds": seconds,
            "examples_per_second": examples / seconds if seconds > 0 else float("inf"), "last_loss": last_loss, "checkpoints": written}


# ---- command line (python -m learnablepoolingmethods_amd.training) ---------------------------------------------------------------
def _flag_value(default):
    if isinstance(default, bool):
        return lambda s: str(s).lower() in ("1", "true", "yes", "y")
    if default is None:                   # (a flag without a default, optimizer_momentum: a number when given)
        return float
    return type(default)


def _parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m learnablepoolingmethods_amd.training",
                                 description="Train a frame-level or video-level model from YT8M TFRecord files (the reference's train.py "
                                             "flags).")
    ap.add_argument("--train_data_pattern", default="", help="comma-separated globs of TFRecord files (train.py:51)")
    ap.add_argument("--train_dir", default="/tmp/yt8m_model/", help="checkpoint directory (train.py:48)")
    ap.add_argument("--model", default="NetVladV1", help="a class of frame_level_models (train.py:64)")
    ap.add_argument("--num_epochs", type=int, default=5, help="train.py:93")
    ap.add_argument("--max_steps", type=int, default=None, help="train.py:95")
    ap.add_argument("--export_model_steps", type=int, default=1000, help="train.py:97")
    ap.add_argument("--summary_dir", default="", help="write TensorBoard event files here (empty: none; may equal --train_dir)")
    ap.add_argument("--histogram_steps", type=int, default=1000, help="steps between histogram summaries (with --summary_dir)")
    ap.add_argument("--start_new_model", type=_flag_value(False), nargs="?", const=True, default=False, help="train.py:68")
    ap.add_argument("--frame_features", type=_flag_value(True), nargs="?", const=True, default=True,
                    help="true: frame-level files (SequenceExample, uint8 frames); false: video-level files (Example, float features) for a "
                         "model of video_level_models.  The reference's default is false (train.py:59-62); this command line keeps true")
    ap.add_argument("--feature_names", default=None, help="train.py:55 (default: rgb,audio; with --frame_features false: mean_rgb,mean_audio)")
    ap.add_argument("--feature_sizes", default=None, help="train.py:57 (default: 1024,128)")
    ap.add_argument("--num_classes", type=int, default=3862)
    ap.add_argument("--max_frames", type=int, default=300, help="frames kept per clip (readers.py:134); ignored with --frame_features false")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--seed", type=int, default=0, help="variable initialisation and input order")
    ap.add_argument("--log_every", type=int, default=10)
    ap.add_argument("--reader_threads", type=int, default=1, help="device_batches' reader threads (GPU route)")
    # every registered flag (flags.py: the reference's names and defaults, and the build extensions): --batch_size, --base_learning_rate,
    # --iterations, --netvlad_cluster_size, ...
    for name, default in FLAGS._defaults.items():
        ap.add_argument("--" + name, type=_flag_value(default), default=None, help=f"FLAGS.{name} (default {default!r})")
    return ap


def write_model_flags(train_dir: str, model_flags: Dict[str, object], start_new_model: bool = False) -> str:
    """train.py:390-411: record which model ``train_dir`` holds, for inference.main.  The reference's five keys (model, feature_names,
    feature_sizes, frame_features, label_loss) must equal those of a file that is already there (ValueError naming both; the reference
    logs them and exits); ``start_new_model`` removes the old file first.  -> the file's path."""
    os.makedirs(train_dir, exist_ok=True)
    path = os.path.join(train_dir, MODEL_FLAGS_FILE)
    if start_new_model and os.path.exists(path):
        os.remove(path)
    if os.path.exists(path):
        with open(path) as f:
            existing = json.load(f)
        five = ("model", "feature_names", "feature_sizes", "frame_features", "label_loss")
        ran, previously = {k: model_flags.get(k) for k in five}, {k: existing.get(k) for k in five}
        if ran != previously:
            raise ValueError(f"Model flags do not match existing file {path}. Please delete the file, change --train_dir, or pass flag "
                             f"--start_new_model. Ran model with flags: {ran}. Previously ran with flags: {previously}")
        return path
    with open(path, "w") as f:
        f.write(json.dumps(model_flags))
    return path


def main(argv=None) -> Dict[str, object]:
    """train.py's ``main``: flags -> reader + Trainer + ``run``.  -> run's dict.  With a ``train_dir`` it also records the model in
    ``train_dir/model_flags.json`` (write_model_flags) once the Trainer stands."""
    from . import readers, registry, summaries
    from .train import Trainer
    args = _parser().parse_args(argv)
    for name in FLAGS._defaults:
        if getattr(args, name) is not None:
            setattr(FLAGS, name, getattr(args, name))
    files: List[str] = []
    for pattern in args.train_data_pattern.split(","):                         # train.py:163-170
        files.extend(sorted(glob.glob(pattern)) if pattern else [])
    if not files:
        raise IOError("Unable to find training files. data_pattern='" + args.train_data_pattern + "'.")
    logging.info("Number of training files: %s.", str(len(files)))
    feature_names = args.feature_names or ("rgb,audio" if args.frame_features else "mean_rgb,mean_audio")
    names = [s.strip() for s in feature_names.split(",") if s.strip()]
    sizes = [int(s) for s in (args.feature_sizes or "1024,128").split(",") if s.strip()]
    if args.frame_features:                                                    # train.py:596-606
        reader = readers.YT8MFrameFeatureReader(num_classes=args.num_classes, feature_sizes=sizes, feature_names=names, max_frames=args.max_frames)
    else:
        reader = readers.YT8MAggregatedFeatureReader(num_classes=args.num_classes, feature_sizes=sizes, feature_names=names)
    device = torch.device(args.device)
    # --optimizer / --optimizer_momentum (train.py:106,577) are registered flags: set above, handed on by name here
    trainer = Trainer(registry.get_model(args.model), vocab_size=args.num_classes, batch_size=FLAGS.batch_size, device=device, seed=args.seed,
                      optimizer=FLAGS.optimizer, optimizer_momentum=FLAGS.optimizer_momentum)
    if args.train_dir:
        write_model_flags(args.train_dir, {
            "model": args.model, "feature_names": ",".join(names), "feature_sizes": ",".join(str(v) for v in sizes),
            "frame_features": bool(args.frame_features), "label_loss": FLAGS.label_loss,                  # the reference's five
            "num_classes": int(args.num_classes), "max_frames": int(args.max_frames),
            "flags": {name: getattr(FLAGS, name) for name, default in FLAGS._defaults.items() if getattr(FLAGS, name) != default},
        }, start_new_model=args.start_new_model)
    kw = dict(reader_threads=args.reader_threads) if device.type == "cuda" else {}
    batches = reader.training_batches(files, FLAGS.batch_size, device=device, num_epochs=args.num_epochs, seed=args.seed, **kw)
    writer = summaries.SummaryWriter(args.summary_dir) if args.summary_dir else None
    try:
        return run(trainer, batches, max_steps=args.max_steps, log_every=args.log_every, train_dir=args.train_dir,
                   export_model_steps=args.export_model_steps, start_new_model=args.start_new_model, summary_writer=writer,
                   histogram_steps=args.histogram_steps)
    finally:
        batches.close()
        if writer is not None:
            writer.close()


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    main()
