"""Inference output (reference: inference.py:88-96,182): the ``VideoId,LabelConfidencePairs`` CSV of each video's top-k
classes, and a driver that runs a trained model over reader batches.  SURVEY 8f rank 5.

``python -m learnablepoolingmethods_amd.inference --train_dir D --input_data_pattern 'files*' --output_file out.csv`` is the reference's
command line (inference.py:49-85, :207-250): ``main`` reads ``D/model_flags.json`` (training.main writes it), builds the reader and a
``predictor.Predictor`` from the newest checkpoint and runs ``write_csv`` over the files.  ``write_csv`` writes the file's bytes: with
FLAGS.csv_rows_fused the rows of a batch are formatted on the device (ops.format_pairs) and joined with their ids in native host code
(ops.csv_join_rows) while the next batch's forward runs; ``write_top_k`` / ``write_predictions`` and the two ``format_*`` functions are
the Python route and the drop-in surface."""
from __future__ import annotations

import argparse
import logging
import os
import time
from typing import Dict, Iterable, Iterator, Sequence

import torch

from . import FLAGS
from .model_flags import MODEL_FLAGS_FILE  # noqa: F401  (this module keeps exporting the name)

CSV_HEADER = "VideoId,LabelConfidencePairs\n"


def format_lines(video_ids: Sequence, predictions, top_k: int) -> Iterator[str]:
    """inference.py:88-96: one line per video, ``<id>,<class> <score> <class> <score> ...`` with the top_k classes in
    descending score order, scores printed with ``%g``.  (Equal scores keep ascending class order here; the reference's
    order among ties follows numpy.argpartition.)"""
    p = torch.as_tensor(predictions)
    k = min(int(top_k), p.shape[1])
    scores, classes = torch.sort(p, dim=1, descending=True, stable=True)
    scores, classes = scores[:, :k].cpu().tolist(), classes[:, :k].cpu().tolist()
    for vid, cs, ss in zip(video_ids, classes, scores):
        if isinstance(vid, bytes):
            vid = vid.decode("utf-8")
        yield vid + "," + " ".join("%i %g" % (c, s) for c, s in zip(cs, ss)) + "\n"


def write_predictions(out_file, trainer, batches: Iterable, top_k: int = 20) -> int:
    """Header + format_lines for every (ids, frames, labels, num_frames) batch of ``readers.YT8MFrameFeatureReader.batches``;
    ``trainer.predict`` is the eval-mode forward (moving batch-norm statistics).  Returns the number of videos written."""
    out_file.write(CSV_HEADER)
    n = 0
    for ids, frames, _, num_frames in batches:
        pred = trainer.predict(frames, num_frames)
        for line in format_lines(ids, pred, top_k):
            out_file.write(line)
        n += len(ids)
    return n


def format_top_k_lines(video_ids: Sequence, class_indexes, scores) -> Iterator[str]:
    """The lines of format_lines from an already selected top k (export_model.py's ``class_indexes`` / ``predictions``)."""
    classes, scores = torch.as_tensor(class_indexes).cpu().tolist(), torch.as_tensor(scores).cpu().tolist()
    for vid, cs, ss in zip(video_ids, classes, scores):
        if isinstance(vid, bytes):
            vid = vid.decode("utf-8")
        yield vid + "," + " ".join("%i %g" % (c, s) for c, s in zip(cs, ss)) + "\n"


def write_top_k(out_file, predictor, batches: Iterable, top_k: int = 20) -> int:
    """write_predictions' CSV, byte for byte, from a predictor.Predictor: the top k of every video selected on the GPU
    (Predictor.top_k, lpm_topk_rows) instead of a sort of all classes.  Returns the number of videos written."""
    k = min(int(top_k), predictor.vocab_size)
    out_file.write(CSV_HEADER)
    n = 0
    for ids, frames, _, num_frames in batches:
        classes, scores = predictor.top_k(frames, num_frames, k)
        for line in format_top_k_lines(ids, classes, scores):
            out_file.write(line)
        n += len(ids)
    return n


def _select_top_k(predictor, frames, num_frames, k):
    """(class_indexes int32 [B, k], predictions fp32 [B, k]) on the predictor's device: Predictor.top_k on the GPU, the stable sort of
    format_lines on the CPU (lpm_topk_rows is a device kernel)."""
    if predictor.device.type == "cuda":
        return predictor.top_k(frames, num_frames, k)
    scores, classes = torch.sort(predictor.predict(frames, num_frames), dim=1, descending=True, stable=True)
    return classes[:, :k].to(torch.int32).contiguous(), scores[:, :k].contiguous()


class _PinnedRows:
    """One of write_csv's two pinned host slots: format_pairs' packed buffer of a batch (text, then length) and the event behind its copy."""

    def __init__(self):
        self.host = None
        self.event = torch.cuda.Event()

    def reserve(self, nbytes):
        if self.host is None or self.host.numel() < nbytes:
            self.host = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, pin_memory=True)
        return self.host[:nbytes]


def write_csv(out_file, predictor, batches: Iterable, top_k: int = 20) -> int:
    """write_top_k's CSV, byte for byte (UTF-8), into a BINARY file object.  Returns the number of videos written.

    With FLAGS.csv_rows_fused every batch is Predictor.top_k, ops.format_pairs (the rows as text, on the device), ONE asynchronous copy
    of text and length into one of two pinned slots, ops.csv_join_rows (ids and rows, native host code) and one ``write``.  Batch n's copy
    is waited for -- its event, no device-wide synchronise -- and joined after batch n + 1's launches are enqueued, so it runs under that
    forward.  A CPU predictor formats through the host entry of the same code.  Without the flag the rows are format_top_k_lines'."""
    from . import ops
    k = min(int(top_k), predictor.vocab_size)
    out_file.write(CSV_HEADER.encode("utf-8"))
    n = 0
    if not FLAGS.csv_rows_fused:
        for ids, frames, _, num_frames in batches:
            classes, scores = _select_top_k(predictor, frames, num_frames, k)
            out_file.write("".join(format_top_k_lines(ids, classes, scores)).encode("utf-8"))
            n += len(ids)
        return n
    stride = ops.format_pairs_stride(k)
    slots, pending = None, None

    def drain(item):
        slot, ids, host = item
        B = len(ids)
        slot.event.synchronize()
        out_file.write(ops.csv_join_rows(ids, host[:B * stride].view(B, stride), host[B * stride:].view(torch.int32)))

    for i, (ids, frames, _, num_frames) in enumerate(batches):
        classes, scores = _select_top_k(predictor, frames, num_frames, k)
        if classes.is_cuda:
            packed = torch.empty(len(ids) * (stride + 4), dtype=torch.uint8, device=classes.device)
            ops.format_pairs(classes, scores, out=packed)
            if slots is None:
                slots = (_PinnedRows(), _PinnedRows())
            slot = slots[i & 1]                          # batch i - 2's: joined and written during batch i - 1
            host = slot.reserve(packed.numel())
            host.copy_(packed, non_blocking=True)
            slot.event.record()
            if pending is not None:
                drain(pending)
            pending = (slot, ids, host)
        else:
            text, length = ops.format_pairs(classes, scores)
            out_file.write(ops.csv_join_rows(ids, text, length))
        n += len(ids)
    if pending is not None:
        drain(pending)
    return n


# ---- command line (python -m learnablepoolingmethods_amd.inference) --------------------------------------------------------------
def _parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m learnablepoolingmethods_amd.inference",
                                 description="Write the VideoId,LabelConfidencePairs CSV of a trained model over YT8M TFRecord files (the "
                                             "reference's inference.py flags).")
    ap.add_argument("--train_dir", default="/tmp/yt8m_model/", help="the directory of model_flags.json and the checkpoints (inference.py:51)")
    ap.add_argument("--input_data_pattern", default="", help="comma-separated globs of TFRecord files (inference.py:54)")
    ap.add_argument("--output_file", default="", help="the CSV to write (inference.py:71)")
    ap.add_argument("--top_k", type=int, default=20, help="inference.py:82")
    ap.add_argument("--batch_size", type=int, default=1024, help="inference.py:77")
    ap.add_argument("--num_readers", type=int, default=1, help="inference.py:79: device_batches' reader_threads (GPU route)")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--checkpoint", default="", help="a model.ckpt-<step>.pt file (default: the newest one of --train_dir)")
    return ap


def main(argv=None) -> Dict[str, object]:
    """inference.py's ``main``: model_flags.json + a checkpoint + files -> the CSV.  -> {num_examples, seconds, examples_per_second,
    output_file}.  Every video appears once, in file order, the last smaller batch included."""
    from . import model_flags, registry, training
    from .predictor import Predictor
    args = _parser().parse_args(argv)
    flags_dict = model_flags.read(args.train_dir, "Cannot find %s. Did you run eval.py?")              # inference.py:221-223
    if not args.output_file:
        raise ValueError("'output_file' was not specified. Unable to continue with inference.")
    if not args.input_data_pattern:
        raise ValueError("'input_data_pattern' was not specified. Unable to continue with inference.")
    files = model_flags.matching_files(args.input_data_pattern)
    if not files:
        raise IOError("Unable to find input files. data_pattern='" + args.input_data_pattern + "'")       # inference.py:117-120
    logging.info("number of input files: " + str(len(files)))
    checkpoint = args.checkpoint or training.latest_checkpoint(args.train_dir)
    if not checkpoint or not os.path.exists(checkpoint):
        raise IOError("Cannot find a checkpoint (model.ckpt-<step>.pt) in %s" % args.train_dir)
    num_classes = int(flags_dict["num_classes"])
    with model_flags.applied(flags_dict):
        reader = model_flags.build_reader(flags_dict)
        device = torch.device(args.device)
        predictor = Predictor.from_checkpoint(checkpoint, registry.get_model(flags_dict["model"]), vocab_size=num_classes, device=device)
        if device.type == "cuda":
            batches = reader.device_batches(files, args.batch_size, device=device, reader_threads=args.num_readers)
        else:
            batches = reader.batches(files, args.batch_size)
        start = time.time()

        def logged():
            done = 0
            for batch in batches:
                yield batch
                done += len(batch[0])
                logging.info("num examples processed: " + str(done) + " elapsed seconds: " + "{0:.2f}".format(time.time() - start))
        try:
            with open(args.output_file, "wb") as out_file:
                num_examples = write_csv(out_file, predictor, logged(), args.top_k)
        finally:
            batches.close()
        seconds = time.time() - start
    return {"num_examples": num_examples, "seconds": seconds,
            "examples_per_second": num_examples / seconds if seconds > 0 else float("inf"), "output_file": args.output_file}


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    main()
