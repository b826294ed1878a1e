"""What the command lines behind training share: ``train_dir/model_flags.json`` (training.write_model_flags records it; the reference:
train.py:390-411, read back by eval.py:295-316 and inference.py:220-238) names the model, its features and the non-default flags of the run.
``evaluation.main`` and ``inference.main`` read the file, run with the recorded flags applied and build the recorded mode's reader through
the three helpers here; the messages of a missing file differ between the two commands, so the caller passes its own."""
from __future__ import annotations

import contextlib
import glob
import json
import os
from typing import Dict, Iterator, List

from . import FLAGS

MODEL_FLAGS_FILE = "model_flags.json"


def read(train_dir: str, missing: str) -> Dict[str, object]:
    """The decoded ``train_dir/model_flags.json``; IOError(missing % path) when it is not there."""
    path = os.path.join(train_dir, MODEL_FLAGS_FILE)
    if not os.path.exists(path):
        raise IOError(missing % path)
    with open(path) as f:
        return json.load(f)


def matching_files(data_pattern: str) -> List[str]:
    """The files of comma-separated globs, each glob's matches sorted (train.py:163-170)."""
    files: List[str] = []
    for pattern in data_pattern.split(","):
        files.extend(sorted(glob.glob(pattern)) if pattern else [])
    return files


@contextlib.contextmanager
def applied(flags_dict: Dict[str, object]) -> Iterator[None]:
    """FLAGS with the recorded run's non-default flags (``flags_dict["flags"]``) set; every flag is put back on exit."""
    saved = {name: getattr(FLAGS, name) for name in FLAGS._defaults}
    try:
        for name, value in flags_dict.get("flags", {}).items():
            setattr(FLAGS, name, value)
        yield
    finally:
        for name, value in saved.items():
            setattr(FLAGS, name, value)


def build_reader(flags_dict: Dict[str, object]):
    """The reader of the recorded mode: frame-level files (SequenceExample) or video-level files (Example)."""
    from . import readers
    names = [s.strip() for s in flags_dict["feature_names"].split(",") if s.strip()]
    sizes = [int(s) for s in flags_dict["feature_sizes"].split(",") if s.strip()]
    num_classes = int(flags_dict["num_classes"])
    if flags_dict["frame_features"]:
        return readers.YT8MFrameFeatureReader(num_classes=num_classes, feature_sizes=sizes, feature_names=names,
                                              max_frames=int(flags_dict["max_frames"]))
    return readers.YT8MAggregatedFeatureReader(num_classes=num_classes, feature_sizes=sizes, feature_names=names)
