"""GPU: lpm_format_pairs (csrc/csv_rows.hip) against the host entry of the same header, byte for byte, with guard regions around both
outputs; inference.write_csv with FLAGS.csv_rows_fused against write_top_k; inference.main on the device, flag on against flag off."""
import io
import os

import numpy as np
import pytest
import torch

from learnablepoolingmethods_amd import FLAGS, inference, ops, registry, training
from learnablepoolingmethods_amd.predictor import Predictor

from tests._util import cuda
from tests import test_format_pairs_host as HF
from tests import test_inference_cli_host as HC

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
GUARD = 0xAA


@pytest.fixture(scope="module")
def pool():
    """The oracle list of the host test (every branch: fixed, exponential, carry, tie, special, negative) in a fixed shuffled order, and
    the indices that go with it."""
    bits = HF.oracle_scores()
    rng = np.random.default_rng(9)
    return bits[rng.permutation(bits.size)], np.array(HF.INDEXES + [7, 3861, 100000, -99], dtype=np.int32)


@pytest.mark.parametrize("B,k,offset", [(1, 1, 0), (3, 20, 0), (5, 64, 0), (130, 7, 0), (3, 20, 4), (130, 7, 3)])
def test_device_rows_equal_host_rows(pool, B, k, offset):
    """offset: the text slice starts that many bytes off a 16-byte boundary (0: the 16-byte store path; other: the byte-store path)."""
    dev = cuda()
    bits, idx = pool
    # a window of the shuffled pool that moves with the shape
    start = (B * 131 + k * 17) % (bits.size - B * k)
    scores = torch.from_numpy(bits[start:start + B * k].view(np.float32).reshape(B, k).copy())
    if B * k >= 8:                                            # whatever the window holds: the specials and the named cases are in
        scores.view(-1)[:8] = torch.tensor([float("nan"), float("inf"), float("-inf"), -0.0, 0.0, 999999.5, 100000.5, 9.9999997e-05])
    classes = torch.from_numpy(np.resize(idx, B * k).reshape(B, k).copy())
    want_text, want_len = ops.format_pairs(classes, scores)
    stride = ops.format_pairs_stride(k)
    pad = 64
    big_text = torch.full((pad + offset + B * stride + pad,), GUARD, dtype=torch.uint8, device=dev)
    big_len = torch.full((16 + B + 16,), 0x2AAAAAAA, dtype=torch.int32, device=dev)
    text = big_text[pad + offset:pad + offset + B * stride].view(B, stride)
    length = big_len[16:16 + B]
    assert (text.data_ptr() % 16 == 0) == (offset == 0)
    c, s = classes.to(dev), scores.to(dev)
    ops.format_pairs_into(c, s, text, length)
    torch.cuda.synchronize()
    first_text, first_len = big_text.cpu().clone(), big_len.cpu().clone()
    got_len = first_len[16:16 + B]
    assert torch.equal(got_len, want_len)
    got = first_text[pad + offset:pad + offset + B * stride].view(B, stride)
    for r in range(B):
        n = int(want_len[r])
        assert torch.equal(got[r, :n], want_text[r, :n]), r
    assert bool((first_text[:pad + offset] == GUARD).all()) and bool((first_text[pad + offset + B * stride:] == GUARD).all())
    assert bool((first_len[:16] == 0x2AAAAAAA).all()) and bool((first_len[16 + B:] == 0x2AAAAAAA).all())
    ops.format_pairs_into(c, s, text, length)                 # the same input gives the same bytes
    torch.cuda.synchronize()
    assert torch.equal(big_text.cpu(), first_text) and torch.equal(big_len.cpu(), first_len)
    # the wrapper's own packed buffer: text first, length behind it
    t2, l2 = ops.format_pairs(c, s)
    assert t2.is_cuda and t2.shape == (B, stride) and torch.equal(l2.cpu(), want_len)
    assert bytes(ops.csv_join_rows(["v"] * B, t2.cpu(), l2.cpu())) == bytes(ops.csv_join_rows(["v"] * B, want_text, want_len))


def test_device_refuses_bad_shapes():
    dev = cuda()
    from learnablepoolingmethods_amd._capi import LpmError
    with pytest.raises(LpmError):
        ops.format_pairs(torch.zeros(2, 65, dtype=torch.int32, device=dev), torch.zeros(2, 65, device=dev))
    with pytest.raises(LpmError):
        ops.format_pairs(torch.zeros(0, 4, dtype=torch.int32, device=dev), torch.zeros(0, 4, device=dev))
    with pytest.raises(LpmError):
        ops.format_pairs(torch.zeros(2, 4, dtype=torch.int32, device=dev), torch.zeros(2, 4))


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """A video-level MoeModel trained for two steps on the CPU (HC's files and flags): train_dir, file pattern, files."""
    tmp = tmp_path_factory.mktemp("csv")
    files = HC._video_files(tmp)
    train_dir, pattern = str(tmp / "model"), str(tmp / "video*.tfrecord")
    try:
        training.main(["--train_data_pattern", pattern, "--train_dir", train_dir] + HC.VIDEO_ARGS)
    finally:
        FLAGS.reset()
    return tmp, train_dir, pattern, files


def test_write_csv_equals_write_top_k(trained):
    dev = cuda()
    _, train_dir, _, _ = trained
    g = torch.Generator().manual_seed(2)
    batches = [([f"b{i}-{j}" if j else "" for j in range(n)], torch.randn(n, 36, generator=g).to(dev), None,
                torch.ones(n, dtype=torch.int32, device=dev)) for i, n in enumerate((4, 4, 3))]
    batches[1][0][2] = "café-\U0001d11e"
    try:
        FLAGS.moe_num_mixtures = 3
        pr = Predictor.from_checkpoint(training.latest_checkpoint(train_dir), registry.get_model("MoeModel"), vocab_size=HC.V, device=dev)
        ref = io.StringIO()
        assert inference.write_top_k(ref, pr, iter(batches), top_k=5) == 11
        want = ref.getvalue().encode("utf-8")
        for fused in (True, False):
            FLAGS.csv_rows_fused = fused
            out = io.BytesIO()
            assert inference.write_csv(out, pr, iter(batches), top_k=5) == 11
            assert out.getvalue() == want, fused
    finally:
        FLAGS.reset()


def test_inference_main_on_the_device(trained):
    cuda()
    tmp, train_dir, pattern, _ = trained
    data = {}
    for fused in (True, False):
        csv = str(tmp / f"gpu_{fused}.csv")
        try:
            FLAGS.csv_rows_fused = fused
            got = inference.main(["--train_dir", train_dir, "--input_data_pattern", pattern, "--output_file", csv, "--device", "cuda",
                                  "--batch_size", "3", "--top_k", "5"])
        finally:
            FLAGS.reset()
        assert got["num_examples"] == 7
        data[fused] = open(csv, "rb").read()
    assert data[True] == data[False]                          # the device formatter against Python's, same checkpoint, same files
    lines = data[True].decode("utf-8").splitlines()
    assert lines[0] == "VideoId,LabelConfidencePairs"
    assert [ln.split(",")[0] for ln in lines[1:]] == [f"f{f}v{i}" for f, n in enumerate((4, 3)) for i in range(n)]
    assert all(len(ln.split(",")[1].split(" ")) == 10 for ln in lines[1:])
    assert os.path.getsize(str(tmp / "gpu_True.csv")) == len(data[True])
