"""-m "not gpu": readers.YT8MAggregatedFeatureReader, the video-level files (tf.train.Example records of float lists), against the
protobuf runtime both ways; batches(); labels and ids; the refusals."""
import numpy as np
import pytest
import torch

from learnablepoolingmethods_amd import readers

from _example_proto import example_class

SIZES, NAMES, V = (24, 12), ("mean_rgb", "mean_audio"), 30


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _vectors(rng, sizes=SIZES):
    return [rng.standard_normal(s).astype(np.float32) for s in sizes]


def _record(vid, labels, vecs, **kw):
    return readers.make_example(vid, labels, dict(zip(NAMES, vecs)), **kw)


def test_protobuf_runtime_records_parse_like_ours():
    """Theirs parsed by us: map entries in another order, an unselected feature of every kind, a repeated label, labels at and above
    num_classes, an id whose length needs a two-byte varint."""
    Example = example_class()
    rng = np.random.default_rng(21)
    reader = readers.YT8MAggregatedFeatureReader(num_classes=V, feature_sizes=SIZES, feature_names=NAMES)
    for vid, labels in (("a" * 3, [3, 17, 29]), ("long-id-" * 20, [V, V + 5, 2, 2, 3861]), ("", [])):
        rgb, audio = _vectors(rng)
        m = Example()
        m.features.feature["mean_audio"].float_list.value.extend(audio.tolist())
        m.features.feature["extra_floats"].float_list.value.extend([1.5, 2.5, 3.5])
        m.features.feature["labels"].int64_list.value.extend(labels)
        m.features.feature["extra_bytes"].bytes_list.value.append(b"xyz")
        m.features.feature["mean_rgb"].float_list.value.extend(rgb.tolist())
        m.features.feature["id"].bytes_list.value.append(vid.encode())
        m.features.feature["extra_ints"].int64_list.value.extend([-1, 7])
        rec = m.SerializeToString()
        got = reader.prepare_serialized_examples(rec)
        assert got[0] == vid and got[3] == 1
        assert got[1].dtype == np.float32 and np.array_equal(_bits(got[1]), _bits(np.concatenate([rgb, audio])))
        assert got[2].dtype == bool and np.flatnonzero(got[2]).tolist() == sorted({v for v in labels if v < V})
        parsed = readers.parse_example(rec)
        assert parsed["extra_bytes"] == ("bytes", [b"xyz"]) and parsed["extra_ints"] == ("int64", [-1, 7])
        assert parsed["extra_floats"][0] == "float" and parsed["extra_floats"][1].tolist() == [1.5, 2.5, 3.5]
        # the hand-written encoder's record of the same video reads the same
        ours = reader.prepare_serialized_examples(_record(vid, labels, [rgb, audio]))
        assert ours[0] == vid and np.array_equal(_bits(ours[1]), _bits(got[1])) and np.array_equal(ours[2], got[2])


@pytest.mark.parametrize("packed", [True, False])
def test_our_records_parse_in_the_protobuf_runtime(packed):
    """Ours parsed by them, in both encodings, with bit patterns a double round trip would change."""
    Example = example_class()
    rng = np.random.default_rng(22)
    rgb, audio = _vectors(rng)
    rgb[:6] = np.array([0x7FA00001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x00000001, 0x80000000], np.uint32).view(np.float32)
    rec = _record("vid-7", [5, 1, 5], [rgb, audio], packed=packed)
    m = Example()
    m.ParseFromString(rec)
    assert sorted(m.features.feature) == ["id", "labels", "mean_audio", "mean_rgb"]
    assert list(m.features.feature["id"].bytes_list.value) == [b"vid-7"]
    assert list(m.features.feature["labels"].int64_list.value) == [5, 1, 5]
    theirs = np.array(m.features.feature["mean_rgb"].float_list.value, np.float32)
    assert np.array_equal(_bits(theirs)[6:], _bits(rgb)[6:]) and np.isnan(theirs[:2]).all()       # (their floats went through doubles)
    assert np.array_equal(_bits(np.array(m.features.feature["mean_audio"].float_list.value, np.float32)), _bits(audio))
    # our parser keeps every bit, the signalling NaN included
    reader = readers.YT8MAggregatedFeatureReader(num_classes=V, feature_sizes=SIZES, feature_names=NAMES)
    assert np.array_equal(_bits(reader.prepare_serialized_examples(rec)[1]), _bits(np.concatenate([rgb, audio])))


def test_batches_shapes_dtypes_and_ones(tmp_path):
    rng = np.random.default_rng(23)
    reader = readers.YT8MAggregatedFeatureReader(num_classes=V, feature_sizes=SIZES, feature_names=NAMES)
    vecs = [_vectors(rng) for _ in range(7)]
    paths = [str(tmp_path / "a.tfrecord"), str(tmp_path / "b.tfrecord")]
    readers.write_tfrecord(paths[0], [_record(f"a{i}", [i, i + 1], vecs[i]) for i in range(3)])
    readers.write_tfrecord(paths[1], [_record(f"b{i}", [i], vecs[i], packed=False) for i in range(3, 7)])
    got = list(reader.batches(paths, 3, verify_crc=True))
    assert [len(b[0]) for b in got] == [3, 3, 1]
    assert [i for b in got for i in b[0]] == ["a0", "a1", "a2", "b3", "b4", "b5", "b6"]
    for ids, x, y, nf in got:
        n = len(ids)
        assert x.dtype == torch.float32 and tuple(x.shape) == (n, sum(SIZES))
        assert y.dtype == torch.bool and tuple(y.shape) == (n, V)
        assert nf.dtype == torch.int32 and nf.tolist() == [1] * n
    want = np.stack([np.concatenate(v) for v in vecs])
    assert np.array_equal(_bits(torch.cat([b[1] for b in got]).numpy()), _bits(want))
    assert np.flatnonzero(got[1][2][1].numpy()).tolist() == [4]
    assert [len(b[0]) for b in reader.batches(paths, 3, drop_remainder=True)] == [3, 3]
    # one feature alone, in the other order
    r1 = readers.YT8MAggregatedFeatureReader(num_classes=V, feature_sizes=(12,), feature_names=("mean_audio",))
    assert np.array_equal(_bits(next(r1.batches(paths, 7))[1].numpy()), _bits(want[:, 24:]))
    r2 = readers.YT8MAggregatedFeatureReader(num_classes=V, feature_sizes=SIZES[::-1], feature_names=NAMES[::-1])
    assert np.array_equal(_bits(next(r2.batches(paths, 7))[1].numpy()), _bits(np.concatenate([want[:, 24:], want[:, :24]], axis=1)))


def test_labels_and_ids():
    rng = np.random.default_rng(24)
    reader = readers.YT8MAggregatedFeatureReader(num_classes=V, feature_sizes=SIZES, feature_names=NAMES)
    vecs = _vectors(rng)
    assert np.flatnonzero(reader.prepare_serialized_examples(_record("d", [7, 7, 2, 7], vecs))[2]).tolist() == [2, 7]        # duplicates
    assert not reader.prepare_serialized_examples(_record("e", [], vecs))[2].any()                                          # an empty list
    assert np.flatnonzero(reader.prepare_serialized_examples(_record("o", [V, 0, -1, 1 << 40, V - 1], vecs))[2]).tolist() == [0, V - 1]
    E = readers._enc_ld
    body = b"".join(E(1, E(1, n.encode()) + E(2, E(2, E(1, v.tobytes())))) for n, v in zip(NAMES, vecs))
    vid, x, y, one = reader.prepare_serialized_examples(E(1, body))                                                        # no id, no labels
    assert vid == "" and not y.any() and one == 1 and np.array_equal(_bits(x), _bits(np.concatenate(vecs)))


def test_refusals_name_the_record(tmp_path):
    rng = np.random.default_rng(25)
    reader = readers.YT8MAggregatedFeatureReader(num_classes=V, feature_sizes=SIZES, feature_names=NAMES)
    vecs = [_vectors(rng) for _ in range(3)]
    good = [_record(f"g{i}", [i], vecs[i]) for i in range(3)]
    E = readers._enc_ld
    path = str(tmp_path / "bad.tfrecord")

    def refused(records, error, *words):
        readers.write_tfrecord(path, records)
        it = reader.batches([path], 1, verify_crc=True)
        assert next(it)[0] == ["g0"]                              # the batch before the bad record arrives
        with pytest.raises(error) as e:
            list(it)
        for w in ("record 1",) + words:
            assert w in str(e.value), str(e.value)

    missing = readers.make_example("m1", [1], {"mean_rgb": vecs[1][0]})
    refused([good[0], missing, good[2]], ValueError, "m1", "mean_audio", "missing")
    short = readers.make_example("s1", [1], {"mean_rgb": vecs[1][0][:23], "mean_audio": vecs[1][1]})
    refused([good[0], short, good[2]], ValueError, "s1", "mean_rgb", "23")
    as_bytes = E(1, E(1, E(1, b"id") + E(2, readers._enc_bytes_feature([b"b1"])))
                 + E(1, E(1, b"mean_rgb") + E(2, readers._enc_bytes_feature([vecs[1][0].tobytes()])))
                 + E(1, E(1, b"mean_audio") + E(2, E(2, E(1, vecs[1][1].tobytes())))))
    refused([good[0], as_bytes, good[2]], ValueError, "b1", "mean_rgb", "bytes")
    # corruption: a flipped payload byte of record 1 (with verify_crc; without, the byte is data), and a file that ends inside record 1
    readers.write_tfrecord(path, good)
    data = bytearray(open(path, "rb").read())
    pos = 16 + len(good[0]) + 12 + len(good[1]) - 20
    data[pos] ^= 0x40
    open(path, "wb").write(bytes(data))
    it = reader.batches([path], 1, verify_crc=True)
    assert next(it)[0] == ["g0"]
    with pytest.raises(IOError, match="record 1"):
        next(it)
    assert [b[0][0] for b in reader.batches([path], 1)] == ["g0", "g1", "g2"]
    data[pos] ^= 0x40
    for cut in (16 + len(good[0]) + 5, 16 + len(good[0]) + 12 + 30, 16 + len(good[0]) + 12 + len(good[1]) + 2):
        open(path, "wb").write(bytes(data[:cut]))
        it = reader.batches([path], 1)
        assert next(it)[0] == ["g0"]
        with pytest.raises(IOError, match="record 1"):
            next(it)
