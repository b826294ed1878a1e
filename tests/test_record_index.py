"""-m "not gpu": the native record indexer (lpm_tfrecord_frame / lpm_yt8m_locate, host code of liblpm_hip.so) against the Python parser of
readers.py, which is the yardstick: TFRecord framing, the offsets of every frame payload, labels and ids, the refusals, and a seeded
robustness run over mutated header bytes -- in the library (every buffer ends at a PROT_NONE page) and in a sanitizer build of
csrc/record_index.h (a standalone executable; CPU code only)."""
import ctypes
import mmap
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from learnablepoolingmethods_amd import readers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "learnablepoolingmethods_amd", "csrc")


def _tf_example_classes():
    """tf.train.{Feature, Features, FeatureList, FeatureLists, SequenceExample} built with the protobuf runtime from their
    public definitions (feature.proto / example.proto): an independent encoder (the helper of tests/test_readers.py)."""
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
    fd = descriptor_pb2.FileDescriptorProto(name="lpm_test_example_index.proto", package="lpmtfi", syntax="proto3")
    T = descriptor_pb2.FieldDescriptorProto

    def msg(name):
        m = fd.message_type.add()
        m.name = name
        return m

    def field(m, name, num, typ, label=T.LABEL_OPTIONAL, type_name=None, packed=None, oneof=None):
        f = m.field.add(name=name, number=num, type=typ, label=label)
        if type_name:
            f.type_name = type_name
        if packed is not None:
            f.options.packed = packed
        if oneof is not None:
            f.oneof_index = oneof
    field(msg("BytesList"), "value", 1, T.TYPE_BYTES, T.LABEL_REPEATED)
    field(msg("FloatList"), "value", 1, T.TYPE_FLOAT, T.LABEL_REPEATED, packed=True)
    field(msg("Int64List"), "value", 1, T.TYPE_INT64, T.LABEL_REPEATED, packed=True)
    feat = msg("Feature")
    feat.oneof_decl.add(name="kind")
    field(feat, "bytes_list", 1, T.TYPE_MESSAGE, type_name=".lpmtfi.BytesList", oneof=0)
    field(feat, "float_list", 2, T.TYPE_MESSAGE, type_name=".lpmtfi.FloatList", oneof=0)
    field(feat, "int64_list", 3, T.TYPE_MESSAGE, type_name=".lpmtfi.Int64List", oneof=0)

    def map_msg(parent, entry_name, value_type):
        e = parent.nested_type.add(name=entry_name)
        e.options.map_entry = True
        field(e, "key", 1, T.TYPE_STRING)
        field(e, "value", 2, T.TYPE_MESSAGE, type_name=value_type)
    feats = msg("Features")
    map_msg(feats, "FeatureEntry", ".lpmtfi.Feature")
    field(feats, "feature", 1, T.TYPE_MESSAGE, T.LABEL_REPEATED, type_name=".lpmtfi.Features.FeatureEntry")
    field(msg("FeatureList"), "feature", 1, T.TYPE_MESSAGE, T.LABEL_REPEATED, type_name=".lpmtfi.Feature")
    fls = msg("FeatureLists")
    map_msg(fls, "FeatureListEntry", ".lpmtfi.FeatureList")
    field(fls, "feature_list", 1, T.TYPE_MESSAGE, T.LABEL_REPEATED, type_name=".lpmtfi.FeatureLists.FeatureListEntry")
    se = msg("SequenceExample")
    field(se, "context", 1, T.TYPE_MESSAGE, type_name=".lpmtfi.Features")
    field(se, "feature_lists", 2, T.TYPE_MESSAGE, type_name=".lpmtfi.FeatureLists")
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    return message_factory.GetMessageClass(pool.FindMessageTypeByName("lpmtfi.SequenceExample"))


def _frames(rng, n, sizes=(1024, 128)):
    return [rng.integers(0, 256, size=(n, s), dtype=np.uint8) for s in sizes]


def _framed(records):
    """The bytes write_tfrecord writes."""
    out = bytearray()
    for data in records:
        head = struct.pack("<Q", len(data))
        out += head + struct.pack("<I", readers.masked_crc32c(head)) + data + struct.pack("<I", readers.masked_crc32c(data))
    return bytes(out)


class _Guarded:
    """A buffer that ends exactly at a PROT_NONE page: a read past its end faults instead of passing unnoticed."""

    def __init__(self, data: bytes):
        page = mmap.PAGESIZE
        n = len(data)
        self.map = mmap.mmap(-1, (n // page + 2) * page)
        whole = np.frombuffer(self.map, dtype=np.uint8)
        base = whole.ctypes.data
        libc = ctypes.CDLL(None, use_errno=True)
        libc.mprotect.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        end = (n // page + 1) * page
        if libc.mprotect(ctypes.c_void_p(base + end), page, 0) != 0:          # PROT_NONE
            raise OSError(ctypes.get_errno(), "mprotect")
        self.array = whole[end - n:end]
        self.array[:] = np.frombuffer(data, dtype=np.uint8)

    def close(self):
        arr, self.array = self.array, None
        del arr


def _agree(reader, record: bytes, buf: np.ndarray, idx: readers.RecordIndex, i: int):
    """Clip i of the native index against prepare_serialized_examples on its record, field by field."""
    vid, q, y, n = reader.prepare_serialized_examples(record)
    assert int(idx.num_frames[i]) == n
    col = 0
    for f, size in enumerate(reader.feature_sizes):
        for t in range(n):
            off = int(idx.frame_offset[i, f, t])
            assert off >= 0 and np.array_equal(buf[off:off + size], q[t, col:col + size]), (i, f, t)
        assert (idx.frame_offset[i, f, n:] == -1).all()
        col += size
    lab = idx.label_index[idx.label_start[i]:idx.label_start[i + 1]]
    assert set(lab.tolist()) == set(np.flatnonzero(y).tolist())
    o, ln = int(idx.id_offset[i]), int(idx.id_length[i])
    assert bytes(buf[o:o + ln]).decode("utf-8") == vid


def _index(reader, data: bytes, verify_crc=True):
    g = _Guarded(data)
    offs, lens, consumed = readers.frame_records(g.array, verify_crc=verify_crc)
    idx = readers.locate_records(g.array, offs, lens, reader.feature_names, reader.feature_sizes, reader.max_frames, reader.num_classes)
    return g.array, offs, lens, consumed, idx


def test_crc32c_matches_the_python_table():
    """Both native CRC routes (the CPU's instruction in three streams, slice-by-8) through framing with verify_crc, over payload lengths
    around the stream and word boundaries."""
    rng = np.random.default_rng(3)
    recs = [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in (0, 1, 7, 8, 9, 63, 1023, 3071, 3072, 3073, 6144 + 5, 10000)]
    data = _framed(recs)
    offs, lens, consumed = readers.frame_records(np.frombuffer(data, np.uint8), verify_crc=True)
    assert consumed == len(data) and lens.tolist() == [len(r) for r in recs]
    assert [data[o:o + n] for o, n in zip(offs.tolist(), lens.tolist())] == recs


def test_index_agrees_with_python_parser_on_written_files(tmp_path):
    rng = np.random.default_rng(11)
    reader = readers.YT8MFrameFeatureReader(num_classes=50, max_frames=9)
    spec = [(5, [1]), (12, [0, 2, 49]), (9, []), (0, [7, 7]), (1, [50, 51, 3, 100000])]
    recs = []
    for i, (n, lab) in enumerate(spec):
        rgb, audio = _frames(rng, n)
        recs.append(readers.make_sequence_example(f"v{i}", lab, {"rgb": rgb, "audio": audio}))
    path = str(tmp_path / "a.tfrecord")
    readers.write_tfrecord(path, recs)
    data = open(path, "rb").read()
    buf, offs, lens, consumed, idx = _index(reader, data)
    assert consumed == len(data) and len(offs) == len(recs)
    assert [bytes(buf[o:o + n]) for o, n in zip(offs.tolist(), lens.tolist())] == list(readers.read_tfrecord(path, verify_crc=True))
    assert idx.num_frames.tolist() == [5, 9, 9, 0, 1]
    for i, rec in enumerate(recs):
        _agree(reader, rec, buf, idx, i)
    # rgb alone
    r1 = readers.YT8MFrameFeatureReader(num_classes=50, feature_sizes=(1024,), feature_names=("rgb",), max_frames=9)
    buf, offs, lens, _, idx = _index(r1, data)
    assert idx.frame_offset.shape == (5, 1, 9)
    for i, rec in enumerate(recs):
        _agree(r1, rec, buf, idx, i)


def test_index_agrees_on_protobuf_runtime_records():
    """Records serialised by the protobuf runtime: map entries in another order, an extra context feature and feature list, a zero-frame
    clip, max_frames + 3 frames, labels at num_classes and above, a repeated label, an id whose length needs a two-byte varint."""
    SE = _tf_example_classes()
    rng = np.random.default_rng(12)
    max_frames, V = 6, 20
    reader = readers.YT8MFrameFeatureReader(num_classes=V, max_frames=max_frames)
    cases = [("a" * 3, [3, 17, 19], 4), ("long-id-" * 30, [V, V + 5, 2, 2, 3861], max_frames + 3), ("zero", [1], 0), ("", [], 2)]
    recs = []
    for vid, labels, n in cases:
        rgb, audio = _frames(rng, n)
        m = SE()
        # audio before rgb, labels before id; unknown features in both maps
        m.feature_lists.feature_list["audio"].SetInParent()
        for row in audio:
            m.feature_lists.feature_list["audio"].feature.add().bytes_list.value.append(row.tobytes())
        m.feature_lists.feature_list["extra_list"].feature.add().float_list.value.extend([1.5, 2.5])
        m.feature_lists.feature_list["rgb"].SetInParent()
        for row in rgb:
            m.feature_lists.feature_list["rgb"].feature.add().bytes_list.value.append(row.tobytes())
        m.context.feature["labels"].int64_list.value.extend(labels)
        m.context.feature["extra"].float_list.value.extend([0.25])
        m.context.feature["id"].bytes_list.value.append(vid.encode())
        recs.append(m.SerializeToString(deterministic=False))
        recs.append(readers.make_sequence_example(vid, labels, {"audio": audio, "rgb": rgb}))     # the same clip, hand-written encoder
    assert len(cases[1][0].encode()) >= 128
    data = _framed(recs)
    buf, offs, lens, consumed, idx = _index(reader, data)
    assert consumed == len(data)
    assert idx.num_frames.tolist() == [4, 4, 6, 6, 0, 0, 2, 2]
    for i, rec in enumerate(recs):
        _agree(reader, rec, buf, idx, i)
    # the repeated label is kept twice in the list (the dense matrix does not care), the out-of-range ones are gone
    assert sorted(idx.label_index[idx.label_start[2]:idx.label_start[3]].tolist()) == [2, 2]


def test_hand_built_wire_variants():
    """Unpacked int64 labels, unknown fields of every skippable wire type, a second context that replaces the first, and a length that
    runs past its message (clamped, as the Python walk's slices are)."""
    rng = np.random.default_rng(13)
    reader = readers.YT8MFrameFeatureReader(num_classes=30, feature_sizes=(8, 4), max_frames=5)
    E = readers._enc_ld
    V = readers._enc_varint

    def flist(name, mat):
        return E(1, E(1, name) + E(2, b"".join(E(1, readers._enc_bytes_feature([r.tobytes()])) for r in mat)))
    rgb, audio = _frames(rng, 3, (8, 4))
    unpacked = E(3, b"".join(V(1 << 3) + V(v) for v in (4, 29, 30, (1 << 64) - 1)))           # field 1, wire type 0, one per value
    ctx = E(1, E(1, b"labels") + E(2, unpacked)) + E(1, E(2, readers._enc_bytes_feature([b"vid"])) + E(1, b"id"))   # value before key
    junk = V((9 << 3) | 0) + V(300) + V((10 << 3) | 5) + b"abcd" + V((11 << 3) | 1) + b"12345678" + E(12, b"xyz")
    lists = flist(b"rgb", rgb) + flist(b"audio", audio)
    rec0 = junk + E(1, ctx) + junk + E(2, lists)
    rec1 = E(1, E(1, E(1, b"id") + E(2, readers._enc_bytes_feature([b"old"])))) + E(2, lists) + E(1, ctx)      # the second context counts
    over = bytearray(E(2, lists))
    assert over[-6] == 0x0A and over[-5] == 4                                               # the last audio frame: ... 0A 04 <4 bytes>
    over[-5] = 0x7F                                                                         # its length now runs past everything
    rec2 = E(1, ctx) + bytes(over)
    recs = [rec0, rec1, rec2]
    buf, offs, lens, _, idx = _index(reader, _framed(recs))
    for i, rec in enumerate(recs):
        _agree(reader, rec, buf, idx, i)
    assert idx.num_frames.tolist() == [3, 3, 3]
    assert sorted(idx.label_index[:idx.label_start[1]].tolist()) == [4, 29]


def test_framing_of_a_buffer_cut_inside_a_record():
    rng = np.random.default_rng(14)
    recs = [readers.make_sequence_example(f"c{i}", [i], dict(zip(("rgb", "audio"), _frames(rng, n)))) for i, n in enumerate([3, 5, 2, 4])]
    data = _framed(recs)
    whole = readers.frame_records(np.frombuffer(data, np.uint8), verify_crc=True)
    assert whole[2] == len(data) and len(whole[0]) == 4
    ends = (whole[0] + whole[1] + 4).tolist()
    for cut in (ends[1] + 1, ends[1] + 11, ends[1] + 12, ends[2] - 1, ends[0], 5, len(data) - 1):
        g = _Guarded(data[:cut])
        o1, l1, used = readers.frame_records(g.array, verify_crc=True)
        assert used == max([0] + [e for e in ends if e <= cut]) and len(o1) == sum(e <= cut for e in ends)
        rest = data[used:cut] + data[cut:]
        o2, l2, used2 = readers.frame_records(np.frombuffer(rest, np.uint8), verify_crc=True)
        assert used + used2 == len(data)
        assert np.array_equal(np.concatenate([o1, o2 + used]), whole[0]) and np.array_equal(np.concatenate([l1, l2]), whole[1])
    # max_records stops the walk as well
    o, ln, used = readers.frame_records(np.frombuffer(data, np.uint8), max_records=2)
    assert len(o) == 2 and used == ends[1]


def test_refusals_name_the_record(tmp_path):
    rng = np.random.default_rng(15)
    reader = readers.YT8MFrameFeatureReader(num_classes=10, max_frames=9)
    mats = [_frames(rng, 3) for _ in range(3)]
    recs = [readers.make_sequence_example(f"r{i}", [1], {"rgb": a, "audio": b}) for i, (a, b) in enumerate(mats)]
    data = _framed(recs)
    buf, offs, lens, _, idx = _index(reader, data)
    # a flipped byte inside a frame's payload of record 1: IOError with verify_crc, data without
    pos = int(idx.frame_offset[1, 0, 2]) + 100
    bad = bytearray(data)
    bad[pos] ^= 0xFF
    with pytest.raises(IOError, match="record 1"):
        readers.frame_records(np.frombuffer(bytes(bad), np.uint8), verify_crc=True)
    o, ln, _ = readers.frame_records(np.frombuffer(bytes(bad), np.uint8), verify_crc=False)
    idx2 = readers.locate_records(np.frombuffer(bytes(bad), np.uint8), o, ln, max_frames=9, num_classes=10)
    assert np.array_equal(idx2.frame_offset, idx.frame_offset)
    path = str(tmp_path / "bad.tfrecord")
    open(path, "wb").write(bytes(bad))
    assert list(readers.read_tfrecord(path))[1][pos - int(offs[1])] == bad[pos]                # the Python route: the byte is data
    # a flipped byte in the length CRC of record 2
    bad = bytearray(data)
    bad[int(offs[2]) - 12 + 9] ^= 0x01
    with pytest.raises(IOError, match="record 2"):
        readers.frame_records(np.frombuffer(bytes(bad), np.uint8), verify_crc=True)
    assert len(readers.frame_records(np.frombuffer(bytes(bad), np.uint8), verify_crc=False)[0]) == 3
    # a truncated buffer: the cut record is not reported; a truncated FILE is an error that names it
    o, ln, used = readers.frame_records(np.frombuffer(data[:-3], np.uint8), verify_crc=True)
    assert len(o) == 2 and used == int(offs[2]) - 12
    for end in (len(data) - 3, len(data) - 30, int(offs[2]) - 5):           # inside the payload CRC, the payload, the header
        open(path, "wb").write(data[:end])
        with pytest.raises(IOError, match="record 2"):
            readers.frame_file(path, verify_crc=True)
        with pytest.raises(IOError):
            list(readers.read_tfrecord(path))
    open(path, "wb").write(data)
    fbuf, fo, fl = readers.frame_file(path, verify_crc=True)
    assert np.array_equal(fo, offs) and np.array_equal(fl, lens) and bytes(fbuf) == data
    # a frame of 1023 bytes (record 1), and audio one frame short of rgb (record 2)
    a, b = mats[1]
    E = readers._enc_ld
    rows = [r.tobytes() for r in a]
    rows[1] = rows[1][:1023]
    fl = E(1, E(1, b"rgb") + E(2, b"".join(E(1, readers._enc_bytes_feature([r])) for r in rows)))
    fl += E(1, E(1, b"audio") + E(2, b"".join(E(1, readers._enc_bytes_feature([r.tobytes()])) for r in b)))
    short = E(1, E(1, E(1, b"id") + E(2, readers._enc_bytes_feature([b"r1"])))) + E(2, fl)
    with pytest.raises(Exception):
        reader.prepare_serialized_examples(short)
    d = _framed([recs[0], short, recs[2]])
    o, ln, _ = readers.frame_records(np.frombuffer(d, np.uint8))
    with pytest.raises(ValueError, match="record 1"):
        readers.locate_records(np.frombuffer(d, np.uint8), o, ln, max_frames=9, num_classes=10)
    a, b = mats[2]
    uneven = readers.make_sequence_example("r2", [1], {"rgb": a, "audio": b[:-1]})
    with pytest.raises(ValueError):
        reader.prepare_serialized_examples(uneven)
    d = _framed([recs[0], recs[1], uneven])
    o, ln, _ = readers.frame_records(np.frombuffer(d, np.uint8))
    with pytest.raises(ValueError, match="record 2"):
        readers.locate_records(np.frombuffer(d, np.uint8), o, ln, max_frames=9, num_classes=10)
    # ... but equal after capping at max_frames is fine, as in the Python path
    a, b = _frames(rng, 12)
    capped = readers.make_sequence_example("cap", [], {"rgb": a, "audio": b[:10]})
    buf, _, _, _, idx = _index(reader, _framed([capped]))
    _agree(reader, capped, buf, idx, 0)


# ---- robustness: mutated header bytes -------------------------------------------------------------------------------------------------
MAX_FRAMES_FUZZ = 12
FUZZ_CLASSES = 3862


def _mutated_records():
    """300 records of 0-15 frames, ids of 'vid<k>' repeated 1-39 times, 0-5 labels; one to four random byte changes each among the bytes
    that are not frame payload (numpy default_rng(7))."""
    rng = np.random.default_rng(7)
    out = []
    for k in range(300):
        n = int(rng.integers(0, 16))
        rgb, audio = _frames(rng, n)
        vid = f"vid{k}" * int(rng.integers(1, 40))
        labels = rng.integers(0, FUZZ_CLASSES, size=int(rng.integers(0, 6))).tolist()
        rec = readers.make_sequence_example(vid, labels, {"rgb": rgb, "audio": audio})
        a = np.frombuffer(rec, np.uint8)
        idx = readers.locate_records(a, [0], [len(rec)], max_frames=16, num_classes=FUZZ_CLASSES)
        header = np.ones(len(rec), dtype=bool)
        for f, size in enumerate((1024, 128)):
            for t in range(n):
                o = int(idx.frame_offset[0, f, t])
                header[o:o + size] = False
        where = np.flatnonzero(header)
        mut = bytearray(rec)
        for _ in range(int(rng.integers(1, 5))):
            mut[int(where[rng.integers(0, len(where))])] = int(rng.integers(0, 256))
        out.append(bytes(mut))
    return out


def _python_outcome(reader, rec):
    try:
        return reader.prepare_serialized_examples(rec)
    except Exception:                                       # ValueError, UnicodeDecodeError, IndexError, KeyError, TypeError, ...
        return None


def test_mutated_headers_in_library():
    reader = readers.YT8MFrameFeatureReader(num_classes=FUZZ_CLASSES, max_frames=MAX_FRAMES_FUZZ)
    recs = _mutated_records()
    accepted = native_only = both_refuse = 0
    for k, rec in enumerate(recs):
        py = _python_outcome(reader, rec)
        g = _Guarded(rec)
        try:
            idx = readers.locate_records(g.array, [0], [len(rec)], max_frames=MAX_FRAMES_FUZZ, num_classes=FUZZ_CLASSES, record_base=k)
        except (ValueError, IOError) as e:
            assert py is None, f"record {k}: the Python parser accepts what the indexer refuses ({e})"
            assert f"record {k}" in str(e)
            both_refuse += 1
            continue
        if py is None:
            native_only += 1
            # what it accepted must still be in bounds
            n = int(idx.num_frames[0])
            assert 0 <= n <= MAX_FRAMES_FUZZ
            for f, size in enumerate((1024, 128)):
                o = idx.frame_offset[0, f, :n]
                assert (o >= 0).all() and (o + size <= len(rec)).all()
            assert 0 <= idx.id_offset[0] and idx.id_offset[0] + idx.id_length[0] <= len(rec)
        else:
            accepted += 1
            _agree(reader, rec, g.array, idx, 0)
    print(f"python accepted {accepted}, indexer alone accepted {native_only}, both refused {both_refuse}")
    assert accepted >= 15, "the agreement branch is (nearly) empty"          # 5 % of 300


_SANITIZER_MAIN = r"""
#include "record_index.h"
#include <stdlib.h>
#include <vector>
// input: u32 count, then per record u64 length + bytes.  Every record is indexed in a heap block of exactly its size.
int main(int argc, char** argv) {
    if (argc < 4) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const int max_frames = atoi(argv[2]), num_classes = atoi(argv[3]);
    uint32_t count = 0;
    if (fread(&count, 4, 1, f) != 1) return 2;
    const char* names[2] = {"rgb", "audio"};
    const int sizes[2] = {1024, 128};
    const lpm_index::Selection sel{2, names, sizes, max_frames, num_classes};
    std::vector<int64_t> offs(2 * (size_t)max_frames);
    for (uint32_t k = 0; k < count; ++k) {
        uint64_t n = 0;
        if (fread(&n, 8, 1, f) != 1) return 2;
        uint8_t* buf = (uint8_t*)malloc(n ? n : 1);
        if (n && fread(buf, 1, n, f) != n) return 2;
        // through the framing as well: a record framed by hand, CRCs verified
        {
            std::vector<uint8_t> framed(16 + n);
            for (int i = 0; i < 8; ++i) framed[i] = (uint8_t)(n >> (8 * i));
            uint32_t c = lpm_index::masked_crc32c(framed.data(), 8);
            memcpy(framed.data() + 8, &c, 4);
            if (n) memcpy(framed.data() + 12, buf, n);
            c = lpm_index::masked_crc32c(buf, n);
            memcpy(framed.data() + 12 + n, &c, 4);
            int64_t ro, rl, used;
            int nrec;
            char why[128];
            if (lpm_index::frame_records(framed.data(), (int64_t)framed.size(), 1, 4, 0, &ro, &rl, &nrec, &used, lpm_index::Err{why, sizeof why}) != 0 ||
                nrec != 1 || ro != 12 || rl != (int64_t)n || used != (int64_t)framed.size()) {
                printf("%u framing-mismatch\n", k);
                return 3;
            }
        }
        const int64_t ro = 0, rl = (int64_t)n;
        int32_t nf = 0, id_len = 0, label_start[2], labels[64];
        int64_t id_off = 0, needed = 0;
        int failed = -1;
        char why[256] = "";
        const int st = lpm_index::locate_records(buf, (int64_t)n, &ro, &rl, 1, k, sel, &nf, offs.data(), label_start, labels, 64, &needed, &id_off,
                                                 &id_len, &failed, lpm_index::Err{why, sizeof why});
        printf("%u %d %d %lld %d %lld", k, st, (int)nf, (long long)id_off, (int)id_len, (long long)needed);
        if (st == 0) {
            for (int64_t i = 0; i < needed && i < 64; ++i) printf(" L%d", (int)labels[i]);
            for (size_t i = 0; i < offs.size(); ++i) printf(" %lld", (long long)offs[i]);
        }
        printf("\n");
        free(buf);
    }
    fclose(f);
    return 0;
}
"""


def test_mutated_headers_under_sanitizers(tmp_path):
    """The same records through csrc/record_index.h built on its own with AddressSanitizer + UBSan (host code; nothing here touches a
    GPU): no report, and the same answers as the library."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ / clang++) to build the sanitizer executable")
    src, exe = tmp_path / "index_main.cc", tmp_path / "index_main"
    src.write_text(_SANITIZER_MAIN)
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else ["-static-libsan"]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static, "-I", CSRC, str(src), "-o",
           str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip(f"the sanitizer executable does not build here: {r.stderr.strip()[-300:]}")
    recs = _mutated_records()
    blob = tmp_path / "records.bin"
    with open(blob, "wb") as f:
        f.write(struct.pack("<I", len(recs)))
        for rec in recs:
            f.write(struct.pack("<Q", len(rec)) + rec)
    r = subprocess.run([str(exe), str(blob), str(MAX_FRAMES_FUZZ), str(FUZZ_CLASSES)], capture_output=True, text=True)
    if r.returncode != 0 and not r.stdout and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr:
        pytest.skip(f"the sanitizer executable does not start here: {r.stderr.strip()[-300:]}")
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(recs)
    for k, (rec, line) in enumerate(zip(recs, lines)):
        tok = line.split()
        assert int(tok[0]) == k
        try:
            idx = readers.locate_records(np.frombuffer(rec, np.uint8), [0], [len(rec)], max_frames=MAX_FRAMES_FUZZ, num_classes=FUZZ_CLASSES)
        except ValueError:
            assert int(tok[1]) != 0
            continue
        assert int(tok[1]) == 0 and int(tok[2]) == int(idx.num_frames[0])
        assert (int(tok[3]), int(tok[4])) == (int(idx.id_offset[0]), int(idx.id_length[0]))
        nlab = int(tok[5])
        assert [int(t[1:]) for t in tok[6:6 + nlab]] == idx.label_index[:nlab].tolist()
        assert [int(t) for t in tok[6 + nlab:]] == idx.frame_offset[0].reshape(-1).tolist()
