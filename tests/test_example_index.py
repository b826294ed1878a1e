"""-m "not gpu": the native indexer of video-level records (lpm_yt8m_locate_examples, host code of liblpm_hip.so) against the Python
parser of readers.py, which is the yardstick: offsets and strides of every float list, labels and ids on written files, protobuf-runtime
records and hand-built wire variants, and a seeded run over mutated header bytes -- in the library (every buffer ends at a PROT_NONE
page) and in a sanitizer build of csrc/record_index.h (a stand-alone executable; CPU code only)."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from learnablepoolingmethods_amd import readers

from _example_proto import example_class, framed
from test_record_index import _Guarded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "learnablepoolingmethods_amd", "csrc")
NAMES = ("mean_rgb", "mean_audio")
E, VI = readers._enc_ld, readers._enc_varint


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _vectors(rng, sizes):
    return [rng.standard_normal(s).astype(np.float32) for s in sizes]


def _features_of(reader, buf, idx, i, record):
    """Example i's feature vector as the device route forms it: the four bytes at offset + stride * k; a stride-0 feature repacked from
    the Python parser's values, as _DevicePipeline does it."""
    parts = []
    for f, (name, size) in enumerate(zip(reader.feature_names, reader.feature_sizes)):
        off, st = int(idx.feature_offset[i, f]), int(idx.feature_stride[i, f])
        assert st in (0, 4, 5)
        if st == 0:
            assert off == -1
            parts.append(np.ascontiguousarray(readers.parse_example(record)[name][1], dtype="<f4"))
        else:
            assert off >= 0 and off + st * (size - 1) + 4 <= len(buf)
            parts.append(np.concatenate([buf[off + st * k:off + st * k + 4] for k in range(size)]).view("<f4"))
    return np.concatenate(parts)


def _agree(reader, record, buf, idx, i):
    vid, x, y, _ = reader.prepare_serialized_examples(record)
    assert np.array_equal(_bits(_features_of(reader, buf, idx, i, record)), _bits(x))
    lab = idx.label_index[idx.label_start[i]:idx.label_start[i + 1]]
    assert set(lab.tolist()) == set(np.flatnonzero(y).tolist())
    o, ln = int(idx.id_offset[i]), int(idx.id_length[i])
    assert bytes(buf[o:o + ln]).decode("utf-8") == vid


def _index(reader, data: bytes):
    g = _Guarded(data)
    offs, lens, consumed = readers.frame_records(g.array, verify_crc=True)
    assert consumed == len(data)
    return g.array, readers.locate_examples(g.array, offs, lens, reader.feature_names, reader.feature_sizes, reader.num_classes)


def test_index_agrees_with_python_parser_on_written_files(tmp_path):
    rng = np.random.default_rng(31)
    reader = readers.YT8MAggregatedFeatureReader(num_classes=50)
    spec = [("v0", [1]), ("", [0, 2, 49]), ("v" * 200, []), ("v3", [7, 7]), ("v4", [50, 51, 3, 100000])]
    recs = [readers.make_example(vid, lab, dict(zip(NAMES, _vectors(rng, (1024, 128)))), packed=i != 3) for i, (vid, lab) in enumerate(spec)]
    path = str(tmp_path / "a.tfrecord")
    readers.write_tfrecord(path, recs)
    buf, idx = _index(reader, open(path, "rb").read())
    assert idx.feature_stride.tolist() == [[4, 4], [4, 4], [4, 4], [5, 5], [4, 4]]
    for i, rec in enumerate(recs):
        _agree(reader, rec, buf, idx, i)
    assert sorted(idx.label_index[idx.label_start[3]:idx.label_start[4]].tolist()) == [7, 7]
    # one feature alone; sizes that are no multiple of 4
    r1 = readers.YT8MAggregatedFeatureReader(num_classes=50, feature_sizes=(128,), feature_names=("mean_audio",))
    buf, idx = _index(r1, open(path, "rb").read())
    assert idx.feature_offset.shape == (5, 1)
    for i, rec in enumerate(recs):
        _agree(r1, rec, buf, idx, i)
    r2 = readers.YT8MAggregatedFeatureReader(num_classes=9, feature_sizes=(5, 3, 1), feature_names=("a", "b", "c"))
    recs = [readers.make_example(f"s{i}", [i], dict(zip("abc", _vectors(rng, (5, 3, 1)))), packed=bool(i % 2)) for i in range(4)]
    buf, idx = _index(r2, framed(recs))
    assert idx.feature_stride.tolist() == [[5] * 3, [4] * 3] * 2
    for i, rec in enumerate(recs):
        _agree(r2, rec, buf, idx, i)


def test_index_agrees_on_protobuf_runtime_records():
    Example = example_class()
    rng = np.random.default_rng(32)
    reader = readers.YT8MAggregatedFeatureReader(num_classes=20, feature_sizes=(24, 200))
    recs = []
    for vid, labels in (("a" * 3, [3, 17, 19]), ("long-id-" * 30, [20, 25, 2, 2, 3861]), ("", [])):
        rgb, audio = _vectors(rng, (24, 200))
        m = Example()
        m.features.feature["mean_audio"].float_list.value.extend(audio.tolist())        # 800 bytes: two-byte length varints
        m.features.feature["extra"].float_list.value.extend([0.25])
        m.features.feature["labels"].int64_list.value.extend(labels)
        m.features.feature["mean_rgb"].float_list.value.extend(rgb.tolist())
        m.features.feature["id"].bytes_list.value.append(vid.encode())
        recs += [m.SerializeToString(), readers.make_example(vid, labels, {"mean_audio": audio, "mean_rgb": rgb})]
    buf, idx = _index(reader, framed(recs))
    assert (idx.feature_stride == 4).all()
    for i, rec in enumerate(recs):
        _agree(reader, rec, buf, idx, i)
    assert sorted(idx.label_index[idx.label_start[2]:idx.label_start[3]].tolist()) == [2, 2]


def _entry(name: bytes, feature: bytes) -> bytes:
    return E(1, E(1, name) + E(2, feature))


def _unpacked(vec) -> bytes:
    raw = vec.tobytes()
    return b"".join(b"\x0d" + raw[i:i + 4] for i in range(0, len(raw), 4))


def test_hand_built_wire_variants():
    rng = np.random.default_rng(33)
    reader = readers.YT8MAggregatedFeatureReader(num_classes=30, feature_sizes=(8, 4))
    rgb, audio, other = _vectors(rng, (8, 4)) + [rng.standard_normal(8).astype(np.float32)]
    ident = _entry(b"id", readers._enc_bytes_feature([b"vid"]))
    labels = _entry(b"labels", readers._enc_int64_feature([4, 29, 30]))
    packed = lambda v: E(2, E(1, v.tobytes()))
    A = _entry(b"mean_audio", packed(audio))
    raw = rgb.tobytes()
    variants = {
        "unpacked": (_entry(b"mean_rgb", E(2, _unpacked(rgb))), 5),
        "two packed runs": (_entry(b"mean_rgb", E(2, E(1, raw[:12]) + E(1, raw[12:]))), 0),
        "packed / unpacked mix": (_entry(b"mean_rgb", E(2, _unpacked(rgb[:3]) + E(1, raw[12:]))), 0),
        "a fixed64 holding two values": (_entry(b"mean_rgb", E(2, E(1, raw[:24]) + VI((1 << 3) | 1) + raw[24:])), 0),
        "an unknown field between": (_entry(b"mean_rgb", E(2, VI((7 << 3) | 0) + VI(300) + E(1, raw))), 0),
        "a non-minimal tag": (_entry(b"mean_rgb", E(2, b"\x8a\x00" + VI(len(raw)) + raw)), 0),
        "a non-minimal length": (_entry(b"mean_rgb", E(2, b"\x0a\xa0\x00" + raw)), 0),
        "a duplicate key: the last wins": (_entry(b"mean_rgb", packed(other)) + _entry(b"mean_rgb", packed(rgb)), 4),
        "a duplicate key, the first of another size": (_entry(b"mean_rgb", packed(other[:5])) + _entry(b"mean_rgb", packed(rgb)), 4),
        "value before key": (E(1, E(2, packed(rgb)) + E(1, b"mean_rgb")), 4),
        "unselected features": (_entry(b"mean_rgb", packed(rgb)) + _entry(b"std_rgb", packed(other)) + _entry(b"tag", readers._enc_bytes_feature([b"x"])), 4),
    }
    recs, want = [], []
    for name, (entry, stride) in variants.items():
        recs.append(E(1, ident + labels + entry + A))
        want.append([stride, 4])
    recs.append(E(1, A + _entry(b"mean_rgb", packed(rgb)) + labels + ident))                       # features in reverse order
    want.append([4, 4])
    recs.append(E(1, ident + _entry(b"labels", E(2, E(1, np.array([30.0, -1.0], "<f4").tobytes()))) + A + _entry(b"mean_rgb", packed(rgb))))
    want.append([4, 4])                                                                            # float-typed labels, none of them an index
    recs.append(E(1, _entry(b"mean_rgb", packed(other))) + E(1, ident + labels + A + _entry(b"mean_rgb", packed(rgb))))   # a second `features`
    want.append([4, 4])
    buf, idx = _index(reader, framed(recs))
    assert idx.feature_stride.tolist() == want
    for i, rec in enumerate(recs):
        _agree(reader, rec, buf, idx, i)
        assert reader.prepare_serialized_examples(rec)[0] == "vid"
    assert idx.label_index[idx.label_start[0]:idx.label_start[1]].tolist() == [4, 29]
    assert idx.label_start[-2] == idx.label_start[-3]                                              # the float labels: none
    # what the Python parser refuses, the indexer refuses, naming the record
    good = recs[-1]
    refused = {
        "float-typed labels that would index": E(1, ident + _entry(b"labels", E(2, E(1, np.array([3.0], "<f4").tobytes()))) + A + variants["unpacked"][0]),
        "a truncated varint": E(1, ident + labels + A + _entry(b"mean_rgb", E(2, E(1, raw)))[:-len(raw) - 1] + b"\xa0"),
        "a run of 30 bytes": E(1, ident + labels + A + _entry(b"mean_rgb", E(2, E(1, raw[:30])))),
        "an unselected feature with a run of 5 bytes": E(1, ident + labels + A + _entry(b"mean_rgb", packed(rgb)) + _entry(b"x", E(2, E(1, b"12345")))),
        "seven values": E(1, ident + labels + A + _entry(b"mean_rgb", packed(rgb[:7]))),
        "the last of a duplicate key is short": E(1, ident + labels + A + _entry(b"mean_rgb", packed(rgb)) + _entry(b"mean_rgb", packed(rgb[:7]))),
        "an int64 list": E(1, ident + labels + A + _entry(b"mean_rgb", readers._enc_int64_feature(list(range(8))))),
        "an id that is no UTF-8": E(1, _entry(b"id", readers._enc_bytes_feature([b"\xff\xfe"])) + labels + A + _entry(b"mean_rgb", packed(rgb))),
        "a key that is no UTF-8": E(1, ident + labels + A + _entry(b"mean_rgb", packed(rgb)) + _entry(b"\xc0\x80", packed(rgb))),
    }
    for name, rec in refused.items():
        with pytest.raises(Exception):
            reader.prepare_serialized_examples(rec)
        data = framed([good, rec])
        offs, lens, _ = readers.frame_records(np.frombuffer(data, np.uint8))
        with pytest.raises(ValueError, match="record 1"):
            readers.locate_examples(np.frombuffer(data, np.uint8), offs, lens, reader.feature_names, reader.feature_sizes, reader.num_classes)


# ---- robustness: mutated header bytes -------------------------------------------------------------------------------------------------
FUZZ_SIZES, FUZZ_CLASSES, FUZZ_RECORDS = (24, 12), 3862, 400


def _mutated_records():
    """400 records in the three encodings (packed, unpacked, two runs), ids of 'vid<k>' repeated 1-19 times, 0-7 labels, sometimes an
    unselected feature; ONE random byte change each among the bytes that are not float payload (numpy default_rng(9)).  One change, not
    several: these records have some 60 header bytes, and with more than one most mutants are refused."""
    rng = np.random.default_rng(9)
    reader = readers.YT8MAggregatedFeatureReader(num_classes=FUZZ_CLASSES, feature_sizes=FUZZ_SIZES)
    out = []
    for k in range(FUZZ_RECORDS):
        rgb, audio = _vectors(rng, FUZZ_SIZES)
        vid = f"vid{k}" * int(rng.integers(1, 20))
        labels = rng.integers(0, FUZZ_CLASSES, size=int(rng.integers(0, 8))).tolist()
        mode = k % 3
        if mode < 2:
            feats = {"mean_rgb": rgb, "mean_audio": audio}
            if k % 5 == 0:
                feats["extra"] = audio[:3]
            rec = readers.make_example(vid, labels, feats, packed=mode == 0)
        else:
            raw = rgb.tobytes()
            rec = E(1, _entry(b"id", readers._enc_bytes_feature([vid.encode()])) + _entry(b"labels", readers._enc_int64_feature(labels))
                    + _entry(b"mean_rgb", E(2, E(1, raw[:40]) + E(1, raw[40:]))) + _entry(b"mean_audio", E(2, E(1, audio.tobytes()))))
        # the header: everything but the float payloads (found by their bytes: 4-byte random patterns do not repeat in 100 bytes of header)
        header = np.ones(len(rec), dtype=bool)
        for v in (rgb, audio):
            for x in v:
                at = rec.find(x.tobytes())
                assert at >= 0
                header[at:at + 4] = False
        where = np.flatnonzero(header)
        mut = bytearray(rec)
        mut[int(where[rng.integers(0, len(where))])] = int(rng.integers(0, 256))
        out.append(bytes(mut))
    return reader, out


def _python_outcome(reader, rec):
    try:
        return reader.prepare_serialized_examples(rec)
    except Exception:                                       # ValueError, UnicodeDecodeError, IndexError, KeyError, TypeError, ...
        return None


def test_mutated_headers_in_library():
    reader, recs = _mutated_records()
    accepted = refused = 0
    for k, rec in enumerate(recs):
        py = _python_outcome(reader, rec)
        g = _Guarded(rec)
        try:
            idx = readers.locate_examples(g.array, [0], [len(rec)], reader.feature_names, reader.feature_sizes, FUZZ_CLASSES, record_base=k)
        except ValueError as e:
            assert py is None, f"record {k}: the Python parser accepts what the indexer refuses ({e})"
            assert f"record {k}" in str(e)
            refused += 1
            continue
        assert py is not None, f"record {k}: the indexer accepts what the Python parser refuses"
        accepted += 1
        _agree(reader, rec, g.array, idx, 0)
    print(f"accepted {accepted}, refused {refused} of {len(recs)}")
    assert accepted >= len(recs) // 4 and refused >= len(recs) // 4


_SANITIZER_MAIN = r"""
#include "record_index.h"
#include <stdlib.h>
#include <vector>
// input: u32 count, then per record u64 length + bytes.  Every record is indexed in a heap block of exactly its size.
int main(int argc, char** argv) {
    if (argc < 5) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const int sizes[2] = {atoi(argv[2]), atoi(argv[3])};
    const int num_classes = atoi(argv[4]);
    uint32_t count = 0;
    if (fread(&count, 4, 1, f) != 1) return 2;
    const char* names[2] = {"mean_rgb", "mean_audio"};
    const lpm_index::Selection sel{2, names, sizes, 1, num_classes};
    for (uint32_t k = 0; k < count; ++k) {
        uint64_t n = 0;
        if (fread(&n, 8, 1, f) != 1) return 2;
        uint8_t* buf = (uint8_t*)malloc(n ? n : 1);
        if (n && fread(buf, 1, n, f) != n) return 2;
        const int64_t ro = 0, rl = (int64_t)n;
        int32_t stride[2] = {0, 0}, id_len = 0, label_start[2], labels[64];
        int64_t off[2] = {-1, -1}, id_off = 0, needed = 0;
        int failed = -1;
        char why[256] = "";
        const int st = lpm_index::locate_example_records(buf, (int64_t)n, &ro, &rl, 1, k, sel, off, stride, label_start, labels, 64, &needed,
                                                         &id_off, &id_len, &failed, lpm_index::Err{why, sizeof why});
        printf("%u %d %lld %d %lld", k, st, (long long)id_off, (int)id_len, (long long)needed);
        if (st == 0) {
            for (int64_t i = 0; i < needed && i < 64; ++i) printf(" L%d", (int)labels[i]);
            printf(" %lld %d %lld %d", (long long)off[0], (int)stride[0], (long long)off[1], (int)stride[1]);
        }
        printf("\n");
        free(buf);
    }
    fclose(f);
    return 0;
}
"""


def test_mutated_headers_under_sanitizers(tmp_path):
    """The same records through csrc/record_index.h built on its own with AddressSanitizer + UBSan (host code with its own main; nothing
    here touches a GPU): no report, the Python parser's accept / refuse, and the library's answers."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ / clang++) to build the sanitizer executable")
    src, exe = tmp_path / "example_index_main.cc", tmp_path / "example_index_main"
    src.write_text(_SANITIZER_MAIN)
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else ["-static-libsan"]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static, "-I", CSRC, str(src), "-o",
           str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip(f"the sanitizer executable does not build here: {r.stderr.strip()[-300:]}")
    reader, recs = _mutated_records()
    blob = tmp_path / "records.bin"
    with open(blob, "wb") as f:
        f.write(struct.pack("<I", len(recs)))
        for rec in recs:
            f.write(struct.pack("<Q", len(rec)) + rec)
    r = subprocess.run([str(exe), str(blob), *map(str, FUZZ_SIZES), str(FUZZ_CLASSES)], capture_output=True, text=True)
    if r.returncode != 0 and not r.stdout and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr:
        pytest.skip(f"the sanitizer executable does not start here: {r.stderr.strip()[-300:]}")
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(recs)
    accepted = refused = 0
    for k, (rec, line) in enumerate(zip(recs, lines)):
        tok = line.split()
        assert int(tok[0]) == k
        py = _python_outcome(reader, rec)
        assert (int(tok[1]) == 0) == (py is not None), f"record {k}: executable status {tok[1]}, Python {'accepts' if py else 'refuses'}"
        if py is None:
            refused += 1
            continue
        accepted += 1
        a = np.frombuffer(rec, np.uint8)
        idx = readers.locate_examples(a, [0], [len(rec)], reader.feature_names, reader.feature_sizes, FUZZ_CLASSES)
        assert (int(tok[2]), int(tok[3])) == (int(idx.id_offset[0]), int(idx.id_length[0]))
        nlab = int(tok[4])
        assert [int(t[1:]) for t in tok[5:5 + nlab]] == idx.label_index[:nlab].tolist()
        assert [int(t) for t in tok[5 + nlab:]] == [int(idx.feature_offset[0, 0]), int(idx.feature_stride[0, 0]), int(idx.feature_offset[0, 1]),
                                                    int(idx.feature_stride[0, 1])]
        _agree(reader, rec, a, idx, 0)
    assert accepted >= len(recs) // 4 and refused >= len(recs) // 4
