// Host-side indexer of YT8M TFRecord files (readers.py: read_tfrecord + parse_sequence_example + prepare_serialized_examples): finds
// WHERE every frame's payload lies in a buffer of records without touching the payload, so that the records can go to the GPU as they
// are and lpm_gather_frames puts the frames in place.  Plain C++ (no HIP header): record_index.hip wraps it into the C ABI, and the
// tests compile it on its own with host sanitizers.
//
// The protobuf walk follows the Python parser's semantics, not the protobuf specification's, because that parser is the yardstick:
//   * a length that runs past the end of its enclosing message is CLAMPED to that end (Python: a slice of a memoryview), the same for a
//     fixed32 / fixed64 cut short; the walk itself never reads past the enclosing message, let alone the buffer;
//   * a varint that runs off the end of its message, and wire types 3, 4, 6, 7, are errors;
//   * varints are unbounded: 128 bits are kept, more than that is remembered as "too large to match anything";
//   * map entries: the last key / value of an entry count, the last entry of a key counts, a second `context` / `feature_lists` field
//     replaces the first; a tf.train.Feature is its FIRST field numbered 1, 2 or 3, whatever follows it is not looked at;
//   * a field of another wire type than the schema's is taken the way the Python walk takes it: its (clamped) bytes are the message,
//     a varint stands for an empty one;
//   * labels: int64 values v with 0 <= v < num_classes, after the two's-complement wrap at 2^63 (so 2^64 + 5 is label 5); a float list
//     is accepted while none of its values lies in [0, num_classes); a bytes list while it is empty;
//   * frames: the first value of every frame's bytes list; EVERY frame of a selected feature has to be exactly feature_size bytes (the
//     Python path fails in np.stack / reshape), frames beyond max_frames included; the frame counts of the selected features are
//     compared after capping at max_frames.
// Where the Python path raises, this one reports LPM_ERR_DATA with the record's index; where Python accepts, so does this, with the
// same fields.  Entries of features that are not selected, and values of an entry that a later value replaces, are skipped unparsed.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/lpm_hip.h"

namespace lpm_index {

typedef unsigned __int128 u128;

struct Err {
    char* buf;
    size_t n;
    void set(const char* fmt, ...) const {
        if (!buf || !n) return;
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, n, fmt, ap);
        va_end(ap);
    }
};

// ---- CRC-32C (Castagnoli) and the TFRecord mask --------------------------------------------------------------------------------------
struct CrcTables {
    uint32_t t[8][256];
    CrcTables() {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
            t[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; ++i)
            for (int s = 1; s < 8; ++s) t[s][i] = (t[s - 1][i] >> 8) ^ t[0][t[s - 1][i] & 0xFF];
    }
};

inline uint64_t load_le64(const uint8_t* p) {
    uint64_t v = 0;
    for (int i = 7; i >= 0; --i) v = (v << 8) | p[i];
    return v;
}
inline uint32_t load_le32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// slice-by-8
inline uint32_t crc32c_sw(uint32_t c, const uint8_t* p, size_t n) {
    static const CrcTables T;
    while (n >= 8) {
        const uint64_t w = load_le64(p) ^ c;
        c = T.t[7][w & 0xFF] ^ T.t[6][(w >> 8) & 0xFF] ^ T.t[5][(w >> 16) & 0xFF] ^ T.t[4][(w >> 24) & 0xFF] ^ T.t[3][(w >> 32) & 0xFF] ^
            T.t[2][(w >> 40) & 0xFF] ^ T.t[1][(w >> 48) & 0xFF] ^ T.t[0][w >> 56];
        p += 8;
        n -= 8;
    }
    while (n--) c = T.t[0][(c ^ *p++) & 0xFF] ^ (c >> 8);
    return c;
}

#if defined(__x86_64__)
// the CPU's crc32 instruction, three independent streams of LANE bytes per round (the instruction has a latency of three cycles and a
// throughput of one); the streams are joined by advancing a CRC over LANE zero bytes, which is linear: four 256-entry tables
constexpr size_t CRC_LANE = 1024;
struct CrcShift {
    uint32_t t[4][256];     // t[k][b]: the CRC state (b << 8k) advanced over CRC_LANE zero bytes
    CrcShift() {
        for (int k = 0; k < 4; ++k)
            for (uint32_t b = 0; b < 256; ++b) {
                uint32_t c = b << (8 * k);
                static const uint8_t zeros[CRC_LANE] = {0};
                t[k][b] = crc32c_sw(c, zeros, CRC_LANE);
            }
    }
    uint32_t shift(uint32_t c) const { return t[0][c & 0xFF] ^ t[1][(c >> 8) & 0xFF] ^ t[2][(c >> 16) & 0xFF] ^ t[3][c >> 24]; }
};
__attribute__((target("sse4.2"))) inline uint32_t crc32c_hw(uint32_t c, const uint8_t* p, size_t n) {
    static const CrcShift S;
    while (n >= 3 * CRC_LANE) {
        uint64_t a = c, b = 0, d = 0;
        for (size_t i = 0; i < CRC_LANE; i += 8) {
            uint64_t x, y, z;
            memcpy(&x, p + i, 8);
            memcpy(&y, p + CRC_LANE + i, 8);
            memcpy(&z, p + 2 * CRC_LANE + i, 8);
            a = __builtin_ia32_crc32di(a, x);
            b = __builtin_ia32_crc32di(b, y);
            d = __builtin_ia32_crc32di(d, z);
        }
        c = S.shift(S.shift((uint32_t)a) ^ (uint32_t)b) ^ (uint32_t)d;
        p += 3 * CRC_LANE;
        n -= 3 * CRC_LANE;
    }
    uint64_t a = c;
    while (n >= 8) {
        uint64_t x;
        memcpy(&x, p, 8);
        a = __builtin_ia32_crc32di(a, x);
        p += 8;
        n -= 8;
    }
    c = (uint32_t)a;
    while (n--) c = __builtin_ia32_crc32qi(c, *p++);
    return c;
}
#endif

// force_sw: the tests compare the two implementations
inline uint32_t crc32c(const uint8_t* p, size_t n, bool force_sw = false) {
#if defined(__x86_64__)
    static const bool hw = __builtin_cpu_supports("sse4.2");
    if (hw && !force_sw) return crc32c_hw(0xFFFFFFFFu, p, n) ^ 0xFFFFFFFFu;
#endif
    return crc32c_sw(0xFFFFFFFFu, p, n) ^ 0xFFFFFFFFu;
}

inline uint32_t masked_crc32c(const uint8_t* p, size_t n) {
    const uint32_t c = crc32c(p, n);
    return ((c >> 15) | (c << 17)) + 0xA282EAD8u;
}

// ---- TFRecord framing -------------------------------------------------------------------------------------------------------------------
// Walks whole records from the start of buf: payload offset / length of each into rec_offset / rec_length (max_records entries), their
// number into *num_records and the bytes they take (framing included) into *consumed.  Stops without an error at max_records or where
// the rest of the buffer does not hold a whole record (a caller reading a file in pieces carries buf + *consumed on).  verify_crc checks
// both masked CRCs; a mismatch is LPM_ERR_IO, *num_records then counts the records before the bad one.
inline int frame_records(const uint8_t* buf, int64_t nbytes, int verify_crc, int max_records, int64_t record_base, int64_t* rec_offset,
                         int64_t* rec_length, int* num_records, int64_t* consumed, const Err& err) {
    int64_t pos = 0;
    int n = 0;
    int status = LPM_OK;
    while (n < max_records && nbytes - pos >= 12) {
        const uint64_t len = load_le64(buf + pos);
        if (verify_crc && masked_crc32c(buf + pos, 8) != load_le32(buf + pos + 8)) {
            err.set("record %lld: corrupt record length", (long long)(record_base + n));
            status = LPM_ERR_IO;
            break;
        }
        const uint64_t rest = (uint64_t)(nbytes - pos - 12);
        if (len > rest || rest - len < 4) break;                  // not all here yet
        const uint8_t* data = buf + pos + 12;
        if (verify_crc && masked_crc32c(data, (size_t)len) != load_le32(data + len)) {
            err.set("record %lld: corrupt record payload", (long long)(record_base + n));
            status = LPM_ERR_IO;
            break;
        }
        rec_offset[n] = pos + 12;
        rec_length[n] = (int64_t)len;
        pos += 16 + (int64_t)len;
        ++n;
    }
    *num_records = n;
    *consumed = pos;
    return status;
}

// ---- protobuf wire format, the Python walk's way ---------------------------------------------------------------------------------------
struct Span {
    const uint8_t* p;
    const uint8_t* e;
    size_t size() const { return (size_t)(e - p); }
};

// false: ran off the end.  v: the low 128 bits; big: bits beyond them were set
inline bool varint(const uint8_t*& p, const uint8_t* e, u128& v, bool& big) {
    v = 0;
    big = false;
    int shift = 0;
    for (;;) {
        if (p >= e) return false;
        const uint8_t b = *p++;
        const uint8_t d = b & 0x7F;
        if (shift < 128) {
            v |= (u128)d << shift;
            if (shift > 121 && (d >> (128 - shift))) big = true;
        } else if (d) {
            big = true;
        }
        if (!(b & 0x80)) return true;
        if (shift < 128) shift += 7;
    }
}

struct Field {
    u128 num;      // field number (all ones when it does not fit)
    int wt;
    u128 val;      // wire type 0
    bool val_big;
    Span s;        // wire types 2, 5, 1: the value's bytes, clamped to the message; wire type 0: empty
    bool is(unsigned k) const { return num == (u128)k; }
};

enum { FIELD_END = 0, FIELD_OK = 1, FIELD_BAD = -1 };

inline int next_field(const uint8_t*& p, const uint8_t* e, Field& f) {
    if (p >= e) return FIELD_END;
    u128 key;
    bool big;
    if (!varint(p, e, key, big)) return FIELD_BAD;
    f.wt = (int)(key & 7);
    f.num = big ? ~(u128)0 : key >> 3;
    f.val = 0;
    f.val_big = false;
    f.s = Span{p, p};
    const size_t avail = (size_t)(e - p);
    switch (f.wt) {
        case 0:
            if (!varint(p, e, f.val, f.val_big)) return FIELD_BAD;
            f.s = Span{p, p};
            return FIELD_OK;
        case 2: {
            u128 ln;
            bool lbig;
            if (!varint(p, e, ln, lbig)) return FIELD_BAD;
            const size_t av = (size_t)(e - p);
            const size_t n = (lbig || ln > (u128)av) ? av : (size_t)ln;
            f.s = Span{p, p + n};
            p = (lbig || ln > (u128)av) ? e : p + n;
            return FIELD_OK;
        }
        case 5:
        case 1: {
            const size_t want = f.wt == 5 ? 4 : 8;
            const size_t n = want < avail ? want : avail;
            f.s = Span{p, p + n};
            p = want < avail ? p + n : e;
            return FIELD_OK;
        }
        default:
            return FIELD_BAD;
    }
}

enum { KIND_EMPTY = 0, KIND_BYTES = 1, KIND_FLOAT = 2, KIND_INT64 = 3 };

// tf.train.Feature: the first field numbered 1 (bytes_list), 2 (float_list) or 3 (int64_list); false: malformed before it
inline bool parse_feature(Span s, int& kind, Span& list) {
    const uint8_t* p = s.p;
    Field f;
    for (;;) {
        const int r = next_field(p, s.e, f);
        if (r == FIELD_BAD) return false;
        if (r == FIELD_END) break;
        if (f.is(1) || f.is(2) || f.is(3)) {
            kind = f.is(1) ? KIND_BYTES : f.is(2) ? KIND_FLOAT : KIND_INT64;
            list = f.s;
            return true;
        }
    }
    kind = KIND_EMPTY;
    list = Span{s.e, s.e};
    return true;
}

// BytesList: the number of values and the first one; -1: malformed (or a first value that is not length-delimited bytes)
inline int bytes_list(Span s, Span& first) {
    const uint8_t* p = s.p;
    Field f;
    int n = 0;
    for (;;) {
        const int r = next_field(p, s.e, f);
        if (r == FIELD_BAD) return -1;
        if (r == FIELD_END) return n;
        if (!f.is(1)) continue;
        if (n == 0) {
            if (f.wt == 0 && (f.val != 0 || f.val_big)) return -1;   // (Python: that many zero bytes.  Not a payload that lies in the file.)
            first = f.s;
        }
        if (n < 0x7FFFFFFF) ++n;
    }
}

// a label value of an Int64List: index in [0, num_classes) or -1
inline int64_t label_of(u128 v, bool big, int num_classes) {
    if (big) return -1;
    const u128 two64 = (u128)1 << 64;
    if (v >= two64) v -= two64;                       // Python: val - 2^64 for val >= 2^63 (values in [2^63, 2^64) come out negative)
    return v < (u128)(num_classes > 0 ? num_classes : 0) ? (int64_t)v : -1;
}

struct LabelSink {
    int32_t* out;
    int64_t cap;
    int64_t n;         // written or wanted
    void put(int32_t v) {
        if (n < cap) out[n] = v;
        ++n;
    }
};

// the labels of a context feature of any kind; false: the Python path raises
inline bool collect_labels(int kind, Span list, int num_classes, LabelSink& sink) {
    const uint8_t* p = list.p;
    Field f;
    if (kind == KIND_EMPTY) return true;
    if (kind == KIND_BYTES) {
        Span first;
        return bytes_list(list, first) == 0;
    }
    for (;;) {
        const int r = next_field(p, list.e, f);
        if (r == FIELD_BAD) return false;
        if (r == FIELD_END) return true;
        if (!f.is(1)) continue;
        if (kind == KIND_INT64) {
            if (f.wt == 0) {
                const int64_t l = label_of(f.val, f.val_big, num_classes);
                if (l >= 0) sink.put((int32_t)l);
            } else {                                   // packed
                const uint8_t* q = f.s.p;
                while (q < f.s.e) {
                    u128 v;
                    bool big;
                    if (!varint(q, f.s.e, v, big)) return false;
                    const int64_t l = label_of(v, big, num_classes);
                    if (l >= 0) sink.put((int32_t)l);
                }
            }
        } else {                                       // floats: fine while none of them would index the dense row
            if (f.wt == 0) {
                if (f.val != 0 || f.val_big) return false;
                continue;
            }
            if (f.s.size() % 4) return false;
            for (const uint8_t* q = f.s.p; q < f.s.e; q += 4) {
                float x;
                const uint32_t u = load_le32(q);
                memcpy(&x, &u, 4);
                if (x >= 0.f && x < (float)num_classes) return false;
            }
        }
    }
}

// a map entry: the last field 1 is the key, the last field 2 the value
inline bool map_entry(Span s, Span& key, bool& has_key, Span& val, bool& has_val) {
    const uint8_t* p = s.p;
    Field f;
    has_key = has_val = false;
    for (;;) {
        const int r = next_field(p, s.e, f);
        if (r == FIELD_BAD) return false;
        if (r == FIELD_END) return true;
        if (f.is(1)) {
            // (a varint as the key stands for that many zero bytes in the Python walk: never one of our names.  An empty span does.)
            key = f.s;
            has_key = !(f.wt == 0);
        } else if (f.is(2)) {
            val = f.s;
            has_val = true;
        }
    }
}

inline bool key_is(Span key, const char* name) {
    const size_t n = strlen(name);
    return key.size() == n && memcmp(key.p, name, n) == 0;
}

struct Selection {
    int num_features;
    const char* const* names;
    const int* sizes;
    int max_frames;
    int num_classes;
};

constexpr int MAX_FEATURES = 8;

// The bytes in front of a frame's payload as every protobuf encoder writes them (minimal varints):
//   0A len(Feature)  0A len(BytesList)  0A size   -- FeatureList.feature = 1 { Feature.bytes_list = 1 { BytesList.value = 1 } }
// 9 bytes for 1024 and for 128.  locate_one compares them in one go and falls back to the field-by-field walk for anything else.
constexpr size_t CANON_MAX = 3 * 11;
inline size_t put_varint(uint64_t v, uint8_t* out) {
    size_t n = 0;
    do {
        out[n++] = (uint8_t)((v & 0x7F) | (v > 0x7F ? 0x80 : 0));
        v >>= 7;
    } while (v);
    return n;
}
inline size_t canonical_frame_header(int size, uint8_t* out) {
    uint8_t l0[10], l1[10], l2[10];
    const size_t n0 = put_varint((uint64_t)size, l0);
    const uint64_t bytes_list = 1 + n0 + (uint64_t)size;
    const size_t n1 = put_varint(bytes_list, l1);
    const uint64_t feature = 1 + n1 + bytes_list;
    const size_t n2 = put_varint(feature, l2);
    size_t n = 0;
    out[n++] = 0x0A;
    memcpy(out + n, l2, n2), n += n2;
    out[n++] = 0x0A;
    memcpy(out + n, l1, n1), n += n1;
    out[n++] = 0x0A;
    memcpy(out + n, l0, n0), n += n0;
    return n;
}

// One SequenceExample.  frame_offset: [num_features, max_frames] for this clip.  Returns LPM_OK or LPM_ERR_DATA (message in err,
// without the record's index: the caller adds it).
inline int locate_one(const uint8_t* buf, Span rec, const Selection& sel, int32_t* num_frames, int64_t* frame_offset, LabelSink& labels,
                      int64_t* id_offset, int32_t* id_length, char* why, size_t why_n) {
    const Err err{why, why_n};
    // state of the two maps, replaced as later fields / entries override earlier ones
    bool id_present = false, id_ok = false;
    Span id = Span{rec.p, rec.p};
    const int64_t labels_mark = labels.n;
    bool feat_present[MAX_FEATURES];
    int64_t feat_count[MAX_FEATURES];
    for (int j = 0; j < sel.num_features; ++j) feat_present[j] = false, feat_count[j] = 0;

    const uint8_t* p = rec.p;
    Field top;
    for (;;) {
        const int r = next_field(p, rec.e, top);
        if (r == FIELD_BAD) {
            err.set("malformed SequenceExample");
            return LPM_ERR_DATA;
        }
        if (r == FIELD_END) break;
        if (top.is(1)) {                                // context: Features { map<string, Feature> feature = 1 }
            id_present = id_ok = false;
            labels.n = labels_mark;
            const uint8_t* q = top.s.p;
            Field ent;
            for (;;) {
                const int r2 = next_field(q, top.s.e, ent);
                if (r2 == FIELD_BAD) {
                    err.set("malformed context");
                    return LPM_ERR_DATA;
                }
                if (r2 == FIELD_END) break;
                if (!ent.is(1)) continue;
                Span key, val;
                bool has_key, has_val;
                if (!map_entry(ent.s, key, has_key, val, has_val)) {
                    err.set("malformed context entry");
                    return LPM_ERR_DATA;
                }
                if (!has_key) continue;
                const bool is_id = key_is(key, "id"), is_labels = key_is(key, "labels");
                if (!is_id && !is_labels) continue;
                int kind = KIND_EMPTY;
                Span list = Span{rec.p, rec.p};
                if (!has_val || !parse_feature(val, kind, list)) {
                    err.set("context feature '%s' has no readable value", is_id ? "id" : "labels");
                    return LPM_ERR_DATA;
                }
                if (is_id) {
                    id_present = true;
                    id_ok = kind == KIND_BYTES && bytes_list(list, id) > 0;
                } else {
                    labels.n = labels_mark;
                    if (!collect_labels(kind, list, sel.num_classes, labels)) {
                        err.set("context feature 'labels' is not a list of class indices");
                        return LPM_ERR_DATA;
                    }
                }
            }
        } else if (top.is(2)) {                         // feature_lists: FeatureLists { map<string, FeatureList> feature_list = 1 }
            for (int j = 0; j < sel.num_features; ++j) feat_present[j] = false, feat_count[j] = 0;
            const uint8_t* q = top.s.p;
            Field ent;
            for (;;) {
                const int r2 = next_field(q, top.s.e, ent);
                if (r2 == FIELD_BAD) {
                    err.set("malformed feature_lists");
                    return LPM_ERR_DATA;
                }
                if (r2 == FIELD_END) break;
                if (!ent.is(1)) continue;
                Span key, val;
                bool has_key, has_val;
                if (!map_entry(ent.s, key, has_key, val, has_val)) {
                    err.set("malformed feature_lists entry");
                    return LPM_ERR_DATA;
                }
                if (!has_key) continue;
                for (int j = 0; j < sel.num_features; ++j) {
                    if (!key_is(key, sel.names[j])) continue;
                    if (!has_val) {
                        err.set("feature list '%s' has no value", sel.names[j]);
                        return LPM_ERR_DATA;
                    }
                    // FeatureList { repeated Feature feature = 1 }
                    int64_t count = 0;
                    const uint8_t* w = val.p;
                    Field fr;
                    uint8_t canon[CANON_MAX];
                    const size_t canon_n = canonical_frame_header(sel.sizes[j], canon);
                    const size_t step = canon_n + (size_t)sel.sizes[j];
                    for (;;) {
                        // the frame every writer emits, byte for byte (what the general walk below would find in it: one value of the
                        // feature's size and nothing else)
                        __builtin_prefetch(w + 8 * step);        // (the headers lie a frame apart: one cache miss each, known in advance)
                        if ((size_t)(val.e - w) >= step && memcmp(w, canon, canon_n) == 0) {
                            if (count < sel.max_frames) frame_offset[(int64_t)j * sel.max_frames + count] = (int64_t)(w + canon_n - buf);
                            ++count;
                            w += step;
                            continue;
                        }
                        const int r3 = next_field(w, val.e, fr);
                        if (r3 == FIELD_BAD) {
                            err.set("malformed feature list '%s'", sel.names[j]);
                            return LPM_ERR_DATA;
                        }
                        if (r3 == FIELD_END) break;
                        if (!fr.is(1)) continue;
                        int kind;
                        Span list, first;
                        if (!parse_feature(fr.s, kind, list) || kind != KIND_BYTES || bytes_list(list, first) <= 0) {
                            err.set("feature '%s': frame %lld is not a bytes value", sel.names[j], (long long)count);
                            return LPM_ERR_DATA;
                        }
                        if (first.size() != (size_t)sel.sizes[j]) {
                            err.set("feature '%s': frame %lld has %zu bytes, expected %d", sel.names[j], (long long)count, first.size(),
                                    sel.sizes[j]);
                            return LPM_ERR_DATA;
                        }
                        if (count < sel.max_frames) frame_offset[(int64_t)j * sel.max_frames + count] = (int64_t)(first.p - buf);
                        ++count;
                    }
                    feat_present[j] = true;
                    feat_count[j] = count;
                }
            }
        }
    }
    if (id_present && !id_ok) {
        err.set("context feature 'id' is not a bytes value");
        return LPM_ERR_DATA;
    }
    int64_t n0 = 0;
    for (int j = 0; j < sel.num_features; ++j) {
        if (!feat_present[j]) {
            err.set("feature list '%s' is missing", sel.names[j]);
            return LPM_ERR_DATA;
        }
        const int64_t n = feat_count[j] < sel.max_frames ? feat_count[j] : sel.max_frames;
        if (j == 0) n0 = n;
        else if (n != n0) {
            err.set("feature '%s' has %lld frames, expected %lld", sel.names[j], (long long)n, (long long)n0);
            return LPM_ERR_DATA;
        }
    }
    for (int j = 0; j < sel.num_features; ++j)
        for (int64_t t = n0; t < sel.max_frames; ++t) frame_offset[(int64_t)j * sel.max_frames + t] = -1;
    *num_frames = (int32_t)n0;
    *id_offset = id_present ? (int64_t)(id.p - buf) : 0;
    *id_length = id_present ? (int32_t)id.size() : 0;
    return LPM_OK;
}

// The loop over the records of a buffer (frame_records' output) that both locators share: bounds of every record, the CSR label list
// (label_start [num_records + 1], label_index [label_capacity]) and the error's record index.  one(i, rec, sink, why, why_n) locates
// record i.  LPM_ERR_DATA: a malformed example, *failed_record its index; LPM_ERR_WORKSPACE: label_capacity is too small,
// *labels_needed says how many there are.
template <class One>
inline int locate_each(const uint8_t* buf, int64_t nbytes, const int64_t* rec_offset, const int64_t* rec_length, int num_records,
                       int64_t record_base, int32_t* label_start, int32_t* label_index, int64_t label_capacity, int64_t* labels_needed,
                       int* failed_record, const Err& err, One one) {
    LabelSink sink{label_index, label_capacity, 0};
    *failed_record = -1;
    for (int i = 0; i < num_records; ++i) {
        if (rec_offset[i] < 0 || rec_length[i] < 0 || rec_offset[i] > nbytes || rec_length[i] > nbytes - rec_offset[i]) {
            err.set("record %lld: offset %lld, length %lld outside the buffer of %lld bytes", (long long)(record_base + i),
                    (long long)rec_offset[i], (long long)rec_length[i], (long long)nbytes);
            *failed_record = i;
            return LPM_ERR_BADARG;
        }
        label_start[i] = (int32_t)sink.n;
        char why[200] = "";
        const Span rec{buf + rec_offset[i], buf + rec_offset[i] + rec_length[i]};
        const int st = one(i, rec, sink, why, sizeof why);
        if (st != LPM_OK) {
            err.set("record %lld: %s", (long long)(record_base + i), why);
            *failed_record = i;
            return st;
        }
        if (sink.n > 0x7FFFFFFF) {
            err.set("record %lld: more than 2^31 labels", (long long)(record_base + i));
            *failed_record = i;
            return LPM_ERR_DATA;
        }
    }
    label_start[num_records] = (int32_t)sink.n;
    *labels_needed = sink.n;
    if (sink.n > label_capacity) {
        err.set("label_capacity %lld is too small for %lld labels", (long long)label_capacity, (long long)sink.n);
        return LPM_ERR_WORKSPACE;
    }
    return LPM_OK;
}

// All SequenceExample records of a buffer.  Per clip: num_frames (capped at max_frames), frame_offset [clip, feature, max_frames]
// (byte offsets from buf of the frame payloads; -1 at and beyond num_frames), the labels in [0, num_classes) as a CSR list and the
// video id's offset / length (0 / 0 without one).
inline int locate_records(const uint8_t* buf, int64_t nbytes, const int64_t* rec_offset, const int64_t* rec_length, int num_records,
                          int64_t record_base, const Selection& sel, int32_t* num_frames, int64_t* frame_offset, int32_t* label_start,
                          int32_t* label_index, int64_t label_capacity, int64_t* labels_needed, int64_t* id_offset, int32_t* id_length,
                          int* failed_record, const Err& err) {
    return locate_each(buf, nbytes, rec_offset, rec_length, num_records, record_base, label_start, label_index, label_capacity, labels_needed,
                       failed_record, err, [&](int i, Span rec, LabelSink& sink, char* why, size_t why_n) {
                           return locate_one(buf, rec, sel, num_frames + i, frame_offset + (int64_t)i * sel.num_features * sel.max_frames,
                                             sink, id_offset + i, id_length + i, why, why_n);
                       });
}

// ---- tf.train.Example records (readers.YT8MAggregatedFeatureReader: parse_example + prepare_serialized_examples) ------------------------
// Example { Features features = 1 },  Features { map<string, Feature> feature = 1 }.  The walk is the one above with these additions,
// again the Python parser's way, which looks at EVERY entry of the map whether selected or not:
//   * every key, and the id, has to be UTF-8 as Python's strict decoder takes it (no overlong forms, no surrogates, nothing beyond
//     U+10FFFF); a varint where a message is expected stands for that many zero bytes, which is a message only when their number is even;
//   * every value is parsed: an unselected feature with a malformed list refuses the record as well;
//   * a FloatList is the concatenation of all its fields numbered 1, whatever their wire type: a length-delimited run, a fixed32, a
//     fixed64 (two floats), a varint (that many zero bytes); every one has to be a whole number of floats;
//   * a selected feature has to be a float list of exactly feature_size values (tf.FixedLenFeature) in the LAST entry of its key.
// A float list that passes is reported by the stride between its values: 4, one packed run and nothing else, as every writer emits it
// (offset: the run); 5, nothing but one-byte-tagged fixed32 values (offset: the first one's payload); 0, anything else that is valid
// (several runs, a mix, unknown fields, non-minimal tags; offset -1: the caller repacks that feature with the Python parser).

// Python's bytes.decode("utf-8")
inline bool utf8_ok(Span s) {
    const uint8_t* p = s.p;
    while (p < s.e) {
        const uint8_t c = *p++;
        if (c < 0x80) continue;
        int more;
        uint8_t lo = 0x80, hi = 0xBF;                   // the range of the first continuation byte
        if (c >= 0xC2 && c <= 0xDF) more = 1;
        else if (c >= 0xE0 && c <= 0xEF) more = 2, lo = c == 0xE0 ? 0xA0 : 0x80, hi = c == 0xED ? 0x9F : 0xBF;
        else if (c >= 0xF0 && c <= 0xF4) more = 3, lo = c == 0xF0 ? 0x90 : 0x80, hi = c == 0xF4 ? 0x8F : 0xBF;
        else return false;
        for (int i = 0; i < more; ++i, lo = 0x80, hi = 0xBF)
            if (p >= s.e || *p < lo || *p++ > hi) return false;
    }
    return true;
}

// a varint in place of a message: Python walks that many zero bytes, pairs of (field 0, varint 0)
inline bool message_ok(const Field& f) { return f.wt != 0 || (!f.val_big && !(f.val & 1)); }

// FloatList: the number of values, or -1 where the Python walk raises
inline int64_t float_list(Span s) {
    const uint8_t* p = s.p;
    Field f;
    int64_t n = 0;
    for (;;) {
        const int r = next_field(p, s.e, f);
        if (r == FIELD_BAD) return -1;
        if (r == FIELD_END) return n;
        if (!f.is(1)) continue;
        u128 bytes = f.wt == 0 ? f.val : (u128)f.s.size();
        if ((f.wt == 0 && f.val_big) || (bytes & 3) || bytes > ((u128)1 << 40)) return -1;
        n += (int64_t)(bytes >> 2);
    }
}

// what _parse_feature does with a value nobody selected: true where it returns
inline bool feature_parses(Span val) {
    int kind;
    Span list;
    if (!parse_feature(val, kind, list)) return false;
    if (kind == KIND_BYTES) {
        const uint8_t* p = list.p;                       // (bytes_list refuses a first value that does not lie in the file: not an error here)
        Field f;
        for (;;) {
            const int r = next_field(p, list.e, f);
            if (r != FIELD_OK) return r == FIELD_END;
        }
    }
    if (kind == KIND_FLOAT) return float_list(list) >= 0;
    if (kind == KIND_INT64) {
        LabelSink none{nullptr, 0, 0};
        return collect_labels(kind, list, 0, none);
    }
    return true;
}

// The bytes of a Feature that holds one packed float run, as every protobuf encoder writes them (minimal varints):
//   12 len(FloatList)  0A 4 * size   -- Feature.float_list = 2 { FloatList.value = 1, packed }
inline size_t canonical_float_header(int size, uint8_t* out) {
    uint8_t l0[10], l1[10];
    const size_t n0 = put_varint(4 * (uint64_t)size, l0);
    const size_t n1 = put_varint(1 + n0 + 4 * (uint64_t)size, l1);
    size_t n = 0;
    out[n++] = 0x12;
    memcpy(out + n, l1, n1), n += n1;
    out[n++] = 0x0A;
    memcpy(out + n, l0, n0), n += n0;
    return n;
}

enum { FEAT_MISSING = 0, FEAT_NO_VALUE, FEAT_NOT_FLOAT, FEAT_FLOAT };

// One Example.  feature_offset / feature_stride: [num_features] for this record.
inline int locate_example(const uint8_t* buf, Span rec, const Selection& sel, const uint8_t (*canon)[CANON_MAX], const size_t* canon_n,
                          int64_t* feature_offset, int32_t* feature_stride, LabelSink& labels, int64_t* id_offset, int32_t* id_length,
                          char* why, size_t why_n) {
    const Err err{why, why_n};
    bool id_present = false, id_ok = false;
    Span id = Span{rec.p, rec.p};
    const int64_t labels_mark = labels.n;
    int state[MAX_FEATURES];
    int64_t count[MAX_FEATURES];
    for (int j = 0; j < sel.num_features; ++j) state[j] = FEAT_MISSING, count[j] = 0;

    const uint8_t* p = rec.p;
    Field top;
    for (;;) {
        const int r = next_field(p, rec.e, top);
        if (r == FIELD_BAD) {
            err.set("malformed Example");
            return LPM_ERR_DATA;
        }
        if (r == FIELD_END) break;
        if (!top.is(1)) continue;
        // features: a second field replaces the first (which has been walked, as in Python)
        id_present = id_ok = false;
        labels.n = labels_mark;
        for (int j = 0; j < sel.num_features; ++j) state[j] = FEAT_MISSING;
        if (!message_ok(top)) {
            err.set("malformed features");
            return LPM_ERR_DATA;
        }
        const uint8_t* q = top.s.p;
        Field ent;
        for (;;) {
            const int r2 = next_field(q, top.s.e, ent);
            if (r2 == FIELD_BAD) {
                err.set("malformed features");
                return LPM_ERR_DATA;
            }
            if (r2 == FIELD_END) break;
            if (!ent.is(1)) continue;
            Span key, val;
            bool has_key, has_val;
            if (!message_ok(ent) || !map_entry(ent.s, key, has_key, val, has_val) || (has_key && !utf8_ok(key))) {
                err.set("malformed features entry");
                return LPM_ERR_DATA;
            }
            int j = -1;
            if (has_key)
                for (int k = 0; k < sel.num_features; ++k)
                    if (key_is(key, sel.names[k])) j = k;
            if (j >= 0) {
                // (a name selected twice: the later column only -- the reader refuses such a selection before it gets here)
                if (!has_val) {
                    state[j] = FEAT_NO_VALUE;
                    continue;
                }
                // the feature every writer emits, byte for byte: one packed run of the feature's size and nothing else
                if (val.size() == canon_n[j] + 4 * (size_t)sel.sizes[j] && memcmp(val.p, canon[j], canon_n[j]) == 0) {
                    state[j] = FEAT_FLOAT, count[j] = sel.sizes[j];
                    feature_offset[j] = (int64_t)(val.p + canon_n[j] - buf), feature_stride[j] = 4;
                    continue;
                }
                int kind;
                Span list;
                if (!parse_feature(val, kind, list)) {
                    err.set("feature '%s' has no readable value", sel.names[j]);
                    return LPM_ERR_DATA;
                }
                if (kind != KIND_FLOAT) {
                    if (!feature_parses(val)) {
                        err.set("feature '%s' has no readable value", sel.names[j]);
                        return LPM_ERR_DATA;
                    }
                    state[j] = FEAT_NOT_FLOAT;
                    continue;
                }
                const int64_t n = float_list(list);
                if (n < 0) {
                    err.set("feature '%s' is not a list of whole floats", sel.names[j]);
                    return LPM_ERR_DATA;
                }
                state[j] = FEAT_FLOAT, count[j] = n;
                feature_offset[j] = -1, feature_stride[j] = 0;
                if (n == sel.sizes[j] && list.size() == 5 * (size_t)n) {
                    bool tagged = true;
                    for (int64_t i = 0; i < n && tagged; ++i) tagged = list.p[5 * i] == 0x0D;       // field 1, fixed32
                    if (tagged) feature_offset[j] = (int64_t)(list.p + 1 - buf), feature_stride[j] = 5;
                }
                continue;
            }
            const bool is_id = has_key && key_is(key, "id"), is_labels = has_key && key_is(key, "labels");
            if (!is_id && !is_labels) {
                if (has_val && !feature_parses(val)) {
                    err.set("malformed feature");
                    return LPM_ERR_DATA;
                }
                continue;
            }
            int kind = KIND_EMPTY;
            Span list = Span{rec.p, rec.p};
            if (!has_val || !parse_feature(val, kind, list)) {
                err.set("feature '%s' has no readable value", is_id ? "id" : "labels");
                return LPM_ERR_DATA;
            }
            if (is_id) {
                id_present = true;
                id_ok = kind == KIND_BYTES && bytes_list(list, id) > 0 && utf8_ok(id);
                if (kind != KIND_BYTES && !feature_parses(val)) {
                    err.set("feature 'id' has no readable value");
                    return LPM_ERR_DATA;
                }
            } else {
                labels.n = labels_mark;
                if (!collect_labels(kind, list, sel.num_classes, labels)) {
                    err.set("feature 'labels' is not a list of class indices");
                    return LPM_ERR_DATA;
                }
            }
        }
    }
    if (id_present && !id_ok) {
        err.set("feature 'id' is not a UTF-8 bytes value");
        return LPM_ERR_DATA;
    }
    for (int j = 0; j < sel.num_features; ++j) {
        if (state[j] == FEAT_MISSING || state[j] == FEAT_NO_VALUE) {
            err.set("feature '%s' is missing", sel.names[j]);
            return LPM_ERR_DATA;
        }
        if (state[j] == FEAT_NOT_FLOAT) {
            err.set("feature '%s' is not a float list", sel.names[j]);
            return LPM_ERR_DATA;
        }
        if (count[j] != sel.sizes[j]) {
            err.set("feature '%s' has %lld values, expected %d", sel.names[j], (long long)count[j], sel.sizes[j]);
            return LPM_ERR_DATA;
        }
    }
    *id_offset = id_present ? (int64_t)(id.p - buf) : 0;
    *id_length = id_present ? (int32_t)id.size() : 0;
    return LPM_OK;
}

// All Example records of a buffer: locate_records' arguments and outputs, with feature_offset int64 / feature_stride int32
// [num_records, num_features] (see above) in place of the frame tables; sel.max_frames is not looked at.
inline int locate_example_records(const uint8_t* buf, int64_t nbytes, const int64_t* rec_offset, const int64_t* rec_length, int num_records,
                                  int64_t record_base, const Selection& sel, int64_t* feature_offset, int32_t* feature_stride,
                                  int32_t* label_start, int32_t* label_index, int64_t label_capacity, int64_t* labels_needed,
                                  int64_t* id_offset, int32_t* id_length, int* failed_record, const Err& err) {
    uint8_t canon[MAX_FEATURES][CANON_MAX];
    size_t canon_n[MAX_FEATURES];
    for (int j = 0; j < sel.num_features; ++j) canon_n[j] = canonical_float_header(sel.sizes[j], canon[j]);
    return locate_each(buf, nbytes, rec_offset, rec_length, num_records, record_base, label_start, label_index, label_capacity, labels_needed,
                       failed_record, err, [&](int i, Span rec, LabelSink& sink, char* why, size_t why_n) {
                           return locate_example(buf, rec, sel, canon, canon_n, feature_offset + (int64_t)i * sel.num_features,
                                                 feature_stride + (int64_t)i * sel.num_features, sink, id_offset + i, id_length + i, why,
                                                 why_n);
                       });
}

}  // namespace lpm_index
