"""tf.train.Example built with the protobuf runtime from its public definition (feature.proto / example.proto): the independent
encoder and decoder of the video-level reader's tests, as tests/test_readers.py builds SequenceExample."""
import struct

from learnablepoolingmethods_amd import readers


def example_class():
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
    fd = descriptor_pb2.FileDescriptorProto(name="lpm_test_video_level_example.proto", package="lpmtfe", syntax="proto3")
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
    field(feat, "bytes_list", 1, T.TYPE_MESSAGE, type_name=".lpmtfe.BytesList", oneof=0)
    field(feat, "float_list", 2, T.TYPE_MESSAGE, type_name=".lpmtfe.FloatList", oneof=0)
    field(feat, "int64_list", 3, T.TYPE_MESSAGE, type_name=".lpmtfe.Int64List", oneof=0)
    feats = msg("Features")
    e = feats.nested_type.add(name="FeatureEntry")
    e.options.map_entry = True
    field(e, "key", 1, T.TYPE_STRING)
    field(e, "value", 2, T.TYPE_MESSAGE, type_name=".lpmtfe.Feature")
    field(feats, "feature", 1, T.TYPE_MESSAGE, T.LABEL_REPEATED, type_name=".lpmtfe.Features.FeatureEntry")
    field(msg("Example"), "features", 1, T.TYPE_MESSAGE, type_name=".lpmtfe.Features")
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    return message_factory.GetMessageClass(pool.FindMessageTypeByName("lpmtfe.Example"))


def framed(records) -> bytes:
    """The bytes write_tfrecord writes."""
    out = bytearray()
    for data in records:
        head = struct.pack("<Q", len(data))
        out += head + struct.pack("<I", readers.masked_crc32c(head)) + data + struct.pack("<I", readers.masked_crc32c(data))
    return bytes(out)
