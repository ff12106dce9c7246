"""The hand-built chunk streams (tests/chunk_streams.py) on the CPU: every fixture decodes to its plain bytes with the byte-at-a-time decoder,
with libsnappy / liblz4 (pyarrow) and with the oracle's po_chunk_decompress; the fixtures hold every element the list below names; and the
forward index `chunk_blob` writes around them is one the oracle's reader loads.  The GPU decoder reads the same fixtures in
tests/test_gpu_chunk_streams.py."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

from pinot_amd import capi, formats
from pinot_amd.executor import NativeSegment
from pinot_amd.segment import HostColumn, HostSegment
from tests import chunk_streams as cs

CODECS = [cs.SNAPPY, cs.LZ4, cs.LZ4_LENGTH_PREFIXED]
RUNS = [("run", offset, total) for offset in (1, 2, 3, 5, 6, 7, 63, 64, 65) for total in (63, 65, 127, 129)]   # both sides of 64 and of 128

# What the fixtures must contain, as stream_elements keys.  A snappy copy holds at most 64 bytes, so offsets 64 and 65 overlap only in LZ4;
# an LZ4 match cannot reach the last byte of a block (the last 5 bytes are literals, the last match starts 12 bytes before the end: liblz4
# rejects a block that breaks either), so "ends on the last byte" is ('ends_in_copy', 0) for snappy and ('ends_in_copy', 5) for LZ4, and the
# largest offset is 65535 in a snappy chunk of 65536 bytes and 65524 in an LZ4 one.
REQUIRED = {
    cs.SNAPPY: [
        # literals: (form = extra length bytes, length)
        ("literal", 0, 1), ("literal", 0, 60), ("literal", 1, 61), ("literal", 1, 256), ("literal", 2, 257), ("literal", 2, cs.SMALL),
        ("literal", 3, 61), ("literal", 4, 61), ("literal", 3, 257), ("literal", 4, 257),
        # copies: (kind, offset, length)
        *[("copy", 1, offset, n) for offset in (1, 255, 256, 2047) for n in (4, 11)],
        *[("copy", 2, offset, n) for offset in (1, 2048) for n in (1, 64)],
        ("copy", 2, 65535, 1), ("copy", 2, 65536 - 64, 64),
        ("copy", 3, 1, 9), ("copy", 3, 3, 64), ("copy", 3, 32768, 64), ("copy", 3, 32769, 1), ("copy", 3, 40000, 33), ("copy", 3, 65536 - 64, 64),
        *[("overlap", offset) for offset in (1, 2, 3, 5, 6, 7, 63)], *RUNS,
        ("ends_in_copy", 0), ("literal_then_copies",),
    ],
    cs.LZ4: [
        *[("literal", n) for n in (0, 14, 15, 15 + 254, 15 + 255, 15 + 2 * 255 + 77)],
        ("literal_chain", 1, True), ("literal_chain", 1, False), ("literal_chain", 2, True), ("literal_chain", 3, False),
        ("match", 14, 4), ("match", 2, 18), ("match", 7, 19), ("match", 100, 19 + 254), ("match", 300, 19 + 255),
        ("match_chain", 1, True), ("match_chain", 1, False), ("match_chain", 2, True),
        *[("copy_offset", offset) for offset in (1, 4095, 4096, 65536 - 12)],
        *[("overlap", offset) for offset in (1, 2, 3, 5, 6, 7, 63, 64, 65)], *RUNS,
        ("ends_in_copy", 5), ("literal_then_copies",),
    ],
}
REQUIRED[cs.LZ4_LENGTH_PREFIXED] = REQUIRED[cs.LZ4]


def _library(stream, codec, n):
    import pyarrow as pa
    if codec == cs.SNAPPY:
        return pa.decompress(stream, decompressed_size=n, codec="snappy", asbytes=True)
    return pa.decompress(stream[4:] if codec == cs.LZ4_LENGTH_PREFIXED else stream, decompressed_size=n, codec="lz4_raw", asbytes=True)


def _oracle(oracle_api, stream, codec, cap):
    fn = oracle_api.lib.po_chunk_decompress
    fn.restype = C.c_int64
    fn.argtypes = [C.c_int32, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64]
    dst = C.create_string_buffer(cap + 16)
    got = fn(codec, stream, len(stream), dst, cap)
    return None if got < 0 else dst.raw[:got]


def test_the_constants_are_the_projects():
    assert (cs.SNAPPY, cs.LZ4, cs.LZ4_LENGTH_PREFIXED) == (formats.CHUNK_COMPRESSION_SNAPPY, formats.CHUNK_COMPRESSION_LZ4,
                                                            formats.CHUNK_COMPRESSION_LZ4_LENGTH_PREFIXED)


@pytest.mark.parametrize("codec", CODECS)
def test_every_decoder_gives_the_plain_bytes(oracle_api, codec):
    """plain decoder == libsnappy / liblz4 == po_chunk_decompress == the bytes the plan was executed to, for every fixture"""
    fixtures = cs.fixtures_for(codec)
    assert len(fixtures) >= 150
    for fx in fixtures:
        stream = cs.fixture_stream(fx, codec)
        n = len(fx.plain)
        assert len(stream) <= cs.staging_bytes(n), fx.name
        assert cs.decode(stream, codec, n) == fx.plain, fx.name
        assert _library(stream, codec, n) == fx.plain, fx.name
        assert _oracle(oracle_api, stream, codec, n) == fx.plain, fx.name


@pytest.mark.parametrize("codec", CODECS)
def test_the_fixtures_hold_every_listed_element(codec):
    have = Counter()
    for fx in cs.fixtures_for(codec):
        have += cs.stream_elements(cs.fixture_stream(fx, codec), codec)
    missing = [key for key in REQUIRED[codec] if have[key] < 1]
    assert not missing, missing
    # the random part: chosen forms and kinds, not only the shortest
    if codec == cs.SNAPPY:
        assert all(have[("literal_form", f)] >= 100 for f in range(5)) and all(have[("copy_kind", k)] >= 50 for k in (1, 2, 3))


@pytest.mark.parametrize("codec", CODECS)
def test_padding_to_the_packed_chunk_sizes_keeps_the_elements(codec):
    """The GPU test loads the fixtures padded to chunks of SMALL or LARGE bytes: every fixture fits one of the two, and the padded streams
    still hold the list (the fixtures that end in a copy are full chunks: a literal behind them would take that away)."""
    have = Counter()
    for fx in cs.fixtures_for(codec):
        size = cs.SMALL if len(fx.plain) <= cs.SMALL else cs.LARGE
        p = cs.padded(fx, size)
        assert len(p.plain) == size and p.plain[:len(fx.plain)] == fx.plain
        stream = cs.fixture_stream(p, codec)
        assert len(stream) <= cs.staging_bytes(size)
        assert _library(stream, codec, size) == p.plain, fx.name
        have += cs.stream_elements(stream, codec)
    missing = [key for key in REQUIRED[codec] if have[key] < 1]
    assert not missing, missing


def test_the_builders_refuse_plans_that_do_not_give_the_plain_bytes():
    plain = bytes(range(40)) + bytes(range(40))
    assert cs.snappy_decode(cs.snappy_stream([("L", 40), ("C", 40, 40)], plain)) == plain
    with pytest.raises(AssertionError):
        cs.snappy_stream([("L", 40), ("C", 39, 40)], plain)          # the copy gives other bytes
    with pytest.raises(AssertionError):
        cs.snappy_stream([("L", 40), ("C", 40, 39)], plain)          # one byte is not covered
    with pytest.raises(AssertionError):
        cs.snappy_stream([("L", 40), ("C", 41, 40)], plain)          # before the start of the chunk
    with pytest.raises(AssertionError):
        cs.snappy_stream([("L", 1)] * 80, plain, literal_form=4)     # 6 stream bytes per byte: larger than the staging area
    assert cs.lz4_decode(cs.lz4_stream([(40, 40, 28), (12, 0, 0)], plain), 80) == plain
    with pytest.raises(AssertionError):
        cs.lz4_stream([(40, 39, 28), (12, 0, 0)], plain)
    with pytest.raises(AssertionError):
        cs.lz4_stream([(40, 40, 28), (11, 0, 0)], plain)
    with pytest.raises(AssertionError):
        cs.lz4_stream([(40, 40, 36), (4, 0, 0)], plain)              # the last 5 bytes are literals
    with pytest.raises(AssertionError):
        cs.lz4_stream([(40, 40, 40)], plain)                         # the last sequence has no match


@pytest.mark.parametrize("codec", CODECS)
def test_the_cpu_decoders_refuse_what_the_refusal_tests_write(oracle_api, codec):
    """The wrong streams of test_gpu_chunk_streams.py, on the CPU: the plain decoder refuses each of them, and the oracle's decompressor,
    given the chunk's size as its capacity, returns no chunk of that size"""
    from tests.test_gpu_chunk_streams import wrong_chunks
    (plain, stream), wrong = wrong_chunks(codec)
    assert cs.decode(stream, codec, len(plain)) == plain
    assert len(wrong) >= 7 and len({what for what, _ in wrong}) == len(wrong)
    for what, bad in wrong:
        assert len(bad) <= cs.staging_bytes(len(plain)), what
        with pytest.raises(ValueError):
            cs.decode(bad, codec, len(plain))
        got = _oracle(oracle_api, bad, codec, len(plain))
        assert got is None or len(got) != len(plain), what


@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("version", [2, 3])
def test_the_oracle_loads_the_blob_around_the_fixtures(oracle_api, codec, version):
    """chunk_blob writes the layout of formats.write_raw_fixed_byte_chunk: the oracle's reader takes the padded fixtures as one INT column"""
    fixtures = [cs.padded(fx, cs.SMALL) for fx in cs.fixtures_for(codec) if len(fx.plain) <= cs.SMALL][:39]
    tail_plain, tail_stream = cs.random_chunk(codec, cs.SMALL - 12, 0)   # the last chunk is three values short
    plain = b"".join(fx.plain for fx in fixtures) + tail_plain
    num_docs = len(plain) // 4
    streams = [cs.fixture_stream(fx, codec) for fx in fixtures] + [tail_stream]
    exp = np.frombuffer(plain, ">i4").astype(np.int64)
    blob = np.frombuffer(cs.chunk_blob(streams, cs.SMALL // 4, 4, num_docs, codec, version), dtype=np.uint8)
    values = exp.astype(np.int32)
    theirs = formats.write_raw_fixed_byte_chunk(values, "INT", version=version, docs_per_chunk=cs.SMALL // 4, compression=codec)
    head = 28 + len(streams) * (4 if version == 2 else 8)
    assert bytes(blob[:28]) == bytes(theirs[:28]) and bytes(blob[28:32]) == bytes(theirs[28:32]) and len(theirs) > head
    col = HostColumn("x", "INT", capi.FWD_RAW_FIXED_BYTE_CHUNK, False, 0, 0, False, 0, blob)
    seg = NativeSegment(oracle_api, HostSegment("c", num_docs, {"x": col}))
    assert seg.execute("SELECT COUNT(*), MIN(x), MAX(x), SUM(x) FROM t").aggregation_result() == [num_docs, float(exp.min()), float(exp.max()),
                                                                                                   float(exp.sum())]
    probe = int(exp[num_docs // 2])
    np.testing.assert_array_equal(seg.filter(f"SELECT COUNT(*) FROM t WHERE x = {probe}").doc_ids(), np.flatnonzero(exp == probe))
    seg.destroy()


def library_tally(codec, n):
    """What libsnappy / liblz4 write for the seeded columns of tests/test_compressed_chunks.py, and the plain decoder on those streams"""
    from tests.test_compressed_chunks import seeded_columns
    have = Counter()
    for name, (vals, dt) in seeded_columns(n).items():
        version, dpc = (3, 777) if name in ("l_step", "f_few") else (2, 1000)
        data = np.ascontiguousarray(vals).astype(formats._BE_DTYPES[dt]).tobytes()
        step = dpc * formats._WIDTHS[dt]
        for i in range(0, len(data), step):
            stream = formats.compress_chunk(data[i:i + step], codec)
            have += cs.stream_elements(stream, codec)
            if i < 3 * step:
                assert cs.decode(stream, codec, len(data[i:i + step])) == data[i:i + step], (name, i)
    return have


@pytest.mark.parametrize("codec", [cs.SNAPPY, cs.LZ4])
def test_what_the_libraries_write(codec):
    """Why the fixtures exist.  Every chunk of seeded_columns(300_000), the data of test_gpu_decompressed_columns_match_oracle, compressed by
    libsnappy / liblz4 (pyarrow 25) and parsed with stream_elements.  The counts differ between library versions, so the test prints its
    tally — of 30 000 docs, to stay quick — and asserts only that the plain decoder reads the libraries' streams.

      snappy  376 440 literals: 375 586 with the length in the tag, 554 with 1 and 300 with 2 length bytes, none with 3 or 4.
              667 405 copies: 385 954 of kind 1, 281 451 of kind 2, none of kind 3 (the 4-byte offset).
              Overlapping copies by offset: 1: 47 794, 2: 23, 3: 2, 4: 30 374, 8: 1 702, 12: 416, 16: 95, 20: 15, 24: 5, 28: 1, 32: 1;
              offsets 5, 6, 7: never.  Copies of 64 bytes: 33 813, of 63 bytes: 23.
      LZ4     633 937 matches.  Overlapping by offset: 1: 773, 2: 28 055, 4: 17 212, 8: 1 681, 12: 417, 16: 95, 20: 15, 24: 5, 28: 1, 32: 1;
              offsets 3, 5, 6, 7: never.  Matches of 63 / 64 / 65 bytes: 1 / 96 / 1.  Length chains that end in a 0 byte: 7 170 literal
              chains and 15 match chains of one byte, none of two or more (255, 0).

    The fixtures (188 snappy chunks, 184 LZ4 chunks): every literal form 170 to 317 times, copy kinds 1 / 2 / 3 99 / 2 409 / 2 196 times, every
    overlapping offset from 1 to 63 at least 10 times (snappy) and 4 times (LZ4), and the elements of REQUIRED."""
    have = library_tally(codec, 30_000)
    print(sorted(cs.tally(have, codec).items(), key=str))
