"""pg_decompress.hip byte for byte.  Raw columns are built from hand-written SNAPPY / LZ4 / LZ4_LENGTH_PREFIXED streams (tests/chunk_streams.py),
loaded, and read back with `SELECT x FROM t LIMIT <all>`: without filter or ORDER BY that gathers the column in docId order and runs no kernel
over the values, so the rows are what the decompressor wrote to HBM.  They must equal, element for element and with no tolerance, the plain
bytes the streams were built from (np.frombuffer(plain, ">i4") — nothing the GPU path produced).  INT and LONG columns of random bytes: every
bit pattern is a value of its own, so a swapped, shifted or wrong byte anywhere shows.

Launch shapes.  decompress_fixed_byte_chunks puts min(4, 65536 / per_wave) chunks (at least 1) into a block, one wavefront each, where
per_wave = align16(chunk_bytes) + align16(chunk_bytes + chunk_bytes / 6 + 64) bytes of LDS:
    3108 B:   3120 +  3696 =   6816 -> 9 -> 4 waves        4000 B:  4000 +  4736 =  8736 -> 7 -> 4 waves      4096 B: 4096 + 4848 = 8944 -> 4 waves
    8000 B:   8000 +  9408 =  17408 -> 3 waves            12000 B: 12000 + 14064 = 26064 -> 2 waves
   16384 B:  16384 + 19184 =  35568 -> 1 wave             65536 B: 65536 + 76528 = 142064 -> 0 -> 1 wave, the largest chunk and the one launch
                                                                    that needs more dynamic LDS than the default limit
The tests cannot see the launch shape and do not try to: SHAPES is chosen so that each of these runs, with doc counts that leave the last
block short of chunks and the last chunk short of values (down to one value)."""
import functools
import random
import struct

import numpy as np
import pytest

from pinot_amd import capi
from pinot_amd.executor import NativeSegment
from pinot_amd.segment import HostColumn, HostSegment
from tests import chunk_streams as cs

CODECS = [cs.SNAPPY, cs.LZ4, cs.LZ4_LENGTH_PREFIXED]
WIDTH = {"INT": 4, "LONG": 8, "DOUBLE": 8}
# (data type, forward index version, docs per chunk, docs)
SHAPES = [
    ("INT", 3, 777, 5 * 777 - 1),       # 3108 B, no multiple of 16; five chunks in blocks of four; the last chunk is one value short
    ("LONG", 2, 1000, 4000),            # 8000 B, three chunks to a block; the last chunk is full
    ("LONG", 2, 1000, 3001),            # ... the last chunk is one value, 8 bytes
    ("INT", 3, 3000, 3 * 3000 + 1),     # 12000 B, two chunks to a block; the last chunk is 4 bytes
    ("INT", 2, 4096, 3 * 4096 - 5),     # 16384 B, one chunk to a block
    ("LONG", 3, 8192, 2 * 8192 + 3),    # 65536 B, the maximum
    ("INT", 2, 16384, 16384 + 1),       # 65536 B
    ("INT", 3, 1000, 1),                # one chunk of one value
    ("INT", 2, 1000, 999),              # one chunk, fewer docs than a chunk
]
FINITE = list(range(1, 0x7F))   # bytes for a DOUBLE column: no first byte 0x7F / 0xFF, so no exponent of all ones (NaN, infinity), and no zero


@functools.lru_cache(maxsize=None)
def _chunks(family, chunk_bytes, total_bytes, finite=False):
    """[(plain, snappy or LZ4 stream)] of a column: random plans sized to each chunk, the last one to what is left of the column"""
    sizes = [min(chunk_bytes, total_bytes - at) for at in range(0, total_bytes, chunk_bytes)]
    return [cs.random_chunk(family, size, i, tuple(FINITE) if finite else None) for i, size in enumerate(sizes)]


def _column(codec, dt, version, dpc, num_docs, finite=False):
    """(plain bytes of the column, its forward index)"""
    family = cs.SNAPPY if codec == cs.SNAPPY else cs.LZ4
    chunks = _chunks(family, dpc * WIDTH[dt], num_docs * WIDTH[dt], finite)
    streams = [cs.lz4_length_prefixed(s, len(p)) if codec == cs.LZ4_LENGTH_PREFIXED else s for p, s in chunks]
    return b"".join(p for p, _ in chunks), cs.chunk_blob(streams, dpc, WIDTH[dt], num_docs, codec, version)


def _load(api, blob, dt, num_docs):
    col = HostColumn("x", dt, capi.FWD_RAW_FIXED_BYTE_CHUNK, False, 0, 0, False, 0, np.frombuffer(blob, dtype=np.uint8))
    return NativeSegment(api, HostSegment("streams", num_docs, {"x": col}))


def _read_back(seg, num_docs):
    rb = seg.execute(f"SELECT x FROM t LIMIT {num_docs}")
    rows = rb.selection_rows
    assert rb.key_columns == ["x"] and len(rows) == num_docs and rb.stats.num_docs_scanned == num_docs
    return [r[0] for r in rows]


def _check_column(seg, plain, dt, num_docs):
    assert len(plain) == num_docs * WIDTH[dt]
    got = _read_back(seg, num_docs)
    if dt == "DOUBLE":   # through the bit pattern
        exp = np.frombuffer(plain, ">u8").astype(np.uint64)
        got = np.array(got, dtype=np.float64).view(np.uint64)
        values = np.frombuffer(plain, ">f8").astype(np.float64)
        assert np.isfinite(values).all()
    else:
        exp = values = np.frombuffer(plain, ">i4" if dt == "INT" else ">i8").astype(np.int64)
        got = np.array(got, dtype=np.int64)
    wrong = np.flatnonzero(got != exp)
    assert wrong.size == 0, f"{wrong.size} of {num_docs} values differ, the first at doc {wrong[0]}: {got[wrong[0]]:#x}, expected {exp[wrong[0]]:#x}"
    # what the query kernels see of the same column
    agg = seg.execute("SELECT COUNT(*), MIN(x), MAX(x) FROM t").aggregation_result()
    assert agg == [num_docs, float(values.min()), float(values.max())]


@pytest.mark.gpu
@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("dt,version,dpc,num_docs", SHAPES)
def test_gpu_reads_back_every_byte(gpu_api, codec, dt, version, dpc, num_docs):
    plain, blob = _column(codec, dt, version, dpc, num_docs)
    seg = _load(gpu_api, blob, dt, num_docs)
    try:
        _check_column(seg, plain, dt, num_docs)
    finally:
        seg.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("codec", CODECS)
def test_gpu_reads_back_a_double_column(gpu_api, codec):
    plain, blob = _column(codec, "DOUBLE", 3, 1000, 2077, finite=True)
    seg = _load(gpu_api, blob, "DOUBLE", 2077)
    try:
        _check_column(seg, plain, "DOUBLE", 2077)
    finally:
        seg.destroy()


def _packed(codec, size):
    """Every fixture of at most `size` bytes (and more than the smaller size), padded by a literal to a chunk of `size` bytes"""
    fixtures = [cs.padded(fx, size) for fx in cs.fixtures_for(codec) if (len(fx.plain) <= cs.SMALL) == (size == cs.SMALL)]
    streams = [cs.fixture_stream(fx, codec) for fx in fixtures]
    plain = b"".join(fx.plain for fx in fixtures)
    return plain, cs.chunk_blob(streams, size // 4, 4, len(plain) // 4, codec, 3 if size == cs.SMALL else 2), len(fixtures)


@pytest.mark.gpu
@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("size", [cs.SMALL, cs.LARGE])
def test_gpu_decodes_every_fixture(gpu_api, codec, size):
    """All of FIXTURES in two INT columns: the chunks of up to 4096 bytes as 1024 docs per chunk (four waves to a block), the few that
    need long offsets as 16384 docs per chunk.  tests/test_chunk_streams.py asserts that the padded streams hold every listed element."""
    plain, blob, n_chunks = _packed(codec, size)
    assert n_chunks >= (150 if size == cs.SMALL else 3)
    seg = _load(gpu_api, blob, "INT", len(plain) // 4)
    try:
        _check_column(seg, plain, "INT", len(plain) // 4)
    finally:
        seg.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("codec", CODECS)
def test_gpu_loads_the_same_blob_twice(gpu_api, codec):
    dt, version, dpc, num_docs = SHAPES[0]
    plain, blob = _column(codec, dt, version, dpc, num_docs)
    rows = []
    for _ in range(2):
        seg = _load(gpu_api, blob, dt, num_docs)
        try:
            rows.append(_read_back(seg, num_docs))
        finally:
            seg.destroy()
    assert rows[0] == rows[1] == np.frombuffer(plain, ">i4").tolist()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
CHUNK = 4000   # 1000 INT docs


def wrong_chunks(codec):
    """((plain, stream) of a 4000-byte chunk, [(what is wrong, stream)]): streams the decoder has an explicit check for — a wrong length in
    front, an output that comes out short, a copy from before the chunk, an element that runs past the chunk's end.  Each stays inside the
    staging area, and what a missing check would get wrong is bytes inside the wave's own LDS window."""
    def rng():
        return random.Random("refusals")
    plan = [("L", 1000), ("C", 500, 2000), ("L", 1000)]
    plain = cs.execute_plan(plan, rng())
    ext = plain + bytes(8)                                              # bytes for a last literal that is too long
    copy_ext = {k: cs.execute_plan([("L", 1000), ("C", 500, 3000 + k)], rng()) for k in (1, 8)}   # a last copy that is too long
    wrong = []
    if codec == cs.SNAPPY:
        ops = cs.snappy_ops(plan)
        good = cs.snappy_stream(ops, plain)
        wrong += [("preamble one more", cs.snappy_stream(ops, plain, length=CHUNK + 1)),
                  ("preamble one less", cs.snappy_stream(ops, plain, length=CHUNK - 1)),
                  ("stops one element early", cs.snappy_stream(ops[:-1], plain, check=False)),
                  ("copy offset 0", cs.snappy_stream([ops[0], ("C", 0, 64, 2)] + ops[2:], plain, check=False)),
                  ("copy offset one more than written", cs.snappy_stream([ops[0], ("C", 1001, 64)] + ops[2:], plain, check=False))]
        for k in (1, 8):
            wrong.append((f"last literal {k} past the chunk", cs.snappy_stream(ops[:-1] + [("L", 1000 + k)], ext[:CHUNK + k], length=CHUNK, check=False)))
            wrong.append((f"last copy {k} past the chunk", cs.snappy_stream(cs.snappy_ops([("L", 1000), ("C", 500, 3000 + k)]), copy_ext[k], length=CHUNK)))
        return (plain, good), wrong
    seqs = cs.lz4_seqs(plan, CHUNK)
    assert seqs == [(1000, 500, 2000), (1000, 0, 0)]
    blocks = [("stops one element early", cs.lz4_stream(seqs[:-1], plain, check=False)),
              ("copy offset 0", cs.lz4_stream([(1000, 0, 2000), seqs[1]], plain, check=False)),
              ("copy offset one more than written", cs.lz4_stream([(1000, 1001, 2000), seqs[1]], plain, check=False))]
    for k in (1, 8):
        blocks.append((f"last literal {k} past the chunk", cs.lz4_stream([seqs[0], (1000 + k, 0, 0)], ext[:CHUNK + k], size=CHUNK, check=False)))
        blocks.append((f"last copy {k} past the chunk", cs.lz4_stream([(1000, 500, 3000 + k)], copy_ext[k], size=CHUNK, check=False)))
    good = cs.lz4_stream(seqs, plain)
    if codec == cs.LZ4:
        return (plain, good), blocks
    wrong = [("prefix one more", struct.pack("<i", CHUNK + 1) + good), ("prefix one less", struct.pack("<i", CHUNK - 1) + good)]
    return (plain, cs.lz4_length_prefixed(good, CHUNK)), wrong + [(what, cs.lz4_length_prefixed(b, CHUNK)) for what, b in blocks]


@pytest.mark.gpu
@pytest.mark.parametrize("codec", CODECS)
def test_gpu_refuses_a_wrong_chunk_and_names_it(gpu_api, codec):
    """Four chunks, chunk 2 alone is wrong: the load fails and says which chunk of which column; the unbroken column then loads in the
    same process and reads back exactly."""
    (plain2, good), wrong = wrong_chunks(codec)
    others = [cs.random_chunk(codec, CHUNK, 100 + i) for i in range(3)]

    def blob(chunk2):
        return cs.chunk_blob([others[0][1], others[1][1], chunk2, others[2][1]], CHUNK // 4, 4, CHUNK, codec, 2)
    for what, stream in wrong:
        assert len(stream) <= cs.staging_bytes(CHUNK), what
        with pytest.raises(capi.NativeError) as e:
            _load(gpu_api, blob(stream), "INT", CHUNK)
        assert e.value.status == capi.PG_ERR_INVALID_ARGUMENT and "chunk 2 " in e.value.message and "column x:" in e.value.message, (what, e.value.message)
    seg = _load(gpu_api, blob(good), "INT", CHUNK)
    try:
        _check_column(seg, others[0][0] + others[1][0] + plain2 + others[2][0], "INT", CHUNK)
    finally:
        seg.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("codec", CODECS)
def test_gpu_refuses_chunks_above_the_maximum(gpu_api, codec):
    """16385 INT docs per chunk are 65540 bytes: refused by the host, before any launch"""
    plain, stream = cs.random_chunk(codec, 65540, 0)
    with pytest.raises(capi.NativeError) as e:
        _load(gpu_api, cs.chunk_blob([stream], 16385, 4, 16385, codec, 2), "INT", 16385)
    assert e.value.status == capi.PG_ERR_UNSUPPORTED and "column x:" in e.value.message and "65540" in e.value.message, e.value.message
