"""Hand-built SNAPPY / LZ4 chunk streams for the decompressor tests: encoders that write exactly the elements a test asks for (libsnappy and
liblz4 never choose most of them), byte-at-a-time decoders written from the format descriptions (snappy format_description.txt, LZ4 block
format), the forward-index blob around already-compressed chunks, a counter of what a stream contains, and FIXTURES — a seeded set of
chunks built by executing operation plans, so that the plain bytes repeat exactly where a copy says so and are random elsewhere.
Plain Python: no pyarrow, no project code.

LZ4 end of block (block format, "End of block restrictions"): the last sequence is literals only, the last 5 bytes are literals and the last
match starts at least 12 bytes before the end.  liblz4 enforces all three when it decodes, so `lz4_stream` asserts them; the nearest thing
to "a copy that ends on the last byte of the chunk" an LZ4 stream can hold is a match that ends 5 bytes before it."""
import random
import struct
from collections import Counter, namedtuple

SNAPPY, LZ4, LZ4_LENGTH_PREFIXED = 1, 3, 4   # ChunkCompressionType values
LZ4_LAST_LITERALS, LZ4_MFLIMIT = 5, 12


def staging_bytes(chunk_bytes):
    """The decoder's staging area for one compressed chunk: align16(chunk_bytes + chunk_bytes / 6 + 64)."""
    return (chunk_bytes + chunk_bytes // 6 + 64 + 15) & ~15


def _varint(n):
    out = bytearray()
    while n >= 0x80:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def _check_copy(plain, pos, offset, n):
    assert 1 <= offset <= pos, f"copy at {pos}: offset {offset} reaches before the chunk"
    assert pos + n <= len(plain), f"copy at {pos}: {n} bytes run past the chunk"
    for i in range(pos, pos + n):
        assert plain[i] == plain[i - offset], f"copy at {pos} (offset {offset}, {n} bytes) does not reproduce byte {i}"


# ---- snappy ------------------------------------------------------------------------------------------------------------------------------
def _min_literal_form(n):
    if n <= 60:
        return 0
    return (((n - 1).bit_length() + 7) // 8)


def _min_copy_kind(offset, n):
    return 1 if (4 <= n <= 11 and offset < 2048) else (2 if offset < 65536 else 3)


def snappy_stream(ops, plain, literal_form=None, copy_kind=None, length=None, check=True):
    """The snappy stream of `plain` written as `ops`: ('L', n[, form]) is a literal of the next n bytes, form 0 = length in the tag (n <= 60),
    1..4 = that many extra length bytes (non-minimal forms are legal); ('C', offset, n[, kind]) is a copy of n bytes (kind 1: 4..11 bytes,
    offset < 2048; kind 2: 1..64 bytes, offset < 65536; kind 3: 1..64 bytes, a 4-byte offset).  An op without form / kind takes
    `literal_form` / `copy_kind`, else the shortest.  Asserts that every copy reproduces the bytes of `plain` it stands for, that the ops
    cover `plain` exactly and that the stream fits the decoder's staging area.  The refusal tests write streams that are wrong on purpose:
    `length` is the preamble's value when it is not len(plain), and check=False leaves the copies and the cover unchecked (a literal still
    takes its bytes from `plain`; the staging area always holds)."""
    out = bytearray(_varint(len(plain) if length is None else length))
    pos = 0
    for op in ops:
        if op[0] == "L":
            n = op[1]
            form = op[2] if len(op) > 2 else (literal_form if literal_form is not None else _min_literal_form(n))
            assert n >= 1 and pos + n <= len(plain), f"literal at {pos}: {n} bytes"
            if form == 0:
                assert n <= 60
                out.append((n - 1) << 2)
            else:
                assert 1 <= form <= 4 and n - 1 < (1 << (8 * form)), f"literal of {n} bytes in {form} length bytes"
                out.append((59 + form) << 2)
                out += (n - 1).to_bytes(form, "little")
            out += plain[pos:pos + n]
        else:
            _, offset, n = op[:3]
            kind = op[3] if len(op) > 3 else (copy_kind if copy_kind is not None else _min_copy_kind(offset, n))
            if check:
                _check_copy(plain, pos, offset, n)
            if kind == 1:
                assert 4 <= n <= 11 and offset < 2048
                out.append(1 | ((n - 4) << 2) | ((offset >> 8) << 5))
                out.append(offset & 0xFF)
            else:
                assert kind in (2, 3) and 1 <= n <= 64 and offset < (1 << (16 if kind == 2 else 32))
                out.append(kind | ((n - 1) << 2))
                out += offset.to_bytes(2 if kind == 2 else 4, "little")
        pos += n
    assert not check or pos == len(plain), f"the ops cover {pos} of {len(plain)} bytes"
    assert len(out) <= staging_bytes(len(plain) if length is None else length), f"{len(out)}-byte stream for a {len(plain)}-byte chunk"
    return bytes(out)


def _snappy_elements(stream):
    """(preamble value, [('L', form, n, data position) | ('C', kind, offset, n)]) — the parse both the decoder and the counter use"""
    want = shift = ip = 0
    while True:
        b = stream[ip]
        ip += 1
        want |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            break
    els = []
    while ip < len(stream):
        tag = stream[ip]
        ip += 1
        kind = tag & 3
        if kind == 0:
            n = (tag >> 2) + 1
            form = 0
            if n > 60:
                form = n - 60
                n = 0
                for k in range(form):
                    n |= stream[ip + k] << (8 * k)
                n += 1
                ip += form
            if ip + n > len(stream):
                raise ValueError("literal runs past the stream")
            els.append(("L", form, n, ip))
            ip += n
        elif kind == 1:
            els.append(("C", 1, ((tag >> 5) << 8) | stream[ip], ((tag >> 2) & 7) + 4))
            ip += 1
        elif kind == 2:
            els.append(("C", 2, stream[ip] | (stream[ip + 1] << 8), (tag >> 2) + 1))
            ip += 2
        else:
            els.append(("C", 3, stream[ip] | (stream[ip + 1] << 8) | (stream[ip + 2] << 16) | (stream[ip + 3] << 24), (tag >> 2) + 1))
            ip += 4
    return want, els


def snappy_decode(stream):
    """Byte-at-a-time snappy decoder (format_description.txt); raises ValueError on a stream that is not one."""
    try:
        want, els = _snappy_elements(stream)
    except IndexError:
        raise ValueError("the stream ends inside an element")
    out = bytearray()
    for el in els:
        if el[0] == "L":
            for i in range(el[2]):
                out.append(stream[el[3] + i])
        else:
            _, _, offset, n = el
            if offset == 0 or offset > len(out):
                raise ValueError(f"copy offset {offset} with {len(out)} bytes written")
            for _ in range(n):
                out.append(out[len(out) - offset])
        if len(out) > want:
            raise ValueError("more bytes than the preamble says")
    if len(out) != want:
        raise ValueError(f"{len(out)} bytes, the preamble says {want}")
    return bytes(out)


# ---- LZ4 ---------------------------------------------------------------------------------------------------------------------------------
def _lz4_chain(n):
    out = bytearray()
    n -= 15
    while n >= 255:
        out.append(255)
        n -= 255
    out.append(n)   # a length of exactly 15 + 255 k ends its chain in a 0 byte
    return out


def lz4_stream(seqs, plain, size=None, check=True):
    """The LZ4 block of `plain` written as (literal_len, offset, match_len) sequences; the last one is (literal_len, 0, 0).  Lengths of 15 /
    19 and more take 255-chains.  Asserts as `snappy_stream` does, and the end-of-block restrictions.  For the refusal tests: `size` is the
    chunk the stream has to fit when it is not len(plain), check=False leaves the matches, the cover and the end of block unchecked and
    writes a last sequence that has a match (offset != 0 or match_len != 0) in full."""
    assert not check or (seqs and seqs[-1][1] == 0 and seqs[-1][2] == 0), "the last sequence holds literals only"
    out = bytearray()
    pos = 0
    for k, (lit, offset, mlen) in enumerate(seqs):
        last = k == len(seqs) - 1 and offset == 0 and mlen == 0
        assert last or mlen >= 4, "a match has at least 4 bytes"
        assert lit >= 0 and pos + lit <= len(plain), f"literal at {pos}: {lit} bytes"
        out.append((min(lit, 15) << 4) | (0 if last else min(mlen - 4, 15)))
        if lit >= 15:
            out += _lz4_chain(lit)
        out += plain[pos:pos + lit]
        pos += lit
        if last:
            break
        assert offset < 65536
        if check:
            _check_copy(plain, pos, offset, mlen)
            assert pos <= len(plain) - LZ4_MFLIMIT and pos + mlen <= len(plain) - LZ4_LAST_LITERALS, f"match at {pos} (+{mlen}) breaks the end of block rules"
        out += offset.to_bytes(2, "little")
        if mlen - 4 >= 15:
            out += _lz4_chain(mlen - 4)
        pos += mlen
    assert not check or pos == len(plain), f"the sequences cover {pos} of {len(plain)} bytes"
    assert len(out) + 4 <= staging_bytes(len(plain) if size is None else size), f"{len(out)}-byte block for a {len(plain)}-byte chunk"
    return bytes(out)


def lz4_length_prefixed(block, n):
    """LZ4_LENGTH_PREFIXED: the decompressed length as a little-endian int, then the block"""
    return struct.pack("<i", n) + block


def _lz4_sequences(stream):
    """[(literal_len, literal position, extra literal length bytes, offset | None, match_len, extra match length bytes, chain ends (lit, match))]"""
    ip = 0
    seqs = []
    while ip < len(stream):
        token = stream[ip]
        ip += 1
        lit, lit_extra, lit_end = token >> 4, 0, None
        if lit == 15:
            while True:
                b = stream[ip]
                ip += 1
                lit += b
                lit_extra += 1
                if b != 255:
                    lit_end = b
                    break
        if ip + lit > len(stream):
            raise ValueError("literals run past the block")
        lit_pos = ip
        ip += lit
        if ip >= len(stream):
            seqs.append((lit, lit_pos, lit_extra, None, 0, 0, (lit_end, None)))
            break
        offset = stream[ip] | (stream[ip + 1] << 8)
        ip += 2
        mlen, m_extra, m_end = token & 15, 0, None
        if mlen == 15:
            while True:
                b = stream[ip]
                ip += 1
                mlen += b
                m_extra += 1
                if b != 255:
                    m_end = b
                    break
        seqs.append((lit, lit_pos, lit_extra, offset, mlen + 4, m_extra, (lit_end, m_end)))
    return seqs


def lz4_decode(stream, n):
    """Byte-at-a-time LZ4 block decoder; `n` is the decompressed length the block must give.  Raises ValueError otherwise."""
    try:
        seqs = _lz4_sequences(stream)
    except IndexError:
        raise ValueError("the block ends inside a sequence")
    out = bytearray()
    for lit, lit_pos, _, offset, mlen, _, _ in seqs:
        for i in range(lit):
            out.append(stream[lit_pos + i])
        if offset is not None:
            if offset == 0 or offset > len(out):
                raise ValueError(f"match offset {offset} with {len(out)} bytes written")
            for _ in range(mlen):
                out.append(out[len(out) - offset])
        if len(out) > n:
            raise ValueError("more bytes than the chunk holds")
    if len(out) != n:
        raise ValueError(f"{len(out)} bytes, the chunk holds {n}")
    return bytes(out)


def decode(stream, codec, n):
    """The plain decoder of a ChunkCompressionType: the chunk's n bytes"""
    if codec == SNAPPY:
        out = snappy_decode(stream)
        if len(out) != n:
            raise ValueError(f"{len(out)} bytes, the chunk holds {n}")
        return out
    if codec == LZ4_LENGTH_PREFIXED:
        if struct.unpack("<i", stream[:4])[0] != n:
            raise ValueError("length prefix")
        stream = stream[4:]
    return lz4_decode(stream, n)


# ---- forward index -----------------------------------------------------------------------------------------------------------------------
def chunk_blob(chunks, docs_per_chunk, width, num_docs, compression, version=2):
    """Raw fixed-byte chunk forward index around already-compressed chunks (BaseChunkForwardIndexWriter: 7 big-endian ints — version,
    numChunks, numDocsPerChunk, sizeOfEntry, totalDocs, compressionType, dataHeaderStart = 28 — then the chunk start offsets, ints in
    version 2 and longs in version 3, then the chunks back to back)."""
    assert version in (2, 3)
    off_size = 4 if version == 2 else 8
    pos = 28 + len(chunks) * off_size
    offs = bytearray()
    for ch in chunks:
        offs += pos.to_bytes(off_size, "big")
        pos += len(ch)
    return struct.pack(">7i", version, len(chunks), docs_per_chunk, width, num_docs, compression, 28) + bytes(offs) + b"".join(chunks)


# ---- what a stream contains --------------------------------------------------------------------------------------------------------------
def stream_elements(stream, codec):
    """Counter of a stream's elements.  Both codecs: ('copy_offset', offset); ('overlap', offset) for a copy with offset < length,
    ('disjoint',) otherwise; ('run', offset, total) for a maximal row of copies with one offset and no literal between (a pattern longer
    than one snappy copy); ('ends_in_copy', d) when the last copy ends d bytes before the end of the chunk; ('literal_then_copies',) for a
    chunk that is one literal followed by copies only (in LZ4: and the literals that have to end the block).
    snappy: ('literal', form, length), ('literal_form', form), ('copy', kind, offset, length), ('copy_kind', kind).
    LZ4: ('literal', length), ('match', offset, length), ('literal_chain', extra bytes, ends in a 0 byte), ('match_chain', ...)."""
    c = Counter()
    copies = []   # (offset, length, a literal came before it)
    total = 0
    last_copy_end = None
    if codec == SNAPPY:
        _, els = _snappy_elements(stream)
        fresh = True
        literals_first = bool(els) and els[0][0] == "L" and sum(el[0] == "L" for el in els) == 1
        for el in els:
            if el[0] == "L":
                c[("literal", el[1], el[2])] += 1
                c[("literal_form", el[1])] += 1
                total += el[2]
                fresh = True
            else:
                _, kind, offset, n = el
                c[("copy", kind, offset, n)] += 1
                c[("copy_kind", kind)] += 1
                copies.append((offset, n, fresh))
                fresh = False
                total += n
                last_copy_end = total
    else:
        literals_first = True
        for lit, _, lit_extra, offset, mlen, m_extra, (lit_end, m_end) in _lz4_sequences(stream[4:] if codec == LZ4_LENGTH_PREFIXED else stream):
            c[("literal", lit)] += 1
            total += lit
            if lit_extra:
                c[("literal_chain", lit_extra, lit_end == 0)] += 1
            if offset is not None:
                c[("match", offset, mlen)] += 1
                if m_extra:
                    c[("match_chain", m_extra, m_end == 0)] += 1
                copies.append((offset, mlen, lit > 0 or not copies))
                total += mlen
                last_copy_end = total
    run = None
    for offset, n, fresh in copies:
        c[("copy_offset", offset)] += 1
        c[("overlap", offset) if offset < n else ("disjoint",)] += 1
        if run and not fresh and run[0] == offset:
            run[1] += n
        else:
            if run:
                c[("run", run[0], run[1])] += 1
            run = [offset, n]
    if run:
        c[("run", run[0], run[1])] += 1
    if last_copy_end is not None:
        c[("ends_in_copy", total - last_copy_end)] += 1
    if len(copies) > 1 and not any(fresh for _, _, fresh in copies[1:]) and literals_first:
        c[("literal_then_copies",)] += 1
    return c


def tally(counter, codec):
    """A stream_elements counter folded for a report: element kinds, and the offsets of the overlapping copies"""
    out = Counter()
    for key, k in counter.items():
        if key[0] in ("literal_form", "copy_kind", "disjoint", "literal_then_copies"):
            out[key] += k
        elif key[0] in ("literal_chain", "match_chain"):
            out[(key[0], key[1] if key[1] < 4 else "4+", "ends in 0" if key[2] else "")] += k
        elif key[0] == "overlap":
            out[("overlap", key[1] if key[1] < 9 else ("9..63" if key[1] < 64 else ">=64"))] += k
        elif key[0] == "run":
            out[("run", "<=64" if key[2] <= 64 else ">64")] += k
        elif key[0] == "copy" and 63 <= key[3] <= 64:
            out[("copy_length", key[3])] += k
        elif key[0] == "match":
            out[("match",)] += k
            if 63 <= key[2] <= 65:
                out[("copy_length", key[2])] += k
    return out


# ---- operation plans ---------------------------------------------------------------------------------------------------------------------
def execute_plan(plan, rng, alphabet=None):
    """The plain bytes of a plan of ('L', n, ...) / ('C', offset, n, ...) ops: random bytes (of `alphabet`) under a literal, the bytes
    `offset` back under a copy."""
    out = bytearray()
    for op in plan:
        if op[0] == "L":
            out += bytes(rng.choices(alphabet, k=op[1])) if alphabet else rng.randbytes(op[1])
        else:
            _, offset, n = op[:3]
            assert 1 <= offset <= len(out), (op, len(out))
            if offset >= n:
                out += out[len(out) - offset:len(out) - offset + n]
            else:
                pat = bytes(out[len(out) - offset:])
                out += (pat * (n // offset + 1))[:n]
    return bytes(out)


def snappy_ops(plan, rng=None):
    """A plan as snappy ops: copies cut into pieces of at most 64 bytes; with `rng`, ops that name no form / kind get a random legal one"""
    ops = []
    for op in plan:
        if op[0] == "L":
            if len(op) > 2 or rng is None:
                ops.append(op)
            else:
                n = op[1]
                ops.append(("L", n, rng.choice([f for f in range(5) if (n <= 60 if f == 0 else n - 1 < (1 << (8 * f)))])))
        else:
            offset, n = op[1], op[2]
            while n > 0:
                m = min(n, 64)
                if len(op) > 3:
                    ops.append(("C", offset, m, op[3]))
                elif rng is None:
                    ops.append(("C", offset, m))
                else:
                    ops.append(("C", offset, m, rng.choice([k for k in (1, 2, 3) if k == 3 or (k == 2 and offset < 65536) or (k == 1 and 4 <= m <= 11 and offset < 2048)])))
                n -= m
    return ops


def lz4_seqs(plan, size):
    """A plan as LZ4 sequences for a chunk of `size` bytes.  A copy the block format cannot hold as a match — under 4 bytes, an offset over
    65535, or one that breaks the end-of-block rules — becomes literals: the bytes are the same."""
    seqs = []
    lit = pos = 0
    for op in plan:
        if op[0] == "L":
            lit += op[1]
            pos += op[1]
        else:
            offset, n = op[1], op[2]
            if n >= 4 and offset < 65536 and pos <= size - LZ4_MFLIMIT and pos + n <= size - LZ4_LAST_LITERALS:
                seqs.append((lit, offset, n))
                lit = 0
            else:
                lit += n
            pos += n
    assert pos == size
    seqs.append((lit, 0, 0))
    return seqs


def random_plan(rng, size, max_len=300):
    """Random ops over `size` bytes: offsets 1 up to the bytes written so far (half of them below 70, where copies overlap), lengths 1 to
    `max_len`; a literal first."""
    plan = [("L", min(size, rng.randint(1, max_len)))]
    pos = plan[0][1]
    while pos < size:
        n = min(size - pos, rng.randint(1, max_len))
        if rng.random() < 0.6:
            offset = rng.randint(1, min(pos, 70)) if rng.random() < 0.5 else rng.randint(1, pos)
            plan.append(("C", offset, n))
        else:
            plan.append(("L", n))
        pos += n
    return plan


def budgeted_snappy_ops(ops, size):
    """`ops` with non-minimal forms dropped from the point where the stream would outgrow the staging area (random forms cost up to 4
    bytes per element; the shortest forms of a plan with lengths 1..300 fit with room to spare, which snappy_stream asserts)"""
    cap = staging_bytes(size)

    def cost(op):
        if op[0] == "L":
            form = op[2] if len(op) > 2 else _min_literal_form(op[1])
            return 1 + form + op[1]
        kind = op[3] if len(op) > 3 else _min_copy_kind(op[1], op[2])
        return (2, 3, 5)[kind - 1]
    used = len(_varint(size))
    slack = cap - used - sum(cost(op[:2] if op[0] == "L" else op[:3]) for op in ops)
    assert slack >= 0
    out = []
    for op in ops:
        extra = cost(op) - cost(op[:2] if op[0] == "L" else op[:3])
        if extra <= slack:
            slack -= extra
            out.append(op)
        else:
            out.append(op[:2] if op[0] == "L" else op[:3])
    return out


Fixture = namedtuple("Fixture", "name codec plain ops")   # codec: SNAPPY or LZ4 (an LZ4 fixture serves LZ4_LENGTH_PREFIXED too); ops: snappy ops / LZ4 sequences


def fixture_stream(fx, codec=None):
    codec = codec or fx.codec
    if fx.codec == SNAPPY:
        assert codec == SNAPPY
        return snappy_stream(fx.ops, fx.plain)
    block = lz4_stream(fx.ops, fx.plain)
    return lz4_length_prefixed(block, len(fx.plain)) if codec == LZ4_LENGTH_PREFIXED else block


def padded(fx, size):
    """The fixture with a literal appended that fills the chunk to `size` bytes (random bytes, seeded by the fixture's name)"""
    pad = size - len(fx.plain)
    assert pad >= 0
    if pad == 0:
        return fx
    plain = fx.plain + random.Random("pad " + fx.name).randbytes(pad)
    if fx.codec == SNAPPY:
        return Fixture(fx.name, fx.codec, plain, list(fx.ops) + [("L", pad)])
    lit = fx.ops[-1][0]
    return Fixture(fx.name, fx.codec, plain, list(fx.ops[:-1]) + [(lit + pad, 0, 0)])


def random_chunk(codec, size, seed, alphabet=None):
    """(plain, stream) of one chunk of `size` bytes from a random plan — the fixtures' random part at any chunk size"""
    rng = random.Random(f"chunk {SNAPPY if codec == SNAPPY else LZ4} {size} {seed}")
    plan = random_plan(rng, size)
    plain = execute_plan(plan, rng, alphabet)
    if codec == SNAPPY:
        return plain, snappy_stream(budgeted_snappy_ops(snappy_ops(plan, rng), size), plain)
    block = lz4_stream(lz4_seqs(plan, size), plain)
    return plain, (lz4_length_prefixed(block, size) if codec == LZ4_LENGTH_PREFIXED else block)


# ---- the fixture set ---------------------------------------------------------------------------------------------------------------------
SMALL, LARGE = 4096, 65536    # the two chunk sizes the fixtures are packed into: every fixture is at most LARGE bytes
OVERLAP_OFFSETS = (1, 2, 3, 5, 6, 7, 63, 64, 65)
RUN_TOTALS = (63, 64, 65, 127, 128, 129)   # on both sides of 64 and of 128
RANDOM_CHUNKS = 160


def _build_fixtures():
    out = []

    def add(name, codec, plan, size=None):
        rng = random.Random(f"fixture {name}")
        plain = execute_plan(plan, rng)
        assert size is None or len(plain) == size, (name, len(plain))
        ops = snappy_ops(plan) if codec == SNAPPY else lz4_seqs(plan, len(plain))
        out.append(Fixture(name, codec, plain, ops))

    # -- snappy literals: every length in its shortest form, 61 and 257 also in 3 and 4 length bytes, the whole chunk
    add("snappy literal lengths", SNAPPY, [("L", 1), ("L", 60), ("L", 61), ("L", 256), ("L", 257), ("L", 61, 3), ("L", 61, 4), ("L", 257, 3),
                                            ("L", 257, 4), ("L", 1, 1), ("L", 60, 2)])
    add("snappy whole-chunk literal", SNAPPY, [("L", SMALL)], SMALL)
    # -- snappy copies, kind 1: lengths 4 and 11 at offsets 1, 255, 256, 2047
    plan = [("L", 2047)]
    for offset in (1, 255, 256, 2047):
        for n in (4, 11):
            plan += [("C", offset, n, 1), ("L", 3)]
    add("snappy kind-1 copies", SNAPPY, plan)
    # -- kind 2: lengths 1 and 64 at offsets 1, 2048 and the largest a chunk allows (everything written so far; 65535 in a full-size chunk)
    plan = [("L", 2048)]
    for offset in (1, 2048):
        for n in (1, 64):
            plan += [("C", offset, n, 2), ("L", 5)]
    for n in (1, 64):
        plan += [("C", sum(op[1] if op[0] == "L" else op[2] for op in plan), n, 2), ("L", 2)]
    add("snappy kind-2 copies", SNAPPY, plan)
    plan = [("L", 65535), ("C", 65535, 1, 2)]
    add("snappy kind-2 largest offset", SNAPPY, plan, LARGE)
    plan = [("L", LARGE - 64), ("C", LARGE - 64, 64, 2)]
    add("snappy kind-2 largest offset, 64 bytes", SNAPPY, plan, LARGE)
    # -- kind 3: small offsets, and offsets above 32 767 (bit 15 and above: a 2-byte or signed read of the offset goes wrong)
    plan = [("L", 40), ("C", 1, 9, 3), ("L", 2), ("C", 3, 64, 3), ("C", 40, 17, 3), ("L", 1), ("C", 7, 1, 3)]
    add("snappy kind-3 small offsets", SNAPPY, plan)
    plan = [("L", 40000), ("C", 32768, 64, 3), ("C", 40000, 33, 3), ("L", 4), ("C", 32769, 1, 3), ("L", 25370), ("C", 65472, 64, 3)]
    add("snappy kind-3 large offsets", SNAPPY, plan, LARGE)
    # -- a copy that ends on the last byte of a full chunk; one short literal followed by copies only
    add("snappy copy ends the chunk", SNAPPY, [("L", SMALL - 100), ("C", 333, 64), ("C", 5, 36)], SMALL)
    add("snappy copy ends the chunk, kind 1", SNAPPY, [("L", SMALL - 11), ("C", 2047, 11, 1)], SMALL)
    add("snappy one literal then copies", SNAPPY, [("L", 3), ("C", 3, 64), ("C", 1, 5), ("C", 60, 64), ("C", 2, 1), ("C", 130, 7), ("C", 3, 64, 3),
                                                   ("C", 64, 64), ("C", 200, 200), ("C", 11, 11, 1)])

    # -- LZ4 literal lengths 0, 14, 15, 15+254, 15+255 and above 15+2*255; match lengths 4, 18, 19, 19+254, 19+255
    plan = [("L", 14), ("C", 14, 4), ("C", 2, 18), ("L", 15), ("C", 7, 19), ("L", 15 + 254), ("C", 100, 19 + 254), ("L", 15 + 255), ("C", 300, 19 + 255),
            ("L", 15 + 2 * 255 + 77), ("C", 1, 4), ("L", 15 + 2 * 255), ("C", 9, 19 + 2 * 255), ("L", 12)]
    add("lz4 length chains", LZ4, plan)
    add("lz4 whole-chunk literal", LZ4, [("L", SMALL)], SMALL)
    # -- offsets 1, 4095, 4096 and the largest a chunk allows (65524: the last match starts 12 bytes before the end of a 65536-byte chunk)
    plan = [("L", 4096), ("C", 1, 4), ("L", 1), ("C", 4095, 4), ("L", 2), ("C", 4096, 18), ("C", 4095, 19), ("C", 4096, 4096), ("L", 30)]
    add("lz4 offsets 4095 and 4096", LZ4, plan)
    plan = [("L", 65535 - 40), ("C", 65535 - 40, 20), ("L", 20)]
    add("lz4 offset of everything written", LZ4, plan)
    add("lz4 largest offset", LZ4, [("L", LARGE - 12), ("C", LARGE - 12, 7), ("L", 5)], LARGE)
    # -- the latest match the block format allows: it starts 12 bytes and ends 5 bytes before the end of a full chunk
    add("lz4 last legal match", LZ4, [("L", SMALL - 100), ("C", 333, 88), ("C", 5, 7), ("L", 5)], SMALL)
    add("lz4 one literal then matches", LZ4, [("L", 3), ("C", 3, 64), ("C", 1, 5), ("C", 60, 64), ("C", 2, 4), ("C", 130, 7), ("C", 3, 65),
                                              ("C", 64, 63), ("C", 200, 200), ("C", 11, 300), ("L", 12)])

    # -- both codecs: overlapping copies, every offset with totals on both sides of 64 and of 128
    for codec, tag in ((SNAPPY, "snappy"), (LZ4, "lz4")):
        for offset in OVERLAP_OFFSETS:
            plan = [("L", offset)]
            for k, total in enumerate(RUN_TOTALS):
                plan += [("C", offset, total), ("L", 1 + k % 3)]
            add(f"{tag} overlap offset {offset}", codec, plan + [("L", 12)])
            if offset > 1:   # the same pattern started in the middle of older data: window = s_out + op - offset is not the chunk's start
                plan = [("L", 100 + offset)]
                for total in RUN_TOTALS:
                    plan += [("C", offset, total), ("L", offset + 1)]
                add(f"{tag} overlap offset {offset}, inner", codec, plan + [("L", 12)])

    # -- the seeded random part
    for codec, tag in ((SNAPPY, "snappy"), (LZ4, "lz4")):
        for k in range(RANDOM_CHUNKS):
            rng = random.Random(f"random {tag} {k}")
            size = SMALL if k % 8 == 0 else rng.randint(16, SMALL)
            plan = random_plan(rng, size)
            plain = execute_plan(plan, rng)
            ops = budgeted_snappy_ops(snappy_ops(plan, rng), size) if codec == SNAPPY else lz4_seqs(plan, size)
            out.append(Fixture(f"{tag} random {k}", codec, plain, ops))
    return out


FIXTURES = _build_fixtures()


def fixtures_for(codec):
    """The fixtures of a ChunkCompressionType (LZ4 and LZ4_LENGTH_PREFIXED share theirs)"""
    return [fx for fx in FIXTURES if fx.codec == (SNAPPY if codec == SNAPPY else LZ4)]
