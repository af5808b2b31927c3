"""A small BAM builder for the tests of the device reader (SAMv1 sections 4.1 and 4.2): records from SAM lines or from
fields, any tags, and BGZF members cut where a test wants them, made with zlib's raw deflate.  It writes no reference
data: what the readers make of these files is compared with the SAM route and the committed CSVs."""
import struct
import zlib

NT16 = "=ACMGRSVTWYHKDBN"
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def header(text: str, refs) -> bytes:
    """magic, l_text, text, n_ref, the binary reference list [(name, length)]"""
    out = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(refs))
    for name, ln in refs:
        out += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<I", ln)
    return out


def tag_of(hexs: str) -> bytes:
    return b"ofH" + hexs.encode() + b"\0"


# one tag of every type the readers walk (A c C s S i I f Z H B), none of them the of:H: tag
EXTRA_TAGS = (b"xaAq" + b"xcc" + struct.pack("<b", -3) + b"xCC" + struct.pack("<B", 200) + b"xss" + struct.pack("<h", -300) +
              b"xSS" + struct.pack("<H", 60000) + b"xii" + struct.pack("<i", -70000) + b"xII" + struct.pack("<I", 4000000000) +
              b"xff" + struct.pack("<f", 0.25) + b"xzZsome text\0" + b"xhH1f8b\0" + b"ofZnot the list\0")
ARRAY_TAGS = (b"bcBc" + struct.pack("<i3b", 3, 1, -2, 3) + b"bsBS" + struct.pack("<i2H", 2, 7, 65535) +
              b"bfBf" + struct.pack("<i2f", 2, 1.5, -2.5) + b"beBi" + struct.pack("<i", 0))


def record(ref_id, pos0, flag, name, seq, tags=b"", n_cigar=0) -> bytes:
    """block_size and the alignment record; seq over =ACMGRSVTWYHKDBN"""
    packed = bytearray((len(seq) + 1) // 2)
    for i, c in enumerate(seq):
        packed[i >> 1] |= NT16.index(c) << (0 if i & 1 else 4)
    body = struct.pack("<iiBBHHHiiii", ref_id, pos0, len(name) + 1, 0, 4680, n_cigar, flag, len(seq), -1, -1, 0)
    body += name.encode() + b"\0" + struct.pack("<I", len(seq) << 4) * n_cigar + bytes(packed) + b"\xff" * len(seq) + tags
    return struct.pack("<i", len(body)) + body


def sam_fields(line: str):
    """a SAM line -> (name, flag, rname, pos0, seq, [of hex digits, one per of:H: field])"""
    f = line.rstrip("\r\n").split("\t")
    return f[0], int(f[1]), f[2], int(f[3]) - 1, f[9], [t[5:] for t in f[11:] if t.startswith("of:H:")]


def from_sam(sam_text: str, refs=None, header_text=None):
    """-> (the header's bytes, [record bytes]) of a SAM text.  refs: the binary reference list (default: the @SQ lines in
    their order); header_text: the text header (default: the SAM text's own header lines).  None when a SEQ has symbols
    a BAM record cannot hold (lower case: the nibbles would not give it back)."""
    lines = [ln for ln in sam_text.split("\n") if ln.strip("\r")]
    head = "".join(ln.rstrip("\r") + "\n" for ln in lines if ln.startswith("@"))
    sq = []
    for ln in lines:
        if ln.startswith("@SQ"):
            t = dict(x.split(":", 1) for x in ln.rstrip("\r").split("\t")[1:] if ":" in x)
            sq.append((t["SN"], int(t["LN"])))
    refs = list(sq if refs is None else refs)
    index = {}
    for i, (n, _) in enumerate(refs):
        index.setdefault(n, i)
    recs = []
    for ln in lines:
        if ln.startswith("@"):
            continue
        name, flag, rname, pos0, seq, ofs = sam_fields(ln)
        if any(c not in NT16 for c in seq):
            return None
        recs.append(record(index.get(rname, -1), pos0, flag, name, seq, b"".join(tag_of(h) for h in ofs)))
    return header(head if header_text is None else header_text, refs), recs


def sam_line(name, flag, rname, pos0, seq, ofs=()) -> str:
    return "\t".join([name, str(flag), rname or "*", str(pos0 + 1), "255", "*", "*", "0", "0", seq, "*"] +
                     ["of:H:" + h for h in ofs]) + "\n"


def member(raw: bytes, level=6) -> bytes:
    """one BGZF member of at most 65,536 bytes"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    data = c.compress(raw) + c.flush()
    size = 18 + len(data) + 8
    assert len(raw) <= 65536 and size <= 65536
    return (bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0]) + struct.pack("<H", size - 1) + data +
            struct.pack("<II", zlib.crc32(raw), len(raw)))


def members(raw: bytes, cuts=(), piece=0xff00, level=6):
    """raw cut at the offsets `cuts` and wherever a piece would exceed `piece` bytes -> [member bytes]"""
    edges = sorted(set([0, len(raw)] + [c for c in cuts if 0 < c < len(raw)]))
    out = []
    for a, b in zip(edges, edges[1:]):
        for at in range(a, b, piece):
            out.append(member(raw[at:min(b, at + piece)], level))
    return out


def dynamic_code_lengths(stream: bytes):
    """the code lengths a deflate stream's first block sends in its dynamic header (RFC 1951 section 3.2.7)
    -> (literal/length lengths, distance lengths)"""
    bits = int.from_bytes(stream[:1200], "little")
    at = 0

    def take(n):
        nonlocal at
        v = (bits >> at) & ((1 << n) - 1)
        at += n
        return v

    take(1)
    assert take(2) == 2, "not a dynamic block"
    nlen, ndist, ncode = take(5) + 257, take(5) + 1, take(4) + 4
    cl = [0] * 19
    for i in range(ncode):
        cl[(16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)[i]] = take(3)
    code, codes = 0, {}
    for ln in range(1, 8):   # canonical codes of the code-length code
        for sym in range(19):
            if cl[sym] == ln:
                codes[(ln, code)] = sym
                code += 1
        code <<= 1
    lens = []
    while len(lens) < nlen + ndist:
        ln, code = 0, 0
        while (ln, code) not in codes:
            code = (code << 1) | take(1)
            ln += 1
        sym = codes[(ln, code)]
        if sym < 16:
            lens.append(sym)
        elif sym == 16:
            lens += [lens[-1]] * (3 + take(2))
        else:
            lens += [0] * (3 + take(3) if sym == 17 else 11 + take(7))
    return lens[:nlen], lens[nlen:]


def _dg():
    import decode_golden
    return decode_golden


def hand_database():
    """records over the hand fixture that take every branch of the field walk, with the SAM text of the same records"""
    sq, recs, fasta = _dg().loaded("hand")
    with_of = [r for r in recs if r.hex and all(c in NT16 for c in r.seq) and r.rname]
    a, b = with_of[0], with_of[-1]
    index = {n: i for i, (n, _) in enumerate(sq)}
    delim = -(sum(n for _, n in sq) + 1)
    words = struct.unpack(f"<{len(a.hex) // 16}q", bytes.fromhex(a.hex))
    e = words.index(delim)
    big = _dg().hexw(list(words[:e - 1]) * (4600 // max(1, e - 1) + 1) + [words[e - 1], delim])   # above 70 KB of digits
    assert len(big) > 70_000
    rows = [
        # (refID by name, pos0, flag, name, seq, tags, the of fields of the SAM line)
        (a.rname, a.pos0, 16 if a.reverse else 0, a.id, a.seq, tag_of(a.hex), [a.hex]),
        (None, 7, 0, "unmapped", "ACGTACGTACGTACGTACGTAGG", tag_of(b.hex), [b.hex]),                    # refID -1
        (b.rname, b.pos0, 16 if b.reverse else 0, "no_of", b.seq, b"", []),                                 # no of tag
        (a.rname, a.pos0, 0, "two_of", a.seq[:21], tag_of(b.hex) + b"xii\1\0\0\0" + tag_of(a.hex), [b.hex, a.hex]),  # odd l_seq 21
        (b.rname, b.pos0, 16 if b.reverse else 0, "every_type", b.seq, EXTRA_TAGS + tag_of(b.hex) + EXTRA_TAGS, [b.hex]),
        (a.rname, 0, 0, "arrays", a.seq[:22], ARRAY_TAGS + tag_of(a.hex) + ARRAY_TAGS, [a.hex]),
        (a.rname, a.pos0, 16 if a.reverse else 0, "big", a.seq, tag_of(big), [big]),
        (b.rname, b.pos0, 0, "behind_big", b.seq, tag_of(b.hex) + b"ztZ\0", [b.hex]),
    ]
    sam = "".join(sam_line(name, flag, rname, pos0, seq, ofs) for rname, pos0, flag, name, seq, tags, ofs in rows)
    return sq, index, rows, sam


def build(rows, index):
    return [record(index.get(rname, -1), pos0, flag, name, seq, tags, n_cigar=1 if name == "arrays" else 0)
            for rname, pos0, flag, name, seq, tags, ofs in rows]
