"""A pure-Python model of the kmers-file rules of `guidescan enumerate -f` (cli::read_kmers, host/cli_common.hpp;
src/genomics/kmer.cxx:9-25), the yardstick of the device reader (csrc/gs_kmers_scan.h, gs_kmersfile.hip), and the files
its tests share.

  parse(raw) -> Parsed(rows=[(id, sequence, pam, plus)], mixed) or raises KmersError(kind, message, line, row, text)
"""
from collections import namedtuple

NAMES = (b"id", b"sequence", b"pam", b"chromosome", b"position", b"sense")
FEW, POSITION, EMPTY, LACKS = 1, 2, 3, 4

Parsed = namedtuple("Parsed", "rows mixed")


class KmersError(Exception):
    def __init__(self, kind, message, line=0, row=0, text=b""):
        super().__init__(message)
        self.kind, self.message, self.line, self.row, self.text = kind, message, line, row, text


def lines_of(raw: bytes):
    """getline: split at '\\n'; a last line without a newline is a line, a newline at the end starts none"""
    if not raw:
        return []
    parts = raw.split(b"\n")
    if raw.endswith(b"\n"):
        parts.pop()
    return [p[:-1] if p.endswith(b"\r") else p for p in parts]           # one trailing '\r' is dropped


def fields_of(line: bytes):
    return [f.strip(b" \t") for f in line.split(b",")]                    # no quoting; ' ' and '\t' only


def position_ok(field: bytes) -> bool:
    """strtoll(field, &end, 10) converts something and *end == 0 (a NUL inside the field ends the C string)"""
    s = field.split(b"\0", 1)[0]
    i = 0
    while i < len(s) and s[i:i + 1] in b" \t\n\v\f\r":
        i += 1
    if i < len(s) and s[i:i + 1] in b"+-":
        i += 1
    digits = 0
    while i < len(s) and s[i:i + 1].isdigit():
        i, digits = i + 1, digits + 1
    return digits > 0 and i == len(s)


def parse(raw: bytes) -> Parsed:
    lines = lines_of(raw)
    if not lines:
        raise KmersError(EMPTY, "empty kmers file")
    header = fields_of(lines[0])
    col = {}
    for name in NAMES:
        where = [j for j, h in enumerate(header) if h == name]
        if not where:
            raise KmersError(LACKS, "kmers file lacks column " + name.decode(), text=name)
        col[name] = where[-1]
    rows = []
    for number, line in enumerate(lines[1:], 1):
        if not line:
            continue
        f = fields_of(line)
        if len(f) < len(header):
            raise KmersError(FEW, "kmers row with too few columns: " + line.decode("latin-1"), number, len(rows), line)
        if not position_ok(f[col[b"position"]]):
            raise KmersError(POSITION, "kmers position is not an integer: " + f[col[b"position"]].decode("latin-1"), number, len(rows),
                             f[col[b"position"]])
        rows.append((f[col[b"id"]], f[col[b"sequence"]], f[col[b"pam"]], f[col[b"sense"]] == b"+"))
    mixed = any((len(r[1]), len(r[2])) != (len(rows[0][1]), len(rows[0][2])) for r in rows) or (bool(rows) and not rows[0][1])
    return Parsed(rows, mixed)


def compare(got, exp: Parsed, where=""):
    """got: the dict of api.parse_kmers_model_tiles / api.kmers_arrays"""
    rows = exp.rows
    assert got["n"] == len(rows), where
    L, P = (len(rows[0][1]), len(rows[0][2])) if rows else (0, 0)
    assert (got["L"], got["P"]) == (L, P), where
    assert got["seqs"] == b"".join(r[1] for r in rows), where
    assert got["pams"] == b"".join(r[2] for r in rows), where
    assert got["ids"] == b"".join(r[0] for r in rows), where
    off = [0]
    for r in rows:
        off.append(off[-1] + len(r[0]))
    assert got["id_off"].tolist() == off, where
    assert got["sense"].tolist() == [1 if r[3] else 0 for r in rows], where


HEADER = b"id,sequence,pam,chromosome,position,sense\n"


def row(i, seq=b"ACGTACGTACGTACGTACGT", pam=b"NGG", chrom=b"chr1", pos=None, sense=b"+"):
    return b"g%d,%s,%s,%s,%d,%s\n" % (i, seq, pam, chrom, 100 + i if pos is None else pos, sense)


def good_files(tile):
    """name -> bytes: files that parse, with their edge cases placed against tiles of `tile` bytes"""
    f = {}
    body = b"".join(row(i, sense=b"+-"[i & 1:][:1]) for i in range(40))
    f["plain"] = HEADER + body
    f["crlf"] = (HEADER + body).replace(b"\n", b"\r\n")
    f["no newline at the end"] = (HEADER + body)[:-1]
    f["blank lines"] = HEADER + b"\n\r\n" + row(1) + b"\n\n" + row(2) + b"\r\n\n" + row(3) + b"\n\r\n\n"
    f["header only"] = HEADER
    f["header only, open"] = HEADER[:-1]
    f["header only, crlf"] = HEADER[:-1] + b"\r\n"
    f["permuted, extra columns"] = (b"x, sense ,position,y,pam,id,chromosome,\tsequence\t,z\n"
                                    b"1,+,5,2,NGG,a,chr1,ACGT,3\n4,-,6,5,NGG,b,chr2,TTTT,6,more,fields\n")
    f["a name twice"] = b"id,sequence,pam,chromosome,position,sense,id,sequence\nno,AAAA,NGG,c,1,+,yes,CCCC\n"
    f["blanks around and inside"] = HEADER + b" \tg 1\t , AC GT ,\tN G\t,c , 7 ,+ \n\t g2,ACG T\t,N\tG  ,c,\t8,\t-\n"
    f["empty id, chromosome, sense"] = HEADER + b",ACGT,NGG,,5,\n ,ACGT,NGG, ,6, \n"
    f["senses"] = HEADER + b"a,AC,G,c,1,+\nb,AC,G,c,1,-\nc,AC,G,c,1,x\nd,AC,G,c,1, +\ne,AC,G,c,1,++\nf,AC,G,c,1,+ +\n"
    f["positions"] = HEADER + b"a,AC,G,c,+5,+\nb,AC,G,c,-0,+\nc,AC,G,c,1234567890123456789012345,+\nd,AC,G,c,\v\f\r 7,+\ne,AC,G,c,  9\t,+\n"
    f["no pam"] = HEADER + b"a,ACGT,,c,5,+\nb,TTTT,,c,6,-\n"
    f["more fields than the header"] = HEADER + b"a,AC,G,c,5,+,x,y\nb,AC,G,c,5,-,,\n"
    # against the tile: a '\r' as the last byte of a tile with its '\n' first in the next; a comma on the edge; an id
    # longer than three tiles; lines of tile - 1, tile and tile + 1 bytes
    def padded_to(prefix, end_at):            # prefix + a row whose id is padded so that the file is end_at bytes long
        tail = b",ACGT,NGG,c,5,+"
        pad = end_at - len(prefix) - len(tail)
        assert pad >= 0
        return prefix + b"i" * pad + tail
    base = HEADER + row(0, seq=b"ACGT")
    k = (len(base) + 20 + tile) // tile * tile
    f["cr ends a tile"] = padded_to(base, k - 1) + b"\r\n" + row(1, seq=b"ACGT")
    f["comma on a tile edge"] = base + b"i" * (k - len(base) - 1) + b",ACGT,NGG,c,5,+\n" + b"i" * tile + b",TTTT,NGG,c,6,-\n"
    f["an id longer than three tiles"] = base + b"L" * (3 * tile + 5) + b",ACGT,NGG,c,5,-\n" + row(2, seq=b"ACGT")
    fixed = []
    for n in (tile - 1, tile, tile + 1):
        tail = b",ACGT,NGG,c,5,+\n"
        if n > len(tail):
            fixed += [b"j" * (n - len(tail)) + tail] * 3
    if fixed:
        f["lines of about a tile"] = HEADER + b"".join(fixed)
    return f


def bad_files():
    """name -> (bytes, kind): files the reader refuses, and which failure wins"""
    f = {}
    f["empty file"] = (b"", EMPTY)
    f["no sense column"] = (b"id,sequence,pam,chromosome,position\n", LACKS)
    f["pam and position missing"] = (b"id,sequence,sense,chromosome\n1,AC,+,c\n", LACKS)
    f["an empty header"] = (b"\nid,sequence,pam,chromosome,position,sense\n", LACKS)
    f["too few columns"] = (HEADER + row(1) + b"g2,ACGT,NGG,chr1,5\n" + row(3), FEW)
    f["too few columns, crlf"] = (HEADER.replace(b"\n", b"\r\n") + b"g2,ACGT,NGG,chr1,5\r\n", FEW)
    f["empty position"] = (HEADER + row(1) + b"g2,ACGT,NGG,chr1,,+\n", POSITION)
    f["digit then letter"] = (HEADER + b"g2,ACGT,NGG,chr1,5x,+\n", POSITION)
    f["digit then vertical tab"] = (HEADER + b"g2,ACGT,NGG,chr1,5\v,+\n", POSITION)
    f["sign only"] = (HEADER + b"g2,ACGT,NGG,chr1, - ,+\n", POSITION)
    f["few then position"] = (HEADER + row(1) + b"a,b\n" + b"g2,ACGT,NGG,chr1,x,+\n", FEW)
    f["position then few"] = (HEADER + row(1) + b"g2,ACGT,NGG,chr1,x,+\n" + b"a,b\n" + row(3), POSITION)
    f["few wins inside a row"] = (HEADER + b"g2,ACGT,NGG,chr1,x\n", FEW)
    f["a line of blanks"] = (HEADER + row(1) + b"  \t \n" + row(2), FEW)
    f["a lone cr behind a cr"] = (HEADER + row(1) + b"\r\r\n", FEW)
    return f


def random_files(count, seed):
    """small files over the bytes that matter, most of them refused somewhere"""
    import random
    rng = random.Random(seed)
    pieces = [b",", b",", b"\n", b"\r\n", b" ", b"\t", b"A", b"ACGT", b"NGG", b"+", b"-", b"12", b"x", b"\r", b"\v", b"chr1"]
    for _ in range(count):
        body = b""
        for _ in range(rng.randrange(0, 6)):
            if rng.random() < 0.7:
                body += row(rng.randrange(100), seq=rng.choice([b"ACGT", b"ACGT", b"ACGT", b"AC"]), sense=rng.choice([b"+", b"-", b" +"]))
            else:
                body += b"".join(rng.choice(pieces) for _ in range(rng.randrange(0, 14)))
        yield rng.choice([HEADER, HEADER, HEADER[:-1] + b"\r\n", b"sense,position,chromosome,pam,sequence,id\n"]) + body


def mixed_files():
    return {"mixed L": HEADER + row(1) + row(2, seq=b"ACGT") + row(3),
            "mixed P": HEADER + row(1) + row(2, pam=b"NGGA"),
            "first row without a sequence": HEADER + row(1, seq=b"") + row(2, seq=b"")}
