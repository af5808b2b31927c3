"""Walk of a reference index file (csa_wt<wt_huff<>,64,8192>::serialize) for the tests of the
exporter: where each section lies, and how many select superblocks are stored long."""
import struct
def walk(buf):
    """(sections, longs): sections[name] = (start, end) in bytes for head, bv, rank, select1, select0, tree, sa_samples,
    isa_samples, alphabet; longs[select1 | select0] = (superblocks, [those whose mini_or_long bit says long]).  Asserts that the
    walk ends at the file's last byte."""
    p = 0
    sec = {}
    def u64():
        nonlocal p
        v = struct.unpack_from("<Q", buf, p)[0]; p += 8; return v
    def ivec(fixed):
        nonlocal p
        bits = u64()
        w = fixed
        if not fixed:
            w = buf[p]; p += 1
        s = p
        p += ((bits + 63) >> 6) * 8
        return bits, w, s
    s0 = p; u64(); u64(); sec["head"] = (s0, p)
    s0 = p; ivec(1); sec["bv"] = (s0, p)
    s0 = p; ivec(64); sec["rank"] = (s0, p)
    longs = {}
    for name in ("select1", "select0"):
        s0 = p
        arg = u64(); sb = 0; nlong = []
        if arg:
            sb = (arg + 4095) >> 12
            ivec(0)
            bits, _, at = ivec(1)
            for i in range(sb):
                if bits and not (buf[at + (i >> 3)] >> (i & 7)) & 1:
                    nlong.append(i)
                ivec(0)
        longs[name] = (sb, nlong)
        sec[name] = (s0, p)
    s0 = p; nn = u64(); p += 22 * nn + 512 + 2048; sec["tree"] = (s0, p)
    s0 = p; ivec(0); sec["sa_samples"] = (s0, p)
    s0 = p; ivec(0); sec["isa_samples"] = (s0, p)
    s0 = p; ivec(8); ivec(8); ivec(64); p += 2; sec["alphabet"] = (s0, p)
    assert p == len(buf), (p, len(buf))
    return sec, longs
