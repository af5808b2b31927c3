"""The index's derived tables restated in numpy from their description in gs_common.h (gs_strand_dev, gs_pairtab_dev) and
in the head of gs_pairtab.hip.  TEST INFRASTRUCTURE: no GPU, no library.  tests/test_gpu_index_tables.py compares every
entry of every device array with what is computed here; tests/test_index_tables_model.py holds this file to account
against brute force on small texts and proves that the comparison helpers below see a single wrong entry.

Everything is stated from the strand's text `t` (uint8, the 0 sentinel as its last byte: sa_model.strand_text) and its
suffix array `sa` (row -> text position).  Symbol classes: A, C, G, T = 0..3, 'N' = 4, every other byte = 5; 6 stands for
"before the text start".  A k-mer is valid when its k symbols are A, C, G, T and lie in the text proper (not the sentinel);
its table index holds its FIRST text symbol in the LOWEST two bits.  The context of a row is the 16 symbols before its
suffix, nearest first.
"""
import numpy as np

CLS = np.full(256, 5, dtype=np.int64)
for _i, _b in enumerate(b"ACGTN"):
    CLS[_b] = _i
PT_BIG = 63            # gs_common.h: GS_PT_BIG
DEEP_MAX_ROWS = 4096   # a deep entry with more rows carries the flag in place of masks
U32 = np.uint32


# ------------------------------------------------------------------------------------------------ the strand's arrays
def kmer_codes(t, k):
    """(code, valid) per text position p = 0 .. n-1: the k-mer that starts at p (n = len(t), sentinel included)"""
    n = t.shape[0]
    cls = CLS[t[:n - 1]]
    code = np.zeros(n, dtype=np.int64)
    valid = np.zeros(n, dtype=bool)
    m = n - 1 - k + 1                      # windows inside the text proper
    if m > 0:
        ok = np.ones(m, dtype=bool)
        for i in range(k):
            c = cls[i:i + m]
            ok &= c < 4
            code[:m] |= (c & 3) << (2 * i)
        valid[:m] = ok
        code[:m][~ok] = 0
    return code, valid


def contexts(t, sa):
    """per ROW: nib (uint64: the 16 symbols before the suffix as classes 0..6, nearest in the lowest nibble), w (uint32: the
    same, 2 bits each, a symbol outside A,C,G,T or before the text start stored as A) and exc (some nibble is not 0..3)"""
    n = t.shape[0]
    pad = np.concatenate([np.full(16, 6, dtype=np.int64), CLS[t]])
    p = np.asarray(sa, dtype=np.int64)
    nib = np.zeros(n, dtype=np.uint64)
    w = np.zeros(n, dtype=np.uint64)
    exc = np.zeros(n, dtype=bool)
    for j in range(1, 17):
        c = pad[p + 16 - j]
        nib |= c.astype(np.uint64) << np.uint64(4 * (j - 1))
        exc |= c > 3
        w |= np.where(c > 3, 0, c).astype(np.uint64) << np.uint64(2 * (j - 1))
    return nib, w.astype(U32), exc


def mask_offsets(mask_off):
    return [(mask_off >> (4 * j)) & 15 for j in range(4)]


def default_mask_off(k):
    """gs_strand_dev::mask_off as the builder chooses it: 0, 2, 4 and 21-k kept within 6..14"""
    return 0 | (2 << 4) | (4 << 8) | (min(max(21 - k if k < 21 else 6, 6), 14) << 12)


def _or_bits(size, index, bit):
    """out[i] = OR over the occurrences with index i of 1 << bit (bit < 32)"""
    out = np.zeros(size, dtype=U32)
    key = np.unique(index.astype(np.int64) * 32 + bit.astype(np.int64))
    np.bitwise_or.at(out, key >> 5, (np.uint64(1) << (key & 31).astype(np.uint64)).astype(U32))
    return out


def pair_masks(size, index, w, offsets):
    """(z, w): four 16-bit sets of the symbol pairs the context words show at the four offsets, per table index"""
    w = w.astype(np.int64)
    v = [(w >> (2 * o)) & 15 for o in offsets]
    z = _or_bits(size, index, v[0]) | _or_bits(size, index, 16 + v[1])
    ww = _or_bits(size, index, v[2]) | _or_bits(size, index, 16 + v[3])
    return z, ww


def strand_tables(t, sa, k, mask_off=None, ctx=True):
    """every array of gs_strand_dev but the rotated copies, as a dict of numpy arrays shaped like GenomeIndex.debug_array's,
    with the scalars of GenomeIndex.debug_layout under "layout".  ctx=False: a handle without context arrays (masks all ones)"""
    t = np.asarray(t, dtype=np.uint8)
    sa = np.asarray(sa, dtype=np.int64)
    n = t.shape[0]
    if mask_off is None:
        mask_off = default_mask_off(k)
    out = {}
    isa = np.empty(n, dtype=np.int64)
    isa[sa] = np.arange(n)
    # ---- Occ blocks: BWT symbol of row r = the symbol before its suffix (the sentinel for the suffix at 0)
    bwt = t[(sa - 1) % n]
    bcls = CLS[bwt]
    nblocks = (n >> 7) + 1
    rows = nblocks * 128
    c = np.full(rows, 5, dtype=np.int64)
    c[:n] = bcls
    base = c < 4

    def words(bits):   # 32 rows per word, row j of the word in bit j
        return np.packbits(bits.astype(np.uint8), bitorder="little").view("<u4").reshape(nblocks, 4)
    blocks = np.zeros((nblocks, 16), dtype=U32)
    for s in range(4):
        per_block = (c == s).reshape(nblocks, 128).sum(axis=1)
        blocks[:, s] = np.concatenate([[0], np.cumsum(per_block)[:-1]])
    blocks[:, 4:8] = words(base & ((c & 1) == 1))
    blocks[:, 8:12] = words(base & ((c & 2) == 2))
    blocks[:, 12:16] = words(~base)
    out["blocks"] = blocks
    out["sa"] = sa.astype(U32)
    # ---- C arrays: symbols of the text (sentinel included) smaller than c
    hist = np.bincount(t, minlength=256)
    smaller = np.concatenate([[0], np.cumsum(hist)[:-1]])
    out["C256"] = np.where(hist > 0, smaller, 0).astype(U32)
    lay = dict(n=n, blocks=nblocks, k=k, mask_off=mask_off if ctx else 0, C0=int(smaller[65]), C1=int(smaller[67]),
               C2=int(smaller[71]), C3=int(smaller[84]), CN=int(smaller[78]), has_n=int(hist[78] > 0))
    # ---- runs of equal symbols outside A,C,G,T (the sentinel is no symbol) in the BWT
    x = (bcls > 3) & (bwt != 0)
    prev = np.concatenate([[0], bwt[:-1]])
    starts = np.nonzero(x & ((np.arange(n) == 0) | (prev != bwt)))[0]
    nxt = np.concatenate([bwt[1:], [0]])
    ends = np.nonzero(x & ((np.arange(n) == n - 1) | (nxt != bwt)))[0] + 1
    sym = bwt[starts]
    seg = np.zeros((256, 2), dtype=U32)
    xs, xc = [], []
    at = 0
    for s in np.unique(sym):
        sel = sym == s
        st, ln = starts[sel], (ends - starts)[sel]
        seg[s] = (at, st.shape[0])
        xs += [st, [0xFFFFFFFF]]                       # the closing entry keeps xr_cum[i + 1] valid for the last run
        xc += [np.concatenate([[0], np.cumsum(ln)])]
        at += st.shape[0] + 1
        if s == 78:
            out["run_start"] = st.astype(U32)
            out["run_cum"] = np.concatenate([[0], np.cumsum(ln)]).astype(U32)
    out["xr_seg"] = seg
    out["xr_start"] = np.concatenate(xs).astype(U32) if xs else None
    out["xr_cum"] = np.concatenate(xc).astype(U32) if xc else None
    out.setdefault("run_start", None)
    out.setdefault("run_cum", None)
    lay["nruns"] = 0 if out["run_start"] is None else int(out["run_start"].shape[0])
    lay["xr_entries"] = at
    # ---- the depth-k table
    size = 4 ** k
    code, valid = kmer_codes(t, k)
    count = np.bincount(code[valid], minlength=size)           # over text positions: no suffix array in this
    rowvalid = valid[sa]
    vrows = np.nonzero(rowvalid)[0]
    rcode = code[sa[vrows]]
    first = np.zeros(size, dtype=np.int64)
    first[rcode[::-1]] = vrows[::-1]                           # the k-mer's first suffix in the suffix array
    nib, w, exc = contexts(t, sa)
    ptab = np.zeros((size, 4), dtype=U32)
    ptab[:, 0] = first
    ptab[:, 1] = count
    if ctx:
        flag = np.zeros(size, dtype=bool)
        flag[rcode[exc[vrows]]] = True
        ptab[:, 1] |= flag.astype(U32) << U32(31)
        ptab[:, 2], ptab[:, 3] = pair_masks(size, rcode, w[vrows], mask_offsets(mask_off))
        out["ctx"] = w
        out["ctx16"] = (w & U32(0xFFFF)).astype(np.uint16)
        er = vrows[exc[vrows]]
        out["exc_row"] = er.astype(U32) if er.size else None
        out["exc_sym"] = nib[er] if er.size else None
        out["isa"] = isa.astype(U32)
        lay["n_exc"] = int(er.size)
    else:
        ptab[:, 2:] = 0xFFFFFFFF
        for name in ("ctx", "ctx16", "exc_row", "exc_sym", "isa"):
            out[name] = None
        lay["n_exc"] = 0
    out["ptab"] = ptab
    out["layout"] = lay
    out["_rows"] = dict(vrows=vrows, rcode=rcode, nib=nib, w=w, exc=exc)   # for the tables derived from these
    return out


def rot_perm(k, step):
    """index i of a depth-k table -> its index in the copy rotated at consumption step `step`: that step's symbol (bits
    2(k-1-step) of i) moves to the lowest two bits, the symbols below it move up by one"""
    i = np.arange(4 ** k, dtype=np.int64)
    sh = 2 * (k - 1 - step)
    return ((i >> (sh + 2)) << (sh + 2)) | ((i & ((1 << sh) - 1)) << 2) | ((i >> sh) & 3)


def rotated(tab, k, rot_first, copies):
    """the rotated copies of steps rot_first .. rot_first+copies-1, back to back"""
    out = np.empty((copies * 4 ** k,) + tab.shape[1:], dtype=tab.dtype)
    for j in range(copies):
        out[j * 4 ** k + rot_perm(k, rot_first + j)] = tab
    return out


# ------------------------------------------------------------------------------------------------ a PAM pair's tables
def pair_tables(st, k, v_rem, code):
    """the pair table of a strand (st = strand_tables(...)) as dict(tab, c16, ctx, rowid, n_slots) plus what the spaced
    table is derived from"""
    r = st["_rows"]
    vrows, rcode, nib, w = r["vrows"], r["rcode"], r["nib"][r["vrows"]], r["w"][r["vrows"]].astype(np.int64)
    near = np.zeros(vrows.shape[0], dtype=bool)           # a symbol outside A,C,G,T (or the text start) nearer than v_rem
    for j in range(v_rem):
        near |= ((nib >> np.uint64(4 * j)) & np.uint64(15)) > 3
    sel = (((w >> (2 * (v_rem - 2))) & 15) == code) & ~near
    rows, ent, ww = vrows[sel], rcode[sel], w[sel]
    order = np.lexsort((rows, ent))                        # by entry, interval order within one
    rows, ent, ww = rows[order], ent[order], ww[order]
    size = 4 ** k
    cnt = np.bincount(ent, minlength=size)
    big = cnt >= PT_BIG
    slots = cnt + big
    start = np.concatenate([[0], np.cumsum(slots)[:-1]])
    n_slots = int(slots.sum())
    sets = np.zeros(size, dtype=U32)
    for p in range(6):
        sets |= _or_bits(size, ent, 4 * p + ((ww >> (2 * p)) & 3))
    one = np.zeros(size, dtype=np.int64)
    one[ent] = ww & 0x3FFFFFF                              # read where cnt == 1 only
    filt = np.where(cnt == 1, one, np.where(cnt > 1, sets.astype(np.int64), 0))
    tab = np.zeros((size, 2), dtype=U32)
    tab[:, 0] = start
    tab[:, 1] = np.minimum(cnt, PT_BIG) | (filt << 6)
    # the row arrays: rows behind their entry's start (behind the header slot of a big entry)
    within = np.arange(rows.shape[0]) - np.concatenate([[0], np.cumsum(cnt)[:-1]])[ent]
    slot = start[ent] + big[ent] + within
    c16 = np.zeros(n_slots + 32, dtype=np.uint16)          # 64 zero bytes behind the rows
    octx = np.zeros(n_slots, dtype=U32)
    rowid = np.zeros(n_slots, dtype=U32)
    c16[slot] = ww & 0xFFFF
    octx[slot] = ww
    rowid[slot] = rows
    rowid[start[big]] = cnt[big]                           # header slot {0, 0, count}
    return dict(tab=tab, c16=c16, ctx=octx, rowid=rowid, n_slots=n_slots, _slot=slot, _ent=ent, _w=ww, _cnt=cnt)


def deep_table(t, st, k, P, kb, code):
    """the deep table: for every kb-symbol index i (symbol y of the entry at bits 2(kb-1-y)) and base x under the PAM's N, the
    interval of the rows whose suffix starts - read left to right in the text - with symbols kb-1 .. 0 of i, then x, then the
    complements 3-c0, 3-c1 of the pair (c0 = code & 3, c1 = code >> 2).  -> uint32[4^kb * 4, 4]; the first row of an entry
    without rows is set to 0 (nothing reads it)"""
    assert P == 3 and kb >= k - P
    sa = st["sa"].astype(np.int64)
    n = sa.shape[0]
    depth = kb + 3
    code_d, valid_d = kmer_codes(t, depth)                 # first text symbol lowest: symbol kb-1 of i ... symbol 0, x, pair
    c0, c1 = code & 3, (code >> 2) & 3
    tail = ((3 - c0) << (2 * (kb + 1))) | ((3 - c1) << (2 * (kb + 2)))
    rows = np.nonzero(valid_d[sa] & ((code_d[sa] >> (2 * (kb + 1))) == (tail >> (2 * (kb + 1)))))[0]
    cd = code_d[sa[rows]]
    x = (cd >> (2 * kb)) & 3
    i = np.zeros(rows.shape[0], dtype=np.int64)
    for y in range(kb):                                    # symbol y of the entry is the text symbol kb-1-y of the window
        i |= ((cd >> (2 * (kb - 1 - y))) & 3) << (2 * (kb - 1 - y))
    idx = 4 * i + x
    size = 4 ** kb * 4
    cnt = np.bincount(idx, minlength=size)
    first = np.zeros(size, dtype=np.int64)
    first[idx[::-1]] = rows[::-1]
    # the depth-k interval an entry descends from: the last k symbols of its window
    parent = np.zeros(size, dtype=np.int64)
    e = np.arange(size, dtype=np.int64)
    ei, ex = e >> 2, e & 3
    parent = ((3 - c1) << (2 * (k - 1))) | ((3 - c0) << (2 * (k - 2))) | (ex << (2 * (k - 3)))
    for y in range(k - P):
        parent = parent | (((ei >> (2 * (kb - 1 - y))) & 3) << (2 * (k - 1 - P - y)))
    pflag = (st["ptab"][:, 1] >> U32(31)).astype(bool)[parent]
    flag = (cnt > 0) & (pflag | (cnt > DEEP_MAX_ROWS))
    w = st["_rows"]["w"][rows]
    z, ww = pair_masks(size, idx, w, (0, 2, 4, 6))
    out = np.zeros((size, 4), dtype=U32)
    out[:, 0] = np.where(cnt > 0, first, 0)
    out[:, 1] = cnt.astype(U32) | (flag.astype(U32) << U32(31))
    out[:, 2] = np.where(flag, 0, z)
    out[:, 3] = np.where(flag, 0, ww)
    return out


def spaced_table(pt, k, x_len, g, rem, d):
    """the spaced table of a pair table pt: (keys, rows) sorted by key with rows[:, 0] = slot in the row arrays and
    rows[:, 1] = O symbols << rem | key & mask(rem), and sp_off[t] = the first row whose key's top d bits are >= t.
    key = X << 2g | the nearest g context symbols; X = the entry index's highest 2 x_len bits, O its other bits"""
    obits = 2 * (k - x_len)
    ent, slot, w = pt["_ent"], pt["_slot"], pt["_w"]
    key = ((ent >> obits) << (2 * g)) | (w & ((1 << (2 * g)) - 1))
    pay = ((ent & ((1 << obits) - 1)) << rem) | (key & ((1 << rem) - 1))
    order = np.lexsort((pay, slot, key))
    key, rows = key[order], np.stack([slot[order], pay[order]], axis=1).astype(U32)
    off = np.searchsorted(key >> rem, np.arange((1 << d) + 1), side="left").astype(U32)
    return key, rows, off


# ------------------------------------------------------------------------------------------------ comparison helpers
class TableMismatch(AssertionError):
    pass


def compare_exact(name, strand, got, want):
    """every entry of `got` equals `want`; raises TableMismatch naming the array, the strand and the first differing index"""
    if want is None or got is None:
        if not (want is None and got is None):
            raise TableMismatch(f"{name}, strand {strand}: the device {'holds' if want is None else 'lacks'} an array "
                                f"the model {'lacks' if want is None else 'holds'}")
        return
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        raise TableMismatch(f"{name}, strand {strand}: shape {got.shape} on the device, {want.shape} in the model")
    bad = got != want
    if bad.any():
        i = np.argwhere(bad)[0]
        at = tuple(int(v) for v in i)
        raise TableMismatch(f"{name}, strand {strand}: first difference at index {at[0]}"
                            + (f" word {at[1]}" if len(at) > 1 else "")
                            + f": device {int(got[at]):#x}, model {int(want[at]):#x} ({int(bad.sum())} entries differ)")


def check_mask_soundness(name, strand, tab, index, w, nib, offsets):
    """the property that loses hits when broken, by itself: for every occurrence (table index, context word w, class
    nibbles nib) and each of the four offsets whose two symbols are A,C,G,T the pair's bit is set in the entry's masks"""
    masks = tab[:, 2].astype(np.uint64) | (tab[:, 3].astype(np.uint64) << np.uint64(32))
    for j, o in enumerate(offsets):
        true = ((((nib >> np.uint64(4 * o)) & np.uint64(15)) < 4) & (((nib >> np.uint64(4 * o + 4)) & np.uint64(15)) < 4))
        bit = (16 * j + ((w.astype(np.int64) >> (2 * o)) & 15)).astype(np.uint64)
        miss = true & (((masks[index] >> bit) & np.uint64(1)) == 0)
        if miss.any():
            i = int(np.nonzero(miss)[0][0])
            raise TableMismatch(f"{name}, strand {strand}: entry at index {int(index[i])} lacks mask bit {int(bit[i])} "
                                f"(pair {j}) of one of its rows ({int(miss.sum())} bits missing)")


def check_strictly_ascending(name, strand, a):
    if a is None:
        return
    a = np.asarray(a).astype(np.int64)
    bad = np.nonzero(a[1:] <= a[:-1])[0]
    if bad.size:
        raise TableMismatch(f"{name}, strand {strand}: not strictly ascending at index {int(bad[0]) + 1}")


def compare_rotated(name, strand, got, tab, k, rot_first, copies):
    """copy j of `got` is `tab` under the permutation of step rot_first + j"""
    if copies == 0:
        return compare_exact(name, strand, got, None)
    compare_exact(name, strand, got, rotated(tab, k, rot_first, copies))


def compare_spaced(name, strand, got_rows, got_off, want_key, want_rows, want_off, rem):
    """sp_off entry by entry; sp_rows as sorted groups: the device's rows, keyed by the bucket sp_off puts them in and the key
    bits they carry, must be in key order and be the model's rows, each exactly once"""
    compare_exact(name + ".sp_off", strand, got_off, want_off)
    compare_exact(name + ".sp_rows (shape)", strand, np.zeros(got_rows.shape), np.zeros(want_rows.shape))
    m = got_rows.shape[0]
    bucket = np.searchsorted(got_off.astype(np.int64), np.arange(m), side="right") - 1
    key = (bucket << rem) | (got_rows[:, 1].astype(np.int64) & ((1 << rem) - 1))
    bad = np.nonzero(key[1:] < key[:-1])[0]
    if bad.size:
        raise TableMismatch(f"{name}.sp_rows, strand {strand}: keys not in order at index {int(bad[0]) + 1}")
    order = np.lexsort((got_rows[:, 1], got_rows[:, 0], key))
    compare_exact(name + ".sp_rows (keys)", strand, key[order], want_key)
    compare_exact(name + ".sp_rows", strand, got_rows[order], want_rows)
