"""tests/index_tables_model.py held to account (no GPU): on small texts the model equals brute force - sorted() suffixes,
startswith for intervals, a literal loop over occurrences for flags, masks and selected rows -, and the comparison helpers
the GPU test relies on report a single corrupted entry with its index."""
import itertools
from importlib import import_module

import numpy as np
import pytest

import index_tables_model as M
import sa_model

api = import_module("guidescan-cli_amd.api")

ACGT = "ACGT"


def texts():
    rng = np.random.default_rng(11)
    out = []
    for n, extra in ((60, ""), (200, "N"), (300, "NRYacgt"), (257, "NN")):
        alphabet = ACGT * 6 + extra
        out.append("".join(alphabet[i] for i in rng.integers(0, len(alphabet), n)))
    out.append("A" * 150 + "".join(ACGT[i] for i in rng.integers(0, 4, 100)) + "N" + "AC" * 20)   # 63 rows and more
    out.append("ACGTACGTTGCA")
    return out


def brute_sa(t):
    b = bytes(t)
    return np.array(sorted(range(len(b)), key=lambda i: b[i:]), dtype=np.int64)


def cls(ch):
    return "ACGTN".index(ch) if ch in "ACGTN" else 5


def brute_context(s, p):
    """class nibbles 1..16 before position p, nearest first"""
    return [cls(s[p - j]) if p >= j else 6 for j in range(1, 17)]


def kmer_index(km):
    return sum(ACGT.index(c) << (2 * i) for i, c in enumerate(km))


def brute_strand(s, sa, k, mask_off):
    """ptab, ctx, exception rows of text s (str, no sentinel) by literal loops"""
    n = len(s) + 1
    suffixes = [s[p:] for p in sa]
    offs = M.mask_offsets(mask_off)
    ptab = np.zeros((4 ** k, 4), dtype=np.uint32)
    ctx = np.zeros(n, dtype=np.uint32)
    exc_row, exc_sym = [], []
    for r, p in enumerate(sa):
        nb = brute_context(s, int(p))
        ctx[r] = sum((c if c < 4 else 0) << (2 * j) for j, c in enumerate(nb))
    for km in map("".join, itertools.product(ACGT, repeat=k)):
        rows = [r for r in range(n) if suffixes[r].startswith(km)]
        e = ptab[kmer_index(km)]
        e[0] = rows[0] if rows else 0
        e[1] = len(rows)
        assert rows == list(range(rows[0], rows[0] + len(rows))) if rows else True
        for r in rows:
            nb = brute_context(s, int(sa[r]))
            if any(c > 3 for c in nb):
                e[1] |= 1 << 31
                exc_row.append(r)
                exc_sym.append(sum(c << (4 * j) for j, c in enumerate(nb)))
            for j, o in enumerate(offs):
                v = (nb[o] if nb[o] < 4 else 0) | ((nb[o + 1] if nb[o + 1] < 4 else 0) << 2)
                e[2 + j // 2] |= 1 << (16 * (j % 2) + v)
    order = np.argsort(exc_row)
    return ptab, ctx, np.array(exc_row, dtype=np.uint32)[order], np.array(exc_sym, dtype=np.uint64)[order]


@pytest.mark.parametrize("k", (2, 3, 4))
@pytest.mark.parametrize("ti", range(len(texts())))
def test_strand_tables_equal_brute_force(ti, k):
    s = texts()[ti]
    for strand in (0, 1):
        t = sa_model.strand_text(sa_model.as_text(s), strand)
        ss = bytes(t[:-1]).decode()
        sa = brute_sa(t)
        assert np.array_equal(sa, sa_model.suffix_array(t[:-1]))
        mask_off = M.default_mask_off(k) if ti % 2 else (1 | (3 << 4) | (9 << 8) | (14 << 12))
        m = M.strand_tables(t, sa, k, mask_off)
        ptab, ctx, er, es = brute_strand(ss, sa, k, mask_off)
        M.compare_exact("ptab", strand, m["ptab"], ptab)
        M.compare_exact("ctx", strand, m["ctx"], ctx)
        M.compare_exact("ctx16", strand, m["ctx16"], (ctx & 0xFFFF).astype(np.uint16))
        M.compare_exact("exc_row", strand, m["exc_row"], er if er.size else None)
        M.compare_exact("exc_sym", strand, m["exc_sym"], es if es.size else None)
        assert [int(m["isa"][p]) for p in sa] == list(range(len(sa)))
        # Occ blocks: header counts and planes row by row
        n = len(sa)
        bwt = [ss[p - 1] if p else "\0" for p in sa]
        seen = [0, 0, 0, 0]
        for r in range(128 * m["layout"]["blocks"]):
            b, wd, bit = r >> 7, (r >> 5) & 3, r & 31
            blk = m["blocks"][b]
            if r % 128 == 0:
                assert list(blk[:4]) == seen, (r, list(blk[:4]), seen)
            c = cls(bwt[r]) if r < n else 5
            got = ((blk[4 + wd] >> bit) & 1, (blk[8 + wd] >> bit) & 1, (blk[12 + wd] >> bit) & 1)
            assert got == ((c & 1, c >> 1, 0) if c < 4 else (0, 0, 1)), (r, got, c)
            if c < 4:
                seen[c] += 1
        # runs of the symbols outside A,C,G,T, per symbol, with the closing entry
        runs = {}
        for r, c in enumerate(bwt):
            if c in ACGT or c == "\0":
                continue
            if r and bwt[r - 1] == c:
                runs[c][-1][1] += 1
            else:
                runs.setdefault(c, []).append([r, 1])
        xs, xc = [], []
        for c in sorted(runs):
            seg = m["xr_seg"][ord(c)]
            assert (int(seg[0]), int(seg[1])) == (len(xs), len(runs[c]))
            xs += [r for r, _ in runs[c]] + [0xFFFFFFFF]
            xc += list(np.concatenate([[0], np.cumsum([ln for _, ln in runs[c]])]))
        assert all(not m["xr_seg"][c].any() for c in range(256) if chr(c) not in runs)
        assert ([] if m["xr_start"] is None else list(m["xr_start"])) == xs
        assert ([] if m["xr_cum"] is None else list(m["xr_cum"])) == xc and m["layout"]["xr_entries"] == len(xs)
        if "N" in runs:
            assert list(m["run_start"]) == [r for r, _ in runs["N"]] and m["layout"]["nruns"] == len(runs["N"])
            assert list(m["run_cum"]) == list(np.concatenate([[0], np.cumsum([ln for _, ln in runs["N"]])]))
        else:
            assert m["run_start"] is None and m["run_cum"] is None and m["layout"]["nruns"] == 0
        full = ss + "\0"
        for c in range(256):
            assert int(m["C256"][c]) == (sum(1 for x in full if ord(x) < c) if chr(c) in full else 0)
        lay = m["layout"]
        assert [lay["C0"], lay["C1"], lay["C2"], lay["C3"], lay["CN"]] == [sum(1 for x in full if x < b) for b in "ACGTN"]
        assert lay["has_n"] == int("N" in ss) and lay["n_exc"] == er.size
        # without context arrays: counts and first rows as before, masks all ones, no flag
        bare = M.strand_tables(t, sa, k, ctx=False)
        assert np.array_equal(bare["ptab"][:, 0], ptab[:, 0]) and np.array_equal(bare["ptab"][:, 1], ptab[:, 1] & 0x7FFFFFFF)
        assert (bare["ptab"][:, 2:] == 0xFFFFFFFF).all() and bare["ctx"] is None and bare["isa"] is None


def test_strand_text_complements_lower_case_as_the_index_does():
    """the other strand's text is the library's reverse complement (sequences.cxx:14-26: a<->t, c<->g too) - what the
    index is built from; the suffix-array verifier once left lower case as it was and reported a correct array of a
    soft-masked text as out of order"""
    synth = import_module("guidescan-cli_amd.synth")
    text = sa_model.as_text("ACGTacgtNRYnry")
    assert bytes(sa_model.strand_text(text, 1)[:-1]) == bytes(synth.reverse_complement_bytes(text)) == b"yrnYRNacgtACGT"


@pytest.mark.parametrize("k", range(2, 9))
def test_rotation_is_a_bijection_and_the_library_agrees(k):
    for step in range(k):
        perm = M.rot_perm(k, step)
        assert np.array_equal(np.sort(perm), np.arange(4 ** k))
        idx = np.arange(4 ** k) if k <= 5 else np.random.default_rng(k).integers(0, 4 ** k, 300)
        assert [api.rot_index(int(i), k, step) for i in idx] == [int(perm[i]) for i in idx]
        # the symbol of the step in the lowest bits, the other symbols in their order
        i = int(idx[-1])
        sym = [(i >> (2 * (k - 1 - p))) & 3 for p in range(k)]
        moved = [sym[p] for p in range(k) if p != step] + [sym[step]]
        assert int(perm[i]) == sum(c << (2 * (k - 1 - p)) for p, c in enumerate(moved))
    tab = np.arange(4 ** k * 2, dtype=np.uint32).reshape(-1, 2)
    rot = M.rotated(tab, k, 1, k - 2) if k > 2 else None
    if rot is not None:
        for j in range(k - 2):
            assert np.array_equal(rot[j * 4 ** k + M.rot_perm(k, 1 + j)], tab)


def brute_pair(s, sa, k, v_rem, code):
    """tab and the row arrays by a literal loop over every k-mer's rows"""
    n = len(s) + 1
    suffixes = [s[p:] for p in sa]
    tab = np.zeros((4 ** k, 2), dtype=np.uint32)
    per_entry = {}
    for km in map("".join, itertools.product(ACGT, repeat=k)):
        rows = []
        for r in range(n):
            if not suffixes[r].startswith(km):
                continue
            nb = brute_context(s, int(sa[r]))
            if any(c > 3 for c in nb[:v_rem]) or (nb[v_rem - 2] | (nb[v_rem - 1] << 2)) != code:
                continue
            rows.append((r, sum((c if c < 4 else 0) << (2 * j) for j, c in enumerate(nb))))
        per_entry[kmer_index(km)] = rows
    c16, ctx, rowid = [], [], []
    for i in range(4 ** k):
        rows = per_entry[i]
        tab[i, 0] = len(rowid)
        if len(rows) >= 63:
            c16.append(0), ctx.append(0), rowid.append(len(rows))
        if len(rows) == 1:
            filt = rows[0][1] & 0x3FFFFFF
        else:
            filt = 0
            for _, w in rows:
                for p in range(6):
                    filt |= 1 << (4 * p + ((w >> (2 * p)) & 3))
        tab[i, 1] = min(len(rows), 63) | (filt << 6)
        for r, w in rows:
            c16.append(w & 0xFFFF), ctx.append(w), rowid.append(r)
    return tab, np.array(c16 + [0] * 32, dtype=np.uint16), np.array(ctx, dtype=np.uint32), np.array(rowid, dtype=np.uint32), per_entry


def brute_deep(s, sa, k, kb, code, strand_ptab, max_rows):
    n = len(s) + 1
    suffixes = [s[p:] for p in sa]
    c0, c1 = code & 3, code >> 2
    out = np.zeros((4 ** kb * 4, 4), dtype=np.uint32)
    for i in range(4 ** kb):
        sym = [(i >> (2 * (kb - 1 - y))) & 3 for y in range(kb)]
        for x in range(4):
            pat = "".join(ACGT[c] for c in sym[::-1]) + ACGT[x] + ACGT[3 - c0] + ACGT[3 - c1]
            rows = [r for r in range(n) if suffixes[r].startswith(pat)]
            e = out[4 * i + x]
            if not rows:
                continue
            assert rows == list(range(rows[0], rows[0] + len(rows)))
            blind = bool(strand_ptab[kmer_index(pat[-k:]), 1] >> 31) or len(rows) > max_rows
            e[0], e[1] = rows[0], len(rows) | (int(blind) << 31)
            if not blind:
                for r in rows:
                    nb = [c if c < 4 else 0 for c in brute_context(s, int(sa[r]))]
                    for j, o in enumerate((0, 2, 4, 6)):
                        e[2 + j // 2] |= 1 << (16 * (j % 2) + (nb[o] | (nb[o + 1] << 2)))
    return out


PAIR_SHAPES = [(2, 2, 0b1010), (3, 4, 0b1010), (3, 16, 0b0010), (4, 3, 0), (4, 9, 0b0101), (4, 2, 0b1111)]


@pytest.mark.parametrize("k,v_rem,code", PAIR_SHAPES)
@pytest.mark.parametrize("ti", range(len(texts())))
def test_pair_deep_and_spaced_tables_equal_brute_force(ti, k, v_rem, code, monkeypatch):
    s = texts()[ti]
    monkeypatch.setattr(M, "DEEP_MAX_ROWS", 3)   # the 4,096-row rule at a size these texts reach
    big_seen = False
    for strand in (0, 1):
        t = sa_model.strand_text(sa_model.as_text(s), strand)
        ss = bytes(t[:-1]).decode()
        sa = brute_sa(t)
        st = M.strand_tables(t, sa, k)
        pt = M.pair_tables(st, k, v_rem, code)
        tab, c16, ctx, rowid, per_entry = brute_pair(ss, sa, k, v_rem, code)
        M.compare_exact("tab", strand, pt["tab"], tab)
        M.compare_exact("c16", strand, pt["c16"], c16)
        M.compare_exact("ctx", strand, pt["ctx"], ctx)
        M.compare_exact("rowid", strand, pt["rowid"], rowid)
        assert pt["n_slots"] == rowid.shape[0]
        big_seen |= any(len(v) >= 63 for v in per_entry.values())
        if k >= 3:
            for kb in (k - 3, k - 2, k - 1):
                if kb < 1:
                    continue
                deep = M.deep_table(t, st, k, 3, kb, code)
                M.compare_exact(f"deep kb={kb}", strand, deep, brute_deep(ss, sa, k, kb, code, st["ptab"], 3))
        # spaced: every row once, payload and offsets by a literal loop
        for x_len, g, d in ((1, 2, 3), (k - 1, 1, 2), (1, 5, 8)):
            if x_len < 1:
                continue
            rem = 2 * (x_len + g) - d
            if rem < 0:
                continue
            key, rows, off = M.spaced_table(pt, k, x_len, g, rem, d)
            want = []
            for i in range(4 ** k):
                base = int(tab[i, 0]) + (len(per_entry[i]) >= 63)
                for j, (r, w) in enumerate(per_entry[i]):
                    kk = ((i >> (2 * (k - x_len))) << (2 * g)) | (w & (4 ** g - 1))
                    want.append((kk, base + j, ((i & (4 ** (k - x_len) - 1)) << rem) | (kk & ((1 << rem) - 1))))
            want.sort()
            assert [(int(a), int(b[0]), int(b[1])) for a, b in zip(key, rows)] == want
            assert list(off) == [sum(1 for w_ in want if (w_[0] >> rem) < tt) for tt in range(2 ** d + 1)]
            M.compare_spaced("spaced", strand, rows, off, key, rows, off, rem)
    if ti == 4 and v_rem <= 4 and code == 0:
        assert big_seen, "the text planted for 63 rows and more does not reach them"


def model_world():
    """one model of everything, for the corruption cases"""
    rng = np.random.default_rng(5)
    s = "".join((ACGT * 8 + "N")[i] for i in rng.integers(0, 33, 3000)) + "A" * 100
    t = sa_model.strand_text(sa_model.as_text(s), 0)
    sa = sa_model.suffix_array(t[:-1])
    k = 4
    st = M.strand_tables(t, sa, k)
    pt = M.pair_tables(st, k, 3, 0)
    assert (pt["_cnt"] >= 63).any() and st["layout"]["n_exc"] > 2
    deep = M.deep_table(t, st, k, 3, 2, 0)
    rem = 3
    key, rows, off = M.spaced_table(pt, k, 2, 2, rem, 5)
    return dict(t=t, sa=sa, k=k, st=st, pt=pt, deep=deep, sp=(key, rows, off, rem))


@pytest.fixture(scope="module")
def world():
    return model_world()


def reported(exc, name, index):
    msg = str(exc.value)
    assert name in msg and f"index {index}" in msg, msg


def test_helpers_report_a_cleared_mask_bit(world):
    st = world["st"]
    tab = st["ptab"].copy()
    i = int(np.nonzero(tab[:, 2])[0][7])
    bit = int(tab[i, 2]).bit_length() - 1
    tab[i, 2] &= ~np.uint32(1 << bit)
    with pytest.raises(M.TableMismatch) as e:
        M.compare_exact("ptab", 0, tab, st["ptab"])
    reported(e, "ptab", i)
    r = st["_rows"]
    offs = M.mask_offsets(st["layout"]["mask_off"])
    M.check_mask_soundness("ptab", 0, st["ptab"], r["rcode"], r["w"][r["vrows"]], r["nib"][r["vrows"]], offs)
    # the bit of a pair that holds an N read as A is no loss: find an entry whose cleared bit belongs to true symbols
    with pytest.raises(M.TableMismatch) as e:
        full = st["ptab"].copy()
        true_i = int(r["rcode"][np.nonzero(~r["exc"][r["vrows"]])[0][0]])
        w0 = int(r["w"][r["vrows"]][np.nonzero(~r["exc"][r["vrows"]])[0][0]])
        full[true_i, 2] &= ~np.uint32(1 << ((w0 >> (2 * offs[0])) & 15))
        M.check_mask_soundness("ptab", 0, full, r["rcode"], r["w"][r["vrows"]], r["nib"][r["vrows"]], offs)
    reported(e, "ptab", true_i)


def test_helpers_report_a_count_off_by_one(world):
    tab = world["st"]["ptab"].copy()
    tab[37, 1] += 1
    with pytest.raises(M.TableMismatch) as e:
        M.compare_exact("ptab", 1, tab, world["st"]["ptab"])
    reported(e, "ptab, strand 1", 37)


def test_helpers_report_two_exception_rows_swapped(world):
    er = world["st"]["exc_row"].copy()
    er[[4, 5]] = er[[5, 4]]
    with pytest.raises(M.TableMismatch) as e:
        M.check_strictly_ascending("exc_row", 0, er)
    reported(e, "exc_row", 5)
    with pytest.raises(M.TableMismatch) as e:
        M.compare_exact("exc_row", 0, er, world["st"]["exc_row"])
    reported(e, "exc_row", 4)
    M.check_strictly_ascending("exc_row", 0, world["st"]["exc_row"])


def test_helpers_report_a_rotated_entry_moved(world):
    k, tab = world["k"], world["st"]["ptab"]
    rot = M.rotated(tab, k, 1, 2)
    M.compare_rotated("ptab_rot", 0, rot, tab, k, 1, 2)
    a = 4 ** k + 9
    b = next(j for j in range(a + 1, 2 * 4 ** k) if not np.array_equal(rot[j], rot[a]))
    rot[[a, b]] = rot[[b, a]]
    with pytest.raises(M.TableMismatch) as e:
        M.compare_rotated("ptab_rot", 0, rot, tab, k, 1, 2)
    reported(e, "ptab_rot", a)


def test_helpers_report_a_dropped_pair_row_and_a_header_count(world):
    pt = world["pt"]
    rowid = np.delete(pt["rowid"], 11)
    with pytest.raises(M.TableMismatch) as e:
        M.compare_exact("rowid", 0, rowid, pt["rowid"])
    assert "shape" in str(e.value)
    rowid = pt["rowid"].copy()          # the same length, the row gone and the rest moved up
    rowid[11:-1] = rowid[12:]
    with pytest.raises(M.TableMismatch) as e:
        M.compare_exact("rowid", 0, rowid, pt["rowid"])
    reported(e, "rowid", 11)
    i = int(np.nonzero(pt["_cnt"] >= 63)[0][0])
    head = int(pt["tab"][i, 0])
    assert int(pt["rowid"][head]) == int(pt["_cnt"][i]) and pt["c16"][head] == 0 and pt["ctx"][head] == 0
    rowid = pt["rowid"].copy()
    rowid[head] -= 1
    with pytest.raises(M.TableMismatch) as e:
        M.compare_exact("rowid", 0, rowid, pt["rowid"])
    reported(e, "rowid", head)


def test_helpers_report_an_sp_off_entry_and_a_deep_flag(world):
    key, rows, off, rem = world["sp"]
    M.compare_spaced("slot 0", 0, rows, off, key, rows, off, rem)
    shuffled = rows.copy()              # rows of equal key may come in any order
    same = np.nonzero(key[1:] == key[:-1])[0]
    assert same.size
    shuffled[[same[0], same[0] + 1]] = shuffled[[same[0] + 1, same[0]]]
    M.compare_spaced("slot 0", 0, shuffled, off, key, rows, off, rem)
    bad = off.copy()
    bad[13] += 1
    with pytest.raises(M.TableMismatch) as e:
        M.compare_spaced("slot 0", 0, rows, bad, key, rows, off, rem)
    reported(e, "sp_off", 13)
    lost = rows.copy()
    lost[5] = lost[6]                   # one row twice, one missing
    with pytest.raises(M.TableMismatch):
        M.compare_spaced("slot 0", 0, lost, off, key, rows, off, rem)
    deep = world["deep"].copy()
    i = int(np.nonzero(deep[:, 1])[0][3])
    deep[i, 1] ^= np.uint32(1 << 31)
    with pytest.raises(M.TableMismatch) as e:
        M.compare_exact("deep", 0, deep, world["deep"])
    reported(e, "deep", i)
