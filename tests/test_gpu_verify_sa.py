"""gs_index_verify_sa (gs_verify.hip: k_v_permutation, k_v_full, k_v_order) against tests/sa_model.py, the same rules in numpy:
every field of every report EQUAL to the model's for the same (text, array, samples, seed) - on correct arrays, on arrays
that are permutations in the wrong order (the handle is built from them: GenomeIndex.build(text, sa_fwd=..., sa_rev=...)), and
on a correct index held against another text (the only way to a BWT symbol that differs).  Every-row mode and sampled mode,
both strands, rows at the Occ block's and the thread block's seams, the step limit and the N-run skip at sizes that reach
them.  Arrays that are no permutation never reach the verifier's kernels: gs_index_build_with_sa refuses them, which is what
is tested.  Last, the importer of the reference's index files at a size where its sampled check sees one pair in 256: one
damaged suffix-array sample must still be refused.  GPU only."""
import os
from importlib import import_module

import numpy as np
import pytest

import sa_model as sm
from sdsl_walk import walk

api = import_module("guidescan-cli_amd.api")

pytestmark = pytest.mark.gpu

GS_ERR_ARG, GS_ERR_UNSUPPORTED, GS_ERR_FORMAT = 1, 3, 6
TEXTS_DIFFER = ".reverse is not the index of the reverse complement of .forward's text"      # the importer's refusals
WRONG_ORDER = "the index file's suffix array samples do not order its text"
FIELDS = ("rows", "not_permutation", "sampled", "out_of_order", "undecided", "bwt_mismatch")


def modes(n):
    """(samples, seed): every row; every pair by direct comparison; 1,000 sampled pairs under two seeds"""
    return [("all", 1), (n - 1, 1), (1000, 1), (1000, 2)]


def model_report(text, sa, samples, seed, strand, built_text=None):
    if samples == "all":
        return sm.every_row_report(text, sa, built_text=built_text, strand=strand)
    return sm.direct_report(text, sa, samples, seed, built_text=built_text, strand=strand)


def assert_reports_equal(gidx, text, want, what):
    """both strands in every mode; want(strand, samples, seed) -> the model's report"""
    for strand in (0, 1):
        for samples, seed in modes(text.shape[0] + 1):
            got = gidx.verify_sa(text, strand=strand, samples=samples, seed=seed)
            model = want(strand, samples, seed)
            print(f"[verify_sa] {what} strand {strand} samples {samples} seed {seed}: gpu {got} model {model}")
            assert sorted(got) == sorted(FIELDS)
            assert got == model, (what, strand, samples, seed)


class Base:
    """the shared text, the model's arrays of both strands, and the model's reports of the correct reverse strand (every
    mutation below leaves that strand alone: computed once)"""

    def __init__(self):
        self.text = sm.base_text()
        self.n = self.text.shape[0] + 1
        self.sa = [sm.suffix_array(self.text), sm.suffix_array(sm.reverse_complement(self.text))]
        self.isa = np.argsort(self.sa[0])
        self._true = {}

    def true_report(self, strand, samples, seed):
        key = (strand, samples, seed)
        if key not in self._true:
            self._true[key] = model_report(self.text, self.sa[strand], samples, seed, strand)
        return dict(self._true[key])


@pytest.fixture(scope="module")
def base():
    return Base()


def swapped(sa, a, b):
    m = sa.copy()
    m[[a, b]] = m[[b, a]]
    return m


def mutate(kind, base):
    sa, n, isa = base.sa[0], base.n, base.isa
    if kind == "none":
        return sa.copy()
    if kind == "neighbours_at_a_third":
        return swapped(sa, n // 3, n // 3 + 1)
    if kind == "rows_0_1":
        return swapped(sa, 0, 1)
    if kind == "last_pair":
        return swapped(sa, n - 2, n - 1)
    if kind == "occ_block_seam":
        return swapped(sa, 127, 128)
    if kind == "thread_block_seam":
        return swapped(sa, 255, 256)
    if kind == "distant_rows":
        return swapped(sa, n // 5, 4 * (n // 5))
    if kind == "rotate_64":
        m = sa.copy()
        m[20_000:20_064] = np.roll(sa[20_000:20_064], 1)
        return m
    if kind == "tandem_group":       # two copies of the repeat at one phase: 9,495 symbols alike
        return swapped(sa, int(isa[12_500]), int(isa[12_505]))
    if kind == "n_group":
        return swapped(sa, int(isa[5_100]), int(isa[5_101]))
    if kind == "reversed":
        m = sa.copy()
        m[1:] = sa[1:][::-1]
        return m
    raise ValueError(kind)


MUTATIONS = ["none", "neighbours_at_a_third", "rows_0_1", "last_pair", "occ_block_seam", "thread_block_seam", "distant_rows",
             "rotate_64", "tandem_group", "n_group", "reversed"]


def test_the_builders_arrays_are_the_models(base):
    gidx = api.GenomeIndex.build(base.text, device=0)
    try:
        for strand in (0, 1):
            assert np.array_equal(gidx.suffix_array(strand), base.sa[strand]), strand
    finally:
        gidx.close()


@pytest.mark.parametrize("kind", MUTATIONS)
def test_reports_equal_the_model_on_permuted_arrays(kind, base):
    m = mutate(kind, base)
    assert sm.bitmap_count(m, base.n) == 0                                   # still a permutation
    full = sm.every_row_report(base.text, m)
    if kind == "none":
        assert full == dict(rows=base.n, not_permutation=0, sampled=base.n - 1, out_of_order=0, undecided=0, bwt_mismatch=0)
    else:   # the model itself finds the mutation: one that happened to be harmless cannot pass as "caught"
        assert full["out_of_order"] >= 1 and not np.array_equal(m, base.sa[0]), (kind, full)
    if kind == "reversed":   # the counters at scale - by direct comparison: the every-row rule takes the order of what follows
        # two suffixes from the array itself, reversed as well, and so finds the few pairs whose first symbols differ
        assert sm.direct_report(base.text, m, base.n - 1, 1)["out_of_order"] > base.n // 2
    if kind == "tandem_group":
        a, b = int(base.isa[12_500]), int(base.isa[12_505])
        assert abs(a - b) == 1 and (base.text[12_500:21_995] == base.text[12_505:22_000]).all()
        # here, where the walks are longest, the GPU's sampled reports are held to the plain symbol-by-symbol walk as well
        # (a quarter of 1,000 samples fall into the repeat's rows; every pair that way would take a minute)
        for seed in (1, 2):
            assert sm.direct_report(base.text, m, 1000, seed, plain=True) == sm.direct_report(base.text, m, 1000, seed)

    def want(strand, samples, seed):
        if strand == 1:
            return base.true_report(strand, samples, seed)
        return model_report(base.text, m, samples, seed, 0)

    gidx = api.GenomeIndex.build(base.text, device=0, sa_fwd=m, sa_rev=base.sa[1])
    try:
        assert np.array_equal(gidx.suffix_array(0), m)
        assert_reports_equal(gidx, base.text, want, kind)
    finally:
        gidx.close()


def other_text(kind, base):
    """(the text to verify against, the position changed)"""
    t = base.text.copy()
    if kind == "A_to_C":
        # the row that holds text[p] as its BWT symbol is isa[p + 1]: not row n-1, which sampled mode never looks at
        p = next(int(p) for p in np.flatnonzero(t == ord("A")) if p > 30_000 and base.isa[p + 1] != base.n - 1)
        t[p] = ord("C")
    elif kind == "C_to_Y":           # a base where the index holds one, a byte of the extra class in the text
        p = next(int(p) for p in np.flatnonzero(t == ord("C")) if p > 31_000 and base.isa[p + 1] != base.n - 1)
        t[p] = ord("Y")
    elif kind == "N_to_R_in_the_run":
        p = 5_150
        assert t[p] == ord("N")
        t[p] = ord("R")
    elif kind == "first_base":
        p = 0
        t[p] = ord("G") if t[p] != ord("G") else ord("T")
    elif kind == "last_base":
        p = t.shape[0] - 1
        assert t[p] == ord("N")
        t[p] = ord("A")
    else:
        raise ValueError(kind)
    return t, p


@pytest.fixture(scope="module")
def true_index(base):
    gidx = api.GenomeIndex.build(base.text, device=0, sa_fwd=base.sa[0], sa_rev=base.sa[1])
    yield gidx
    gidx.close()


@pytest.mark.parametrize("kind", ["A_to_C", "C_to_Y", "N_to_R_in_the_run", "first_base", "last_base"])
def test_a_correct_index_against_another_text(kind, base, true_index):
    text, p = other_text(kind, base)
    assert int((text != base.text).sum()) == 1
    full = [sm.every_row_report(text, base.sa[s], built_text=base.text, strand=s) for s in (0, 1)]
    if kind == "N_to_R_in_the_run":          # the same BWT class: only the order rule can speak
        assert full[0]["bwt_mismatch"] == full[1]["bwt_mismatch"] == 0
        assert full[0]["out_of_order"] >= 1
    else:
        assert full[0]["bwt_mismatch"] == full[1]["bwt_mismatch"] == 1
    if kind in ("A_to_C", "C_to_Y"):         # ... and seen by the direct comparison of all pairs as well
        assert sm.direct_report(text, base.sa[0], base.n - 1, 1, built_text=base.text)["bwt_mismatch"] == 1

    def want(strand, samples, seed):
        return model_report(text, base.sa[strand], samples, seed, strand, built_text=base.text)

    assert_reports_equal(true_index, text, want, kind)


def test_a_text_of_another_length_is_refused(base, true_index):
    for text in (base.text[:-1], np.concatenate([base.text, base.text[:1]])):
        for samples in ("all", 1000):
            with pytest.raises(api.GsError) as e:
                true_index.verify_sa(text, strand=0, samples=samples)
            assert e.value.status == GS_ERR_ARG


def test_step_limit_on_one_symbol():
    """'A' * 70,000, every pair by direct comparison: the pair (r, r+1) is decided at step r, so pairs 65,536 .. 69,999 are
    not (4,464 of them; tests/test_sa_model.py derives it).  T * 70,000 on the reverse strand: the same."""
    text = np.full(70_000, ord("A"), dtype=np.uint8)
    sa = sm.suffix_array(text)
    model = sm.direct_report(text, sa, 70_000, 1)
    assert model == dict(rows=70_001, not_permutation=0, sampled=70_000, out_of_order=0, undecided=4_464, bwt_mismatch=0)
    # (the reverse strand's text is one symbol too: the same array, the same walks, the same report -
    # tests/test_sa_model.py runs the model on it)
    gidx = api.GenomeIndex.build(text, device=0)
    try:
        for strand in (0, 1):
            assert np.array_equal(gidx.suffix_array(strand), sa)
            got = gidx.verify_sa(text, strand=strand, samples=70_000, seed=1)
            print(f"[verify_sa] one symbol strand {strand}: gpu {got} model {model}")
            assert got == model, strand
            assert got["undecided"] == 4_464 and got["out_of_order"] == 0 and got["sampled"] == 70_000
            assert gidx.verify_sa(text, strand=strand, samples="all") == sm.every_row_report(text, sa, strand=strand)
    finally:
        gidx.close()


def long_run_text():
    """200,000 symbols, one run of 70,001 N - more than the step limit, so only the skip decides its rows - and a second
    run that ends the text"""
    rng = np.random.default_rng(11)
    t = sm.as_text("ACGT")[rng.integers(0, 4, 200_000)]
    t[50_000:120_001] = sm.N
    t[-7:] = sm.N
    return t


def test_runs_of_n_longer_than_the_step_limit():
    text = long_run_text()
    n = text.shape[0] + 1
    sas = [sm.suffix_array(text), sm.suffix_array(sm.reverse_complement(text))]
    clean = dict(rows=n, not_permutation=0, sampled=n - 1, out_of_order=0, undecided=0, bwt_mismatch=0)
    gidx = api.GenomeIndex.build(text, device=0)
    try:
        for strand in (0, 1):
            assert np.array_equal(gidx.suffix_array(strand), sas[strand])
            model = sm.direct_report(text, sas[strand], n - 1, 1, strand=strand)
            assert model == clean                       # (without the skip: thousands of pairs undecided)
            got = gidx.verify_sa(text, strand=strand, samples=n - 1, seed=1)
            print(f"[verify_sa] long run strand {strand}: gpu {got} model {model}")
            assert got == model, strand
    finally:
        gidx.close()
    # two rows of the N group swapped, 30,000 and 30,001 symbols into the long run: the first wrong pair that goes
    # through the skip
    isa = np.argsort(sas[0])
    a, b = int(isa[80_000]), int(isa[80_001])
    assert abs(a - b) == 1
    m = swapped(sas[0], a, b)
    gidx = api.GenomeIndex.build(text, device=0, sa_fwd=m, sa_rev=sas[1])
    try:
        for samples in ("all", n - 1):
            model = model_report(text, m, samples, 1, 0)
            assert model["out_of_order"] >= 1 and model["undecided"] == 0, model
            got = gidx.verify_sa(text, strand=0, samples=samples, seed=1)
            print(f"[verify_sa] long run, N group swapped, samples {samples}: gpu {got} model {model}")
            assert got == model, samples
    finally:
        gidx.close()


def not_a_permutation(sa, kind, n):
    m = sa.copy()
    m[1_000] = {"duplicate": m[2_000], "value_n": n, "value_ffffffff": 0xFFFFFFFF}[kind]
    return m


@pytest.mark.parametrize("kind", ["duplicate", "value_n", "value_ffffffff"])
def test_arrays_that_are_no_permutation_are_refused_at_the_build(kind, base):
    """for either strand's array.  (The refusal's message counts the bad rows, but GS_ERR_ARG's text is the status's own:
    the binding shows no count to hold against the model's, which is 1 in each case.)"""
    bad = [not_a_permutation(base.sa[s], kind, base.n) for s in (0, 1)]
    assert sm.bitmap_count(bad[0], base.n) == sm.bitmap_count(bad[1], base.n) == 1
    for fwd, rev in ((bad[0], base.sa[1]), (base.sa[0], bad[1])):
        with pytest.raises(api.GsError) as e:
            api.GenomeIndex.build(base.text, device=0, sa_fwd=fwd, sa_rev=rev)
        assert e.value.status == GS_ERR_ARG


# ---- the importer: one damaged suffix-array sample in a 2^24-symbol genome ---------------------------------------------

def sample_vector(buf):
    """(bit offset of sample 0 in buf, width, samples) of the file's SA sample vector (an int_vector<0>: bits, width, words)"""
    sec, _ = walk(buf)
    s0, _ = sec["sa_samples"]
    bits = int.from_bytes(buf[s0:s0 + 8], "little")
    width = buf[s0 + 8]
    return 8 * (s0 + 9), width, bits // width


def get_sample(buf, at, width, j):
    b = at + j * width
    return (int.from_bytes(buf[b >> 3:(b >> 3) + 9], "little") >> (b & 7)) & ((1 << width) - 1)


def set_sample(buf, at, width, j, v):
    b = at + j * width
    word = int.from_bytes(buf[b >> 3:(b >> 3) + 9], "little")
    mask = ((1 << width) - 1) << (b & 7)
    buf[b >> 3:(b >> 3) + 9] = ((word & ~mask) | (v << (b & 7))).to_bytes(9, "little")


REPEAT_COPIES, REPEAT_UNIT, REPEAT_EVERY, REPEAT_AT = 130, 600, 1_000, 1_000_000


def repeat_text():
    """(2^24 random ACGT symbols with 130 copies of one 600-symbol unit, a copy every 1,000 symbols; the copies' starts)"""
    rng = np.random.default_rng(25)
    text = sm.as_text("ACGT")[rng.integers(0, 4, 1 << 24)]
    starts = REPEAT_AT + REPEAT_EVERY * np.arange(REPEAT_COPIES)
    unit = text[starts[0]:starts[0] + REPEAT_UNIT].copy()
    for s in starts:
        text[s:s + REPEAT_UNIT] = unit
    return text, starts


def swapped_walks(isa, pa, pb, symbols):
    """{row: value} the importer reconstructs where the samples at text positions pa and pb have their values swapped and
    both walks are `symbols` long: the rows of pa - k and pb - k, k < symbols, hold each other's value"""
    changed = {}
    for k in range(symbols):
        changed[int(isa[pa - k])] = pb - k
        changed[int(isa[pb - k])] = pa - k
    return changed


def sampled_check_finds(t, sa, changed, strand):
    """out_of_order of sa_model.direct_report(.., 65536, the importer's seed) on the array `sa with changed`, where sa is the
    strand's true suffix array and t its text without 'N': only a sampled pair that holds a changed row can be out of order,
    so only those are walked"""
    assert sm.N not in t
    n = len(t)
    found = 0
    for r in sm.sampled_rows(n, 65536, 0x5D51 + strand):
        if r in changed or r + 1 in changed:
            found += sm.compare_pair(t, {}, changed.get(r, int(sa[r])), changed.get(r + 1, int(sa[r + 1]))) == "bad"
    return found


def repeat_sample_pairs(text, starts, true_sa):
    """[(strand, a, b, symbols, changed)]: SA samples a and b (rows 64a, 64b) of the strand's file that hold the same place in two
    copies of the repeat, and whose LF walks - `symbols` long, down to the next sample below in the text - stay inside the
    copies: the two walks spell the same symbols, so with the two values swapped the importer reconstructs the SAME text
    and a permutation in which 2 * symbols rows name the other copy (changed: {row: the value it then holds}).  Why such
    pairs exist: the suffixes at one place
    of the 130 copies are 130 consecutive rows, in the same order of copies at every place (LF keeps the order of rows
    with one symbol), so two copies 64 rows apart are sampled at the same places.  Three pairs per strand."""
    n = text.shape[0] + 1
    pairs = []
    for strand in (0, 1):
        t = sm.strand_text(text, strand)
        sa = true_sa[strand].astype(np.int64)
        at = starts if strand == 0 else (n - 1) - (starts + REPEAT_UNIT)      # the copies' starts in this strand's text
        assert all((t[s:s + REPEAT_UNIT] == t[at[0]:at[0] + REPEAT_UNIT]).all() for s in at)
        isa = np.empty(n, dtype=np.int64)
        isa[sa] = np.arange(n)
        sampled_at = np.sort(sa[::64])
        found = 0
        for o in range(REPEAT_UNIT - 200, 200, -1):   # (200 symbols and more still shared after the place: one group of rows)
            rows = np.sort(isa[at + o])
            if rows[-1] - rows[0] != REPEAT_COPIES - 1:
                continue
            hit = rows[rows % 64 == 0]
            if hit.shape[0] < 2:
                continue
            ra, rb = int(hit[0]), int(hit[1])
            pa, pb = int(sa[ra]), int(sa[rb])
            ga = pa - int(sampled_at[np.searchsorted(sampled_at, pa) - 1])
            gb = pb - int(sampled_at[np.searchsorted(sampled_at, pb) - 1])
            if ga != gb or ga > o - 100 or ga < 8:
                continue
            assert (t[pa - ga:pa] == t[pb - ga:pb]).all()
            pairs.append((strand, ra // 64, rb // 64, ga, swapped_walks(isa, pa, pb, ga)))
            found += 1
            if found == 3:
                break
        assert found == 3, (strand, found)
    return pairs


def saved_pair(tmp_path, text):
    """the text's index written as <tmp_path>/g.forward and g.reverse, and opened again: (the two files' bytes, the built
    handle's suffix arrays); the undamaged pair must open and hold those arrays"""
    built = api.GenomeIndex.build(text, device=0)
    try:
        built.save_sdsl(text, tmp_path / "g")
        true_sa = [built.suffix_array(s) for s in (0, 1)]
    finally:
        built.close()
    again = api.GenomeIndex.open_sdsl(tmp_path / "g", device=0)
    try:
        for s in (0, 1):
            assert np.array_equal(again.suffix_array(s), true_sa[s]), s
    finally:
        again.close()
    return {sfx: (tmp_path / f"g.{sfx}").read_bytes() for sfx in ("forward", "reverse")}, true_sa


def open_with_two_samples_swapped(tmp_path, files, true_sa, trial, strand, a, b):
    """samples a and b of the strand's file swapped, the other file as it is: (trial, file, a, b, status - 0: it opened -,
    the refusal's message or how many rows of the opened handle hold a wrong suffix_array value)"""
    sfx, other = (("forward", "reverse"), ("reverse", "forward"))[strand]
    buf = bytearray(files[sfx])
    at, width, ns = sample_vector(buf)
    n = true_sa[strand].shape[0]
    assert ns == (n + 63) // 64 and (1 << width) >= n
    va, vb = get_sample(buf, at, width, a), get_sample(buf, at, width, b)
    assert va == true_sa[strand][64 * a] and vb == true_sa[strand][64 * b]       # these are the samples
    set_sample(buf, at, width, a, vb)
    set_sample(buf, at, width, b, va)
    assert get_sample(buf, at, width, a) == vb and get_sample(buf, at, width, b) == va
    changed = int((np.frombuffer(buf, np.uint8) != np.frombuffer(files[sfx], np.uint8)).sum())
    assert 1 <= changed <= 2 * ((width + 7) // 8 + 1)
    (tmp_path / f"d{trial}.{sfx}").write_bytes(buf)
    os.link(tmp_path / f"g.{other}", tmp_path / f"d{trial}.{other}")
    try:
        g = api.GenomeIndex.open_sdsl(tmp_path / f"d{trial}", device=0)
    except api.GsError as e:
        outcome = (trial, sfx, a, b, e.status, str(e))
    else:
        try:
            differ = [int((g.suffix_array(s) != true_sa[s]).sum()) for s in (0, 1)]
        finally:
            g.close()
        outcome = (trial, sfx, a, b, 0, f"opened; rows whose suffix_array value differs: {differ}")
    os.unlink(tmp_path / f"d{trial}.{sfx}")
    os.unlink(tmp_path / f"d{trial}.{other}")
    print("[importer] trial %d: .%s samples %d <-> %d: status %d (%s)" % outcome)
    return outcome


def assert_all_refused(outcomes, message, trials=6):
    opened = [o for o in outcomes if o[4] == 0]
    assert not opened, f"damaged files that opened and answer from a wrong suffix array: {opened}"
    assert [o[4] for o in outcomes] == [GS_ERR_FORMAT] * trials, outcomes
    assert all(message in o[5] for o in outcomes), outcomes              # which check refuses them (DESIGN.md §3 says so)


def test_importer_refuses_one_damaged_sample_at_2_to_the_24(tmp_path):
    """two SA samples of one strand's file swapped (the reconstructed array stays a permutation), six trials, three per
    file: each must be refused with GS_ERR_FORMAT.  In a random genome a sample's value places its walk's symbols somewhere
    else in the text, so the two files' texts no longer agree and the order check is not reached."""
    rng = np.random.default_rng(24)
    text = sm.as_text("ACGT")[rng.integers(0, 4, 1 << 24)]
    files, true_sa = saved_pair(tmp_path, text)
    outcomes = []
    for trial in range(6):
        a, b = (int(x) for x in rng.choice(np.arange(1, ((1 << 24) + 1 + 63) // 64), 2, replace=False))
        outcomes.append(open_with_two_samples_swapped(tmp_path, files, true_sa, trial, trial // 3, a, b))
    assert_all_refused(outcomes, TEXTS_DIFFER)


def test_importer_refuses_samples_swapped_between_copies_of_a_repeat(tmp_path):
    """the damage that keeps the text: the two samples hold the same place in two copies of a 130-fold repeat, so both
    files still spell the genome and only the order of 2 * (24 .. 126) rows is wrong - 4 pairs of neighbouring rows out of
    2^24 by the every-row rule.  Sampling 65,536 pairs sees one pair in 256: by the model's rule for the sampled mode, with
    the importer's seeds, it finds one wrong pair in trials 0 and 2 and none in trials 1, 3, 4, 5 (asserted below) - with
    that check alone those four files open and answer with the other copy's coordinates.  The importer checks every row
    where the strand has its inverse array: all six must be refused, for the order."""
    text, starts = repeat_text()
    files, true_sa = saved_pair(tmp_path, text)
    pairs = repeat_sample_pairs(text, starts, true_sa)
    assert [p[0] for p in pairs] == [0, 0, 0, 1, 1, 1]
    texts = [sm.strand_text(text, s).tobytes() for s in (0, 1)]
    assert [sampled_check_finds(texts[s], true_sa[s], changed, s) for s, _, _, _, changed in pairs] == [1, 0, 1, 0, 0, 0]
    outcomes = [open_with_two_samples_swapped(tmp_path, files, true_sa, trial, strand, a, b)
                for trial, (strand, a, b, _, _) in enumerate(pairs)]
    assert_all_refused(outcomes, WRONG_ORDER)


def tandem_sample_pair(base):
    """(a, b, the array reconstructed with the two values swapped): two samples of the forward file, 64 rows apart, that hold
    the same phase of base_text's tandem repeat with walks of one length inside it - swapped, the text stays"""
    t, sa, isa = base.text, base.sa[0], base.isa
    sampled_at = np.sort(sa[::64])
    for pa in range(19_000, 14_000, -1):
        ra = int(isa[pa])
        if ra % 64 or ra + 64 >= base.n:
            continue
        pb = int(sa[ra + 64])
        if not 14_000 < pb < 19_000 or (pa - pb) % 5:
            continue
        ga = pa - int(sampled_at[np.searchsorted(sampled_at, pa) - 1])
        gb = pb - int(sampled_at[np.searchsorted(sampled_at, pb) - 1])
        if ga != gb or not 8 <= ga < 1_000:
            continue
        assert (t[pa - ga:pa] == t[pb - ga:pb]).all()
        m = sa.copy()
        for row, value in swapped_walks(isa, pa, pb, ga).items():
            m[row] = value
        return ra // 64, ra // 64 + 1, m
    raise AssertionError("no such pair of samples")


def test_importer_keeps_the_sampled_check_on_a_handle_without_the_inverse_array(tmp_path, monkeypatch, base):
    """GS_NO_ISA: the every-row rule cannot run (GS_ERR_UNSUPPORTED from verify_sa) and the importer keeps its 65,536 sampled
    pairs, which at this size are every pair: the good files open with the same arrays, and a file with two samples swapped
    inside the tandem repeat - the text stays, the order is wrong - is refused for the order"""
    files, true_sa = saved_pair(tmp_path, base.text)
    a, b, m = tandem_sample_pair(base)
    for report in (sm.every_row_report(base.text, m), sm.direct_report(base.text, m, 65536, 0x5D51)):
        assert report["not_permutation"] == 0 and report["out_of_order"] >= 1, report
    monkeypatch.setenv("GS_NO_ISA", "1")
    g = api.GenomeIndex.open_sdsl(tmp_path / "g", device=0)
    try:
        for s in (0, 1):
            assert np.array_equal(g.suffix_array(s), base.sa[s]), s
        with pytest.raises(api.GsError) as e:
            g.verify_sa(base.text, strand=0, samples="all")
        assert e.value.status == GS_ERR_UNSUPPORTED
        assert g.verify_sa(base.text, strand=0, samples=base.n - 1) == base.true_report(0, base.n - 1, 1)
    finally:
        g.close()
    assert_all_refused([open_with_two_samples_swapped(tmp_path, files, true_sa, 0, 0, a, b)], WRONG_ORDER, trials=1)
