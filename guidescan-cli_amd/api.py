"""ctypes binding of libgsamd.so (include/guidescan_amd.h) plus the thin host layer
that mirrors the reference's per-guide pipeline interface
(include/genomics/process.hpp:35-158) over the batch C-ABI.

The product path is the HIP library only: there is no CPU fallback.  Importing
this module without the built library raises; calling it without a GPU returns
GS_ERR_DEVICE from the library, surfaced as GsError.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np

PKG = Path(__file__).resolve().parent
# GS_LIB_PATH: another build of the same library (kernel tuning experiments); default in-tree
LIB_PATH = Path(os.environ.get("GS_LIB_PATH", str(PKG / "libgsamd.so")))

GS_FLAG_PAM_AT_START = 1
GS_FLAG_FAITHFUL_WALK = 2
GS_FLAG_COUNT_REQUESTS = 4
GS_FLAG_RAW_COUNTS = 8
GS_FLAG_NO_NEW_TABLES = 16


class GsError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"gs_status {status}: {msg}")
        self.status = status


class GsHit(C.Structure):
    _fields_ = [("pos", C.c_int64), ("key", C.c_uint64)]


HIT_DTYPE = np.dtype([("pos", "<i8"), ("key", "<u8")])
HIT_EX_DTYPE = np.dtype([("pos", "<i8"), ("seq", "S32"), ("mismatches", "<u4"),
                         ("dna_bulges", "u1"), ("rna_bulges", "u1"), ("index", "u1"), ("seq_len", "u1")])


class GsResultView(C.Structure):
    _fields_ = [("n_guides", C.c_uint64), ("n_hits", C.c_uint64),
                ("guide_offsets", C.POINTER(C.c_uint64)), ("hits", C.POINTER(GsHit)),
                ("n_ext", C.c_uint64), ("n_matches", C.c_uint64),
                ("ms_search", C.c_float), ("ms_total", C.c_float),
                ("n_unsupported", C.c_uint64), ("guide_flags", C.POINTER(C.c_uint8)),
                ("raw_hits", C.POINTER(C.c_uint32))]


class GsSaReport(C.Structure):
    _fields_ = [("rows", C.c_uint64), ("not_permutation", C.c_uint64), ("sampled", C.c_uint64),
                ("out_of_order", C.c_uint64), ("undecided", C.c_uint64), ("bwt_mismatch", C.c_uint64)]


class GsGenomeStructure(C.Structure):
    _fields_ = [("chr_names", C.POINTER(C.c_char_p)), ("chr_lengths", C.POINTER(C.c_uint64)),
                ("n_chr", C.c_uint32)]


class GsKmer(C.Structure):
    _fields_ = [("id", C.c_char_p), ("sequence", C.c_char_p), ("pam", C.c_char_p),
                ("sense_positive", C.c_int)]


GS_TEXT_SAM = 0x100
GS_TEXT_COMPLETE = 0x200
GS_TEXT_BAM = 0x800    # gs_format_device / gs_enumerate_text: BAM alignment blocks in place of SAM lines
GS_TEXT_BGZF = 0x1000  # with GS_TEXT_BAM: the blocks as BGZF members
GS_TEXT_FEATURES = 0x4000
GS_DECODE_NO_HEADER = 0x400
GS_DECODE_BAM_END = 0x2000  # gs_decode_bam: the data ends with these members (a cut record is an error)
GS_DECODE_FEATURES_ONLY = 0x8000  # with GS_TEXT_FEATURES | GS_TEXT_COMPLETE: only the rows that have a feature


class GsDecodeBatch(C.Structure):
    _fields_ = [("n", C.c_uint64), ("ids", C.c_void_p), ("id_off", C.c_void_p), ("seqs", C.c_void_p),
                ("seq_off", C.c_void_p), ("reverse", C.c_void_p), ("chr", C.c_void_p), ("pos0", C.c_void_p),
                ("hex", C.c_void_p), ("hex_off", C.c_void_p)]


class GsKmersReport(C.Structure):
    _fields_ = [("n", C.c_uint64), ("L", C.c_uint64), ("P", C.c_uint64), ("n_lines", C.c_uint64),
                ("bad_kind", C.c_uint32), ("pad", C.c_uint32), ("bad_line", C.c_uint64), ("bad_row", C.c_uint64),
                ("bad_off", C.c_uint64), ("bad_len", C.c_uint64), ("bad_text", C.c_void_p), ("ms", C.c_double * 8)]


class GsRegionsReport(C.Structure):
    _fields_ = [("n_lines", C.c_uint64), ("n_intervals", C.c_uint64), ("n_groups", C.c_uint64),
                ("bad_kind", C.c_uint32), ("pad", C.c_uint32), ("bad_line", C.c_uint64), ("bad_len", C.c_uint64),
                ("bad_text", C.c_void_p)]


class GsSeqRule(C.Structure):
    _fields_ = [("gc_min", C.c_uint32), ("gc_max", C.c_uint32), ("max_run", C.c_uint32), ("n_motifs", C.c_uint32),
                ("motif_len", C.c_uint8 * 16), ("motif_set", (C.c_uint8 * 16) * 16)]


class GsControlsRule(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("first", C.c_uint64), ("n", C.c_uint64), ("max_candidates", C.c_uint64), ("round", C.c_uint64),
                ("L", C.c_uint32), ("n_alt", C.c_uint32), ("mismatches", C.c_uint32), ("flags", C.c_uint32),
                ("min_distance", C.c_uint32), ("pad", C.c_uint32), ("pam", C.c_char_p), ("alt_pams", C.c_char_p),
                ("seq_rule", C.POINTER(GsSeqRule)), ("id_prefix", C.c_char_p)]


class GsControlsReport(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("kept", "looked_at", "gc", "run", "motif", "targeting", "close", "last_counter", "rounds")] + \
               [("ms", C.c_double * 5)]


class GsPairRule(C.Structure):
    _fields_ = [("min_span", C.c_uint64), ("max_span", C.c_uint64), ("cut_offset", C.c_uint32), ("orientation", C.c_uint32),
                ("per_region", C.c_uint32), ("flags", C.c_uint32), ("min_specificity", C.c_float), ("pad", C.c_uint32)]


def build_library():
    subprocess.run(["make", "-s", "-C", str(PKG / "csrc")], check=True, timeout=3600)


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise ImportError(f"{LIB_PATH} is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(the HIP extension is mandatory; there is no CPU fallback)")
    L = C.CDLL(str(LIB_PATH))
    vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
    L.gs_index_build.restype = i32
    L.gs_index_build.argtypes = [vp, u64, i32, C.POINTER(vp)]
    L.gs_index_build_with_sa.restype = i32
    L.gs_index_build_with_sa.argtypes = [vp, u64, vp, vp, i32, C.POINTER(vp)]
    L.gs_index_open_sdsl.restype = i32
    L.gs_index_open_sdsl.argtypes = [C.c_char_p, i32, C.POINTER(vp)]
    L.gs_sdsl_extract_text.restype = i32
    L.gs_sdsl_extract_text.argtypes = [C.c_char_p, C.POINTER(vp), C.POINTER(u64)]
    L.gs_index_save_sa.restype = i32
    L.gs_index_save_sa.argtypes = [vp, vp, u64, C.c_char_p]
    L.gs_index_save_sdsl.restype = i32
    L.gs_index_save_sdsl.argtypes = [vp, vp, u64, C.c_char_p]
    L.gs_debug_sdsl_sections.restype = i32
    L.gs_debug_sdsl_sections.argtypes = [vp, C.POINTER(vp), C.POINTER(u64), C.POINTER(vp), C.POINTER(u64)]
    L.gs_debug_sdsl_export_scratch.restype = u64
    L.gs_debug_sdsl_export_scratch.argtypes = []
    L.gs_index_open_sa.restype = i32
    L.gs_index_open_sa.argtypes = [vp, u64, C.c_char_p, i32, C.POINTER(vp)]
    L.gs_index_close.argtypes = [vp]
    L.gs_index_genome_length.restype = u64
    L.gs_index_genome_length.argtypes = [vp]
    L.gs_index_device_bytes.restype = u64
    L.gs_index_device_bytes.argtypes = [vp]
    L.gs_enumerate.restype = i32
    L.gs_enumerate.argtypes = [vp, vp, u64, u32, vp, u32, C.c_char_p, u32, u32, u32, C.POINTER(vp)]
    L.gs_enumerate_device.restype = i32
    L.gs_enumerate_device.argtypes = [vp, vp, u64, u32, vp, u32, C.c_char_p, u32, u32, u32, vp,
                                      C.POINTER(vp), C.POINTER(vp), C.POINTER(GsResultView)]
    L.gs_result_get.restype = i32
    L.gs_result_get.argtypes = [vp, C.POINTER(GsResultView)]
    L.gs_result_free.argtypes = [vp]
    L.gs_decode_sequence.restype = i32
    L.gs_decode_sequence.argtypes = [C.c_char_p, u32, u32, u32, u64, C.c_char_p]
    L.gs_rank_bwt4.restype = i32
    L.gs_rank_bwt4.argtypes = [vp, i32, vp, u64, vp]
    L.gs_resolve.restype = i32
    L.gs_resolve.argtypes = [vp, i32, vp, u64, vp]
    L.gs_index_meta.restype = i32
    L.gs_index_meta.argtypes = [vp, i32, vp, C.POINTER(u64)]
    L.gs_index_copy_sa.restype = i32
    L.gs_index_copy_sa.argtypes = [vp, i32, vp]
    L.gs_index_last_counters.restype = i32
    L.gs_index_last_counters.argtypes = [vp, vp]
    L.gs_index_last_launch.restype = i32
    L.gs_index_last_launch.argtypes = [vp, vp]
    L.gs_index_last_sharing.restype = i32
    L.gs_index_last_sharing.argtypes = [vp, vp]
    L.gs_index_prepare.restype = i32
    L.gs_index_prepare.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32]
    L.gs_index_set_option.restype = i32
    L.gs_index_set_option.argtypes = [vp, C.c_char_p, C.c_char_p]
    L.gs_index_get_option.restype = i32
    L.gs_index_get_option.argtypes = [vp, C.c_char_p, C.c_char_p, u64]
    L.gs_index_lock.restype = i32
    L.gs_index_lock.argtypes = [vp]
    L.gs_index_unlock.restype = i32
    L.gs_index_unlock.argtypes = [vp]
    L.gs_index_verify_sa.restype = i32
    L.gs_index_verify_sa.argtypes = [vp, i32, vp, u64, u64, u64, C.POINTER(GsSaReport)]
    L.gs_calculate_cfd.restype = C.c_float
    L.gs_calculate_cfd.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p]
    L.gs_format_guide.restype = i32
    L.gs_format_guide.argtypes = [C.POINTER(GsGenomeStructure), C.POINTER(GsKmer), vp, u64, u32, u32,
                                  C.c_int64, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.gs_format_guide_scored.restype = i32
    L.gs_format_guide_scored.argtypes = [C.POINTER(GsGenomeStructure), C.POINTER(GsKmer), vp, u64, u32, u32,
                                         C.c_int64, C.c_float, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.gs_format_guides_scored.restype = i32
    L.gs_format_guides_scored.argtypes = [C.POINTER(GsGenomeStructure), vp, u64, vp, vp, vp, vp, u32, u32, C.c_int64,
                                          C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.gs_format_header.restype = i32
    L.gs_format_header.argtypes = [C.POINTER(GsGenomeStructure), u32, C.POINTER(vp),
                                   C.POINTER(C.c_size_t)]
    L.gs_free.argtypes = [vp]
    L.gs_enumerate_bulges.restype = i32
    L.gs_enumerate_bulges.argtypes = [vp, vp, u64, u32, vp, u32, C.c_char_p, u32, u32, u32, u32, u32,
                                      C.POINTER(vp)]
    L.gs_result_ex_get.restype = i32
    L.gs_result_ex_get.argtypes = [vp, C.POINTER(u64), C.POINTER(vp), C.POINTER(vp)]
    L.gs_result_ex_free.argtypes = [vp]
    L.gs_result_ex_raw_hits.restype = i32
    L.gs_result_ex_raw_hits.argtypes = [vp, C.POINTER(vp)]
    L.gs_decode_sequence_ex.restype = i32
    L.gs_decode_sequence_ex.argtypes = [vp, C.c_char_p]
    L.gs_enumerate_general.restype = i32
    L.gs_enumerate_general.argtypes = [vp, vp, u64, u32, vp, u32, C.c_char_p, u32, u32, u32, u32, u32,
                                       C.POINTER(vp)]
    L.gs_enumerate_general_pams.restype = i32
    L.gs_enumerate_general_pams.argtypes = [vp, vp, u64, u32, vp, u32, C.c_char_p, vp, u32, u32, u32, u32, u32,
                                            C.POINTER(vp)]
    L.gs_debug_general_last.restype = i32
    L.gs_debug_general_last.argtypes = [vp, C.POINTER(u64)]
    L.gs_debug_bulge_last.restype = i32
    L.gs_debug_bulge_last.argtypes = [vp, C.POINTER(u64)]
    L.gs_debug_bulge_seeds.restype = i32
    L.gs_debug_bulge_seeds.argtypes = [C.c_char_p, u32, u32, u32, u32, u32, u32, u32, u32, vp, u64, C.POINTER(u64)]
    L.gs_debug_bulge_verify.restype = i32
    L.gs_debug_bulge_verify.argtypes = [u32, vp, u64, C.c_char_p, u32, C.c_char_p, u32, C.c_char_p, vp, u32, u32, u32, u32,
                                        u32, u32, vp, u64, C.POINTER(u64)]
    L.gs_index_last_guide_flags.restype = i32
    L.gs_index_last_guide_flags.argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
    L.gs_format_guide_ex.restype = i32
    L.gs_format_guide_ex.argtypes = [C.POINTER(GsGenomeStructure), C.POINTER(GsKmer), vp, u64, u32, u32,
                                     C.c_int64, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.gs_score_device.restype = i32
    L.gs_score_device.argtypes = [vp, vp, u64, u32, u32, u32, C.c_int64, C.POINTER(GsGenomeStructure), vp, vp,
                                  vp, vp, vp]
    L.gs_score.restype = i32
    L.gs_score.argtypes = [vp, vp, u64, u32, u32, u32, C.c_int64, C.POINTER(GsGenomeStructure), vp, vp, vp, vp]
    L.gs_format_device.restype = i32
    L.gs_format_device.argtypes = [vp, C.POINTER(GsGenomeStructure), vp, u64, u32, vp, u32, vp, vp, vp, vp, vp, vp, vp, u32, u32,
                                   C.c_int64, vp, C.POINTER(vp), C.POINTER(u64)]
    L.gs_enumerate_text.restype = i32
    L.gs_enumerate_text.argtypes = [vp, vp, u64, u32, vp, u32, C.c_char_p, u32, u32, u32, C.c_int64,
                                    C.POINTER(GsGenomeStructure), vp, vp, vp, vp, C.POINTER(vp), C.POINTER(u64),
                                    C.POINTER(GsResultView)]
    L.gs_index_last_text_offsets.restype = i32
    L.gs_index_last_text_offsets.argtypes = [vp, vp, u64]
    L.gs_kmers_generate.restype = i32
    L.gs_kmers_generate.argtypes = [i32, vp, u64, i32, C.c_char_p, u32, u32, vp, C.POINTER(vp)]
    L.gs_kmers_get.restype = i32
    L.gs_kmers_get.argtypes = [vp, i32, C.POINTER(u64), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                               C.POINTER(vp)]
    L.gs_kmers_free.argtypes = [vp]
    L.gs_format_device_ids.restype = i32
    L.gs_format_device_ids.argtypes = L.gs_format_device.argtypes
    L.gs_enumerate_text_device.restype = i32
    L.gs_enumerate_text_device.argtypes = [vp, vp, u64, u32, vp, u32, C.c_char_p, u32, u32, u32, C.c_int64,
                                           C.POINTER(GsGenomeStructure), vp, vp, vp, vp, C.POINTER(vp), C.POINTER(u64),
                                           C.POINTER(GsResultView), vp]
    L.gs_kmers_encode_ids.restype = i32
    L.gs_kmers_encode_ids.argtypes = [vp, C.c_char_p, C.c_char_p, vp]
    L.gs_kmers_get_ids.restype = i32
    L.gs_kmers_get_ids.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.gs_kmers_csv.restype = i32
    L.gs_kmers_csv.argtypes = [vp, C.c_char_p, C.c_char_p, C.POINTER(vp), C.POINTER(u64)]
    L.gs_kmers_concat.restype = i32
    L.gs_kmers_concat.argtypes = [vp, u32, C.POINTER(vp)]
    L.gs_decoder_open.restype = i32
    L.gs_decoder_open.argtypes = [i32, vp, u64, C.POINTER(GsGenomeStructure), vp, vp, C.POINTER(vp)]
    L.gs_decoder_close.argtypes = [vp]
    L.gs_decode_records.restype = i32
    L.gs_decode_records.argtypes = [vp, C.POINTER(GsDecodeBatch), u32, u64, C.POINTER(vp), C.POINTER(u64), C.POINTER(u64)]
    L.gs_decode_records_device.restype = i32
    L.gs_decode_records_device.argtypes = L.gs_decode_records.argtypes
    L.gs_decode_sam.restype = i32
    L.gs_decode_sam.argtypes = [vp, vp, u64, u32, u64, C.POINTER(vp), C.POINTER(u64), C.POINTER(u64)]
    L.gs_debug_repr_doubles.restype = i32
    L.gs_debug_repr_doubles.argtypes = [vp, u64, vp]
    L.gs_bgzf_compress_device.restype = i32
    L.gs_bgzf_compress_device.argtypes = [vp, vp, u64, vp, C.POINTER(vp), C.POINTER(u64)]
    L.gs_bgzf_compress.restype = i32
    L.gs_bgzf_compress.argtypes = [vp, vp, u64, C.POINTER(vp), C.POINTER(u64)]
    L.gs_bgzf_inflate.restype = i32
    L.gs_bgzf_inflate.argtypes = [i32, vp, u64, C.POINTER(vp), C.POINTER(u64)]
    L.gs_bgzf_inflate_device.restype = i32
    L.gs_bgzf_inflate_device.argtypes = [vp, vp, u64, u64, C.POINTER(vp), C.POINTER(u64), C.POINTER(u64)]
    L.gs_bgzf_inflate_base.restype = i32
    L.gs_bgzf_inflate_base.argtypes = [vp, u64, u64]
    L.gs_debug_inflate_member.restype = i32
    L.gs_debug_inflate_member.argtypes = [vp, u64, vp, u64, C.POINTER(u64), C.POINTER(u32)]
    L.gs_debug_bgzf_members.restype = i32
    L.gs_debug_bgzf_members.argtypes = [vp, u64, vp, vp, u64, C.POINTER(u64), C.POINTER(u32)]
    L.gs_decode_bam.restype = i32
    L.gs_decode_bam.argtypes = [vp, vp, u64, u64, vp, u32, u32, u64, C.POINTER(vp), C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    L.gs_decode_bam_device.restype = i32
    L.gs_decode_bam_device.argtypes = L.gs_decode_bam.argtypes
    L.gs_debug_decode_bam_last.restype = i32
    L.gs_debug_decode_bam_last.argtypes = [vp, vp, vp]
    L.gs_debug_huffman_lengths.restype = i32
    L.gs_debug_huffman_lengths.argtypes = [vp, u32, u32, vp]
    L.gs_debug_sp_float.restype = C.c_float
    L.gs_debug_sp_float.argtypes = [u32]
    L.gs_debug_decode_tables.restype = i32
    L.gs_debug_decode_tables.argtypes = [vp, vp]
    L.gs_fasta_parse.restype = i32
    L.gs_fasta_parse.argtypes = [i32, vp, u64, u32, C.POINTER(vp)]
    L.gs_fasta_parse_file.restype = i32
    L.gs_fasta_parse_file.argtypes = [i32, C.c_char_p, u32, C.POINTER(vp)]
    L.gs_fasta_parse_device.restype = i32
    L.gs_fasta_parse_device.argtypes = [i32, vp, u64, u32, vp, C.POINTER(vp)]
    L.gs_fasta_info.restype = i32
    L.gs_fasta_info.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    L.gs_fasta_records.restype = i32
    L.gs_fasta_records.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    L.gs_fasta_text.restype = i32
    L.gs_fasta_text.argtypes = [vp, i32, C.POINTER(vp)]
    L.gs_fasta_free.restype = None
    L.gs_fasta_free.argtypes = [vp]
    L.gs_decoder_open_fasta.restype = i32
    L.gs_decoder_open_fasta.argtypes = [i32, vp, C.POINTER(GsGenomeStructure), C.POINTER(vp)]
    L.gs_debug_fasta_tile_bytes.restype = u64
    L.gs_debug_fasta_tile_bytes.argtypes = []
    L.gs_debug_fasta_host.restype = i32
    L.gs_debug_fasta_host.argtypes = [vp, u64, u32, u64, C.POINTER(vp)]
    L.gs_debug_fasta_chunk_bytes.restype = u64
    L.gs_debug_fasta_chunk_bytes.argtypes = [u64]
    L.gs_debug_fasta_ms.restype = i32
    L.gs_debug_fasta_ms.argtypes = [vp, vp]
    L.gs_kmers_parse.restype = i32
    L.gs_kmers_parse.argtypes = [i32, vp, u64, C.POINTER(vp), C.POINTER(GsKmersReport)]
    L.gs_kmers_parse_file.restype = i32
    L.gs_kmers_parse_file.argtypes = [i32, C.c_char_p, C.POINTER(vp), C.POINTER(GsKmersReport)]
    L.gs_kmers_parse_device.restype = i32
    L.gs_kmers_parse_device.argtypes = [i32, vp, u64, vp, C.POINTER(vp), C.POINTER(GsKmersReport)]
    L.gs_debug_kmers_tile_bytes.restype = u64
    L.gs_debug_kmers_tile_bytes.argtypes = []
    L.gs_debug_kmers_chunk_bytes.restype = u64
    L.gs_debug_kmers_chunk_bytes.argtypes = [u64]
    L.gs_debug_kmers_host.restype = i32
    L.gs_debug_kmers_host.argtypes = [vp, u64, u64, C.POINTER(vp), C.POINTER(GsKmersReport)]
    pgs, f32 = C.POINTER(GsGenomeStructure), C.c_float
    L.gs_regions_parse.restype = i32
    L.gs_regions_parse.argtypes = [vp, u64, pgs, C.c_char_p, C.POINTER(vp), C.POINTER(GsRegionsReport)]
    L.gs_regions_parse_file.restype = i32
    L.gs_regions_parse_file.argtypes = [C.c_char_p, pgs, C.c_char_p, C.POINTER(vp), C.POINTER(GsRegionsReport)]
    L.gs_regions_info.restype = i32
    L.gs_regions_info.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    L.gs_regions_free.restype = None
    L.gs_regions_free.argtypes = [vp]
    L.gs_design_restrict.restype = i32
    L.gs_design_restrict.argtypes = [vp, u32, vp, vp, C.POINTER(vp)]
    L.gs_design_concat.restype = i32
    L.gs_design_concat.argtypes = [vp, u32, C.POINTER(vp)]
    L.gs_design_score.restype = i32
    L.gs_design_score.argtypes = [vp, vp, C.c_char_p, u32, u32, u32, C.c_int64, u64, vp]
    L.gs_design_select.restype = i32
    L.gs_design_select.argtypes = [vp, C.c_char_p, u32, f32, vp, C.POINTER(vp)]
    L.gs_design_rows.restype = i32
    L.gs_design_rows.argtypes = [vp, C.c_char_p, u32, f32, vp, C.POINTER(vp), C.POINTER(u64)]
    L.gs_design_get.restype = i32
    L.gs_design_get.argtypes = [vp, C.POINTER(u64)] + [C.POINTER(vp)] * 6
    L.gs_design_info.restype = i32
    L.gs_design_info.argtypes = [vp, C.POINTER(u64), C.POINTER(C.c_int)]
    L.gs_design_last_select.restype = i32
    L.gs_design_last_select.argtypes = [vp, vp]
    L.gs_design_free.restype = None
    L.gs_design_free.argtypes = [vp]
    L.gs_debug_design_host.restype = i32
    L.gs_debug_design_host.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, vp, C.c_char_p, u32, C.c_char_p, u32, f32,
                                       C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)]
    L.gs_regions_group_name.restype = i32
    L.gs_regions_group_name.argtypes = [vp, u64, C.POINTER(C.c_char_p)]
    L.gs_annot_build.restype = i32
    L.gs_annot_build.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.gs_annot_info.restype = i32
    L.gs_annot_info.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    L.gs_annot_free.restype = None
    L.gs_annot_free.argtypes = [vp]
    L.gs_debug_annot_entry_cap.restype = u64
    L.gs_debug_annot_entry_cap.argtypes = [u64]
    L.gs_annotate_device.restype = i32
    L.gs_annotate_device.argtypes = [vp, vp, pgs, u64, u32, u32, u32, vp, vp, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.gs_annotate.restype = i32
    L.gs_annotate.argtypes = [vp, vp, pgs, u64, u32, u32, u32, vp, vp, vp, C.POINTER(vp), C.POINTER(u64), vp]
    L.gs_debug_annotate_host.restype = i32
    L.gs_debug_annotate_host.argtypes = [vp, pgs, u64, u32, u32, u32, vp, vp, vp, C.POINTER(vp), C.POINTER(u64), vp]
    L.gs_index_set_annotation.restype = i32
    L.gs_index_set_annotation.argtypes = [vp, vp]
    L.gs_format_guides_features.restype = i32
    L.gs_format_guides_features.argtypes = [pgs, vp, u64, vp, vp, vp, vp, u32, u32, C.c_int64, vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.gs_format_guide_features.restype = i32
    L.gs_format_guide_features.argtypes = [pgs, vp, vp, u64, u32, u32, C.c_int64, f32, vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.gs_format_guide_ex_features.restype = i32
    L.gs_format_guide_ex_features.argtypes = [pgs, vp, vp, u64, u32, u32, C.c_int64, vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.gs_design_set_feature_rule.restype = i32
    L.gs_design_set_feature_rule.argtypes = [vp, vp, u32, u32]
    L.gs_design_get_feature_hits.restype = i32
    L.gs_design_get_feature_hits.argtypes = [vp, C.POINTER(vp)]
    L.gs_design_pairs.restype = i32
    L.gs_design_pairs.argtypes = [vp, C.c_char_p, C.POINTER(GsPairRule), vp, C.POINTER(vp), C.POINTER(vp)]
    L.gs_pairs_get.restype = i32
    L.gs_pairs_get.argtypes = [vp, C.POINTER(u64)] + [C.POINTER(vp)] * 8
    L.gs_pairs_rows.restype = i32
    L.gs_pairs_rows.argtypes = [vp, vp, C.POINTER(vp), C.POINTER(u64)]
    L.gs_pairs_last.restype = i32
    L.gs_pairs_last.argtypes = [vp, vp]
    L.gs_pairs_ms.restype = i32
    L.gs_pairs_ms.argtypes = [vp, vp]
    L.gs_pairs_free.restype = None
    L.gs_pairs_free.argtypes = [vp]
    L.gs_debug_pairs_host.restype = i32
    L.gs_debug_pairs_host.argtypes = [u64, vp, vp, vp, vp, vp, vp, u32, u32, u32, C.POINTER(GsPairRule), C.POINTER(vp)]
    L.gs_debug_pairs_chunk.restype = u64
    L.gs_debug_pairs_chunk.argtypes = [u64]
    L.gs_seq_rule_init.restype = i32
    L.gs_seq_rule_init.argtypes = [C.POINTER(GsSeqRule)]
    L.gs_seq_rule_add_motif.restype = i32
    L.gs_seq_rule_add_motif.argtypes = [C.POINTER(GsSeqRule), C.c_char_p, C.c_int]
    L.gs_kmers_filter.restype = i32
    L.gs_kmers_filter.argtypes = [vp, C.POINTER(GsSeqRule), vp, C.POINTER(vp), vp]
    L.gs_debug_kmers_filter_ms.restype = i32
    L.gs_debug_kmers_filter_ms.argtypes = [vp, vp]
    L.gs_debug_kmers_filter_host.restype = i32
    L.gs_debug_kmers_filter_host.argtypes = [vp, u64, u32, C.POINTER(GsSeqRule), vp, vp]
    L.gs_design_set_spacing.restype = i32
    L.gs_design_set_spacing.argtypes = [vp, u32, u32, u32]
    L.gs_design_last_spacing.restype = i32
    L.gs_design_last_spacing.argtypes = [vp, vp]
    L.gs_debug_design_space_ms.restype = i32
    L.gs_debug_design_space_ms.argtypes = [vp, C.POINTER(C.c_double)]
    L.gs_debug_design_host_spaced.restype = i32
    L.gs_debug_design_host_spaced.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, vp, C.c_char_p, u32, C.c_char_p, u32, f32, u32, u32, u32,
                                              C.POINTER(vp), C.POINTER(vp), C.POINTER(u64), vp]
    L.gs_debug_design_set_scores.restype = i32
    L.gs_debug_design_set_scores.argtypes = [vp, vp, vp]
    L.gs_controls_generate.restype = i32
    L.gs_controls_generate.argtypes = [vp, C.POINTER(GsControlsRule), vp, C.POINTER(vp), C.POINTER(GsControlsReport)]
    L.gs_controls_rows.restype = i32
    L.gs_controls_rows.argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
    L.gs_controls_counters.restype = i32
    L.gs_controls_counters.argtypes = [vp, C.POINTER(u64), C.POINTER(vp)]
    L.gs_debug_controls_host.restype = i32
    L.gs_debug_controls_host.argtypes = [C.POINTER(GsControlsRule), vp, u64, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64),
                                         C.POINTER(GsControlsReport)]
    L.gs_debug_controls_sequences.restype = i32
    L.gs_debug_controls_sequences.argtypes = [u64, u64, u64, u32, vp]
    L.gs_debug_controls_round.restype = u64
    L.gs_debug_controls_round.argtypes = [u64]
    L.gs_decoder_set_annotation.restype = i32
    L.gs_decoder_set_annotation.argtypes = [vp, vp]
    L.gs_debug_decode_annot_ms.restype = i32
    L.gs_debug_decode_annot_ms.argtypes = [vp, C.POINTER(C.c_double)]
    L.gs_status_string.restype = C.c_char_p
    L.gs_status_string.argtypes = [i32]
    L.gs_version.restype = C.c_char_p
    _lib = L
    return L


EXPORTS = ["gs_index_build", "gs_index_build_with_sa", "gs_index_open_sdsl", "gs_index_close",
           "gs_index_genome_length", "gs_index_device_bytes", "gs_enumerate", "gs_enumerate_device",
           "gs_result_get", "gs_result_free", "gs_decode_sequence", "gs_rank_bwt4", "gs_resolve",
           "gs_index_meta", "gs_index_copy_sa", "gs_calculate_cfd", "gs_status_string", "gs_version",
           "gs_format_guide", "gs_format_header", "gs_free", "gs_sdsl_extract_text",
           "gs_enumerate_bulges", "gs_result_ex_get", "gs_result_ex_free", "gs_decode_sequence_ex",
           "gs_format_guide_ex", "gs_score_device", "gs_score", "gs_kmers_generate", "gs_kmers_get",
           "gs_kmers_free", "gs_format_guide_scored", "gs_index_verify_sa", "gs_index_last_counters", "gs_index_last_launch", "gs_enumerate_general",
           "gs_index_last_guide_flags", "gs_enumerate_general_pams", "gs_index_save_sa", "gs_index_open_sa", "gs_format_guides_scored", "gs_result_ex_raw_hits",
           "gs_debug_seed_recipes", "gs_debug_choose_thresholds", "gs_debug_tile_plan", "gs_debug_search_form", "gs_debug_guide_descriptor", "gs_debug_general_last", "gs_index_lock", "gs_index_unlock",
           "gs_index_last_sharing", "gs_index_set_option", "gs_index_get_option", "gs_index_prepare",
           "gs_index_save_sdsl", "gs_debug_sdsl_sections", "gs_debug_sdsl_export_scratch",
           "gs_format_device", "gs_enumerate_text", "gs_index_last_text_offsets",
           "gs_format_device_ids", "gs_enumerate_text_device", "gs_kmers_encode_ids", "gs_kmers_get_ids", "gs_kmers_csv",
           "gs_kmers_concat", "gs_decoder_open", "gs_decoder_close", "gs_decode_records", "gs_decode_records_device",
           "gs_decode_sam", "gs_debug_repr_doubles", "gs_debug_decode_tables",
           "gs_index_last_spaced", "gs_debug_seed_recipes_a8", "gs_debug_spaced_rows", "gs_debug_resident",
           "gs_debug_buffers_live", "gs_debug_workspace", "gs_debug_index_layout", "gs_debug_index_array",
           "gs_debug_seed_probes", "gs_debug_seed_path", "gs_debug_rot_index",
           "gs_debug_bulge_last", "gs_debug_bulge_seeds", "gs_debug_bulge_verify",
           "gs_bgzf_compress_device", "gs_bgzf_compress", "gs_debug_huffman_lengths", "gs_debug_sp_float",
           "gs_bgzf_inflate", "gs_bgzf_inflate_device", "gs_bgzf_inflate_base", "gs_debug_inflate_member", "gs_debug_bgzf_members",
           "gs_decode_bam", "gs_decode_bam_device", "gs_debug_decode_bam_last",
           "gs_fasta_parse", "gs_fasta_parse_file", "gs_fasta_parse_device", "gs_fasta_info", "gs_fasta_records", "gs_fasta_text",
           "gs_fasta_free", "gs_decoder_open_fasta", "gs_debug_fasta_tile_bytes", "gs_debug_fasta_host",
           "gs_debug_fasta_chunk_bytes", "gs_debug_fasta_ms",
           "gs_kmers_parse", "gs_kmers_parse_file", "gs_kmers_parse_device", "gs_debug_kmers_tile_bytes",
           "gs_debug_kmers_chunk_bytes", "gs_debug_kmers_host",
           "gs_regions_parse", "gs_regions_parse_file", "gs_regions_info", "gs_regions_free", "gs_design_restrict",
           "gs_design_concat", "gs_design_score", "gs_design_select", "gs_design_rows", "gs_design_get", "gs_design_info",
           "gs_design_last_select", "gs_design_free", "gs_debug_design_host",
           "gs_regions_group_name", "gs_annot_build", "gs_annot_info", "gs_annot_free", "gs_debug_annot_entry_cap",
           "gs_annotate_device", "gs_annotate", "gs_debug_annotate_host", "gs_index_set_annotation",
           "gs_format_guides_features", "gs_format_guide_features", "gs_format_guide_ex_features",
           "gs_design_set_feature_rule", "gs_design_get_feature_hits",
           "gs_decoder_set_annotation", "gs_debug_decode_annot_ms",
           "gs_design_pairs", "gs_pairs_get", "gs_pairs_rows", "gs_pairs_last", "gs_pairs_ms", "gs_pairs_free", "gs_debug_pairs_host",
           "gs_debug_pairs_chunk",
           "gs_seq_rule_init", "gs_seq_rule_add_motif", "gs_kmers_filter", "gs_debug_kmers_filter_ms", "gs_debug_kmers_filter_host",
           "gs_design_set_spacing", "gs_design_last_spacing", "gs_debug_design_space_ms", "gs_debug_design_host_spaced",
           "gs_debug_design_set_scores",
           "gs_controls_generate", "gs_controls_rows", "gs_controls_counters", "gs_debug_controls_host",
           "gs_debug_controls_sequences", "gs_debug_controls_round"]


def _check(rc):
    if rc != 0:
        raise GsError(rc, lib().gs_status_string(rc).decode())


def buffers_live():
    """(allocations, bytes) of the workspace buffers alive in the process (gs_debug_buffers_live)"""
    L_ = lib()
    L_.gs_debug_buffers_live.restype = C.c_int
    L_.gs_debug_buffers_live.argtypes = [C.c_void_p]
    out = (C.c_uint64 * 2)()
    _check(L_.gs_debug_buffers_live(out))
    return int(out[0]), int(out[1])


WORKSPACE_GROUPS = ("batch", "big", "tile", "score", "text", "bgzf", "annot")


BULGE_SEED_DTYPE = np.dtype([("index", "<u4"), ("state", "<u4"), ("seq", "S32")])
BULGE_MATCH_DTYPE = np.dtype([("state", "<u4"), ("consumed", "<u4"), ("seq", "S32")])


def bulge_state(word):
    """the fields of a state word of the bulge-aware search (gs_bulge_step.h)"""
    word = int(word)
    return dict(t=word & 63, mismatches=(word >> 6) & 7, dna_bulges=(word >> 9) & 7, rna_bulges=(word >> 12) & 7,
                bulge_state=(word >> 15) & 3, bulge_size=(word >> 17) & 1, seq_len=(word >> 18) & 63)


def bulge_seeds(guide, k, mismatches=0, rna_bulges=0, dna_bulges=0, start=False, prefix_len=0, prefix=0, count_only=False):
    """the seeds of one guide in the seeded form of the bulge-aware search (gs_debug_bulge_seeds; host only): a
    BULGE_SEED_DTYPE array, one entry per path of index.hpp:250-375's tree that consumes k genome symbols"""
    g = guide.encode() if isinstance(guide, str) else bytes(guide)
    flags = GS_FLAG_PAM_AT_START if start else 0
    n = C.c_uint64(0)
    _check(lib().gs_debug_bulge_seeds(g, len(g), k, mismatches, rna_bulges, dna_bulges, flags, prefix_len, prefix, None, 0,
                                      C.byref(n)))
    if count_only:
        return int(n.value)
    out = np.zeros(n.value, dtype=BULGE_SEED_DTYPE)
    _check(lib().gs_debug_bulge_seeds(g, len(g), k, mismatches, rna_bulges, dna_bulges, flags, prefix_len, prefix,
                                      out.ctypes.data, out.size, C.byref(n)))
    assert n.value == out.size
    return out


def bulge_verify(state, seq, ctx_nibbles, guide, pam, k, alt_pams=(), mismatches=0, rna_bulges=0, dna_bulges=0, start=False):
    """the matches one seed (state word, sequence bytes so far) reaches in a row whose 16-symbol left context is
    ctx_nibbles (nearest first: 0..3 A,C,G,T, 4 N, 5 another symbol, 6 before the text start) - gs_debug_bulge_verify;
    host only -> a BULGE_MATCH_DTYPE array"""
    g = guide.encode() if isinstance(guide, str) else bytes(guide)
    p = pam.encode() if isinstance(pam, str) else bytes(pam)
    sq = np.frombuffer(bytes(seq).ljust(32, b"\0"), dtype=np.uint8).copy()
    alts = "".join(alt_pams).encode()
    lens = np.array([len(a) for a in alt_pams], dtype=np.uint32)
    flags = GS_FLAG_PAM_AT_START if start else 0

    def call(out, cap, n):
        _check(lib().gs_debug_bulge_verify(int(state), sq.ctypes.data, int(ctx_nibbles), g, len(g), p if p else None, len(p),
                                           alts if alt_pams else None, lens.ctypes.data if alt_pams else None,
                                           len(alt_pams), k, mismatches, rna_bulges, dna_bulges, flags, out, cap, C.byref(n)))
    n = C.c_uint64(0)
    call(None, 0, n)
    out = np.zeros(n.value, dtype=BULGE_MATCH_DTYPE)
    call(out.ctypes.data, out.size, n)
    assert n.value == out.size
    return out


def seed_recipes(k, L, P, m, n_x, astar=None, deep=False):
    """the seed plan of k_search for a batch shape (gs_debug_seed_recipes; host only):
    (one-sided, this strand's share, the other strand's share) as uint64 arrays"""
    L_ = lib()
    L_.gs_debug_seed_recipes.restype = C.c_int
    L_.gs_debug_seed_recipes.argtypes = [C.c_uint32] * 5 + [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
    a = None
    if astar is not None:
        a = (C.c_uint32 * 8)(*(list(astar) + [15] * 8)[:8])
    counts = (C.c_uint64 * 3)()
    _check(L_.gs_debug_seed_recipes(k, L, P, m, n_x, a, 1 if deep else 0, None, 0, counts))
    n = sum(counts)
    out = np.zeros(n, dtype=np.uint64)
    _check(L_.gs_debug_seed_recipes(k, L, P, m, n_x, a, 1 if deep else 0, out.ctypes.data, n, counts))
    c0, c1 = int(counts[0]), int(counts[1])
    return out[:c0], out[c0:c0 + c1], out[c0 + c1:]


def seed_recipes_a8(k, m, n_x, astar, trimmed=False):
    """this strand's share as read through PAM-pair tables (gs_debug_seed_recipes_a8; host only): the whole list, or the one
    without the spaced tables' class (no substitution in X, all m in O)"""
    L_ = lib()
    L_.gs_debug_seed_recipes_a8.restype = C.c_int
    L_.gs_debug_seed_recipes_a8.argtypes = [C.c_uint32] * 3 + [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
    a = (C.c_uint32 * 8)(*(list(astar) + [15] * 8)[:8])
    n = C.c_uint64()
    _check(L_.gs_debug_seed_recipes_a8(k, m, n_x, a, 1 if trimmed else 0, None, 0, C.byref(n)))
    out = np.zeros(int(n.value), dtype=np.uint64)
    _check(L_.gs_debug_seed_recipes_a8(k, m, n_x, a, 1 if trimmed else 0, out.ctypes.data, out.shape[0], C.byref(n)))
    return out


def seed_probes(k, L, P, m, n_x, astar, side, rot_first=31):
    """the probe list the seeding launches read beside a batch shape's recipes (gs_debug_seed_probes; host only), an (n, 2)
    uint32 array in the recipes' order.  side 0: the other strand's share (deep tables; the order of seed_recipes(...,
    deep=True)[2]); side 1 / 2: this strand's, whole / trimmed (the order of seed_recipes_a8), through a PAM-pair table whose
    rotated copies start at step rot_first (31: none)"""
    L_ = lib()
    L_.gs_debug_seed_probes.restype = C.c_int
    L_.gs_debug_seed_probes.argtypes = [C.c_uint32] * 5 + [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
    a = (C.c_uint32 * 8)(*(list(astar) + [15] * 8)[:8])
    n = C.c_uint64()
    _check(L_.gs_debug_seed_probes(k, L, P, m, n_x, a, side, rot_first, None, 0, C.byref(n)))
    out = np.zeros((int(n.value), 2), dtype=np.uint32)
    _check(L_.gs_debug_seed_probes(k, L, P, m, n_x, a, side, rot_first, out.ctypes.data, out.shape[0], C.byref(n)))
    return out


def seed_path(q: int, word: int, L: int, P: int, nst: int, side_b: bool = False, sid: int = 0, pams=(0, 0, 0, 0)):
    """what the seeding launches make of one recipe word for the packed guide q (gs_debug_seed_path; host only):
    (the seed's path word, the recipe's xor on a table index of nst symbols)"""
    L_ = lib()
    L_.gs_debug_seed_path.restype = C.c_int
    L_.gs_debug_seed_path.argtypes = [C.c_uint64, C.c_void_p, C.c_uint64] + [C.c_uint32] * 5 + [C.c_void_p]
    pam = (C.c_uint32 * 4)(*(list(pams) + [0] * 4)[:4])
    out = (C.c_uint64 * 2)()
    _check(L_.gs_debug_seed_path(q, pam, int(word), sid, 1 if side_b else 0, L, P, nst, out))
    return int(out[0]), int(out[1])


def rot_index(pidx: int, k: int, rs: int) -> int:
    """index pidx of a depth-k table as the copy rotated at consumption step rs holds it (gs_debug_rot_index; host only)"""
    L_ = lib()
    L_.gs_debug_rot_index.restype = C.c_int
    L_.gs_debug_rot_index.argtypes = [C.c_uint32] * 3 + [C.c_void_p]
    out = C.c_uint32()
    _check(L_.gs_debug_rot_index(pidx, k, rs, C.byref(out)))
    return int(out.value)


def guide_descriptor(q: int, pams, L: int, P: int, k: int, x_len: int, codes=(0, 0xFFFFFFFF), n_pt: int = 1, valid: bool = True):
    """the sixteen words an item of the seeding launches starts from (gs_debug_guide_descriptor; host only)"""
    L_ = lib()
    L_.gs_debug_guide_descriptor.restype = C.c_int
    L_.gs_debug_guide_descriptor.argtypes = [C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                             C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    pam = (C.c_uint32 * 4)(*(list(pams) + [0] * (4 - len(pams))))
    code = (C.c_uint32 * 2)(*codes)
    out = (C.c_uint32 * 16)()
    _check(L_.gs_debug_guide_descriptor(q, pam, len(pams), 1 if valid else 0, L, P, k, x_len, n_pt, code, out))
    names = ("q_lo", "q_hi", "pam0", "pam1", "pam2", "pam3", "meta", "pidx0", "pidxg", "qrem_b", "bsel_z", "bsel_w", "qhot",
             "key_a", "key_b", "guide")
    return dict(zip(names, (int(x) for x in out)))


def choose_thresholds(m, n_x, n_o, n_r, pam_expansions=4.0, verify_a=1.5, verify_b=1.9):
    """the cost model's thresholds a*(o) (gs_debug_choose_thresholds)"""
    L_ = lib()
    L_.gs_debug_choose_thresholds.restype = None
    L_.gs_debug_choose_thresholds.argtypes = [C.c_uint32] * 4 + [C.c_double] * 3 + [C.c_void_p]
    out = (C.c_uint32 * 8)()
    L_.gs_debug_choose_thresholds(m, n_x, n_o, n_r, pam_expansions, verify_a, verify_b, out)
    return list(out)


def tile_plan(records):
    """the tile ordering's plan for an item of `records` match records (gs_debug_tile_plan; host only):
    dict(buckets, slot, per, wave_tile, max_buckets)"""
    L_ = lib()
    L_.gs_debug_tile_plan.restype = None
    L_.gs_debug_tile_plan.argtypes = [C.c_uint32, C.c_void_p]
    out = (C.c_uint32 * 5)()
    L_.gs_debug_tile_plan(records, out)
    return dict(buckets=out[0], slot=out[1], per=out[2], wave_tile=out[3], max_buckets=out[4])


SEARCH_FORM_IN = ("items", "cus", "share_min", "backoff", "main", "walk", "one_chunk", "counting", "spec", "m", "est_heavy",
                  "est_max", "last_hpass", "last_items", "heavy", "split_share", "split_from", "seed_form")


def search_form(**kw):
    """the search's form for a pass (gs_debug_search_form; host only): dict(estimate, thresh, heavy, split, seed_form, form).
    Keyword arguments: SEARCH_FORM_IN; the switches default to -1 (not set), split_from to 2^19, the rest to 0."""
    L_ = lib()
    L_.gs_debug_search_form.restype = None
    L_.gs_debug_search_form.argtypes = [C.c_void_p, C.c_void_p]
    vals = dict(heavy=-1, split_share=-1, seed_form=-1, split_from=1 << 19)
    vals.update(kw)
    unknown = set(vals) - set(SEARCH_FORM_IN)
    if unknown:
        raise TypeError(f"unknown inputs {sorted(unknown)}")
    inp = (C.c_int64 * len(SEARCH_FORM_IN))(*[int(vals.get(k, 0)) for k in SEARCH_FORM_IN])
    out = (C.c_uint32 * 6)()
    L_.gs_debug_search_form(inp, out)
    return dict(zip(("estimate", "thresh", "heavy", "split", "seed_form", "form"), (int(x) for x in out)))


def make_genome_structure(names, lengths):
    arr_n = (C.c_char_p * len(names))(*[n.encode() for n in names])
    arr_l = (C.c_uint64 * len(lengths))(*lengths)
    g = GsGenomeStructure(arr_n, arr_l, len(names))
    g._keep = (arr_n, arr_l)
    return g


def format_header(gs, sam=False, complete=True, features=False) -> str:
    out, n = C.c_void_p(), C.c_size_t()
    flags = (GS_TEXT_SAM if sam else 0) | (GS_TEXT_COMPLETE if complete else 0) | (GS_TEXT_FEATURES if features else 0)
    _check(lib().gs_format_header(C.byref(gs), flags, C.byref(out), C.byref(n)))
    s = C.string_at(out, n.value).decode()
    lib().gs_free(out)
    return s


def format_guide(gs, gid, sequence, pam, sense_positive, hits, mismatches, sam=False, complete=True,
                 start=False, max_off_targets=-1, specificity=None, features=None) -> str:
    """hits: numpy HIT_DTYPE array of this guide (canonical order, as gs_enumerate returns);
    specificity: the guide's float from GenomeIndex.score (then the host does no CFD arithmetic);
    features: an Annotation - the match_features column (gs_format_guide_features; needs the specificity)"""
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    k = GsKmer(gid.encode(), sequence.encode(), pam.encode(), int(sense_positive))
    out, n = C.c_void_p(), C.c_size_t()
    flags = ((GS_TEXT_SAM if sam else 0) | (GS_TEXT_COMPLETE if complete else 0) |
             (GS_FLAG_PAM_AT_START if start else 0))
    if features is not None:
        _check(lib().gs_format_guide_features(C.byref(gs), C.byref(k), hits.ctypes.data, hits.shape[0], mismatches,
                                              flags | GS_TEXT_FEATURES, max_off_targets, float(specificity), features._h,
                                              C.byref(out), C.byref(n)))
    elif specificity is None:
        _check(lib().gs_format_guide(C.byref(gs), C.byref(k), hits.ctypes.data, hits.shape[0], mismatches,
                                     flags, max_off_targets, C.byref(out), C.byref(n)))
    else:
        _check(lib().gs_format_guide_scored(C.byref(gs), C.byref(k), hits.ctypes.data, hits.shape[0],
                                            mismatches, flags, max_off_targets, float(specificity),
                                            C.byref(out), C.byref(n)))
    s = C.string_at(out, n.value).decode()
    lib().gs_free(out)
    return s


def format_guides(gs, ids, seqs, pams, senses_positive, offsets, hits, specificity, mismatches, sam=False,
                  complete=True, start=False, max_off_targets=-1, skip=None, features=None) -> bytes:
    """the lines of a whole batch in one call (gs_format_guides_scored); features: an Annotation - with the
    match_features column (gs_format_guides_features)"""
    n = len(ids)
    arr = (GsKmer * n)(*[GsKmer(ids[i].encode(), seqs[i].encode(), pams[i].encode(), int(senses_positive[i]))
                         for i in range(n)])
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    spec = np.ascontiguousarray(specificity, dtype=np.float32)
    sk = None if skip is None else np.ascontiguousarray(skip, dtype=np.uint8)
    out, ln = C.c_void_p(), C.c_size_t()
    flags = ((GS_TEXT_SAM if sam else 0) | (GS_TEXT_COMPLETE if complete else 0) |
             (GS_FLAG_PAM_AT_START if start else 0))
    if features is not None:
        _check(lib().gs_format_guides_features(C.byref(gs), arr, n, offsets.ctypes.data,
                                               hits.ctypes.data if hits.shape[0] else None, spec.ctypes.data,
                                               sk.ctypes.data if sk is not None else None, mismatches,
                                               flags | GS_TEXT_FEATURES, max_off_targets, features._h, C.byref(out), C.byref(ln)))
    else:
        _check(lib().gs_format_guides_scored(C.byref(gs), arr, n, offsets.ctypes.data,
                                             hits.ctypes.data if hits.shape[0] else None, spec.ctypes.data,
                                             sk.ctypes.data if sk is not None else None, mismatches, flags,
                                             max_off_targets, C.byref(out), C.byref(ln)))
    s = C.string_at(out, ln.value)
    lib().gs_free(out)
    return s


def _id_blob(ids):
    """ids -> (bytes back to back, uint64 offsets[n+1]): the layout gs_format_device / gs_enumerate_text take"""
    enc = [i.encode() if isinstance(i, str) else bytes(i) for i in ids]
    off = np.zeros(len(enc) + 1, dtype=np.uint64)
    if enc:
        off[1:] = np.cumsum([len(e) for e in enc], dtype=np.uint64)
    return b"".join(enc), off


def _bytes_or_none(x, n):
    if x is None:
        return None
    a = np.ascontiguousarray(np.asarray(x) != 0, dtype=np.uint8)
    if a.shape != (n,):
        raise ValueError("one entry per guide")
    return a


class SeqRule:
    """The sequence rules on the candidates of a scan (csrc/gs_select_scan.h): gc=(MIN, MAX) integer percentages,
    max_run >= 1, exclude_motifs and exclude_sites IUPAC motifs over ACGTRYSWKMBDHVN - a site also excludes its reverse
    complement.  At most 16 motifs after that expansion, 1 to 32 letters each; ValueError names the motif refused."""

    def __init__(self, gc=None, max_run=None, exclude_motifs=(), exclude_sites=()):
        self.c = GsSeqRule()
        _check(lib().gs_seq_rule_init(C.byref(self.c)))
        if gc is not None:
            lo, hi = gc
            if int(lo) != lo or int(hi) != hi or not 0 <= lo <= hi <= 100:
                raise ValueError("gc: (MIN, MAX), integer percentages with 0 <= MIN <= MAX <= 100")
            self.c.gc_min, self.c.gc_max = int(lo), int(hi)
        if max_run is not None:
            if int(max_run) != max_run or max_run < 1:
                raise ValueError("max_run >= 1")
            self.c.max_run = int(max_run)
        for motifs, both in ((exclude_motifs, 0), (exclude_sites, 1)):
            for m in motifs:
                rc = lib().gs_seq_rule_add_motif(C.byref(self.c), m.encode(), both)
                if rc != 0:
                    raise ValueError(lib().gs_status_string(rc).decode())

    @property
    def n_motifs(self):
        return int(self.c.n_motifs)


def seq_rule_host(seqs, k, rule):
    """the rule on the host through the kernels' shared header, no GPU (gs_debug_kmers_filter_host).  seqs: uint8[n, k] ->
    (charge uint8[n]: 0 passes, 1 GC, 2 run, 3 motif; counts: dict(scanned, gc, run, motif))"""
    a = np.ascontiguousarray(seqs, dtype=np.uint8).reshape(-1, k)
    n = a.shape[0]
    charge = np.zeros(n, dtype=np.uint8)
    counts = (C.c_uint64 * 4)()
    _check(lib().gs_debug_kmers_filter_host(a.ctypes.data if n else None, n, k, C.byref(rule.c), charge.ctypes.data if n else None, counts))
    return charge, dict(zip(("scanned", "gc", "run", "motif"), (int(x) for x in counts)))


class DeviceKmers:
    """Candidate guides of one chromosome, resident in HBM (gs_kmers_generate).  `seqs_ptr` /
    `pams_ptr` are raw device addresses in the layout GenomeIndex.enumerate_device takes."""

    def __init__(self, handle, k, P):
        self._h, self.k, self.P = handle, k, P
        n, a, b, c, d = C.c_uint64(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().gs_kmers_get(handle, 1, C.byref(n), C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        self.n = int(n.value)
        self.seqs_ptr, self.pams_ptr, self.pos_ptr, self.sense_ptr = a.value, b.value, c.value, d.value

    @classmethod
    def parse(cls, src, device=0):
        """The rows of a kmers file parsed on the GPU (gs_kmers_parse / gs_kmers_parse_file) under the rules of the
        command's host reader.  src: a path (read in chunks through page-locked staging), or the file's bytes.  The
        object carries the file's ids (ids_ptr, id_offsets_ptr, sense_positive_ptr) and no positions; .report holds
        n, L, P, n_lines and ms.  Raises KmersFileError (status 6) where the host reader fails, GsError with status 3
        for rows of several shapes."""
        h, rep = C.c_void_p(), GsKmersReport()
        if isinstance(src, (str, os.PathLike)):
            rc = lib().gs_kmers_parse_file(device, os.fsencode(src), C.byref(h), C.byref(rep))
        else:
            raw = np.frombuffer(src, dtype=np.uint8) if isinstance(src, (bytes, bytearray, memoryview)) else np.ascontiguousarray(src, dtype=np.uint8)
            rc = lib().gs_kmers_parse(device, raw.ctypes.data if raw.size else None, raw.size, C.byref(h), C.byref(rep))
        return cls._parsed(rc, h, rep)

    @classmethod
    def parse_device(cls, d_raw_ptr, length, device=0, stream=None):
        """the raw bytes are in HBM already (d_raw_ptr: a device address, at any alignment)"""
        h, rep = C.c_void_p(), GsKmersReport()
        rc = lib().gs_kmers_parse_device(device, d_raw_ptr if length else None, length, stream, C.byref(h), C.byref(rep))
        return cls._parsed(rc, h, rep)

    @classmethod
    def _parsed(cls, rc, h, rep, on_device=True):
        report = _kmers_report(rc, rep)
        km = cls.__new__(cls)
        km._h, km.k, km.P, km.n, km.report = h, report["L"], report["P"], report["n"], report
        km.pos_ptr = None
        if on_device:
            a, b, d = C.c_void_p(), C.c_void_p(), C.c_void_p()
            _check(lib().gs_kmers_get(h, 1, None, C.byref(a), C.byref(b), None, C.byref(d)))
            km.seqs_ptr, km.pams_ptr, km.sense_ptr = a.value, b.value, d.value
            _check(lib().gs_kmers_get_ids(h, 1, C.byref(a), C.byref(b), C.byref(d)))
            km.ids_ptr, km.id_offsets_ptr, km.sense_positive_ptr = a.value, b.value, d.value
        return km

    def to_host(self):
        """-> (seqs uint8[n,k], pams uint8[n,P], positions uint32[n] 1-based, senses uint8[n]); the positions are None
        on the rows of a kmers file"""
        n, a, b, c, d = C.c_uint64(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().gs_kmers_get(self._h, 0, C.byref(n), C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        m = int(n.value)
        if m == 0:
            return (np.empty((0, self.k), np.uint8), np.empty((0, self.P), np.uint8),
                    None if getattr(self, "report", None) else np.empty(0, np.uint32), np.empty(0, np.uint8))
        seqs = np.frombuffer(C.string_at(a, m * self.k), dtype=np.uint8).reshape(m, self.k).copy()
        pams = np.frombuffer(C.string_at(b, m * self.P), dtype=np.uint8).reshape(m, self.P).copy()
        pos = np.frombuffer(C.string_at(c, 4 * m), dtype=np.uint32).copy() if c.value else None
        sense = np.frombuffer(C.string_at(d, m), dtype=np.uint8).copy()
        return seqs, pams, pos, sense

    def encode_ids(self, prefix, chr_name):
        """the ids "{prefix}{chr_name}:{position}:{sense}" encoded in HBM (gs_kmers_encode_ids); sets ids_ptr,
        id_offsets_ptr (n + 1 uint64) and sense_positive_ptr (n bytes, 1 = "+"): raw device addresses"""
        _check(lib().gs_kmers_encode_ids(self._h, prefix.encode(), chr_name.encode(), None))
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().gs_kmers_get_ids(self._h, 1, C.byref(a), C.byref(b), C.byref(c)))
        self.ids_ptr, self.id_offsets_ptr, self.sense_positive_ptr = a.value, b.value, c.value

    def ids_to_host(self):
        """-> (ids bytes back to back, offsets uint64[n+1], sense_positive uint8[n]) of the last encode_ids"""
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().gs_kmers_get_ids(self._h, 0, C.byref(a), C.byref(b), C.byref(c)))
        off = np.frombuffer(C.string_at(b, 8 * (self.n + 1)), dtype=np.uint64).copy()
        ids = C.string_at(a, int(off[-1])) if off[-1] else b""
        sp = np.frombuffer(C.string_at(c, self.n), dtype=np.uint8).copy() if self.n else np.empty(0, np.uint8)
        return ids, off, sp

    def csv(self, prefix, chr_name) -> bytes:
        """the records as rows of the kmers file, no header (gs_kmers_csv)"""
        out, ln = C.c_void_p(), C.c_uint64()
        _check(lib().gs_kmers_csv(self._h, prefix.encode(), chr_name.encode(), C.byref(out), C.byref(ln)))
        s = C.string_at(out, ln.value)
        lib().gs_free(out)
        return s

    def filter(self, rule):
        """the candidates that pass a SeqRule, in the scan's order, as a fresh DeviceKmers (gs_kmers_filter); before
        encode_ids.  .filter_counts: dict(scanned, gc, run, motif); .filter_ms: the three passes between stream events"""
        h, counts, ms = C.c_void_p(), (C.c_uint64 * 4)(), (C.c_double * 3)()
        _check(lib().gs_kmers_filter(self._h, C.byref(rule.c), None, C.byref(h), counts))
        km = DeviceKmers(h, self.k, self.P)
        km.filter_counts = dict(zip(("scanned", "gc", "run", "motif"), (int(x) for x in counts)))
        _check(lib().gs_debug_kmers_filter_ms(h, ms))
        km.filter_ms = dict(zip(("rule", "scan", "gather"), (float(x) for x in ms)))
        return km

    def controls_rows(self) -> bytes:
        """the kmers-file rows "id,sequence,pam,NA,0,+" of the controls api.controls made, no header (gs_controls_rows)"""
        out, ln = C.c_void_p(), C.c_uint64()
        _check(lib().gs_controls_rows(self._h, C.byref(out), C.byref(ln)))
        s = C.string_at(out, ln.value)
        lib().gs_free(out)
        return s

    def control_counters(self):
        """the counters of the controls api.controls made, in order (gs_controls_counters) -> uint64[n]"""
        n, p = C.c_uint64(), C.c_void_p()
        _check(lib().gs_controls_counters(self._h, C.byref(n), C.byref(p)))
        return np.frombuffer(C.string_at(p, 8 * n.value), dtype=np.uint64).copy() if n.value else np.empty(0, np.uint64)

    def restrict(self, regions, chr_index):
        """the records of this scan - of chromosome chr_index of the regions' structure - that lie in a group of
        `regions` (gs_design_restrict) -> Design"""
        h = C.c_void_p()
        _check(lib().gs_design_restrict(regions._h, chr_index, self._h, None, C.byref(h)))
        return Design(h, regions, self.k, self.P)

    def close(self):
        if self._h:
            lib().gs_kmers_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _selected_kmers(h, k, P):
    """a DeviceKmers over the object gs_design_select / gs_debug_design_host made: ids from the start"""
    km = DeviceKmers.__new__(DeviceKmers)
    km._h, km.k, km.P = h, k, P
    n = C.c_uint64()
    _check(lib().gs_kmers_get(h, 0, C.byref(n), None, None, None, None))
    km.n = int(n.value)
    return km


CONTROLS_COUNTS = ("kept", "looked_at", "gc", "run", "motif", "targeting", "close", "last_counter", "rounds")
CONTROLS_STAGES = ("generate", "search", "keep", "distance", "ids")


def _controls_rule(n, L, pam, seed, first, mismatches, alt_pams, start, seq_rule, min_distance, max_candidates, round, prefix,
                   no_new_tables=False):
    """-> (GsControlsRule, what it points to: keep alive for the call)"""
    alts = "".join(alt_pams).encode()
    if any(len(p) != len(pam) for p in alt_pams):
        raise ValueError("an alt PAM has the PAM's length")
    keep = (pam.encode(), alts, prefix.encode(), seq_rule)
    r = GsControlsRule(seed=seed, first=first, n=n, max_candidates=max_candidates, round=round, L=L, n_alt=len(alt_pams),
                       mismatches=mismatches, flags=(1 if start else 0) | (16 if no_new_tables else 0), min_distance=min_distance,
                       pam=keep[0], alt_pams=keep[1] if alt_pams else None,
                       seq_rule=C.pointer(seq_rule.c) if seq_rule is not None else None, id_prefix=keep[2])
    return r, keep


def _controls_report(rep):
    out = {k: int(getattr(rep, k)) for k in CONTROLS_COUNTS}
    out["ms"] = dict(zip(CONTROLS_STAGES, (float(x) for x in rep.ms)))
    return out


def controls(index, n, L=20, pam="NGG", seed=0, first=0, mismatches=3, alt_pams=(), start=False, seq_rule=None, min_distance=1,
             max_candidates=1 << 32, round=0, prefix="control_", no_new_tables=False):
    """Non-targeting controls (gs_controls_generate; the rules are csrc/gs_controls_scan.h's): the first n candidates of
    the seed's counter sequence from `first` that pass seq_rule (a SeqRule), have no site within `mismatches` under pam and
    alt_pams, and lie min_distance mismatches or more from every control kept before them; at most max_candidates are
    looked at.  -> (DeviceKmers with ids "{prefix}{counter}" from the start, as a parsed object: .controls_rows() its
    kmers-file rows, .control_counters() the kept counters; report: dict of kept, looked_at, gc, run, motif, targeting,
    close, last_counter, rounds and ms by stage).  Fewer than n kept is no error: report["kept"] says so.  round: counters
    per device round (0: the default); the result does not depend on it."""
    r, keep = _controls_rule(n, L, pam, seed, first, mismatches, alt_pams, start, seq_rule, min_distance, max_candidates, round, prefix,
                             no_new_tables)
    h, rep = C.c_void_p(), GsControlsReport()
    _check(lib().gs_controls_generate(index._h, C.byref(r), None, C.byref(h), C.byref(rep)))
    km = DeviceKmers.__new__(DeviceKmers)
    km._h, km.k, km.P, km.pos_ptr = h, L, len(pam), None
    a, b, d, m = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
    _check(lib().gs_kmers_get(h, 1, C.byref(m), C.byref(a), C.byref(b), None, C.byref(d)))
    km.n, km.seqs_ptr, km.pams_ptr, km.sense_ptr = int(m.value), a.value, b.value, d.value
    _check(lib().gs_kmers_get_ids(h, 1, C.byref(a), C.byref(b), C.byref(d)))
    km.ids_ptr, km.id_offsets_ptr, km.sense_positive_ptr = a.value, b.value, d.value
    km.report = _controls_report(rep)                      # as a parsed object: no positions
    return km, km.report


def controls_round(set_to=0) -> int:
    """the counters of a device round where the call says 0 (gs_debug_controls_round); set_to != 0 sets it"""
    return int(lib().gs_debug_controls_round(set_to))


def controls_host_model(targeting, n, L=20, pam="NGG", seed=0, first=0, seq_rule=None, min_distance=1, max_candidates=1 << 32,
                        prefix="control_", round=0):
    """the walk on the host through the kernels' shared header, no GPU and no search (gs_debug_controls_host).  targeting:
    one byte per candidate from `first`, nonzero where it has a hit; round != 0: the walk cut into rounds as the device cuts it
    -> (kept counters uint64[kept], rows bytes, report)"""
    t = np.ascontiguousarray(np.asarray(targeting) != 0, dtype=np.uint8)
    r, keep = _controls_rule(n, L, pam, seed, first, 0, (), False, seq_rule, min_distance, max_candidates, round, prefix)
    kc, rows, ln, rep = C.c_void_p(), C.c_void_p(), C.c_uint64(), GsControlsReport()
    _check(lib().gs_debug_controls_host(C.byref(r), t.ctypes.data if t.size else None, t.size, C.byref(kc), C.byref(rows), C.byref(ln),
                                        C.byref(rep)))
    report = _controls_report(rep)
    counters = np.frombuffer(C.string_at(kc, 8 * report["kept"]), dtype=np.uint64).copy()
    text = C.string_at(rows, ln.value)
    lib().gs_free(kc)
    lib().gs_free(rows)
    return counters, text, report


def control_sequences(seed, first, n, L):
    """the generator alone (gs_debug_controls_sequences) -> uint8[n, L], candidates first .. first + n - 1"""
    out = np.empty((n, L), dtype=np.uint8)
    _check(lib().gs_debug_controls_sequences(seed, first, n, L, out.ctypes.data if n else None))
    return out


class RegionsFileError(GsError):
    """a regions file that the parser refuses: .message is "regions line N: REASON"; kind and line as in
    gs_regions_report"""

    def __init__(self, status, msg, kind, line):
        super().__init__(status, msg)
        self.message, self.kind, self.line = msg, kind, line


class Regions:
    """The intervals of a BED file, grouped and merged against a genome structure (gs_regions_parse; host side)."""

    def __init__(self, handle, structure, report):
        self._h, self.structure, self.report = handle, structure, report
        self.n_groups, self.n_intervals = report["n_groups"], report["n_intervals"]

    @classmethod
    def parse(cls, src, structure, prefix=""):
        """src: a path, or the file's bytes.  structure: a GsGenomeStructure (make_genome_structure), or (names,
        lengths).  prefix: the id prefix the cap on group names is checked with.  Raises RegionsFileError (status 6)
        with the 1-based line and the reason."""
        gs = structure if isinstance(structure, GsGenomeStructure) else make_genome_structure(*structure)
        h, rep = C.c_void_p(), GsRegionsReport()
        if isinstance(src, (str, os.PathLike)):
            rc = lib().gs_regions_parse_file(os.fsencode(src), C.byref(gs), prefix.encode(), C.byref(h), C.byref(rep))
        else:
            raw = bytes(src)
            rc = lib().gs_regions_parse(raw if raw else None, len(raw), C.byref(gs), prefix.encode(), C.byref(h), C.byref(rep))
        text = C.string_at(rep.bad_text, rep.bad_len).decode("latin-1") if rep.bad_text else ""
        if rep.bad_text:
            lib().gs_free(rep.bad_text)
        if rc != 0 and rep.bad_kind:
            raise RegionsFileError(rc, text, int(rep.bad_kind), int(rep.bad_line))
        _check(rc)
        return cls(h, gs, {k: int(getattr(rep, k)) for k in ("n_lines", "n_intervals", "n_groups")})

    def close(self):
        if self._h:
            lib().gs_regions_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Annotation:
    """The lookup table of a BED file's features (gs_annot_build): which groups a printed off-target row touches.
    device None: host only (the host encoders and annotate_host_model)."""

    def __init__(self, handle, regions, device):
        self._h, self.structure, self.device = handle, regions.structure, device
        name = C.c_char_p()
        self.names = []
        for g in range(regions.n_groups):
            _check(lib().gs_regions_group_name(regions._h, g, C.byref(name)))
            self.names.append(name.value.decode("latin-1"))

    @classmethod
    def build(cls, regions, device=0):
        h = C.c_void_p()
        _check(lib().gs_annot_build(regions._h, -1 if device is None else device, C.byref(h)))
        return cls(h, regions, device)

    def info(self):
        """-> dict(groups, segments, entries) (gs_annot_info)"""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib().gs_annot_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"groups": int(a.value), "segments": int(b.value), "entries": int(c.value)}

    def close(self):
        if self._h:
            lib().gs_annot_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def annot_entry_cap(set_to=0) -> int:
    """the entry cap of Annotation.build; set_to != 0 sets it (gs_debug_annot_entry_cap)"""
    return int(lib().gs_debug_annot_entry_cap(set_to))


def _annotate_call(fn, head, annotation, gs, offsets, hits, L, P, mismatches):
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    n = offsets.shape[0] - 1
    nh = int(offsets[n] - offsets[0]) if n > 0 else 0
    foff = np.zeros(nh + 1, dtype=np.uint64)
    gcnt = np.zeros((max(n, 0), mismatches + 1), dtype=np.uint32)
    feats, nf = C.c_void_p(), C.c_uint64()
    _check(fn(*head, annotation._h, C.byref(gs), max(n, 0), L, P, mismatches, offsets.ctypes.data,
              hits.ctypes.data if hits.shape[0] else None, foff.ctypes.data, C.byref(feats), C.byref(nf),
              gcnt.ctypes.data if gcnt.size else None))
    try:
        f = np.frombuffer(C.string_at(feats, 4 * nf.value), dtype=np.uint32).copy() if nf.value else np.empty(0, np.uint32)
    finally:
        lib().gs_free(feats)
    return foff, f, gcnt


def annotate_host_model(annotation, gs, offsets, hits, L, P, mismatches):
    """GenomeIndex.annotate on the host through the kernels' shared header, no GPU (gs_debug_annotate_host)"""
    return _annotate_call(lib().gs_debug_annotate_host, (), annotation, gs, offsets, hits, L, P, mismatches)


def _select_args(per_region, min_specificity):
    n = 0 if per_region is None else int(per_region)
    if per_region is not None and n < 1:
        raise ValueError("per_region >= 1")
    s = -1.0 if min_specificity is None else float(min_specificity)
    if min_specificity is not None and not 0.0 <= s <= 1.0:
        raise ValueError("0 <= min_specificity <= 1")
    return n, s


class Design:
    """The (candidate, group) records of a set of regions in HBM (gs_design_restrict / gs_design_concat); keeps its
    Regions alive."""

    def __init__(self, handle, regions, k, P):
        self._h, self.regions, self.k, self.P = handle, regions, k, P

    @classmethod
    def concat(cls, parts):
        arr = (C.c_void_p * len(parts))(*[p._h for p in parts])
        h = C.c_void_p()
        _check(lib().gs_design_concat(arr, len(parts), C.byref(h)))
        return cls(h, parts[0].regions, parts[0].k, parts[0].P)

    def score(self, index, mismatches=3, alt_pams=(), start=False, threshold=-1, batch=0, no_new_tables=False):
        """the specificity of every record through the index's search and scoring (gs_design_score); threshold >= 0
        also runs the counting pass of --threshold and marks what it would drop as not eligible"""
        alt = b"".join(p.encode() for p in alt_pams)
        flags = (GS_FLAG_PAM_AT_START if start else 0) | (GS_FLAG_NO_NEW_TABLES if no_new_tables else 0)
        _check(lib().gs_design_score(index._h, self._h, alt if alt_pams else None, len(alt_pams), mismatches, flags,
                                     threshold, batch, None))
        return self

    def set_feature_rule(self, annotation, distance, max_hits):
        """before score(): count, per record, the off-target hits within `distance` that touch a feature of `annotation`
        (the record's own site left out); more than max_hits and the record is not eligible
        (gs_design_set_feature_rule).  annotation None takes the rule off."""
        _check(lib().gs_design_set_feature_rule(self._h, annotation._h if annotation is not None else None, distance, max_hits))
        self._rule = annotation   # keeps it alive through score()
        return self

    def set_spacing(self, min_spacing, cut_offset=3, start=False):
        """the picks of a group lie min_spacing bases apart or more, by the cut that leaves cut_offset protospacer bases
        between it and the PAM (gs_design_set_spacing; the rule is csrc/gs_select_scan.h's).  0 takes the rule off.
        select() and rows() then need 1 <= per_region <= 1024, and pairs() is refused."""
        _check(lib().gs_design_set_spacing(self._h, int(min_spacing), int(cut_offset), GS_FLAG_PAM_AT_START if start else 0))
        return self

    def last_spacing(self):
        """of the last select() / rows() under set_spacing (gs_design_last_spacing)"""
        out = (C.c_uint64 * 2)()
        _check(lib().gs_design_last_spacing(self._h, out))
        return {"passed_over": int(out[0]), "groups_short_for_spacing": int(out[1])}

    def space_ms(self):
        """the milliseconds of that selection's walk kernel alone (gs_debug_design_space_ms)"""
        ms = C.c_double()
        _check(lib().gs_debug_design_space_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def set_scores(self, spec, eligible=None):
        """specificities (float32[n]) and eligibility bytes (uint8[n], None: all) from the host, in record order; the
        design then counts as scored (gs_debug_design_set_scores).  For tests of the selection."""
        n = self.info()[0]
        s = np.ascontiguousarray(spec, dtype=np.float32)
        e = None if eligible is None else np.ascontiguousarray(eligible, dtype=np.uint8)
        if s.shape != (n,) or (e is not None and e.shape != (n,)):
            raise ValueError("one entry per record")
        _check(lib().gs_debug_design_set_scores(self._h, s.ctypes.data if n else None, e.ctypes.data if e is not None and n else None))
        return self

    def select(self, prefix="", per_region=None, min_specificity=None):
        """the records in order, cut to the first per_region eligible ones of each group with specificity >=
        min_specificity (gs_design_select) -> DeviceKmers with ids"""
        n, s = _select_args(per_region, min_specificity)
        h = C.c_void_p()
        _check(lib().gs_design_select(self._h, prefix.encode(), n, s, None, C.byref(h)))
        km = _selected_kmers(h, self.k, self.P)
        a, b, c, d = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().gs_kmers_get(h, 1, None, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        km.seqs_ptr, km.pams_ptr, km.pos_ptr, km.sense_ptr = a.value, b.value, c.value, d.value
        _check(lib().gs_kmers_get_ids(h, 1, C.byref(a), C.byref(b), C.byref(c)))
        km.ids_ptr, km.id_offsets_ptr, km.sense_positive_ptr = a.value, b.value, c.value
        return km

    def rows(self, prefix="", per_region=None, min_specificity=None) -> bytes:
        """the same selection as rows of the kmers file, no header (gs_design_rows)"""
        n, s = _select_args(per_region, min_specificity)
        out, ln = C.c_void_p(), C.c_uint64()
        _check(lib().gs_design_rows(self._h, prefix.encode(), n, s, None, C.byref(out), C.byref(ln)))
        t = C.string_at(out, ln.value)
        lib().gs_free(out)
        return t

    def pairs(self, prefix, max_span, min_span=1, cut_offset=3, orientation="any", per_region=None, min_specificity=None,
              start=False):
        """the guide pairs of every group under the rule of csrc/gs_pairs_scan.h (gs_design_pairs): cuts min_span to
        max_span apart on one chromosome, orientation "any", "pam-out" or "pam-in", ranked by the smaller specificity, the
        first per_region of each group -> (DeviceKmers with ids: the guides of the kept pairs, Pairs)"""
        rule = _pair_rule(max_span, min_span, cut_offset, orientation, per_region, min_specificity, start)
        h, ph = C.c_void_p(), C.c_void_p()
        _check(lib().gs_design_pairs(self._h, prefix.encode(), C.byref(rule), None, C.byref(h), C.byref(ph)))
        km = _selected_kmers(h, self.k, self.P)
        a, b, c, d = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().gs_kmers_get(h, 1, None, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        km.seqs_ptr, km.pams_ptr, km.pos_ptr, km.sense_ptr = a.value, b.value, c.value, d.value
        _check(lib().gs_kmers_get_ids(h, 1, C.byref(a), C.byref(b), C.byref(c)))
        km.ids_ptr, km.id_offsets_ptr, km.sense_positive_ptr = a.value, b.value, c.value
        return km, Pairs(ph)

    def to_host(self):
        """-> dict(n, group uint32[n], chr uint32[n], pos uint32[n], sense uint8[n], spec float32[n], eligible uint8[n]);
        after a score() under set_feature_rule also feature_hits uint32[n]"""
        n = C.c_uint64()
        p = [C.c_void_p() for _ in range(6)]
        _check(lib().gs_design_get(self._h, C.byref(n), *[C.byref(x) for x in p]))
        m = int(n.value)
        out = {"n": m}
        for name, x, dt in zip(("group", "chr", "pos", "sense", "spec", "eligible"), p,
                               (np.uint32, np.uint32, np.uint32, np.uint8, np.float32, np.uint8)):
            out[name] = np.frombuffer(C.string_at(x, m * np.dtype(dt).itemsize), dtype=dt).copy() if m else np.empty(0, dt)
        fh = C.c_void_p()
        if getattr(self, "_rule", None) is not None and lib().gs_design_get_feature_hits(self._h, C.byref(fh)) == 0:
            out["feature_hits"] = np.frombuffer(C.string_at(fh, 4 * m), dtype=np.uint32).copy() if m else np.empty(0, np.uint32)
        return out

    def info(self):
        """-> (records, scored) without copying anything (gs_design_info)"""
        n, sc = C.c_uint64(), C.c_int()
        _check(lib().gs_design_info(self._h, C.byref(n), C.byref(sc)))
        return int(n.value), bool(sc.value)

    def last_select(self):
        out = (C.c_uint64 * 4)()
        _check(lib().gs_design_last_select(self._h, out))
        return dict(zip(("records", "kept", "groups_empty", "groups_short"), (int(x) for x in out)))

    def close(self):
        if self._h:
            lib().gs_design_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


ORIENTATIONS = {"any": 0, "pam-out": 1, "pam-in": 2}


def _pair_rule(max_span, min_span, cut_offset, orientation, per_region, min_specificity, start):
    if orientation not in ORIENTATIONS:
        raise ValueError('orientation: "any", "pam-out" or "pam-in"')
    n, s = _select_args(per_region, min_specificity)
    return GsPairRule(int(min_span), int(max_span), int(cut_offset), ORIENTATIONS[orientation], n,
                      GS_FLAG_PAM_AT_START if start else 0, s, 0)


class Pairs:
    """The kept pairs of Design.pairs / pairs_host (gs_pairs), on the host."""
    COLUMNS = (("group", np.uint32), ("chr", np.uint32), ("a", np.uint32), ("b", np.uint32), ("cut_a", np.uint32),
               ("cut_b", np.uint32), ("spec_a", np.float32), ("spec_b", np.float32))

    def __init__(self, handle):
        self._h = handle

    def to_host(self):
        """-> dict(n, group, chr, a, b, cut_a, cut_b uint32[n], spec_a, spec_b float32[n]); a and b are places in the
        guides object (record indices from pairs_host)"""
        n = C.c_uint64()
        p = [C.c_void_p() for _ in range(8)]
        _check(lib().gs_pairs_get(self._h, C.byref(n), *[C.byref(x) for x in p]))
        m = int(n.value)
        out = {"n": m}
        for (name, dt), x in zip(self.COLUMNS, p):
            out[name] = np.frombuffer(C.string_at(x, 4 * m), dtype=dt).copy() if m else np.empty(0, dt)
        return out

    def rows(self, guides) -> bytes:
        """the table, header included, with the ids of `guides`, the object that came with these pairs (gs_pairs_rows)"""
        out, ln = C.c_void_p(), C.c_uint64()
        _check(lib().gs_pairs_rows(self._h, guides._h, C.byref(out), C.byref(ln)))
        t = C.string_at(out, ln.value)
        lib().gs_free(out)
        return t

    def last(self):
        out = (C.c_uint64 * 6)()
        _check(lib().gs_pairs_last(self._h, out))
        return dict(zip(("eligible", "counted", "kept", "chunks", "groups_without", "groups_short"), (int(x) for x in out)))

    def ms(self):
        """the milliseconds of Design.pairs' stages between stream events (gs_pairs_ms)"""
        out = (C.c_double * 8)()
        _check(lib().gs_pairs_ms(self._h, out))
        return dict(zip(("compact", "order", "count", "offsets", "emit", "rank", "keep", "guides"), (float(x) for x in out)))

    def close(self):
        if self._h:
            lib().gs_pairs_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pairs_chunk(set_to=0) -> int:
    """the most pairs a chunk of Design.pairs holds; set_to != 0 sets it (gs_debug_pairs_chunk)"""
    return int(lib().gs_debug_pairs_chunk(set_to))


def pairs_host(group, chr, pos, sense, spec, eligible, k, P, n_groups, max_span, min_span=1, cut_offset=3, orientation="any",
               per_region=None, min_specificity=None, start=False):
    """the passes of Design.pairs on the host through the kernels' shared header, no GPU (gs_debug_pairs_host), over
    plain arrays of records -> (Pairs.to_host() with a and b as record indices, Pairs.last())"""
    rule = _pair_rule(max_span, min_span, cut_offset, orientation, per_region, min_specificity, start)
    cols = [np.ascontiguousarray(x, dtype=dt) for x, dt in
            ((group, np.uint32), (chr, np.uint32), (pos, np.uint32), (sense, np.uint8), (spec, np.float32), (eligible, np.uint8))]
    n = cols[0].shape[0]
    h = C.c_void_p()
    _check(lib().gs_debug_pairs_host(n, *[c.ctypes.data if n else None for c in cols], k, P, n_groups, C.byref(rule), C.byref(h)))
    pr = Pairs(h)
    try:
        return pr.to_host(), pr.last()
    finally:
        pr.close()


def design(index, regions, pam, k, per_region=None, min_specificity=None, *, chromosomes, mismatches=3, alt_pams=(),
           start=False, threshold=-1, prefix="", device=0, seq_rule=None, min_spacing=0, cut_offset=3):
    """Guides for regions in one call: scan, (filter,) restrict, (score,) select -> DeviceKmers with ids.  chromosomes:
    iterable of (index in the regions' structure, the chromosome's bytes).  `index` (a GenomeIndex) may be None when neither
    per_region, min_specificity nor threshold asks for scores.  seq_rule: a SeqRule, applied to every scan before it is
    restricted, so a candidate it drops is never scored.  min_spacing > 0 (with per_region <= 1024): the picks of a group
    lie that many bases apart or more, by the cut at cut_offset (Design.set_spacing)."""
    parts = []
    try:
        for ci, chrm in chromosomes:
            km = generate_kmers(chrm, pam, k, start, device)
            try:
                if seq_rule is not None:
                    kept = km.filter(seq_rule)
                    km.close()
                    km = kept
                parts.append(km.restrict(regions, ci))
            finally:
                km.close()
        whole = Design.concat(parts)
    finally:
        for p in parts:
            p.close()
    try:
        if per_region is not None or min_specificity is not None or threshold >= 0:
            whole.score(index, mismatches, alt_pams, start, threshold)
        if min_spacing:
            whole.set_spacing(min_spacing, cut_offset, start)
        return whole.select(prefix, per_region, min_specificity)
    finally:
        whole.close()


def design_host_model(regions, parts, pam, k, prefix="", per_region=None, min_specificity=None, rows=False, min_spacing=None,
                      cut_offset=3, start=False):
    """the stages of Design on the host through the kernels' shared header, no GPU (gs_debug_design_host).  parts: list of
    (chr_index, seqs uint8[n,k], positions uint32[n], senses uint8[n], specificity float32[n] or None, eligible
    uint8[n] or None) -> dict as kmers_arrays plus pos, and rows bytes when asked for.  min_spacing not None: through
    gs_debug_design_host_spaced, and the dict also holds last_select and last_spacing as Design gives them"""
    npart = len(parts)
    keep = []

    def col(i, dt):
        ptrs = (C.c_void_p * max(1, npart))()
        given = False
        for j, p in enumerate(parts):
            if p[i] is not None:
                a = np.ascontiguousarray(p[i], dtype=dt)
                keep.append(a)
                ptrs[j] = a.ctypes.data if a.size else None
                given = True
        return ptrs, given

    chr_index = np.array([p[0] for p in parts], dtype=np.uint32)
    counts = np.array([len(p[2]) for p in parts], dtype=np.uint64)
    seqs, _ = col(1, np.uint8)
    pos, _ = col(2, np.uint32)
    sense, _ = col(3, np.uint8)
    spec, have_spec = col(4, np.float32)
    elig, have_elig = col(5, np.uint8)
    n, s = _select_args(per_region, min_specificity)
    h, text, ln = C.c_void_p(), C.c_void_p(), C.c_uint64()
    report = (C.c_uint64 * 6)()
    if min_spacing is None:
        _check(lib().gs_debug_design_host(regions._h, npart, chr_index.ctypes.data, counts.ctypes.data, seqs, pos, sense,
                                          spec if have_spec else None, elig if have_elig else None, pam.encode(), k,
                                          prefix.encode(), n, s, C.byref(h), C.byref(text) if rows else None, C.byref(ln)))
    else:
        _check(lib().gs_debug_design_host_spaced(regions._h, npart, chr_index.ctypes.data, counts.ctypes.data, seqs, pos, sense,
                                                 spec if have_spec else None, elig if have_elig else None, pam.encode(), k,
                                                 prefix.encode(), n, s, int(min_spacing), int(cut_offset),
                                                 GS_FLAG_PAM_AT_START if start else 0, C.byref(h),
                                                 C.byref(text) if rows else None, C.byref(ln), report))
    km = _selected_kmers(h, k, len(pam))
    try:
        sq, pm, ps, sn = km.to_host()
        ids, off, sp = km.ids_to_host()
        out = {"n": km.n, "seqs": sq.tobytes(), "pams": pm.tobytes(), "pos": ps, "sense_chars": sn, "ids": ids,
               "id_off": off, "sense": sp}
        if min_spacing is not None:
            out["last_select"] = dict(zip(("records", "kept", "groups_empty", "groups_short"), (int(x) for x in report[:4])))
            out["last_spacing"] = {"passed_over": int(report[4]), "groups_short_for_spacing": int(report[5])}
        if rows:
            out["rows"] = C.string_at(text, ln.value)
            lib().gs_free(text)
        return out
    finally:
        km.close()


class KmersFileError(GsError):
    """a kmers file that the host reader refuses: .message is that reader's message; kind, line, row, offset and text as
    in gs_kmers_report"""

    def __init__(self, status, msg, report):
        super().__init__(status, msg)
        self.message = msg
        self.kind, self.line, self.row = report["bad_kind"], report["bad_line"], report["bad_row"]
        self.offset, self.text = report["bad_off"], report["bad_text"]


def _kmers_report(rc, rep):
    """gs_kmers_report -> dict; raises for rc != 0"""
    text = C.string_at(rep.bad_text, rep.bad_len) if rep.bad_text else b""
    if rep.bad_text:
        lib().gs_free(rep.bad_text)
    report = {k: int(getattr(rep, k)) for k in ("n", "L", "P", "n_lines", "bad_kind", "bad_line", "bad_row", "bad_off")}
    report["bad_text"] = text
    report["ms"] = dict(zip(("file_reads", "upload_waits", "device_stage", "summaries", "line_starts", "line_walk",
                             "row_scan", "emit"), (float(x) for x in rep.ms)))
    if rc != 0 and report["bad_kind"]:
        what = ("", "kmers row with too few columns: ", "kmers position is not an integer: ", "empty kmers file",
                "kmers file lacks column ")[report["bad_kind"]]
        raise KmersFileError(rc, what + text.decode("latin-1"), report)
    _check(rc)
    return report


def parse_kmers_model_tiles(raw: bytes, tile_bytes):
    """the host model of the device reader with tiles of tile_bytes (gs_debug_kmers_host; no GPU) ->
    dict(n, L, P, seqs bytes, pams bytes, ids bytes, id_off uint64[n+1], sense uint8[n], report)"""
    h, rep = C.c_void_p(), GsKmersReport()
    raw = bytes(raw)
    rc = lib().gs_debug_kmers_host(raw if raw else None, len(raw), tile_bytes, C.byref(h), C.byref(rep))
    km = DeviceKmers._parsed(rc, h, rep, on_device=False)
    try:
        return kmers_arrays(km)
    finally:
        km.close()


def kmers_arrays(km):
    """the host copies of a parsed DeviceKmers as parse_kmers_model_tiles returns them"""
    seqs, pams, _, _ = km.to_host()
    ids, off, sp = km.ids_to_host()
    return {"n": km.n, "L": km.k, "P": km.P, "seqs": seqs.tobytes(), "pams": pams.tobytes(), "ids": ids, "id_off": off,
            "sense": sp, "report": km.report}


def kmers_tile_bytes() -> int:
    return int(lib().gs_debug_kmers_tile_bytes())


def kmers_chunk_bytes(set_to=0) -> int:
    """the staging chunk of gs_kmers_parse_file; set_to != 0 replaces it for the process"""
    return int(lib().gs_debug_kmers_chunk_bytes(set_to))


def generate_kmers(chrm, pam="NGG", k=20, start=False, device=0, chrm_device_ptr=None, chrm_len=None):
    """scripts/generate_kmers.py:70-118 for ONE chromosome on the GPU -> DeviceKmers.
    chrm: bytes / uint8 array (host), or pass chrm_device_ptr + chrm_len for text already in HBM."""
    h = C.c_void_p()
    flags = GS_FLAG_PAM_AT_START if start else 0
    if chrm_device_ptr is not None:
        _check(lib().gs_kmers_generate(device, chrm_device_ptr, int(chrm_len), 1, pam.encode(), k, flags, None,
                                       C.byref(h)))
    else:
        arr = np.frombuffer(bytes(chrm), dtype=np.uint8) if not isinstance(chrm, np.ndarray) else \
            np.ascontiguousarray(chrm, dtype=np.uint8)
        _check(lib().gs_kmers_generate(device, arr.ctypes.data if arr.size else None, arr.shape[0], 0,
                                       pam.encode(), k, flags, None, C.byref(h)))
    return DeviceKmers(h, k, len(pam))


def concat_kmers(parts):
    """the records of several DeviceKmers in one, in HBM, ids included when every part has them (gs_kmers_concat)"""
    arr = (C.c_void_p * max(1, len(parts)))(*[p._h for p in parts])
    h = C.c_void_p()
    _check(lib().gs_kmers_concat(arr, len(parts), C.byref(h)))
    km = DeviceKmers(h, parts[0].k if parts else 0, parts[0].P if parts else 0)
    if parts and all(hasattr(p, "ids_ptr") for p in parts):
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().gs_kmers_get_ids(h, 1, C.byref(a), C.byref(b), C.byref(c)))
        km.ids_ptr, km.id_offsets_ptr, km.sense_positive_ptr = a.value, b.value, c.value
    return km


def repr_doubles(values) -> list:
    """Python's repr() of each double as the decoder's kernels print it (gs_debug_repr_doubles; host only)"""
    v = np.ascontiguousarray(values, dtype=np.float64)
    out = np.zeros((v.shape[0], 32), np.uint8)
    _check(lib().gs_debug_repr_doubles(v.ctypes.data if v.size else None, v.shape[0], out.ctypes.data if v.size else None))
    return [r.tobytes().rstrip(b"\0").decode() for r in out]


def huffman_lengths(freq, max_len=15) -> np.ndarray:
    """the code lengths the BGZF compressor gives symbols with these counts, none above max_len (gs_debug_huffman_lengths;
    host only: the function its kernel runs)"""
    f = np.ascontiguousarray(freq, dtype=np.uint32)
    out = np.zeros(f.shape[0], np.uint8)
    _check(lib().gs_debug_huffman_lengths(f.ctypes.data, f.shape[0], max_len, out.ctypes.data))
    return out


def inflate_bgzf(data: bytes, device=0) -> bytes:
    """the bytes of BGZF members, inflated on the GPU (gs_bgzf_inflate); GsError(GS_ERR_FORMAT) names the first member
    that fails, its byte offset and the reason"""
    out, ln = C.c_void_p(), C.c_uint64()
    _check(lib().gs_bgzf_inflate(device, data, len(data), C.byref(out), C.byref(ln)))
    raw = C.string_at(out, ln.value)
    lib().gs_free(out)
    return raw


def inflate_member(member: bytes):
    """one BGZF member through the function the inflate kernel's lane runs (gs_debug_inflate_member; host only)
    -> (bytes made, reason: 0 when the member is sound)"""
    isize = int.from_bytes(member[-4:], "little") if len(member) >= 4 else 0
    cap = min(isize, 65536)
    out = np.zeros(max(cap, 1), np.uint8)
    ln, reason = C.c_uint64(), C.c_uint32()
    rc = lib().gs_debug_inflate_member(member, len(member), out.ctypes.data, cap, C.byref(ln), C.byref(reason))
    if rc != 0 and reason.value == 0:
        _check(rc)
    return out[:ln.value].tobytes(), reason.value


def bgzf_members(data: bytes):
    """the member table's walk (gs_debug_bgzf_members; host only) -> ([(offset, ISIZE)], reason); a refused member ends the
    list, reason says why"""
    n, reason = C.c_uint64(), C.c_uint32()
    rc = lib().gs_debug_bgzf_members(data, len(data), None, None, 0, C.byref(n), C.byref(reason))
    cap = n.value
    off, isz = np.zeros(max(cap, 1), np.uint64), np.zeros(max(cap, 1), np.uint32)
    rc = lib().gs_debug_bgzf_members(data, len(data), off.ctypes.data, isz.ctypes.data, cap, C.byref(n), C.byref(reason))
    if rc != 0 and reason.value == 0:
        _check(rc)
    return [(int(off[i]), int(isz[i])) for i in range(cap)], reason.value


def sp_float(q) -> float:
    """the float a BAM record's sp:f tag stores for a specificity printed as q / 10^6 (gs_debug_sp_float; host only)"""
    return float(lib().gs_debug_sp_float(int(q)))


def decode_tables():
    """the CFD tables the decoder uploads, keyed as the reference's score tables are -> (mm {key: float}, pam {pair: float})"""
    mm, pam = np.zeros(320), np.zeros(16)
    _check(lib().gs_debug_decode_tables(mm.ctypes.data, pam.ctypes.data))
    keys = {f"r{r}:d{d},{i + 1}": float(mm[(ri * 4 + di) * 20 + i]) for ri, r in enumerate("ACGU")
            for di, d in enumerate("ACGT") for i in range(20) if "TGCA"[ri] != d}
    return keys, {a + b: float(pam[ai * 4 + bi]) for ai, a in enumerate("ACGT") for bi, b in enumerate("ACGT")}


FASTA_RULES = {"index": 0, "records": 1}


class DeviceFasta:
    """A FASTA file parsed on one GPU (gs_fasta_parse*): the text stays in HBM until close().  rules: "index" (what
    `guidescan index` reads, seqio.parse_fasta) or "records" (SeqIO.to_dict, what `guidescan decode` reads)."""

    def __init__(self, handle, rules):
        self._h = handle
        self.rules = rules

    @classmethod
    def parse(cls, src, rules="index", device=0):
        """src: a path (read in chunks through page-locked staging), or the file's bytes (bytes or a uint8 array)"""
        h = C.c_void_p()
        if isinstance(src, (str, os.PathLike)):
            _check(lib().gs_fasta_parse_file(device, os.fsencode(src), FASTA_RULES[rules], C.byref(h)))
        else:
            raw = np.frombuffer(src, dtype=np.uint8) if isinstance(src, (bytes, bytearray, memoryview)) else np.ascontiguousarray(src, dtype=np.uint8)
            _check(lib().gs_fasta_parse(device, raw.ctypes.data if raw.size else None, raw.size, FASTA_RULES[rules], C.byref(h)))
        return cls(h, rules)

    @classmethod
    def parse_device(cls, d_raw_ptr, length, rules="index", device=0, stream=None):
        """the raw bytes are in HBM already (d_raw_ptr: a device address)"""
        h = C.c_void_p()
        _check(lib().gs_fasta_parse_device(device, d_raw_ptr if length else None, length, FASTA_RULES[rules], stream, C.byref(h)))
        return cls(h, rules)

    @classmethod
    def host_model(cls, raw: bytes, rules, tile_bytes):
        """gs_debug_fasta_host: the device passes run on the host with tiles of any size; no GPU"""
        h = C.c_void_p()
        raw = bytes(raw)
        _check(lib().gs_debug_fasta_host(raw if raw else None, len(raw), FASTA_RULES[rules], tile_bytes, C.byref(h)))
        return cls(h, rules)

    def info(self):
        """(records, bytes of the text, bytes of all names)"""
        n, tl, nb = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib().gs_fasta_info(self._h, C.byref(n), C.byref(tl), C.byref(nb)))
        return n.value, tl.value, nb.value

    def records(self):
        """{title_off, title_len, text_off, text_len, line_len: uint64 arrays; names: list of bytes}"""
        n, _, nb = self.info()
        cols = {k: np.zeros(n, dtype=np.uint64) for k in ("title_off", "title_len", "text_off", "text_len", "line_len")}
        name_off, names = np.zeros(n + 1, dtype=np.uint64), np.zeros(max(nb, 1), dtype=np.uint8)
        _check(lib().gs_fasta_records(self._h, *(cols[k].ctypes.data for k in ("title_off", "title_len", "text_off", "text_len", "line_len")),
                                      name_off.ctypes.data, names.ctypes.data))
        blob = names.tobytes()
        cols["names"] = [blob[int(name_off[r]):int(name_off[r + 1])] for r in range(n)]
        return cols

    def text(self) -> np.ndarray:
        """the text, copied to the host (uint8)"""
        p = C.c_void_p()
        _check(lib().gs_fasta_text(self._h, 0, C.byref(p)))
        tl = self.info()[1]
        return np.frombuffer(C.string_at(p, tl), dtype=np.uint8).copy() if tl else np.zeros(0, dtype=np.uint8)

    def text_device_ptr(self) -> int:
        p = C.c_void_p()
        _check(lib().gs_fasta_text(self._h, 1, C.byref(p)))
        return p.value or 0

    def ms(self):
        """milliseconds of the object's making, by host clocks: file reads, waits for the uploads, "kernels" = the device
        stage (its allocations, the five passes, the waits for their results), title gather with the names; "passes": the
        five passes alone, by events in the stream (tile summaries, their two scans, tile counts, the counts' scan, emit)"""
        v = np.zeros(9, np.float64)
        _check(lib().gs_debug_fasta_ms(self._h, v.ctypes.data))
        out = dict(zip(("read", "upload", "kernels", "names"), (float(x) for x in v[:4])))
        out["passes"] = dict(zip(("summaries", "summary_scans", "counts", "count_scan", "emit"), (float(x) for x in v[4:])))
        return out

    def close(self):
        if self._h:
            lib().gs_fasta_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _fasta_result(fa):
    rec = fa.records()
    text = fa.text()
    if fa.rules == "index":
        return text, [n.decode("latin-1") for n in rec["names"]], [int(x) for x in rec["line_len"]]
    blob = text.tobytes()
    return {n.decode("latin-1"): blob[int(o):int(o) + int(l)] for n, o, l in zip(rec["names"], rec["text_off"], rec["text_len"])}


def parse_fasta_device(path_or_bytes, rules="index", device=0):
    """A FASTA file parsed on the GPU.  rules="index": (text uint8[L], names, lengths), the tuple of seqio.parse_fasta;
    rules="records": {name: symbols as bytes}, what SeqIO.to_dict holds (a name twice: GsError, GS_ERR_FORMAT)."""
    with DeviceFasta.parse(path_or_bytes, rules, device) as fa:
        return _fasta_result(fa)


def parse_fasta_model_tiles(raw: bytes, rules, tile_bytes):
    """the same result from the host model of the device passes with tiles of tile_bytes (gs_debug_fasta_host), plus the
    record table: (result as parse_fasta_device, records dict of DeviceFasta.records)"""
    with DeviceFasta.host_model(raw, rules, tile_bytes) as fa:
        return _fasta_result(fa), fa.records()


def fasta_tile_bytes() -> int:
    return int(lib().gs_debug_fasta_tile_bytes())


def fasta_chunk_bytes(set_to=0) -> int:
    """the staging chunk of gs_fasta_parse_file; set_to != 0 replaces it for the process"""
    return int(lib().gs_debug_fasta_chunk_bytes(set_to))


class Decoder:
    """A SAM/BAM database's decoder on one GPU (gs_decoder_open): sq = [(name, LN)] of the @SQ lines, fasta =
    {name: symbols} of the genome's FASTA records (decode.parse_fasta_records), or a DeviceFasta parsed under the
    "records" rules, whose text then goes to the decoder inside HBM (gs_decoder_open_fasta).  decode_records() takes
    decode.Record objects and returns the rows scripts/decode_database.py prints, without the header line."""

    def __init__(self, sq, fasta, device=0):
        names = [n for n, _ in sq]
        if isinstance(fasta, DeviceFasta):
            self.names = names
            gs = self._gs = make_genome_structure(names, [n for _, n in sq])
            h = C.c_void_p()
            _check(lib().gs_decoder_open_fasta(device, fasta._h, C.byref(gs), C.byref(h)))
            self._h = h
            return
        parts, off, ln, at = [], [], [], 0
        for n in names:
            if n in fasta:
                b = fasta[n].encode("latin-1")
                parts.append(b)
                off.append(at)
                ln.append(len(b))
                at += len(b)
            else:
                off.append(0)
                ln.append(2**64 - 1)
        text = np.frombuffer(b"".join(parts), dtype=np.uint8)
        self.names = names
        gs = self._gs = make_genome_structure(names, [n for _, n in sq])
        off, ln = np.array(off, dtype=np.uint64), np.array(ln, dtype=np.uint64)
        h = C.c_void_p()
        _check(lib().gs_decoder_open(device, text.ctypes.data if text.size else None, text.shape[0], C.byref(gs),
                                     off.ctypes.data if len(names) else None, ln.ctypes.data if len(names) else None, C.byref(h)))
        self._h = h

    def _batch(self, records):
        index = {}
        for i, n in enumerate(self.names):
            index.setdefault(n, i)

        def blob(items):
            items = [x.encode("latin-1") for x in items]
            return (np.frombuffer(b"".join(items) + b"\0", dtype=np.uint8),
                    np.cumsum([0] + [len(x) for x in items], dtype=np.uint64))

        ids, id_off = blob([r.id for r in records])
        seqs, seq_off = blob([r.seq for r in records])
        hexs, hex_off = blob([r.hex or "" for r in records])
        rev = np.array([1 if r.reverse else 0 for r in records], dtype=np.uint8)
        chrm = np.array([index.get(r.rname, -1) for r in records], dtype=np.int32)
        pos0 = np.array([r.pos0 for r in records], dtype=np.int64)
        keep = (ids, id_off, seqs, seq_off, hexs, hex_off, rev, chrm, pos0)
        b = GsDecodeBatch(len(records), ids.ctypes.data, id_off.ctypes.data, seqs.ctypes.data, seq_off.ctypes.data,
                          rev.ctypes.data, chrm.ctypes.data, pos0.ctypes.data, hexs.ctypes.data, hex_off.ctypes.data)
        return b, keep

    def set_annotation(self, annotation):
        """attaches an Annotation built for the decoder's device against its @SQ lines, None detaches
        (gs_decoder_set_annotation); the decoder keeps it alive.  features=True in the decode_* calls then adds the
        columns, features_only=True (complete mode) leaves out the rows without a feature"""
        _check(lib().gs_decoder_set_annotation(self._h, annotation._h if annotation is not None else None))
        self._annotation = annotation

    def annot_ms(self) -> float:
        """the annotation pass of the last batch that ran one, in milliseconds (gs_debug_decode_annot_ms)"""
        ms = C.c_double()
        _check(lib().gs_debug_decode_annot_ms(self._h, C.byref(ms)))
        return float(ms.value)

    @staticmethod
    def _feature_flags(features, features_only):
        return (GS_TEXT_FEATURES if features else 0) | (GS_DECODE_FEATURES_ONLY if features_only else 0)

    def decode_records(self, records, complete=False, first_record=0, on_device=False, features=False, features_only=False) -> str:
        """on_device: through gs_decode_records_device, the text copied back from HBM here"""
        if not records:
            return ""
        b, keep = self._batch(records)
        flags = (GS_TEXT_COMPLETE if complete else 0) | self._feature_flags(features, features_only)
        out, ln, rows = C.c_void_p(), C.c_uint64(), C.c_uint64()
        fn = lib().gs_decode_records_device if on_device else lib().gs_decode_records
        _check(fn(self._h, C.byref(b), flags, first_record, C.byref(out), C.byref(ln), C.byref(rows)))
        self.last_rows = rows.value
        if on_device:
            if ln.value == 0:
                return ""
            hip = C.CDLL("libamdhip64.so")
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            host = np.empty(ln.value, dtype=np.uint8)
            if hip.hipMemcpy(host.ctypes.data, out, ln.value, 2) != 0:
                raise GsError(2, "copy of the decoded text")
            return host.tobytes().decode("latin-1")
        s = C.string_at(out, ln.value).decode("latin-1")
        lib().gs_free(out)
        return s

    def decode_sam(self, sam: bytes, complete=False, header=True, first_record=0, features=False, features_only=False) -> str:
        flags = ((GS_TEXT_COMPLETE if complete else 0) | (0 if header else GS_DECODE_NO_HEADER) |
                 self._feature_flags(features, features_only))
        out, ln, n = C.c_void_p(), C.c_uint64(), C.c_uint64()
        _check(lib().gs_decode_sam(self._h, sam, len(sam), flags, first_record, C.byref(out), C.byref(ln), C.byref(n)))
        s = C.string_at(out, ln.value).decode("latin-1")
        lib().gs_free(out)
        return s

    def inflate_base(self, members_before=0, bytes_before=0):
        """where the next calls' members lie in their file: added to the index and offset an error names (gs_bgzf_inflate_base)"""
        _check(lib().gs_bgzf_inflate_base(self._h, members_before, bytes_before))

    def inflate_bgzf(self, data: bytes, keep=0) -> bytes:
        """BGZF members inflated into the decoder's workspace (gs_bgzf_inflate_device), `keep` bytes of the call before in
        front; copied back from HBM here"""
        out, ln, nm = C.c_void_p(), C.c_uint64(), C.c_uint64()
        _check(lib().gs_bgzf_inflate_device(self._h, data, len(data), keep, C.byref(out), C.byref(ln), C.byref(nm)))
        self.last_members = nm.value
        if ln.value == 0:
            return b""
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        host = np.empty(ln.value, dtype=np.uint8)
        if hip.hipMemcpy(host.ctypes.data, out, ln.value, 2) != 0:
            raise GsError(2, "copy of the inflated bytes")
        return host.tobytes()

    def decode_bam(self, bgzf: bytes, skip=0, ref_to_sq=(), complete=False, first_record=0, end=False, on_device=False,
                   features=False, features_only=False):
        """whole BGZF members of a BAM database -> (rows without the header line, complete records, bytes of a cut record
        that the decoder keeps for the next call) (gs_decode_bam; on_device: gs_decode_bam_device, the text copied back
        here).  skip: inflated bytes of the BAM header, in the first call of a file; ref_to_sq: the binary reference
        list's entries as indices into sq (negative: none); end: the data ends here"""
        flags = ((GS_TEXT_COMPLETE if complete else 0) | (GS_DECODE_BAM_END if end else 0) |
                 self._feature_flags(features, features_only))
        m = np.ascontiguousarray(ref_to_sq, dtype=np.int32)
        out, ln, n, tail = C.c_void_p(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        fn = lib().gs_decode_bam_device if on_device else lib().gs_decode_bam
        _check(fn(self._h, bgzf, len(bgzf), skip, m.ctypes.data if m.size else None, m.size, flags, first_record,
                  C.byref(out), C.byref(ln), C.byref(n), C.byref(tail)))
        if on_device:
            host = np.empty(ln.value, dtype=np.uint8)
            if ln.value:
                hip = C.CDLL("libamdhip64.so")
                hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
                if hip.hipMemcpy(host.ctypes.data, out, ln.value, 2) != 0:
                    raise GsError(2, "copy of the decoded text")
            text = host.tobytes().decode("latin-1")
        else:
            text = C.string_at(out, ln.value).decode("latin-1")
            lib().gs_free(out)
        return text, n.value, tail.value

    def decode_bam_last(self):
        """the last decode_bam call: ({members, compressed, inflated, records}, {inflate, starts, fields, decode} in ms)"""
        c, ms = np.zeros(4, np.uint64), np.zeros(4, np.float64)
        _check(lib().gs_debug_decode_bam_last(self._h, c.ctypes.data, ms.ctypes.data))
        return (dict(zip(("members", "compressed", "inflated", "records"), (int(x) for x in c))),
                dict(zip(("inflate", "starts", "fields", "decode"), (float(x) for x in ms))))

    def close(self):
        if self._h:
            lib().gs_decoder_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def sdsl_extract_text(index_file) -> np.ndarray:
    """genome text held in a reference `.forward` / `.reverse` index file"""
    out, n = C.c_void_p(), C.c_uint64()
    _check(lib().gs_sdsl_extract_text(str(index_file).encode(), C.byref(out), C.byref(n)))
    t = np.frombuffer(C.string_at(out, n.value), dtype=np.uint8).copy()
    lib().gs_free(out)
    return t


def sdsl_sections(counts):
    """(tree, alphabet): the serialised _byte_tree and byte_alphabet sections of a reference index file whose text,
    sentinel included, has these 256 symbol counts (gs_debug_sdsl_sections; host only)"""
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    if counts.shape != (256,):
        raise ValueError("counts: 256 entries, one per byte value")
    t, tn, a, an = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
    _check(lib().gs_debug_sdsl_sections(counts.ctypes.data, C.byref(t), C.byref(tn), C.byref(a), C.byref(an)))
    tree, alphabet = C.string_at(t, tn.value), C.string_at(a, an.value)
    lib().gs_free(t)
    lib().gs_free(a)
    return tree, alphabet


def sdsl_export_scratch() -> int:
    """peak device scratch in bytes of this process's last GenomeIndex.save_sdsl"""
    return int(lib().gs_debug_sdsl_export_scratch())


def decode_sequence_ex(hit) -> str:
    """match.sequence of one HIT_EX_DTYPE record"""
    return bytes(hit["seq"])[:int(hit["seq_len"])].decode()


def format_guide_ex(gs, gid, sequence, pam, sense_positive, hits, mismatches, sam=False, complete=True,
                    start=False, max_off_targets=-1, features=None) -> str:
    """hits: numpy HIT_EX_DTYPE array of this guide (bulge path); features: an Annotation - with the match_features
    column (gs_format_guide_ex_features)"""
    hits = np.ascontiguousarray(hits, dtype=HIT_EX_DTYPE)
    k = GsKmer(gid.encode(), sequence.encode(), pam.encode(), int(sense_positive))
    out, n = C.c_void_p(), C.c_size_t()
    flags = ((GS_TEXT_SAM if sam else 0) | (GS_TEXT_COMPLETE if complete else 0) |
             (GS_FLAG_PAM_AT_START if start else 0))
    if features is not None:
        _check(lib().gs_format_guide_ex_features(C.byref(gs), C.byref(k), hits.ctypes.data, hits.shape[0], mismatches,
                                                 flags | GS_TEXT_FEATURES, max_off_targets, features._h, C.byref(out), C.byref(n)))
    else:
        _check(lib().gs_format_guide_ex(C.byref(gs), C.byref(k), hits.ctypes.data, hits.shape[0], mismatches,
                                        flags, max_off_targets, C.byref(out), C.byref(n)))
    s = C.string_at(out, n.value).decode()
    lib().gs_free(out)
    return s


def decode_sequence(guide: str, P: int, key: int, flags: int = 0) -> str:
    buf = C.create_string_buffer(len(guide) + P + 1)
    _check(lib().gs_decode_sequence(guide.encode(), len(guide), P, flags, key, buf))
    return buf.value.decode()


class GenomeIndex:
    """Both strand indexes of one genome in one GPU's HBM.  Mirrors the pair of
    genome_index objects of src/guidescan.cxx:210-211."""

    def __init__(self, handle, device):
        self._h = handle
        self.device = device

    @classmethod
    def build(cls, text: np.ndarray, device: int = 0, sa_fwd=None, sa_rev=None):
        text = np.ascontiguousarray(text, dtype=np.uint8)
        h = C.c_void_p()
        if sa_fwd is not None:
            sa_fwd = np.ascontiguousarray(sa_fwd, dtype=np.uint32)
            sa_rev = np.ascontiguousarray(sa_rev, dtype=np.uint32)
            _check(lib().gs_index_build_with_sa(text.ctypes.data, text.shape[0], sa_fwd.ctypes.data,
                                                sa_rev.ctypes.data, device, C.byref(h)))
        else:
            _check(lib().gs_index_build(text.ctypes.data, text.shape[0], device, C.byref(h)))
        return cls(h, device)

    def save_sa(self, text, path):
        """store both suffix arrays next to the text (gs_index_save_sa)"""
        text = np.ascontiguousarray(text, dtype=np.uint8)
        _check(lib().gs_index_save_sa(self._h, text.ctypes.data, text.shape[0], str(path).encode()))

    def save_sdsl(self, text, prefix):
        """write <prefix>.forward and <prefix>.reverse, the reference's own index files, byte for byte
        (gs_index_save_sdsl); text as given to build"""
        text = np.ascontiguousarray(text, dtype=np.uint8)
        _check(lib().gs_index_save_sdsl(self._h, text.ctypes.data, text.shape[0], str(prefix).encode()))

    @classmethod
    def open_sa(cls, text, path, device: int = 0):
        """text + stored suffix arrays -> index without the suffix sort (gs_index_open_sa)"""
        text = np.ascontiguousarray(text, dtype=np.uint8)
        h = C.c_void_p()
        _check(lib().gs_index_open_sa(text.ctypes.data, text.shape[0], str(path).encode(), device, C.byref(h)))
        return cls(h, device)

    @classmethod
    def open_sdsl(cls, prefix, device: int = 0):
        """import the reference's <prefix>.forward index file (sdsl::load_from_file replacement)"""
        h = C.c_void_p()
        _check(lib().gs_index_open_sdsl(str(prefix).encode(), device, C.byref(h)))
        return cls(h, device)

    def close(self):
        if self._h:
            lib().gs_index_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def genome_length(self):
        return int(lib().gs_index_genome_length(self._h))

    @property
    def device_bytes(self):
        return int(lib().gs_index_device_bytes(self._h))

    def meta(self, strand=0):
        c = (C.c_uint64 * 5)()
        n = C.c_uint64()
        _check(lib().gs_index_meta(self._h, strand, c, C.byref(n)))
        return list(c), int(n.value)

    def rank_bwt4(self, rows, strand=0):
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        out = np.empty((rows.shape[0], 4), dtype=np.uint64)
        _check(lib().gs_rank_bwt4(self._h, strand, rows.ctypes.data, rows.shape[0], out.ctypes.data))
        return out

    def resolve(self, rows, strand=0):
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        out = np.empty(rows.shape[0], dtype=np.uint64)
        _check(lib().gs_resolve(self._h, strand, rows.ctypes.data, rows.shape[0], out.ctypes.data))
        return out

    def suffix_array(self, strand=0):
        _, n = self.meta(strand)
        out = np.empty(n, dtype=np.uint32)
        _check(lib().gs_index_copy_sa(self._h, strand, out.ctypes.data))
        return out

    def verify_sa(self, text, strand=0, samples=1 << 20, seed=1):
        """self-check from the text alone -> dict of gs_sa_report (all counters but rows/sampled must be 0).
        samples="all": every adjacent pair of rows by the linear-time rule (GS_VERIFY_ALL_ROWS) - a complete proof"""
        text = np.ascontiguousarray(text, dtype=np.uint8)
        rep = GsSaReport()
        if samples == "all":
            samples = (1 << 64) - 1
        _check(lib().gs_index_verify_sa(self._h, strand, text.ctypes.data, text.shape[0], samples, seed,
                                        C.byref(rep)))
        return {k: int(getattr(rep, k)) for k, _ in GsSaReport._fields_}

    def enumerate(self, seqs: np.ndarray, pams: np.ndarray, mismatches=3, alt_pams=(), start=False,
                  faithful=False, raw_counts=False, no_new_tables=False):
        """seqs uint8[n,L], pams uint8[n,P] -> (offsets uint64[n+1], hits HIT_DTYPE[], stats dict).
        Hits of guide i are hits[offsets[i]:offsets[i+1]] in the reference's canonical order."""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        n, L = seqs.shape
        pams = np.ascontiguousarray(pams, dtype=np.uint8)
        P = pams.shape[1] if pams.ndim == 2 else 0
        pams = pams.reshape(n, P)
        alt = b"".join(p.encode() for p in alt_pams)
        for p in alt_pams:
            if len(p) != P:
                raise ValueError("alt PAM length differs from the guides' PAM length")
        r = C.c_void_p()
        flags = ((GS_FLAG_PAM_AT_START if start else 0) | (GS_FLAG_FAITHFUL_WALK if faithful else 0) |
                 (GS_FLAG_RAW_COUNTS if raw_counts else 0) | (GS_FLAG_NO_NEW_TABLES if no_new_tables else 0))
        _check(lib().gs_enumerate(self._h, seqs.ctypes.data, n, L, pams.ctypes.data if P else None, P,
                                  alt if alt_pams else None, len(alt_pams), mismatches, flags,
                                  C.byref(r)))
        try:
            v = GsResultView()
            _check(lib().gs_result_get(r, C.byref(v)))
            offsets = np.ctypeslib.as_array(v.guide_offsets, shape=(n + 1,)).copy()
            if v.n_hits:
                raw = C.string_at(C.cast(v.hits, C.c_void_p), int(v.n_hits) * 16)
                hits = np.frombuffer(raw, dtype=HIT_DTYPE).copy()
            else:
                hits = np.empty(0, dtype=HIT_DTYPE)
            stats = dict(n_ext=int(v.n_ext), n_matches=int(v.n_matches), n_hits=int(v.n_hits),
                         ms_search=float(v.ms_search), ms_total=float(v.ms_total),
                         raw_hits=(np.ctypeslib.as_array(v.raw_hits, shape=(n,)).copy() if raw_counts and n and v.raw_hits
                                   else None),
                         needs_general=(np.nonzero(np.ctypeslib.as_array(v.guide_flags, shape=(n,)) & 1)[0].tolist()
                                        if v.n_unsupported and n else []))
        finally:
            lib().gs_result_free(r)
        return offsets, hits, stats

    def annotate(self, annotation, gs, offsets, hits, L, P, mismatches):
        """the features of every hit of a CSR hit list (gs_annotate; offsets[0] need not be 0) -> (feat_offsets
        uint64[n_hits + 1], feats uint32 group numbers, guide_counts uint32[n, mismatches + 1]: per guide and distance the
        hits that have a row and a feature)"""
        return _annotate_call(lib().gs_annotate, (self._h,), annotation, gs, offsets, hits, L, P, mismatches)

    def annotate_device(self, annotation, gs, n, L, P, mismatches, d_offsets_ptr, d_hits_ptr, stream=None):
        """device-resident variant (gs_annotate_device): raw device addresses in, (feat_offsets, feats, guide_counts)
        device addresses out, owned by the handle until the next call on it"""
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().gs_annotate_device(self._h, annotation._h, C.byref(gs), n, L, P, mismatches, d_offsets_ptr, d_hits_ptr,
                                        stream, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def set_annotation(self, annotation):
        """attach the Annotation the text calls' features=True looks rows up in; None detaches
        (gs_index_set_annotation)"""
        _check(lib().gs_index_set_annotation(self._h, annotation._h if annotation is not None else None))
        self._annotation = annotation

    def score(self, gs, seqs, P, offsets, hits, sam=False, start=False, max_off_targets=-1, want_cfd=True):
        """CFD per hit and specificity per guide on the device (printer.hpp:98-113, 115-170, 251-297)
        -> (cfd float32[n_hits] or None, specificity float32[n])"""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        n, L = seqs.shape
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
        cfd = np.empty(hits.shape[0], dtype=np.float32) if want_cfd else None
        spec = np.empty(n, dtype=np.float32)
        flags = (GS_TEXT_SAM if sam else 0) | (GS_FLAG_PAM_AT_START if start else 0)
        _check(lib().gs_score(self._h, seqs.ctypes.data, n, L, P, flags, max_off_targets, C.byref(gs),
                              offsets.ctypes.data, hits.ctypes.data if hits.shape[0] else None,
                              cfd.ctypes.data if want_cfd and hits.shape[0] else None, spec.ctypes.data))
        return cfd, spec

    def score_device(self, gs, d_guides_ptr, n, L, P, d_offsets_ptr, d_hits_ptr, d_cfd_ptr, d_spec_ptr,
                     sam=False, start=False, max_off_targets=-1, stream=None):
        """device-resident variant: all pointers are raw device addresses"""
        flags = (GS_TEXT_SAM if sam else 0) | (GS_FLAG_PAM_AT_START if start else 0)
        _check(lib().gs_score_device(self._h, d_guides_ptr, n, L, P, flags, max_off_targets, C.byref(gs),
                                     d_offsets_ptr, d_hits_ptr, stream, d_cfd_ptr, d_spec_ptr))

    def format_device(self, gs, d_guides_ptr, n, L, d_pams_ptr, P, ids, senses, skip, d_offsets_ptr, d_hits_ptr,
                      d_spec_ptr, mismatches, sam=False, complete=True, start=False, max_off_targets=-1, stream=None, bam=False, bgzf=False,
                      features=False):
        """the database text of a fast-path batch encoded in HBM (gs_format_device): raw device addresses in (ids,
        senses and skip are host sequences, the last two may be None), (d_text_ptr, length) out - device memory of
        the handle, valid until the next call on it; the bytes are those of format_guides.  bam=True (in place of sam):
        the SAM lines as BAM alignment blocks; bgzf=True with it: the blocks' BGZF members"""
        blob, off = _id_blob(ids)
        if len(ids) != n:
            raise ValueError("one id per guide")
        se, sk = _bytes_or_none(senses, n), _bytes_or_none(skip, n)
        flags = ((GS_TEXT_SAM if sam else 0) | (GS_TEXT_COMPLETE if complete else 0) |
                 (GS_FLAG_PAM_AT_START if start else 0) | (GS_TEXT_BAM if bam else 0) | (GS_TEXT_BGZF if bgzf else 0) |
                 (GS_TEXT_FEATURES if features else 0))
        d_text, ln = C.c_void_p(), C.c_uint64()
        keep = C.create_string_buffer(blob, len(blob) + 1)
        _check(lib().gs_format_device(self._h, C.byref(gs), d_guides_ptr, n, L, d_pams_ptr, P, C.addressof(keep),
                                      off.ctypes.data, se.ctypes.data if se is not None else None,
                                      sk.ctypes.data if sk is not None else None, d_offsets_ptr, d_hits_ptr, d_spec_ptr,
                                      mismatches, flags, max_off_targets, stream, C.byref(d_text), C.byref(ln)))
        return d_text.value, int(ln.value)

    def enumerate_text(self, seqs, pams, ids, senses, gs, mismatches=3, alt_pams=(), start=False, sam=False,
                       complete=True, max_off_targets=-1, skip=None, bam=False, bgzf=False, features=False) -> bytes:
        """guides in, database text out (gs_enumerate_text): search, scoring and encoding on the device.  Raises
        GsError with status 3 (GS_ERR_UNSUPPORTED) when a guide of the batch needs the general path."""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        n, L = seqs.shape
        pams = np.ascontiguousarray(pams, dtype=np.uint8)
        P = pams.shape[1] if pams.ndim == 2 else 0
        pams = pams.reshape(n, P)
        for p in alt_pams:
            if len(p) != P:
                raise ValueError("alt PAM length differs from the guides' PAM length")
        alt = b"".join(p.encode() for p in alt_pams)
        if len(ids) != n:
            raise ValueError("one id per guide")
        blob, off = _id_blob(ids)
        se, sk = _bytes_or_none(senses, n), _bytes_or_none(skip, n)
        flags = ((GS_TEXT_SAM if sam else 0) | (GS_TEXT_COMPLETE if complete else 0) |
                 (GS_FLAG_PAM_AT_START if start else 0) | (GS_TEXT_BAM if bam else 0) | (GS_TEXT_BGZF if bgzf else 0) |
                 (GS_TEXT_FEATURES if features else 0))
        keep = C.create_string_buffer(blob, len(blob) + 1)
        out, ln = C.c_void_p(), C.c_uint64()
        _check(lib().gs_enumerate_text(self._h, seqs.ctypes.data, n, L, pams.ctypes.data if P else None, P,
                                       alt if alt_pams else None, len(alt_pams), mismatches, flags, max_off_targets,
                                       C.byref(gs), C.addressof(keep), off.ctypes.data,
                                       se.ctypes.data if se is not None else None,
                                       sk.ctypes.data if sk is not None else None, C.byref(out), C.byref(ln), None))
        s = C.string_at(out, ln.value)
        lib().gs_free(out)
        return s

    def format_device_ids(self, gs, d_guides_ptr, n, L, d_pams_ptr, P, d_ids_ptr, d_id_offsets_ptr, d_senses_ptr, skip,
                          d_offsets_ptr, d_hits_ptr, d_spec_ptr, mismatches, sam=False, complete=True, start=False,
                          max_off_targets=-1, stream=None, bam=False, bgzf=False, features=False):
        """format_device with ids, id offsets and senses that are in HBM already (gs_format_device_ids): raw device
        addresses; `skip` stays a host sequence or None"""
        sk = _bytes_or_none(skip, n)
        flags = ((GS_TEXT_SAM if sam else 0) | (GS_TEXT_COMPLETE if complete else 0) |
                 (GS_FLAG_PAM_AT_START if start else 0) | (GS_TEXT_BAM if bam else 0) | (GS_TEXT_BGZF if bgzf else 0) |
                 (GS_TEXT_FEATURES if features else 0))
        d_text, ln = C.c_void_p(), C.c_uint64()
        _check(lib().gs_format_device_ids(self._h, C.byref(gs), d_guides_ptr, n, L, d_pams_ptr, P, d_ids_ptr,
                                          d_id_offsets_ptr, d_senses_ptr, sk.ctypes.data if sk is not None else None,
                                          d_offsets_ptr, d_hits_ptr, d_spec_ptr, mismatches, flags, max_off_targets, stream,
                                          C.byref(d_text), C.byref(ln)))
        return d_text.value, int(ln.value)

    def enumerate_text_device(self, d_guides_ptr, n, L, d_pams_ptr, P, d_ids_ptr, d_id_offsets_ptr, d_senses_ptr, gs,
                              mismatches=3, alt_pams=(), start=False, sam=False, complete=True, max_off_targets=-1,
                              skip=None, bam=False, bgzf=False, features=False) -> bytes:
        """enumerate_text over guides, ids and senses in HBM (gs_enumerate_text_device): only the text comes back.
        Raises GsError with status 3 when a guide needs the general path or 2L + 3P > 59."""
        alt = b"".join(p.encode() for p in alt_pams)
        sk = _bytes_or_none(skip, n)
        flags = ((GS_TEXT_SAM if sam else 0) | (GS_TEXT_COMPLETE if complete else 0) |
                 (GS_FLAG_PAM_AT_START if start else 0) | (GS_TEXT_BAM if bam else 0) | (GS_TEXT_BGZF if bgzf else 0) |
                 (GS_TEXT_FEATURES if features else 0))
        out, ln = C.c_void_p(), C.c_uint64()
        _check(lib().gs_enumerate_text_device(self._h, d_guides_ptr, n, L, d_pams_ptr, P, alt if alt_pams else None,
                                              len(alt_pams), mismatches, flags, max_off_targets, C.byref(gs), d_ids_ptr,
                                              d_id_offsets_ptr, d_senses_ptr, sk.ctypes.data if sk is not None else None,
                                              C.byref(out), C.byref(ln), None, None))
        s = C.string_at(out, ln.value)
        lib().gs_free(out)
        return s

    def raw_counts_device(self, d_guides_ptr, n, L, d_pams_ptr, P, gs, mismatches, alt_pams=(), start=False):
        """the counting pass of --threshold over guides in HBM (gs_enumerate_text_device with GS_FLAG_RAW_COUNTS):
        hits per guide before duplicate sequences collapse, uint32[n]"""
        alt = b"".join(p.encode() for p in alt_pams)
        raw = np.zeros(n, dtype=np.uint32)
        flags = GS_FLAG_RAW_COUNTS | (GS_FLAG_PAM_AT_START if start else 0)
        _check(lib().gs_enumerate_text_device(self._h, d_guides_ptr, n, L, d_pams_ptr, P, alt if alt_pams else None,
                                              len(alt_pams), mismatches, flags, -1, C.byref(gs), None, None, None, None,
                                              None, None, None, raw.ctypes.data))
        return raw

    def bgzf_compress(self, raw) -> bytes:
        """BGZF members of `raw` (bytes or a uint8 array), compressed on the device; no end-of-file block
        (gs_bgzf_compress)"""
        a = np.frombuffer(bytes(raw), dtype=np.uint8) if not isinstance(raw, np.ndarray) else np.ascontiguousarray(raw, dtype=np.uint8)
        out, ln = C.c_void_p(), C.c_uint64()
        _check(lib().gs_bgzf_compress(self._h, a.ctypes.data if a.size else None, a.size, C.byref(out), C.byref(ln)))
        try:
            return C.string_at(out.value, ln.value) if ln.value else b""
        finally:
            if out.value:
                lib().gs_free(out)

    def bgzf_compress_device(self, d_raw_ptr, raw_len, stream=None):
        """BGZF members of raw_len bytes that are in HBM: (device pointer owned by the handle, length)
        (gs_bgzf_compress_device)"""
        out, ln = C.c_void_p(), C.c_uint64()
        _check(lib().gs_bgzf_compress_device(self._h, d_raw_ptr, raw_len, stream, C.byref(out), C.byref(ln)))
        return out.value, ln.value

    def last_text_offsets(self, n):
        """byte offset at which each guide's lines begin in the text of the last format_device / enumerate_text of n
        guides on this handle, uint64[n+1] (gs_index_last_text_offsets)"""
        out = np.empty(n + 1, dtype=np.uint64)
        _check(lib().gs_index_last_text_offsets(self._h, out.ctypes.data, n))
        return out

    def enumerate_general(self, seqs, pams, mismatches=3, rna_bulges=0, dna_bulges=0, alt_pams=(),
                          start=False, force_pams=False, raw=False):
        """the general path (any symbol, any number of PAMs, bulges) -> (offsets uint64[n+1], hits HIT_EX_DTYPE[])"""
        return self.enumerate_bulges(seqs, pams, mismatches, rna_bulges, dna_bulges, alt_pams, start, force_pams, raw)

    def enumerate_bulges(self, seqs, pams, mismatches=3, rna_bulges=0, dna_bulges=0, alt_pams=(),
                         start=False, force_pams=False, raw=False):
        """bulge-aware search (index.hpp:250-375) -> (offsets uint64[n+1], hits HIT_EX_DTYPE[]).  Alt PAMs whose lengths
        differ from one another or from the guides' PAM go through gs_enumerate_general_pams with a length per pattern;
        force_pams=True takes that entry point for equal lengths too.  raw=True: a third value, uint32[n], the hits of
        each guide before duplicate sequences are dropped (gs_result_ex_raw_hits)."""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        n, L = seqs.shape
        pams = np.ascontiguousarray(pams, dtype=np.uint8)
        P = pams.shape[1] if pams.ndim == 2 else 0
        pams = pams.reshape(n, P)
        alt = b"".join(p.encode() for p in alt_pams)
        flags = GS_FLAG_PAM_AT_START if start else 0
        r = C.c_void_p()
        if force_pams or any(len(p) != P for p in alt_pams):
            lens = np.array([len(p) for p in alt_pams], dtype=np.uint32)
            _check(lib().gs_enumerate_general_pams(self._h, seqs.ctypes.data, n, L, pams.ctypes.data if P else None, P,
                                                   alt if alt_pams else None, lens.ctypes.data if alt_pams else None,
                                                   len(alt_pams), mismatches, rna_bulges, dna_bulges, flags, C.byref(r)))
        else:
            _check(lib().gs_enumerate_bulges(self._h, seqs.ctypes.data, n, L, pams.ctypes.data if P else None, P,
                                             alt if alt_pams else None, len(alt_pams), mismatches, rna_bulges,
                                             dna_bulges, flags, C.byref(r)))
        try:
            ng, po, ph = C.c_uint64(), C.c_void_p(), C.c_void_p()
            _check(lib().gs_result_ex_get(r, C.byref(ng), C.byref(po), C.byref(ph)))
            offsets = np.frombuffer(C.string_at(po, 8 * (n + 1)), dtype=np.uint64).copy()
            nh = int(offsets[-1])
            hits = (np.frombuffer(C.string_at(ph, 48 * nh), dtype=HIT_EX_DTYPE).copy() if nh
                    else np.empty(0, dtype=HIT_EX_DTYPE))
            if raw:
                pr = C.c_void_p()
                _check(lib().gs_result_ex_raw_hits(r, C.byref(pr)))
                raw_hits = (np.frombuffer(C.string_at(pr, 4 * n), dtype=np.uint32).copy() if n
                            else np.empty(0, dtype=np.uint32))
        finally:
            lib().gs_result_ex_free(r)
        return (offsets, hits, raw_hits) if raw else (offsets, hits)

    def general_last(self):
        """the last general-path call on this handle (gs_debug_general_last): [items, workgroups, the first pass's pool,
        match records T, search passes, largest stack of any item, steps the room rule cut, steps without room]"""
        out = (C.c_uint64 * 8)()
        _check(lib().gs_debug_general_last(self._h, out))
        return [int(x) for x in out]

    def bulge_last(self):
        """the same call's routing and the seeded form's counters (gs_debug_bulge_last): [guides seeded, guides walked,
        seeds looked up, seeds with an empty interval, row nodes, interval nodes, exception-row lookups, largest stack]"""
        out = (C.c_uint64 * 8)()
        _check(lib().gs_debug_bulge_last(self._h, out))
        return [int(x) for x in out]

    def locked(self):
        """context manager: hold the handle across several device-pointer calls (gs_index_lock / gs_index_unlock);
        calls on this handle from other threads wait meanwhile"""
        import contextlib

        @contextlib.contextmanager
        def hold():
            _check(lib().gs_index_lock(self._h))
            try:
                yield self
            finally:
                _check(lib().gs_index_unlock(self._h))
        return hold()

    def prepare(self, n, L=20, pam="NGG", alt_pams=(), mismatches=3, start=False):
        """the first batch's one-off work (seed recipes, PAM-pair and deep tables, workspace for n guides) ahead of the first job
        (gs_index_prepare)"""
        alts = "".join(alt_pams).encode()
        _check(lib().gs_index_prepare(self._h, int(n), L, pam.encode(), len(pam), alts if alt_pams else None, len(alt_pams), mismatches,
                                      GS_FLAG_PAM_AT_START if start else 0))

    def set_option(self, key, value):
        """a switch of this handle (gs_index_set_option): value None removes it.  The environment's GS_* variables are
        read once, when the handle is made; afterwards this is the only way to change one."""
        _check(lib().gs_index_set_option(self._h, key.encode(), None if value is None else str(value).encode()))

    def set_options(self, **kv):
        for k, v in kv.items():
            self.set_option(k, v)

    def get_option(self, key):
        buf = C.create_string_buffer(256)
        rc = lib().gs_index_get_option(self._h, key.encode(), buf, 256)
        return buf.value.decode() if rc == 0 else None

    def last_sharing(self):
        """heavy items shared among waves in the last search launch (gs_index_last_sharing); form: 0 one launch, every item
        with its wave; 1 one launch that publishes heavy passes and helps; 2 two launches (publishing + helpers); 3 the two
        seeding launches of gs_seed.hip (no sharing); guides_with_heavy_kmer: what the form was chosen from"""
        out = (C.c_uint64 * 8)()
        _check(lib().gs_index_last_sharing(self._h, out))
        return dict(shared_items=int(out[0]), packages=int(out[1]), queue_packages=int(out[2]), tickets=int(out[3]),
                    guides_ordered_device_wide_alone=int(out[4]), launches_behind=int(out[5]), form=int(out[6]),
                    guides_with_heavy_kmer=int(out[7]))

    def last_counters(self):
        """k_search's counters of the last enumerate_device call (see gs_index_last_counters)"""
        out = (C.c_uint64 * 16)()
        _check(lib().gs_index_last_counters(self._h, out))
        v = list(out)
        sp = (C.c_uint64 * 6)()
        L_ = lib()
        L_.gs_index_last_spaced.restype = C.c_int
        L_.gs_index_last_spaced.argtypes = [C.c_void_p, C.c_void_p]
        _check(L_.gs_index_last_spaced(self._h, sp))
        return dict(spaced_items=int(sp[0]), spaced_rows=int(sp[1]), spaced_rows_max=int(sp[2]), spaced_matches=int(sp[3]),
                    spaced_bytes=int(sp[4]), spaced_build_us=int(sp[5]),
                    n_ext=v[0], overflow_items=v[1], n_matches=v[2], items_two_sided=v[4], items_one_sided=v[5],
                    guides_redone=v[6], ordered_device_wide=bool(v[7] & 1), redo_ordered_device_wide=bool(v[7] & 2),
                    overflow_from_arena=bool(v[7] & 4),
                    ordered_by_one_composite_sort=bool(v[7] & 8), runs_turned_round=bool(v[7] & 16),
                    ordered_in_tiles=bool(v[7] & 32), tile_ordering_gave_up=bool(v[7] & 64),
                    items_pair_tables=v[7] >> 8, recipe_lines=v[3],
                    slots_per_item=v[13], matches_sum=v[14], matches_max_per_item=v[15],
                    table_lines=v[8], ctx16_lines=v[9], ctx_words=v[10], sa_isa_gathers=v[11], occ_lines=v[12])

    def resident(self):
        """the arrays the handle keeps on the device and the bytes they count for (gs_debug_resident)"""
        L_ = lib()
        L_.gs_debug_resident.restype = C.c_int
        L_.gs_debug_resident.argtypes = [C.c_void_p, C.c_void_p]
        out = (C.c_uint64 * 4)()
        _check(L_.gs_debug_resident(self._h, out))
        return dict(zip(("strand_arrays", "strand_bytes", "pairtab_arrays", "pairtab_bytes"), (int(x) for x in out)))

    STRAND_LAYOUT = ("n", "blocks", "k", "mask_off", "n_exc", "nruns", "C0", "C1", "C2", "C3", "CN", "has_n", "rot_first",
                     "rot_copies", "xr_entries")
    SLOT_LAYOUT = ("valid", "v_rem", "code", "rot_first", "rot_copies", "n_slots", "deep", "deep_P", "deep_kb", "spaced", "sp_x",
                   "sp_g", "sp_rem", "sp_rows", "d", "k")
    # element types of the arrays gs_debug_index_array names (uint4 / uint2 entries come back as rows of words)
    STRAND_ARRAYS = dict(blocks=("<u4", 16), sa=("<u4", 1), ptab=("<u4", 4), ptab_rot=("<u4", 4), ctx=("<u4", 1), ctx16=("<u2", 1),
                         isa=("<u4", 1), exc_row=("<u4", 1), exc_sym=("<u8", 1), run_start=("<u4", 1), run_cum=("<u4", 1),
                         xr_seg=("<u4", 2), xr_start=("<u4", 1), xr_cum=("<u4", 1), C256=("<u4", 1))
    SLOT_ARRAYS = dict(tab=("<u4", 2), rot=("<u4", 2), c16=("<u2", 1), ctx=("<u4", 1), rowid=("<u4", 1), deep=("<u4", 4),
                       sp_off=("<u4", 1), sp_rows=("<u4", 2))

    def debug_layout(self, strand, slot=-1):
        """the scalars that size and explain the index's device arrays (gs_debug_index_layout): a strand's, or a PAM-pair
        table slot's as `strand` holds it.  Tests only."""
        L_ = lib()
        L_.gs_debug_index_layout.restype = C.c_int
        L_.gs_debug_index_layout.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        out = (C.c_uint64 * 32)()
        _check(L_.gs_debug_index_layout(self._h, slot, strand, out))
        return dict(zip(self.STRAND_LAYOUT if slot < 0 else self.SLOT_LAYOUT, (int(x) for x in out)))

    def debug_array(self, strand, which, slot=-1):
        """one named device array of a strand or a slot as a numpy array, or None when the handle does not hold it
        (gs_debug_index_array).  Tests only."""
        L_ = lib()
        L_.gs_debug_index_array.restype = C.c_int
        L_.gs_debug_index_array.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
        dtype, width = (self.STRAND_ARRAYS if slot < 0 else self.SLOT_ARRAYS)[which]
        total = C.c_uint64()
        _check(L_.gs_debug_index_array(self._h, slot, strand, which.encode(), 0, None, 0, C.byref(total)))
        if not total.value:
            return None
        out = np.empty(int(total.value), dtype=np.uint8)
        _check(L_.gs_debug_index_array(self._h, slot, strand, which.encode(), 0, out.ctypes.data, out.nbytes, C.byref(total)))
        a = out.view(dtype)
        return a.reshape(-1, width) if width > 1 else a

    def workspace(self):
        """per group of the handle's workspace (WORKSPACE_GROUPS): buffers held, bytes held, bytes an out-of-memory
        recovery would release (gs_debug_workspace)"""
        L_ = lib()
        L_.gs_debug_workspace.restype = C.c_int
        L_.gs_debug_workspace.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        out = (C.c_uint64 * (3 * len(WORKSPACE_GROUPS)))()
        _check(L_.gs_debug_workspace(self._h, out, len(WORKSPACE_GROUPS)))
        return {g: dict(buffers=int(out[3 * i]), bytes=int(out[3 * i + 1]), releasable=int(out[3 * i + 2]))
                for i, g in enumerate(WORKSPACE_GROUPS)}

    def spaced_rows(self, slot, strand, key, cap=4096):
        """the rows under `key` in a slot's spaced table (gs_debug_spaced_rows) -> (rows uint32[n, 4], n under the key, info)"""
        L_ = lib()
        L_.gs_debug_spaced_rows.restype = C.c_int
        L_.gs_debug_spaced_rows.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        out = np.zeros((cap, 4), dtype=np.uint32)
        n = C.c_uint64()
        info = (C.c_uint32 * 8)()
        _check(L_.gs_debug_spaced_rows(self._h, slot, strand, int(key), out.ctypes.data, cap, C.byref(n), info))
        names = ("built", "code", "v_rem", "x_len", "r_len", "k", "key_bits_in_row", "rows")
        return out[:min(cap, int(n.value))], int(n.value), dict(zip(names, (int(x) for x in info)))

    def last_launch(self):
        """what the main pass of the last enumerate_device call was launched with (gs_index_last_launch)"""
        out = (C.c_uint64 * 8)()
        _check(lib().gs_index_last_launch(self._h, out))
        v = [int(x) for x in out]
        return dict(walk=bool(v[0]), spec=bool(v[1]), deep=bool(v[2]), take=v[3], seed_take=v[4], pair_tables=v[5],
                    x_len=v[6], rot_copies=v[7])

    def enumerate_device(self, d_guides_ptr, n, L, d_pams_ptr, P, mismatches=3, alt_pams=(),
                         start=False, stream=None, faithful=False, count_requests=False):
        """Device-resident variant (what bench.py times): pointers are raw device addresses.
        Returns (d_offsets_ptr, d_hits_ptr, stats)."""
        alt = b"".join(p.encode() for p in alt_pams)
        flags = ((GS_FLAG_PAM_AT_START if start else 0) | (GS_FLAG_FAITHFUL_WALK if faithful else 0) |
                 (GS_FLAG_COUNT_REQUESTS if count_requests else 0))
        d_off, d_hits = C.c_void_p(), C.c_void_p()
        v = GsResultView()
        _check(lib().gs_enumerate_device(self._h, d_guides_ptr, n, L, d_pams_ptr, P,
                                         alt if alt_pams else None, len(alt_pams), mismatches, flags,
                                         stream, C.byref(d_off), C.byref(d_hits), C.byref(v)))
        stats = dict(n_ext=int(v.n_ext), n_matches=int(v.n_matches), n_hits=int(v.n_hits),
                     ms_search=float(v.ms_search), ms_total=float(v.ms_total))
        return d_off.value, d_hits.value, stats
