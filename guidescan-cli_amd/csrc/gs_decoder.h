/* gs_decoder.h -- the decoder object of gs_decode.hip, shared with the units that lend its workspace and its lock
 * (gs_bgzf_inflate.hip: the inflated bytes of a BAM database stay in HBM between its calls) */
#ifndef GS_DECODER_H
#define GS_DECODER_H

#include "gs_common.h"
#include "gs_repr.h"

struct gs_annot;

struct gs_decoder {
  std::recursive_mutex mtx;
  int device = 0;
  uint32_t n_chr = 0;
  uint64_t total = 0;
  std::vector<std::string> names;
  std::vector<uint64_t> lengths;   /* the @SQ LN values: what an attached annotation must have been parsed against */
  const gs_annot *annot = nullptr; /* gs_decoder_set_annotation: the caller's, for GS_TEXT_FEATURES */
  double last_annot_ms = 0;        /* the annotation pass of the last batch, by stream events (gs_debug_decode_annot_ms) */
  gs_buffer text, tabs; /* the FASTA bytes; prefix sums, text offsets, record lengths, name offsets, names, powers of five */
  const uint64_t *d_cum = nullptr, *d_toff = nullptr, *d_flen = nullptr;
  const uint32_t *d_name_off = nullptr;
  const uint8_t *d_names = nullptr;
  gs_pow5_tables pw{nullptr, nullptr};
  gs_buffer w_in, w_tmp, w_text;
  /* gs_bgzf_inflate.hip: the compressed bytes and the member table; reasons; the inflated bytes of the last two calls (the
   * later call takes the tail of the earlier one in front), which of the two is the last, and its length */
  gs_buffer w_bi_in, w_bi_tmp, w_inf[2];
  uint32_t inf_cur = 0;
  uint64_t inf_len = 0;
  uint64_t inf_base_member = 0, inf_base_byte = 0; /* gs_bgzf_inflate_base: what a message adds to a member's index and offset */
  /* gs_bamsplit.hip: record starts (sized by the bytes); the records' sizes and their scans (sized by the records found); the bytes of a cut record the last gs_decode_bam
   * call left at the end of w_inf[inf_cur]; the last call's members, compressed bytes, inflated bytes, records and the
   * milliseconds of its stages (inflate with the upload, record starts, fields, the decoder's kernels) */
  gs_buffer w_bs_tmp, w_bs_rec;
  uint64_t bam_tail = 0;
  uint64_t last_bam[4] = {0, 0, 0, 0};
  double last_bam_ms[4] = {0, 0, 0, 0};
};

/* a batch of gs_decode_batch's arrays in HBM, with the word offsets (hex digits / 16, prefix-summed) */
struct gs_decode_batch_dev {
  const uint8_t *ids, *seqs, *hex, *reverse;
  const uint64_t *id_off, *seq_off, *hex_off, *word_off;
  const int32_t *chr;
  const int64_t *pos0;
};
/* gs_decode.hip */
/* gs_decoder_open with the text in host memory or, text_on_device != 0, in HBM already (gs_fasta.hip: copied device to device) */
gs_status gs_decoder_open_text(int device, const uint8_t *text, uint64_t len, int text_on_device, const gs_genome_structure *sq,
                               const uint64_t *chr_text_off, const uint64_t *chr_text_len, gs_decoder **out);
/* the flags of a decode entry point against the decoder's state: GS_TEXT_FEATURES needs an annotation, GS_DECODE_FEATURES_ONLY
 * needs GS_TEXT_FEATURES | GS_TEXT_COMPLETE; GS_ERR_ARG with the message otherwise */
gs_status gs_decode_check_flags(const gs_decoder *d, uint32_t flags);
gs_status gs_decode_run_device(gs_decoder *d, const gs_decode_batch_dev &db, uint64_t n, uint64_t nw, uint32_t flags, uint64_t first_record,
                               const gs_decode_batch *host_batch, const void **d_text, uint64_t *text_len, uint64_t *n_rows);

#endif
