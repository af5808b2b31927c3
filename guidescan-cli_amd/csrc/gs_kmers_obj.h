/* gs_kmers_obj.h -- the object behind gs_kmers: the candidates of a scan (gs_kmers.hip) or the rows of a kmers file
 * (gs_kmersfile.hip), their arrays in HBM and the host copies made when first asked for. */
#ifndef GS_KMERS_OBJ_H
#define GS_KMERS_OBJ_H

#include "gs_common.h"

#include <string>
#include <vector>

struct gs_kmers {
  int device = 0; /* -1: made on the host (gs_debug_kmers_host), nothing in HBM */
  /* parsed from a kmers file: no positions, the ids are the file's (have_ids from the start), and gs_kmers_encode_ids /
   * gs_kmers_csv are GS_ERR_ARG */
  bool parsed = false;
  /* selected for regions (gs_design.hip): positions as a scan's, but the ids name each record's group and chromosome
   * (have_ids from the start) and gs_kmers_encode_ids is GS_ERR_ARG */
  bool ids_fixed = false;
  uint64_t n = 0;
  uint32_t k = 0, P = 0;
  void *d_seqs = nullptr, *d_pams = nullptr, *d_pos = nullptr, *d_sense = nullptr;
  std::vector<uint8_t> h_seqs, h_pams, h_sense;
  std::vector<uint32_t> h_pos;
  bool have_host = false;
  /* gs_kmers_encode_ids: the ids back to back, n + 1 offsets, the senses as 0 / 1 ("+") */
  void *d_ids = nullptr, *d_id_off = nullptr, *d_sense01 = nullptr;
  uint64_t id_bytes = 0;
  bool have_ids = false, have_host_ids = false;
  std::vector<uint8_t> h_ids, h_sense01;
  std::vector<uint64_t> h_id_off;
  double filter_ms[3] = {0, 0, 0}; /* made by gs_kmers_filter: its rule, scan and gather passes between stream events */
  /* made by gs_controls_generate (gs_controls.hip): a parsed object in every respect, plus the kept counters and the id
   * prefix its rows are written with */
  bool controls = false;
  std::vector<uint64_t> h_counters;
  std::string ct_prefix;
};

/* frees the object and its arrays in HBM (gs_kmers_free; the deleter of an object under construction) */
void km_release(gs_kmers *km);

/* The id and kmers-file row writer of gs_kmers.hip (the row itself: gs_guide_row, gs_rowtext.h).  The name table: the prefix,
 * then the group names, then the chromosome names back to back; goff / coff say where each name begins, one more entry closes
 * each.  goff empty: the ids name no group. */
struct gs_km_names {
  std::string names;
  std::vector<uint32_t> goff, coff;
  uint32_t prefix_len = 0;
};
/* The ids "{prefix}[{group}:]{chromosome}:{position}:{sense}" of km's records (rows == false: they become the object's
 * d_ids, d_id_off and d_sense01) or their kmers-file rows in HBM (*d_text, the caller's to free).  d_group / d_chr: uint32[n]
 * in HBM, the group and chromosome of every record, or nullptr: no group (goff empty), chromosome 0.  what: names the scan
 * in an error message.  The caller has set the device. */
gs_status gs_km_encode_text(gs_kmers *km, const gs_km_names &nt, const uint32_t *d_group, const uint32_t *d_chr, bool rows, const char *what,
                            hipStream_t st, void **d_text, uint64_t *bytes);

#endif
