/* gs_kmers_obj.h -- the object behind gs_kmers: the candidates of a scan (gs_kmers.hip) or the rows of a kmers file
 * (gs_kmersfile.hip), their arrays in HBM and the host copies made when first asked for. */
#ifndef GS_KMERS_OBJ_H
#define GS_KMERS_OBJ_H

#include <stdint.h>

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
};

#endif
