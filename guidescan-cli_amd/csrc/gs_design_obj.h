/* gs_design_obj.h -- the object behind gs_design (gs_design.hip): the (candidate, group) records of a set of regions, as
 * the units that read them see it (gs_pairs.hip), and the ordering, gather and id passes of gs_design.hip that they share. */
#ifndef GS_DESIGN_OBJ_H
#define GS_DESIGN_OBJ_H

#include "gs_common.h"
#include "gs_kmers_obj.h"
#include "gs_regions_obj.h"
#include "gs_annot_obj.h"

struct gs_design {
  int device = 0; /* -1: made on the host (gs_debug_design_host), nothing in HBM */
  const gs_regions *rg = nullptr;
  uint64_t n = 0;
  uint32_t k = 0, P = 0;
  bool scored = false;
  /* per record, in HBM: the layout gs_enumerate_device takes, then where the record comes from and what it scored */
  void *d_seqs = nullptr, *d_pams = nullptr, *d_pos = nullptr, *d_sense = nullptr, *d_group = nullptr, *d_chr = nullptr,
       *d_spec = nullptr, *d_elig = nullptr;
  std::vector<uint8_t> h_seqs, h_pams, h_sense, h_elig;
  std::vector<uint32_t> h_pos, h_group, h_chr;
  std::vector<float> h_spec;
  bool have_host = false;
  uint64_t last[4] = {0, 0, 0, 0}; /* of the last select: records, kept, groups left empty, groups short of N */
  /* gs_design_set_feature_rule: the score phase counts, per record, the off-target hits within rule_distance that have a
   * feature of rule_annot (d_fhits, uint32[n]); more than rule_max of them and the record is not eligible */
  const gs_annot *rule_annot = nullptr;
  uint32_t rule_distance = 0, rule_max = 0;
  void *d_fhits = nullptr;
  bool have_fhits = false;
  std::vector<uint32_t> h_fhits;
  /* gs_design_set_spacing: the picks of a group lie space_d bases apart or more (0: no rule), by the cut that leaves
   * space_c protospacer bases between it and the PAM; of the last select under the rule: marked records passed over, and
   * groups short of N that hold N marked records */
  uint32_t space_d = 0, space_c = 3;
  bool space_start = false;
  uint64_t last_spacing[2] = {0, 0};
  double space_ms = 0; /* k_ds_space of that select, between stream events */
};

/* The ordering, gather and id passes of gs_design_select over the eligibility bytes d_elig (uint8[n] in HBM, the
 * design's own or another unit's): the kept records in order as a gs_kmers with ids (rows == false), or their kmers-file
 * rows in HBM (*d_text, the caller's to free).  d_place (or NULL): uint32[n], the place in the result of every kept record,
 * untouched for the others.  tally: the design's last[] is updated. */
struct gs_ds_select_rule {
  const uint8_t *d_elig;
  uint32_t per_region;
  bool filter;
  float min_spec;
  uint32_t *d_place;
  bool tally;
  /* min_spacing > 0: k_ds_space takes the place of k_ds_cut (1 <= per_region <= 1024), the cut by cut_offset and
   * pam_at_start; with tally the design's last_spacing[] is updated too */
  uint32_t min_spacing = 0, cut_offset = 0;
  bool pam_at_start = false;
};
gs_status gs_ds_select(gs_design *d, const char *prefix, const gs_ds_select_rule &rule, hipStream_t st, bool rows, gs_kmers **out,
                       void **d_text, uint64_t *text_bytes);
/* an array of an object: nothing frees it but the object's release */
gs_status gs_ds_array(size_t bytes, void **out);

#endif
