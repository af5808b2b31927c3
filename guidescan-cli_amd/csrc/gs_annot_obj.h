/* gs_annot_obj.h -- an annotation (gs_annot.hip: gs_annot_build) as the units that read it see it: the segment table of
 * gs_annot_scan.h and the group names, on the host and - device >= 0 - in one allocation in HBM */
#ifndef GS_ANNOT_OBJ_H
#define GS_ANNOT_OBJ_H

#include "gs_common.h"
#include "gs_annot_scan.h"

struct gs_annot {
  int device = -1; /* -1: host only */
  gs_an_host h;
  std::vector<std::string> group_names;
  std::vector<uint64_t> chr_lengths;
  std::string names;              /* the group names back to back */
  std::vector<uint32_t> name_off; /* n_groups + 1 */
  void *d_blob = nullptr;         /* chr_bp | bp | seg_off | ent | name_off | names */
  gs_an_table d_table{};
  const uint32_t *d_name_off = nullptr;
  const uint8_t *d_names = nullptr;
};

/* The record a hit list belongs to, for the selection rule of gs_design_set_feature_rule: hits of guide g within
 * `distance` that have a feature are counted in hits[g], the record's own site - the distance-0 hit that resolves to
 * chr[g], pos[g], sense[g] - left out.  Device arrays of n entries. */
struct gs_annot_own {
  const uint32_t *chr, *pos;
  const uint8_t *sense;
  uint32_t *hits;
  uint32_t distance;
};
/* gs_annotate_device with that count made in the count pass (own may be nullptr) */
gs_status gs_annotate_device_own(gs_index *ix, const gs_annot *an, const gs_genome_structure *gs, uint64_t n, uint32_t L, uint32_t P,
                                 uint32_t mismatches, const void *d_offsets, const void *d_hits, void *stream, const gs_annot_own *own,
                                 const void **d_feat_offsets, const void **d_feats, const void **d_guide_counts);

#endif
