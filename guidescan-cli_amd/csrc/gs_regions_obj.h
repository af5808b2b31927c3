/* gs_regions_obj.h -- a parsed BED file (gs_design.hip: gs_regions_parse), as the units that read it see it */
#ifndef GS_REGIONS_OBJ_H
#define GS_REGIONS_OBJ_H

#include "gs_common.h"

struct gs_rg_chr { /* one chromosome's table, as uploaded */
  std::vector<uint32_t> start, end, maxend, group;
};
struct gs_regions {
  std::vector<std::string> chr_names, group_names;
  std::vector<uint64_t> chr_lengths;
  std::vector<const char *> chr_name_ptrs;
  std::vector<gs_rg_chr> chr;
  uint64_t n_intervals = 0;
  gs_genome_structure structure() const {
    return gs_genome_structure{chr_name_ptrs.data(), chr_lengths.data(), (uint32_t)chr_names.size()};
  }
};

#endif
