/* fasta_names.hpp -- a FASTA record's name from its title line, one function per rule set: the host readers (`index`'s
 * parse_fasta, `decode`'s read_fasta) and the device reader (gs_fasta.hip) all call these, so the paths cannot drift.
 * line[0, n): the title line from its '>' on, without its newline. */
#ifndef GS_FASTA_NAMES_HPP
#define GS_FASTA_NAMES_HPP

#include <cctype>
#include <cstddef>
#include <cstring>

namespace fasta_names {

/* GS_FASTA_INDEX_RULES: line.substr(1) up to the first ' ' (seq_io.cxx:83-98 splits at ' ' too).  Where this departs from
 * the reference: a CRLF title without a space keeps its '\r'; "> chr1" gives an empty name. */
inline void index_name(const char *line, size_t n, size_t *begin, size_t *len) {
  const char *sp = n > 1 ? (const char *)memchr(line + 1, ' ', n - 1) : nullptr;
  *begin = n ? 1 : 0;
  *len = sp ? (size_t)(sp - line) - 1 : (n ? n - 1 : 0);
}

/* GS_FASTA_RECORD_RULES: the first run of non-blank bytes behind '>', leading blanks skipped (SeqIO's record.id) */
inline void record_name(const char *line, size_t n, size_t *begin, size_t *len) {
  size_t b = n ? 1 : 0, e;
  while (b < n && isspace((unsigned char)line[b])) b++;
  e = b;
  while (e < n && !isspace((unsigned char)line[e])) e++;
  *begin = b;
  *len = e - b;
}

}  // namespace fasta_names

#endif
