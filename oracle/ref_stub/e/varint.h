// TEST SCAFFOLDING ONLY (oracle/Makefile, target _ref/libref_store.so).
// Stand-in for libe's <e/varint.h>: declarations only.  oracle/ref_store_glue.cc
// defines them as abort(): only the key-prefix functions of
// daemon/datalayer_encodings.cc call them, and no test reaches those.
#ifndef e_varint_h_
#define e_varint_h_
#include <stddef.h>
#include <stdint.h>
namespace e {
size_t varint_length(uint64_t v);
char* packvarint64(uint64_t v, char* p);
const char* varint64_decode(const char* p, const char* end, uint64_t* v);
}  // namespace e
#endif
