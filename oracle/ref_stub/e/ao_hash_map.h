// TEST SCAFFOLDING ONLY (oracle/Makefile, target _ref/libref_store.so).
// Stand-in for libe's <e/ao_hash_map.h>: daemon/datalayer.h holds one as a member; an
// empty template of the same parameters.
#ifndef e_ao_hash_map_h_
#define e_ao_hash_map_h_
#include <stdint.h>
namespace e {
template <typename K, typename V, uint64_t (*H)(K), const K& EMPTY>
class ao_hash_map {};
}  // namespace e
#endif
