// TEST SCAFFOLDING ONLY (oracle/Makefile, target _ref/libref_hash.so).
// Stand-in for libe's <e/serialization.h>: the reference's headers only
// declare operators over these two types; nothing on the hash path calls them.
#ifndef e_serialization_h_
#define e_serialization_h_
namespace e {
class packer;
class unpacker;
}  // namespace e
#endif
