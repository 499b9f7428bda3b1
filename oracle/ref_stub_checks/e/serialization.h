// TEST SCAFFOLDING ONLY (oracle/Makefile, target _ref/libref_checks.so).
// Stand-in for libe's <e/serialization.h>, ahead of ref_stub/ on that target's
// include path only: common/attribute_check.cc defines operator << / >> over
// e::packer / e::unpacker by value, so the two types are complete here.  Every
// operator and every pack_size aborts: nothing a test calls packs or unpacks.
// No predicate, compare or validate logic lives here.
#ifndef e_serialization_h_
#define e_serialization_h_
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
namespace e {
class slice;
class packer {
  public:
    packer operator<<(uint8_t) { abort(); }
    packer operator<<(uint16_t) { abort(); }
    packer operator<<(uint32_t) { abort(); }
    packer operator<<(uint64_t) { abort(); }
    packer operator<<(const slice&) { abort(); }
};
class unpacker {
  public:
    unpacker operator>>(uint8_t&) { abort(); }
    unpacker operator>>(uint16_t&) { abort(); }
    unpacker operator>>(uint32_t&) { abort(); }
    unpacker operator>>(uint64_t&) { abort(); }
    unpacker operator>>(slice&) { abort(); }
};
inline size_t pack_size(const slice&) { abort(); }
}  // namespace e
// common/serialization.h names ::pack_size and e::pack_size in using-declarations
inline size_t pack_size(const e::packer&) { abort(); }
#endif
