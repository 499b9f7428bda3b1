// TEST SCAFFOLDING ONLY (oracle/Makefile, target _ref/libref_checks.so).
// Stand-in for libe's <e/slice.h>, ahead of ref_stub/ on that target's include
// path only: ref_stub's e::slice plus the equality common/attribute_check.cc
// uses under EQUALS.  Equality is libe's: the same size and the same bytes.
//
// This is the one piece of semantics a stand-in of this target holds.  For
// every comparable type it never decides alone: EQUALS is
// `check.value == value || compare(check.value, value) == 0`, and equal bytes
// imply compare == 0 in all nine datatypes the glue's lookup() knows.  No
// predicate logic, no compare and no validate lives here.
#ifndef e_slice_checks_h_
#define e_slice_checks_h_
#include_next <e/slice.h>
namespace e {
inline bool operator==(const slice& lhs, const slice& rhs) {
    return lhs.size() == rhs.size() && (lhs.size() == 0 || memcmp(lhs.data(), rhs.data(), lhs.size()) == 0);
}
inline bool operator!=(const slice& lhs, const slice& rhs) { return !(lhs == rhs); }
}  // namespace e
#endif
