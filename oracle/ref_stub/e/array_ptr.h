// TEST SCAFFOLDING ONLY (oracle/Makefile, target _ref/libref_store.so).
// Stand-in for libe's <e/array_ptr.h>: common/hyperspace.h and common/configuration.h
// hold members of it.  operator[] is declared for an inline accessor that is
// never called, and defined nowhere.
#ifndef e_array_ptr_h_
#define e_array_ptr_h_
#include <stddef.h>
namespace e {
template <typename T>
class array_ptr {
  public:
    T& operator[](size_t) const;
};
}  // namespace e
#endif
