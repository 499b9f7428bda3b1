// TEST SCAFFOLDING ONLY (oracle/Makefile, target _ref/libref_store.so).
// Stand-in for libe's <e/compat.h>: e::compat::shared_ptr is std::shared_ptr.
#ifndef e_compat_h_
#define e_compat_h_
#include <memory>
namespace e {
namespace compat {
using std::shared_ptr;
}  // namespace compat
}  // namespace e
#endif
