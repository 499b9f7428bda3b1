// TEST SCAFFOLDING ONLY (oracle/Makefile, target _ref/libref_store.so).
// Stand-in for libpo6's <po6/path.h>: daemon/datalayer.h includes it and uses nothing of it.
#ifndef po6_path_h_
#define po6_path_h_
namespace po6 {
class path {};
}  // namespace po6
#endif
