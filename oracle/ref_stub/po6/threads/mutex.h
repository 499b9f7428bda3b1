// TEST SCAFFOLDING ONLY (oracle/Makefile, target _ref/libref_store.so).
// Stand-in for libpo6's <po6/threads/mutex.h>: daemon/datalayer.h includes it and uses nothing of it.
#ifndef po6_threads_mutex_h_
#define po6_threads_mutex_h_
namespace po6 {
namespace threads {
class mutex {};
}  // namespace threads
}  // namespace po6
#endif
