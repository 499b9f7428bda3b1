// TEST SCAFFOLDING ONLY (oracle/Makefile, target _ref/libref_store.so).
// Stand-in for libpo6's <po6/net/hostname.h>: named in daemon/datalayer.h's declarations only.
#ifndef po6_net_hostname_h_
#define po6_net_hostname_h_
namespace po6 {
namespace net {
class hostname {};
}  // namespace net
}  // namespace po6
#endif
