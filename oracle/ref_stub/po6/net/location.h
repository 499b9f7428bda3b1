// TEST SCAFFOLDING ONLY (oracle/Makefile, target _ref/libref_store.so).
// Stand-in for libpo6's <po6/net/location.h>: the reference's daemon headers name the
// type in declarations; nothing the store library runs touches it.
#ifndef po6_net_location_h_
#define po6_net_location_h_
namespace po6 {
namespace net {
class location {};
}  // namespace net
}  // namespace po6
#endif
