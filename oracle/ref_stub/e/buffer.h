// TEST SCAFFOLDING ONLY (oracle/Makefile, target _ref/libref_hash.so).
// Stand-in for libe's <e/buffer.h>: common/ids.h includes it and uses nothing
// of it on the hash path.
#ifndef e_buffer_h_
#define e_buffer_h_
namespace e {
class buffer;
}  // namespace e
#endif
