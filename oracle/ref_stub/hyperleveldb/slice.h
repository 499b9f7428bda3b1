// TEST SCAFFOLDING ONLY (oracle/Makefile, target _ref/libref_store.so).
// Stand-in for <hyperleveldb/slice.h>: a pointer and a size.
#ifndef hyperleveldb_slice_h_
#define hyperleveldb_slice_h_
#include <stddef.h>
namespace leveldb {
class Slice {
  public:
    Slice() : m_data(""), m_sz(0) {}
    Slice(const char* d, size_t n) : m_data(d), m_sz(n) {}
    const char* data() const { return m_data; }
    size_t size() const { return m_sz; }

  private:
    const char* m_data;
    size_t m_sz;
};
}  // namespace leveldb
#endif
