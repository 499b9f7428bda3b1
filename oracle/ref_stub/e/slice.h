// TEST SCAFFOLDING ONLY (oracle/Makefile, target _ref/libref_hash.so).
// Stand-in for libe's <e/slice.h>: the part of e::slice that the reference's
// common/hash.cc and common/datatype_{string,int64,float,timestamp}.cc use.
// Same idea as tests/cpp/shim_e/e/slice.h, plus the (pointer, size)
// constructor over char buffers.  No hashing logic lives here.
#ifndef e_slice_h_
#define e_slice_h_
#include <assert.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>
namespace e {
class slice {
  public:
    slice() : m_data(NULL), m_sz(0) {}
    slice(const void* d, size_t sz) : m_data(static_cast<const uint8_t*>(d)), m_sz(sz) {}
    slice(const char* s) : m_data(reinterpret_cast<const uint8_t*>(s)), m_sz(strlen(s)) {}
    const uint8_t* data() const { return m_data; }
    size_t size() const { return m_sz; }
    bool empty() const { return m_sz == 0; }

  private:
    const uint8_t* m_data;
    size_t m_sz;
};
}  // namespace e
#endif
