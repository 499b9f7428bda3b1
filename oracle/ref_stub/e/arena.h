// TEST SCAFFOLDING ONLY (oracle/Makefile, target _ref/libref_hash.so).
// Stand-in for libe's <e/arena.h>: allocations that live as long as the
// arena.  Only the datatypes' apply() methods allocate; the hash path never does.
#ifndef e_arena_h_
#define e_arena_h_
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <vector>

namespace e {
class arena {
  public:
    arena() : m_blocks() {}
    ~arena() {
        for (size_t i = 0; i < m_blocks.size(); ++i) free(m_blocks[i]);
    }
    void allocate(size_t sz, uint8_t** ptr) {
        *ptr = static_cast<uint8_t*>(malloc(sz ? sz : 1));
        if (!*ptr) abort();
        m_blocks.push_back(*ptr);
    }

  private:
    arena(const arena&);
    arena& operator=(const arena&);
    std::vector<void*> m_blocks;
};
}  // namespace e
#endif
